"""Back-projection and the stitched cloud of include/colvo.h in float64, and how far a float32 evaluation may lie from them.

Nothing here touches a GPU: tests/test_reconstruct_cpu.py holds this file to oracle/colvo_spec.py and to float32 emulations of the
kernel's arithmetic; tests/test_reconstruct_gpu.py holds csrc/reconstruct.hip's k_backproject, k_stitch_count and k_stitch_write, and
the scan between them (csrc/scan.hip k_scan_top), to it.

world_points   the operation: float64 arithmetic on the float32 inputs, taken exactly.  Pixel (u, v) of frame b with depth d:
                   px = (u - cx) / fx * d,  py = (v - cy) / fy * d,  X_a = r_a0 px + r_a1 py + r_a2 d + t_a      (a = x, y, z)
               with fx = K[b,0,0], fy = K[b,1,1], cx = K[b,0,2], cy = K[b,1,2], r = M[b,:3,:3], t = M[b,:3,3].
world_bound    per-element bound on |float32 evaluation - world_points|.  Derived below, never fitted to what a kernel returned.
stitch         the kept samples of the stitched cloud in their order, with their reference points and bounds.
block_counts   the kept count of every 256-sample block: what k_stitch_count writes and the scan turns into offsets.
emulate_f32    world_point() of csrc/reconstruct.hip in NumPy float32, in several operation orders (the bound's self-check).
scene          the test inputs.

The bound.  u = 2^-24 is float32's unit round-off: every correctly rounded operation multiplies its exact result by (1 + e),
|e| <= u; k of them in a row by at most 1 + gamma_k, gamma_k = k u / (1 - k u).  world_point() of csrc/reconstruct.hip spends
  * on px (and py): one rounding for the subtraction u - cx (u itself is an integer below 2^24: exact), one for the division by fx,
    one for the product by d: 3;
  * per coordinate three products and three additions.  The term r0 px carries px's 3 roundings, its own product's and at most three
    additions': 7.  So does r1 py.  r2 d carries its product's and at most three additions': 4; t at most three additions': 3.  "At
    most three" holds for every way of bracketing a sum of four terms, so the bound does not depend on the association.
Hence |X^ - X| <= gamma_7 (|r0 px| + |r1 py|) + gamma_4 |r2 d| + gamma_3 |t| <= gamma_7 (|r0 px| + |r1 py| + |r2 d| + |t|); the last
form is the bound (one constant, as include/colvo.h states it).  A fused multiply-add forms a product and a sum with ONE rounding
where the plain form has two: contraction only removes roundings, so the uncontracted count is the bound for both, and the file
needs no contraction pragma for it to hold.
  Division: the count above takes fp32 division as correctly rounded.  coivo_amd/build.py passes no flag that says otherwise
(no -ffast-math, no -fno-hip-fp32-correctly-rounded-divide-sqrt, no -cl-* option), and clang's default for HIP is
-fhip-fp32-correctly-rounded-divide-sqrt: the division is the v_div_scale / v_div_fmas / v_div_fixup sequence, correctly rounded.
tests/test_reconstruct_cpu.py pins that absence of flags; were one of them added, the division's allowance would have to become the
documented 2.5 ulp (DIV_ULP below: 1 rounding = half an ulp; 2.5 ulp = 5 roundings, gamma_11 in all).
  Underflow: gfx950 keeps float32 subnormals (clang's default for HIP on it; no flush-to-zero flag in build.py), so a product or
quotient that lands below 2^-126 is off by at most 2^-150 absolutely instead of relatively (sums never underflow inexactly).  Those
of px reach X through |r0| (the quotient's also through |d|), the three products of a coordinate directly: the absolute term
2^-149 ((|r0| + |r1|) (1 + |d|) + 3), which is twice what the count gives and vanishes beside the first term unless d is subnormal.
  The reference's own float64 rounding (16 operations at 2^-53) is added as 16 * 2^-53 of the same sum: 3e-9 of the bound.

max_depth.  The C entry receives a `float`, so the contract is the float32 comparison  d < float32(max_depth).  The oracle's
`depths < max_depth` is that same comparison when it is given float32 depths (torch rounds the Python scalar to the tensor's dtype),
and is NOT when it is given float64 depths, as the parity tests give it: there the double max_depth is compared, and for a
max_depth that float32 cannot represent and that rounds DOWN (3.3 -> 3.2999999523) the one depth d = float32(max_depth) is kept by
the float64 oracle and dropped by the contract; for one that rounds UP the two agree everywhere.  For a representable max_depth (the
default 10.0) they agree.  tests/test_reconstruct_cpu.py shows all three statements on the CPU.
"""
import numpy as np

U = 2.0 ** -24              # unit round-off of float32
NT = 256                    # samples per block of k_stitch_count / k_stitch_write, pixels per block of k_backproject
DIV_ULP = 0.5               # the division's error in ulp: 0.5 = correctly rounded (see above)
K_ROUNDINGS = 6.0 + 2.0 * DIV_ULP    # 7: roundings on the longest path, r0 px


def gamma(k: float) -> float:
    """k roundings in a row: (1 + U)^k - 1 <= k U / (1 - k U)."""
    return k * U / (1.0 - k * U)


def f32(x) -> float:
    """x rounded to float32, as a Python float: what a `float` argument of the C ABI receives."""
    return float(np.float32(x))


def pred32(x) -> np.float32:
    """The float32 just below float32(x)."""
    return np.nextafter(np.float32(x), np.float32(-np.inf))


def _np32(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    return a


def _depth3(depth):
    d = _np32(depth)
    if d.ndim == 4:
        assert d.shape[1] == 1
        d = d[:, 0]
    assert d.ndim == 3
    return d


def _terms(d, us, vs, K, M):
    """d [B,h,w] float32 at columns us [w], rows vs [h] -> float64 terms [B,h,w,3,4]: r_a0 px, r_a1 py, r_a2 d, t_a."""
    K, M = _np32(K).astype(np.float64), _np32(M).astype(np.float64)
    B = d.shape[0]
    assert K.shape == (B, 3, 3) and M.shape == (B, 4, 4)
    d = d.astype(np.float64)
    fx, fy = K[:, 0, 0].reshape(B, 1, 1), K[:, 1, 1].reshape(B, 1, 1)
    cx, cy = K[:, 0, 2].reshape(B, 1, 1), K[:, 1, 2].reshape(B, 1, 1)
    u = np.asarray(us, dtype=np.float64).reshape(1, 1, -1)
    v = np.asarray(vs, dtype=np.float64).reshape(1, -1, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.stack([(u - cx) / fx * d, (v - cy) / fy * d, d], axis=-1)           # [B,h,w,3]
        R = M[:, :3, :3].reshape(B, 1, 1, 3, 3)
        T = np.empty(d.shape + (3, 4))
        T[..., :3] = R * p[..., None, :]
        T[..., 3] = M[:, :3, 3].reshape(B, 1, 1, 3)
    return T, R, d


def _ref_and_bound(d, us, vs, K, M):
    T, R, dd = _terms(d, us, vs, K, M)
    with np.errstate(invalid="ignore", over="ignore"):
        ref = ((T[..., 0] + T[..., 1]) + T[..., 2]) + T[..., 3]
        mag = np.abs(T).sum(axis=-1)
        tiny = 2.0 ** -149 * ((np.abs(R[..., 0]) + np.abs(R[..., 1])) * (1.0 + np.abs(dd)[..., None]) + 3.0)
        bound = (gamma(K_ROUNDINGS) + 16.0 * 2.0 ** -53) * mag + tiny
    return ref, bound


def world_points(depth, K, M):
    """depth [B,1,H,W] (or [B,H,W]), K [B,3,3], M [B,4,4], float32 -> [B,H*W,3] float64, row-major pixel order."""
    d = _depth3(depth)
    B, H, W = d.shape
    return _ref_and_bound(d, np.arange(W), np.arange(H), K, M)[0].reshape(B, H * W, 3)


def world_bound(depth, K, M):
    """-> [B,H*W,3] float64: the bound on |float32 evaluation - world_points| (module docstring).  inf / NaN where the point is."""
    d = _depth3(depth)
    B, H, W = d.shape
    return _ref_and_bound(d, np.arange(W), np.arange(H), K, M)[1].reshape(B, H * W, 3)


def keep_mask(depths, stride, max_depth):
    """[N,Hs,Ws] bool over the walked samples (v, u) = (j stride, i stride): depth < float32(max_depth), compared in float32."""
    d = _depth3(depths)[:, ::stride, ::stride]
    with np.errstate(invalid="ignore"):
        return d < np.float32(max_depth)


def stitch(depths, K, M, stride=1, max_depth=10.0):
    """-> (idx [m] int64, points [m,3] float64, bounds [m,3] float64) of the kept samples, frame-major then row-major.  idx is a
    sample's place in the walk: (frame * Hs + j) * Ws + i."""
    d = _depth3(depths)
    N, H, W = d.shape
    ds = d[:, ::stride, ::stride]
    keep = keep_mask(depths, stride, max_depth)
    ref, bound = _ref_and_bound(ds, np.arange(0, W, stride), np.arange(0, H, stride), K, M)
    idx = np.flatnonzero(keep.reshape(-1))
    return idx, ref.reshape(-1, 3)[idx], bound.reshape(-1, 3)[idx]


def block_counts(depths, stride, max_depth):
    """[N * blocks_per_frame] int64: kept samples of every NT-sample block, as k_stitch_count numbers them."""
    keep = keep_mask(depths, stride, max_depth)
    N = keep.shape[0]
    per_frame = keep.shape[1] * keep.shape[2]
    bpf = -(-per_frame // NT)
    padded = np.zeros((N, bpf * NT), dtype=np.int64)
    padded[:, :per_frame] = keep.reshape(N, per_frame)
    return padded.reshape(N * bpf, NT).sum(axis=1)


def n_blocks(N, H, W, stride):
    return N * -(-(-(-H // stride) * -(-W // stride)) // NT)


def exclusive(counts):
    out = np.zeros(len(counts), dtype=np.int64)
    np.cumsum(counts[:-1], out=out[1:])
    return out


# ---- world_point() in float32, several ways ------------------------------------------------------------------------------------ #
def _fma(a, b, c):
    """float32 fma emulated: the product of two float32 is exact in float64; the sum is rounded to float64 and then to float32 (the
    double rounding moves a result by far less than the bound's slack can hide: it matters on ties only)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


FORMS = ("left_to_right", "pairs", "right_to_left", "fma_chain", "fma_contract")


def emulate_f32(depth, K, M, form, us=None, vs=None):
    """world_point() on float32 inputs in NumPy float32 -> [B,h*w,3] float32 (every pixel, or columns us and rows vs).  Forms of X = r0 px + r1 py + r2 d + t:
    left_to_right ((r0 px + r1 py) + r2 d) + t -- the source's order; pairs (r0 px + r1 py) + (r2 d + t); right_to_left
    r0 px + (r1 py + (r2 d + t)); fma_chain fma(r0, px, fma(r1, py, fma(r2, d, t))); fma_contract fma(r2, d, fma(r1, py, r0 px)) + t
    -- the source's order with every product-sum pair contracted."""
    d = _depth3(depth)
    K, M = _np32(K), _np32(M)
    B, H, W = d.shape
    us = np.arange(W) if us is None else np.asarray(us)
    vs = np.arange(H) if vs is None else np.asarray(vs)
    d = d[:, vs][:, :, us]                              # the pixels at columns us, rows vs
    u = np.asarray(us, dtype=np.float32).reshape(1, 1, -1)
    v = np.asarray(vs, dtype=np.float32).reshape(1, -1, 1)
    c = lambda a: a.reshape(B, 1, 1)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        px = (u - c(K[:, 0, 2])) / c(K[:, 0, 0]) * d
        py = (v - c(K[:, 1, 2])) / c(K[:, 1, 1]) * d
        out = np.empty(d.shape + (3,), dtype=np.float32)
        for a in range(3):
            r0, r1, r2, t = c(M[:, a, 0]), c(M[:, a, 1]), c(M[:, a, 2]), c(M[:, a, 3])
            t = np.broadcast_to(t, d.shape)
            if form == "left_to_right":
                x = ((r0 * px + r1 * py) + r2 * d) + t
            elif form == "pairs":
                x = (r0 * px + r1 * py) + (r2 * d + t)
            elif form == "right_to_left":
                x = r0 * px + (r1 * py + (r2 * d + t))
            elif form == "fma_chain":
                x = _fma(r0, px, _fma(r1, py, _fma(r2, d, t)))
            elif form == "fma_contract":
                x = _fma(r2, d, _fma(r1, py, r0 * px)) + t
            else:
                raise ValueError(form)
            assert x.dtype == np.float32
            out[..., a] = x
    return out.reshape(B, -1, 3)


# ---- comparison ---------------------------------------------------------------------------------------------------------------- #
def worst_ratio(got, ref, bound):
    """(worst |got - ref| / bound over the elements whose reference is finite, its flat index; (0.0, -1) if there is none).  An
    element whose `got` is not finite where the reference is counts as inf."""
    got, ref, bound = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (got, ref, bound))
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    fin = np.isfinite(ref)
    if not fin.any():
        return 0.0, -1
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.where(fin, np.abs(got - ref) / bound, 0.0)
    r = np.where(fin & ~np.isfinite(got), np.inf, r)
    i = int(np.argmax(r))
    return float(r[i]), i


def same_class(got, ref):
    """Where the reference is not finite: the value has the same class (NaN, +inf, -inf).  -> bool."""
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
    nf = ~np.isfinite(ref)
    g, r = got[nf], ref[nf]
    return bool(np.all(np.isnan(g) == np.isnan(r)) and np.all((g == np.inf) == (r == np.inf)) and np.all((g == -np.inf) == (r == -np.inf)))


def old_bar(got, want) -> bool:
    """The bar of tests/test_inference_gpu.py: same shape and max|got - want| < 1e-5 max|want|."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    if want.size == 0:
        return True
    return bool(np.abs(got - want).max() < 1e-5 * np.abs(want).max())


def new_bar(got, ref, bound) -> bool:
    """The bar of tests/test_reconstruct_gpu.py: exact count and |got - ref| <= bound on every element."""
    got = np.asarray(got, dtype=np.float64)
    if got.shape != ref.shape:
        return False
    return worst_ratio(got, ref, bound)[0] <= 1.0


# ---- inputs -------------------------------------------------------------------------------------------------------------------- #
def rigid_chain(rng, n, trans=0.05, rot=0.1):
    """n camera-to-world transforms [n,4,4] float32: integrated random relative poses (M_{k+1} = M_k inverse(T_k), R = Rz Ry Rx),
    computed in float64 and rounded."""
    M = np.eye(4)
    out = np.empty((n, 4, 4))
    for k in range(n):
        t = rng.normal(0.0, trans, 3)
        rx, ry, rz = rng.normal(0.0, rot, 3)
        cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
        R = np.array([[cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx],
                      [sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx],
                      [-sy, cy * sx, cy * cx]])
        Tinv = np.eye(4)
        Tinv[:3, :3] = R.T
        Tinv[:3, 3] = -(R.T @ t)
        M = M @ Tinv
        out[k] = M
    return out.astype(np.float32)


def intrinsics(rng, N, H, W):
    """Per-frame K [N,3,3] float32: a zoom per frame, fy 3-5 % above fx, the principal point up to a tenth of the frame off centre,
    different per frame, and at least a quarter pixel away from every integer (so that u - cx is never 0: 0 * inf stays out)."""
    K = np.zeros((N, 3, 3))
    fx = 0.8 * max(W, 4) * rng.uniform(0.8, 1.25, N)
    K[:, 0, 0] = fx
    K[:, 1, 1] = fx * rng.uniform(1.03, 1.05, N)
    for col, n in ((0, W), (1, H)):
        c = (n - 1) / 2.0 + rng.uniform(-0.1, 0.1, N) * n
        K[:, col, 2] = np.floor(c) + rng.uniform(0.25, 0.75, N)
    K[:, 2, 2] = 1.0
    return K.astype(np.float32)


def scene(N, H, W, seed, max_depth=10.0, far=0.1, drop_frames=(), identity_first=False):
    """-> (depth [N,1,H,W], K [N,3,3], M [N,4,4]) float32 NumPy arrays.  Depths in (0.3, 4.3); a fraction `far` of them at or beyond
    float32(max_depth) (the first of those exactly at it); the frames in drop_frames wholly +inf, as filter_depths writes a rejected
    pixel.  identity_first: frame 0's pose is the identity (t = 0: a subnormal depth then gives a subnormal point)."""
    rng = np.random.default_rng(seed)
    depth = (0.3 + 4.0 * rng.random((N, 1, H, W))).astype(np.float32)
    K = intrinsics(rng, N, H, W)
    M = rigid_chain(rng, N)
    if identity_first:
        M[0] = np.eye(4, dtype=np.float32)
    md = np.float32(max_depth)
    is_far = rng.random(depth.shape) < far
    beyond = (md + md * rng.random(int(is_far.sum()))).astype(np.float32)
    if beyond.size:
        beyond[0] = md
    depth[is_far] = beyond
    for f in drop_frames:
        depth[f] = np.inf
    return depth, K, M


def plant(depth, values, seed, each=4):
    """Puts every value of `values` at `each` distinct places of depth (in place), the first and the last element among them.
    -> positions [len(values), each], flat."""
    rng = np.random.default_rng(seed)
    flat = depth.reshape(-1)
    n = len(values) * each
    assert flat.size >= 2 * n
    pos = np.concatenate([[0, flat.size - 1], 1 + rng.choice(flat.size - 2, size=n - 2, replace=False)]).reshape(each, len(values)).T
    for i, val in enumerate(values):
        flat[pos[i]] = np.float32(val)
    return pos


# ---- the cases of tests/test_reconstruct_gpu.py; tests/test_reconstruct_cpu.py holds the reference to its own conditions on each -- #
BACKPROJECT_SHAPES = [(1, 1, 1), (2, 5, 7), (3, 16, 16), (2, 1, 257), (2, 257, 1), (3, 17, 23), (300, 4, 4), (2, 256, 320)]
FINITE_SPECIALS = (0.0, -0.0, -1.5, 1e-40, -1e-40, 2.0 ** -149, 2.0 ** -126)
NONFINITE_SPECIALS = (np.inf, -np.inf, np.nan)
MAX_DEPTH = 10.0
ODD_MAX_DEPTH = 3.3          # float32(3.3) = 3.2999999523 < 3.3: rounds down, where the float64 oracle and the contract differ

# name -> (N, H, W, stride): n = N * ceil(Hs * Ws / 256) blocks around the thresholds of k_scan_top (per = ceil(n / 256))
STITCH_SHAPES = {
    "n255": (255, 16, 16, 1), "n256": (256, 16, 16, 1), "n257": (257, 16, 16, 1),      # last per == 1; first per == 2
    "n600": (300, 17, 23, 1),        # two blocks per frame, the second partial; per = 3, ragged
    "n1000": (1000, 9, 13, 1),       # every block partial; per = 4, 250 threads used
    "n4099": (4099, 4, 6, 2),        # N far above 256; per = 17
    "n120": (40, 64, 96, 3),         # stride leaves ragged rows and columns (control, per == 1)
    "n1280": (64, 256, 320, 4),      # the default stride at a sequence length the pipeline meets
    "n2560": (8, 256, 320, 1),       # stride 1 at the production frame
    "n6": (3, 17, 23, 1),            # the small scene of the special depths
}
# variant -> scene keywords, given the frame count N and a run length that exceeds `per` consecutive blocks
VARIANTS = {
    "plain": lambda N, run: {},
    "ends": lambda N, run: dict(drop_frames=(0, N - 1)),
    "run": lambda N, run: dict(drop_frames=tuple(range(N // 3, N // 3 + run))),
    "all": lambda N, run: dict(far=0.0),
    "none": lambda N, run: dict(far=1.0),
}
# the special depths of the stitch: (value as a function of float32 max_depth, kept?)
STITCH_SPECIALS = ((lambda md: np.inf, False), (lambda md: np.nan, False), (lambda md: -np.inf, True), (lambda md: 0.0, True),
                   (lambda md: -1.5, True), (lambda md: md, False), (lambda md: pred32(md), True))

STITCH_CASES = ([(name, "plain", MAX_DEPTH) for name in STITCH_SHAPES if name != "n6"]
                + [(name, var, MAX_DEPTH) for name in ("n600", "n1000") for var in ("ends", "run", "all", "none")]
                + [(name, "special", md) for name in ("n6", "n600") for md in (MAX_DEPTH, ODD_MAX_DEPTH)])

_cache = {}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def backproject_case(B, H, W, kind="plain"):
    """-> (depth, K, M, ref [B,HW,3], bound, planted positions or None), computed once and read-only."""
    key = ("bp", B, H, W, kind)
    if key not in _cache:
        depth, K, M = scene(B, H, W, seed=1000 + 7 * B + H + 3 * W, identity_first=(kind == "finite"))
        pos = None
        if kind == "finite":
            pos = plant(depth, FINITE_SPECIALS, seed=5)
        elif kind == "nonfinite":
            pos = plant(depth, NONFINITE_SPECIALS, seed=6)
        _cache[key] = _frozen(depth, K, M, world_points(depth, K, M), world_bound(depth, K, M)) + (pos,)
    return _cache[key]


def stitch_case(name, variant="plain", max_depth=MAX_DEPTH):
    """-> dict(depth, K, M, stride, max_depth, idx, ref, bound, counts, cap, planted), computed once and read-only.  max_depth is
    the value a caller passes (a double); the comparison uses float32(max_depth)."""
    key = ("st", name, variant, max_depth)
    if key not in _cache:
        N, H, W, stride = STITCH_SHAPES[name]
        n = n_blocks(N, H, W, stride)
        per = -(-n // NT)
        bpf = n // N
        run = -(-(2 * per) // bpf) + 1                  # frames: at least 2 per blocks, so one thread's whole share is inside
        kw = VARIANTS["plain" if variant == "special" else variant](N, run)
        seed = 2000 + sum(map(ord, name + variant)) + int(max_depth * 10)
        depth, K, M = scene(N, H, W, seed=seed, max_depth=max_depth, **kw)
        planted = None
        if variant == "special":
            md = np.float32(max_depth)
            planted = plant(depth, [f(md) for f, _ in STITCH_SPECIALS], seed=9)
        idx, ref, bound = stitch(depth, K, M, stride, max_depth)
        counts = block_counts(depth, stride, max_depth)
        assert len(counts) == n and counts.sum() == len(idx)
        _frozen(depth, K, M, idx, ref, bound, counts)
        _cache[key] = dict(depth=depth, K=K, M=M, stride=stride, max_depth=max_depth, idx=idx, ref=ref, bound=bound, counts=counts,
                           cap=N * -(-H // stride) * -(-W // stride), planted=planted, n_blocks=n, per=per, run=run)
    return _cache[key]
