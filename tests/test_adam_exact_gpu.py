"""-m gpu: every Adam entry point of csrc/adam.hip (k_adam, k_adam_multi, k_adam_pack<ES>) against float64, one step at a time.

Each case builds float32 state on the host, runs ONE kernel step and compares parameters and both moments with
tests/adam_ref.adam_step_f64 of the same state under the derived per-element bounds of adam_bounds (a few float32 roundings; a
zero bound means bit-equal).  The moments are held to 3 and 5 roundings at every t; the update's coefficient allowance is the one
of the 1 - powf(b, t) form that adam_coef uses (coef_allowance_pow: 8000 U at t = 2, 12 U at t = 1000, 3 U from t = 1e5 on).  With
the fixed 22.5 U allowance of the cancellation-free form -expm1f(t logf(b)) the kernels miss the bound at t = 2, 3, 5 (worst
|error| / bound 1.70, 1.61, 1.22: profiles/adam_exact.md) and meet it with that form, which was measured slower and not kept
(profiles/adam_coef_ab.md).  Cases of several steps feed the kernel's own outputs back as the next reference input, so no
error accumulates into a bar.  The operand copies of the one-pass form are held bit-equal to the cast / transpose of the
kernel's own updated parameters, and everything a launch must not touch (guard bands, untouched gradients, the rest of the
operand buffers) to its bits.  Each case prints its worst |error| / bound per quantity (`ADAM_EXACT ...`, pytest -s)."""
import functools

import numpy as np
import pytest
import torch

from tests import adam_ref as R
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

KW = dict(lr=1e-4, b1=0.9, b2=0.999, eps=1e-8)
T_HOST = (1, 2, 3, 5, 1000, 100000)
# 4096 workgroups x 256 threads x 4 floats is one sweep of k_adam's capped grid: a second grid-stride iteration of 300 float4 AND
# a 3-element scalar tail
BIG = 4096 * 256 * 4 + 4 * 300 + 3
SIZES = (1, 3, 4, 7, 4 * 1024 + 3, BIG)
PAD = 16                      # sentinel floats behind every arena (16-byte alignment of the arena itself is torch's)


@functools.lru_cache(maxsize=None)
def _cached_state(n, seed, gscale):
    p, g, m, v = R.make_state(n, seed)
    k = R.plant_specials(p, g, m, v, gscale)
    p[k + 1::2] = 0                                   # p normal AND p = 0, element by element
    for x in (p, g, m, v):
        x.setflags(write=False)
    return p, g, m, v


def _state(n, seed, gscale=1.0):
    return tuple(x.copy() for x in _cached_state(n, seed, gscale))


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


class _Arena:
    """One (p, g, m, v) quadruple on the device, each followed by PAD sentinel floats."""

    def __init__(self, p, g, m, v):
        self.n = len(p)
        self.host = [np.concatenate([x, np.full(PAD, 7.25, np.float32)]) for x in (p, g, m, v)]
        self.buf = [torch.from_numpy(x).to(dev()) for x in self.host]

    def views(self):
        return [b[:self.n] for b in self.buf]

    def read(self):
        out = [b.cpu().numpy() for b in self.buf]
        for name, x, h in zip("pgmv", out, self.host):
            assert np.array_equal(_bits(x[self.n:]), _bits(h[self.n:])), f"{name}: written past the end of the arena"
        assert np.array_equal(_bits(out[1]), _bits(self.host[1])), "the gradient was written"
        return out[0][:self.n], out[2][:self.n], out[3][:self.n]


def _hold(kernel, case, got, state, t, gscale, eps=KW["eps"]):
    """Assert got = (p, m, v) float32 arrays within the bounds of one reference step from `state`; -> the reference."""
    p, g, m, v = state
    ref = R.adam_step_f64(p, g, m, v, t, KW["lr"], KW["b1"], KW["b2"], eps, gscale)
    # the kernels' bias corrections are 1 - powf(b, t): the coefficient allowance is pow's limit carried through that cancellation
    coef_u = R.coef_allowance_pow(t, KW["b1"], KW["b2"])
    r = R.worst_ratios(dict(p=got[0], m=got[1], v=got[2]), ref, R.adam_bounds(ref, coef_u=coef_u))
    line = ", ".join(f"{k} {r[k][0]:.3f} @{r[k][1]}" for k in "pmv")
    print(f"ADAM_EXACT {kernel} [{case}]: {line}")
    bad = {k: x for k, x in r.items() if not x[0] <= 1.0}
    detail = "; ".join(f"{k}[{i}]: got {got['pmv'.index(k)][i]!r}, float64 {ref[k][i]!r}, from p {p[i]!r} g {g[i]!r} m {m[i]!r} v {v[i]!r}"
                       for k, (_, i) in bad.items())
    assert not bad, f"{kernel} [{case}]: worst |error| / bound: {line} -- {detail}"
    return ref


def _kw(gscale, eps=KW["eps"]):
    return dict(lr=KW["lr"], beta1=KW["b1"], beta2=KW["b2"], eps=eps, grad_scale=gscale)


# ---------------------------------------------------------------- k_adam ------------------------------------------------ #
@pytest.mark.parametrize("t", T_HOST)
def test_k_adam_host_step_number(t):
    from coivo_amd import ops
    for gscale in (1.0, 0.125):
        st = _state(4 * 1024 + 3, 100 + t % 97, gscale)
        a = _Arena(*st)
        ops.adam_step_t(*a.views(), t, **_kw(gscale))
        p1, m1, v1 = a.read()
        _hold("k_adam", f"host t={t} gscale={gscale}", (p1, m1, v1), st, t, gscale)
        for i in (0, 1):                                            # g = m = v = 0: nothing moves, not even the sign of a zero
            assert _bits(p1)[i] == _bits(st[0])[i] and _bits(m1)[i] == 0 and _bits(v1)[i] == 0


@pytest.mark.parametrize("n", SIZES)
def test_k_adam_sizes(n):
    """From one element to the smallest size that takes a second grid-stride iteration and a scalar tail."""
    from coivo_amd import ops
    t, gscale = 2, 0.125
    st = _state(n, 7, gscale)
    a = _Arena(*st)
    ops.adam_step_t(*a.views(), t, **_kw(gscale))
    _hold("k_adam", f"n={n} t={t} gscale={gscale}", a.read(), st, t, gscale)


@pytest.mark.parametrize("count0", [0, 999])
def test_k_adam_device_step_counter(count0):
    """colvo_adam_step: t = counter + 1 is used and the counter ends one higher; three steps, gradients scaled 0.1, 1, 10, each
    held to one reference step from the kernel's own previous outputs."""
    from coivo_amd import ops
    n, gscale = 4 * 1024 + 3, 1.0
    p, g0, m, v = _state(n, 21 + count0, gscale)
    step = torch.tensor([count0], dtype=torch.int32, device=dev())
    for it in range(3):
        g = (g0 * np.float32(10.0 ** (it - 1))).astype(np.float32)
        a = _Arena(p, g, m, v)
        ops.adam_step(*a.views(), step, **_kw(gscale))
        assert int(step.item()) == count0 + it + 1
        got = a.read()
        _hold("k_adam", f"device counter {count0}+{it}", got, (p, g, m, v), count0 + it + 1, gscale)
        p, m, v = (x.copy() for x in got)


@pytest.mark.parametrize("via", ["host", "device"])
def test_k_adam_coefficients_alone(via):
    """eps = 0, m = v = 0, g = 1, p = 0: p' = -step_size (1 - b1) / (sqrt(1 - b2) rs) -- nothing but the two bias corrections."""
    from coivo_amd import ops
    n = 7
    st = (np.zeros(n, np.float32), np.ones(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32))
    for t in T_HOST:
        a = _Arena(*st)
        if via == "host":
            ops.adam_step_t(*a.views(), t, **_kw(1.0, eps=0.0))
        else:
            step = torch.tensor([t - 1], dtype=torch.int32, device=dev())
            ops.adam_step(*a.views(), step, **_kw(1.0, eps=0.0))
            assert int(step.item()) == t
        _hold("k_adam", f"eps=0 {via} t={t}", a.read(), st, t, 1.0, eps=0.0)


# ---------------------------------------------------------------- k_adam_multi ------------------------------------------ #
@pytest.mark.parametrize("count", [1, 2, 4])
def test_k_adam_multi_against_float64(count):
    from coivo_amd import ops
    sizes = (BIG, 64, 3, 4096 * 5 + 4)[:count]
    t, gscale = 3, 0.125
    states = [_state(n, 7 if n == BIG else 40 + i, gscale) for i, n in enumerate(sizes)]
    arenas = [_Arena(*st) for st in states]
    ops.adam_step_multi([tuple(a.views()) for a in arenas], t, **_kw(gscale))
    for n, a, st in zip(sizes, arenas, states):
        _hold("k_adam_multi", f"{count} arenas, n={n} t={t} gscale={gscale}", a.read(), st, t, gscale)


def test_k_adam_multi_three_steps():
    from coivo_amd import ops
    sizes, gscale = (4096 * 5 + 4, 3, 64, 7), 1.0
    cur = [_state(n, 60 + i, gscale) for i, n in enumerate(sizes)]
    g0 = [st[1] for st in cur]
    for it in range(3):
        cur = [(st[0], (g * np.float32(10.0 ** (it - 1))).astype(np.float32), st[2], st[3]) for st, g in zip(cur, g0)]
        arenas = [_Arena(*st) for st in cur]
        ops.adam_step_multi([tuple(a.views()) for a in arenas], it + 1, **_kw(gscale))
        nxt = []
        for n, a, st in zip(sizes, arenas, cur):
            got = a.read()
            _hold("k_adam_multi", f"step {it + 1} of 3, n={n}", got, st, it + 1, gscale)
            nxt.append((got[0].copy(), st[1], got[1].copy(), got[2].copy()))
        cur = nxt


def test_k_adam_multi_three_arenas_equals_three_single_launches():
    """k_adam and k_adam_multi walk an arena with the same function: tail only, body and tail, body only -- bit for bit."""
    from coivo_amd import ops
    sizes, t, gscale = (3, 1029, 4), 3, 0.125
    states = [_state(n, 80 + i, gscale) for i, n in enumerate(sizes)]
    multi, single = [_Arena(*st) for st in states], [_Arena(*st) for st in states]
    ops.adam_step_multi([tuple(a.views()) for a in multi], t, **_kw(gscale))
    for a in single:
        ops.adam_step_t(*a.views(), t, **_kw(gscale))
    for n, a, b in zip(sizes, multi, single):
        for name, x, y in zip("pmv", a.read(), b.read()):
            assert np.array_equal(_bits(x), _bits(y)), f"n={n}: {name} of the three-arena launch differs from the single launch"


def test_zero_multi_three_buffers_between_canaries():
    """colvo_zero_multi shares k_adam_multi's arena table: 16, 4112 and 48 bytes, each between four canary words."""
    from coivo_amd import _lib, ops
    canary, words = 0x5A5A5A5A, [n // 4 for n in (16, 4112, 48)]
    bufs = [torch.full((4 + n + 4,), canary, dtype=torch.int32, device=dev()) for n in words]
    inner = [b[4:4 + n] for b, n in zip(bufs, words)]
    assert len(inner) <= _lib.MAX_ARENAS and all(v.data_ptr() % 16 == 0 for v in inner)      # the one-launch path of ops.zero_multi
    ops.zero_multi(inner)
    for b, n in zip(bufs, words):
        h = b.cpu().numpy()
        assert not h[4:4 + n].any(), f"{4 * n} bytes: not zero"
        assert (h[:4] == canary).all() and (h[4 + n:] == canary).all(), f"{4 * n} bytes: written outside the buffer"


# ---------------------------------------------------------------- k_adam_pack ------------------------------------------- #
SHAPES = [(32, 8), (40, 72), (16, 16), (136, 200), (8, 64)]         # (Cout, Cin): ragged against the 32 x 64 transpose tile
PLAIN = [1, 7, 2048, 2049, 4099]                                     # plain ranges around the 2048-element workgroup boundary
GUARD, GUARD_FWD, GUARD_BWD = 64, 80, 96
ENT = np.dtype([("param", "<u8"), ("grad", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"), ("fwd", "<u8"), ("bwd", "<u8"),
                ("w_off", "<i8"), ("fwd_off", "<i8"), ("bwd_off", "<i8"), ("n", "<i8"),
                ("Cout", "<i4"), ("kk", "<i4"), ("Cin", "<i4"), ("blk", "<i4"), ("kind", "<i4"), ("zero_grad", "<i4")])


def _pack_layout():
    """Layers and plain ranges interleaved, 64-float guard bands between the ranges (and in front: w_off is never zero), operand
    offsets that differ from the arena's and from each other, zero_grad set on every other entry of either kind."""
    from coivo_amd import _lib
    ents, off, foff, boff, blk = [], GUARD, GUARD_FWD, GUARD_BWD, 0
    for (co, ci), npl in zip(SHAPES, PLAIN):
        e = len(ents)
        n = co * 9 * ci
        ents.append(dict(kind=0, w_off=off, n=n, co=co, ci=ci, fwd_off=foff, bwd_off=boff, blk=blk, zg=(e // 2 + e) % 2))
        off, foff, boff = off + n + GUARD, foff + n + GUARD_FWD, boff + n + GUARD_BWD
        blk += 9 * ((co + 31) // 32) * ((ci + 63) // 64)
        e = len(ents)
        ents.append(dict(kind=1, w_off=off, n=npl, co=0, ci=0, fwd_off=-1, bwd_off=0, blk=blk, zg=(e // 2 + e) % 2))
        off += npl + GUARD
        blk += (npl + _lib.ADAM_PLAIN_PER_WG - 1) // _lib.ADAM_PLAIN_PER_WG
    assert {(e["kind"], e["zg"]) for e in ents} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    return ents, off, foff, boff, blk


def _sentinel(n, dtype):
    return torch.full((n,), 3.0, dtype=dtype, device=dev())


def _raw(t):
    return t.cpu().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _pack_step(dtype, state, t, gscale_host, gscale_dev=None, step=None, with_fwd=True):
    """One colvo_adam_pack_step[_scaled] over the hand-built table -> (p, g, m, v float32 arrays, fwd, bwd CPU tensors), with every
    byte the launch must not touch checked."""
    from coivo_amd import _lib, ops
    ents, total, ftotal, btotal, nblk = _pack_layout()
    assert len(state[0]) == total
    dev_state = [torch.from_numpy(x).to(dev()) for x in state]
    fwd = _sentinel(ftotal, dtype) if with_fwd else None
    bwd = _sentinel(btotal, dtype)
    tab = np.zeros(len(ents), dtype=ENT)
    for i, e in enumerate(ents):
        tab[i] = tuple(x.data_ptr() for x in dev_state) + (0 if fwd is None else fwd.data_ptr(), bwd.data_ptr(), e["w_off"],
                                                          e["fwd_off"] if with_fwd or e["kind"] else -1, e["bwd_off"],
                                                          e["n"] if e["kind"] else 0, e["co"], 9 if e["kind"] == 0 else 0, e["ci"],
                                                          e["blk"], e["kind"], e["zg"])
    table = torch.from_numpy(tab.view(np.uint8).copy()).to(dev())
    lib, args = _lib.load(), (ops.dt_code(dtype), _lib.ptr(table), len(ents), nblk, KW["lr"], KW["b1"], KW["b2"], KW["eps"], gscale_host)
    if gscale_dev is None:
        _lib.check(lib.colvo_adam_pack_step(*args, _lib.ptr(step), t, _lib.stream_ptr()), "colvo_adam_pack_step")
    else:
        _lib.check(lib.colvo_adam_pack_step_scaled(*args, _lib.ptr(gscale_dev), _lib.ptr(step), t, _lib.stream_ptr()),
                   "colvo_adam_pack_step_scaled")
    torch.cuda.synchronize()
    p1, g1, m1, v1 = (x.cpu().numpy() for x in dev_state)
    inside = np.zeros(total, bool)
    for e in ents:
        sl = slice(e["w_off"], e["w_off"] + e["n"])
        inside[sl] = True
        if e["zg"]:
            assert not _bits(g1[sl]).any(), ("zero_grad: the gradient range must read +0 throughout", e)
        else:
            assert np.array_equal(_bits(g1[sl]), _bits(state[1][sl])), ("gradient written without zero_grad", e)
    for name, new, old in zip("pgmv", (p1, g1, m1, v1), state):
        assert np.array_equal(_bits(new[~inside]), _bits(old[~inside])), f"{name}: a guard band was written"
    # operand copies: bit-equal to the cast / transpose of the kernel's OWN parameters, sentinel everywhere else
    layers = [e for e in ents if e["kind"] == 0]
    want = R.operand_copies(torch.from_numpy(p1), [(e["w_off"], e["co"], e["ci"]) for e in layers], dtype)
    exp_f, exp_b = _sentinel(ftotal, dtype).cpu(), _sentinel(btotal, dtype).cpu()
    for e, (wf, wb) in zip(layers, want):
        exp_f[e["fwd_off"]:e["fwd_off"] + e["n"]] = wf.reshape(-1)
        exp_b[e["bwd_off"]:e["bwd_off"] + e["n"]] = wb.reshape(-1)
    if with_fwd:
        assert torch.equal(_raw(fwd), _raw(exp_f)), "forward operand copy (or a byte outside the layers)"
    assert torch.equal(_raw(bwd), _raw(exp_b)), "transposed operand copy (or a byte outside the layers)"
    return (p1, g1, m1, v1), inside


def _pack_state(seed, gscale):
    """Random state over the whole arena (guard bands included); every range opens with the special elements."""
    ents, total, _, _, _ = _pack_layout()
    p, g, m, v = R.make_state(total, seed)
    for e in ents:
        sl = slice(e["w_off"], e["w_off"] + e["n"])
        k = R.plant_specials(p[sl], g[sl], m[sl], v[sl], gscale)
        p[sl][k + 1::2] = 0
    return p, g, m, v


def _hold_pack(kernel, case, new, inside, state, t, gscale):
    sel = lambda x: np.ascontiguousarray(x[inside])
    _hold(kernel, case, (sel(new[0]), sel(new[2]), sel(new[3])), tuple(sel(x) for x in state), t, gscale)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("t", [1, 2, 5, 1000])
def test_k_adam_pack_host_step_number(dtype, t):
    gscale = 0.125 if t % 2 else 1.0
    st = _pack_state(300 + t % 89, gscale)
    new, inside = _pack_step(dtype, st, t, gscale)
    _hold_pack(f"k_adam_pack<{'f32' if dtype == torch.float32 else 'bf16'}>", f"host t={t} gscale={gscale}", new, inside, st, t, gscale)


def test_k_adam_pack_without_a_forward_copy():
    """fp32 networks read the arena itself: fwd = NULL, fwd_off = -1 (optim.FusedAdam)."""
    st = _pack_state(311, 1.0)
    new, inside = _pack_step(torch.float32, st, 3, 1.0, with_fwd=False)
    _hold_pack("k_adam_pack<f32>", "no forward copy, t=3", new, inside, st, 3, 1.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_k_adam_pack_scaled_by_a_device_factor(dtype):
    """colvo_adam_pack_step_scaled: the gradient factor is float32(host) * float32(device), rounded to float32."""
    host, devf = np.float32(0.125), np.float32(0.37)
    gscale = float(np.float32(host * devf))
    st = _pack_state(322, gscale)
    factor = torch.tensor([0.37], dtype=torch.float32, device=dev())
    new, inside = _pack_step(dtype, st, 2, 0.125, gscale_dev=factor)
    assert float(factor.item()) == float(devf)
    _hold_pack(f"k_adam_pack<{'f32' if dtype == torch.float32 else 'bf16'}>", "scaled 0.125 x 0.37 (device), t=2", new, inside, st, 2, gscale)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("count0", [0, 999])
def test_k_adam_pack_device_step_counter(dtype, count0):
    gscale = 1.0
    p, g0, m, v = _pack_state(333 + count0, gscale)
    step = torch.tensor([count0], dtype=torch.int32, device=dev())
    for it in range(3):
        g = (g0 * np.float32(10.0 ** (it - 1))).astype(np.float32)
        new, inside = _pack_step(dtype, (p, g, m, v), 0, gscale, step=step)      # (t = 0: the host's step number is not read)
        assert int(step.item()) == count0 + it + 1
        _hold_pack(f"k_adam_pack<{'f32' if dtype == torch.float32 else 'bf16'}>", f"device counter {count0}+{it}", new, inside,
                   (p, g, m, v), count0 + it + 1, gscale)
        p, m, v = new[0].copy(), new[2].copy(), new[3].copy()
