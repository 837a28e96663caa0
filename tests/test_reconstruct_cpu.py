"""tests/reconstruct_ref.py held to its own conditions, without a GPU: it equals the oracle, its bound is honest (float32
evaluations of the formula in several orders stay inside it on every scene of tests/test_reconstruct_gpu.py), tight enough to matter,
and sensitive to the mistakes the bar of tests/test_inference_gpu.py lets through."""
import numpy as np
import pytest
import torch

from coivo_amd import synth
from tests import reconstruct_ref as R


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---- the replica is the oracle's operation -------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (2, 5, 7), (3, 17, 23), (2, 1, 257), (4, 64, 96)])
def test_world_points_are_the_oracles(B, H, W):
    from oracle import colvo_spec as S
    depth, K, M = R.scene(B, H, W, seed=11 + B)
    want = S.backproject(_t(depth).double(), _t(K).double(), _t(M).double()).numpy()
    got = R.world_points(depth, K, M)
    assert got.shape == want.shape == (B, H * W, 3) and got.dtype == np.float64
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("N,H,W,stride", [(2, 5, 7, 1), (3, 17, 23, 2), (4, 64, 96, 3), (2, 5, 7, 9), (5, 33, 47, 4), (300, 4, 4, 1)])
def test_stitch_is_the_oracles_membership_and_order(N, H, W, stride):
    from oracle import colvo_spec as S
    depth, K, M = R.scene(N, H, W, seed=31 + N, drop_frames=(1,) if N > 2 else ())
    want = S.stitch_point_cloud(_t(depth).double(), _t(K).double(), _t(M).double(), stride=stride).numpy()
    idx, ref, bound = R.stitch(depth, K, M, stride, S.MAX_DEPTH)
    keep = (_t(depth).double()[:, 0, ::stride, ::stride] < S.MAX_DEPTH).numpy()
    assert np.array_equal(idx, np.flatnonzero(keep.reshape(-1)))                  # membership and order, exactly
    assert ref.shape == want.shape == bound.shape and 0 < len(idx) <= keep.size
    assert np.abs(ref - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert R.block_counts(depth, stride, S.MAX_DEPTH).sum() == len(idx)
    # the points of the stitch are the back-projection's at the walked pixels
    full = R.world_points(depth, K, M).reshape(N, H, W, 3)[:, ::stride, ::stride].reshape(-1, 3)
    assert np.array_equal(ref, full[idx])


def test_max_depth_is_compared_in_float32():
    """What the module docstring says of the oracle's `depths < max_depth`, shown on the CPU."""
    from oracle import colvo_spec as S
    K, M = _t(R.intrinsics(np.random.default_rng(0), 1, 1, 4)), torch.eye(4)[None]
    for md, rounds_down in ((R.ODD_MAX_DEPTH, True), (0.1, False), (10.0, None)):
        m32 = np.float32(md)
        assert (float(m32) < md) == (rounds_down is True) and (float(m32) > md) == (rounds_down is False)
        d = np.array([R.pred32(md), m32, np.nextafter(m32, np.float32(np.inf)), np.inf], dtype=np.float32).reshape(1, 1, 1, 4)
        contract = R.keep_mask(d, 1, md).reshape(-1)
        assert contract.tolist() == [True, False, False, False]
        n32 = S.stitch_point_cloud(_t(d), K, M, max_depth=md).shape[0]              # float32 depths: the contract's comparison
        n64 = S.stitch_point_cloud(_t(d).double(), K.double(), M.double(), max_depth=md).shape[0]
        assert n32 == 1
        assert n64 == (2 if rounds_down else 1)                                     # float64 depths: keeps d == float32(md) iff md rounds down
        assert S.stitch_point_cloud(_t(d).double(), K.double(), M.double(), max_depth=R.f32(md)).shape[0] == 1


def test_build_keeps_fp32_division_correctly_rounded():
    """The bound counts one rounding for the division: no flag of the build may hand it to a faster, less exact expansion, or flush
    subnormals."""
    from coivo_amd import build
    flags = list(build.FLAGS) + [f for extra in build.FILE_FLAGS.values() for f in extra]
    for f in flags:
        assert "fast-math" not in f and "correctly-rounded" not in f and not f.startswith("-cl-") and "denormal" not in f \
            and "flush" not in f and "unsafe" not in f and "reciprocal" not in f and f != "-Ofast", f
    assert "reconstruct.hip" not in build.FILE_FLAGS
    assert R.DIV_ULP == 0.5 and R.K_ROUNDINGS == 7.0


# ---- the bound ------------------------------------------------------------------------------------------------------------------ #
def _forms_worst(depth, K, M, ref, bound, us=None, vs=None, sel=None):
    """Worst error / bound of every float32 form (and the class check where the reference is not finite)."""
    worst = {}
    for form in R.FORMS:
        got = R.emulate_f32(depth, K, M, form, us, vs).reshape(-1, 3)
        if sel is not None:
            got = got[sel]
        assert R.same_class(got, ref), form
        worst[form] = R.worst_ratio(got, ref, bound)[0]
    return worst


def _all_gpu_scenes():
    for B, H, W in R.BACKPROJECT_SHAPES:
        yield f"backproject {B}x{H}x{W}", lambda B=B, H=H, W=W: R.backproject_case(B, H, W)[:5]
    for kind in ("finite", "nonfinite"):
        yield f"backproject {kind}", lambda kind=kind: R.backproject_case(3, 17, 23, kind)[:5]
    for case in R.STITCH_CASES:
        yield "stitch " + "/".join(map(str, case)), lambda case=case: R.stitch_case(*case)


def test_bound_is_honest_and_tight_on_every_gpu_scene():
    """Every float32 form of the formula stays within the bound on every scene the GPU tests use, with the same class where the
    reference is not finite; and somewhere a form uses more than 5 % of it (a padded count would not be reached)."""
    top = 0.0
    for name, make in _all_gpu_scenes():
        c = make()
        if isinstance(c, dict):
            N, _, H, W = c["depth"].shape
            s = c["stride"]
            worst = _forms_worst(c["depth"], c["K"], c["M"], c["ref"], c["bound"], np.arange(0, W, s), np.arange(0, H, s), c["idx"])
        else:
            depth, K, M, ref, bound = c
            worst = _forms_worst(depth, K, M, ref.reshape(-1, 3), bound.reshape(-1, 3))
        print(f"RECONSTRUCT_REF {name}: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
        assert max(worst.values()) <= 1.0, (name, worst)
        top = max(top, max(worst.values()))
    assert top > 0.05, top


def test_special_depth_cases_hold_what_they_claim():
    depth, K, M, ref, bound, pos = R.backproject_case(3, 17, 23, "finite")
    assert np.array_equal(M[0], np.eye(4, dtype=np.float32)) and np.isfinite(ref).all() and np.isfinite(bound).all()
    flat = depth.reshape(-1)
    for i, v in enumerate(R.FINITE_SPECIALS):
        assert np.array_equal(flat[pos[i]], np.full(pos.shape[1], np.float32(v))) and (v == 0.0 or np.float32(v) != 0.0)
    assert pos[0][0] == 0 and np.all(ref.reshape(-1, 3)[0] == 0.0)         # depth 0 under the identity pose: the camera centre, 0
    in_frame0 = np.concatenate([pos[i][pos[i] < 17 * 23] for i in (3, 4, 5)])          # subnormal depths under the identity pose
    assert len(in_frame0) and np.all(np.abs(ref.reshape(-1, 3)[in_frame0]) < 2.0 ** -126)
    depth, K, M, ref, bound, pos = R.backproject_case(3, 17, 23, "nonfinite")
    nf = ~np.isfinite(ref.reshape(-1, 3)).all(axis=1)
    assert np.array_equal(np.sort(np.flatnonzero(nf)), np.sort(pos.reshape(-1)))    # exactly the planted pixels, every one decided
    assert np.isnan(ref).any() and (ref == np.inf).any() and (ref == -np.inf).any()
    assert not np.any(np.rint(K[:, :2, 2]) == K[:, :2, 2])                          # cx, cy off the integers: no 0 * inf
    for name, md in (("n6", R.MAX_DEPTH), ("n600", R.ODD_MAX_DEPTH)):
        c = R.stitch_case(name, "special", md)
        N, _, H, W = c["depth"].shape
        kept = np.zeros(N * H * W, dtype=bool)
        kept[c["idx"]] = True                                                       # stride 1: a sample's index is its pixel's
        for i, (_, want) in enumerate(R.STITCH_SPECIALS):
            assert np.all(kept[c["planted"][i]] == want), (name, md, i)
        m32 = np.float32(md)
        flat = c["depth"].reshape(-1)
        assert np.all(flat[c["planted"][5]] == m32) and np.all(flat[c["planted"][6]] == R.pred32(md)) and R.pred32(md) < m32
    assert R.f32(R.ODD_MAX_DEPTH) != R.ODD_MAX_DEPTH and R.f32(R.MAX_DEPTH) == R.MAX_DEPTH


def test_stitch_scenes_reach_what_they_are_for():
    """Block counts and `per` of the table; the variants' dropped runs cover a thread's whole share of k_scan_top."""
    want = {"n255": (255, 1), "n256": (256, 1), "n257": (257, 2), "n600": (600, 3), "n1000": (1000, 4), "n4099": (4099, 17),
            "n120": (120, 1), "n1280": (1280, 5), "n2560": (2560, 10), "n6": (6, 1)}
    for name, (n, per) in want.items():
        N, H, W, s = R.STITCH_SHAPES[name]
        assert R.n_blocks(N, H, W, s) == n and -(-n // 256) == per, name
    for name in ("n600", "n1000"):
        c = R.stitch_case(name, "run")
        zero = c["counts"] == 0
        per = c["per"]
        shares = [zero[i:i + per].all() for i in range(0, len(zero), per)]          # thread t holds blocks [t per, t per + per)
        assert any(shares), name
        c = R.stitch_case(name, "ends")
        bpf = c["n_blocks"] // c["depth"].shape[0]
        assert not c["counts"][:bpf].any() and not c["counts"][-bpf:].any() and c["counts"][bpf:-bpf].all()
        assert len(R.stitch_case(name, "all")["idx"]) == c["cap"] and len(R.stitch_case(name, "none")["idx"]) == 0
    c = R.stitch_case("n600", "plain")
    assert (c["counts"][0::2] > c["counts"][1::2]).all() and c["counts"][1::2].max() <= 17 * 23 - 256      # the second block is partial


def _class_pattern(p):
    return np.where(np.isnan(p), 3, np.where(p == np.inf, 1, np.where(p == -np.inf, 2, 0)))


def test_order_is_visible_on_every_stitch_scene():
    """Consecutive kept samples differ in at least one coordinate by more than the sum of their two bounds (or, where a coordinate is
    not finite, in its class): a shift or a swap of rows cannot hide inside the bar."""
    for case in R.STITCH_CASES:
        c = R.stitch_case(*case)
        ref, bound = c["ref"], c["bound"]
        if len(ref) < 2:
            continue
        with np.errstate(invalid="ignore"):
            far = np.abs(ref[1:] - ref[:-1]) > bound[1:] + bound[:-1]
        other_class = _class_pattern(ref[1:]) != _class_pattern(ref[:-1])
        visible = (far | other_class).any(axis=1)
        assert visible.all(), (case, np.flatnonzero(~visible)[:5])


# ---- sensitivity: one mutation of the reference at a time ------------------------------------------------------------------------ #
def _synth_scene(N, H, W, seed):
    """The scene of tests/test_inference_gpu.py: one K for every frame, fx == fy."""
    g = torch.Generator().manual_seed(seed)
    depth = (0.3 + 4.0 * torch.rand(N, 1, H, W, generator=g)).numpy()
    K = synth.intrinsics(N, H, W).numpy()
    M = R.rigid_chain(np.random.default_rng(seed), N)
    return depth, K, M


def _write_with_offsets(c, offsets):
    """What k_stitch_write leaves in rows [0, count) when block b starts at offsets[b] (unwritten rows: zero)."""
    out = np.zeros((c["cap"] + 2, 3))
    starts = R.exclusive(c["counts"])
    for b in np.flatnonzero(c["counts"]):
        n = c["counts"][b]
        out[offsets[b]:offsets[b] + n] = c["ref"][starts[b]:starts[b] + n]
    return out[:len(c["ref"])]


def _mutations(c):
    """name -> the mutated result for the stitch case c, as the kernel would have returned it."""
    depth, K, M, s, md = c["depth"], c["K"], c["M"], c["stride"], c["max_depth"]
    ref = c["ref"]
    k = len(ref) // 2
    yield "K of frame 0 for every frame", R.stitch(depth, np.ascontiguousarray(np.broadcast_to(K[:1], K.shape)), M, s, md)[1]
    Kx = K.copy(); Kx[:, 0, 0], Kx[:, 1, 1] = K[:, 1, 1], K[:, 0, 0]
    yield "fx <-> fy", R.stitch(depth, Kx, M, s, md)[1]
    Kc = K.copy(); Kc[:, 0, 2], Kc[:, 1, 2] = K[:, 1, 2], K[:, 0, 2]
    yield "cx <-> cy", R.stitch(depth, Kc, M, s, md)[1]
    yield "one kept sample dropped", np.delete(ref, k, axis=0)
    sw = ref.copy(); sw[[k, k + 1]] = ref[[k + 1, k]]
    yield "two consecutive kept samples exchanged", sw
    off = R.exclusive(c["counts"]); off[257:] += 1
    yield "every offset after block 256 shifted by one", _write_with_offsets(c, off)
    e = ref.copy(); e[:, 1] *= 1.0 + 64.0 * R.U
    yield "relative error 64 u on one coordinate", e


def test_every_mutation_breaks_the_new_bar_and_the_gap_is_the_old_bars():
    c = R.stitch_case("n600", "plain")
    assert R.new_bar(c["ref"], c["ref"], c["bound"]) and R.old_bar(c["ref"], c["ref"])
    assert R.new_bar(_write_with_offsets(c, R.exclusive(c["counts"])), c["ref"], c["bound"])       # the unmutated write-out
    # the old bar on its own kind of scene (one K, fx == fy, cx and cy the frame's centre), at the same shape
    depth, K, M = _synth_scene(*R.STITCH_SHAPES["n600"][:3], seed=60)
    s = dict(depth=depth, K=K, M=M, stride=1, max_depth=R.MAX_DEPTH)
    s["idx"], s["ref"], s["bound"] = R.stitch(depth, K, M, 1, R.MAX_DEPTH)
    s["counts"], s["cap"] = R.block_counts(depth, 1, R.MAX_DEPTH), depth.size
    on_synth = {name: got for name, got in _mutations(s)}
    print("\nRECONSTRUCT_SENSITIVITY mutation | seen by new bar | seen by old bar | seen by old bar on a synth.intrinsics scene")
    rows = {}
    for name, got in _mutations(c):
        new_sees, old_sees = not R.new_bar(got, c["ref"], c["bound"]), not R.old_bar(got, c["ref"])
        old_sees_synth = not R.old_bar(on_synth[name], s["ref"])
        rows[name] = (new_sees, old_sees, old_sees_synth)
        print(f"RECONSTRUCT_SENSITIVITY {name} | {new_sees} | {old_sees} | {old_sees_synth}")
        assert new_sees, name
        if got.shape == c["ref"].shape:
            assert R.worst_ratio(got, c["ref"], c["bound"])[0] > 1.0, name           # more than the bound on at least one element
    assert len(rows) == 7
    # the gap: the old bar passes these
    assert not rows["relative error 64 u on one coordinate"][1] and not rows["relative error 64 u on one coordinate"][2]
    assert not rows["K of frame 0 for every frame"][2] and not rows["fx <-> fy"][2]
