"""No GPU: the registration replica (tests/register_ref.py) recovers known motions of an analytic tube and of a fused scene, ends in
every status where it must, and never returns a state it measures as worse; the argument checks of the colvo_register_* entry
points and of the Python functions."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from tests import register_ref as G

ITER = 8


@pytest.fixture(scope="module")
def lib():
    from coivo_amd import _lib, build
    build.ensure()
    return _lib.load()


@functools.lru_cache(maxsize=None)
def _loop(small, mode, metric, iterations=ITER):
    sc = G.tube(small=small, s_true=1.03 if mode == "sim3" else 1.0)
    return sc, G.register(sc["source"], sc["target"], sc["normals"], max_dist=sc["max_dist"], mode=mode, metric=metric,
                          iterations=iterations)


def _worst(sc, res):
    return float(G.true_error(sc["source"], sc["truth"], res["R"], res["t"], res["s"]).max())


# ---- 1. recovery ------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("mode", ["sim3", "se3"])
def test_plane_recovers_the_motion(mode):
    """The largest true point error after is at most 1/50 of the one before (what is left is the chord error of the sampling and
    does not shrink with iterations; this replica reaches 1/356 and 1/399), the scale within 1e-3 of the true one."""
    sc, res = _loop(False, mode, "plane")
    before = float(G.true_error(sc["source"], sc["truth"], *G.IDENTITY).max())
    after = _worst(sc, res)
    print(mode, "largest true error", before, "->", after, "ratio", before / after, "scale", res["s"], "true", sc["s"])
    assert res["status"] == G.OK
    assert after <= before / 50
    assert abs(res["s"] - sc["s"]) <= 1e-3
    h = res["history"]
    assert (h[:, 0] == len(sc["source"])).all() and (h[:, 1] == h[:, 0]).all() and (h[:, 2] == h[:, 0]).all()    # every point, every time
    if mode == "se3":
        assert res["s"] == 1.0


def test_small_scene_recovers_too():
    sc, res = _loop(True, "sim3", "plane")
    before = float(G.true_error(sc["source"], sc["truth"], *G.IDENTITY).max())
    print("small: largest true error", before, "->", _worst(sc, res))
    assert res["status"] == G.OK and _worst(sc, res) <= before / 50


# ---- 2. why plane is the default -------------------------------------------------------------------------------------------- #
def test_point_to_point_crawls_where_plane_converges():
    sc, plane = _loop(False, "sim3", "plane")
    _, point = _loop(False, "sim3", "point", 20)
    e_plane, e_point = _worst(sc, plane), _worst(sc, point)
    print("largest true error: plane after", ITER, "iterations", e_plane, "point after 20", e_point, "ratio", e_point / e_plane)
    assert point["status"] == G.OK
    assert e_point > 10 * e_plane


# ---- 3. never worse by its own measure -------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("seed,degrees,shift", [(1, 1.0, 0.02), (2, 5.0, 0.1), (3, 20.0, 0.5), (4, 20.0, 0.0), (5, 0.0, 0.5)])
def test_final_cost_is_not_above_the_first_or_the_state_is_the_input(seed, degrees, shift):
    sc = G.tube(small=True)
    init = G.bad_start(seed, degrees, shift)
    res = G.register(sc["source"], sc["target"], sc["normals"], init=init, max_dist=sc["max_dist"], iterations=4)
    h = res["history"]
    with np.errstate(all="ignore"):
        F0, F1 = h[0, 3] / h[0, 0], h[-1, 3] / h[-1, 0]
    print("start", degrees, "degrees", shift, "status", res["status"], "F", F0, "->", F1)
    if res["status"] == G.OK:
        assert F1 <= F0
    else:
        assert np.array_equal(res["R"], init[0]) and np.array_equal(res["t"], init[1]) and res["s"] == init[2]
        if res["status"] == G.REVERTED:
            assert F1 > F0


# ---- 4. status cases -------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("name", ["cylinder", "nearly_cylinder", "empty_target", "out_of_reach", "min_pairs"])
def test_status_cases(name):
    Q, P, Nrm, kw, want = G.status_cases()[name]
    res = G.register(Q, P, Nrm, **kw)
    print(name, "status", res["status"], "history", res["history"][:, :3].tolist())
    assert res["status"] == want
    init = kw["init"]
    assert np.array_equal(res["R"], init[0]) and np.array_equal(res["t"], init[1]) and res["s"] == init[2]
    if name == "cylinder":
        assert res["normal_matrix"][2, 2] == 0.0 and res["history"][0, 2] > 64
    if name == "nearly_cylinder":
        h = res["history"]
        assert h[-1, 3] / h[-1, 0] > 1.5 * h[0, 3] / h[0, 0]


# ---- 5. a fused scene ------------------------------------------------------------------------------------------------------- #
def test_fused_scene_registers():
    """fuse_ref.scene(6, 48, 64, 5): the stride-2 fusion onto the stride-1 fusion with normals_ref's normals.  The mean true error
    falls at least tenfold."""
    sc = G.fused_scene()
    has = int((np.abs(sc["normals"]).sum(1) > 0).sum())
    print("target rows", len(sc["target"]), "with a normal", has, "source points", len(sc["source"]))
    assert len(sc["target"]) > 10000 and has > 0.8 * len(sc["target"]) and len(sc["source"]) > 3000
    res = G.register(sc["source"], sc["target"], sc["normals"], max_dist=sc["max_dist"], iterations=ITER)
    before = float(G.true_error(sc["source"], sc["truth"], *G.IDENTITY).mean())
    after = float(G.true_error(sc["source"], sc["truth"], res["R"], res["t"], res["s"]).mean())
    print("mean true error", before, "->", after, "ratio", before / after, "pairs used", res["history"][0, 2], "->", res["history"][-1, 2])
    assert res["status"] == G.OK
    assert after <= before / 10


# ---- 6. entry points and wrappers ------------------------------------------------------------------------------------------- #
def _refused(lib, rc, *words):
    msg = lib.colvo_last_error()
    assert rc != 0, msg
    assert msg.startswith(b"colvo_register_"), msg
    for w in words:
        assert w in msg, msg


def test_register_entry_points_validate_their_arguments(lib):
    """Refused before any launch, with a message (without a GPU a call that got as far as a launch would report a HIP error
    instead of the check's message)."""
    from coivo_amd import _lib
    assert lib.colvo_abi_version() == _lib.ABI_VERSION >= 22
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    p = p if p % 16 == 0 else p + 8
    assert p % 16 == 0
    # the scratch: one row of 40 doubles per 1024 source points, the float32 state (64 bytes), the status (16 bytes)
    for n, size in ((0, 80), (1, 400), (1024, 400), (1025, 720), (6783, 2320), (2 ** 30 - 1, 2 ** 20 * 320 + 80)):
        assert lib.colvo_register_scratch_bytes(n) == size, n
    assert lib.colvo_register_scratch_bytes(-1) == 0 and lib.colvo_register_scratch_bytes(2 ** 30) == 0

    names = ("source", "N", "target", "normals", "M", "max_dist", "index", "state", "pivot")
    base = dict(source=p, N=4, target=p, normals=p, M=4, max_dist=0.1, index=p, state=p, pivot=p)
    acc = lambda **kw: lib.colvo_register_accumulate(*[kw.get(k, base[k]) for k in names], kw.get("metric", 0), kw.get("ws", p),
                                                     kw.get("sums", p), kw.get("counts", p), 0)
    loop = lambda **kw: lib.colvo_register_clouds(*[kw.get(k, base[k]) for k in names], kw.get("mode", 1), kw.get("metric", 0),
                                                  kw.get("iterations", 3), kw.get("damping", 1e-9), kw.get("min_pairs", 8),
                                                  kw.get("ws", p), kw.get("out", p + 512 if "out" not in kw else 0), kw.get("history", p),
                                                  kw.get("status", p), kw.get("normal", p), 0)
    for call, who, outs in ((acc, b"colvo_register_accumulate", ("sums", "counts")),
                            (loop, b"colvo_register_clouds", ("history", "status", "normal"))):
        for name in ("source", "target", "normals", "index", "state", "pivot", "ws") + outs:
            _refused(lib, call(**{name: 0}), who, b"null pointer")
        _refused(lib, call(N=2 ** 30), who, b"bad shape")
        _refused(lib, call(M=2 ** 30), who, b"bad shape")
        _refused(lib, call(N=-1), who, b"bad shape")
        for bad in (0.0, -0.1, math.inf, math.nan, 1e-30, 1e30):
            _refused(lib, call(max_dist=bad), who, b"bad max_dist")
        for bad in (-1, 2):
            _refused(lib, call(metric=bad), who, b"bad metric")
        _refused(lib, call(ws=p + 8), who, b"16-byte aligned")
        _refused(lib, call(index=p + 8), who, b"16-byte aligned")
    _refused(lib, lib.colvo_register_clouds(p, 4, p, p, 4, 0.1, p, p, p, 1, 0, 3, 1e-9, 8, p, 0, p, p, p, 0), b"null pointer")
    _refused(lib, loop(mode=2), b"bad mode")
    _refused(lib, loop(mode=-1), b"bad mode")
    for bad in (0, 65, -3):
        _refused(lib, loop(iterations=bad), b"bad iterations")
    for bad in (-1e-9, math.inf, math.nan):
        _refused(lib, loop(damping=bad), b"bad damping")
    _refused(lib, loop(min_pairs=0), b"min_pairs")
    _refused(lib, lib.colvo_register_clouds(p, 4, p, p, 4, 0.1, p, p, p, 1, 0, 3, 1e-9, 8, p, p, p, p, p, 0), b"alias")
    # the point metric takes no normals; an empty side needs no pointer: both get past the pointer check to the next refusal
    _refused(lib, acc(normals=0, metric=1, max_dist=0.0), b"bad max_dist")
    _refused(lib, acc(source=0, N=0, target=0, normals=0, M=0, max_dist=0.0), b"bad max_dist")


def test_kernels_use_no_scratch(lib, tmp_path):
    """The resource metadata of the four kernels (init, solve, and k_register_accum for each metric): no private segment, no spilled
    register -- the 37 float64 accumulators of k_register_accum stay in registers."""
    import re
    from coivo_amd import build
    asm = open(build.emit_asm("register.hip", str(tmp_path / "register.s"))).read()
    kernels = set(re.findall(r"\.name:\s+(\S*k_register_\w+)", asm))
    assert len(kernels) == 4 and all(any(f"k_register_{n}" in k for k in kernels) for n in ("init", "accum", "solve")), kernels
    assert sum("k_register_accum" in k for k in kernels) == 2
    for key in ("private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count"):
        vals = re.findall(rf"\.{key}:\s+(\d+)", asm)
        assert len(vals) == 4 and all(int(v) == 0 for v in vals), (key, vals)
    assert re.findall(r"\.agpr_count:\s+(\d+)", asm) in ([], ["0"] * 4)      # ... and are not parked in accumulation registers


def test_python_wrappers_refuse_bad_arguments_before_any_native_call():
    from coivo_amd import evaluate as E, registration
    assert E.Registration._fields == ("mode", "metric", "iterations", "max_dist", "damping", "min_pairs")
    assert tuple(E.Registration()) == ("sim3", "plane", 20, None, 1e-9, 64)
    assert E.RegistrationResult._fields == ("R", "t", "s", "history", "status", "normal_matrix")
    assert (E.REGISTER_OK, E.REGISTER_TOO_FEW, E.REGISTER_NOT_PD, E.REGISTER_REVERTED) == (G.OK, G.TOO_FEW, G.NOT_PD, G.REVERTED)
    import inspect
    for f in (E.cloud_metrics, E.reconstruction_metrics):
        assert inspect.signature(f).parameters["register"].default is None
    assert inspect.signature(E.cloud_metrics).parameters["gt_normals"].default is None
    assert E.CloudMetrics._fields[:3] == ("accuracy", "completeness", "chamfer") and len(E.CloudMetrics._fields) == 12
    m = E.CloudMetrics(*range(12))
    assert len(m) == 12 and m.registration is None and E.CloudMetrics(*range(12), registration=5).registration == 5
    assert m._replace(accuracy=7).accuracy == 7 and E.CloudMetrics(*range(12), registration=5)._replace(chamfer=1).registration == 5
    ok = torch.zeros(4, 3)
    for bad in (ok, ok.double(), torch.zeros(4, 2), [[0.0, 0.0, 0.0]]):           # (no CUDA tensor here: every cloud is refused)
        with pytest.raises(ValueError, match="float32 CUDA tensor of shape"):
            E.register_clouds(bad, bad, target_normals=bad, max_dist=0.1)
        with pytest.raises(ValueError, match="float32 CUDA tensor of shape"):
            E.register_accumulate(bad, bad, target_normals=bad, max_dist=0.1)
    for kw, word in ((dict(mode="affine"), "mode"), (dict(metric="colour"), "metric"), (dict(iterations=0), "iterations"),
                     (dict(iterations=65), "iterations"), (dict(iterations=2.0), "iterations"), (dict(iterations=True), "iterations"),
                     (dict(damping=-1.0), "damping"), (dict(damping=math.nan), "damping"), (dict(damping=math.inf), "damping"),
                     (dict(damping="x"), "damping"), (dict(min_pairs=0), "min_pairs"), (dict(min_pairs=1.5), "min_pairs")):
        with pytest.raises(ValueError, match=word):                                # (the policy is looked at before the clouds)
            E.register_clouds(ok, ok, max_dist=0.1, **kw)
        with pytest.raises(ValueError, match=word):
            registration.check_registration("x", E.Registration(**kw))
    for md in (0.0, -1.0, math.inf, math.nan, 1e-30, "a"):
        with pytest.raises(ValueError, match="max_dist"):
            registration.check_registration("x", E.Registration(max_dist=md))
    with pytest.raises(ValueError, match="Registration"):
        registration.check_registration("x", dict(mode="sim3"))
    with pytest.raises(ValueError, match="Registration"):
        E.cloud_metrics(ok, ok, max_dist=0.1, thresholds=(0.05,), register="sim3")
    with pytest.raises(ValueError):
        E.reconstruction_metrics(ok, torch.eye(4)[None], torch.zeros(1, 1, 8, 8), torch.eye(3)[None], torch.eye(4)[None], voxel_size=0.1,
                                 register=E.Registration(iterations=0))
