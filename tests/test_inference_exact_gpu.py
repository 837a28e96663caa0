"""-m gpu: inference.run_networks -- DepthNet on every frame, PoseNet on every consecutive pair, `chunk` at a time -- against the
oracle's networks at real resolutions and at the call sizes inference produces: a full chunk, the tail of a sequence, one frame.

run_networks sits under reconstruct_sequence and every post-training feature; until now it was compared with the oracle once, at 5
frames of 64x96 in fp32 (tests/test_inference_gpu.py), and bf16 inference with nothing.  Cases (frames, H, W, chunk):
  (6, 256, 320, 4)     DepthNet calls of 4 + 2 frames, PoseNet calls of 4 + 1 pairs (the last pose call is frames[i:j], j = min(i + chunk, n - 1));
  (14, 256, 320, 16)   one call of 14 frames and one of 13 pairs: a chunk that is not full;
  (3, 512, 640, 2)     calls of 2 + 1 frames and one call of 2 pairs at the large resolution;
  (2, 256, 320, 1)     single-frame calls throughout: the live stream.
The reference is the oracle run whole on the GPU, MIOpen off (gpu_util.oracle_networks).

fp32: the HIP networks on the spec weights against the oracle in float64 (PoseNet fed the float64 depths).  Bars: depth
max|d - d64| < 1e-4 (DEPTH_TOL, the north-star figure of tests/test_config1_gpu.py), relative poses < 1e-6 (as
test_reconstruct_sequence_end_to_end).  The fp32 oracle's own distance from float64 is measured beside them, and the depth error is
also held to GRAD_K x it (the step tests' factor): the fixed bar is 500 x the rounding noise measured here.
bf16: no constant.  The target is the fp32 oracle on bf16-rounded weights, the noise scale the same oracle with the HIP networks' bf16
storage points emulated (gpu_util._bf16_hooks).  Depth: the mean error is at most K_NOISE x the emulated run's.  Poses: per pair, the
6-vector's distance from the target is at most K_NOISE x the larger of the emulated run's distance for that pair and the typical
(median) one over the pairs -- one emulated run is one draw of the noise (gpu_util.assert_bf16_step_at_the_noise_level).
Plumbing, bit for bit: every chunk's rows equal a direct call of the network on that slice, and the result under
torch.inference_mode() equals the one under no_grad.
Forms: the kernel forms a case selects lie inside what tests/test_conv_exact_small_batch_gpu.py pinned (FORMS) for the part-1 batch
sizes that bracket each call size at that resolution; a form outside means a shape is missing there.

First run (profiles/inference_shapes.md): fp32 depth 1.6e-7 ... 2.7e-7 and poses 2e-9 ... 6e-9 from float64 in every case, 512x640
included -- the fp32 oracle's own distance (1.3e-7 ... 2.7e-7, 1.5e-9 ... 4e-9), so both fixed bars hold with room and no derived bar
is needed.  bf16: depth error / emulated 1.00 in every case, worst pose ratio 1.47 (bar K_NOISE = 3).  Under a second per case."""
import gc
import time

import pytest
import torch

from coivo_amd import synth
from tests.gpu_util import GRAD_K, K_NOISE, bf16_rounded_state, dev, oracle_networks
from tests.test_conv_exact_small_batch_gpu import FORMS as PINNED

pytestmark = pytest.mark.gpu

DEPTH_TOL, POSE_TOL = 1e-4, 1e-6
CASES = [(6, 256, 320, 4), (14, 256, 320, 16), (3, 512, 640, 2), (2, 256, 320, 1)]


@pytest.fixture(autouse=True)
def _free_between_cases():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _call_sizes(n, chunk):
    """(DepthNet call sizes, PoseNet call sizes) of run_networks on n frames."""
    depth = [min(chunk, n - i) for i in range(0, n, chunk)]
    pose = [min(i + chunk, n - 1) - i for i in range(0, n - 1, chunk)]
    return depth, pose


def _pinned_for(net, c, H, W, dtype):
    """The union of the forms part 1 pinned for the batch sizes nearest to c from below and from above at this resolution."""
    sizes = sorted(B for (nt, B, h, w) in PINNED if (nt, h, w) == (net, H, W))
    assert sizes, f"no {net} shape of {H}x{W} in tests/test_conv_exact_small_batch_gpu.py"
    near = {max([b for b in sizes if b <= c], default=None), min([b for b in sizes if b >= c], default=None)} - {None}
    return set().union(*(PINNED[net, b, H, W][dtype] for b in near))


def _hip_networks(seed, dtype):
    from coivo_amd import nn as hnn
    from oracle import colvo_spec as S
    dn_o, pn_o = S.make_models(seed)
    dn, pn = hnn.DepthNet(compute_dtype=dtype), hnn.PoseNet(compute_dtype=dtype)
    bf = dtype == torch.bfloat16
    dn.load_state_dict(bf16_rounded_state(dn_o) if bf else dn_o.state_dict())
    pn.load_state_dict(bf16_rounded_state(pn_o) if bf else pn_o.state_dict())
    return dn, pn


def _run(n, H, W, chunk, dtype, seed):
    """run_networks on the HIP networks -> (frames, depths, poses on the CPU, seconds); checks the plumbing and the selected forms."""
    from coivo_amd import _lib, inference as I
    assert _lib.tune_get("wgrad_rt") == 0 and _lib.tune_get("quad_min_wgs") == 8192 and _lib.tune_get("res_min_tiles") == 2048, \
        "production tuning expected"
    frames_cpu = synth.make_batch(n, H, W, seed=seed)["tgt"]
    frames = frames_cpu.to(dev())
    dn, pn = _hip_networks(seed, dtype)
    torch.cuda.synchronize()
    _lib.form_counts(reset=True)
    t0 = time.perf_counter()
    depths, poses = I.run_networks(dn, pn, frames, chunk=chunk)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    forms = {k for k, v in _lib.form_counts().items() if v}
    assert depths.shape == (n, 1, H, W) and poses.shape == (n - 1, 6)
    # every chunk's rows are what the network returns for that slice alone
    with torch.no_grad():
        for i in range(0, n, chunk):
            assert torch.equal(depths[i:i + chunk], dn(frames[i:i + chunk].contiguous())), f"DepthNet rows {i}.."
        for i in range(0, n - 1, chunk):
            j = min(i + chunk, n - 1)
            p, _, _ = pn(frames[i:j].contiguous(), frames[i + 1:j + 1].contiguous(), depths[i:j].contiguous(), depths[i + 1:j + 1].contiguous())
            assert torch.equal(poses[i:j], p), f"PoseNet rows {i}..{j}"
    # ... and inference_mode changes nothing
    with torch.inference_mode():
        d_i, p_i = I.run_networks(dn, pn, frames, chunk=chunk)
    assert torch.equal(d_i, depths) and torch.equal(p_i, poses), "inference_mode differs from no_grad"
    # the forms: inside what part 1 pinned for the call sizes involved
    key = str(dtype)[6:]
    dsz, psz = _call_sizes(n, chunk)
    allowed = set().union(*[_pinned_for("depth", c, H, W, key) for c in dsz], *[_pinned_for("pose", c, H, W, key) for c in psz])
    print(f"INFER-FORMS {n}x{H}x{W} chunk {chunk} {key}: calls depth {dsz} pose {psz}: {sorted(forms)}")
    assert forms <= allowed, f"forms outside part 1's pinned sets: {sorted(forms - allowed)}"
    return frames_cpu, depths.cpu(), poses.cpu(), seconds


@pytest.mark.parametrize("n,H,W,chunk", CASES)
def test_run_networks_fp32_against_the_float64_oracle(n, H, W, chunk):
    seed = 200 + n
    t0 = time.perf_counter()
    frames, depths, poses, t_hip = _run(n, H, W, chunk, torch.float32, seed)
    d64, p64 = oracle_networks(seed, frames, torch.float64, dev())
    d32, p32 = oracle_networks(seed, frames, torch.float32, dev())
    ed, ep = (depths.double() - d64).abs().max().item(), (poses.double() - p64).abs().max().item()
    od, op = (d32.double() - d64).abs().max().item(), (p32.double() - p64).abs().max().item()
    print(f"INFER fp32 {n}x{H}x{W} chunk {chunk}: depth max|d - d64| hip {ed:.3e} (fp32 oracle {od:.3e}, bar {DEPTH_TOL:g}); "
          f"pose hip {ep:.3e} (fp32 oracle {op:.3e}, bar {POSE_TOL:g}); run_networks {1e3 * t_hip:.1f} ms, case {time.perf_counter() - t0:.1f} s")
    assert ed < DEPTH_TOL, (ed, od)
    assert ep < POSE_TOL, (ep, op)
    # ... and beside the fixed bars: the depth error is a maximum over 1.6e5 pixels or more per frame, a stable statistic, and the fp32
    # oracle's own on the same input is the size of fp32 rounding in this network -- a HIP error GRAD_K times that is no rounding.
    # (The poses are 6 to 78 numbers: their maximum is a small sample, printed and held by the fixed bar only.)
    assert ed <= GRAD_K * od, (ed, od)


@pytest.mark.parametrize("n,H,W,chunk", CASES)
def test_run_networks_bf16_at_the_noise_level(n, H, W, chunk):
    seed = 300 + n
    t0 = time.perf_counter()
    frames, depths, poses, t_hip = _run(n, H, W, chunk, torch.bfloat16, seed)
    d_t, p_t = oracle_networks(seed, frames, torch.float32, dev(), bf16_weights=True)                     # the target
    d_e, p_e = oracle_networks(seed, frames, torch.float32, dev(), bf16_weights=True, emulate=True)       # the noise scale
    eh, ee = (depths - d_t).abs().mean().item(), (d_e - d_t).abs().mean().item()
    ph, pe = (poses - p_t).norm(dim=1), (p_e - p_t).norm(dim=1)
    typical = pe.sort().values[len(pe) // 2].item()
    scale = torch.clamp(pe, min=typical)
    worst = (ph / scale).max().item()
    print(f"INFER bf16 {n}x{H}x{W} chunk {chunk}: depth mean|d - target| hip {eh:.3e} (emulated {ee:.3e}, ratio {eh / ee:.2f}); "
          f"pose |p - target| hip max {ph.max().item():.3e} (emulated max {pe.max().item():.3e}, typical {typical:.3e}, worst ratio {worst:.2f}); "
          f"run_networks {1e3 * t_hip:.1f} ms, case {time.perf_counter() - t0:.1f} s")
    assert eh <= K_NOISE * ee, (eh, ee)
    assert bool((ph <= K_NOISE * scale).all()), (ph.tolist(), pe.tolist(), typical)
