"""-m gpu: the whole training step against the float64 oracle at the two largest shapes, tensor by tensor.

Every kernel is held hard at the benchmark shapes by itself (tests/test_conv_exact_gpu.py bit for bit, the heads and the fused loss
against float64); what was not is their COMPOSITION there -- the recorded program with its forks and side streams, the fused
full-resolution kernels, the sliced and grouped weight gradients, the gradient hand-over from the loss, PoseNet's input filled by
DepthNet's pass.  configs[2] (512x640) was "finite only", configs[4] per rank (64 pairs of 256x320) was judged by a cosine against
its own slices.  The step-level bars of tests/gpu_util.py -- the fp64 truth, the fp32 oracle as the noise scale, matched ReLU
decisions; for bf16 the oracle on bf16-rounded weights with the emulated storage points as the noise scale -- stopped at 8 pairs
(fp32) and 32 pairs (bf16) because the oracle ran on the CPU.  Here it runs on the GPU, in slices of 16 frames of 256x320 (or the
same pixel count at 512x640) so that its autograd graph stays small; tests/test_step_ref_cpu.py checks that reference first.

Shapes (pairs, H, W):
  (64, 256, 320)   configs[4] per rank;
  (P, 512, 640)    P the SMALLEST pair count whose step selects the same set of kernel forms (non-zero colvo_form_counts) as the
                   32 pairs of configs[2] do -- found per dtype by stepping 2, 4, 8, 16, 32 pairs (profiles/step_parity_shapes.md);
  (8, 256, 320)    the widened objective (full_loss), fp32, unsliced: compared with the oracle at 2x64x96 only until now.
Every case runs the production tuning and the networks' default form (float atomics), and asserts which forms its step selected.

The fp32 yardstick on the GPU: MIOpen is switched off for the oracle (tests/gpu_util.py _plain_convs), and its distance from float64
was measured beside the CPU oracle's at (2, 64, 96) and (8, 256, 320), decisions matched -- profiles/step_parity_shapes.md: worst
tensor 4.1e-6 against the CPU's 6.5e-6, and 7.2e-4 against 6.9e-4.  At the second shape the GPU's is the larger one (by 5 %, on
DepthNet's middle layers; on PoseNet's tensors it is a third smaller), so the fp32 cases here do not rely on it alone: the fp32
oracle runs on the CPU as well, in the same slices, and the noise scale of every tensor is GRAD_K x the SMALLER of the two
distances (matched_grad_rows cpu_yardstick=True).  That CPU run is most of these cases' time.

First run on the GPU (profiles/step_parity_shapes.md): 58 tensors judged in every case; worst HIP error over its noise scale 0.85
(fp32, 64 pairs), 0.71 (fp32, 32 pairs of 512x640), 2.83 (widened objective; the tensor nearest its bar uses 65 % of it), 2.52 and 1.53
(bf16); largest forced pre-activation 5.3e-6 (RELU_MARGIN 1e-5).  Seconds per case: 36, 59, 3, 4.5, 7 -- of the first two, 23 and 46
are the CPU's fp32 oracle, 8 and 6 the float64 oracle on the GPU.
"""
import contextlib
import os
import time

import pytest
import torch

from coivo_amd import synth
from tests.gpu_util import (assert_bf16_step_at_the_noise_level, bf16_hip_step, dev, grad_parity_failures, matched_grad_rows,
                            oracle_step, to_dev)

pytestmark = pytest.mark.gpu

DEPTH_TOL, LOSS_TOL = 1e-4, 1e-5                 # BASELINE.json north_star, as in tests/test_config1_gpu.py
SLICE_PIXELS = 8 * 256 * 320                     # pairs x pixels of one oracle slice: 16 frames of 256x320

# The kernel forms a step selects (non-zero counters), measured once with the production tuning: profiles/step_parity_shapes.md.
# At 512x640 the 32 pairs of configs[2] are the smallest count of 2, 4, 8, 16, 32 that selects configs[2]'s set, in both dtypes: the
# image-sliced weight gradient (a tensor of 1 GiB) starts at 16 pairs in fp32 and above 16 in bf16, and in fp32 the last conv_res
# launch of 16 pairs is gone at 32.
_LARGE = {"conv_rt", "conv_rt_bn32", "conv_tile", "conv_ring", "conv_bn64", "conv_res_s2", "conv_up2_bn16", "conv_up2_bn32",
           "dgrad_s2", "dgrad_s2_ring", "dgrad_up2", "dgrad_both", "wgrad_full_grid", "wgrad_halved_grid", "wgrad_up2", "wgrad_teams",
           "wgrad_tail", "wgrad_mt4"}
_HEAD16 = {"fwd16_head", "bwd16", "dgrad_planes_mfma"}            # the fused full-resolution kernels of bf16 mode
_SMALL = {"conv_rt", "conv_rt_bn32", "conv_tile", "conv_ring", "conv_res", "conv_res_s2", "conv_up2_bn16", "dgrad_s2", "dgrad_s2_ring",
          "dgrad_up2", "dgrad_both", "wgrad_full_grid", "wgrad_halved_grid", "wgrad_up2", "wgrad_teams", "wgrad_tail", "wgrad_mt4",
          "wgrad_store_clean"}
FORMS = {
    ("fp32", 64, 256, 320): _LARGE | {"conv_res", "wgrad_sliced", "wgrad_store_clean"},
    ("bf16", 64, 256, 320): _LARGE | _HEAD16 | {"conv_res"},
    ("fp32", 512, 640): _LARGE | {"wgrad_sliced", "wgrad_store_clean"},                     # 32 pairs
    ("bf16", 512, 640): _LARGE | _HEAD16 | {"conv_res", "wgrad_sliced"},                    # 32 pairs; tests/test_large_gpu.py too
    ("fp32", 8, 256, 320, "full_loss"): _SMALL,
}
P_512x640 = {"fp32": 32, "bf16": 32}


def selected(forms):
    return {k for k, v in forms.items() if v}


def _production_tuning():
    from coivo_amd import _lib
    assert _lib.tune_get("wgrad_rt") == 0 and _lib.tune_get("quad_min_wgs") == 8192, "production tuning expected"
    assert _lib.tune_get("march_rows_fwd") == 0 and _lib.tune_get("march_rows_bwd") == 0, "production tuning expected"


def _out(name):
    """Where a case's per-tensor table goes: the directory COLVO_TEST_TABLES names, if it names one."""
    d = os.environ.get("COLVO_TEST_TABLES")
    return os.path.join(d, name) if d and os.path.isdir(d) else None


def _slice_pairs(H, W):
    return SLICE_PIXELS // (H * W)


def _fp32_case(pairs, H, W, seed, full_loss=False):
    """One fp32 HIP step against the matched oracles: the assertions of test_config1_fp32_step_parity.  -> the step's forms."""
    from coivo_amd import _lib, nn as hnn
    from oracle import colvo_spec as S
    _production_tuning()
    b = synth.make_batch(pairs, H, W, seed=seed)
    d = to_dev(b)
    dn_o, pn_o = S.make_models(seed)
    dn, pn = hnn.DepthNet(compute_dtype=torch.float32), hnn.PoseNet(compute_dtype=torch.float32)
    dn.load_state_dict(dn_o.state_dict())
    pn.load_state_dict(pn_o.state_dict())
    dn.deterministic = pn.deterministic = False            # the default form (float atomics), whatever COLVO_DETERMINISTIC says
    dn.zero_grad(); pn.zero_grad()
    _lib.form_counts(reset=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss, d_t, d_r, pose, a, bb = hnn.dcdp_forward(dn, pn, d["tgt"], d["ref"], d["K"], full_loss=full_loss)
    loss.backward()
    dn.join_side(); pn.join_side()
    torch.cuda.synchronize()
    t_hip = time.perf_counter() - t0
    forms = _lib.form_counts()
    print(f"kernel forms of this step: {forms}")
    tag = f"fp32_b{pairs}_{H}x{W}" + ("_full" if full_loss else "")
    timings = {}
    sp = None if full_loss else _slice_pairs(H, W)
    rows, m32, _ = matched_grad_rows(seed, b, dn, pn, _out(f"step_parity_{tag}.txt"), device=dev(), slice_pairs=sp, full_loss=full_loss,
                                     timings=timings, cpu_yardstick=True)
    figures = dict(loss=abs(loss.item() - m32["loss"]), d_t=(d_t.detach().cpu() - m32["d_t"]).abs().max().item(),
                   d_r=(d_r.detach().cpu() - m32["d_r"]).abs().max().item(), pose=(pose.detach().cpu() - m32["pose"]).abs().max().item(),
                   a=(a.detach().cpu() - m32["a"]).abs().max().item(), b=(bb.detach().cpu() - m32["b"]).abs().max().item())
    worst = max(max(r[5] / max(r[6], 1e-300), (r[3] / max(r[4], 1e-300))) for r in rows)
    print(f"{tag}: {len(rows)} tensors judged, worst hip / fp32-oracle noise ratio {worst:.2f} (relL2: hip {max(r[5] for r in rows):.2e}, "
          f"fp32 oracle {max(r[6] for r in rows):.2e}); |d| vs the matched fp32 oracle: " + ", ".join(f"{k} {v:.2e}" for k, v in figures.items()))
    print(f"{tag}: seconds: HIP step {t_hip:.2f}, masks {timings['masks']:.2f}, fp32 oracle {timings['o32']:.2f}, fp64 oracle {timings['o64']:.2f}, "
          f"masks to the CPU {timings['masks_cpu']:.2f}, fp32 oracle on the CPU {timings['c32']:.2f}")
    assert figures["loss"] < LOSS_TOL, (loss.item(), m32["loss"])
    assert figures["d_t"] < DEPTH_TOL and figures["d_r"] < DEPTH_TOL, figures
    assert figures["pose"] < 1e-6 and figures["a"] < 1e-6 and figures["b"] < 1e-6, figures
    assert len(rows) == 58
    bad = grad_parity_failures(rows)
    assert not bad, "\n".join(bad)
    return forms


def _bf16_case(pairs, H, W, seed):
    """One bf16 HIP step at the bf16 noise bar (tests/test_bf16_step_gpu.py's assertions).  -> (forms, recorded backward ops)."""
    _production_tuning()
    step = bf16_hip_step(pairs, H, W, seed)
    timings = {}
    out = _out(f"step_parity_bf16_b{pairs}_{H}x{W}.txt")
    with (open(out, "w") if out else contextlib.nullcontext()) as table:
        worst = assert_bf16_step_at_the_noise_level(step, seed, device=dev(), slice_pairs=_slice_pairs(H, W), timings=timings, table=table)
    print(f"bf16_b{pairs}_{H}x{W}: 58 tensors judged, worst hip / noise ratio {worst:.2f}; seconds: HIP step {step['seconds']:.2f}, "
          f"masks {timings['masks']:.2f}, target oracle {timings['target']:.2f}, emulated oracle {timings['emulated']:.2f}")
    return step["forms"], step["ops_recorded"]


@pytest.fixture(autouse=True)
def _free_between_cases():
    yield
    import gc
    gc.collect()
    torch.cuda.empty_cache()


def test_the_gpu_oracle_is_the_cpu_oracle():
    """Float64 on the GPU, sliced, against float64 on the CPU, whole: the same numbers up to the order of float64 sums.  The fp32
    oracle's own distance from float64 is 2e-6 at this shape with a unit roundoff of 6e-8, so float64's (1e-16) is ~4e-15; 1e-10
    is four orders under the noise the bars work at."""
    seed, shape = 71, (2, 64, 96)
    b = synth.make_batch(*shape, seed=seed)
    c64 = oracle_step(seed, b, torch.float64)
    g64 = oracle_step(seed, b, torch.float64, device=dev(), slice_pairs=1)
    assert abs(g64["loss"] - c64["loss"]) <= 1e-12
    for (n, g), (_, c) in zip(g64["grads"], c64["grads"]):
        assert (g - c).norm().item() <= 1e-10 * c.norm().item(), n
    assert (g64["d_t"] - c64["d_t"]).abs().max().item() <= 1e-12 and (g64["d_r"] - c64["d_r"]).abs().max().item() <= 1e-12


def test_config4_per_rank_fp32_step_parity():
    forms = _fp32_case(64, 256, 320, seed=81)
    assert selected(forms) == FORMS["fp32", 64, 256, 320], sorted(selected(forms))


def test_config4_per_rank_bf16_step_parity():
    from coivo_amd import _lib
    forms, ops_recorded = _bf16_case(64, 256, 320, seed=82)
    assert forms["wgrad_rt"] == 0 and forms["wgrad_up2"] == 5, forms
    assert _lib.CMD_CONV_BWD_FUSED in ops_recorded and _lib.CMD_FORK in ops_recorded, ops_recorded
    assert selected(forms) == FORMS["bf16", 64, 256, 320], sorted(selected(forms))


def test_config2_shape_fp32_step_parity():
    forms = _fp32_case(P_512x640["fp32"], 512, 640, seed=83)
    assert selected(forms) == FORMS["fp32", 512, 640], sorted(selected(forms))


def test_config2_shape_bf16_step_parity():
    forms, _ = _bf16_case(P_512x640["bf16"], 512, 640, seed=84)
    assert selected(forms) == FORMS["bf16", 512, 640], sorted(selected(forms))


def test_config1_widened_objective_fp32_step_parity():
    forms = _fp32_case(8, 256, 320, seed=85, full_loss=True)
    assert selected(forms) == FORMS["fp32", 8, 256, 320, "full_loss"], sorted(selected(forms))
