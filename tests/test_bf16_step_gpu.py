"""-m gpu: the BENCHMARKED backward pass against the oracle.

Every bitwise test of the step (hipGraph, RCCL, 2-rank data parallel) runs in deterministic mode, which switches the fused
full-resolution backward kernel (k_bwd16, HEAD form) and every fp32 atomic off; the configuration bench.py times -- bf16, float
atomics, k_fwd16_head / k_bwd16, forks on the kernels' completion signals, the gradient hand-over of the fused loss -- was compared
with the oracle only through network-level bounds (relative depth L1 < 1e-2, cosine > 0.97 on six tensors).  Here every parameter
gradient of that configuration goes against the fp32 oracle evaluated on the same bf16-rounded weights at the HIP path's ReLU
decisions, and the bar is DERIVED in the same step: the distance between that oracle and the oracle with the bf16 storage points
of the HIP networks emulated (tests/gpu_util.py oracle_step_bf16) is the size of the bf16 data path's own noise -- 0.5-1.5 % of a
gradient tensor's norm at B=2 64x96 (first run on the GPU: HIP 0.5-1.2e-2, emulated 0.3-1.6e-2) -- and a HIP gradient may be at
most 3 x that far from the oracle.  A dropped tile, a lost
atomic flush or a fork that lets a weight gradient read its dy early moves a layer's gradient by >= 10 %.
(bench.py times its networks with deterministic weight gradients, so that two runs compute the same thing; the form held here is
the library's default, the one a train loop runs.)"""
import pytest

from tests.gpu_util import K_NOISE, assert_bf16_step_at_the_noise_level, bf16_hip_step  # noqa: F401  (K_NOISE: the bar's factor)

pytestmark = pytest.mark.gpu


# (8, 256, 320) = BASELINE configs[1]; (32, 256, 320) = the per-GPU shape of configs[3], where the forms that are selected by GRID SIZE
# run -- k_conv_rt (>= 1024 workgroups), full weight-gradient grids beside halved ones, 64-wide weight-gradient tiles, whole-round
# k_bwd16 grids: VERDICT r5 item 4 (rounds 4-5 held the benchmarked backward to the oracle tensor by tensor at toy shapes only, where
# none of them is reached; at these shapes it was judged by cosines and a 1e-2 depth bar).
@pytest.mark.parametrize("B,H,W,seed", [(2, 64, 96, 71), (1, 96, 128, 72), (8, 256, 320, 73), (32, 256, 320, 74)])
def test_benchmarked_bf16_backward_against_the_oracle_at_the_bf16_noise_level(B, H, W, seed):
    from coivo_amd import _lib
    step = bf16_hip_step(B, H, W, seed)
    forms, ops_recorded = step["forms"], step["ops_recorded"]
    # what the dispatchers chose (include/colvo.h colvo_form_counts): production thresholds, nothing lowered for the test
    assert forms["wgrad_rt"] == 0
    if B >= 8:
        assert forms["wgrad_up2"] == 5                     # DepthNet's five up-sampled layers: the four-class form
    if B == 8:              # configs[1]: every weight-gradient grid halved (26 launches), the four single-split layers store behind zero_grad()
        assert forms["conv_rt"] == 0 and forms["wgrad_halved_grid"] == 26 and forms["wgrad_full_grid"] == 0, forms
        assert forms["wgrad_store_clean"] == 4 and forms["conv_res_s2"] >= 1, forms
    if B == 32:             # configs[3] per GPU: the register-tiled kernel on seven launches, ten full weight-gradient grids beside sixteen halved
        assert forms["conv_rt"] >= 7 and forms["wgrad_full_grid"] >= 10 and forms["wgrad_halved_grid"] >= 1, forms
    assert _lib.CMD_CONV_BWD_FUSED in ops_recorded and _lib.CMD_FORK in ops_recorded, ops_recorded
    assert _lib.tune_get("fork_stop_event") == 1

    # (tests/gpu_util.py: the body this test had, shared with tests/test_step_shapes_gpu.py; here the oracle stays on the CPU, whole)
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if os.path.isdir(os.path.join(root, "gpurun_out")):
        with open(os.path.join(root, "gpurun_out", f"bf16_step_parity_b{B}_{H}x{W}.txt"), "w") as f:
            assert_bf16_step_at_the_noise_level(step, seed, table=f)
    else:
        assert_bf16_step_at_the_noise_level(step, seed)
