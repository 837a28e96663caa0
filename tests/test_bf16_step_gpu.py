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
import torch

from coivo_amd import synth
from tests.gpu_util import bf16_rounded_state, hip_relu_masks, oracle_step_bf16, to_dev

pytestmark = pytest.mark.gpu

K_NOISE = 3.0


def _rel(a, b):
    return (a - b).norm().item() / max(b.norm().item(), 1e-30)


# (8, 256, 320) = BASELINE configs[1]; (32, 256, 320) = the per-GPU shape of configs[3], where the forms that are selected by GRID SIZE
# run -- k_conv_rt (>= 1024 workgroups), full weight-gradient grids beside halved ones, 64-wide weight-gradient tiles, whole-round
# k_bwd16 grids: VERDICT r5 item 4 (rounds 4-5 held the benchmarked backward to the oracle tensor by tensor at toy shapes only, where
# none of them is reached; at these shapes it was judged by cosines and a 1e-2 depth bar).
@pytest.mark.parametrize("B,H,W,seed", [(2, 64, 96, 71), (1, 96, 128, 72), (8, 256, 320, 73), (32, 256, 320, 74)])
def test_benchmarked_bf16_backward_against_the_oracle_at_the_bf16_noise_level(B, H, W, seed):
    from coivo_amd import _lib, nn as hnn
    from oracle import colvo_spec as S
    b = synth.make_batch(B, H, W, seed=seed)
    d = to_dev(b)
    dn_o, pn_o = S.make_models(seed)
    dn, pn = hnn.DepthNet(compute_dtype=torch.bfloat16), hnn.PoseNet(compute_dtype=torch.bfloat16)
    dn.load_state_dict(bf16_rounded_state(dn_o))
    pn.load_state_dict(bf16_rounded_state(pn_o))
    dn.deterministic = pn.deterministic = False            # the default form (float atomics), whatever COLVO_DETERMINISTIC says
    dn.zero_grad(); pn.zero_grad()
    _lib.form_counts(reset=True)
    loss, d_t, d_r, pose, a, bb = hnn.dcdp_forward(dn, pn, d["tgt"], d["ref"], d["K"])     # the fast path of bench.py
    loss.backward()
    dn.join_side(); pn.join_side()
    torch.cuda.synchronize()
    forms = _lib.form_counts()
    print(f"kernel forms of this step: {forms}")
    # what the dispatchers chose (include/colvo.h colvo_form_counts): production thresholds, nothing lowered for the test
    assert forms["wgrad_rt"] == 0
    if B >= 8:
        assert forms["wgrad_up2"] == 5                     # DepthNet's five up-sampled layers: the four-class form
    if B == 8:              # configs[1]: every weight-gradient grid halved (26 launches), the four single-split layers store behind zero_grad()
        assert forms["conv_rt"] == 0 and forms["wgrad_halved_grid"] == 26 and forms["wgrad_full_grid"] == 0, forms
        assert forms["wgrad_store_clean"] == 4 and forms["conv_res_s2"] >= 1, forms
    if B == 32:             # configs[3] per GPU: the register-tiled kernel on seven launches, ten full weight-gradient grids beside sixteen halved
        assert forms["conv_rt"] >= 7 and forms["wgrad_full_grid"] >= 10 and forms["wgrad_halved_grid"] >= 1, forms
    # this IS the benchmarked backward: the fused full-resolution kernel in its HEAD form and recorded forks
    bwd = [pr for which, (pr, _) in next(iter(dn._insts.values()))[-1].passes.items() if which.startswith("bwd")]
    assert len(bwd) == 1
    ops_recorded = [bwd[0]._arr[i].op for i in range(len(bwd[0]))]
    assert _lib.CMD_CONV_BWD_FUSED in ops_recorded and _lib.CMD_FORK in ops_recorded, ops_recorded
    assert _lib.tune_get("fork_stop_event") == 1

    masks = hip_relu_masks(dn, pn)
    o = oracle_step_bf16(seed, b, masks)                   # the target: fp32 oracle, bf16-rounded weights, HIP's ReLU decisions
    e = oracle_step_bf16(seed, b, masks, emulate=True)     # ... with the bf16 storage points emulated: the noise scale
    hip = [("depth." + n, p.grad) for n, p in dn.named_parameters()] + [("pose." + n, p.grad) for n, p in pn.named_parameters()]
    # One emulated run is ONE realisation of the noise.  PoseNet's tensors all carry the error of the same eight numbers (d pose,
    # d a, d b: sums over the image in which a handful of validity flips at the border weigh in), so their distance is one shared
    # random factor -- seen at B=1 96x128: 2.3-3.2e-2 on every PoseNet tensor against 0.5-0.8e-2 in the emulated run and 1.2-2e-2
    # on DepthNet's tensors of both.  The scale is therefore the tensor's own emulated distance or the step's typical one (the
    # median over all 58 tensors), whichever is larger.
    rows = [(n, _rel(gh.detach().float().cpu(), go), _rel(ge, go)) for (n, gh), (_, go), (_, ge) in zip(hip, o["grads"], e["grads"])]
    typical = sorted(le for _, _, le in rows)[len(rows) // 2]
    bad, worst = [], 0.0
    for n, lh, le in rows:
        scale = max(le, typical)
        worst = max(worst, lh / scale)
        if lh > K_NOISE * scale:
            bad.append(f"{n}: relL2 hip {lh:.3e} vs emulated bf16 data path {le:.3e} (typical {typical:.3e})")
    print(f"bf16 backward vs oracle: worst hip / noise ratio {worst:.2f} over {len(hip)} tensors")
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if os.path.isdir(os.path.join(root, "gpurun_out")):
        with open(os.path.join(root, "gpurun_out", f"bf16_step_parity_b{B}_{H}x{W}.txt"), "w") as f:
            f.write("param relL2_hip_vs_oracle relL2_emulated_bf16_vs_oracle\n")
            for (n, gh), (_, go), (_, ge) in zip(hip, o["grads"], e["grads"]):
                f.write(f"{n} {_rel(gh.detach().float().cpu(), go):.3e} {_rel(ge, go):.3e}\n")
            f.write(f"loss hip {loss.item():.7f} oracle {o['loss']:.7f} emulated {e['loss']:.7f}\n")
    assert len(hip) == 58 and not bad, "\n".join(bad)
    # forward quantities on the same scale
    # (the loss is ONE number: the emulated run's distance is one draw of a zero-mean quantity and can be anything down to nothing --
    #  4.8e-7 at 32 pairs, where HIP's is 1.7e-5 with all 58 gradient tensors inside their bars -- so the floor is absolute: 5e-5, a sixth
    #  of the bf16 loss bar of tests/test_config1_gpu.py)
    dl_h, dl_e = abs(loss.item() - o["loss"]), abs(e["loss"] - o["loss"])
    assert dl_h <= K_NOISE * dl_e + 5e-5, (loss.item(), o["loss"], e["loss"])
    for th, key in ((d_t, "d_t"), (d_r, "d_r")):
        eh = (th.detach().cpu() - o[key]).abs().mean().item()
        ee = (e[key] - o[key]).abs().mean().item()
        assert eh <= K_NOISE * ee, (key, eh, ee)
