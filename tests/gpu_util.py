"""Helpers shared by the -m gpu parity tests."""
import contextlib
import time

import numpy as np
import torch


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def to_dev(d, keys=None):
    return {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in d.items() if keys is None or k in keys}


def assert_close_frac(got, ref, rtol, atol_scale, max_bad_frac, what=""):
    """Element-wise closeness that tolerates a tiny fraction of outliers (pixels whose hard validity
    mask flips under 1-ulp differences of sin/cos between host libm and the GPU)."""
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    atol = atol_scale * max(ref.abs().max().item(), 1e-30)
    bad = (got - ref).abs() > (atol + rtol * ref.abs())
    frac = bad.double().mean().item()
    assert frac <= max_bad_frac, f"{what}: {frac:.3e} of elements differ (allowed {max_bad_frac:.1e}); " \
                                 f"max abs err {(got - ref).abs().max().item():.3e}, atol {atol:.3e}"


def load_npz(path):
    g = np.load(path)
    return {k: torch.from_numpy(np.asarray(g[k])) for k in g.files}


def grad_parity_table(named_hip, named_o32, named_o64, out_path=None, named_o32_other=None):
    """Per-parameter gradient errors of the HIP path and of the fp32 oracle, both measured against the fp64 oracle
    (the yardstick: fp32 summation order alone moves these heavily cancelling sums by up to a few 1e-3 of their largest
    element).  Returns rows (name, n, scale = max|g64|, err_hip = max|hip-g64|, err_o32 = max|o32-g64|,
    l2_hip = |hip-g64|_2 / |g64|_2, l2_o32).  named_o32_other: a second evaluation of the fp32 oracle (another device);
    err_o32 and l2_o32 are then the SMALLER of the two, tensor by tensor."""
    rows = []
    for i, ((n, gh), (_, g32), (_, g64)) in enumerate(zip(named_hip, named_o32, named_o64)):
        gh = gh.detach().cpu().double()
        g64 = g64.detach().cpu().double()
        scale = max(g64.abs().max().item(), 1e-30)
        nrm = max(g64.norm().item(), 1e-30)
        o32s = [g32] if named_o32_other is None else [g32, named_o32_other[i][1]]
        o32s = [g.detach().cpu().double() for g in o32s]
        rows.append((n, gh.numel(), scale, (gh - g64).abs().max().item(), min((g - g64).abs().max().item() for g in o32s),
                     (gh - g64).norm().item() / nrm, min((g - g64).norm().item() / nrm for g in o32s)))
    if out_path is not None:
        try:
            with open(out_path, "w") as f:
                f.write("param n scale max_err_hip/scale max_err_o32/scale relL2_hip relL2_o32\n")
                for r in rows:
                    f.write(f"{r[0]} {r[1]} {r[2]:.4e} {r[3] / r[2]:.3e} {r[4] / r[2]:.3e} {r[5]:.3e} {r[6]:.3e}\n")
        except OSError:
            pass
    return rows


# SPEC.md §7: the yardstick for a parameter gradient is the fp64 evaluation of the spec.  These are heavily cancelling
# sums, so the fp32 ORACLE itself sits some way from it -- 2e-6 (relative L2) at B=2 64x96, 5e-4 at B=8 256x320, 2e-3 at
# B=1 256x320 -- and that distance, measured in the same step, is the only scale the bar uses: there is NO absolute floor.
# A gradient tensor passes when
#   * its relative L2 error is at most GRAD_K x the fp32 oracle's on the same tensor, or at most the fp32 oracle's own
#     worst tensor of this step; and
#   * its largest element error (relative to the tensor's largest element) is at most GRAD_K x the fp32 oracle's on the same
#     tensor, or at most GRAD_MAX_SLACK x the fp32 oracle's worst tensor of this step (the maximum over up to 2.4 M elements
#     is an extreme-value statistic: two fp32 summation orders differ by more in it than in the L2 norm).
# Round-3 tables of the final round-2 build (gpurun_out/grad_parity_*.txt): HIP / fp32-oracle worst tensors 2.1e-6 / 1.6e-6
# (B=2 64x96), 7.8e-4 / 4.9e-4 (configs[1]), 2.0e-3 / 1.9e-3 (B=1 256x320); a gradient 3x worse than the oracle's own
# rounding noise fails at every shape.
# Tensors of at most GRAD_TINY elements (the heads' biases: 1, 8, 16 values): their L2 norm is a small-sample statistic like
# the maximum -- for the depth head's ONE bias value the two are the same number -- so the maximum's slack applies to it too
# (seen: that scalar at 1.73e-6 against 3 x 5.7e-7 = 1.72e-6 and a worst oracle tensor of 1.61e-6 in one run of several; it is
# summed with float atomics and moves in the last digits from run to run).
GRAD_K, GRAD_MAX_SLACK, GRAD_TINY = 3.0, 2.0, 16


def grad_parity_failures(rows):
    worst_l2 = max(r[6] for r in rows)
    worst_max = max(r[4] / r[2] for r in rows)
    bad = []
    for name, n, scale, eh, eo, lh, lo in rows:
        l2_bar = max(GRAD_K * lo, (GRAD_MAX_SLACK if n <= GRAD_TINY else 1.0) * worst_l2)
        if lh > l2_bar or eh > max(GRAD_K * eo, GRAD_MAX_SLACK * worst_max * scale):
            bad.append(f"{name}: relL2 hip {lh:.3e} vs o32 {lo:.3e} (worst o32 {worst_l2:.3e}); max err/scale hip "
                       f"{eh / scale:.3e} vs o32 {eo / scale:.3e} (worst o32 {worst_max:.3e})")
    return bad


# ---------------------------------------------------------------------------------------------------------------------- #
# Matched ReLU decisions.                                                                                                  #
# A ReLU whose pre-activation lies within rounding distance of zero is decided by the summation order: the HIP kernels and  #
# torch's CPU conv (and the fp32 and fp64 oracle between themselves) may disagree on it, and ONE such element moves every    #
# upstream parameter gradient by ~1e-3 at B=2 64x96 -- a thousand times the rounding noise of everything else (round 3:      #
# tests/golden/net_b2_64x96, pre-activation 4.5e-7 in `up1`; profiles/r3_relu_flip.md).  At 256x320 there are hundreds of    #
# them, which is what the fp32 oracle's own 5e-4 ... 2e-3 distance from its fp64 evaluation consists of.  Gradient parity    #
# is therefore judged against oracles whose ReLU decisions are FORCED to the HIP path's wherever they differ -- allowed only #
# where the oracle's own pre-activation is below RELU_MARGIN in magnitude, anything larger is a genuine forward mismatch     #
# and fails.  With the decisions matched all three evaluations differ by rounding only.                                      #
# ---------------------------------------------------------------------------------------------------------------------- #
RELU_MARGIN = 1e-5


def hip_relu_masks(dn, pn, device=None):
    """{'depth.enc1a': bool [2B,C,h,w], ..., 'pose.conv7': ...}: which activations of the LAST recorded forward of the two
    HIP networks are positive (read from the persistent activation buffers of the recorded passes: call right after the step).
    On the CPU unless `device` is given: at 128 frames the masks are gigabytes, and an oracle that runs on the GPU wants them there."""
    masks = {}
    for tag, net in (("depth", dn), ("pose", pn)):
        pools = [p for p in net._insts.values() if p]
        assert len(pools) == 1 and pools[0], "expected exactly one recorded shape (and COLVO_NO_PROGRAM unset)"
        A = pools[0][-1].passes["fwd"][1]
        for k, t in A.items():
            if k == "in":
                continue
            name = k if isinstance(k, str) else f"conv{k}"
            m = t.float().permute(0, 3, 1, 2) > 0
            masks[f"{tag}.{name}"] = m.cpu() if device is None else m.to(device)
    return masks


# ---------------------------------------------------------------------------------------------------------------------- #
# The oracle step on a device, in slices of pairs.                                                                         #
# One float64 step of ONE 512x640 pair takes 12 s on 16 CPU threads, so on the CPU the step-level bars stop at 8 pairs of   #
# 256x320 (fp32) / 32 pairs (bf16).  oracle/colvo_spec.py creates every tensor on its inputs' device; with `device` the      #
# oracle runs there, and with `slice_pairs` it runs k pairs at a time so that its autograd graph stays small: the loss is a  #
# masked mean over the BATCH, so a first sweep without gradients adds up the batch's valid-pixel count and a second one      #
# backpropagates  sum(map * valid) / max(3 n_batch, 1)  slice by slice -- parameter gradients accumulate, the loss is the    #
# sum of the slice terms.  tests/test_step_ref_cpu.py holds sliced == whole to 1e-12 in float64.                             #
# On the GPU the convolutions run with MIOpen switched off (torch's own im2col + GEMM, which exists in float64 too): the     #
# fp32 oracle is the NOISE YARDSTICK of grad_parity_failures, and a reduced-accuracy convolution algorithm would make it a   #
# looser one than the CPU oracle is.                                                                                         #
# ---------------------------------------------------------------------------------------------------------------------- #
class _Rows:
    """What the oracle networks are looking at right now: pairs [s, s+k) of B (DepthNet: frames s.. and B+s..).  The forward
    hooks are registered once and read the current slice from here."""

    def __init__(self):
        self.B = self.s = self.k = None          # None: the whole batch
        self.count = True                        # False during the valid-pixel sweep: forced decisions are counted once

    def of(self, m, tag):
        if self.B is None:
            return m
        s, k, B = self.s, self.k, self.B
        return torch.cat([m[s:s + k], m[B + s:B + s + k]]) if tag == "depth" else m[s:s + k]


def _forced(out, m, flip):
    """`out` with the sign of the elements `flip` turned to the decision `m`.  -o has the other sign (exactly); an exact zero becomes
    +-1e-30.  Added as a CONSTANT: the gradient still flows through the element, the ReLU behind it now takes the HIP path's decision."""
    o = out.detach()
    delta = torch.where(o == 0, torch.where(m, torch.full_like(o, 1e-30), torch.full_like(o, -1e-30)), -2 * o)
    return out + torch.where(flip, delta, torch.zeros_like(o))


@contextlib.contextmanager
def _plain_convs(device):
    """On a GPU: MIOpen off, no TF32-style shortcut in the GEMMs behind torch's own convolution."""
    if device is None or torch.device(device).type != "cuda":
        yield
        return
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        with torch.backends.cudnn.flags(enabled=False, allow_tf32=False):
            yield
    finally:
        torch.backends.cuda.matmul.allow_tf32 = old


def _coupled_step(dn, pn, tgt, ref, K, rows, slice_pairs, full_loss, normaliser=None):
    """S.dcdp_forward + backward, whole or in slices of `slice_pairs` pairs.  -> (loss, d_t, d_r, pose, a, b), detached.
    normaliser: only tests/test_step_ref_cpu.py passes one, to plant a wrong one -- it maps (the slices' valid-pixel counts,
    slice index) to the count a slice divides by; the right one is the batch's sum for every slice."""
    from oracle import colvo_spec as S
    B = tgt.shape[0]
    if slice_pairs is None or slice_pairs >= B:
        loss, *outs = S.dcdp_forward(dn, pn, tgt, ref, K, full_loss=full_loss)
        loss.backward()
        return (loss.item(), *[o.detach() for o in outs])
    if full_loss:
        raise ValueError("the widened objective's terms normalise over the batch each in its own way: full_loss runs unsliced only")
    assert slice_pairs >= 1

    def forward(s):
        rows.B, rows.s, rows.k = B, s, min(slice_pairs, B - s)
        sl = slice(s, s + rows.k)
        d = dn(torch.cat([tgt[sl], ref[sl]], dim=0))
        d_t, d_r = d[:rows.k], d[rows.k:]
        pose, a, b = pn(tgt[sl], ref[sl], d_t, d_r)
        m, valid = S.photometric_loss_map(tgt[sl], ref[sl], d_t, pose, K[sl], a, b)
        return m, valid, (d_t, d_r, pose, a, b)

    try:
        rows.count = False
        with torch.no_grad():
            counts = [int(forward(s)[1].sum().item()) for s in range(0, B, slice_pairs)]
        rows.count = True
        loss, outs = 0.0, []
        for i, s in enumerate(range(0, B, slice_pairs)):
            m, valid, o = forward(s)
            n_batch = sum(counts) if normaliser is None else normaliser(counts, i)
            term = (m * valid).sum() / max(m.shape[1] * n_batch, 1)
            term.backward()
            loss += term.item()
            outs.append([x.detach() for x in o])
    finally:
        rows.B = rows.s = rows.k = None
        rows.count = True
    return (loss, *[torch.cat(x) for x in zip(*outs)])


def _named_grads(dn, pn):
    return [("depth." + n, p.grad.cpu()) for n, p in dn.named_parameters()] + [("pose." + n, p.grad.cpu()) for n, p in pn.named_parameters()]


def oracle_step(seed, batch, dtype=torch.float32, masks=None, weights_seed=None, device=None, slice_pairs=None, full_loss=False):
    """The oracle's coupled step (spec init `weights_seed`, default = seed) in `dtype`; with `masks` the ReLU decisions are
    forced to them.  device: where it runs (default: the CPU; the results come back to the CPU either way); slice_pairs: evaluated
    that many pairs at a time (see above); full_loss: the widened objective, unsliced only.
    -> dict(loss, d_t, d_r, pose, a, b, grads [(name, tensor)], flips, flip_worst)."""
    from oracle import colvo_spec as S
    dn, pn = S.make_models(seed if weights_seed is None else weights_seed, dtype=dtype)
    if device is not None:
        dn, pn = dn.to(device), pn.to(device)
    stats = {"flips": 0, "worst": 0.0}
    rows = _Rows()
    if masks is not None:
        for tag, net in (("depth", dn), ("pose", pn)):
            for name, mod in net.named_children():
                m = masks.get(f"{tag}.{name}")
                if m is None:
                    continue

                def hook(mod, inp, out, m=m, tag=tag):
                    m = rows.of(m, tag).to(out.device)
                    flip = (out > 0) != m
                    n = int(flip.sum())
                    if not n:
                        return None
                    if rows.count:
                        stats["flips"] += n
                        stats["worst"] = max(stats["worst"], out[flip].abs().max().item())
                    return _forced(out, m, flip)
                mod.register_forward_hook(hook)
    t = lambda v: v.to(device=device, dtype=dtype)
    with _plain_convs(device):
        loss, d_t, d_r, pose, a, b = _coupled_step(dn, pn, t(batch["tgt"]), t(batch["ref"]), t(batch["K"]), rows, slice_pairs, full_loss)
    return dict(loss=loss, d_t=d_t.cpu(), d_r=d_r.cpu(), pose=pose.cpu(), a=a.cpu(), b=b.cpu(),
                grads=_named_grads(dn, pn), flips=stats["flips"], flip_worst=stats["worst"])


def oracle_networks(seed, frames, dtype=torch.float32, device=None, bf16_weights=False, emulate=False):
    """The oracle's two networks forward only, on the frames [N+1,3,H,W] of one sequence, whole (no chunks, no slices): DepthNet on
    every frame, PoseNet on every consecutive pair with the depths this very run made (in float64: the float64 depths) -- what
    inference.run_networks computes.  dtype: the oracle's arithmetic; device: where it runs (on a GPU with MIOpen off, as in
    oracle_step); bf16_weights: the spec weights rounded to bf16 (bf16_rounded_state), the target of bf16 mode; emulate: the HIP
    networks' bf16 storage points inserted (_bf16_hooks), the noise scale of bf16 mode.
    -> (depths [N+1,1,H,W], rel_poses [N,6]) in `dtype` on the CPU."""
    from oracle import colvo_spec as S
    dn, pn = S.make_models(seed, dtype=dtype)
    if bf16_weights:
        dn.load_state_dict(bf16_rounded_state(dn))
        pn.load_state_dict(bf16_rounded_state(pn))
    if device is not None:
        dn, pn = dn.to(device), pn.to(device)
    if emulate:
        _bf16_hooks(dn, pn, None, True, _Rows())
    f = frames.to(device=device, dtype=dtype)
    with torch.no_grad(), _plain_convs(device):
        d = dn(f)
        pose, _, _ = pn(f[:-1], f[1:], d[:-1], d[1:])
    return d.cpu(), pose.cpu()


def _timed(timings, key, fn):
    if timings is None:
        return fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    timings[key] = time.perf_counter() - t0
    return out


def matched_grad_rows(seed, batch, dn, pn, out_path=None, weights_seed=None, device=None, slice_pairs=None, full_loss=False, timings=None,
                      cpu_yardstick=False):
    """Gradient parity rows (grad_parity_table) of the HIP networks' current .grad against the fp32 / fp64 oracle evaluated at
    the HIP path's ReLU decisions (device, slice_pairs, full_loss: as in oracle_step).  Asserts that decisions were only ever
    forced at marginal pre-activations.  timings: a dict that receives the seconds of 'masks', 'o32', 'o64' (and 'c32').
    cpu_yardstick (with a device): the fp32 oracle runs on the CPU as well, and the noise scale of a tensor is the smaller of the
    two fp32 oracles' distances from fp64 -- the device's fp32 oracle never makes the bar looser than the CPU's would."""
    masks = _timed(timings, "masks", lambda: hip_relu_masks(dn, pn, device))
    o32 = _timed(timings, "o32", lambda: oracle_step(seed, batch, torch.float32, masks, weights_seed, device, slice_pairs, full_loss))
    o64 = _timed(timings, "o64", lambda: oracle_step(seed, batch, torch.float64, masks, weights_seed, device, slice_pairs, full_loss))
    c32 = None
    if cpu_yardstick and device is not None:
        masks_c = _timed(timings, "masks_cpu", lambda: {k: v.cpu() for k, v in masks.items()})
        c32 = _timed(timings, "c32", lambda: oracle_step(seed, batch, torch.float32, masks_c, weights_seed, None, slice_pairs, full_loss))
        del masks_c
    for tag, o in (("fp32", o32), ("fp64", o64)) + ((("CPU fp32", c32),) if c32 is not None else ()):
        assert o["flip_worst"] < RELU_MARGIN, \
            f"a HIP activation has the other sign than the {tag} oracle's pre-activation of magnitude {o['flip_worst']:.3e}: " \
            f"not a rounding-distance ReLU decision but a forward mismatch"
    print(f"matched ReLU decisions: {o32['flips']} forced in the fp32 oracle (largest |pre| {o32['flip_worst']:.2e}), "
          f"{o64['flips']} in the fp64 oracle ({o64['flip_worst']:.2e})")
    hip = [("depth." + n, p.grad) for n, p in dn.named_parameters()] + [("pose." + n, p.grad) for n, p in pn.named_parameters()]
    if c32 is not None:
        far = lambda o: max((g.double() - t).norm().item() / max(t.norm().item(), 1e-30) for (_, g), (_, t) in zip(o["grads"], o64["grads"]))
        print(f"fp32 yardstick, worst tensor's relL2 from fp64: on the device {far(o32):.3e}, on the CPU {far(c32):.3e} "
              f"({c32['flips']} decisions forced there, largest |pre| {c32['flip_worst']:.2e})")
    return grad_parity_table(hip, o32["grads"], o64["grads"], out_path, None if c32 is None else c32["grads"]), o32, o64


# ---------------------------------------------------------------------------------------------------------------------- #
# bf16 mode against the oracle.                                                                        #
# What the HIP networks do differently in bf16 mode: weights are rounded to bf16 (operand copies), every conv layer's output #
# is STORED in bf16 (its accumulation is fp32), so is every layer's input gradient, and the packed network inputs; heads,    #
# loss and weight-gradient accumulation stay fp32.  `oracle_step_bf16` evaluates the fp32 oracle on bf16-rounded weights --  #
# the target -- and, with emulate=True, with exactly those roundings inserted: the distance between the two is the size of    #
# the bf16 data path's own noise, measured in the same step on the same inputs, and the bar for the HIP gradients is a       #
# multiple of it (no constant that has to be re-tuned per shape).                                                            #
# ---------------------------------------------------------------------------------------------------------------------- #
class _RoundBf16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def bf16_rounded_state(module):
    return {k: v.to(torch.bfloat16).to(v.dtype) for k, v in module.state_dict().items()}


def _bf16_hooks(dn, pn, masks, emulate, rows):
    """Forward hooks on the oracle networks for bf16 mode: with `emulate` every conv layer's output (not the fp32 heads') and the first
    layer's input are rounded to bf16 -- the storage points of the HIP networks; with `masks` the ReLU decisions are forced to them
    (rows: which rows of the masks the networks are looking at).  Shared by the step (oracle_step_bf16) and the forward-only run
    (oracle_networks)."""
    for tag, net, first, fp32_layers in (("depth", dn, "enc1a", ("head",)), ("pose", pn, "conv1", ("pred",))):
        for name, mod in net.named_children():
            if name in fp32_layers:
                continue
            m = None if masks is None else masks.get(f"{tag}.{name}")

            def hook(mod, inp, out, m=m, tag=tag):
                if emulate:
                    out = _RoundBf16.apply(out)           # (commutes with the ReLU behind it)
                if m is None:
                    return out
                m = rows.of(m, tag).to(out.device)
                flip = (out > 0) != m
                if not bool(flip.any()):
                    return out
                return _forced(out, m, flip)
            mod.register_forward_hook(hook)
            if emulate and name == first:
                mod.register_forward_pre_hook(lambda mod, inp: (_RoundBf16.apply(inp[0]),))


def oracle_step_bf16(seed, batch, masks=None, emulate=False, weights_seed=None, device=None, slice_pairs=None):
    """The fp32 oracle's coupled step on bf16-ROUNDED weights; ReLU decisions forced to `masks` (hip_relu_masks) where given;
    emulate: the bf16 storage points of the HIP networks inserted (see above); device, slice_pairs: as in oracle_step.
    -> dict(loss, d_t, d_r, grads [(name, tensor)])."""
    from oracle import colvo_spec as S
    dn, pn = S.make_models(seed if weights_seed is None else weights_seed)
    dn.load_state_dict(bf16_rounded_state(dn))
    pn.load_state_dict(bf16_rounded_state(pn))
    if device is not None:
        dn, pn = dn.to(device), pn.to(device)
    rows = _Rows()
    _bf16_hooks(dn, pn, masks, emulate, rows)
    t = lambda v: v.to(device=device)
    with _plain_convs(device):
        loss, d_t, d_r, pose, a, b = _coupled_step(dn, pn, t(batch["tgt"]), t(batch["ref"]), t(batch["K"]), rows, slice_pairs, False)
    return dict(loss=loss, d_t=d_t.cpu(), d_r=d_r.cpu(), pose=pose.cpu(), grads=_named_grads(dn, pn))


K_NOISE = 3.0


def _rel(a, b):
    return (a - b).norm().item() / max(b.norm().item(), 1e-30)


def bf16_hip_step(B, H, W, seed):
    """One step of the BENCHMARKED form -- bf16 networks on bf16-rounded spec weights, float atomics, the fast path of bench.py --
    on synth.make_batch(B, H, W, seed).  -> dict(batch, dn, pn, loss, d_t, d_r, forms, ops_recorded, seconds)."""
    from coivo_amd import _lib, nn as hnn, synth
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
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss, d_t, d_r, pose, a, bb = hnn.dcdp_forward(dn, pn, d["tgt"], d["ref"], d["K"])     # the fast path of bench.py
    loss.backward()
    dn.join_side(); pn.join_side()
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    forms = _lib.form_counts()
    print(f"kernel forms of this step: {forms}")
    # this IS the benchmarked backward: the fused full-resolution kernel in its HEAD form and recorded forks
    bwd = [pr for which, (pr, _) in next(iter(dn._insts.values()))[-1].passes.items() if which.startswith("bwd")]
    assert len(bwd) == 1
    ops_recorded = [bwd[0]._arr[i].op for i in range(len(bwd[0]))]
    return dict(batch=b, dn=dn, pn=pn, loss=loss, d_t=d_t, d_r=d_r, forms=forms, ops_recorded=ops_recorded, seconds=seconds)


def assert_bf16_step_at_the_noise_level(step, seed, device=None, slice_pairs=None, timings=None, table=None):
    """Every parameter gradient of bf16_hip_step's step against the fp32 oracle on the same bf16-rounded weights at the HIP path's
    ReLU decisions; the bar is K_NOISE x the distance of the oracle with the bf16 storage points emulated from that target
    (oracle_step_bf16).  device, slice_pairs: where and how the two oracle steps run (default: the CPU, whole); table: an open
    text file that receives the per-tensor figures before anything is asserted."""
    b, dn, pn, loss = step["batch"], step["dn"], step["pn"], step["loss"]
    B, _, H, W = b["tgt"].shape
    masks = _timed(timings, "masks", lambda: hip_relu_masks(dn, pn, device))
    # the target: fp32 oracle, bf16-rounded weights, HIP's ReLU decisions
    o = _timed(timings, "target", lambda: oracle_step_bf16(seed, b, masks, device=device, slice_pairs=slice_pairs))
    # ... with the bf16 storage points emulated: the noise scale
    e = _timed(timings, "emulated", lambda: oracle_step_bf16(seed, b, masks, emulate=True, device=device, slice_pairs=slice_pairs))
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
    if table is not None:
        table.write("param relL2_hip_vs_oracle relL2_emulated_bf16_vs_oracle\n")
        for n, lh, le in rows:
            table.write(f"{n} {lh:.3e} {le:.3e}\n")
        table.write(f"loss hip {loss.item():.7f} oracle {o['loss']:.7f} emulated {e['loss']:.7f}\n")
        table.flush()
    assert len(hip) == 58 and not bad, "\n".join(bad)
    # forward quantities on the same scale
    # (the loss is ONE number: the emulated run's distance is one draw of a zero-mean quantity and can be anything down to nothing --
    #  4.8e-7 at 32 pairs, where HIP's is 1.7e-5 with all 58 gradient tensors inside their bars -- so the floor is absolute: 5e-5, a sixth
    #  of the bf16 loss bar of tests/test_config1_gpu.py)
    dl_h, dl_e = abs(loss.item() - o["loss"]), abs(e["loss"] - o["loss"])
    print(f"bf16 forward vs oracle: loss {dl_h:.2e} (emulated {dl_e:.2e})")
    assert dl_h <= K_NOISE * dl_e + 5e-5, (loss.item(), o["loss"], e["loss"])
    for key in ("d_t", "d_r"):
        eh = (step[key].detach().cpu() - o[key]).abs().mean().item()
        ee = (e[key] - o[key]).abs().mean().item()
        assert eh <= K_NOISE * ee, (key, eh, ee)
    return worst
