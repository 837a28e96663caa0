"""Exact-data checks of the depth and pose heads (the conv_exact.py approach: small integers times power-of-two quanta), with float64
references in plain torch and, where a head is not exact (sigmoid, reciprocal, the rebuilt sigmoid of d(pre), 1 / HW), an error bound
derived from the kernel's sequence of fp32 operations.  Nothing here calls the library: the tests hand these functions what the
kernels wrote.

Value sets (quanta):
    head input y        multiples of QY = 2^-6 (a 16 -> 16 layer's output under conv_exact's sets), drawn from [-y_max, y_max]
                        clamped at 0 and rounded once to bf16; y_max = Y_FWD = conv_exact.bound_fwd(16) for the forward, X_MAX = 3
                        for the gradients (so that d(pre) can be dense enough to cover every pixel range)
    head weights        [-8, 8] * QH, QH = 2^-8 (op level: |pre| of a few units on the full-range y) or 2^-4 behind the fused
                        layer (whose output is small); exact in bf16, so the fused kernel's hi / lo split leaves lo = 0
    head bias           [-2^14, 2^14] * QY * QH (|bias| <= 1/4 ... 4)
    d(pre), given       {-2, -1, 1, 2} * 2^-3 (conv_exact.make_dy): exact in bf16, so the MFMA forms' rounding loses nothing
    d depth             {-4 .. 4} * 2^-4
Exact bounds (sums of |terms| in quanta, below 2^22 = conv_exact.BOUND, so every order of fp32 summation is exact):
    bound_pre           9 * C * y_max * 8 + 2^14 (C = 16; the generic kernels' checks use C = 8)
    head weight grad.   X_MAX * 2 * (non-zero d(pre)) -- conv_exact.bound_wgrad at conv_exact.dy_density(B * H * W)
    HEAD-form gradient  g = (y > 0) * (d(pre) (*) head weights) <= 9 * 2 * 8 = 144 quanta of 2^-3 * QH: exact in bf16 (8 bits)
    ... through the layer  its weight gradient sums X_MAX * 8 * 9 * 2 per non-zero d(pre) (head_g_density keeps it below the bound)
Rounding bounds (U = 2^-24; the kernels' formulas are csrc/heads.hip k_depth_head_fwd* / head_dpre / k_depth_head_dgrad* /
k_pose_head_*, csrc/fwd16.hip's epilogue): see depth_rel_bound, dpre_bound, dgrad_bound, pose_ref, pose_bwd_bounds."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import conv_exact as CX

U, U_BF = 2.0 ** -24, 2.0 ** -8          # unit roundoff of fp32 (24-bit significand), bf16 (8-bit)
EXP_ULPS = 3                             # expf: the OpenCL full-profile bound (3 ulp, i.e. a relative 6 U)
QY = 2.0 ** -6
Y_FWD = CX.bound_fwd(16)                 # 3472: the largest 16 -> 16 layer output, in QY
QH_OP, QH_FUSED, H_MAX = 2.0 ** -8, 2.0 ** -4, 8
HB_MAX = 2 ** 14
QDD, DD_MAX = 2.0 ** -4, 4
SAT_PRE = 17.0                           # beyond this 1 / (1 + exp(-pre)) rounds to 1 in fp32: the sigmoid is saturated

_f32 = np.float32
LO = float(_f32(1.0) / _f32(10.0))                      # ops.MAX_DEPTH -> the kernels' lo = 1 / max_depth, hi = 1 / min_depth (fp32)
HI = float(_f32(1.0) / _f32(0.1))
K = HI - LO                                             # exact in float64; the kernels round it to fp32 (one more U)
POSE_S, LCC_S = float(_f32(0.01)), float(_f32(0.1))     # ops.POSE_SCALE, LCC_SCALE as the kernels receive them


def gamma(n):
    return n * U / (1 - n * U)


def bound_pre(y_max: int, C: int = 16) -> int:
    """Pre-activation of the depth head, quanta of QY * QH: 9 taps x C channels and the bias."""
    return 9 * C * y_max * H_MAX + HB_MAX


def head_g_bound() -> int:
    """The HEAD form's gradient g = (y > 0) * sum_t head_w[t][c] d(pre)[p + 1 - t], quanta of 2^-3 * QH."""
    return 9 * CX.DY_MAX * H_MAX


def head_g_density(npix: int) -> float:
    """Density of the non-zero d(pre) of a HEAD-form check: every non-zero d(pre) reaches 9 pixels of g, each at most H_MAX * DY_MAX
    quanta, and the layer's weight gradient multiplies g by X_MAX -- the expected sum stays at 3 / 4 of conv_exact.BOUND."""
    return min(CX.RHO_MAX, CX.BOUND / (CX.X_MAX * 9 * H_MAX * CX.DY_MAX * npix) * 0.75)


def bound_head_g_wgrad(npix: int) -> float:
    """Worst sum of |terms| of the layer's weight gradient in the HEAD form (quanta of conv_exact.QX * 2^-3 * QH): six standard
    deviations above the mean count of non-zero d(pre)."""
    rho = head_g_density(npix)
    n = rho * npix + 6.0 * math.sqrt(rho * (1 - rho) * npix) + 1
    return CX.X_MAX * 9 * H_MAX * CX.DY_MAX * n


# ------------------------------------------------------------------------------------------------------------------------------- #
# operands                                                                                                                        #
# ------------------------------------------------------------------------------------------------------------------------------- #
def make_y(shape, y_max, g, device):
    """[B, H, W, C] fp32 holding bf16 values: multiples of QY in [0, y_max], about half of them zero, rounded once to bf16."""
    v = CX._ints(-y_max, y_max, shape, g, device).clamp_(min=0) * QY
    return v.bfloat16().float()


def make_head_w(C, g, device, q=QH_OP):
    return CX._ints(-H_MAX, H_MAX, (1, 9, C), g, device) * q


def make_head_w_saturating(C, g, device, y_max=Y_FWD):
    """make_head_w, drawn again until saturate()'s patches reach |pre| > SAT_PRE + 4 (|bias| <= 4) in both directions."""
    for _ in range(1000):
        w = make_head_w(C, g, device)
        ws = w.view(9, C).sum(0) * (y_max * QY)
        if min(float(ws.clamp(min=0).sum()), float((-ws).clamp(min=0).sum())) > SAT_PRE + 4:
            return w
    raise AssertionError("no saturating head weights drawn")


def make_head_b(g, device, q=QH_OP):
    return CX._ints(-HB_MAX, HB_MAX, (1,), g, device) * (QY * q)


def saturate(y, w, g, n_patches, y_max=Y_FWD):
    """Push some pixels into saturation on purpose: n_patches 4 x 4 patches per image whose channels are y_max where the head's
    weights summed over the taps are positive (pre far above SAT_PRE) or negative (far below -SAT_PRE), zero elsewhere."""
    B, H, W, C = y.shape
    ws = w.view(9, C).sum(0)
    pos, neg = (ws > 0).float() * (y_max * QY), (ws < 0).float() * (y_max * QY)
    pos, neg = pos.bfloat16().float(), neg.bfloat16().float()
    ys = torch.randint(0, max(1, H - 3), (B, n_patches), generator=g, device=y.device)
    xs = torch.randint(0, max(1, W - 3), (B, n_patches), generator=g, device=y.device)
    for b in range(B):
        for k in range(n_patches):
            y0, x0 = int(ys[b, k]), int(xs[b, k])
            y[b, y0:y0 + 4, x0:x0 + 4] = pos if k % 2 == 0 else neg
    return y


def make_d_depth(shape, g, device):
    return CX._ints(-DD_MAX, DD_MAX, shape, g, device) * QDD


# ------------------------------------------------------------------------------------------------------------------------------- #
# float64 references                                                                                                              #
# ------------------------------------------------------------------------------------------------------------------------------- #
def _w4(w):                                            # [1][9][C] -> [1][C][3][3]
    C = w.shape[-1]
    return w.double().view(1, 3, 3, C).permute(0, 3, 1, 2)


def ref_pre(y, w, b):
    """pre [B, H, W] float64 = conv3x3(y NHWC; w [1][9][C], zero padding) + b, in image slices."""
    B, H, W, C = y.shape
    out = torch.empty(B, H, W, dtype=torch.float64, device=y.device)
    for b0, b1 in CX.image_slices(B, H * W * C):
        out[b0:b1] = F.conv2d(y[b0:b1].permute(0, 3, 1, 2).double(), _w4(w), b.double(), padding=1)[:, 0]
    return out


def sig64(pre):
    return torch.sigmoid(pre), torch.sigmoid(-pre)        # sig and 1 - sig, each without cancellation


def ref_depth(pre):
    s, _ = sig64(pre)
    return 1.0 / (LO + K * s)


def ref_dpre(pre, gdd):
    """d(pre) = d_depth * d depth / d pre = -gdd * K * depth^2 * sig * (1 - sig), float64."""
    s, c = sig64(pre)
    d = 1.0 / (LO + K * s)
    return -gdd * K * d * d * s * c


def ref_head_dgrad(dpre, w, C):
    """sum_t w[t][c] dpre[p + 1 - t] (unmasked) [B, H, W, C] float64, and the same over |dpre| and |w| (the bound's sum)."""
    B, H, W = dpre.shape
    out, absum = [], []
    for b0, b1 in CX.image_slices(B, H * W * C):
        d = dpre[b0:b1, None].double()
        out.append(torch.nn.grad.conv2d_input((b1 - b0, C, H, W), _w4(w), d, padding=1).permute(0, 2, 3, 1))
        absum.append(torch.nn.grad.conv2d_input((b1 - b0, C, H, W), _w4(w).abs(), d.abs(), padding=1).permute(0, 2, 3, 1))
    return torch.cat(out), torch.cat(absum)


def ref_head_wgrad(y, dpre):
    """dw [1][9][C] = sum_p dpre[p] y[p + t - 1][c], db [1] = sum_p dpre[p], float64 (exact slices, exact sums)."""
    B, H, W, C = y.shape
    dw = torch.zeros(1, C, 3, 3, dtype=torch.float64, device=y.device)
    db = torch.zeros(1, dtype=torch.float64, device=y.device)
    for b0, b1 in CX.image_slices(B, H * W * C):
        d = dpre[b0:b1, None].double()
        dw += torch.nn.grad.conv2d_weight(y[b0:b1].permute(0, 3, 1, 2).double(), dw.shape, d, padding=1)
        db += d.sum()
    return dw.permute(0, 2, 3, 1).reshape(1, 9, C), db


# ------------------------------------------------------------------------------------------------------------------------------- #
# rounding bounds                                                                                                                 #
# ------------------------------------------------------------------------------------------------------------------------------- #
def depth_rel_bound(pre):
    """Relative error of the kernels' depth = 1 / (lo + fl(hi - lo) * sig), sig = 1 / (1 + expf(-pre)), pre exact:
        expf                      EXP_ULPS ulp = 2 EXP_ULPS U relative; through 1 / (1 + e) it is scaled by e / (1 + e) = 1 - sig
        1 + e, 1 / (1 + e)        U each                               -> sig:      2 EXP_ULPS U (1 - sig) + 2 U
        fl(hi - lo), the product  U each                               -> K sig:    + 2 U
        lo + K sig                the sum of two positives: the product's error scaled by K sig / D, plus U
        1 / D                     U
    second-order terms: a factor 1 + 1e-5."""
    s, c = sig64(pre)
    D = LO + K * s
    return ((2 * EXP_ULPS * U * c + 4 * U) * (K * s / D) + 2 * U) * (1 + 1e-5)


def dpre_bound(pre, gdd, gdd_err=None):
    """Absolute error of head_dpre(depth, g) = -g * fl(hi - lo) * depth * depth * sig' * (1 - sig'), with depth the kernels' depth
    (depth_rel_bound) and sig' = (1 / depth - lo) / fl(hi - lo) rebuilt from it:
        1 / depth                 the depth's error E_D plus U                 -> e_r = (E_D + U) D (1 + 2 E_D) absolute
        - lo                      exact operands; its rounding U of K sig + e_r
        / fl(hi - lo)             two roundings U of sig                        -> e_s absolute on sig'
        1 - sig'                  e_s plus its rounding U                       -> e_c absolute
        five products, fl(hi - lo) and depth twice: the relative gamma = (1 + U)^6 (1 + E_D)^2 - 1
    |error| <= |g| K d^2 [ s c gamma + (s e_c + c e_s + e_s e_c)(1 + gamma) ] + |error of g| K d^2 (s + e_s)(c + e_c)(1 + gamma).
    Near saturation (c -> 0 or s -> 0) the e_s terms dominate: the rebuilt sigmoid's subtraction amplifies the depth's rounding by
    D / (K sig) -- that is this bound's margin, not a tolerance."""
    s, c = sig64(pre)
    D = LO + K * s
    d = 1.0 / D
    ed = depth_rel_bound(pre)
    e_r = (ed + U) * D * (1 + 2 * ed)
    e_s = ((e_r + U * (K * s + e_r)) / K) * (1 + 3 * U) + 2 * U * s * (1 + 3 * U)
    e_c = e_s + U * (c + e_s)
    gam = (1 + U) ** 6 * (1 + ed) ** 2 - 1
    scale = K * d * d
    b = gdd.abs() * scale * (s * c * gam + (s * e_c + c * e_s + e_s * e_c) * (1 + gam))
    if gdd_err is not None:
        b = b + gdd_err * scale * (s + e_s) * (c + e_c) * (1 + gam)
    return b * (1 + 1e-6)


def dgrad_bound(absum, out_dtype):
    """k_depth_head_dgrad*: nine fp32 multiply-adds per element (gamma_9 of the sum of |terms|) and, in bf16, the one store rounding
    (half a bf16 ulp: U_BF relative) of the result."""
    b = gamma(9) * absum
    if out_dtype == torch.bfloat16:
        b = b * (1 + U_BF) + U_BF * absum
    return b


def parts_g(g0, graw, sa, sb):
    """k_depth_head_dpre_parts' incoming gradient g = fmaf(fl(sa * sb), graw, g0), float64, and the bound of its fp32 error
    (sa * sb rounds once unless it is exact; the fma once)."""
    s = sa * sb
    g = g0.double() + s * graw.double()
    exact_s = float(_f32(sa) * _f32(sb)) == s
    err = (0.0 if exact_s else U) * abs(s) * graw.double().abs() + U * (g0.double().abs() + abs(s) * graw.double().abs())
    return g, err * (1 + 4 * U)


def pose_ref(x, w, b):
    """[B, 8] float64 of k_pose_head_fwd: s_j (bias_j + sum_{p,c} x w_j / HW) (+1 for j = 6), the scales as fp32; and the sum of
    |terms| that its rounding count applies to: fl(S / HW), + bias, * s_j, (+ 1) -- 3 (4 for j = 6) roundings."""
    B, H, W, C = x.shape
    S = (x.double().sum(dim=(1, 2)) @ w.double().view(8, C).t())           # exact: sums of exact products (few hundred quanta)
    pre = b.double() + S / (H * W)
    s = torch.tensor([POSE_S] * 6 + [LCC_S] * 2, dtype=torch.float64, device=x.device)
    out = s * pre
    out[:, 6] += 1.0
    mag = s * (b.double().abs() + S.abs() / (H * W))
    mag[:, 6] += 1.0
    nround = torch.tensor([3] * 6 + [4, 3], dtype=torch.float64, device=x.device)
    return out, mag * (nround * U) * (1 + 8 * U)


def pose_bwd_refs(x, w, d_out, sa, sb):
    """float64 dx [B, H, W, C] (masked), dw [8, C], db [8] of k_pose_head_bwd* with go_j = d_j * fl(s_j * fl(sa * sb)), and the
    sums of |terms| their bounds multiply: the go chain rounds 1 + (0 if sa * sb is exact else 1) + 1 times."""
    B, H, W, C = x.shape
    HW = H * W
    s = torch.tensor([POSE_S] * 6 + [LCC_S] * 2, dtype=torch.float64, device=x.device)
    gs = sa * sb
    go = d_out.double() * s * gs                                            # [B, 8]
    wd = w.double().view(8, C)
    g = (go @ wd) / HW                                                     # [B, C]
    gabs = (go.abs() @ wd.abs()) / HW
    mask = (x > 0).double()
    dx = mask * g[:, None, None, :]
    dxabs = mask * gabs[:, None, None, :]
    sx = x.double().sum(dim=(1, 2))                                         # [B, C], exact
    dw = go.t() @ sx / HW
    dwabs = go.abs().t() @ sx.abs() / HW
    db = go.sum(0)
    dbabs = go.abs().sum(0)
    n_go = 1 + (0 if float(_f32(sa) * _f32(sb)) == gs else 1) + 1            # fl(sa sb), fl(s gs), fl(d * .)
    return dict(dx=dx, dxabs=dxabs, dw=dw, dwabs=dwabs, db=db, dbabs=dbabs, n_go=n_go)


def pose_bwd_bounds(r, B, out_dtype, det):
    """dx: go (n_go) then eight products summed (8) then * fl(1 / HW) (2): gamma of that count times the sum of |terms|, and the bf16
    store.  dw: per image fl(fl(go sx) * fl(1/HW)) (n_go + 3) and B atomics (or, deterministic, B ordered adds and the one add into
    dw).  db: B additions of go."""
    n = r["n_go"]
    dxb = gamma(n + 10) * r["dxabs"]
    if out_dtype == torch.bfloat16:
        dxb = dxb * (1 + U_BF) + U_BF * r["dxabs"]
    dwb = gamma(n + 3 + B + (1 if det else 0)) * r["dwabs"]
    dbb = gamma(n + B + (1 if det else 0)) * r["dbabs"]
    return dxb, dwb, dbb


# ------------------------------------------------------------------------------------------------------------------------------- #
# comparisons                                                                                                                     #
# ------------------------------------------------------------------------------------------------------------------------------- #
def ulp32(t):
    """fp32 ulp of |t| (float64 tensor; 2^-149 at 0)."""
    a = t.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double().clamp(min=2.0 ** -149)


def expect_within(got, ref, bound, what):
    """|got - ref| <= bound element-wise (got: the kernel's tensor, ref / bound: float64).  Returns (largest error in fp32 ulps of the
    reference, largest bound in the same ulps, largest error / bound): the margin on record."""
    got64 = got.double()
    err = (got64 - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    bad = err > bound
    if bool(bad.any()):
        n = int(bad.sum())
        first = tuple(int(i) for i in bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {n} of {bad.numel()} elements beyond the derived bound; first {first}: got {float(got64[first])!r}, "
                             f"float64 {float(ref[first])!r}, error {float(err[first]):.3e} > bound {float(bound[first]):.3e}")
    u = ulp32(ref)
    ratio = torch.where(bound > 0, err / bound, torch.zeros_like(err))
    return float((err / u).max()), float((bound / u).max()), float(ratio.max())


def check_pose_in(pose_in, frames, depth):
    """pose_in [Bh, H, W, 8] bf16 against frames [2 Bh, 3, H, W] cast by torch (channels 0..2 the target, 3..5 the reference frame of
    pair i) and depth [2 Bh, 1, H, W] (the head's fp32 output) rounded once to bf16 (channel 6: target, 7: reference): bit for bit."""
    Bh = pose_in.shape[0]
    want = torch.cat([frames[:Bh].permute(0, 2, 3, 1), frames[Bh:].permute(0, 2, 3, 1), depth[:Bh].permute(0, 2, 3, 1),
                      depth[Bh:].permute(0, 2, 3, 1)], dim=3).to(torch.bfloat16)
    bad = pose_in.view(torch.int16) != want.view(torch.int16)
    if bool(bad.any()):
        first = tuple(int(i) for i in bad.nonzero()[0].tolist())
        raise AssertionError(f"pose_in: {int(bad.sum())} of {bad.numel()} elements differ; first (pair, y, x, channel) {first}: "
                             f"got {float(pose_in[first])}, want {float(want[first])}")
