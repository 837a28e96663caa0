"""A chunked evaluation of the spec's loss terms (oracle/colvo_spec.py) with decision margins.

`evaluate` returns the value and every gradient of the photometric loss or of dcdp_full_loss, computed image chunk by
image chunk with the spec's own functions and combined with the spec's GLOBAL normalisers:

  * photometric, per level s:  sum(map * mask) / max(3 sum(n_valid), 1), the levels averaged;
  * geometric:  sum(|D_proj - D_samp| / (D_proj + D_samp) * mask) / max(sum(n_valid at level 0), 1);
  * smoothness:  a mean over all neighbour pairs of the batch (every image has as many, so a chunk of c images
    contributes c / B times its own mean).

The normalisers count validity, which carries no gradient, so the gradient of the whole objective is the sum over chunks
of the chunk's autograd gradient of its unnormalised sums times the global factors.  A batch at 32 x 512 x 640 then
never holds more than CHUNK_BYTES of float64 autograd graph.  With dtype=torch.float32 the same function is the fp32
oracle: the distance between the two is the rounding noise a kernel is measured against.

`margins=True` also returns, from the evaluation's own values, where an fp32 evaluation may take another DISCRETE
decision than this one (a validity flip, another bilinear cell, another sign of |.|, the SSIM clamp).  Those pixels may
differ by more than rounding; every other pixel may not.  The margin widths are justified by tests/test_loss_ref_cpu.py.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import colvo_spec as S

# Distance (pixels; and in z, camera units) from a validity bound or from an integer tap coordinate within which fp32 and
# fp64 may decide differently.  fp32 puts x, y about 1e-4 px off at 640 columns (|x| ~ 2^9, 2^-24 relative, a few
# operations); 2^-9 px leaves a factor of ~20.
DELTA = 2.0 ** -9
# |tgt - recal| below this may have either sign in fp32: recal moves by |grad I| * (error of x) ~ 0.2 * 1e-4 on the noisy
# test images, plus a few ulp of 1.
L1_EPS = 2.0 ** -12
# (1 - SSIM) / 2 this close to 0 or 1 may be clamped in one evaluation and not the other (its fp32 error: ~1e-5 of
# the variances' scale, which cancels where the window is flat)
SSIM_EPS = 2.0 ** -12
# |D_proj - D_samp| / (D_proj + D_samp) below this may have either sign in fp32
GEO_EPS = 2.0 ** -14
# |disp[x+1] - disp[x]| below this (relative to disp) may have either sign in fp32
SMOOTH_EPS = 2.0 ** -16

# float64 graph held at once: the chunk holds as many images as fit (at least one)
CHUNK_BYTES = 2 << 30
# measured peak bytes per pixel of one chunk's float64 graph (dcdp_full_loss, 3 scales, with the margin pass); the plain
# photometric loss needs about two thirds of it
GRAPH_BYTES_PER_PX = 2000


def noisy_case(B, H, W, seed, pose_scale=1.0, noise=0.1):
    """synth.make_batch frames with i.i.d. per-pixel noise (amplitude `noise`, clamped into [0, 1]) so that a one-row or
    one-column slip of any window or tap moves the result by the noise, not by a fraction of a smooth field; target and
    reference depth = the ground truth with 5 % noise each.  -> fp32 CPU dict(tgt, ref, K, depth, d_r, pose, lcc_a, lcc_b)."""
    from coivo_amd import synth
    b = synth.make_batch(B, H, W, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)

    def jitter(img):
        return (img + noise * (2 * torch.rand(img.shape, generator=g) - 1)).clamp(0.0, 1.0)

    def dep():
        return (b["gt_depth"] * (1 + 0.05 * torch.randn(B, 1, H, W, generator=g))).clamp(0.2, 9.0)

    return dict(tgt=jitter(b["tgt"]), ref=jitter(b["ref"]), K=b["K"], depth=dep(), d_r=dep(),
                pose=b["gt_pose"] * pose_scale + 0.003 * torch.randn(B, 6, generator=g), lcc_a=b["gt_a"], lcc_b=b["gt_b"])


def default_chunk(H, W, budget=CHUNK_BYTES):
    return max(1, int(budget // (GRAPH_BYTES_PER_PX * H * W)))


def _levels(tgt, ref, depth, K, num_scales):
    """(tgt, ref, depth, K) of every pyramid level, as multiscale_photometric_loss builds them."""
    out = [(tgt, ref, depth, K)]
    for _ in range(1, num_scales):
        tgt, ref, depth, K = S.downsample2(tgt), S.downsample2(ref), S.downsample2(depth), S.scale_intrinsics(K)
        out.append((tgt, ref, depth, K))
    return out


def _camera_z_and_pixel(depth, pose, K):
    """Pz of every target pixel in the reference camera and its projection WITHOUT project()'s safe divide (the margin
    needs the position a point behind or near the z bound would have)."""
    x, y, _ = S.project(depth, pose, K)
    B, _, H, W = depth.shape
    fx, fy = K[:, 0, 0].view(B, 1, 1), K[:, 1, 1].view(B, 1, 1)
    cx, cy = K[:, 0, 2].view(B, 1, 1), K[:, 1, 2].view(B, 1, 1)
    u = torch.arange(W, dtype=depth.dtype).view(1, 1, W)
    v = torch.arange(H, dtype=depth.dtype).view(1, H, 1)
    d = depth[:, 0]
    T = S.pose_vec2mat(pose)
    P = [T[:, i, 0].view(B, 1, 1) * ((u - cx) / fx * d) + T[:, i, 1].view(B, 1, 1) * ((v - cy) / fy * d)
         + T[:, i, 2].view(B, 1, 1) * d + T[:, i, 3].view(B, 1, 1) for i in range(3)]
    Pz = P[2]
    Pz_nz = torch.where(Pz.abs() > 1e-300, Pz, torch.full_like(Pz, 1e-300))
    return Pz, fx * P[0] / Pz_nz + cx, fy * P[1] / Pz_nz + cy


def validity_margin(x, y, Pz, H, W, delta=DELTA):
    """-> (sure, doubt) [B,H,W] bool: valid with room to spare; within `delta` of a validity bound (either way)."""
    loose = (Pz > S.Z_EPS - delta) & (x >= -delta) & (x <= W - 1 + delta) & (y >= -delta) & (y <= H - 1 + delta)
    tight = (Pz > S.Z_EPS + delta) & (x >= delta) & (x <= W - 1 - delta) & (y >= delta) & (y <= H - 1 - delta)
    return tight, loose & ~tight


def tap_margin(x, y, delta=DELTA):
    """x or y within `delta` of an integer: floor() may differ."""
    return ((x - torch.round(x)).abs() < delta) | ((y - torch.round(y)).abs() < delta)


def _dilate(m, r):
    if r == 0:
        return m
    return F.max_pool2d(m.unsqueeze(1).double(), 2 * r + 1, 1, r)[:, 0] > 0


def _up(m, s):
    """a level-s pixel mask -> level 0 (the 2^s x 2^s block every level-s pixel averages)."""
    f = 1 << s
    return m.repeat_interleave(f, dim=-2).repeat_interleave(f, dim=-1)


def _tap_scatter(mask, x, y, H, W):
    """the reference-depth pixels the 4 taps of every masked target pixel may touch (floor -1 .. +2 for slack)."""
    out = torch.zeros(mask.shape[0], H * W, dtype=torch.bool)
    bi, vi, ui = mask.nonzero(as_tuple=True)
    if bi.numel() == 0:
        return out.view(-1, H, W)
    xs = x[bi, vi, ui].clamp(0, W - 1).floor().long()
    ys = y[bi, vi, ui].clamp(0, H - 1).floor().long()
    for dy in (-1, 0, 1, 2):
        for dx in (-1, 0, 1, 2):
            idx = (ys + dy).clamp(0, H - 1) * W + (xs + dx).clamp(0, W - 1)
            out[bi, idx] = True
    return out.view(-1, H, W)


def _recal_pose_jacobian(rf, dp, pose, K, a):
    """|d recal / d pose_k| of every pixel and channel, k = 0..5 (forward mode, one tangent per component) -> [6,c,C,h,w]."""
    import torch.autograd.forward_ad as fwAD
    out = []
    for k in range(6):
        tan = torch.zeros_like(pose)
        tan[:, k] = 1.0
        with fwAD.dual_level():
            p = fwAD.make_dual(pose, tan)
            x, y, valid = S.project(dp, p, K)
            recal = S.lcc_recalibrate(S.bilinear_sample(rf, x, y, valid), a, torch.zeros_like(a))
            out.append(fwAD.unpack_dual(recal).tangent.abs())
    return torch.stack(out)


def _chunk_margins(lv, d_r, pose, a, b, geo, smooth, tgt0, d_t0, f_ph):
    """Decision margins of one chunk (no gradient).  -> dict(doubt [S][c,H_s,W_s], sure [S][...], m_t [c,1,H,W], m_r,
    allow [c, 8]: how far ONE decision in the margin may move d_pose (6), d_a, d_b of each image)."""
    B, _, H, W = d_t0.shape
    allow = torch.zeros(B, 8, dtype=d_t0.dtype)
    m_t = torch.zeros(B, H, W, dtype=torch.bool)
    m_r = torch.zeros(B, H, W, dtype=torch.bool)
    sure_l, doubt_l = [], []
    for s, (tg, rf, dp, K) in enumerate(lv):
        h, w = dp.shape[-2:]
        Pz, xr, yr = _camera_z_and_pixel(dp, pose, K)
        sure, doubt = validity_margin(xr, yr, Pz, h, w)
        sure_l.append(sure)
        doubt_l.append(doubt)
        maybe = sure | doubt                              # a pixel that may be valid in either evaluation
        x, y, valid = S.project(dp, pose, K)
        warped = S.bilinear_sample(rf, x, y, valid)
        recal = S.lcc_recalibrate(warped, a, b)
        l1 = ((tg - recal).abs() < L1_EPS).any(dim=1) & maybe
        ss = S.ssim_dissimilarity(tg, recal)
        clamp = ((ss <= SSIM_EPS) | (ss >= 1 - SSIM_EPS)).any(dim=1) & maybe
        # a validity flip changes recal at the pixel: every SSIM window that sees it (radius 1), and the gradient of every
        # window reaches the recal of its 3 x 3 (radius 2 in all)
        m = _dilate(doubt, 2) | (tap_margin(x, y) & maybe) | l1 | _dilate(clamp, 1)
        m_t |= _up(m, s)
        # A decision taken the other way at pixel p changes the terms that see recal_p: the sign of its L1 term (weight
        # 1 - alpha), its slope d recal_p / d(x, y) (another cell: at most about twice the slope), or recal_p itself (validity).
        # Each moves a reduced gradient by about 2 x |d recal_p / d theta| x the level's normaliser (|d map / d recal| <= 1
        # taken as the bound).  `allow` is the largest such move of one decision in the margin, per image.
        dec = (_dilate(doubt, 1) | (tap_margin(x, y) & maybe) | l1 | _dilate(clamp, 1)).unsqueeze(1)
        if bool(dec.any()):
            J = _recal_pose_jacobian(rf, dp, pose, K, a)
            decf = dec.to(dp.dtype)
            one = torch.cat([(J * decf).amax(dim=(2, 3, 4)).t(), (warped.abs() * decf).amax(dim=(1, 2, 3)).unsqueeze(1),
                             decf.amax(dim=(1, 2, 3)).unsqueeze(1)], dim=1)
            allow = torch.maximum(allow, 2 * f_ph[s] * one)
        if s == 0 and geo:
            d_samp = S.bilinear_sample(d_r, x, y, valid)[:, 0]
            gs = ((Pz - d_samp).abs() < GEO_EPS * (Pz + d_samp).abs()) & maybe
            m_t |= gs | doubt
            m_r |= _tap_scatter(gs | doubt, xr, yr, H, W)
    if smooth:
        disp = 1.0 / d_t0[:, 0]
        kx = (disp[:, :, 1:] - disp[:, :, :-1]).abs() < SMOOTH_EPS * disp[:, :, 1:]
        ky = (disp[:, 1:, :] - disp[:, :-1, :]).abs() < SMOOTH_EPS * disp[:, 1:, :]
        m_t[:, :, 1:] |= kx
        m_t[:, :, :-1] |= kx
        m_t[:, 1:, :] |= ky
        m_t[:, :-1, :] |= ky
    return dict(sure=sure_l, doubt=doubt_l, m_t=m_t.unsqueeze(1), m_r=m_r.unsqueeze(1), allow=allow)


def evaluate(t, *, dtype=torch.float64, num_scales=1, geo_weight=0.0, smooth_weight=0.0, ssim_weight=S.SSIM_WEIGHT,
             chunk=None, margins=False):
    """Value and gradients of the spec's dcdp_full_loss (num_scales=1 and no geo / smoothness weight: photometric_loss)
    at t = dict(tgt, ref, K, depth, pose, lcc_a, lcc_b[, d_r]), on the CPU in `dtype`, `chunk` images at a time.

    -> dict(loss (python float), d_depth, d_r (None without the geometric term), d_pose, d_a, d_b (CPU, `dtype`),
            n_valid [S, B] (float64: valid pixels per level and image));
       margins=True adds  n_sure, n_doubt [S, B] (valid with room to spare / within DELTA of a validity bound),
            m_depth, m_r [B,1,H,W] bool (the elements of d_depth / d_r that may take another discrete decision in fp32),
            allow [B, 8] (how far one of those decisions may move d_pose [:, :6], d_a [:, 6], d_b [:, 7])."""
    c = lambda k: t[k].detach().to("cpu", dtype)
    tgt, ref, dep, pose, K, la, lb = (c(k) for k in ("tgt", "ref", "depth", "pose", "K", "lcc_a", "lcc_b"))
    d_r = c("d_r") if geo_weight else None
    B, _, H, W = dep.shape
    chunk = chunk or default_chunk(H, W)
    parts = [slice(i, min(i + chunk, B)) for i in range(0, B, chunk)]
    # pass 1: the global normalisers (validity carries no gradient)
    n_valid = torch.zeros(num_scales, B, dtype=torch.float64)
    with torch.no_grad():
        for sl in parts:
            for s, (_, _, dp, Ks) in enumerate(_levels(tgt[sl], ref[sl], dep[sl], K[sl], num_scales)):
                n_valid[s, sl] = S.project(dp, pose[sl], Ks)[2].sum(dim=(1, 2)).double()
    tot = n_valid.sum(dim=1)
    f_ph = [1.0 / (num_scales * max(3.0 * tot[s].item(), 1.0)) for s in range(num_scales)]
    f_geo = geo_weight / max(tot[0].item(), 1.0)
    # pass 2: per chunk, the gradient of its unnormalised sums times the global factors
    loss = 0.0
    g = dict(d_depth=torch.zeros_like(dep), d_pose=torch.zeros_like(pose), d_a=torch.zeros_like(la), d_b=torch.zeros_like(lb),
             d_r=torch.zeros_like(d_r) if geo_weight else None)
    mg = dict(m_depth=torch.zeros(B, 1, H, W, dtype=torch.bool), m_r=torch.zeros(B, 1, H, W, dtype=torch.bool),
              n_sure=torch.zeros(num_scales, B, dtype=torch.float64), n_doubt=torch.zeros(num_scales, B, dtype=torch.float64),
              allow=torch.zeros(B, 8, dtype=torch.float64))
    for sl in parts:
        leaves = [x[sl].clone().requires_grad_(True) for x in (dep, pose, la, lb)]
        lr = d_r[sl].clone().requires_grad_(True) if geo_weight else None
        lv = _levels(tgt[sl], ref[sl], leaves[0], K[sl], num_scales)
        obj = 0.0
        for s, (tg, rf, dp, Ks) in enumerate(lv):
            m, valid = S.photometric_loss_map(tg, rf, dp, leaves[1], Ks, leaves[2], leaves[3], ssim_weight=ssim_weight)
            obj = obj + (m * valid).sum() * f_ph[s]
        if geo_weight:
            n0 = n_valid[0, sl].sum().item()
            obj = obj + S.geometric_consistency_loss(leaves[0], lr, leaves[1], K[sl]) * (max(n0, 1.0) * f_geo)
        if smooth_weight:
            obj = obj + S.smoothness_loss(leaves[0], tgt[sl]) * (smooth_weight * (sl.stop - sl.start) / B)
        grads = torch.autograd.grad(obj, leaves + ([lr] if geo_weight else []))
        loss += obj.item()
        for k, gr in zip(("d_depth", "d_pose", "d_a", "d_b", "d_r"), grads):
            g[k][sl] = gr
        del obj, grads, lv
        if margins:
            with torch.no_grad():
                lvd = _levels(tgt[sl], ref[sl], dep[sl], K[sl], num_scales)
                cm = _chunk_margins(lvd, d_r[sl] if geo_weight else None, pose[sl], la[sl], lb[sl], geo_weight,
                                    smooth_weight, tgt[sl], dep[sl], f_ph)
            mg["allow"][sl] = cm["allow"]
            mg["m_depth"][sl] = cm["m_t"]
            mg["m_r"][sl] = cm["m_r"]
            for s in range(num_scales):
                mg["n_sure"][s, sl] = cm["sure"][s].sum(dim=(1, 2)).double()
                mg["n_doubt"][s, sl] = cm["doubt"][s].sum(dim=(1, 2)).double()
    out = dict(loss=loss, n_valid=n_valid, **g)
    if margins:
        out.update(mg)
    return out


def spec_value_and_grads(t, *, dtype=torch.float64, num_scales=1, geo_weight=0.0, smooth_weight=0.0):
    """The unchunked spec (dcdp_full_loss in one piece) -- what `evaluate` must equal."""
    c = lambda k: t[k].detach().to("cpu", dtype)
    leaves = [c(k).requires_grad_(True) for k in ("depth", "pose", "lcc_a", "lcc_b")]
    lr = c("d_r").requires_grad_(True) if geo_weight else None
    loss = S.dcdp_full_loss(c("tgt"), c("ref"), leaves[0], lr, leaves[1], c("K"), leaves[2], leaves[3],
                            geo_weight=geo_weight, smooth_weight=smooth_weight, num_scales=num_scales)
    grads = torch.autograd.grad(loss, leaves + ([lr] if geo_weight else []))
    out = dict(loss=loss.item(), d_depth=grads[0], d_pose=grads[1], d_a=grads[2], d_b=grads[3],
               d_r=grads[4] if geo_weight else None)
    return out


def margin_fraction(r):
    return r["m_depth"].double().mean().item()

