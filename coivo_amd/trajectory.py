"""Trajectories (host, float64; camera-to-world [M,4,4], the convention of inference.integrate_trajectory)
  align_trajectory  Umeyama on the camera positions, mode "sim3" (default: monocular scale is unobservable), "se3" or "none",
                    with the reflection fix; returns (R, t, s) such that gt_position ~ s R pred_position + t.
  ate               RMSE of the position error after alignment.
  rpe               on E_i = (G_i^-1 G_{i+d})^-1 (P_i^-1 P_{i+d}), P's translations multiplied by the alignment scale:
                    (RMSE of |t(E_i)|, RMSE of the rotation angle arccos(clamp((tr R(E_i) - 1) / 2, -1, 1)) in degrees).
SURVEY.md §6, DESIGN.md §3.6b.  coivo_amd.evaluate re-exports every name here."""
import math
from typing import Tuple

import torch

ALIGN_MODES = ("sim3", "se3", "none")


def poses(T, name: str) -> torch.Tensor:
    """-> T as [M,4,4] float64 on the host; ValueError for another shape."""
    T = torch.as_tensor(T).detach().to("cpu", torch.float64)
    if T.dim() != 3 or tuple(T.shape[1:]) != (4, 4):
        raise ValueError(f"{name}: expected [M,4,4] camera-to-world transforms, got {tuple(T.shape)}")
    return T


def _pair(pred, gt) -> Tuple[torch.Tensor, torch.Tensor]:
    P, G = poses(pred, "pred"), poses(gt, "gt")
    if P.shape != G.shape:
        raise ValueError(f"pred {tuple(P.shape)} and gt {tuple(G.shape)} differ in length")
    return P, G


def align_trajectory(pred, gt, mode: str = "sim3") -> Tuple[torch.Tensor, torch.Tensor, float]:
    """Umeyama alignment of pred's camera positions to gt's: (R [3,3], t [3], s) minimising sum |g - (s R p + t)|^2, float64.
    mode "sim3" estimates the scale, "se3" fixes s = 1, "none" returns the identity."""
    if mode not in ALIGN_MODES:
        raise ValueError(f"align_trajectory: mode must be one of {ALIGN_MODES}, got {mode!r}")
    P, G = _pair(pred, gt)
    if mode == "none":
        return torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64), 1.0
    x, y = P[:, :3, 3], G[:, :3, 3]
    mx, my = x.mean(dim=0), y.mean(dim=0)
    xc, yc = x - mx, y - my
    cov = yc.t() @ xc / x.shape[0]
    U, D, Vt = torch.linalg.svd(cov)
    S = torch.ones(3, dtype=torch.float64)
    if torch.det(U) * torch.det(Vt) < 0:                 # reflection fix: a proper rotation
        S[2] = -1.0
    R = U @ torch.diag(S) @ Vt
    s = 1.0
    if mode == "sim3":
        var = float((xc * xc).sum(dim=1).mean())
        s = float((D * S).sum()) / var if var > 0 else 1.0
    t = my - s * (R @ mx)
    return R, t, s


def ate(pred, gt, mode: str = "sim3") -> float:
    """Absolute trajectory error: RMSE of the camera-position error after align_trajectory(pred, gt, mode)."""
    P, G = _pair(pred, gt)
    R, t, s = align_trajectory(P, G, mode)
    err = G[:, :3, 3] - (s * (P[:, :3, 3] @ R.t()) + t)
    return math.sqrt(float((err * err).sum(dim=1).mean()))


def _rel(T: torch.Tensor, delta: int) -> torch.Tensor:
    return torch.linalg.inv(T[:-delta]) @ T[delta:]


def rpe(pred, gt, delta: int = 1, mode: str = "sim3") -> Tuple[float, float]:
    """Relative pose error over `delta` frames: (RMSE of the translation error, RMSE of the rotation error in degrees) of
    E_i = (G_i^-1 G_{i+delta})^-1 (P_i^-1 P_{i+delta}), pred's translations scaled by align_trajectory's s."""
    P, G = _pair(pred, gt)
    if delta < 1 or delta >= P.shape[0]:
        raise ValueError(f"rpe: delta must be in [1, {P.shape[0] - 1}], got {delta}")
    _, _, s = align_trajectory(P, G, mode)
    P = P.clone()
    P[:, :3, 3] *= s
    E = torch.linalg.inv(_rel(G, delta)) @ _rel(P, delta)
    te = (E[:, :3, 3] ** 2).sum(dim=1)
    cos = ((E[:, 0, 0] + E[:, 1, 1] + E[:, 2, 2] - 1.0) / 2.0).clamp(-1.0, 1.0)
    ang = torch.rad2deg(torch.arccos(cos))
    return math.sqrt(float(te.mean())), math.sqrt(float((ang * ang).mean()))
