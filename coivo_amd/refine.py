"""Trajectory refinement by dense depth and intensity alignment (csrc/refine.hip): refine_edges / refine_trajectory
correct the trajectory against the depth maps and frames it connects.  coivo_amd.inference re-exports every name here.
"""
from typing import NamedTuple, Optional

import torch

from . import _lib
from ._args import MAX_DEPTH, depth_views, device_f32, finite_nonneg64, finite_pos32, int_range


class Refinement(NamedTuple):
    """The policy of refine_edges / refine_trajectory; also what reconstruct_sequence takes.  The defaults are choices, not values
    tuned on colonoscopy data (none is here): what the tests establish is on a synthetic textured tube."""
    iterations: int = 6          # Gauss-Newton steps
    sigma_geo: float = 0.01      # whitening of the geometric residual (P_z - s) / (P_z + s)
    sigma_photo: float = 0.02    # ... of the photometric residual (a c + b) - I_i, intensities in [0, 1]
    gate_geo: float = 0.05       # a geometric sample is used iff |residual| < gate_geo
    gate_photo: float = 0.1      # a photometric sample is used iff |residual| < gate_photo
    damping: float = 1e-6        # H + damping * diag(H)
    min_samples: int = 256       # an edge with fewer visible samples keeps its input
    geometric: bool = True       # alone, the geometric term is ill-conditioned in a tube: both terms are on by default
    photometric: bool = True
    brightness: bool = True      # solve a gain and an offset per edge alongside the pose (needs the photometric term)


class RefinementResult(NamedTuple):
    T: torch.Tensor          # [E,4,4] float64: frame-i camera coordinates -> frame j
    gain: torch.Tensor       # [E] float64
    offset: torch.Tensor     # [E] float64
    history: torch.Tensor    # [E, iterations + 1, 5] float64: n_visible, n_geo, C_g, n_photo, C_p of every evaluation
    status: torch.Tensor     # [E] int32: REFINE_OK, _TOO_FEW, _NOT_PD, _REVERTED, _BAD_EDGE


REFINE_OK, REFINE_TOO_FEW, REFINE_NOT_PD, REFINE_REVERTED, REFINE_BAD_EDGE = range(5)


def check_refinement(who: str, policy: Refinement, max_depth) -> int:
    """ValueError for what colvo_refine_edges would refuse; -> the `terms` bits."""
    int_range(who, "iterations", policy.iterations, 1, 64)
    int_range(who, "min_samples", policy.min_samples, 1)
    for name in ("sigma_geo", "sigma_photo", "gate_geo", "gate_photo"):
        finite_pos32(who, name, getattr(policy, name))
    finite_pos32(who, "max_depth", max_depth)
    finite_nonneg64(who, "damping", policy.damping)              # (damping is a double in the C ABI: judged in float64)
    for name in ("geometric", "photometric", "brightness"):
        if not isinstance(getattr(policy, name), (bool, int)):
            raise ValueError(f"{who}: {name} must be a bool, got {getattr(policy, name)!r}")
    if not (policy.geometric or policy.photometric):
        raise ValueError(f"{who}: at least one of the geometric and the photometric term must be enabled")
    return (1 if policy.geometric else 0) | (2 if policy.photometric else 0) | (4 if policy.brightness else 0)


def _refine_inputs(who: str, depths, frames, K, edges_ij, T):
    """Checked inputs of the refinement calls: (depths, frames, K, edges [E,2] int32 on the device, T [E,4,4] float64 on the device,
    N, H, W, E).  edges_ij is host data -- a sequence of (i, j) or an integer CPU tensor [E,2] -- so that a bad edge is a ValueError
    here and not a status on the device."""
    depths, K, _, N, H, W = depth_views(who, depths, K)
    frames = device_f32(who, "frames", frames, (N, 3, H, W))
    if isinstance(edges_ij, torch.Tensor):
        if edges_ij.is_cuda or edges_ij.is_floating_point():
            raise ValueError(f"{who}: edges_ij must be host data: a sequence of (i, j) or an integer CPU tensor [E,2]")
        edges_ij = edges_ij.tolist()
    try:
        pairs = [(int(i), int(j)) for i, j in edges_ij]
    except (TypeError, ValueError):
        raise ValueError(f"{who}: edges_ij must be a sequence of (i, j)") from None
    E = len(pairs)
    if not 1 <= E <= 65535 or N > 65535 or H <= 0 or W <= 0 or H * W >= 1 << 30:
        raise ValueError(f"{who}: E={E} N={N} H={H} W={W} beyond the kernels' limits (1 <= E <= 65535, N <= 65535, H*W < 2^30)")
    for i, j in pairs:
        if not (0 <= i < N and 0 <= j < N) or i == j:
            raise ValueError(f"{who}: bad edge ({i}, {j}): i != j, both in [0, {N})")
    if not isinstance(T, torch.Tensor) or T.dtype != torch.float64 or tuple(T.shape) != (E, 4, 4):
        raise ValueError(f"{who}: T must be a float64 tensor of shape ({E}, 4, 4), got {getattr(T, 'dtype', None)} "
                         f"{tuple(getattr(T, 'shape', ()))}")
    edges = torch.tensor(pairs, dtype=torch.int32).to(depths.device)
    return depths, frames, K, edges, T.to(depths.device).contiguous(), N, H, W, E


def refine_accumulate(depths: torch.Tensor, frames: torch.Tensor, K: torch.Tensor, edges_ij, T: torch.Tensor, *,
                      gain: Optional[torch.Tensor] = None, offset: Optional[torch.Tensor] = None, sigma_geo: float = 0.01,
                      sigma_photo: float = 0.02, gate_geo: float = 0.05, gate_photo: float = 0.1, geometric: bool = True,
                      photometric: bool = True, max_depth: float = MAX_DEPTH):
    """One evaluation of the refinement's sums at the edge states given (contract: include/colvo.h colvo_refine_accumulate):
    -> (sums [E,48] float64: the 36 upper-triangle entries of sum J^T J, the 8 of sum J^T e, C_g, C_p, two zeros;
    counts [E,4] int32: n_visible, n_geo, n_photo, 0), on the device.  gain / offset [E] float64 default to 1 / 0."""
    who = "refine_accumulate"
    terms = check_refinement(who, Refinement(sigma_geo=sigma_geo, sigma_photo=sigma_photo, gate_geo=gate_geo, gate_photo=gate_photo,
                                             geometric=geometric, photometric=photometric), max_depth) & 3
    depths, frames, K, edges, T, N, H, W, E = _refine_inputs(who, depths, frames, K, edges_ij, T)
    dev = depths.device
    for name, t in (("gain", gain), ("offset", offset)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or tuple(t.shape) != (E,)):
            raise ValueError(f"{who}: {name} must be a float64 tensor of shape ({E},)")
    gain = None if gain is None else gain.to(dev).contiguous()
    offset = None if offset is None else offset.to(dev).contiguous()
    lib = _lib.load()
    ws = torch.empty(int(lib.colvo_refine_workspace_bytes(E, N, H, W, 1)), device=dev, dtype=torch.uint8)
    sums = torch.empty(E, 48, device=dev, dtype=torch.float64)
    counts = torch.empty(E, 4, device=dev, dtype=torch.int32)
    _lib.call("colvo_refine_accumulate", depths, frames, K, N, H, W, edges, E, T, gain, offset, float(sigma_geo), float(sigma_photo),
              float(gate_geo), float(gate_photo), terms, float(max_depth), ws, sums, counts, _lib.stream_ptr())
    return sums, counts


def refine_edges(depths: torch.Tensor, frames: torch.Tensor, K: torch.Tensor, edges_ij, T_init: torch.Tensor, *,
                 iterations: int = 6, sigma_geo: float = 0.01, sigma_photo: float = 0.02, gate_geo: float = 0.05,
                 gate_photo: float = 0.1, damping: float = 1e-6, min_samples: int = 256, geometric: bool = True,
                 photometric: bool = True, brightness: bool = True, max_depth: float = MAX_DEPTH) -> RefinementResult:
    """Dense direct alignment of every edge (i, j, T) (contract: include/colvo.h colvo_refine_edges, DESIGN.md §3.6g;
    csrc/refine.hip).  depths [N,1,H,W], frames [N,3,H,W] in [0,1], K [N,3,3] (per frame), float32 on the device; edges_ij host data (a
    sequence of (i, j) or an integer CPU tensor [E,2], i != j, both in [0, N)); T_init [E,4,4] float64, T maps frame-i camera
    coordinates into frame j.  `iterations` Gauss-Newton steps on the geometric residual (P_z - s) / (P_z + s) and the photometric
    residual (a c + b) - I_i of every pixel of frame i that frame j sees, with a gain a and an offset b per edge; hard gates; float32
    per sample, float64 sums in a fixed order, float64 solve on the device.  An edge with fewer than min_samples visible samples or a
    normal matrix that is not positive definite keeps its input (status REFINE_TOO_FEW / REFINE_NOT_PD); one whose truncated cost per
    visible sample ends above where it started is reverted to it (REFINE_REVERTED).  Everything stays on the device: no read-back and
    no host synchronisation (the edge list is uploaded)."""
    who = "refine_edges"
    policy = Refinement(iterations, sigma_geo, sigma_photo, gate_geo, gate_photo, damping, min_samples, geometric, photometric,
                        brightness)
    terms = check_refinement(who, policy, max_depth)
    depths, frames, K, edges, T_init, N, H, W, E = _refine_inputs(who, depths, frames, K, edges_ij, T_init)
    dev = depths.device
    lib = _lib.load()
    ws = torch.empty(int(lib.colvo_refine_workspace_bytes(E, N, H, W, iterations)), device=dev, dtype=torch.uint8)
    T = torch.empty(E, 4, 4, device=dev, dtype=torch.float64)
    gain = torch.empty(E, device=dev, dtype=torch.float64)
    offset = torch.empty(E, device=dev, dtype=torch.float64)
    history = torch.empty(E, iterations + 1, 5, device=dev, dtype=torch.float64)
    status = torch.empty(E, device=dev, dtype=torch.int32)
    _lib.call("colvo_refine_edges", depths, frames, K, N, H, W, edges, E, T_init, iterations, float(sigma_geo), float(sigma_photo),
              float(gate_geo), float(gate_photo), float(damping), min_samples, terms, float(max_depth), ws, T, gain, offset, history,
              status, _lib.stream_ptr())
    return RefinementResult(T, gain, offset, history, status)


def rigid_inverse(T: torch.Tensor) -> torch.Tensor:
    R, t = T[:3, :3], T[:3, 3]
    out = torch.eye(4, dtype=torch.float64)
    out[:3, :3] = R.t()
    out[:3, 3] = -(R.t() @ t)
    return out


def refine_trajectory(depths: torch.Tensor, frames: torch.Tensor, K: torch.Tensor, cam2world: torch.Tensor, *,
                      max_depth: float = MAX_DEPTH, **policy):
    """Refines the N - 1 consecutive edges k -> k+1 of a trajectory (cam2world [N,4,4], any device; taken in float64):
    T_k = inverse(M_{k+1}) M_k, refine_edges with the Refinement policy given as keywords, one read-back of T, and the trajectory
    re-integrated from frame 0's pose exactly as integrate_trajectory does it, M_{k+1} = M_k inverse(T_k).
    -> (cam2world [N,4,4] float64 on the CPU, RefinementResult)."""
    policy = Refinement(**policy)
    if not isinstance(cam2world, torch.Tensor) or cam2world.dim() != 3 or tuple(cam2world.shape[1:]) != (4, 4):
        raise ValueError("refine_trajectory: cam2world must be [N,4,4]")
    M = cam2world.detach().to("cpu", torch.float64)
    n = M.shape[0]
    if n < 2:
        raise ValueError("refine_trajectory: need at least two frames")
    T0 = torch.stack([rigid_inverse(M[k + 1]) @ M[k] for k in range(n - 1)])
    res = refine_edges(depths, frames, K, [(k, k + 1) for k in range(n - 1)], T0, **policy._asdict(), max_depth=max_depth)
    T = res.T.cpu()
    out = [M[0].clone()]
    for k in range(n - 1):
        out.append(out[-1] @ rigid_inverse(T[k]))
    return torch.stack(out), res
