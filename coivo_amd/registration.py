"""Registration (csrc/register.hip; the contract is include/colvo.h colvo_register_*)
  register_clouds(source, target)  a few Gauss-Newton steps of point-to-plane ICP (metric "plane", the default; "point" is point to
            point, which crawls on a tube: the points slide along the wall) that refine a Sim(3) ("sim3") or SE(3) ("se3") moving
            source onto target, x' = s R x + t.  Every iteration is one nearest-neighbour pass of the transformed source over the
            target's index -- nearest_neighbors' own walk, rule for rule -- and 37 float64 sums in a fixed order; the 6x6 / 7x7 step is
            solved on the device.  No read-back and no host synchronisation; identical bits on every call and stream.
  status    REGISTER_OK; REGISTER_TOO_FEW (fewer than min_pairs pairs used), REGISTER_NOT_PD (a surface with a free motion: an exact
            cylinder) and REGISTER_REVERTED (the final truncated cost per valid point is above the initial one) return the initial
            state to the bit.  There is no convergence test and no early exit.
coivo_amd.evaluate re-exports every name here."""
import math
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib
from ._args import cloud, finite_nonneg64, int_range, reach, sim3

REGISTER_MODES = ("se3", "sim3")          # the C ABI's 0 and 1
REGISTER_METRICS = ("plane", "point")
REGISTER_OK, REGISTER_TOO_FEW, REGISTER_NOT_PD, REGISTER_REVERTED = 0, 1, 2, 3
REGISTER_HISTORY = ("n_valid", "n_reached", "n_used", "cost", "sum_r2")


class Registration(NamedTuple):
    """The policy of register_clouds.  Choices, not tuned values: sim3 because monocular scale is unobservable, plane because point
    to point crawls on a tube, 20 iterations where the test scenes converge in 3, a damping that only keeps a well-posed system
    away from a zero pivot, and 64 pairs as the least a 7-parameter fit should rest on."""
    mode: str = "sim3"              # "sim3" or "se3" (s is then left as given)
    metric: str = "plane"           # "plane" (needs the target's normals) or "point"
    iterations: int = 20            # 1 .. 64 Gauss-Newton steps; there is no early exit
    max_dist: Optional[float] = None    # reach of the nearest-neighbour search; None: the metrics' own max_dist
    damping: float = 1e-9           # H_kk <- H_kk + damping * H_kk
    min_pairs: int = 64             # fewer used pairs freeze the state (REGISTER_TOO_FEW)


class RegistrationResult(NamedTuple):
    R: torch.Tensor                 # [3,3] float64 on the device
    t: torch.Tensor                 # [3]   float64
    s: torch.Tensor                 # []    float64: x' = s R x + t
    history: torch.Tensor           # [iterations+1,5] float64: REGISTER_HISTORY of every evaluation
    status: torch.Tensor            # []    int32: REGISTER_*
    normal_matrix: torch.Tensor     # [7,7] float64: sum J^T J of the final evaluation (v, omega, sigma), undamped

    def transform(self) -> Tuple[torch.Tensor, torch.Tensor, float]:
        """(R [3,3], t [3], s) on the host, float64, as align_trajectory returns it and cloud_metrics(transform=...) and
        transform_cloud take it.  The one read-back."""
        v = torch.cat([self.R.reshape(9), self.t.reshape(3), self.s.reshape(1)]).to("cpu")
        return v[:9].reshape(3, 3).clone(), v[9:12].clone(), float(v[12])


def check_registration(who: str, policy) -> Registration:
    """-> policy; ValueError for what colvo_register_clouds would refuse of it."""
    if not isinstance(policy, Registration):
        raise ValueError(f"{who}: register must be a Registration or None, got {type(policy).__name__}")
    if policy.mode not in REGISTER_MODES:
        raise ValueError(f"{who}: mode must be one of {REGISTER_MODES}, got {policy.mode!r}")
    if policy.metric not in REGISTER_METRICS:
        raise ValueError(f"{who}: metric must be one of {REGISTER_METRICS}, got {policy.metric!r}")
    int_range(who, "iterations", policy.iterations, 1, 64)
    int_range(who, "min_pairs", policy.min_pairs, 1, 2 ** 31 - 1)
    finite_nonneg64(who, "damping", policy.damping)
    if policy.max_dist is not None:
        reach(who, policy.max_dist, ())
    return policy


def _register_inputs(who: str, source, target, target_normals, init, pivot, max_dist, metric):
    """Checked inputs of the registration calls: (source, target, normals or None, state [13] float64 on the device, pivot [3] float32
    on the device, max_dist as float32, index workspace with the target's index enqueued)."""
    source = cloud(who, "source", source)
    target = cloud(who, "target", target)
    dev = source.device
    if target.device != dev:
        raise ValueError(f"{who}: target is on {target.device}, source on {dev}")
    if metric not in REGISTER_METRICS:
        raise ValueError(f"{who}: metric must be one of {REGISTER_METRICS}, got {metric!r}")
    if target_normals is None:
        if metric == "plane":
            raise ValueError(f"{who}: metric 'plane' needs target_normals [M,3] (inference.cloud_normals(...).normals)")
    else:
        target_normals = cloud(who, "target_normals", target_normals)
        if target_normals.shape != target.shape or target_normals.device != dev:
            raise ValueError(f"{who}: target_normals {tuple(target_normals.shape)} on {target_normals.device} do not match target "
                             f"{tuple(target.shape)} on {dev}")
    md, _ = reach(who, max_dist, ())
    R, t, s = (torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64), 1.0) if init is None else sim3(who, "init", init)
    state = torch.cat([R.reshape(9), t, torch.tensor([s], dtype=torch.float64)])
    M = target.shape[0]
    if pivot is None:
        # the centre of the box of the target's finite points: amin / amax are exact and order-free; no read-back
        if M == 0:
            pv = torch.zeros(3, device=dev, dtype=torch.float32)
        else:
            fin = torch.isfinite(target).all(dim=1, keepdim=True)
            lo = torch.where(fin, target, torch.full_like(target, math.inf)).amin(dim=0)
            hi = torch.where(fin, target, torch.full_like(target, -math.inf)).amax(dim=0)
            pv = 0.5 * lo + 0.5 * hi
            pv = torch.where(torch.isfinite(pv), pv, torch.zeros_like(pv))
    else:
        try:
            pv = torch.as_tensor(pivot).detach().to(torch.float32).reshape(-1)
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f"{who}: pivot must be three numbers") from None
        if pv.numel() != 3:
            raise ValueError(f"{who}: pivot must be three numbers, got {pv.numel()}")
        pv = pv.to(dev).contiguous()
    lib = _lib.load()
    nbytes = int(lib.colvo_cloud_workspace_bytes(0, M))
    if nbytes == 0 or int(lib.colvo_register_scratch_bytes(source.shape[0])) == 0:
        raise ValueError(f"{who}: {source.shape[0]} source and {M} target points: each cloud must hold fewer than 2^30")
    index = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    _lib.call("colvo_cloud_index_build", target, M, md, index, _lib.stream_ptr())
    return source, target, target_normals, state.to(dev), pv, md, index


def register_accumulate(source: torch.Tensor, target: torch.Tensor, *, target_normals: Optional[torch.Tensor] = None, init=None,
                        pivot=None, max_dist: float, metric: str = "plane") -> Tuple[torch.Tensor, torch.Tensor]:
    """One evaluation of the registration's sums at the state `init` (contract: include/colvo.h colvo_register_accumulate):
    (sums [40] float64: the 28 upper-triangle entries of sum J^T J, the 7 of sum J^T r, the truncated cost C, sum r^2, three zeros;
    counts [4] int64: n_valid, n_reached, n_used, 0), on the device.  The test hook of register_clouds."""
    who = "register_accumulate"
    source, target, normals, state, pv, md, index = _register_inputs(who, source, target, target_normals, init, pivot, max_dist, metric)
    dev = source.device
    N, M = source.shape[0], target.shape[0]
    ws = torch.empty(int(_lib.load().colvo_register_scratch_bytes(N)), device=dev, dtype=torch.uint8)
    sums = torch.empty(40, device=dev, dtype=torch.float64)
    counts = torch.empty(4, device=dev, dtype=torch.int64)
    _lib.call("colvo_register_accumulate", source, N, target, normals, M, md, index, state, pv,
              REGISTER_METRICS.index(metric), ws, sums, counts, _lib.stream_ptr())
    return sums, counts


def register_clouds(source: torch.Tensor, target: torch.Tensor, *, target_normals: Optional[torch.Tensor] = None, init=None,
                    pivot=None, max_dist: float, mode: str = "sim3", metric: str = "plane", iterations: int = 20,
                    damping: float = 1e-9, min_pairs: int = 64) -> RegistrationResult:
    """Register source [N,3] onto target [M,3] (float32 clouds on the GPU): `iterations` Gauss-Newton steps of point-to-plane ICP
    against target_normals [M,3] (a zero normal: the point takes no part), or of point-to-point ICP, on the (R, t, s) of
    x' = s R x + t (module docstring; contract: include/colvo.h colvo_register_clouds).
    init = (R, t, s) as align_trajectory returns it (None: the identity); the source itself is never pre-transformed, so a sample is
    rounded to float32 once.  pivot: the point the update turns and scales about -- it conditions the problem and does not change
    what is minimised --, by default the centre of the box of the target's finite points.  max_dist is the reach of the search; pairs
    further apart do not exist.  The defaults are Registration's: choices, not tuned.
    Builds the target's index, enqueues everything on the current stream and returns device tensors: no read-back and no host
    synchronisation (RegistrationResult.transform() is the read-back).  Check `status`: anything but REGISTER_OK returned init."""
    who = "register_clouds"
    policy = check_registration(who, Registration(mode, metric, iterations, None, damping, min_pairs))
    source, target, normals, state, pv, md, index = _register_inputs(who, source, target, target_normals, init, pivot, max_dist, metric)
    dev = source.device
    N, M = source.shape[0], target.shape[0]
    ws = torch.empty(int(_lib.load().colvo_register_scratch_bytes(N)), device=dev, dtype=torch.uint8)
    out = torch.empty(13, device=dev, dtype=torch.float64)
    history = torch.empty(policy.iterations + 1, 5, device=dev, dtype=torch.float64)
    status = torch.empty(1, device=dev, dtype=torch.int32)
    normal = torch.empty(7, 7, device=dev, dtype=torch.float64)
    _lib.call("colvo_register_clouds", source, N, target, normals, M, md, index, state, pv,
              REGISTER_MODES.index(policy.mode), REGISTER_METRICS.index(policy.metric), policy.iterations, float(policy.damping),
              int(policy.min_pairs), ws, out, history, status, normal, _lib.stream_ptr())
    return RegistrationResult(out[:9].view(3, 3), out[9:12], out[12], history, status[0], normal)
