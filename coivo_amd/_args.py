"""How the post-training entry points (inference, fusion, consistency, refine, render, localize, evaluate) check an argument: the one
place that knows.  Every helper takes `who` -- the entry point's name -- and the argument's name, so a ValueError names both."""
import math
import struct
from typing import Optional, Tuple

import torch

MAX_DEPTH = 10.0     # spec: MAX_DEPTH


def f32(x) -> float:
    """x rounded to float32, as a Python float (what the C ABI's `float` arguments receive)."""
    return struct.unpack("f", struct.pack("f", float(x)))[0]


def _finite32(who: str, name: str, val, least: str) -> float:
    try:
        v = f32(val)
    except (TypeError, ValueError, OverflowError, struct.error):      # None, a string, 1e39
        v = math.nan
    if not (math.isfinite(v) and (v > 0.0 or (v == 0.0 and least == ">= 0"))):
        raise ValueError(f"{who}: {name} must be finite and {least} (as float32), got {val!r}")
    return v


def finite_pos32(who: str, name: str, val) -> float:
    """-> val as float32; ValueError unless that is finite and positive."""
    return _finite32(who, name, val, "positive")


def finite_nonneg32(who: str, name: str, val) -> float:
    """-> val as float32; ValueError unless that is finite and >= 0."""
    return _finite32(who, name, val, ">= 0")


def int_range(who: str, name: str, val, lo: int, hi: Optional[int] = None) -> int:
    """-> val; ValueError unless it is an int (a bool is not) with lo <= val, and val <= hi where a hi is given."""
    if isinstance(val, bool) or not isinstance(val, int) or val < lo or (hi is not None and val > hi):
        raise ValueError(f"{who}: {name} must be an int " + (f">= {lo}" if hi is None else f"in {lo}..{hi}") + f", got {val!r}")
    return val


def device_f32(who: str, name: str, t, shape) -> torch.Tensor:
    """-> t contiguous; ValueError unless it is a float32 tensor of that shape on the GPU."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{who}: {name}: expected a float32 CUDA tensor of shape {tuple(shape)}, got "
                         f"{getattr(t, 'dtype', None)} {tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', None)}")
    return t.contiguous()


def frames_shape(who: str, name: str, depths) -> Tuple[int, int, int]:
    """(N, H, W) of a stack of depth maps [N,1,H,W]; ValueError for anything that is not a 4-D tensor."""
    if not isinstance(depths, torch.Tensor) or depths.dim() != 4:
        raise ValueError(f"{who}: {name} must be [N,1,H,W]")
    return int(depths.shape[0]), int(depths.shape[2]), int(depths.shape[3])


def depth_views(who: str, depths, K, cam2world=None, name: str = "depths"):
    """The trio depths [N,1,H,W] / K [N,3,3] / cam2world [N,4,4] (the latter may be left out: None comes back), float32 on the device:
    -> (depths, K, cam2world, N, H, W), the tensors contiguous."""
    N, H, W = frames_shape(who, name, depths)
    depths = device_f32(who, name, depths, (N, 1, H, W))
    K = device_f32(who, "K", K, (N, 3, 3))
    cam2world = None if cam2world is None else device_f32(who, "cam2world", cam2world, (N, 4, 4))
    return depths, K, cam2world, N, H, W


def per_view_K(K, N: int):
    """K [3,3] -> a view [N,3,3] of it; anything else as it came (device_f32 judges it)."""
    return K.unsqueeze(0).expand(N, 3, 3) if isinstance(K, torch.Tensor) and K.dim() == 2 else K


def voxel_grid(who: str, origin, dims, voxel_size):
    """(origin, dims, voxel_size) as the kernels take them: origin three float32 values, dims three positive multiples of 8 (whole
    8x8x8 bricks), voxel_size a finite positive float32.  origin and dims come together; with neither, both come back None and the
    grid is the caller's to choose (fusion.fusion_grid)."""
    vs = finite_pos32(who, "voxel_size", voxel_size)
    if (origin is None) != (dims is None):
        raise ValueError(f"{who}: give origin and dims together, or neither")
    if origin is None:
        return None, None, vs
    origin = tuple(f32(o) for o in origin)
    dims = tuple(int(d) for d in dims)
    if len(origin) != 3 or len(dims) != 3 or any(d <= 0 or d % 8 for d in dims):
        raise ValueError(f"{who}: the grid's dims must be three positive multiples of 8, got {dims} (origin {origin})")
    return origin, dims, vs
