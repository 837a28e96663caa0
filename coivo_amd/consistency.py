"""Multi-view consistency filtering of a sequence's depth maps (csrc/consistency.hip): the cross-view check in front
of the stitching, the fusion and the localisation.  coivo_amd.inference re-exports every name here.
"""
from typing import NamedTuple

import torch

from . import _lib
from ._args import MAX_DEPTH, depth_views, finite_pos32, int_range


class Consistency(NamedTuple):
    """The policy of filter_depths; also what reconstruct_sequence takes.  The defaults are choices, not tuned values."""
    window: int = 2          # neighbours i +/- k*step, k = 1..window, that exist in [0, N)
    step: int = 1            # frame distance between neighbours (a wider baseline discriminates better)
    rel_tol: float = 0.01    # agree iff |P_z - s| / (P_z + s) < rel_tol
    min_agree: int = 1       # keep iff agree >= min_agree ...
    max_violated: int = 0    # ... and violated <= max_violated


class ConsistencyResult(NamedTuple):
    depths: torch.Tensor     # [N,1,H,W] float32: the input depth where kept, +inf elsewhere
    votes: torch.Tensor      # [N,3,H,W] uint8: planes agree / occluded / violated
    stats: torch.Tensor      # [N,5] int32: candidates, kept, no_view, few_agree, violated_out


def check_consistency(who: str, window, step, rel_tol, min_agree, max_violated, max_depth) -> None:
    """ValueError for what colvo_consistency_filter would refuse of the policy."""
    int_range(who, "window", window, 1, 16)
    int_range(who, "step", step, 1)
    int_range(who, "min_agree", min_agree, 0)
    int_range(who, "max_violated", max_violated, 0)
    if min_agree > 2 * window:
        raise ValueError(f"{who}: min_agree {min_agree} can never be reached with 2 * window = {2 * window} neighbours")
    finite_pos32(who, "rel_tol", rel_tol)
    finite_pos32(who, "max_depth", max_depth)


def filter_depths(depths: torch.Tensor, K: torch.Tensor, cam2world: torch.Tensor, *, window: int = 2, step: int = 1,
                  rel_tol: float = 0.01, min_agree: int = 1, max_violated: int = 0,
                  max_depth: float = MAX_DEPTH) -> ConsistencyResult:
    """Multi-view consistency check of a sequence's depth maps (contract: include/colvo.h colvo_consistency_filter, DESIGN.md
    §3.6f; csrc/consistency.hip).  depths [N,1,H,W], K [N,3,3] (per frame), cam2world [N,4,4], float32 on the device.  Every
    pixel with 0 < d < max_depth is carried through the trajectory into the frames i +/- k*step, k = 1..window, that exist;
    a neighbour that sees the point (in front, inside the image, four valid taps) AGREES if |P_z - s| / (P_z + s) < rel_tol
    for its own interpolated depth s, is OCCLUDED if s < P_z (legitimate: it does not count against the pixel) and is
    VIOLATED otherwise (the neighbour sees through the point).  A pixel is kept iff agree >= min_agree and violated <=
    max_violated.  N = 1, or a window * step that reaches past the sequence, is legal: those neighbours do not exist.

    A rejected pixel, and one that never was a candidate, is written as +inf, not 0: stitch_point_cloud keeps d < max_depth,
    so 0 would pass and put a point at the camera centre; fuse_point_cloud and localize_polyps keep 0 < d < max_depth.  +inf
    is dropped by all three, so the result feeds them unchanged.  No read-back and no host synchronisation."""
    who = "filter_depths"
    check_consistency(who, window, step, rel_tol, min_agree, max_violated, max_depth)
    depths, K, cam2world, N, H, W = depth_views(who, depths, K, cam2world)
    lib = _lib.load()
    ws_bytes = int(lib.colvo_consistency_workspace_bytes(N, window))
    if ws_bytes == 0 or H <= 0 or W <= 0 or H * W >= 1 << 30:
        raise ValueError(f"{who}: shape N={N} H={H} W={W} beyond the kernels' limits (N <= 65535, H*W < 2^30)")
    dev = depths.device
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    out = torch.empty(N, 1, H, W, device=dev, dtype=torch.float32)
    votes = torch.empty(N, 3, H, W, device=dev, dtype=torch.uint8)
    stats = torch.empty(N, 5, device=dev, dtype=torch.int32)
    _lib.call("colvo_consistency_filter", depths, K, cam2world, N, H, W, window, min(step, 1 << 30), float(rel_tol), min_agree,
              max_violated, float(max_depth), ws, out, votes, stats, _lib.stream_ptr())
    return ConsistencyResult(out, votes, stats)
