"""HIP-backed DepthNet / PoseNet with the spec's nn.Module signatures and state_dict keys.

Concept: /root/reference/README.md:5,7 (DCDP depth + pose networks, "multimodal fusion" coupling).
The reference ships no code; the layer stack, names and shapes are the frozen spec's
(oracle/colvo_spec.py DepthNet / PoseNet, oracle/SPEC.md §3), so `load_state_dict` works both ways.

MI355X-first host design
  * ParamArena (arena.py): every parameter of a network is a strided view into ONE flat fp32 buffer (weights in
    [Cout][kh][kw][Cin] memory order = the forward GEMM operand layout), gradients likewise in one flat
    buffer -> one fused Adam launch, and data-parallel all-reduce runs in place on bucket slices.
  * A whole network is ONE autograd node: forward enqueues its kernels back to back on the current
    stream, backward walks the layers in reverse, writing weight gradients straight into the arena
    (on a side stream: sidechain.py) and reporting each finished layer to an optional hook (gradient buckets for data parallel).
  * Feature maps are NHWC in `compute_dtype` (torch.float32 = exact-f32 MFMA parity mode,
    torch.bfloat16 = throughput mode, fp32 accumulation in both).
  * Each pass (forward / backward of a network at one shape) is RECORDED once as a command list with persistent
    activation buffers and replayed by one native call (passes.py, program.py, colvo_run_commands): driven layer by layer from
    Python the batch-8 step was bound by the host's ~18 us per launch, not by the GPU.  COLVO_NO_PROGRAM=1 keeps the
    layer-by-layer path: the same commands, each issued on its own as it is made (colvo_run_command), not recorded.
"""
from __future__ import annotations

import os
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np  # noqa: F401
import torch
import torch.nn as nn

from . import _lib, ops
from .arena import Arena, ConvParams
from .passes import RecordedPasses, _dealias, _Lease, _PassInst  # noqa: F401
from .program import Program
from .sidechain import SideChain, _SIDE_PRIORITY, _shared_side, _side_stream, share_side_stream, unshare_side_stream  # noqa: F401

ENC_CH = (32, 64, 128, 256, 512)
DEC_CH = (16, 32, 64, 128, 256)
POSE_CH = (16, 32, 64, 128, 256, 256, 256)
# The networks' topology, one row per layer: (name, input channels, output channels, kind, source activations).  Kinds: "s2" stride 2,
# "plain", "up" the source up-sampled x2, "cat" a second source (the encoder's skip) concatenated, "head".  The order is the
# REGISTRATION order: the arena offsets, the gradient buckets and every checkpoint depend on it.
DEPTH_LAYERS = (
    ("enc1a", 3, 32, "s2", ("in",)), ("enc1b", 32, 32, "plain", ("enc1a",)),
    ("enc2a", 32, 64, "s2", ("enc1b",)), ("enc2b", 64, 64, "plain", ("enc2a",)),
    ("enc3a", 64, 128, "s2", ("enc2b",)), ("enc3b", 128, 128, "plain", ("enc3a",)),
    ("enc4a", 128, 256, "s2", ("enc3b",)), ("enc4b", 256, 256, "plain", ("enc4a",)),
    ("enc5a", 256, 512, "s2", ("enc4b",)), ("enc5b", 512, 512, "plain", ("enc5a",)),
    ("up5", 512, 256, "up", ("enc5b",)), ("iconv5", 512, 256, "cat", ("up5", "enc4b")),
    ("up4", 256, 128, "up", ("iconv5",)), ("iconv4", 256, 128, "cat", ("up4", "enc3b")),
    ("up3", 128, 64, "up", ("iconv4",)), ("iconv3", 128, 64, "cat", ("up3", "enc2b")),
    ("up2", 64, 32, "up", ("iconv3",)), ("iconv2", 64, 32, "cat", ("up2", "enc1b")),
    ("up1", 32, 16, "up", ("iconv2",)), ("iconv1", 16, 16, "cat", ("up1",)),
    ("head", 16, 1, "head", ("iconv1",)))
POSE_LAYERS = (
    ("conv1", 8, 16, "s2", ("in",)), ("conv2", 16, 32, "s2", ("conv1",)), ("conv3", 32, 64, "s2", ("conv2",)),
    ("conv4", 64, 128, "s2", ("conv3",)), ("conv5", 128, 256, "s2", ("conv4",)), ("conv6", 256, 256, "s2", ("conv5",)),
    ("conv7", 256, 256, "s2", ("conv6",)), ("pred", 256, 8, "head", ("conv7",)))


class _ArenaModule(Arena, RecordedPasses, SideChain, nn.Module):
    """Base: owns the flat parameter / gradient arenas of its ConvParams children (arena.py), runs its passes as recorded programs
    (passes.py) and its weight gradients on a side stream (sidechain.py).  All per-network state of the three is set here."""

    def __init__(self, compute_dtype: torch.dtype):
        super().__init__()
        if compute_dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("compute_dtype must be torch.float32 or torch.bfloat16")
        self.compute_dtype = compute_dtype
        self.flat_param: Optional[torch.Tensor] = None
        self.flat_grad: Optional[torch.Tensor] = None
        self._packed_version = None
        self._manual_version = 0
        self._pack_table = None
        self._pack_dtype = None
        self._side = None
        self._plans = {}
        self._insts: Dict[tuple, List["_PassInst"]] = {}     # recorded programs + their activation buffers, per shape
        self.use_programs = _lib.dev_env("COLVO_NO_PROGRAM") is None           # developer switches: COLVO_DEV=1 only
        self._rec: Optional[Program] = None
        self.overlap_wgrad = _lib.dev_env("COLVO_NO_OVERLAP") is None
        # defer_join: the main stream does not wait for this network's weight gradients at the end of ITS backward node but
        # at the end of the whole backward pass (an autograd-engine callback), so the nodes that follow are enqueued in
        # between.  PoseNet's backward sits on the critical path in front of DepthNet's: only its input-gradient chain has
        # to finish before DepthNet's backward may start; its weight gradients then run beside DepthNet's kernels.
        self.defer_join = _lib.dev_env("COLVO_NO_DEFER_JOIN") is None
        self._join_pending = False
        self._cap_side_open = False          # under hipGraph capture: a pass of this network left its side chain open (carry mode)
        self.grad_ready_hook: Optional[Callable[["_ArenaModule", int, int], None]] = None
        # deterministic: weight gradients through per-split slabs + fixed-order second launches instead of float atomics
        # (include/colvo.h colvo_conv_wgrad_det): bitwise repeatable steps at the price of ~one small launch per layer.  Read when a
        # pass is RECORDED: call clear_programs() after changing it.
        self.deterministic = os.environ.get("COLVO_DETERMINISTIC") is not None
        # group_wgrad (round 4; OFF by default): the conv layers' weight gradients leave their kernels as per-split slabs (plain
        # stores, no float atomics) and ONE launch per group of layers adds the slabs to the gradient arena (include/colvo.h
        # colvo_conv_wgrad_slabs / colvo_wgrad_reduce_group).  Built on the in-kernel stamps of profiles/r4_wgrad_phases.md -- the
        # atomics are 6-7.7 us of every weight-gradient launch, the slab stores 2.3 -- and a LOSS in the step: 1.491-1.506 ms against
        # 1.420-1.427 with the atomics at configs[1] (+5 %), 3.80-3.83 against 3.73-3.76 at the configs[3] shape (+2 %), worse with
        # more splits (512-workgroup grids: 1.59 ms) and no better with groups of 3 / 12 / 64 MB; the per-layer deterministic form is
        # +1.6 %.  The slabs are 180 MB a step written and read back through HBM beside kernels that are bandwidth-bound at the top
        # of the network, and a group's launch waits for BOTH weight-gradient streams; the atomics are slow per launch but ride in
        # L2 under the other streams' kernels.  A group closes when it holds wgrad_group_bytes of gradients (or 16 layers); its
        # layers are reported to the gradient-ready hook then, in backward order.  Kept as an option (weight gradients are bitwise
        # repeatable in it; `deterministic` stays the per-layer form, which is the cheaper of the two).  Read when a pass is RECORDED.
        self.group_wgrad = _lib.dev_env("COLVO_WGRAD_GROUPED") is not None
        self.wgrad_group_bytes = int(_lib.dev_env("COLVO_WGRAD_GROUP_MB", "6")) << 20
        self._group: list = []
        self._group_bytes = 0

    def _trigger(self) -> torch.Tensor:
        # a leaf that requires grad so that autograd schedules the network's backward node
        t = getattr(self, "_trig", None)
        if t is None or t.device != self.flat_param.device:
            t = torch.zeros(1, device=self.flat_param.device, requires_grad=True)
            self._trig = t
        return t


def _conv(x0, L: ConvParams, desc, x1=None, whole_k: bool = False):
    y = torch.empty(desc.B, desc.Ho, desc.Wo, desc.Cout, device=x0.device, dtype=x0.dtype)
    ops.conv_fwd(desc, x0, x1, L.w_fwd, L.bias.data, y, whole_k)
    return y


class DepthNet(_ArenaModule):
    """forward(img [B,3,H,W] fp32) -> depth [B,1,H,W] fp32 in (0.1, 10).  H, W multiples of 32."""

    def __init__(self, compute_dtype: torch.dtype = torch.float32, device="cuda"):
        super().__init__(compute_dtype)
        for name, cin, cout, _, _ in DEPTH_LAYERS:
            setattr(self, name, ConvParams(cin, cout, 3, cin_pad=8 if cin == 3 else cin))
        self._build_arena(torch.device(device))

    def forward(self, img: torch.Tensor) -> torch.Tensor:
        """depth [B,1,H,W].  For an even batch -- the DCDP pair batch `depth_net(torch.cat([tgt, ref]))` of the spec's train step --
        the result is a _PairDepth: an ordinary depth tensor for every use, except that the spec's own next line, `d[:B]` /
        `d[B:]` with B = half the batch, returns the two halves as OUTPUTS of the network's autograd node (as forward_pair_split
        does) instead of slices of one output: no slice-backward nodes (zero-fill + copy + add each), PoseNet's input can come
        from the pass, and photometric_loss(.., d[:B], ..) finds the loss's own gradient path (functional.photometric_loss)."""
        # (the pair form exists for the backward pass: under no_grad / inference_mode -- where tensors carry no version counter for
        #  its tags, and the extra PoseNet-input buffer would only be kept alive -- the plain node runs.  ADVICE r5)
        if (img.dim() == 4 and img.shape[0] % 2 == 0 and img.shape[0] >= 2 and self.use_programs
                and torch.is_grad_enabled() and not torch.is_inference_mode_enabled()
                and _lib.dev_env("COLVO_NO_PAIR_FORWARD") is None):
            d_t, d_r, d_l, full = self._pair_node("forward", img, handover=True, whole=True)
            d_t._colvo_loss_twin = (d_l, d_l._version)      # photometric_loss swaps it in (once): the loss's own gradient path
            return _PairDepth.wrap(full, d_t, d_r)
        return _DepthNetFn.apply(self, img, self._trigger())

    def forward_pair(self, frames: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """frames [2B,3,H,W] = target frames then reference frames -> (depth_t, depth_r), each [B,1,H,W].
        Same as `d = self(frames); d[:B], d[B:]`, but the two halves are outputs of ONE autograd node: the backward
        gets their gradients directly instead of through two slice-backward nodes (zero-fill + copy + add each, ~8
        small launches on the critical path between the PoseNet and the DepthNet backward)."""
        return self._pair_node("forward_pair", frames)[:2]

    def forward_pair_split(self, frames: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """forward_pair with a third output: the target-frame depth AGAIN, as the tensor to hand to photometric_loss (and
        to nothing else).  It aliases depth_t, but being an output of its own the backward node receives the loss
        gradient separately from PoseNet's: no autograd add, no concatenation, and -- through the GradHandover it carries --
        no normalisation pass: the fused loss returns its unnormalised depth gradient plus two device scalars and the
        head backward applies them while it reads the gradient (functional.GradHandover)."""
        return self._pair_node("forward_pair_split", frames, handover=True)

    def forward_pair_full(self, frames: torch.Tensor):
        """forward_pair with BOTH depths a second time -> (depth_t, depth_r, depth_t', depth_r'): the primed pair goes to an
        objective that consumes both frames' depth (functional.dcdp_full_loss) and to nothing else, the plain pair to
        PoseNet.  The backward node then receives the four gradients separately and the head's backward kernel adds them
        while it reads them: no autograd accumulation, zero-fill or concatenation kernels."""
        return self._pair_node("forward_pair_full", frames, both=True)

    def _pair_node(self, entry: str, frames: torch.Tensor, handover: bool = False, both: bool = False, whole: bool = False):
        """The pair node's outputs for the entry point `entry`.  handover: the third output (the loss's depth) carries a GradHandover.
        The target-frame depth carries the PoseNet input this pass filled (see _forward_impl) to PoseNet.forward."""
        if frames.dim() != 4 or frames.shape[0] % 2:
            raise ValueError(f"{entry}: expected [2B,3,H,W]")
        from .functional import GradHandover
        hand = GradHandover() if handover else None
        outs = _DepthNetPairFn.apply(self, frames, self._trigger(), hand, both, whole)
        if hand is not None:
            outs[2]._colvo_handover = hand
        outs[0]._colvo_pose_in = getattr(self, "_pose_in", None)
        self._pose_in = None
        return outs

    # ---- whole-network forward / backward ---------------------------------------------------- #
    def _plan(self, B, H, W):
        dt = self.compute_dtype
        key = (B, H, W, dt)
        if key in self._plans:
            return self._plans[key]
        P = self._plans[key] = {}
        size = {"in": (H, W)}
        for name, cin, cout, kind, srcs in DEPTH_LAYERS[:-1]:
            h, w = (2 * s if kind == "up" else s for s in size[srcs[0]])      # (a descriptor's input size is the up-sampled one)
            cin = max(cin, 8)                               # (the stem's three channels are padded to eight)
            c0 = cout if kind == "cat" else cin             # (a skip's channels are the second source's)
            P[name] = ops.conv_desc(dt, B, h, w, c0, cout, stride=2 if kind == "s2" else 1, C1=cin - c0, up0=kind == "up")
            size[name] = (P[name].Ho, P[name].Wo)
        return P

    def _forward_impl(self, img: torch.Tensor, pair: bool = False):
        """pair: img is the DCDP pair batch [target frames | reference frames]; where the top of the network runs fused
        (colvo_conv_head_fused) the pass then also fills PoseNet's 8-channel input -- rgb from the stem's packing kernel, the two
        depth channels from the head -- and leaves it in self._pose_in for PoseNet.forward (which checks that it is handed these
        very frames and depths, and packs for itself otherwise)."""
        if img.dim() != 4 or img.shape[1] != 3:
            raise ValueError(f"DepthNet: expected [B,3,H,W], got {tuple(img.shape)}")
        B, _, H, W = img.shape
        if H % 32 or W % 32:
            raise ValueError("DepthNet: H and W must be multiples of 32")
        if not img.is_cuda or img.dtype != torch.float32:
            raise RuntimeError("DepthNet: expects a float32 CUDA tensor (no CPU fallback)")
        self._prepare_weights()
        P = self._plan(B, H, W)
        img = img.contiguous()
        depth = torch.empty(B, 1, H, W, device=img.device, dtype=torch.float32)
        fuse_top = ops.conv_head_fused_ok(P["iconv1"]) and _lib.dev_env("COLVO_NO_FWD16") is None
        pose_fill = (pair and fuse_top and B % 2 == 0 and not torch.is_inference_mode_enabled()      # (its tag reads version counters)
                     and _lib.dev_env("COLVO_NO_POSE_FILL") is None)
        # the packing pass, enc1a and enc1b as one launch (csrc/stem.hip) where the planner selects the shape: its answer follows the
        # tuning table (`stem_fused`), so it is asked per call and is part of the recorded pass's key
        stem = pose_fill and ops.stem_plan(P["enc1a"]) is not None
        inst = self._acquire((B, H, W, self.compute_dtype, pose_fill, stem))

        def body():
            A: Dict[str, torch.Tensor] = {}
            if pose_fill:
                x = torch.empty(B, H, W, 8, device=img.device, dtype=self.compute_dtype)
                # (the two depth channels of every pixel are written by the head below, the six rgb channels here)
                A["pose_in"] = torch.empty(B // 2, H, W, 8, device=img.device, dtype=self.compute_dtype)
                if stem:
                    # all four tensors are written, the bits are the three launches'
                    La, Lb, Pa = self.enc1a, self.enc1b, P["enc1a"]
                    for name in ("enc1a", "enc1b"):
                        A[name] = torch.empty(B, Pa.Ho, Pa.Wo, Pa.Cout, device=img.device, dtype=self.compute_dtype)
                    ops.stem_fused(Pa, img, x, A["pose_in"], La.w_fwd, La.bias.data, A["enc1a"], Lb.w_fwd, Lb.bias.data, A["enc1b"])
                else:
                    ops.pack_stem_pose(img, x, A["pose_in"])
            else:
                x = ops.pack_nchw([img], 8, self.compute_dtype)
            A["in"] = x
            if stem:
                x = A["enc1b"]
            for name, _, _, _, srcs in DEPTH_LAYERS[:-1]:
                if stem and name in ("enc1a", "enc1b"):
                    continue
                if name == "iconv1" and fuse_top:
                    # the narrow full-resolution layer and the depth head in one pass: its 42 MB output is written, not read back
                    L = self.iconv1
                    y = torch.empty(P["iconv1"].B, P["iconv1"].Ho, P["iconv1"].Wo, 16, device=x.device, dtype=x.dtype)
                    ops.conv_head_fused(P["iconv1"], x, L.w_fwd, L.bias.data, self.head.w_master, self.head.bias.data, y, depth,
                                        A.get("pose_in"))
                    A["iconv1"] = y
                    return A
                A[name] = x = _conv(A[srcs[0]], getattr(self, name), P[name], A[srcs[1]] if len(srcs) > 1 else None)
            ops.depth_head_fwd(x, self.head.w_master, self.head.bias.data, depth)
            return A

        A = self._run_pass(inst, "fwd", {"img": img, "depth": depth}, body)
        inst.gen += 1
        # (the tag holds `img` itself: while the tag lives the frames' memory cannot be handed to another tensor)
        self._pose_in = (A["pose_in"], img, depth.data_ptr(), depth._version, inst, inst.gen, img._version) if pose_fill else None
        return depth, (A, P, inst)

    def _backward_impl(self, saved, depth: torch.Tensor, d_depth: Optional[torch.Tensor], parts=None) -> None:
        """d_depth [B,1,H,W], or parts = (g_first, g_second, g_raw, scale_a, scale_b[, g_raw_second]): the gradient of the
        first / second half of the images and a (scaled) addend for each half (ops.depth_head_bwd_parts), each may be None."""
        A, P, inst = saved
        self._take_arena_zero()
        self.attach_grads()
        self._order_deterministic_pass()
        B, _, H, W = depth.shape
        dev = depth.device
        if parts is None:
            d_depth = d_depth.contiguous()
            ext = {"depth": depth, "d_depth": d_depth}
            which = "bwd"
        else:
            parts = tuple(_dealias([None if t is None else t.contiguous() for t in parts]))
            names = ("g_first", "g_second", "g_raw", "scale_a", "scale_b", "g_raw_second")
            ext = {"depth": depth}
            ext.update({n: t for n, t in zip(names, parts) if t is not None})
            which = "bwd:" + ",".join(n for n, t in zip(names, parts) if t is not None)

        def body():
            self._bwd_begin()

            def wgrad(name, x0, x1, dy):
                self._conv_wgrad(getattr(self, name), P[name], x0, x1, dy)

            def dgrad(name, src, dy, mask_like, dx=None, accumulate=False):
                L = getattr(self, name)
                if dx is None:
                    dx = torch.empty_like(mask_like)
                ops.conv_dgrad(P[name], src, dy, L.w_bwd, mask_like, dx, accumulate)
                return dx

            x1 = A["iconv1"]
            scratch = torch.empty(B * H * W, device=dev, dtype=torch.float32)
            # The narrow full-resolution layer (iconv1) takes its input gradient and weight gradient in ONE pass over its input and
            # output (include/colvo.h colvo_conv_bwd_fused); in the training step's form of this call (gradient in parts) the head's
            # input gradient is made inside that pass as well (HEAD form) and never touches memory.
            # Deterministic mode takes the fused pass with the slab way-out (colvo_conv_bwd_fused_det): the workgroups' sums go to rows
            # of a scratch and are added in row order by a reduction on a weight-gradient stream (below).  It keeps the head's input
            # gradient g from the head's own kernel (mode 0): the HEAD form makes g by split-bf16 MFMA, 2^-16 relative in front of the bf16
            # rounding, so which elements round up depends on the SCALE of the incoming gradient -- a step whose loss normaliser is
            # applied by the optimizer instead (ddp.GradBuckets(defer_loss_normalisation=True)) then differs from the plain step in
            # ~1 % of g's elements instead of ~1e-4 of them, and the two trajectories part (tests/test_ddp_gpu.py
            # test_rccl_path_with_one_rank).  Developer switch COLVO_DET_BWD16_HEAD=1: the HEAD form all the same.
            fuse1 = (not self.group_wgrad and ops.conv_bwd_fused_ok(P["iconv1"]) and _lib.dev_env("COLVO_NO_BWD16") is None)
            fuse_head = (fuse1 and parts is not None and _lib.dev_env("COLVO_NO_BWD16_HEAD") is None and
                         (not self.deterministic or _lib.dev_env("COLVO_DET_BWD16_HEAD") is not None))
            g = None if fuse_head else torch.empty_like(x1)
            # head: d(pre) + input gradient on the main stream, its weight gradient beside it like every other layer's
            if parts is None:
                ops.depth_head_bwd(x1, self.head.w_master, depth, d_depth, scratch, g, None, None)
            else:
                ops.depth_head_bwd_parts(x1, self.head.w_master, depth, *parts[:5], scratch, g,
                                         parts[5] if len(parts) > 5 else None)
            # (the head's OWN weight gradient can ride along too -- colvo_conv_bwd_fused's head_partials -- and measured no gain: it
            # leaves the side streams, where it overlapped, for the main chain: 1.464 against 1.455 ms at configs[1], 3.729 against
            # 3.732 at the configs[3] shape; developer switch COLVO_BWD16_HEADW=1)
            fuse_headw = fuse_head and not self.deterministic and _lib.dev_env("COLVO_BWD16_HEADW") is not None
            if not fuse_headw:
                if (self.compute_dtype == torch.bfloat16 and ops.depth_head_wgrad_mfma_ok(B, H, W) and
                        _lib.dev_env("COLVO_NO_HEAD_WGRAD_MFMA") is None):
                    # the head's weight gradient by MFMA (partial rows + table reduction: reproducible in every mode); from 2^25
                    # pixels on the table form of the VALU kernel below, reproducible as well
                    self._run_wgrad(self.head, lambda: ops.depth_head_wgrad_mfma(x1, scratch, self.head.g_master, self.head.g_bias),
                                    x1, scratch)
                else:
                    self._run_wgrad(self.head, lambda: ops.depth_head_wgrad(x1, scratch, self.head.g_master, self.head.g_bias,
                                                                            self.deterministic), x1, scratch)
            d_skip: Dict[int, torch.Tensor] = {}
            for i in range(1, 6):                       # decoder, output side first
                u = A[f"up{i}"]
                skip = A[f"enc{i - 1}b"] if i >= 2 else None
                L, Pi = getattr(self, f"iconv{i}"), P[f"iconv{i}"]
                if i == 1 and fuse1:
                    # on the main stream: d_u is the next layer's dy
                    d_u = torch.empty_like(u)
                    side_sum = False
                    if fuse_headw:
                        rows = ops.conv_bwd_fused_head_rows(Pi)
                        hp = torch.empty(rows * 145, device=dev, dtype=torch.float32)
                        ops.conv_bwd_fused(Pi, x1, L.w_bwd, u, True, d_u, L.g_master, L.g_bias, scratch, self.head.w_master, hp)
                        self._run_wgrad(self.head, lambda: ops.depth_head_wgrad_reduce(hp, rows, self.head.g_master, self.head.g_bias), hp)
                    else:
                        # (deterministic: the slab rows -- a recorded pass keeps them, like the other deterministic scratch.  The
                        # kernel runs here without dw: the rows are added below, on a weight-gradient stream)
                        rows = ops.conv_bwd_fused_scratch(Pi, 1 if fuse_head else 0, dev) if self.deterministic else None
                        side_sum = rows is not None and _lib.dev_env("COLVO_DET_BWD16_MAIN") is None
                        dw1 = None if side_sum else L.g_master
                        if fuse_head:
                            ops.conv_bwd_fused(Pi, x1, L.w_bwd, u, True, d_u, dw1, L.g_bias, scratch, self.head.w_master, scratch=rows)
                        else:
                            ops.conv_bwd_fused(Pi, g, L.w_bwd, u, True, d_u, dw1, L.g_bias, scratch=rows)
                    if side_sum:
                        # The rows are added by a command of its own on a weight-gradient stream, like every other layer's second
                        # launch, and iconv1 is reported done THERE, behind the reduction (_run_wgrad): the main chain goes on with
                        # dx.  The next pass's k_bwd16, which overwrites the rows on the main stream, is ordered behind this
                        # reduction by _order_deterministic_pass (a second backward pass joins the first one's side work in
                        # deterministic mode) and by the optimizer's join.  (Developer switch COLVO_DET_BWD16_MAIN=1: the reduction
                        # inside the command, on the main stream -- the B side of that measurement, profiles/det_bwd16_ab.md.)
                        sets = [(rows, L.g_master, L.g_bias, rows.numel() // (16 * 9 * 16 + 16), 16, 16)]
                        self._run_wgrad(L, lambda: ops.wgrad_reduce_group(sets), rows)
                    else:
                        self._layer_done(L)
                else:
                    wgrad(f"iconv{i}", u, skip, g)
                    if skip is not None:                # both sources' input gradients in one launch
                        d_u, d_skip[i - 1] = torch.empty_like(u), torch.empty_like(skip)
                        ops.conv_dgrad_both(Pi, g, L.w_bwd, u, skip, d_u, d_skip[i - 1])
                    else:
                        d_u = dgrad(f"iconv{i}", 0, g, u)
                below = A[f"iconv{i + 1}"] if i < 5 else A["enc5b"]
                wgrad(f"up{i}", below, None, d_u)
                g = dgrad(f"up{i}", 0, d_u, below)
            for i in range(5, 0, -1):                   # encoder
                a = A[f"enc{i}a"]
                wgrad(f"enc{i}b", a, None, g)
                g_a = dgrad(f"enc{i}b", 0, g, a)
                src = A["in"] if i == 1 else A[f"enc{i - 1}b"]
                wgrad(f"enc{i}a", src, None, g_a)
                if i > 1:
                    g = dgrad(f"enc{i}a", 0, g_a, src, dx=d_skip[i - 1], accumulate=True)
            self._bwd_end()

        self._run_pass(inst, which, ext, body)


class _PairDepth(torch.Tensor):
    """What DepthNet.forward returns for an even batch: the depth of the whole batch, an ordinary tensor in every respect (ops on
    it return plain tensors), whose two half-batch slices `d[:B]` / `d[B:]` are the pre-split outputs of the network's node."""
    __torch_function__ = torch._C._disabled_torch_function_impl

    @staticmethod
    def wrap(full: torch.Tensor, d_t: torch.Tensor, d_r: torch.Tensor) -> "_PairDepth":
        t = full.as_subclass(_PairDepth)
        t._colvo_halves = (full.shape[0] // 2, d_t, d_r, full._version)
        return t

    def __getitem__(self, idx):
        h = self.__dict__.get("_colvo_halves")
        if h is not None and isinstance(idx, slice) and idx.step in (None, 1) and self._version == h[3]:
            B, d_t, d_r, _ = h
            start, stop, _ = idx.indices(2 * B)
            if (start, stop) == (0, B):
                return d_t
            if (start, stop) == (B, 2 * B):
                return d_r
        return super().__getitem__(idx)


class _DepthNetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net: DepthNet, img, trigger):
        depth, saved = net._forward_impl(img)
        ctx.net, ctx.saved = net, saved
        ctx.lease = _Lease(saved[2])          # frees the pass instance when this context dies without a backward
        ctx.save_for_backward(depth)
        return depth

    @staticmethod
    def backward(ctx, d_depth):
        (depth,) = ctx.saved_tensors
        ctx.net._backward_impl(ctx.saved, depth, d_depth)
        ctx.saved = None
        ctx.lease.release()
        return None, None, None


class _DepthNetPairFn(torch.autograd.Function):
    """depth of [target frames | reference frames] as THREE outputs of one node: depth_t, depth_r and depth_t once more
    for the loss (forward_pair_split).  The backward receives the three gradients separately and hands them to the head's
    backward kernel as they are (no zero-fill, cat or add kernels in between)."""

    @staticmethod
    def forward(ctx, net: DepthNet, frames, trigger, handover, both=False, whole=False):
        depth, saved = net._forward_impl(frames, pair=True)
        ctx.net, ctx.saved, ctx.handover, ctx.whole = net, saved, handover, whole
        ctx.set_materialize_grads(False)           # an output nobody used arrives as None, not as a tensor of zeros to add
        ctx.lease = _Lease(saved[2])
        ctx.save_for_backward(depth)
        B = frames.shape[0] // 2
        if both:                                   # forward_pair_full: BOTH depths once more, for an objective that takes both
            return depth[:B], depth[B:], depth[:B], depth[B:]
        if whole:                                  # DepthNet.forward: the whole batch as a fourth output (any other use of `d`)
            return depth[:B], depth[B:], depth[:B], depth.view_as(depth)
        return depth[:B], depth[B:], depth[:B]

    @staticmethod
    def backward(ctx, g_t, g_r, g_l, g_4=None):
        (depth,) = ctx.saved_tensors
        sa = sb = None
        if ctx.handover is not None:
            sa, sb = ctx.handover.take((g_l,))     # unnormalised loss gradient + its two device scale factors
        if ctx.whole and g_4 is not None:
            # the whole-batch output was used as well (d.mean(), a slice other than the halves ...): the general backward on the sum
            B = depth.shape[0] // 2
            d_depth = g_4.clone()
            for half, g in ((d_depth[:B], g_t), (d_depth[B:], g_r)):
                if g is not None:
                    half.add_(g)
            if g_l is not None:
                d_depth[:B].add_(g_l * (sa * sb) if sa is not None else g_l)
            ctx.net._backward_impl(ctx.saved, depth, d_depth)
        else:
            ctx.net._backward_impl(ctx.saved, depth, None, parts=(g_t, g_r, g_l, sa, sb, None if ctx.whole else g_4))
        ctx.saved = None
        ctx.lease.release()
        return None, None, None, None, None, None


class PoseNet(_ArenaModule):
    """forward(tgt, ref, tgt_depth=None, ref_depth=None) -> (pose [B,6], lcc_a [B,1], lcc_b [B,1])."""

    def __init__(self, compute_dtype: torch.dtype = torch.float32, device="cuda"):
        super().__init__(compute_dtype)
        for name, cin, cout, kind, _ in POSE_LAYERS:
            setattr(self, name, ConvParams(cin, cout, 1 if kind == "head" else 3))
        # 7 tiny layers: driven from Python the fork/join bookkeeping costs more than it hides; recorded it is free.
        # With a deferred join (FusedAdam) only the input-gradient chain stays in front of DepthNet's backward.
        self.overlap_wgrad = self.overlap_wgrad and self.use_programs and _lib.dev_env("COLVO_NO_POSE_OVERLAP") is None
        self._build_arena(torch.device(device))

    def forward(self, tgt, ref, tgt_depth: Optional[torch.Tensor] = None, ref_depth: Optional[torch.Tensor] = None):
        from .functional import GradHandover
        hand = GradHandover()
        pose, a, b = _PoseNetFn.apply(self, tgt, ref, tgt_depth, ref_depth, self._trigger(), hand)
        # handed DIRECTLY to photometric_loss, the three outputs get their gradients unnormalised plus two device scalars
        # which the head's backward kernel applies (functional.GradHandover); any other use takes the ordinary path
        pose._colvo_handover = a._colvo_handover = b._colvo_handover = hand
        return pose, a, b

    def _plan(self, B, H, W):
        key = (B, H, W, self.compute_dtype)
        P = self._plans.get(key)
        if P is None:
            P = self._plans[key] = {}
            h, w = H, W
            for i, (_, cin, cout, _, _) in enumerate(POSE_LAYERS[:-1], start=1):
                P[i] = ops.conv_desc(self.compute_dtype, B, h, w, cin, cout, stride=2)
                h, w = P[i].Ho, P[i].Wo
        return P

    def _forward_impl(self, tgt, ref, d_t, d_r):
        B, _, H, W = tgt.shape
        for t in (tgt, ref):
            if tuple(t.shape) != (B, 3, H, W) or not t.is_cuda or t.dtype != torch.float32:
                raise RuntimeError("PoseNet: expects float32 CUDA images of equal shape [B,3,H,W] (no CPU fallback)")
        if (d_t is None) != (d_r is None):
            raise ValueError("PoseNet: pass both depth maps or neither")
        for t in (d_t, d_r):
            if t is not None and tuple(t.shape) != (B, 1, H, W):
                raise ValueError("PoseNet: depth maps must be [B,1,H,W]")
        self._prepare_weights()
        dt = self.compute_dtype
        has_depth = d_t is not None
        # DepthNet's pair pass may have assembled this very input already (DepthNet._forward_impl): taken only when tgt, ref, d_t
        # and d_r are, untouched, the frames that pass read and the depths it wrote
        filled = getattr(d_t, "_colvo_pose_in", None) if has_depth else None
        if filled is not None:
            # ... and the buffer still holds THAT pass: it belongs to DepthNet's pass instance, which a later forward re-uses as
            # soon as this one's autograd context is gone (at once under no_grad) -- `gen` names the run that filled it -- and
            # the frames have not been written in place since (d1 = forward_pair(f1); d2 = forward_pair(f2);
            # pose_net(f1[:B], f1[B:], *d1) passed the address / depth-version checks with f2's rgb and d2's depth in the buffer)
            buf, frames, depth_ptr, version, src_inst, gen, frames_version = filled
            frames_ptr = frames.data_ptr()
            ok = (tuple(buf.shape) == (B, H, W, 8) and buf.dtype == dt and tgt.is_contiguous() and ref.is_contiguous()
                  and d_t.is_contiguous() and d_r.is_contiguous() and tgt.data_ptr() == frames_ptr
                  and ref.data_ptr() == frames_ptr + 12 * B * H * W and d_t.data_ptr() == depth_ptr
                  and d_r.data_ptr() == depth_ptr + 4 * B * H * W and d_t._version == version and d_r._version == version
                  and src_inst.gen == gen and frames._version == frames_version and tgt._version == frames_version
                  and ref._version == frames_version)
            filled = buf if ok else None
        if filled is not None:
            has_depth = "filled"
            srcs = []
        else:
            srcs = _dealias([tgt.contiguous(), ref.contiguous()] + ([d_t.contiguous(), d_r.contiguous()] if has_depth else []))
        P = self._plan(B, H, W)
        # the planner's answer follows the tuning table (`pose_front`): asked per call, and part of the recorded pass's key
        P["front"] = front = ops.pose_front_plan(P[1]) is not None
        # ... and conv5-conv7 one by one (`pose_tail`, csrc/pose_tail.hip): the whole-K resident form where the planner selects it
        P["tail"] = tail = tuple(ops.pose_tail_plan(P[i]) is not None for i in (5, 6, 7))
        out = torch.empty(8 * B, device=tgt.device, dtype=torch.float32)     # planar: [pose Bx6 | a B | b B]
        inst = self._acquire((B, H, W, dt, front, tail, has_depth))

        def body():
            x = filled if filled is not None else ops.pack_nchw(srcs, 8, dt)
            A = {"in": x}
            first = 1
            if front:
                # conv1-conv3 as one launch (csrc/pose_front.hip): all three maps are written, the bits are the three launches'
                lays = []
                for i in range(1, 4):
                    L, d = getattr(self, f"conv{i}"), P[i]
                    A[i] = torch.empty(d.B, d.Ho, d.Wo, d.Cout, device=x.device, dtype=x.dtype)
                    lays.append((L.w_fwd, L.bias.data, A[i]))
                ops.conv_fwd_chain(P[1], x, lays)
                x, first = A[3], 4
            for i in range(first, len(POSE_LAYERS)):
                A[i] = x = _conv(x, getattr(self, POSE_LAYERS[i - 1][0]), P[i], whole_k=5 <= i <= 7 and tail[i - 5])
            ops.pose_head_fwd(x, self.pred.w_master, self.pred.bias.data, out)
            return A

        ext = {f"src{k}": t for k, t in enumerate(srcs)}
        ext["out"] = out
        if filled is not None:
            ext["in"] = filled             # belongs to DepthNet's pass instance: may be another buffer at the next step
        A = self._run_pass(inst, "fwd", ext, body)
        return out, (A, P, (B, H, W), has_depth, inst, filled)

    def _backward_impl(self, saved, d_pose, d_a, d_b, scale_a=None, scale_b=None):
        A, P, (B, H, W), has_depth, inst, filled = saved
        self._take_arena_zero()
        self.attach_grads()
        self._order_deterministic_pass()
        dev = self.flat_param.device
        grads = {"d_pose": d_pose, "d_a": d_a, "d_b": d_b, "scale_a": scale_a, "scale_b": scale_b}
        grads = {k: v.contiguous() for k, v in grads.items() if v is not None}
        grads = dict(zip(grads.keys(), _dealias(list(grads.values()))))
        # both depth gradients from one launch: [2][B,1,H,W], each half a contiguous tensor of its own
        d_tr = torch.empty(2, B, 1, H, W, device=dev, dtype=torch.float32) if has_depth else None
        d_t, d_r = (d_tr[0], d_tr[1]) if has_depth else (None, None)
        # the input-gradient chain ends in the depth planes: only a call with depth maps has it (asked per call, as in the forward pass)
        chain = bool(has_depth) and _lib.dev_env("COLVO_NO_DGRAD_PLANES") is None and ops.pose_front_plan(P[1], 1) is not None
        tail = tuple(ops.pose_tail_plan(P[i], 1) is not None for i in (5, 6, 7))      # (asked per call as well)

        def body():
            self._bwd_begin()
            x = A[7]
            g = torch.empty_like(x)
            ops.pose_head_bwd(x, self.pred.w_master, grads.get("d_pose"), grads.get("d_a"), grads.get("d_b"),
                              g, self.pred.g_master, self.pred.g_bias, grads.get("scale_a"), grads.get("scale_b"), self.deterministic)
            self._layer_done(self.pred)
            for i in range(7, 0, -1):
                L = getattr(self, f"conv{i}")
                src = (filled if filled is not None else A["in"]) if i == 1 else A[i - 1]
                self._conv_wgrad(L, P[i], src, None, g)
                if i == 3 and chain:
                    # g3 -> g2 -> g1 -> d_tr in one launch (csrc/pose_front.hip; the bits of the three launches below).  conv3's
                    # weight gradient was forked before it, conv2's and conv1's follow it, in today's order
                    g2, g1 = torch.empty_like(A[2]), torch.empty_like(A[1])
                    ops.conv_dgrad_chain(P[1], g, L.w_bwd, self.conv2.w_bwd, A[2], A[1], g2, g1, self.conv1.w_master, 6, 2, d_tr)
                    self._conv_wgrad(self.conv2, P[2], A[1], None, g2)
                    self._conv_wgrad(self.conv1, P[1], filled if filled is not None else A["in"], None, g1)
                    break
                if i > 1:
                    dx = torch.empty_like(src)
                    ops.conv_dgrad(P[i], 0, g, L.w_bwd, src, dx, False, whole_k=5 <= i <= 7 and tail[i - 5])
                    g = dx
                elif has_depth and _lib.dev_env("COLVO_NO_DGRAD_PLANES") is None:
                    # only the two depth channels of the 8-channel input gradient are wanted, as fp32 planes: one small kernel
                    # instead of the full input gradient + an unpack pass (include/colvo.h colvo_conv_dgrad_planes)
                    ops.conv_dgrad_planes(P[1], g, L.w_master, 6, 2, d_tr)
                elif has_depth:                      # (developer A/B switch: the round-3 form)
                    dx = torch.empty_like(src)
                    ops.conv_dgrad(P[i], 0, g, L.w_bwd, None, dx, False)
                    ops.unpack_nhwc_grad(dx, 6, 2, d_tr, False, by_channel=True)
            self._bwd_end()

        ext = dict(grads)
        if has_depth:
            ext["d_tr"] = d_tr
        if filled is not None:
            ext["in"] = filled
        # a missing (None) gradient changes the recorded commands, and so do the planners' answers
        which = "bwd:" + ",".join(sorted(grads)) + ",tail" + "".join(str(int(t)) for t in tail) + (",chain" if chain else "")
        self._run_pass(inst, which, ext, body)
        return d_t, d_r


class _PoseNetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net: PoseNet, tgt, ref, d_t, d_r, trigger, handover):
        out, saved = net._forward_impl(tgt, ref, d_t, d_r)
        ctx.net, ctx.saved, ctx.handover = net, saved, handover
        ctx.lease = _Lease(saved[4])
        B = tgt.shape[0]
        # three contiguous views of the planar head output: no slicing kernels forward or backward
        return out[:6 * B].view(B, 6), out[6 * B:7 * B].view(B, 1), out[7 * B:].view(B, 1)

    @staticmethod
    def backward(ctx, d_pose, d_a, d_b):
        sa, sb = ctx.handover.take((d_pose, d_a, d_b)) if ctx.handover is not None else (None, None)
        d_t, d_r = ctx.net._backward_impl(ctx.saved, d_pose, d_a, d_b, sa, sb)
        ctx.saved = None
        ctx.lease.release()
        return None, None, None, d_t, d_r, None, None


def dcdp_forward(depth_net: DepthNet, pose_net: PoseNet, tgt, ref, K, *, ssim_weight: float = 0.85, full_loss: bool = False,
                 frames: Optional[torch.Tensor] = None):
    """One coupled DCDP forward (spec: dcdp_forward): depth of both frames -> pose + LCC -> loss
    (full_loss: the widened objective dcdp_full_loss -- multi-scale photometric + geometric consistency + smoothness).
    frames (not in the spec): the pair batch already stacked as [target frames | reference frames] = [2B,3,H,W], as the loader
    delivers it; tgt / ref are then ignored (may be None) and the concatenation kernel is saved."""
    from .functional import dcdp_full_loss, photometric_loss
    if frames is not None:
        if frames.dim() != 4 or frames.shape[0] % 2:
            raise ValueError("dcdp_forward: frames must be [2B,3,H,W]")
        tgt, ref = frames[:frames.shape[0] // 2], frames[frames.shape[0] // 2:]
    else:
        frames = torch.cat([tgt, ref], dim=0)
        if not (tgt.requires_grad or ref.requires_grad):
            tgt, ref = frames[:tgt.shape[0]], frames[tgt.shape[0]:]     # the same values; PoseNet then recognises the pair batch
    if full_loss:
        # the objective is one native call that returns finished gradients (no hand-over of scale factors); the depth of both
        # frames reaches it through outputs of their own, so no gradient is accumulated by autograd
        d_t, d_r, d_lt, d_lr = depth_net.forward_pair_full(frames)
        pose, a, b = pose_net(tgt, ref, d_t, d_r)
        loss = dcdp_full_loss(tgt, ref, d_lt, d_lr, pose, K, a, b, ssim_weight=ssim_weight)
        return loss, d_t, d_r, pose, a, b
    d_t, d_r, d_l = depth_net.forward_pair_split(frames)
    pose, a, b = pose_net(tgt, ref, d_t, d_r)
    loss = photometric_loss(tgt, ref, d_l, pose, K, a, b, ssim_weight=ssim_weight)     # d_l aliases d_t (its own grad path)
    return loss, d_t, d_r, pose, a, b
