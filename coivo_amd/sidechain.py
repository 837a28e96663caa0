"""The weight-gradient side chain of a network's backward pass (nn._ArenaModule inherits SideChain): weight gradients run on a
side stream beside the input-gradient chain on the main stream, and these are the rules by which the two are joined again.
Needs from the arena (arena.py) only `flat_param`, `flat_grad` and `_arena_zero_for_pass`; `_rec` is the Program a pass is being
recorded into (passes.py), None while the layer bodies run launch by launch; the switches are those of nn._ArenaModule.__init__.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib, ops
from .arena import ConvParams

# weight-gradient stream: high priority (-1) -- it is the longer of the two chains of the backward pass (measured ~0.4 %
# of the step against normal priority, 0)
_SIDE_PRIORITY = int(_lib.dev_env("COLVO_SIDE_PRIORITY", "-1"))

_shared_side = {}


def _side_stream(device) -> "torch.cuda.Stream":
    """The weight-gradient side stream of one network.  Developer A/B COLVO_SHARED_SIDE_STREAM=1: ONE per device, shared by every
    network.  Measured (round 4, 8 pairs): a stream of its own per network is a hardware queue of its own and only four queues are
    served at a time -- with main + two side streams + the library's auxiliary stream the limit is reached, a THIRD weight-gradient
    stream (COLVO_SIDE_STREAMS=3) takes the step from 1.34 to 3.5 ms whatever GPU_MAX_HW_QUEUES says, with the shared stream it
    does not (1.344 ms) -- but it does not win either (two: 1.333), the eager step is level (1.333 against 1.336), and the replayed
    hipGraph lands its side branch on the main chain's queue (2.8-4.0 ms against 1.44; two more streams created in front of the
    capture cure that: graph.py COLVO_GRAPH_SPACER_STREAMS).  Hence: per network, as before."""
    if _lib.dev_env("COLVO_SHARED_SIDE_STREAM") is None:
        return torch.cuda.Stream(device=device, priority=_SIDE_PRIORITY)
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    st = _shared_side.get(key)
    if st is None:
        st = _shared_side[key] = torch.cuda.Stream(device=device, priority=_SIDE_PRIORITY)
    return st


def share_side_stream(modules) -> Optional["torch.cuda.Stream"]:
    """Put the weight gradients of every network in `modules` on ONE side stream (they keep running beside the main stream; the
    networks' backward passes follow one another anyway) and tell the stream policy: a hardware queue is then free for an external
    party -- ddp.GradBuckets calls this for RCCL's stream (streams.py has the measurements)."""
    from . import streams
    nets = [m for m in modules if isinstance(m, SideChain) and m.flat_param.is_cuda]
    if not nets or torch.cuda.is_current_stream_capturing():
        return None
    shared = next((m._side for m in nets if m._side is not None), None)
    if shared is None:
        shared = torch.cuda.Stream(device=nets[0].flat_param.device, priority=_SIDE_PRIORITY)
    for m in nets:
        if m._side is not shared:
            m.join_side()
            if m._side is not None:
                shared.wait_stream(m._side)        # (work a hook may still have in flight there)
            if not hasattr(m, "_side_before_sharing"):
                m._side_before_sharing = m._side   # what unshare_side_stream() gives back (created early: it keeps its hardware queue)
            m._side = shared
    streams.networks_share_side_stream(True)
    return shared


def unshare_side_stream(modules) -> None:
    """Undo share_side_stream(): every network gets the side stream it had before (ddp.GradBuckets.detach() left the
    networks on one stream and the policy's flag set; streams.configure() / reset() cleared the flag while the networks still shared).
    A network that had none yet creates its own at its next backward pass."""
    from . import streams
    if torch.cuda.is_current_stream_capturing():
        return
    for m in modules:
        if isinstance(m, SideChain) and hasattr(m, "_side_before_sharing"):
            m.join_side()
            old = m.__dict__.pop("_side_before_sharing")
            if old is not None and m._side is not None and old is not m._side:
                old.wait_stream(m._side)           # (work still in flight on the shared stream stays ahead of this network's next pass)
            m._side = old
    streams.networks_share_side_stream(False)


class SideChain:
    # ---- backward scheduling: weight gradients on a side stream, concurrent with the input gradients ------ #
    def _bwd_begin(self) -> None:
        self._group, self._group_bytes = [], 0
        self._main = torch.cuda.current_stream()
        if self.overlap_wgrad and self._side is None:
            self._side = _side_stream(self.flat_param.device)
        self._side_used = False

    def _run_wgrad(self, L, fn, *tensors) -> None:
        """fn() enqueues weight-gradient kernel(s); with overlap it runs on the side stream, ordered after everything already
        enqueued on the main stream (its inputs), and so does the gradient-ready hook (the data-parallel all-reduce of finished
        buckets) of the layers that are COMPLETE once fn() has run: L = one ConvParams, a list of them, or None."""
        layers = [] if L is None else ([L] if isinstance(L, ConvParams) else list(L))
        rec = self._rec

        def run():
            fn()
            for l_ in layers:
                self._layer_done(l_)
        if not self.overlap_wgrad:
            return run()
        if rec is not None:
            rec.fork()
            rec.stream = 1
            run()
            rec.stream = 0
        else:
            ev = torch.cuda.Event()
            ev.record(self._main)
            self._side.wait_event(ev)
            with torch.cuda.stream(self._side):
                run()
            for t in tensors:
                if t is not None:
                    t.record_stream(self._side)
        self._side_used = True

    def _conv_wgrad(self, L: ConvParams, desc, x0, x1, dy) -> None:
        """Weight / bias gradient of conv layer L into the gradient arena: atomics (default), the per-layer deterministic form, or grouped slabs (see group_wgrad)."""
        if not self.group_wgrad:
            scr = ops.conv_wgrad_scratch(desc, dy.device) if self.deterministic else None       # (per-layer deterministic form)
            self._run_wgrad(L, lambda: ops.conv_wgrad(desc, x0, x1, dy, L.g_master, L.g_bias, scr), x0, x1, dy)
            return
        scr = ops.conv_wgrad_scratch(desc, dy.device)          # (recorded passes keep it: persistent, like the activations)
        nsplit = ops.conv_wgrad_splits(desc)
        self._run_wgrad(None, lambda: ops.conv_wgrad_slabs(desc, x0, x1, dy, scr), x0, x1, dy, scr)
        self._group.append((L, (scr, L.g_master, L.g_bias, nsplit, desc.Cout, desc.C0 + desc.C1)))
        self._group_bytes += L.g_master.numel() * 4
        if self._group_bytes >= self.wgrad_group_bytes or len(self._group) == _lib.WGRAD_GROUP_MAX:
            self._wgrad_flush()

    def _wgrad_flush(self) -> None:
        """Close the open group: one launch adds its layers' slabs to the arena, then the layers count as done (in order)."""
        if not self._group:
            return
        group, self._group, self._group_bytes = self._group, [], 0
        sets = [g_[1] for g_ in group]

        def fn():
            if self._rec is not None:
                self._rec.side_sync()        # the group's kernels were dealt onto both side streams: wait for all of them
            ops.wgrad_reduce_group(sets)
        self._run_wgrad([g_[0] for g_ in group], fn, *[t for st_ in sets for t in st_[:3]])

    def _bwd_end(self) -> None:
        self._wgrad_flush()
        if self.overlap_wgrad and self._side_used:
            if self.defer_join:
                if self._rec is not None:
                    self._rec.deferred_join = True
                self._queue_join()
            elif self._rec is not None:
                self._rec.join()
            elif not torch.cuda.is_current_stream_capturing():
                self._main.wait_stream(self._side)

    def _queue_join(self) -> None:
        """Join the side stream when the running backward pass ends (falls back to joining now outside the engine)."""
        if self._join_pending or torch.cuda.is_current_stream_capturing():      # (a captured pass ends joined: program.hip)
            return
        self._join_pending = True
        main = torch.cuda.current_stream()

        def _final_join():
            if self._join_pending and self._side is not None:
                main.wait_stream(self._side)
            self._join_pending = False
        try:
            torch.autograd.Variable._execution_engine.queue_callback(_final_join)
        except RuntimeError:              # not inside a backward pass (a backward body driven by hand)
            _final_join()

    def join_side(self) -> None:
        """Make the current stream wait for the weight gradients still running on this network's side stream.  Under hipGraph
        capture the side chain lives in the library (csrc/program.hip, carry mode): the next captured node is made to depend on it."""
        if torch.cuda.is_current_stream_capturing():
            _lib.check(_lib.load().colvo_capture_join(_lib.stream_ptr()), "colvo_capture_join")
            self._cap_side_open = False
        elif self._join_pending and self._side is not None:
            torch.cuda.current_stream().wait_stream(self._side)
        self._join_pending = False
        self._stored_pass_open = False

    _stored_pass_open = False            # a backward pass of this network stored (not added) its weight gradients and is not joined yet

    def _order_deterministic_pass(self) -> None:
        """Deterministic mode, a SECOND backward pass of this network while the first one's weight gradients may still be running on
        the side streams (deferred join: one network applied twice inside one backward): the one-split write-out of
        colvo_conv_wgrad_det adds to dw / db with a plain read-modify-write -- sole writer within a launch, not across two launches on
        different streams -- so the earlier pass's side work is joined first.  The default (atomic) form needs no order."""
        # (the same holds for an earlier pass that STORED into the clean arena -- colvo_conv_wgrad_clean -- while this one adds
        #  with atomics: an add that lands before the store is lost.  Such a pass is joined too.)
        if self.deterministic or self._stored_pass_open:
            if torch.cuda.is_current_stream_capturing():
                if self._cap_side_open:          # (carry mode leaves this network's side chain open; policy 3 has two of them)
                    self.join_side()
            elif self._join_pending:
                self.join_side()
        self._stored_pass_open = self._arena_zero_for_pass

    def _layer_done(self, L: ConvParams) -> None:
        if self._rec is not None:
            self._rec.mark((L, self._rec.stream == 1))
        elif self.grad_ready_hook is not None:
            self.grad_ready_hook(self, L.span[0], L.span[1])
