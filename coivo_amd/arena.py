"""The parameter / gradient arena of a network (nn._ArenaModule inherits Arena; the layout is described there), its operand copies
and the "arena is still zero" flag.  Needs from the other parts of a network only `compute_dtype`, `_insts` (recorded programs hold
arena pointers: dropped when the arena or the operand copies move) and `join_side()` (sidechain.py) in front of zero_grad's clearing.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import ops


class ConvParams(nn.Module):
    """weight [Cout, Cin, k, k] (logical, OIHW like nn.Conv2d) + bias [Cout]; memory is arena-owned."""

    def __init__(self, cin: int, cout: int, k: int, cin_pad: Optional[int] = None):
        super().__init__()
        self.cin, self.cout, self.k = cin, cout, k
        self.cin_pad = cin_pad or cin
        self.weight = nn.Parameter(torch.zeros(cout, k, k, cin).permute(0, 3, 1, 2))
        self.bias = nn.Parameter(torch.zeros(cout))
        # filled by the arena
        self.w_master: Optional[torch.Tensor] = None   # [Cout, k*k, cin_pad] fp32 view (arena)
        self.g_master: Optional[torch.Tensor] = None
        self.g_bias: Optional[torch.Tensor] = None
        self.w_fwd: Optional[torch.Tensor] = None      # operand copies in compute dtype
        self.w_bwd: Optional[torch.Tensor] = None
        self.span: Tuple[int, int] = (0, 0)            # [begin, end) of this layer inside the arena


class Arena:
    """Owns the flat parameter / gradient arenas of the ConvParams children of the nn.Module it is mixed into."""

    def _layers(self) -> List[ConvParams]:
        # the module tree is fixed after construction: walk it once (per step this list and the parameter list below were
        # ~0.3 ms of the host's 1.1 ms enqueue time, tools/host_profile.py)
        ll = self.__dict__.get("_layer_list")
        if ll is None:
            ll = [m for m in self.modules() if isinstance(m, ConvParams)]
            self.__dict__["_layer_list"] = ll
            self.__dict__["_param_list"] = list(self.parameters())
        return ll

    def _build_arena(self, device) -> None:
        layers = self._layers()
        total = 0
        for L in layers:
            total += L.cout * L.k * L.k * L.cin_pad + L.cout
            total = (total + 63) // 64 * 64         # keep every layer 256-byte aligned
        flat = torch.zeros(total, device=device, dtype=torch.float32)
        grad = torch.zeros(total, device=device, dtype=torch.float32)
        off = 0
        for L in layers:
            nw = L.cout * L.k * L.k * L.cin_pad
            begin = off
            wv = flat[off:off + nw].view(L.cout, L.k, L.k, L.cin_pad)
            gv = grad[off:off + nw].view(L.cout, L.k, L.k, L.cin_pad)
            with torch.no_grad():
                wv[..., :L.cin].copy_(L.weight.detach().permute(0, 2, 3, 1).to(device))
            L.weight.data = wv[..., :L.cin].permute(0, 3, 1, 2)
            L.weight.grad = None
            L.w_master = flat[off:off + nw].view(L.cout, L.k * L.k, L.cin_pad)
            L.g_master = grad[off:off + nw].view(L.cout, L.k * L.k, L.cin_pad)
            L._gw_view = gv[..., :L.cin].permute(0, 3, 1, 2)
            off += nw
            with torch.no_grad():
                flat[off:off + L.cout].copy_(L.bias.detach().to(device))
            L.bias.data = flat[off:off + L.cout]
            L.bias.grad = None
            L.g_bias = grad[off:off + L.cout]
            off += L.cout
            off = (off + 63) // 64 * 64
            L.span = (begin, off)
            L.w_fwd = L.w_bwd = None
        self.flat_param, self.flat_grad = flat, grad
        self._packed_version = None
        self._pack_table = None
        self._insts = {}            # recorded programs hold pointers into the old arena

    def _apply(self, fn, *a, **kw):   # .to() / .cuda(): rebuild the arena on the new device
        super()._apply(fn, *a, **kw)
        p = next(self.parameters())
        self._build_arena(p.device)
        return self

    # True while the gradient arena is known to be all zero (set by optim.FusedAdam(zero_grad_in_step=True).step(), cleared by every
    # backward pass): the optimizer's zero_grad() then skips its launch
    _arena_zero_for_pass = False        # _grads_clean as the running backward pass found it (handed to its weight-gradient commands)
    _clean_flag = False
    _clean_version = -1
    _clean_in_capture = False

    # "The gradient arena is all zero."  Setting the flag records the arena's version counter: every torch-side write to a .grad view
    # (AccumulateGrad for a parameter that is also used outside the fused network, a manual p.grad.add_) bumps it, the library's own
    # kernels -- raw pointers -- do not; the flag reads True only while the counter is where the clearing left it.  Set while a stream
    # is being captured (the graph holds the clearing launch, nothing has executed) it holds inside that capture only: a capture that
    # fails, or ends, leaves it False.  (the flag alone was unguarded, and single-split layers STORE into an arena they
    # believe to be zero; an eager zero_grad() skips its launch on it.)
    @property
    def _grads_clean(self) -> bool:
        if not self._clean_flag or self.flat_grad is None:
            return False
        if self._clean_in_capture:
            return torch.cuda.is_current_stream_capturing()
        return self.flat_grad._version == self._clean_version

    @_grads_clean.setter
    def _grads_clean(self, clean: bool) -> None:
        self._clean_flag = bool(clean)
        if clean and self.flat_grad is not None:
            self._clean_version = self.flat_grad._version
            self._clean_in_capture = self.flat_grad.is_cuda and torch.cuda.is_current_stream_capturing()

    def _take_arena_zero(self) -> None:
        """Opens a backward pass: 'the arena is still zero' goes to its weight-gradient commands, and stops being true."""
        self._arena_zero_for_pass = self._grads_clean
        self._clean_flag = False

    def attach_grads(self) -> None:
        """Point every p.grad at its arena view (zeroing the arena if grads were set to None)."""
        layers = self._layers()
        for p in self.__dict__["_param_list"]:          # (the Parameter objects themselves: no nn.Module attribute lookups)
            if p.grad is None:
                break
        else:
            return
        ops.zero_(self.flat_grad)
        for L in layers:
            L.weight.grad = L._gw_view
            L.bias.grad = L.g_bias

    def zero_grad(self, set_to_none: bool = False) -> None:   # arena semantics: grads stay attached
        self.join_side()
        if self.flat_grad is not None:
            ops.zero_(self.flat_grad)          # one hipMemsetAsync, no torch fill kernel
            self.attach_grads()
            self._grads_clean = True           # until a backward pass -- or a torch-side write to .grad (version counter) -- touches it

    def mark_params_changed(self) -> None:
        self._manual_version += 1

    def _weights_version(self):
        # in-place updates of the parameters (any optimizer, load_state_dict) bump their version counters
        self._layers()
        return (sum(p._version for p in self.__dict__["_param_list"]), self._manual_version, self.compute_dtype)

    def _prepare_weights(self) -> None:
        """Refresh the operand-layout copies of the weights when the master changed (one launch per network)."""
        ver = self._weights_version()
        if ver == self._packed_version:
            return
        self._ensure_operand_buffers()
        ops.pack_weights_multi(self.flat_param, self._pack_table, self._pack_n, self._pack_blocks, self.compute_dtype, self._op_fwd,
                               self._op_bwd)
        self._packed_version = ver

    def operand_layout(self):
        """For an optimizer that writes the operand copies itself (optim.FusedAdam -> colvo_adam_pack_step):
        -> (layers, rest, op_fwd, op_bwd): layers = [(w_off, fwd_off or -1, bwd_off, Cout, Cin_pad)] of the 3x3 layers whose
        weights have operand copies, rest = [(offset, n)] every other range of the arena, the two operand buffers."""
        self._ensure_operand_buffers()
        layers, rest, at = [], [], 0
        for w_off, fwd_off, bwd_off, cout, cin in self._pack_layers:
            if w_off > at:
                rest.append((at, w_off - at))
            layers.append((w_off, fwd_off, bwd_off, cout, cin))
            at = w_off + cout * 9 * cin
        if self.flat_param.numel() > at:
            rest.append((at, self.flat_param.numel() - at))
        return layers, rest, self._op_fwd, self._op_bwd

    def operands_written(self) -> None:
        """The caller has just rewritten the master weights AND both operand copies (see operand_layout)."""
        self._manual_version += 1
        self._packed_version = self._weights_version()

    def _ensure_operand_buffers(self) -> None:
        dt = self.compute_dtype
        dev = self.flat_param.device
        if self._pack_table is None or self._pack_dtype != dt:
            layers = [L for L in self._layers() if L.k == 3 and L.cout > 1]   # heads read the fp32 master directly
            tab = np.zeros(len(layers), dtype=np.dtype([("w_off", "<i8"), ("fwd_off", "<i8"), ("bwd_off", "<i8"),
                                                        ("Cout", "<i4"), ("kk", "<i4"), ("Cin", "<i4"), ("blk", "<i4")]))
            total = sum(L.cout * 9 * L.cin_pad for L in layers)
            self._insts = {}        # recorded programs hold pointers into the old operand copies
            self._op_bwd = torch.empty(total, device=dev, dtype=dt)
            self._op_fwd = None if dt == torch.float32 else torch.empty(total, device=dev, dtype=dt)
            off = blk = 0
            self._pack_layers = []
            for i, L in enumerate(layers):
                n = L.cout * 9 * L.cin_pad
                tab[i] = (L.span[0], -1 if self._op_fwd is None else off, off, L.cout, 9, L.cin_pad, blk)
                self._pack_layers.append((L.span[0], -1 if self._op_fwd is None else off, off, L.cout, L.cin_pad))
                L.w_bwd = self._op_bwd[off:off + n].view(L.cin_pad, 9, L.cout)
                L.w_fwd = L.w_master if self._op_fwd is None else self._op_fwd[off:off + n].view(L.cout, 9, L.cin_pad)
                off += n
                blk += 9 * ((L.cout + 31) // 32) * ((L.cin_pad + 63) // 64)   # include/colvo.h: colvo_pack_weights_multi
            self._pack_table = torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
            self._pack_n, self._pack_blocks, self._pack_dtype = len(layers), blk, dt
            self._packed_version = None
