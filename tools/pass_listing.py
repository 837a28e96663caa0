#!/usr/bin/env python3
"""Every recorded pass of both networks after one training step, as text that two trees can be diffed on:
   python tools/pass_listing.py > listing.txt
Per command: op, stream, the descriptor's fields, i[], f[] and, for each pointer slot, the external's name or the ordinal of that
address's first appearance within the pass (never the address).  Per pass: marks, uses_side, flag_slots, deferred_join.
Shapes (pairs x H x W): 1x64x96, the smallest with both halves of a pair, and 8x256x320, where the fused top, the pose-front chain
and the halved grids are selected.  Modes: bf16, bf16 deterministic, bf16 grouped weight gradients, f32, bf16 with a hook."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coivo_amd import _lib, functional as Fh, nn as hnn, synth  # noqa: E402

MODES = [("bf16", torch.bfloat16, {}), ("bf16 deterministic", torch.bfloat16, {"deterministic": True}),
         ("bf16 group_wgrad", torch.bfloat16, {"group_wgrad": True}), ("f32", torch.float32, {}),
         ("bf16 hook", torch.bfloat16, {"grad_ready_hook": lambda net, begin, end: False})]


def show_pass(net, pr):
    names = {id(L): n for n, L in net.named_modules()}
    ext = {slot: name for name, slots in pr._slots.items() for slot in slots}
    seen = {}
    for ci in range(len(pr)):
        c = pr._arr[ci]
        ptrs = []
        for k in range(_lib.NPTR):
            if (ci, k) in ext:
                ptrs.append(ext[(ci, k)])
            elif c.p[k]:
                ptrs.append(f"#{seen.setdefault(c.p[k], len(seen))}")
            else:
                ptrs.append("-")
        desc = ",".join(str(getattr(c.desc, f)) for f, _ in c.desc._fields_)
        print(f"  {ci:3d} op {c.op} s{c.stream} desc[{desc}] p[{' '.join(ptrs)}] i{list(c.i)} f{[float(v).hex() for v in c.f]}")
    print(f"  marks {[(idx, names[id(L)], bool(on_side)) for idx, (L, on_side) in pr.marks]}")
    print(f"  uses_side {pr.uses_side} flag_slots {pr.flag_slots} deferred_join {bool(getattr(pr, 'deferred_join', False))}")


def main():
    dev = torch.device("cuda:0")
    for B, H, W in ((1, 64, 96), (8, 256, 320)):
        batch = synth.make_batch(B, H, W, seed=1, device=dev)
        frames = torch.cat([batch["tgt"], batch["ref"]]).contiguous()
        for label, dt, attrs in MODES:
            nets = {"DepthNet": hnn.DepthNet(compute_dtype=dt, device=dev), "PoseNet": hnn.PoseNet(compute_dtype=dt, device=dev)}
            for net in nets.values():
                for k, v in attrs.items():
                    setattr(net, k, v)
                net.zero_grad()
            d_t, d_r, d_l = nets["DepthNet"].forward_pair_split(frames)
            pose, a, b = nets["PoseNet"](frames[:B], frames[B:], d_t, d_r)
            Fh.photometric_loss(frames[:B], frames[B:], d_l, pose, batch["K"], a, b).backward()
            for net in nets.values():
                net.join_side()
            torch.cuda.synchronize()
            for name, net in nets.items():
                for key in net._insts:
                    for n, inst in enumerate(net._insts[key]):
                        for which in inst.passes:
                            print(f"== {B}x{H}x{W} {label}: {name} {key} inst {n} pass {which}")
                            show_pass(net, inst.passes[which][0])


if __name__ == "__main__":
    main()
