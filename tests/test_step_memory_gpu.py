"""-m gpu: the whole training step held to its own memory (tests/guarded.py).

2 pairs of 64 x 96 in bf16: dcdp_forward -> backward -> FusedAdam.step(), twice -- the first step records the passes, the second replays
them -- with everything the Python side allocates taken from the pool: the parameter, gradient and optimiser arenas (all layers' dw and
db side by side), the operand copies, the recorded passes' resident activations, the deterministic slabs and rows, the loss workspace
and its gradient planes.  Frames and intrinsics are guarded copies.  The guards of EVERYTHING allocated since the networks were built
are checked after each step.

Deterministic mode: the step runs plain, under 0xFF (every fresh buffer NaN) and under 0x55 (every fresh buffer a large finite number)
on freshly built networks with the same seed; loss, depths, pose, brightness terms, both gradient arenas and both parameter arenas
after each step are the same bits in the three runs.  A kernel that reads a buffer it never wrote, needs scratch zeroed, or leaves part
of an activation unwritten shows as a difference or as NaN.  Default (atomic) mode: guards intact and everything finite under both
poisons; float atomics leave no bits to compare."""
import contextlib

import pytest
import torch

from coivo_amd import synth
from tests import guarded as G
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

SEED, PAIRS, H, W = 14, 2, 64, 96


def _steps(poison, full_loss, deterministic):
    """Two steps -> [per step: dict of tensors], the pool (None for the plain run)."""
    from coivo_amd import nn as hnn
    from coivo_amd.optim import FusedAdam
    from oracle import colvo_spec as S
    pool = None if poison is None else G.Pool(dev(), poison)
    b = synth.make_batch(PAIRS, H, W, seed=SEED)
    snaps = []
    with contextlib.nullcontext() if pool is None else G.guarded_allocations(pool):
        dn_o, pn_o = S.make_models(SEED)
        dn, pn = hnn.DepthNet(compute_dtype=torch.bfloat16), hnn.PoseNet(compute_dtype=torch.bfloat16)
        dn.load_state_dict(dn_o.state_dict())
        pn.load_state_dict(pn_o.state_dict())
        dn.deterministic = pn.deterministic = deterministic
        opt = FusedAdam([dn, pn], lr=1e-3)
        d = {k: (b[k].to(dev()) if pool is None else pool.place(b[k].to(dev()), k)) for k in ("tgt", "ref", "K")}
        for step in range(2):
            opt.zero_grad()
            loss, d_t, d_r, pose, a, bb = hnn.dcdp_forward(dn, pn, d["tgt"], d["ref"], d["K"], full_loss=full_loss)
            loss.backward()
            dn.join_side()                               # (what FusedAdam.step() does before it reads the arenas)
            pn.join_side()
            torch.cuda.synchronize()
            snap = dict(loss=loss.detach().clone(), d_t=d_t.detach().clone(), d_r=d_r.detach().clone(), pose=pose.detach().clone(),
                        a=a.detach().clone(), b=bb.detach().clone(), depth_grad=dn.flat_grad.clone(), pose_grad=pn.flat_grad.clone())
            opt.step()
            torch.cuda.synchronize()
            snap.update(depth_param=dn.flat_param.clone(), pose_param=pn.flat_param.clone())
            snaps.append(snap)
            if pool is not None:
                pool.check(f"step {step}, poison {poison:#04x}, full_loss {full_loss}, deterministic {deterministic}", release=False)
        assert all(sum(1 for p in n._insts.values() if p) == 1 for n in (dn, pn))              # one recorded shape each: the second step replayed it
    return snaps, pool


def _sane(snaps, what):
    for i, s in enumerate(snaps):
        for k, v in s.items():
            assert bool(torch.isfinite(v).all()), f"{what}: step {i}: {k} is not finite"
        assert float(s["depth_grad"].abs().max()) > 0 and float(s["pose_grad"].abs().max()) > 0, f"{what}: step {i}: no gradient"
    assert not torch.equal(snaps[0]["depth_param"], snaps[1]["depth_param"]) and not torch.equal(snaps[0]["loss"], snaps[1]["loss"]), what


@pytest.mark.parametrize("full_loss", [False, True], ids=["photometric", "full_loss"])
def test_deterministic_step_is_the_same_bits_plain_and_under_both_poisons(full_loss):
    plain, _ = _steps(None, full_loss, True)
    _sane(plain, "plain")
    for poison in G.POISONS:
        got, pool = _steps(poison, full_loss, True)
        assert len(pool.served) > 50, len(pool.served)                   # the arenas, the activations, the scratch: the patch was there
        G.assert_same_bits(plain, got, f"plain against poison {poison:#04x}, full_loss {full_loss}")


@pytest.mark.parametrize("full_loss", [False, True], ids=["photometric", "full_loss"])
def test_atomic_step_stays_inside_its_buffers(full_loss):
    for poison in G.POISONS:
        got, pool = _steps(poison, full_loss, False)
        assert len(pool.served) > 50, len(pool.served)
        _sane(got, f"poison {poison:#04x}, full_loss {full_loss}")
