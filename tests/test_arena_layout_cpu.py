"""The parameter / gradient arena of both networks against a recording of it (tests/golden/arena_layout.json): layer spans and
padded shapes in registration order, the arena's size, the state_dict keys, the operand-copy layout and the packing table's
counts, for both compute dtypes.  Gradient buckets, the optimizer's operand offsets and every checkpoint depend on these.

    python tests/test_arena_layout_cpu.py --record      rewrites the recording from the tree it is run in
"""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "arena_layout.json")
CASES = [(net, dt) for net in ("DepthNet", "PoseNet") for dt in ("float32", "bfloat16")]


def describe(net_name: str, dtype_name: str) -> dict:
    from coivo_amd import nn as hnn
    net = getattr(hnn, net_name)(compute_dtype=getattr(torch, dtype_name), device="cpu")
    names = {id(m): n for n, m in net.named_modules()}
    layers, rest, _, _ = net.operand_layout()
    return {"layers": [[names[id(L)], L.span[0], L.span[1], L.cin_pad, L.cout, L.k] for L in net._layers()],
            "numel": net.flat_param.numel(),
            "state_dict": list(net.state_dict().keys()),
            "operand_layers": [list(t) for t in layers],
            "operand_rest": [list(t) for t in rest],
            "pack_n": net._pack_n,
            "pack_blocks": net._pack_blocks}


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("net_name,dtype_name", CASES)
def test_arena_layout_is_the_recorded_one(recorded, net_name, dtype_name):
    got, want = describe(net_name, dtype_name), recorded[f"{net_name}/{dtype_name}"]
    assert sorted(got) == sorted(want)
    for field in want:
        assert got[field] == want[field], field


def test_recorded_sizes(recorded):
    assert len(recorded["DepthNet/float32"]["layers"]) == 21 and recorded["DepthNet/float32"]["numel"] == 7855424
    assert len(recorded["PoseNet/float32"]["layers"]) == 8 and recorded["PoseNet/float32"]["numel"] == 1575680
    order = [r[0] for r in recorded["DepthNet/bfloat16"]["layers"]]
    assert order == ([f"enc{i}{ab}" for i in range(1, 6) for ab in "ab"] +
                     [f"{kind}{i}" for i in range(5, 0, -1) for kind in ("up", "iconv")] + ["head"])
    assert [r[0] for r in recorded["PoseNet/bfloat16"]["layers"]] == [f"conv{i}" for i in range(1, 8)] + ["pred"]


if __name__ == "__main__" and "--record" in sys.argv:
    with open(GOLDEN, "w") as f:
        json.dump({f"{n}/{d}": describe(n, d) for n, d in CASES}, f, indent=0, sort_keys=True)
        f.write("\n")
