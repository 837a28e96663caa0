"""tests/guarded.py on the CPU device: the layout, the report of a write into a guard, and what the patch takes and leaves."""
import pytest
import torch

from tests import guarded as G

CPU = torch.device("cpu")


def _raw(pool, i=-1):
    return pool.slots[i].raw


def test_layout_and_poison():
    pool = G.Pool(CPU)
    for poison, dtype, shape in ((0xFF, torch.float32, (3, 5)), (0x55, torch.bfloat16, (7,)), (0x55, torch.int32, (2, 1, 3)),
                                 (0xFF, torch.int32, (4,)), (0x55, torch.uint8, (17,)), (0x55, torch.float32, (0, 4))):
        t = pool.empty(shape, dtype, poison=poison)
        raw, n = _raw(pool), t.numel() * t.element_size()
        assert t.shape == shape and t.dtype == dtype and t.is_contiguous()
        assert (n == 0 or t.data_ptr() == raw.data_ptr() + G.GUARD) and raw.numel() == 2 * G.GUARD + (n + 15) // 16 * 16
        assert bool((raw[:G.GUARD] == 0xFF).all()) and bool((raw[G.GUARD + n:] == 0xFF).all())
        assert bool((raw[G.GUARD:G.GUARD + n] == poison).all())
    assert torch.isnan(pool.empty((4,), torch.float32, poison=0xFF)).all()
    assert torch.isnan(pool.empty((4,), torch.bfloat16, poison=0xFF).float()).all()
    assert pool.empty((2,), torch.int32, poison=0xFF).tolist() == [-1, -1]
    assert pool.empty((2,), torch.int32, poison=0x55).tolist() == [1431655765] * 2
    big = pool.empty((2,), torch.float32, poison=0x55)
    assert torch.isfinite(big).all() and float(big[0]) > 1e13
    assert pool.served[:3] == [60, 14, 24] and pool.total_served() == sum(pool.served)
    pool.check("layout")
    assert pool.slots == []                                              # checked slots are released


def test_place_copies_and_works_as_a_leaf():
    pool = G.Pool(CPU)
    src = torch.arange(24, dtype=torch.float32).view(2, 3, 4).transpose(0, 2)       # not contiguous
    t = pool.place(src, "x")
    assert t.is_contiguous() and torch.equal(t, src) and pool.place(None) is None
    v = t._version
    leaf = t.requires_grad_(True)
    (leaf * 2).sum().backward()
    assert torch.equal(leaf.grad, torch.full_like(src, 2.0)) and t._version == v
    pool.check("place")


@pytest.mark.parametrize("side,index,offset", [("front", G.GUARD - 1, -1), ("back", G.GUARD + 40, 40)])
def test_a_write_one_byte_outside_is_reported(side, index, offset):
    pool = G.Pool(CPU)
    pool.empty((3,), torch.float32, label="before")
    t = pool.empty((2, 5), torch.float32, label="victim")               # 40 bytes of payload, 8 of pad
    pool.empty((3,), torch.float32, label="after")
    pool.slots[1].raw[index] = 0
    with pytest.raises(G.GuardError) as e:
        pool.check("probe")
    msg = str(e.value)
    assert "probe" in msg and "(2, 5)" in msg and "torch.float32" in msg and "'victim'" in msg, msg
    assert f"{side} guard" in msg and f"first at payload offset {offset} " in msg, msg
    assert "'before'" not in msg and "'after'" not in msg and ("front" if side == "back" else "back") not in msg, msg
    assert pool.slots == [] and t.numel() == 10


def test_a_write_into_the_pad_is_reported():
    pool = G.Pool(CPU)
    pool.empty((5,), torch.bfloat16)                                      # 10 bytes: the pad is bytes 10..15
    pool.slots[0].raw[G.GUARD + 10] = 0x55
    with pytest.raises(G.GuardError, match="back guard written: 1 bytes, first at payload offset 10 "):
        pool.check()


def test_the_patch_is_undone_after_an_exception():
    real = {n: getattr(torch, n) for n in G._NAMES}
    pool = G.Pool(CPU)
    with pytest.raises(ZeroDivisionError):
        with G.guarded_allocations(pool, 0x55):
            assert all(getattr(torch, n) is not real[n] for n in G._NAMES)
            1 / 0
    assert all(getattr(torch, n) is real[n] for n in G._NAMES)
    with G.guarded_allocations(pool):
        pass
    assert all(getattr(torch, n) is real[n] for n in G._NAMES)


def test_plain_calls_go_through_the_pool():
    pool = G.Pool(CPU)
    with G.guarded_allocations(pool, 0x55):
        a = torch.empty(3, 4)
        b = torch.empty((5,), dtype=torch.int32, device="cpu")
        c = torch.zeros(torch.Size((2, 3)), dtype=torch.bfloat16, device=CPU)
        d = torch.ones(size=(4,), requires_grad=True)
        e = torch.full((2, 2), 7.5)
        f = torch.full((3,), 3, dtype=torch.int32)
        g = torch.full([2], fill_value=True)
        like = torch.arange(6.0).view(2, 3)
        h, i, j, k = torch.empty_like(like), torch.zeros_like(like, dtype=torch.int32), torch.ones_like(like), torch.full_like(like, -2.0)
        m = torch.full_like(like, fill_value=4.0, requires_grad=True)
        n = torch.empty(0)
    assert len(pool.slots) == 13 and pool.served == [48, 20, 12, 16, 16, 12, 2, 24, 24, 24, 24, 24, 0]
    assert a.shape == (3, 4) and a.dtype == torch.float32 and bool((a.view(torch.uint8) == 0x55).all())
    assert b.tolist() == [1431655765] * 5 and bool((h.view(torch.uint8) == 0x55).all()) and n.shape == (0,)
    assert c.dtype == torch.bfloat16 and not bool(c.any()) and d.requires_grad and d.is_leaf and d.tolist() == [1.0] * 4
    assert e.tolist() == [[7.5, 7.5], [7.5, 7.5]] and f.dtype == torch.int32 and f.tolist() == [3] * 3
    assert g.dtype == torch.bool and g.tolist() == [True, True]
    assert i.dtype == torch.int32 and not bool(i.any()) and bool((j == 1).all()) and bool((k == -2).all())
    assert m.requires_grad and bool((m == 4).all())
    # every payload sits between intact guards, whatever filled it
    for s in pool.slots:
        assert bool((s.raw[:G.GUARD] == 0xFF).all()) and bool((s.raw[G.GUARD + s.nbytes:] == 0xFF).all()), s.name()
    pool.check("factories")
    d.sum().backward()
    assert d.grad.tolist() == [1.0] * 4


def test_other_calls_pass_through():
    pool = G.Pool(CPU)
    out = torch.zeros(3)
    strided = torch.arange(6.0).view(2, 3).t()
    with G.guarded_allocations(pool):
        a = torch.empty(4, pin_memory=False)                             # a keyword the patch does not know
        b = torch.zeros(3, layout=torch.strided)
        c = torch.ones(3, out=out)
        d = torch.empty((2, 3), memory_format=torch.contiguous_format)
        e = torch.empty_like(strided)                                     # keeps the strides of its argument
        f = torch.zeros_like(strided, memory_format=torch.preserve_format)
        g = torch.full((2,), torch.tensor(3.0))
        h = torch.empty(3, device="meta")
        i = torch.full((2,), 1 + 2j)
        with pytest.raises(TypeError):
            torch.empty(3, no_such_argument=1)
    assert pool.served == [] and pool.slots == []
    assert a.shape == (4,) and not bool(b.any()) and c is out and out.tolist() == [1.0] * 3 and d.shape == (2, 3)
    assert e.stride() == strided.stride() and f.stride() == strided.stride() and g.tolist() == [3.0, 3.0]
    assert h.device.type == "meta" and i.dtype.is_complex


def test_a_cuda_pool_leaves_cpu_calls_alone():
    pool = G.Pool(torch.device("cuda", 0))
    with G.guarded_allocations(pool):
        a = torch.zeros(3)
        b = torch.empty_like(a)
    assert pool.served == [] and a.device.type == "cpu" and b.device.type == "cpu"


def test_assert_served():
    pool = G.Pool(CPU)
    with pytest.raises(AssertionError, match="no allocation went through"):
        G.assert_served(pool, 0, what="nothing")
    with G.guarded_allocations(pool):
        torch.empty(100, dtype=torch.uint8)
    G.assert_served(pool, 0, 100)
    with pytest.raises(AssertionError, match="no allocation of 101 bytes"):
        G.assert_served(pool, 0, 101)
    with pytest.raises(AssertionError, match="no allocation went through"):
        G.assert_served(pool, 1)
    pool.check()


def test_sizes_that_count_as_ints_go_through_the_pool():
    import numpy as np
    pool = G.Pool(CPU)
    with G.guarded_allocations(pool):
        assert G.active_pool() is pool
        a = torch.empty(np.int64(5), dtype=torch.uint8)
        b = torch.zeros((np.int32(2), 3))
        with pytest.raises(TypeError):
            torch.empty(2.5)                                              # not a size: the real factory refuses it
    assert pool.served == [5, 24] and a.shape == (5,) and b.shape == (2, 3)
    with pytest.raises(AssertionError):
        G.active_pool()


def test_slots_of_tensors_that_are_gone_are_let_go():
    pool = G.Pool(CPU)
    a, b, z = pool.empty((4,)), pool.empty((8,)), pool.empty((0,))
    pool.check("all live", release=False)
    assert len(pool.slots) == 3
    pool.forget(z)                                                        # a zero-byte slot is forgotten like any other
    assert len(pool.slots) == 2
    pool.slots[1].raw[G.GUARD - 1] = 0                                    # outside b, which is then dropped: the check still sees it
    del b
    with pytest.raises(G.GuardError, match=r"\(8,\)"):
        pool.check("b is gone", release=False)
    assert len(pool.slots) == 1 and pool.slots[0].ref() is a


def test_the_module_fixture_checks_guards_and_that_the_pool_served():
    fx = G.fixture(lambda: CPU, allocates_nothing=("test_quiet",))
    gen = fx.__wrapped__                                                  # the generator function behind pytest's fixture object

    class Node:
        def __init__(self, name):
            self.name = self.originalname = name

    class Request:
        def __init__(self, name):
            self.node = Node(name)

    it = gen(Request("test_allocates"))
    pool = next(it)
    t = torch.zeros(3)
    assert pool.served == [12]
    with pytest.raises(StopIteration):
        next(it)
    it = gen(Request("test_nothing"))
    next(it)
    with pytest.raises(AssertionError, match="no allocation went through"):
        next(it)
    it = gen(Request("test_quiet"))
    next(it)
    with pytest.raises(StopIteration):
        next(it)
    it = gen(Request("test_writes_outside"))
    pool = next(it)
    t = torch.zeros(3)
    pool.slots[0].raw[G.GUARD + 12] = 0
    with pytest.raises(G.GuardError, match="test_writes_outside"):
        next(it)
    assert torch.zeros is G._REAL["zeros"] and t.numel() == 3
