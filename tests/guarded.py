"""Guard bands and poisoned scratch: one allocator for the tests that hold a kernel to its own memory.

Every tensor a Pool hands out is a view into a private uint8 buffer laid out as

    GUARD bytes of 0xFF | payload | 0xFF up to the next multiple of 16 | GUARD bytes of 0xFF

GUARD is a multiple of 512, so a payload keeps the alignment the torch allocator gives the buffer.  0xFF bytes read as NaN in bf16 and
fp32 and as -1 in int32: a load from a guard that reaches arithmetic poisons the result, and the bit-exact comparison the test already
makes fails.  A store into a guard is found by Pool.check, which names the slot, the side and the first changed byte.

Payloads of Pool.empty start out as the pool's POISON byte, 0xFF or 0x55 (bf16 / fp32: a large finite number, int32: 1 431 655 765).  A
kernel that reads scratch it never wrote, or leaves part of an output unwritten, gives different bits under the two poisons, or NaN.

guarded_allocations(pool) routes the Python-level factories (torch.empty / zeros / ones / full and their *_like forms) through the pool
for its duration, so the workspaces and outputs a wrapper allocates for itself are guarded and poisoned as well."""
import contextlib
import math
import operator
import weakref

import torch

GUARD = 4096                      # bytes in front of and behind every payload
GUARD_BYTE = 0xFF
POISONS = (0xFF, 0x55)

_FACTORIES = ("empty", "zeros", "ones", "full")
_NAMES = _FACTORIES + tuple(n + "_like" for n in _FACTORIES)
_REAL = {n: getattr(torch, n) for n in _NAMES}          # the factories themselves: what the pool allocates with, patched or not


class GuardError(AssertionError):
    pass


class _Slot:
    __slots__ = ("raw", "nbytes", "shape", "dtype", "label", "ref")

    def __init__(self, raw, nbytes, shape, dtype, label, t):
        self.raw, self.nbytes, self.shape, self.dtype, self.label = raw, nbytes, shape, dtype, label
        self.ref = weakref.ref(t)          # the tensor handed out: once it is gone the slot can go after its next check

    def name(self):
        return f"{tuple(self.shape)} {self.dtype}" + (f" '{self.label}'" if self.label else "")


def _shape_of(shape):
    if isinstance(shape, int):
        return (shape,)
    return tuple(int(s) for s in shape)


class Pool:
    """Guarded allocations on one device.  `served`: the byte size of every payload handed out since the pool was made (check() does
    not clear it)."""

    def __init__(self, device, poison=GUARD_BYTE):
        self.device = torch.device(device)
        self.poison = int(poison)
        self.slots = []
        self.served = []

    def _carve(self, shape, dtype, fill_byte, label):
        shape = _shape_of(shape)
        nbytes = math.prod(shape) * _REAL["empty"]((), dtype=dtype).element_size()
        total = GUARD + (nbytes + 15) // 16 * 16 + GUARD
        raw = _REAL["full"]((total,), GUARD_BYTE, dtype=torch.uint8, device=self.device)
        payload = raw[GUARD:GUARD + nbytes]
        if fill_byte is not None and fill_byte != GUARD_BYTE and nbytes:
            payload.fill_(fill_byte)
        t = payload.view(dtype).view(shape)
        assert t.is_contiguous() and (nbytes == 0 or t.data_ptr() == raw.data_ptr() + GUARD)
        self.slots.append(_Slot(raw, nbytes, shape, dtype, label, t))
        self.served.append(nbytes)
        return t

    def empty(self, shape, dtype=torch.float32, poison=None, label=""):
        """A contiguous tensor whose every byte is `poison` (default: the pool's)."""
        return self._carve(shape, dtype, self.poison if poison is None else int(poison), label)

    def filled(self, shape, value, dtype=torch.float32, label=""):
        t = self._carve(shape, dtype, None, label)
        if t.numel():
            t.fill_(value)
        return t

    def place(self, t, label=""):
        """A contiguous copy of `t` (None stays None) in a guarded slot."""
        if t is None:
            return None
        out = self._carve(t.shape, t.dtype, None, label)
        if out.numel():
            out.copy_(t.detach())
        return out

    def place_tree(self, x, label=""):
        """`x` with every tensor in it placed: tuples, named tuples, lists and dicts are rebuilt, everything else is passed on."""
        if torch.is_tensor(x):
            return self.place(x, label)
        if isinstance(x, dict):
            return {k: self.place_tree(v, f"{label}[{k!r}]") for k, v in x.items()}
        if isinstance(x, tuple) and hasattr(x, "_fields"):
            return type(x)(*(self.place_tree(v, f"{label}.{n}") for n, v in zip(x._fields, x)))
        if isinstance(x, (tuple, list)):
            return type(x)(self.place_tree(v, f"{label}[{i}]") for i, v in enumerate(x))
        return x

    def forget(self, *tensors):
        """Release the slots of these tensors (None is skipped) without a check: they are about to be freed."""
        gone = [t for t in tensors if t is not None]
        self.slots = [s for s in self.slots if not any(s.ref() is t for t in gone)]

    def check(self, what="", release=True):
        """Synchronise, then every guard byte of every live slot must still be GUARD_BYTE.  Releases the slots it checked; with
        release=False only those whose tensor no longer exists, so that operands and scratch that outlive one launch are checked again
        next time and what a test has dropped gives its memory back."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        slots = self.slots
        self.slots = [] if release else [s for s in slots if s.ref() is not None]
        if not slots:
            return
        flags = []
        for s in slots:
            front = s.raw[:GUARD].view(torch.int64)
            flags.append((front != -1).any() | (s.raw[GUARD + s.nbytes:] != GUARD_BYTE).any())
        bad = torch.stack(flags).cpu()
        if not bool(bad.any()):
            return
        lines = []
        for s, b in zip(slots, bad.tolist()):
            if not b:
                continue
            for side, lo, hi in (("front", 0, GUARD), ("back", GUARD + s.nbytes, s.raw.numel())):
                hit = (s.raw[lo:hi] != GUARD_BYTE).nonzero().flatten().cpu()
                if hit.numel():
                    first, last = int(hit[0]) + lo - GUARD, int(hit[-1]) + lo - GUARD
                    lines.append(f"slot {s.name()}: {side} guard written: {hit.numel()} bytes, first at payload offset {first} "
                                 f"(payload is {s.nbytes} bytes), last at {last}")
        raise GuardError((what + ": " if what else "") + "; ".join(lines))

    def total_served(self):
        return sum(self.served)


# --------------------------------------------------------------------------------------------------------------------------------- #
# the patch                                                                                                                           #
# --------------------------------------------------------------------------------------------------------------------------------- #
def _same_device(pool, device):
    """Whether `device` (None: torch's default) names the pool's device."""
    if device is None:
        device = torch.get_default_device() if hasattr(torch, "get_default_device") else torch.device("cpu")
    try:
        device = torch.device(device)
    except (TypeError, RuntimeError):
        return False
    if device.type != pool.device.type:
        return False
    if device.type != "cuda":
        return True
    cur = torch.cuda.current_device()
    return (cur if device.index is None else device.index) == (cur if pool.device.index is None else pool.device.index)


_ACTIVE = []


def active_pool():
    """The pool of the innermost guarded_allocations block that is running (an error outside one)."""
    assert _ACTIVE, "no guarded_allocations block is active"
    return _ACTIVE[-1]


def _capturing(pool):
    return pool.device.type == "cuda" and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def _parse_sizes(args, kw):
    """The sizes of a factory call given as ints, one sequence or size=; None where they are anything else."""
    if "size" in kw:
        if args:
            return None
        args = (kw.pop("size"),)
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        args = tuple(args[0])
    try:                                   # ints and whatever counts as one (a NumPy integer, a ctypes query's result), not bools or floats
        sizes = tuple(operator.index(a) for a in args if not isinstance(a, bool))
    except TypeError:
        return None
    if len(sizes) != len(args) or any(a < 0 for a in sizes):
        return None
    return sizes


def _fill_dtype(value):
    if isinstance(value, bool):
        return torch.bool
    if isinstance(value, int):
        return torch.int64
    if isinstance(value, float):
        return torch.get_default_dtype()
    return None


def _make(pool, kind, shape, dtype, value, requires_grad):
    if kind == "empty":
        t = pool.empty(shape, dtype, label="torch.empty")
    else:
        t = pool.filled(shape, {"zeros": 0, "ones": 1}.get(kind, value), dtype, label="torch." + kind)
    return t.requires_grad_(True) if requires_grad else t


def _wrap(pool, kind, real):
    def factory(*orig, **kwargs):
        args, kw = orig, dict(kwargs)
        dtype, device, rg = kw.pop("dtype", None), kw.pop("device", None), kw.pop("requires_grad", False)
        value = None
        if kind == "full":
            if "fill_value" in kw:
                value = kw.pop("fill_value")
            elif len(args) == 2:
                args, value = args[:1], args[1]
            else:
                return real(*orig, **kwargs)
            if dtype is None:
                dtype = _fill_dtype(value)
            if not isinstance(value, (bool, int, float)) or dtype is None:
                return real(*orig, **kwargs)
        shape = _parse_sizes(args, kw)
        if kw or shape is None or type(rg) is not bool or not _same_device(pool, device) or _capturing(pool):
            return real(*orig, **kwargs)
        if dtype is None:
            dtype = torch.get_default_dtype()
        if not isinstance(dtype, torch.dtype) or dtype.is_complex:
            return real(*orig, **kwargs)
        return _make(pool, kind, shape, dtype, value, rg)
    factory.__name__ = kind
    return factory


def _wrap_like(pool, kind, real):
    def factory(*orig, **kwargs):
        args, kw = orig, dict(kwargs)
        dtype, device, rg = kw.pop("dtype", None), kw.pop("device", None), kw.pop("requires_grad", False)
        value = None
        if kind == "full" and len(args) == 1 and "fill_value" in kw:
            value = kw.pop("fill_value")
        elif kind == "full" and len(args) == 2:
            args, value = args[:1], args[1]
        like = args[0] if len(args) == 1 else None
        plain = (torch.is_tensor(like) and like.layout == torch.strided and like.is_contiguous() and not like.is_quantized
                 and (kind != "full" or isinstance(value, (bool, int, float))))
        if not plain or kw or type(rg) is not bool or _capturing(pool):
            return real(*orig, **kwargs)
        dtype = like.dtype if dtype is None else dtype
        if not _same_device(pool, like.device if device is None else device) or not isinstance(dtype, torch.dtype) or dtype.is_complex:
            return real(*orig, **kwargs)
        return _make(pool, kind, tuple(like.shape), dtype, value, rg)
    factory.__name__ = kind + "_like"
    return factory


@contextlib.contextmanager
def guarded_allocations(pool, poison=None):
    """torch.empty / zeros / ones / full and their *_like forms allocate from `pool` while the block runs, where the call asks for a
    plain dense tensor on the pool's device (sizes, dtype, device, requires_grad); every other call -- further keyword arguments, out=,
    pinned memory, another device, a stream that is being captured -- goes to the real factory untouched.  empty payloads hold the
    poison byte (`poison` sets the pool's), zeros / ones / full their value; the guards are 0xFF either way."""
    if poison is not None:
        pool.poison = int(poison)
    saved = {n: getattr(torch, n) for n in _NAMES}
    try:
        _ACTIVE.append(pool)
        for kind in _FACTORIES:
            setattr(torch, kind, _wrap(pool, kind, saved[kind]))
            setattr(torch, kind + "_like", _wrap_like(pool, kind, saved[kind + "_like"]))
        yield pool
    finally:
        if _ACTIVE and _ACTIVE[-1] is pool:
            _ACTIVE.pop()
        for n, f in saved.items():
            setattr(torch, n, f)


def fixture(device, allocates_nothing=()):
    """An autouse pytest fixture for a test module: `_guarded = guarded.fixture(dev)`.  Every test of the module runs inside
    guarded_allocations on a pool of its own (device(): the module's device, asked for when the test starts), so every tensor the test
    makes with torch.empty / zeros / ones / full or a *_like form, and every scratch the ops allocate for themselves, lies between
    guard bands, what torch.empty gives filled with 0xFF bytes (NaN).  Operands a test wants guarded it places itself:
    guarded.active_pool().place(t).  The guards of everything still in the pool are checked when the test is over -- a test that
    frees large tensors on the way calls active_pool().check(release=False), which checks everything and lets go of what is gone --
    and the pool must have served something: a module the patch does not reach fails.  allocates_nothing: the names of the tests
    that make no device tensor this way."""
    import pytest

    @pytest.fixture(autouse=True)
    def _guarded_allocations(request):
        pool = Pool(device())
        with guarded_allocations(pool):
            yield pool
        pool.check(f"{request.node.name}: a kernel wrote outside a destination or a scratch")
        if request.node.originalname not in allocates_nothing:
            assert pool.served, f"{request.node.name}: no allocation went through the pool"
    return _guarded_allocations


def assert_served(pool, since, nbytes=None, what=""):
    """The pool served at least one allocation after its first `since`, and -- with nbytes -- one of exactly that many bytes (a
    workspace sized by its query): a call the patch did not reach must fail, not pass."""
    got = pool.served[since:]
    assert got, f"{what}: no allocation went through the pool"
    if nbytes is not None:
        assert int(nbytes) in got, f"{what}: no allocation of {int(nbytes)} bytes among {sorted(set(got))}"


# --------------------------------------------------------------------------------------------------------------------------------- #
# one call under both poisons                                                                                                         #
# --------------------------------------------------------------------------------------------------------------------------------- #
def _leaves(x, path, out):
    if torch.is_tensor(x):
        out.append((path, x))
    elif isinstance(x, dict):
        for k in x:
            _leaves(x[k], f"{path}[{k!r}]", out)
    elif isinstance(x, (tuple, list)):
        names = getattr(x, "_fields", None)
        for i, v in enumerate(x):
            _leaves(v, f"{path}.{names[i]}" if names else f"{path}[{i}]", out)
    elif hasattr(x, "__array_interface__"):
        out.append((path, torch.from_numpy(x.copy())))
    elif isinstance(x, float):
        out.append((path, torch.tensor(x, dtype=torch.float64)))
    else:
        out.append((path, x))
    return out


def assert_same_bits(a, b, what=""):
    """Two results of one call (tensors, numbers, None; tuples, named tuples, lists and dicts of them) are the same bytes: NaN equals
    the same NaN, -0.0 is not +0.0."""
    la, lb = _leaves(a, "out", []), _leaves(b, "out", [])
    assert [p for p, _ in la] == [p for p, _ in lb], f"{what}: the results differ in structure"
    for (path, x), (_, y) in zip(la, lb):
        if torch.is_tensor(x):
            assert torch.is_tensor(y) and x.shape == y.shape and x.dtype == y.dtype, f"{what}: {path}: shape or dtype differs"
            if x.numel() == 0:
                continue
            xb, yb = (t.detach().contiguous().reshape(-1).view(torch.uint8) for t in (x, y))
            same = xb == yb
            if not bool(same.all()):
                first = int((~same).nonzero()[0]) // x.element_size()
                raise AssertionError(f"{what}: {path} {tuple(x.shape)} {x.dtype} depends on the poison: {int((~same).sum())} bytes differ, "
                                     f"first at flat element {first} ({x.reshape(-1)[first].item()!r} / {y.reshape(-1)[first].item()!r})")
        else:
            assert x == y, f"{what}: {path}: {x!r} / {y!r}"


def under_both_poisons(device, fn, what=""):
    """fn(pool) once per poison, each inside guarded_allocations on a pool of its own; fn places its inputs with pool.place.  The guards of
    everything allocated must be intact after each call, at least one allocation must have gone through the pool, and the two results
    must be the same bytes.  Returns ([result under 0xFF, result under 0x55], [the two pools]) for the caller's own comparison with its
    reference and for assert_served."""
    outs, pools = [], []
    for poison in POISONS:
        pool = Pool(device, poison)
        with guarded_allocations(pool):
            out = fn(pool)
        pool.check(f"{what}, poison {poison:#04x}")
        assert_served(pool, 0, None, f"{what}, poison {poison:#04x}")
        outs.append(out)
        pools.append(pool)
    assert_same_bits(outs[0], outs[1], what)
    return outs, pools
