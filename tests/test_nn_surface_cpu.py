"""coivo_amd.nn after its split into arena.py, passes.py and sidechain.py: every name callers import from coivo_amd.nn is still there
and is the object of its new module, the networks carry the state _ArenaModule.__init__ has always set, the layer tables spell the
topology the channel constants do, and Program.run_with_marks replays a program with hook points in the order the data-parallel
path relies on."""
import pytest
import torch

from coivo_amd import arena, nn as hnn, passes, program, sidechain

MOVED = {arena: ("ConvParams",),
         passes: ("_PassInst", "_Lease", "_dealias"),
         sidechain: ("_SIDE_PRIORITY", "_side_stream", "_shared_side", "share_side_stream", "unshare_side_stream")}
KEPT = ("ENC_CH", "DEC_CH", "POSE_CH", "_ArenaModule", "_conv", "DepthNet", "_PairDepth", "PoseNet", "_DepthNetFn", "_DepthNetPairFn",
        "_PoseNetFn", "dcdp_forward", "Program", "ops", "_lib", "np", "os", "torch", "nn", "Callable", "Dict", "List", "Optional", "Tuple")
METHODS = {arena.Arena: ("_layers", "_build_arena", "_apply", "attach_grads", "zero_grad", "mark_params_changed", "_weights_version",
                         "_prepare_weights", "operand_layout", "operands_written", "_ensure_operand_buffers", "_grads_clean",
                         "_take_arena_zero", "_arena_zero_for_pass"),
           passes.RecordedPasses: ("clear_programs", "_acquire", "_run_pass"),
           sidechain.SideChain: ("_bwd_begin", "_run_wgrad", "_conv_wgrad", "_wgrad_flush", "_bwd_end", "_queue_join", "join_side",
                                 "_order_deterministic_pass", "_layer_done")}
# what _ArenaModule.__init__ sets, with the defaults of a process without developer switches
STATE = {"_packed_version": None, "_manual_version": 0, "_pack_table": None, "_pack_dtype": None, "_side": None, "_plans": {},
         "_insts": {}, "use_programs": True, "_rec": None, "overlap_wgrad": True, "defer_join": True, "_join_pending": False,
         "_cap_side_open": False, "grad_ready_hook": None, "deterministic": False, "group_wgrad": False,
         "wgrad_group_bytes": 6 << 20, "_group": [], "_group_bytes": 0,
         # class-level defaults the instances read until a pass sets them
         "_arena_zero_for_pass": False, "_clean_flag": False, "_clean_version": -1, "_clean_in_capture": False,
         "_stored_pass_open": False, "_grads_clean": False}


def test_names_resolve_from_nn_and_are_the_moved_objects():
    for mod, names in MOVED.items():
        for name in names:
            assert getattr(hnn, name) is getattr(mod, name), name
    for name in KEPT:
        assert hasattr(hnn, name), name
    from coivo_amd.nn import _ArenaModule       # as optim.py does
    assert issubclass(hnn.DepthNet, _ArenaModule) and issubclass(hnn.PoseNet, _ArenaModule)
    assert issubclass(_ArenaModule, (arena.Arena, passes.RecordedPasses, sidechain.SideChain, torch.nn.Module))
    for part, names in METHODS.items():
        for name in names:
            assert getattr(_ArenaModule, name) is getattr(part, name), name


@pytest.mark.parametrize("cls", ["DepthNet", "PoseNet"])
def test_networks_carry_the_base_state_with_its_defaults(cls, monkeypatch):
    for var in ("COLVO_DEV", "COLVO_DETERMINISTIC"):
        monkeypatch.delenv(var, raising=False)
    net = getattr(hnn, cls)(device="cpu")
    assert net.compute_dtype == torch.float32
    assert net.flat_param.shape == net.flat_grad.shape and net.flat_param.dtype == net.flat_grad.dtype == torch.float32
    for name, default in STATE.items():
        assert getattr(net, name) == default, name
        assert type(getattr(net, name)) is type(default), name
    with pytest.raises(TypeError):
        getattr(hnn, cls)(compute_dtype=torch.float16, device="cpu")


def test_layer_tables_spell_the_channel_constants():
    rows = {r[0]: r for r in hnn.DEPTH_LAYERS}
    cin = 3
    for i, c in enumerate(hnn.ENC_CH, start=1):
        assert rows[f"enc{i}a"][1:4] == (cin, c, "s2") and rows[f"enc{i}b"][1:4] == (c, c, "plain")
        cin = c
    for i in range(5, 0, -1):
        d, skip = hnn.DEC_CH[i - 1], hnn.ENC_CH[i - 2] if i >= 2 else 0
        assert rows[f"up{i}"][1:4] == (cin, d, "up") and rows[f"iconv{i}"][1:4] == (d + skip, d, "cat")
        assert rows[f"iconv{i}"][4] == ((f"up{i}", f"enc{i - 1}b") if i >= 2 else ("up1",))
        cin = d
    assert rows["head"][1:4] == (cin, 1, "head")
    cin = 8
    for i, c in enumerate(hnn.POSE_CH, start=1):
        assert hnn.POSE_LAYERS[i - 1][:4] == (f"conv{i}", cin, c, "s2")
        cin = c
    assert hnn.POSE_LAYERS[-1][:4] == ("pred", cin, 8, "head") and hnn.PoseNet(device="cpu").pred.k == 1


# ---- Program.run_with_marks: the expected sequences are read off the replay loop this method was moved out of ---------------- #
class _Stub(program.Program):
    """A recorded program of 12 commands with hook points behind commands 3, 5 and 9; run() logs its range instead of launching."""

    def __init__(self, log):
        super().__init__()
        self.log = log
        self.marks = [(3, ("L1", False)), (5, ("L2", True)), (9, ("L3", False))]

    def run(self, side, begin=0, end=None):
        self.log.append((begin, end))


def _replay(pr, log, launches):
    """One replay with a hook that reports a launch at the layers in `launches` (a dict value None = a hook without an answer)."""
    del log[:]

    def call(L, on_side):
        log.append(L)
        return launches.get(L, False)
    pr.run_with_marks("side", call)
    return list(log)


EVERY_MARK = [(0, 3), "L1", (3, 5), "L2", (5, 9), "L3", (9, None)]


def test_hook_split_replay_learns_where_the_hook_launches():
    log = []
    pr = _Stub(log)
    assert pr.flush is None and pr.deferred_join is False
    assert _replay(pr, log, {"L2": True}) == EVERY_MARK             # first replay: split after every mark
    assert pr.flush == [False, True, False]
    grouped = [(0, 5), "L1", "L2", (5, 9), "L3", (9, None)]
    assert _replay(pr, log, {"L2": True}) == grouped                # split only where the hook launched; hooks still in order
    assert pr.flush == [False, True, False]
    assert _replay(pr, log, {"L2": True, "L3": True}) == grouped    # a launch at an unexpected mark ...
    assert pr.flush is None
    assert _replay(pr, log, {"L2": True}) == EVERY_MARK             # ... and every mark is split again
    assert pr.flush == [False, True, False]
    # (unexpected inside a group: the same ranges, L1 and L2 in order, learning re-armed)
    seq = _replay(pr, log, {"L1": True, "L2": True})
    assert seq[:4] == [(0, 5), "L1", "L2", (5, 9)] and seq[-1] == (9, None) and pr.flush is None


def test_hook_without_an_answer_counts_as_launching():
    log = []
    pr = _Stub(log)
    assert _replay(pr, log, {"L1": None, "L2": None, "L3": None}) == EVERY_MARK
    assert pr.flush == [True, True, True]
    assert _replay(pr, log, {"L1": None, "L2": None, "L3": None}) == EVERY_MARK
    assert pr.flush == [True, True, True]


def test_one_run_without_marks_or_without_a_hook():
    log = []
    pr = _Stub(log)
    pr.marks = []
    assert _replay(pr, log, {}) == [(0, None)]
    # no hook: _run_pass replays the whole program with one run(side), marks or not
    net = hnn.PoseNet(device="cpu")
    inst = passes._PassInst()
    inst.passes["fwd"] = (_Stub(log), "recorded result")
    del log[:]
    assert net.grad_ready_hook is None and net._run_pass(inst, "fwd", {}, None) == "recorded result"
    assert log == [(0, None)]
