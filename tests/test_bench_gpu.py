"""-m gpu: bench.py --dump-outputs writes the same files in every run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out, extra_env):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **extra_env)
    env.pop("COLVO_DETERMINISTIC", None)           # bench.py itself has to make the timed step deterministic
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "2", "--batch-per-gpu", "2", "--height", "64",
           "--width", "96", "--no-cpu-baseline", "--no-roofline-cfg2", "--no-side-measurements", "--graph", "best",
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_bench_dump_outputs_repeat_bit_for_bit(tmp_path):
    """Two runs with the same arguments, the second with its graph trial forced to capture, run 20 more replayed steps and keep the
    replay for the timed steps (COLVO_BENCH_GRAPH_THRESHOLD=0).  bench.py puts parameters and optimizer state back after the trial,
    and the deterministic step computes the same bits eagerly and replayed, so both runs write the same files; loss.npy is the
    loss of the last timed step (the JSON line's final_loss)."""
    a = _bench(tmp_path / "a", {})
    b = _bench(tmp_path / "b", {"COLVO_BENCH_GRAPH_THRESHOLD": "0"})
    assert b["hipgraph"] and a["deterministic_weight_gradients"] and b["deterministic_weight_gradients"]
    assert a["first_loss"] == b["first_loss"] and a["final_loss"] == b["final_loss"]
    for f in ("loss.npy", "depth_net_params.npy", "pose_net_params.npy"):
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float32 and np.array_equal(x, y), f
    assert np.load(tmp_path / "a" / "loss.npy")[0] == np.float32(a["final_loss"])
