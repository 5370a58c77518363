"""bench.py's plain command line on the GPU: `--gpus 1 --steps K --warmup W --dump-outputs DIR` times exactly K
steps, prints one JSON line with `ms_per_step`, leaves what --full measures out, and writes the last timed
horizon's arrays -- float32 / float64, small, and the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, N, SAMPLE = 20, 65536, 1024


def _bench(d):
    """The plain 20-step command in a process of its own, dumping into `d`: its result line."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K),
                        "--warmup", "5", "--dump-outputs", d], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def first(tmp_path_factory):
    """One run shared by the tests below: (result line, dump directory)."""
    d = str(tmp_path_factory.mktemp("dump0"))
    return _bench(d), d


@pytest.mark.gpu
def test_plain_run_prints_the_headline_line_only(first):
    line, _ = first
    assert line["steps"] == K and line["unit"] == "env-steps/s" and line["higher_is_better"] is True
    assert line["dtype"] == "u8" and line["n_gpus"] == 1 and line["full"] is False
    # value is the K timed steps of all N envs over the region's wall time, ms_per_step that time per step
    assert line["ms_per_step"] > 0
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 / N - 1.0) < 1e-9
    assert line["window"]["episodes_consumed"] > 0 and line["roofline"]["timed_launches"] >= 1
    for moved in ("cpu_baseline", "compact_layout", "sb3_layout", "gae", "steady_state"):
        assert line.get(moved) is None, moved
    assert line["roofline"]["probe_launches"] == 0 and line["roofline"]["rocprof"] is None


@pytest.mark.gpu
def test_dump_outputs_are_float_arrays_of_the_last_horizon_and_repeat(first, tmp_path):
    line, d0 = first
    d1 = str(tmp_path)
    _bench(d1)                                             # a second run, a process of its own
    names = sorted(os.listdir(d0))
    assert names == sorted(n + ".npy" for n in line["outputs"]["arrays"]) == sorted(os.listdir(d1))
    a = {n[:-4]: np.load(os.path.join(d0, n)) for n in names}
    assert sum(os.path.getsize(os.path.join(d0, n)) for n in names) <= 64 * 2 ** 20
    for n, x in a.items():
        assert x.dtype == (np.float64 if n == "adv_stats" else np.float32), n
        assert list(x.shape) == line["outputs"]["arrays"][n] and np.isfinite(x).all(), n
        assert np.array_equal(x, np.load(os.path.join(d1, n + ".npy"))), n      # same inputs, same arrays
    H = line["config"]["horizon"]
    for n in ("rewards", "dones", "advantages", "returns"):
        assert a[n].shape == (H, SAMPLE), n
    ix = a["env_index"]
    assert ix.shape == (SAMPLE,) and (np.diff(ix) > 0).all() and 0 <= ix[0] and ix[-1] < N
    assert a["adv_stats"][2] == H * N                      # the horizon's GAE saw every env-step
    assert set(np.unique(a["dones"])) <= {0.0, 1.0} and 0 < a["dones"].sum() < a["dones"].size
    assert ((a["rewards"] >= 0) & (a["rewards"] <= 1)).all()
    # reward > 0 only on a step that ended its episode (GTG: reaching the goal)
    assert (a["dones"][a["rewards"] > 0] == 1).all()
    rows = a["obs_rows"]
    assert rows.shape == (min(H, 16), SAMPLE, 148) and a["mission_ids"].shape == rows.shape[:2]
    assert (rows == np.round(rows)).all() and rows.min() >= 0 and rows.max() <= 255
    assert (rows[..., 0] <= 3).all()                       # byte 0: the agent's direction
    assert len(np.unique(rows.reshape(-1, 148), axis=0)) > SAMPLE     # the envs are in different states
