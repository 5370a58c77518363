"""The refill wave-cost model (tools/refill_wave_model.cpp, .py) builds, and the lanes it runs attempt by attempt,
grouped in waves, consume exactly the MT19937 words the plain host generator (tests/host_gen: reset_env, one env
after the other) consumes for the same envs and episodes; its union counts are no less than its lane means."""
import importlib.util
import os

import numpy as np
import pytest

from test_generator_host import _lib, _p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    spec = importlib.util.spec_from_file_location("refill_wave_model", os.path.join(ROOT, "tools", "refill_wave_model.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m, m.build_binary()


@pytest.mark.parametrize("mission,size,wave", [(5, 8, 64), (-1, 8, 32), (2, 11, 64)])
def test_wave_model_lanes_consume_the_generators_words(model, tmp_path, mission, size, wave):
    m, binary = model
    n, E, seed, S = 160, 6, 42, size
    cur = str(tmp_path / "cursors.txt")
    res = m.run_model(binary, mission, size, n, E, wave, 4096, cursors=cur)
    assert res["err"] == 0 and res["lane_attempts"] == n * E + res["abandoned"]
    got = np.loadtxt(cur, dtype=np.int64)
    L = _lib()
    grids = np.zeros((n, E, S * S), np.uint8)
    agent = np.zeros((n, E, 3), np.uint8)
    target = np.zeros((n, E, 4), np.uint8)
    cursor = np.zeros((n, E), np.int64)
    pcg = np.zeros((n, E, 4), np.uint64)
    ll = np.zeros((n, E), np.int32)
    assert L.hg_run(0, mission, S, 4, 0, 0, n, seed, E, _p(grids), _p(agent), _p(target), _p(cursor), _p(pcg), _p(ll)) == 0
    assert np.array_equal(got, cursor[:, E - 1])
    assert int(ll.sum()) == res["abandoned"]
    for k, v in res["lane_mean"].items():
        assert res["wave_union"][k] >= v - 1e-9, k
    assert res["wave_union"]["tail_entries"] == 0              # no word-by-word tail left
    priced = m.price(res, "r07")
    assert priced["valu_per_round"] > 0 and priced["salu_per_round"] > 0
