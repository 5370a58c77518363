"""The placement draws of the multi-room generator (minigrid-rl_amd/csrc/mgx_device.h: draw_cell and the key /
object task loop, the goal / agent loop) on the HOST against the C oracle, at live-lock word caps small enough
that the cap fires inside the placement draws: inside a choice, an x, a y, and at the ten-word pass boundaries
(at 48 words about one attempt in ten is abandoned).  tests/host_wave/placement_host.cpp is the driver (the
generator compiled with -DMGX_HOST_SIM, `livelock_words` an argument); every episode's grid, agent, target,
MT19937 cursor, PCG64 state and abandoned-attempt count must equal the oracle's.  Test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_generator_host import encode

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "minigrid-rl_amd", "csrc")
SRC = os.path.join(HERE, "host_wave", "placement_host.cpp")
DEPS = [SRC, os.path.join(HERE, "host_wave", "host_lane.h"), os.path.join(HERE, "host_gen", "host_sim.h"),
        os.path.join(CSRC, "mgx_device.h"), os.path.join(CSRC, "mgx_diag.h")]
LIB = os.path.join(HERE, "host_wave", "libplacement_host.so")

# (mission, size, all_doors_open): S 8 one 64-bit cell set, S 11 two (NW = 2), S 16 the LDS-grid path (NW = 4)
CASES = [(5, 8, 0), (None, 8, 0), (None, 8, 1), (2, 11, 0), (1, 16, 0)]
CAPS = [4096, 96, 64, 48]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB) or any(os.path.getmtime(LIB) < os.path.getmtime(p) for p in DEPS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DMGX_HOST_SIM",
                               "-I", os.path.join(HERE, "host_gen"), "-I", CSRC, "-o", LIB, SRC])
    L = ctypes.CDLL(LIB)
    L.pd_run.argtypes = [ctypes.c_int] * 7 + [ctypes.c_int64, ctypes.c_int] + [ctypes.c_void_p] * 6
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("llw", CAPS, ids=["llw%d" % c for c in CAPS])
@pytest.mark.parametrize("mission,size,ado", CASES, ids=["m%s_s%d_ado%d" % c for c in CASES])
def test_placement_draws_match_oracle(lib, mission, size, ado, llw):
    import oracle as O
    from mgx._lib import mission_tokens
    n, E, seed, S = 64, 24, 42, size
    grids = np.zeros((n, E, S * S), np.uint8)
    agent = np.zeros((n, E, 3), np.uint8)
    target = np.zeros((n, E, 4), np.uint8)
    cursor = np.zeros((n, E), np.int64)
    pcg = np.zeros((n, E, 4), np.uint64)
    ll = np.zeros((n, E), np.int32)
    err = lib.pd_run(0, -1 if mission is None else mission, S, 4, ado, llw, n, seed, E,
                     _p(grids), _p(agent), _p(target), _p(cursor), _p(pcg), _p(ll))
    assert err == 0, err
    ov = O.OracleVec("multi", mission, S, 4, n, seed, all_doors_open=bool(ado), livelock_words=llw)
    r = ov.reset()
    tok = mission_tokens()
    g = encode(grids, S)
    o = None
    for k in range(E):
        d = ov.dump()
        assert np.array_equal(ll[:, k], r["livelock"] if k == 0 else o["livelock"]), ("livelock", k)
        assert np.array_equal(cursor[:, k], d["mtwords"]), ("mt cursor", k)
        assert np.array_equal(g[:, k], d["grid"]), ("grid", k)
        assert np.array_equal(agent[:, k], d["agent"]), ("agent", k)
        assert np.array_equal(target[:, k, :3], d["target"]), ("target", k)
        assert np.array_equal(pcg[:, k, 0], d["pcg"][:, 0]) and np.array_equal(pcg[:, k, 1], d["pcg"][:, 1]), ("pcg", k)
        assert np.array_equal(pcg[:, k, 2], d["pcg"][:, 4]) and np.array_equal(pcg[:, k, 3], d["pcg"][:, 5]), ("pcg buf", k)
        assert np.array_equal(tok[target[:, k, 3]], r["mission"] if k == 0 else o["r_mission"]), ("mission", k)
        o = ov.step(np.full(n, 6, np.int32))                  # 'done': ends every episode, auto-reset
        assert (o["terminated"] | o["truncated"]).all()
    if llw == 48:
        assert ll.sum() > 0                                   # the cap did fire
