"""The key / object task loop of the multi-room generator (minigrid-rl_amd/csrc/mgx_device.h: gen_rooms' one loop over
the placement draws' ten-word passes, cell_pass) on the HOST against the C oracle, with enough lanes and episodes
(256 x 48) that every way out of the loop is taken while other placements of the same attempt are done or pending:
the live-lock word cap inside a choice, an x, a y and at a pass boundary, on a key A, a key B and on objects.
tests/host_wave/task_loop_host.cpp is the driver (the generator compiled with -DMGX_HOST_SIM, one attempt at a time);
every episode's grid, agent, target, MT19937 cursor, PCG64 state (buffer included), mission and abandoned-attempt
count must equal the oracle's.  From the driver's counts of what the abandoned attempts had placed: at every cap of 64
words and below attempts are abandoned, and where doors can be locked some of them after a key was placed.

Object counts 0, 1 and 9 (rooms without an object, rooms that cannot hold theirs: the live-lock policy fires at once)
run at 64 lanes x 12 episodes, the shape at which the parent commit's host generator and the oracle were first
established to end and to agree at these counts.  18 is not covered: there the parent's host generator sets G.err = 8
(more placements than obj_choice or the objs list holds) and its abandoned-attempt counts differ from the oracle's, so
that count has no reference to compare against.  Test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_generator_host import encode

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "minigrid-rl_amd", "csrc")
SRC = os.path.join(HERE, "host_wave", "task_loop_host.cpp")
DEPS = [SRC, os.path.join(HERE, "host_wave", "host_lane.h"), os.path.join(HERE, "host_gen", "host_sim.h"),
        os.path.join(CSRC, "mgx_device.h"), os.path.join(CSRC, "mgx_diag.h")]
LIB = os.path.join(HERE, "host_wave", "libtask_loop_host.so")

# (mission, size, all_doors_open): S 8 one 64-bit cell set, S 11 two (NW = 2), S 16 the LDS-grid path (NW = 4)
CASES = [(5, 8, 0), (None, 8, 0), (None, 8, 1), (2, 11, 0), (1, 16, 0)]
CAPS = [4096, 96, 64, 48, 40]
N, E, SEED = 256, 48, 42


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB) or any(os.path.getmtime(LIB) < os.path.getmtime(p) for p in DEPS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DMGX_HOST_SIM",
                               "-I", os.path.join(HERE, "host_gen"), "-I", CSRC, "-o", LIB, SRC])
    L = ctypes.CDLL(LIB)
    L.tl_run.argtypes = [ctypes.c_int] * 7 + [ctypes.c_int64, ctypes.c_int] + [ctypes.c_void_p] * 7
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _compare(lib, mission, size, ado, llw, nobj, n, E):
    """Every episode against the oracle; returns the abandoned-attempt counts and what the abandoned attempts had placed."""
    import oracle as O
    from mgx._lib import mission_tokens
    S = size
    grids = np.zeros((n, E, S * S), np.uint8)
    agent = np.zeros((n, E, 3), np.uint8)
    target = np.zeros((n, E, 4), np.uint8)
    cursor = np.zeros((n, E), np.int64)
    pcg = np.zeros((n, E, 4), np.uint64)
    ll = np.zeros((n, E), np.int32)
    left = np.zeros((n, E, 4), np.int32)      # abandoned attempts: with a key, with an object, with nothing, with two keys placed
    err = lib.tl_run(0, -1 if mission is None else mission, S, nobj, ado, llw, n, SEED, E,
                     _p(grids), _p(agent), _p(target), _p(cursor), _p(pcg), _p(ll), _p(left))
    assert err == 0, err
    ov = O.OracleVec("multi", mission, S, nobj, n, SEED, all_doors_open=bool(ado), livelock_words=llw)
    r = ov.reset()
    tok = mission_tokens()
    g = encode(grids, S)
    done = np.full(n, 6, np.int32)                            # 'done': ends every episode, auto-reset
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
        o = ov.step(done)
        assert (o["terminated"] | o["truncated"]).all()
    assert (left[..., :3].sum(axis=2) >= ll).all()            # every abandoned attempt counted
    return ll, left


@pytest.mark.parametrize("llw", CAPS, ids=["llw%d" % c for c in CAPS])
@pytest.mark.parametrize("mission,size,ado", CASES, ids=["m%s_s%d_ado%d" % c for c in CASES])
def test_task_loop_matches_oracle(lib, mission, size, ado, llw):
    ll, left = _compare(lib, mission, size, ado, llw, 4, N, E)
    by = left.reshape(-1, 4).sum(axis=0)
    print("llw %d: abandoned %d, with a key %d, with an object %d, with nothing %d, with two keys %d"
          % (llw, int(ll.sum()), by[0], by[1], by[2], by[3]))
    if llw <= 64:
        assert ll.sum() > 0                                   # the cap did fire
        if not ado:
            assert by[0] > 0                                  # ... also after a key of the same attempt was placed
            assert by[1] > 0                                  # ... and between the objects


@pytest.mark.parametrize("llw", [4096, 64], ids=["llw4096", "llw64"])
@pytest.mark.parametrize("nobj", [0, 1, 9], ids=["nobj0", "nobj1", "nobj9"])
@pytest.mark.parametrize("mission,size,ado", CASES, ids=["m%s_s%d_ado%d" % c for c in CASES])
def test_task_loop_other_object_counts(lib, mission, size, ado, nobj, llw):
    ll, _ = _compare(lib, mission, size, ado, llw, nobj, 64, 12)
    if nobj == 9 and size == 8:
        assert ll.sum() > 0       # nine objects do not fit every 8x8 layout: attempts abandoned without the cap
