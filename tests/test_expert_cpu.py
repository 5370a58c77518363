"""The shortest-path expert's definition (mgx.expert.expert_reference) without a GPU: optimality against an independent
Dijkstra written here, the closed loop over the C oracle, the solved share, hand-built states, and the kernel's
per-lane routine compiled for the host (tests/host_expert) against the definition.

The closed loop is the strong check: over OracleVec, every episode whose first state has cost >= 0 must end with a
positive reward after exactly `cost` steps ('go to goal', and 'go to', whose `done` completes and ends at once) or
cost + 1 steps (the other missions: the target action completes, `done` ends)."""
import ctypes
import heapq
import os
import subprocess

import numpy as np
import pytest

import oracle as O
from mgx.expert import (DONE, DROP, DV, FORWARD, LEFT, NONE, PICKUP, RIGHT, TOGGLE, expert_reference)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMPTY, WALL, DOOR, KEY, BALL, BOX, GOAL, LAVA = 1, 2, 4, 5, 6, 7, 8, 9
SINGLE = {"gtg": 5, "gto": 0, "pkp": 2, "opn": 1}


def _cfg(problem, size):
    if problem == "multi":
        return dict(problem="multi", mission=None, size=size, num_objects=4)
    return dict(problem=problem, mission=SINGLE[problem], size=size, num_objects=4 if size > 5 else 1)


# ------------------------------------------------------------------ an independent Dijkstra (none of expert.py's code)
def _enter(cell, carry):
    t, colour, state = int(cell[0]), int(cell[1]), int(cell[2])
    if t == EMPTY or (t == DOOR and state == 0):
        return 1
    if t == DOOR and (state == 1 or (int(carry[0]) == KEY and int(carry[1]) == colour)):
        return 2
    return None


def _dijkstra(grid, agent, carry, is_goal, final_cell=None):
    """Forward Dijkstra from the agent's state over (x, y, dir) -> the cost of the nearest goal state, or None."""
    S = grid.shape[0]
    start = (int(agent[0]), int(agent[1]), int(agent[2]))
    dist, heap = {start: 0}, [(0, start)]
    while heap:
        d, s = heapq.heappop(heap)
        if d > dist[s]:
            continue
        if is_goal(s):
            return d
        x, y, dr = s
        nxt = [(1, (x, y, (dr + 3) % 4)), (1, (x, y, (dr + 1) % 4))]
        nx, ny = x + DV[dr][0], y + DV[dr][1]
        if 0 <= nx < S and 0 <= ny < S:
            w = 1 if (nx, ny) == final_cell else _enter(grid[nx, ny], carry)
            if w is not None:
                nxt.append((w, (nx, ny, dr)))
        for w, s2 in nxt:
            if d + w < dist.get(s2, 1 << 30):
                dist[s2] = d + w
                heapq.heappush(heap, (d + w, s2))
    return None


def _independent_cost(st, i):
    """The mission route's cost of env i by the cost model alone (rule 4), or None when the target is out of reach or
    the env has no target cell."""
    tx, ty, ta = (int(v) for v in st["target"][i])
    if tx == NONE:
        return None
    if ta in (NONE, 0):
        return _dijkstra(st["grid"][i], st["agent"][i], st["carrying"][i], lambda s: (s[0], s[1]) == (tx, ty),
                         final_cell=(tx, ty))
    d = _dijkstra(st["grid"][i], st["agent"][i], st["carrying"][i],
                  lambda s: (s[0] + DV[s[2]][0], s[1] + DV[s[2]][1]) == (tx, ty))
    return None if d is None else d + 1


def _check_optimal(st):
    actions, cost = expert_reference(st)
    checked = 0
    for i in range(len(cost)):
        if st["mission_done"][i] or st["target"][i][0] == NONE:
            continue
        want = _independent_cost(st, i)
        if cost[i] >= 0:
            assert want == cost[i], (i, want, int(cost[i]))
            checked += 1
        elif cost[i] in (-3, -4):
            assert want is None, (i, want, int(cost[i]))          # the route was given up only because there is none
    return checked


@pytest.mark.parametrize("problem,size", [("gtg", 8), ("gto", 8), ("pkp", 8), ("opn", 8), ("multi", 8), ("multi", 11)])
def test_cost_is_optimal(problem, size):
    """expert_reference's cost equals the independent Dijkstra's wherever it is >= 0, on reset states and 10 and 30
    steps into expert play."""
    vec = O.OracleVec(n_envs=64, **_cfg(problem, size))
    vec.reset()
    checked = 0
    for t in range(31):
        st = vec.dump()
        if t in (0, 10, 30):
            checked += _check_optimal(st)
        vec.step(expert_reference(st)[0])
    assert checked > 96


# ------------------------------------------------------------------ closed loop over the oracle
_LOOPS = {}


def _closed_loop(problem, size):
    key = (problem, size)
    if key in _LOOPS:
        return _LOOPS[key]
    n, T = 64, 3 * size * size
    vec = O.OracleVec(n_envs=n, **_cfg(problem, size))
    vec.reset()
    first = np.zeros(n, np.int64)
    out = dict(episodes=0, solved=0, negative=0, planned=0, wrong=[])
    for _ in range(T):
        st = vec.dump()
        a, c = expert_reference(st)
        new = st["step_count"] == 0
        first[new] = c[new]
        o = vec.step(a)
        for i in np.nonzero(o["terminated"] | o["truncated"])[0]:
            out["episodes"] += 1
            ok = o["reward"][i] > 0
            out["solved"] += int(ok)
            if first[i] < 0:
                out["negative"] += 1
                continue
            out["planned"] += 1
            length = int(st["step_count"][i]) + 1
            ends_at_once = int(st["target"][i][2]) in (NONE, 0, DONE)
            if not ok or length != first[i] + (0 if ends_at_once else 1):
                out["wrong"].append((int(i), int(first[i]), length, bool(ok), st["target"][i].tolist()))
    _LOOPS[key] = out
    return out


@pytest.mark.parametrize("problem,size", [("gtg", 8), ("gto", 8), ("pkp", 8), ("opn", 8), ("gtg", 5), ("multi", 8),
                                          ("multi", 11), ("multi", 16)])
def test_closed_loop_lengths(problem, size):
    """64 envs x 3 S^2 steps: ALL episodes with a plan at their first state end solved in exactly the predicted
    number of steps; on the single-room problems at most 2 % of the episodes start without one."""
    r = _closed_loop(problem, size)
    print("%s %dx%d: %d episodes, %d solved, %d planned, %d without a plan at the first state"
          % (problem, size, size, r["episodes"], r["solved"], r["planned"], r["negative"]))
    assert r["episodes"] > 64 and r["planned"] > 0
    assert not r["wrong"], r["wrong"][:5]
    if problem != "multi":
        assert r["negative"] <= 0.02 * r["episodes"]


@pytest.mark.parametrize("size", [8, 11, 16])
def test_solved_share(size):
    """multi, every mission, locked doors: at least 0.95 of the episodes are solved (a sanity floor on the rules;
    0.973, 0.970 and 0.968 at 8, 11 and 16)."""
    r = _closed_loop("multi", size)
    share = r["solved"] / r["episodes"]
    print("multi %dx%d solved share %.4f (%d of %d)" % (size, size, share, r["solved"], r["episodes"]))
    assert share >= 0.95


# ------------------------------------------------------------------ hand-built states
def _state(cells, agent, target, carrying=(0, 0, 0, 0), mission_done=0, S=7):
    """One env: a walled S x S room, `cells` {(x, y): (type, colour, state, aux)} on top."""
    g = np.zeros((1, S, S, 4), np.uint8)
    g[..., 0] = EMPTY
    g[0, 0, :], g[0, S - 1, :], g[0, :, 0], g[0, :, S - 1] = (WALL, 5, 0, 0), (WALL, 5, 0, 0), (WALL, 5, 0, 0), (WALL, 5, 0, 0)
    for (x, y), c in cells.items():
        g[0, x, y] = c
    return dict(grid=g, agent=np.array([agent], np.uint8), carrying=np.array([carrying], np.uint8),
                target=np.array([target], np.uint8), mission_done=np.array([mission_done], np.uint8),
                step_count=np.zeros(1, np.int32))


def _wall_column(x, but=()):
    return {(x, y): (WALL, 5, 0, 0) for y in range(1, 6) if y not in but}


GOAL_C, LAVA_C = (GOAL, 1, 0, 0), (LAVA, 0, 0, 0)
HAND_BUILT = {
    # agent (1, 1) facing +x, goal (5, 1): four steps forward
    "straight": (_state({(5, 1): GOAL_C}, (1, 1, 0), (5, 1, NONE)), FORWARD, 4),
    "lava beside the path": (_state({(5, 1): GOAL_C, (3, 2): LAVA_C}, (1, 1, 0), (5, 1, NONE)), FORWARD, 4),
    # lava on the path: forward, right, forward, left, 3 x forward, left, forward = 9 (tie with right first: forward wins)
    "lava on the path": (_state({(5, 1): GOAL_C, (3, 1): LAVA_C}, (1, 1, 0), (5, 1, NONE)), FORWARD, 9),
    "a second goal on the path": (_state({(5, 1): GOAL_C, (3, 1): GOAL_C}, (1, 1, 0), (5, 1, NONE)), FORWARD, 9),
    # a wall column at x = 3 with a closed door at (3, 1): 1 + 2 + 1 + 1
    "closed door, only way": (_state({**_wall_column(3), (3, 1): (DOOR, 2, 1, 0), (5, 1): GOAL_C}, (1, 1, 0), (5, 1, NONE)),
                              FORWARD, 5),
    "closed door, in front": (_state({**_wall_column(3), (3, 1): (DOOR, 2, 1, 0), (5, 1): GOAL_C}, (2, 1, 0), (5, 1, NONE)),
                              TOGGLE, 4),
    # the same with a gap at (3, 2): around it is right, forward, left, 3 x forward, left, forward = 8 > 4
    "closed door beats the detour": (_state({**_wall_column(3, but=(2,)), (3, 1): (DOOR, 2, 1, 0), (5, 1): GOAL_C},
                                            (2, 1, 0), (5, 1, NONE)), TOGGLE, 4),
    # goal (4, 2); through the door at (3, 2): right, forward, left, 2, forward = 6; along the top row: 2 x forward,
    # right, forward = 4
    "closed door loses to the shorter way": (_state({(3, 2): (DOOR, 2, 1, 0), (3, 3): (WALL, 5, 0, 0), (4, 2): GOAL_C},
                                                    (2, 1, 0), (4, 2, NONE)), FORWARD, 4),
    "open door": (_state({**_wall_column(3), (3, 1): (DOOR, 2, 0, 0), (5, 1): GOAL_C}, (2, 1, 0), (5, 1, NONE)), FORWARD, 3),
    "locked door, no key anywhere": (_state({**_wall_column(3), (3, 1): (DOOR, 2, 2, 0), (5, 1): GOAL_C}, (2, 1, 0),
                                            (5, 1, NONE)), DONE, -4),
    "locked door, its key in hand": (_state({**_wall_column(3), (3, 1): (DOOR, 2, 2, 0), (5, 1): GOAL_C}, (2, 1, 0),
                                            (5, 1, NONE), carrying=(KEY, 2, 0, 0)), TOGGLE, 4),
    "locked door, another key in hand": (_state({**_wall_column(3), (3, 1): (DOOR, 2, 2, 0), (5, 1): GOAL_C}, (2, 1, 0),
                                                (5, 1, NONE), carrying=(KEY, 3, 0, 0)), RIGHT, -2),
    # its key lies at (2, 3): right (facing +y), forward to (2, 2), then pick it up
    "locked door, its key in the room": (_state({**_wall_column(3), (3, 1): (DOOR, 2, 2, 0), (5, 1): GOAL_C,
                                                 (2, 3): (KEY, 2, 0, 0)}, (2, 1, 0), (5, 1, NONE)), RIGHT, -3),
    "facing its key": (_state({**_wall_column(3), (3, 1): (DOOR, 2, 2, 0), (5, 1): GOAL_C, (2, 3): (KEY, 2, 0, 0)},
                              (2, 2, 1), (5, 1, NONE)), PICKUP, -3),
    "facing the box that holds its key": (_state({**_wall_column(3), (3, 1): (DOOR, 2, 2, 0), (5, 1): GOAL_C,
                                                  (2, 3): (BOX, 2, 0, 1)}, (2, 2, 1), (5, 1, NONE)), TOGGLE, -3),
    "a key of another colour is no help": (_state({**_wall_column(3), (3, 1): (DOOR, 2, 2, 0), (5, 1): GOAL_C,
                                                   (2, 3): (KEY, 4, 0, 0), (1, 3): (BOX, 2, 0, 0)}, (2, 2, 1),
                                                  (5, 1, NONE)), DONE, -4),
    # 'pick up' the ball at (4, 1), hand full (a box): the wall ahead, so turn to the empty cell on the right
    "full hand, front blocked": (_state({(4, 1): (BALL, 0, 0, 0)}, (1, 1, 3), (4, 1, PICKUP), carrying=(BOX, 3, 0, 0)),
                                 RIGHT, -2),
    "full hand, front empty": (_state({(4, 1): (BALL, 0, 0, 0)}, (1, 1, 0), (4, 1, PICKUP), carrying=(BOX, 3, 0, 0)),
                               DROP, -2),
    "boxed in": (_state({(4, 1): (BALL, 0, 0, 0), (2, 1): (BOX, 0, 0, 0), (1, 2): (BOX, 1, 0, 0)}, (1, 1, 0),
                        (4, 1, PICKUP), carrying=(BOX, 3, 0, 0)), DONE, -2),
    # 'pick up' with an empty hand: forward to (3, 1), then the pickup itself
    "pick up": (_state({(4, 1): (BALL, 0, 0, 0)}, (1, 1, 0), (4, 1, PICKUP)), FORWARD, 3),
    "pick up, facing it": (_state({(4, 1): (BALL, 0, 0, 0)}, (3, 1, 0), (4, 1, PICKUP)), PICKUP, 1),
    "go to, facing it": (_state({(4, 1): (BALL, 0, 0, 0)}, (3, 1, 0), (4, 1, DONE)), DONE, 1),
    "toggle the door beside": (_state({(3, 3): (DOOR, 1, 1, 0)}, (3, 2, 0), (3, 3, TOGGLE)), RIGHT, 2),
    "drop": (_state({}, (1, 1, 0), (NONE, NONE, DROP), carrying=(KEY, 1, 0, 0)), DROP, 1),
    "move": (_state({}, (1, 1, 0), (NONE, NONE, NONE), carrying=(KEY, 1, 0, 0)), DONE, -1),
    "mission done": (_state({(5, 1): GOAL_C}, (1, 1, 0), (5, 1, NONE), mission_done=1), DONE, 0),
}


@pytest.mark.parametrize("name", sorted(HAND_BUILT))
def test_hand_built(name):
    st, action, cost = HAND_BUILT[name]
    a, c = expert_reference(st)
    assert (int(a[0]), int(c[0])) == (action, cost)
    if cost > 0 and st["target"][0][0] != NONE:
        assert _independent_cost(st, 0) == cost


# ------------------------------------------------------------------ the kernel's lane routine on the host
def _host_lib():
    src = os.path.join(HERE, "host_expert", "expert_host.cpp")
    csrc = os.path.join(ROOT, "minigrid-rl_amd", "csrc")
    lib = os.path.join(HERE, "host_expert", "libexpert_host.so")
    deps = [src, os.path.join(csrc, "mgx_expert.h"), os.path.join(csrc, "mgx_device.h"),
            os.path.join(HERE, "host_gen", "host_sim.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(lib) < os.path.getmtime(p) for p in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas",
                               "-I", os.path.join(HERE, "host_gen"), "-I", csrc, "-o", lib, src])
    return ctypes.CDLL(lib)


def _codes(typ, colour, state, aux):
    """The engine's cell code (csrc/mgx_device.h) of dump-layout cells; type 0 (the empty hand) -> 0."""
    typ, colour, state, aux = (np.asarray(v).astype(np.int64) for v in (typ, colour, state, aux))
    door = typ == DOOR
    t = np.where(door & (state == 0), 11, typ)
    bit = np.where(door, state == 2, aux != 0).astype(np.int64)
    return np.where(typ == 0, 0, t | (colour << 4) | (bit << 7)).astype(np.uint8)


def _host_expert(lib, st):
    g = st["grid"]
    n, S = g.shape[0], g.shape[1]
    GS = (S * S + 15) & ~15
    grid = np.zeros((n, GS), np.uint8)
    grid[:, :S * S] = _codes(g[..., 0], g[..., 1], g[..., 2], g[..., 3]).transpose(0, 2, 1).reshape(n, -1)
    es = np.zeros((n, 16), np.uint8)                       # EnvState: ax, ay, dir, carry, ..., tx, ty, ta, mid, done
    es[:, 0:3] = st["agent"]
    c = st["carrying"]
    es[:, 3] = _codes(c[:, 0], c[:, 1], c[:, 2], c[:, 3])
    es[:, 8:11] = st["target"]
    es[:, 12] = st["mission_done"]
    act, cost = np.zeros(n, np.int32), np.zeros(n, np.int32)
    P = ctypes.c_void_p
    lib.expert_host(P(grid.ctypes.data), P(es.ctypes.data), n, S, GS, P(act.ctypes.data), P(cost.ctypes.data))
    return act, cost


@pytest.mark.parametrize("cfg", [dict(problem="gtg", mission=5, size=5, num_objects=1),
                                 dict(problem="multi", mission=None, size=6, num_objects=4),
                                 dict(problem="multi", mission=None, size=8, num_objects=4),
                                 dict(problem="multi", mission=None, size=11, num_objects=4),
                                 dict(problem="multi", mission=None, size=16, num_objects=4),
                                 dict(problem="full", mission=None, size=9, num_objects=4),
                                 dict(problem="multi", mission=5, size=8, num_objects=4, obstacles=True,
                                      percent_obstacles=0.1)], ids=lambda c: "%s%d" % (c["problem"], c["size"]))
def test_host_lane_equals_reference(cfg):
    """The kernel's board scan, layered search and rules, compiled for the host, against expert_reference: 100 envs,
    40 steps of 0.7 expert / 0.3 uniform play."""
    lib = _host_lib()
    vec = O.OracleVec(n_envs=100, **cfg)
    vec.reset()
    rng = np.random.default_rng(7)
    for t in range(41):
        st = vec.dump()
        a, c = expert_reference(st)
        ha, hc = _host_expert(lib, st)
        bad = np.nonzero((a != ha) | (c != hc))[0]
        assert bad.size == 0, (t, int(bad[0]), int(a[bad[0]]), int(c[bad[0]]), int(ha[bad[0]]), int(hc[bad[0]]))
        vec.step(np.where(rng.random(100) < 0.7, a, rng.integers(0, 7, 100)).astype(np.int32))


def test_host_lane_hand_built():
    lib = _host_lib()
    for name, (st, action, cost) in sorted(HAND_BUILT.items()):
        ha, hc = _host_expert(lib, st)
        assert (int(ha[0]), int(hc[0])) == (action, cost), name
