"""The scripted agent (tests/golden/scripted_agent.py) is a function of the env state alone, so running it
again over the C oracle must give back the actions that were stored when it ran over the oracle (the action
scripts, tests/golden/actions) and over the reference (the deep_* fixtures).  The second ties the block-scale
scripts, which no reference run backs, to the reference: same agent, same states, same actions."""
import os
import sys

import numpy as np
import pytest

import trajcheck as TC

sys.path.insert(0, TC.GOLDEN)

import scripted_agent as SA  # noqa: E402

SCRIPTS = {"multi_all_s8": (520, 160), "multi_tgl_s16": (520, 288), "full_s8": (200, 160)}


def load_script(name):
    """(actions int8 [T][n], OracleVec / MgxEngine config keywords, agent seed) of one action script."""
    z = np.load(os.path.join(TC.GOLDEN, "actions", name + ".npz"))
    m = int(z["mission"])
    cfg = dict(problem=str(z["problem"]), mission=None if m < 0 else m, size=int(z["size"]),
               num_objects=int(z["num_objects"]), seed=int(z["seed"]))
    return z["actions"], cfg, int(z["agent_seed"])


@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_script_shape(name):
    """n = eight blocks and eight envs (three and eight for `full`), T a multiple of 32 above 2 * size^2 (above
    size^2 at S = 16); only actions 0..6, and the wanderers (env % 5 == 3) never play `done`."""
    acts, cfg, _ = load_script(name)
    T, n = acts.shape
    S = cfg["size"]
    assert (n, T) == SCRIPTS[name] and acts.dtype == np.int8
    assert T % 32 == 0 and T > (1 if S == 16 else 2) * S * S and n % 64 == 8
    assert acts.min() >= 0 and acts.max() == 6
    assert (acts[:, 3::5] != 6).all()


@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_agent_over_oracle_reproduces_script(name):
    import oracle as O
    acts, cfg, agent_seed = load_script(name)
    n = acts.shape[1]
    ov = O.OracleVec(cfg["problem"], cfg["mission"], cfg["size"], cfg["num_objects"], n, cfg["seed"])
    ov.reset()
    got = SA.run(ov, SA.ScriptedAgent(n, agent_seed), 64)
    assert np.array_equal(got, acts[:64]), np.argwhere(got != acts[:64])[:4]


@pytest.mark.parametrize("name", ["deep_multi_all_s8", "deep_multi_tgl_s16"])
def test_agent_over_oracle_reproduces_reference_run(name):
    d = dict(np.load(os.path.join(TC.GOLDEN, "traj", name + ".npz")))
    cfg, T = TC.fixture_cfg(d)
    src = TC.OracleSource(cfg)
    src.reset()
    got = SA.run(src, SA.ScriptedAgent(cfg["n_envs"], int(d["agent_seed"])), 128)
    assert np.array_equal(got, d["actions"][:128]), np.argwhere(got != d["actions"][:128])[:4]


def test_modes_and_noise():
    """Mode = env index % 5; the same (seed, index) gives the same stream, another index another one."""
    assert [SA.AgentCtx(1, i).mode for i in range(6)] == ["solver", "solver", "keyer", "wanderer", "laststep", "solver"]
    a, b, c = SA.AgentCtx(7, 3), SA.AgentCtx(7, 3), SA.AgentCtx(7, 4)
    x = [a.rng.random() for _ in range(4)]
    assert x == [b.rng.random() for _ in range(4)] and x != [c.rng.random() for _ in range(4)]


def _view(rows, agent, carry=(0, 0, 0, 0), target=(255, 255, 255), mission_done=0, step_count=5):
    """A View of a small walled room drawn as text: '#' wall, '.' empty, 'G' goal, 'L' locked red door,
    'k' red key, 'D' closed blue door; rows[y][x]."""
    cell = {"#": [2, 5, 0, 0], ".": [1, 0, 0, 0], "G": [8, 1, 0, 0], "L": [4, 0, 2, 0], "k": [5, 0, 0, 0],
            "D": [4, 2, 1, 0]}
    S = len(rows)
    grid = [[cell[rows[y][x]] for y in range(S)] for x in range(S)]
    return SA.View(S, grid, list(agent), list(carry), list(target), mission_done, step_count)


class _NoNoise:
    """A Generator stand-in that never triggers the random action (random() = 0.5) and always draws 0."""

    def random(self):
        return 0.5

    def integers(self, lo, hi):
        return lo


def _ctx(mode):
    c = SA.AgentCtx(0, SA.MODES.index(mode))
    c.rng = _NoNoise()
    return c


ROOM = ["#######",
        "#..#..#",
        "#..L.G#",
        "#.k#..#",
        "#..#..#",
        "#..D..#",
        "#######"]


def test_solver_routes_through_the_closed_door_and_toggles_it():
    """`go to goal` behind a wall: the locked door is no way through without its key, the closed door is."""
    goal = (5, 2, 255)
    assert SA.act(_view(ROOM, (2, 5, 1), target=goal), _ctx("solver")) == SA.LEFT          # turn to face +x
    assert SA.act(_view(ROOM, (2, 5, 0), target=goal), _ctx("solver")) == SA.TOGGLE        # the closed door
    assert SA.act(_view(ROOM, (2, 2, 0), carry=(5, 0, 0, 0), target=goal), _ctx("solver")) == SA.TOGGLE   # unlocks


def test_keyer_fetches_the_key_then_the_door():
    goal = (5, 2, 255)
    assert SA.act(_view(ROOM, (1, 3, 0), target=goal), _ctx("keyer")) == SA.PICKUP          # facing the red key
    assert SA.act(_view(ROOM, (2, 2, 1), carry=(5, 0, 0, 0), target=goal), _ctx("keyer")) == SA.LEFT
    assert SA.act(_view(ROOM, (2, 2, 0), carry=(6, 3, 0, 0), target=goal), _ctx("keyer")) in (SA.LEFT, SA.RIGHT)
    assert SA.act(_view(ROOM, (1, 1, 0), carry=(6, 3, 0, 0), target=goal), _ctx("keyer")) == SA.DROP


def test_last_step_mode_holds_until_the_final_step():
    S2 = 49
    done_kw = dict(target=(2, 3, 3), mission_done=1)
    assert SA.act(_view(ROOM, (1, 3, 0), step_count=10, **done_kw), _ctx("laststep")) != SA.DONE
    assert SA.act(_view(ROOM, (1, 3, 0), step_count=S2 - 1, **done_kw), _ctx("laststep")) == SA.DONE
    assert SA.act(_view(ROOM, (1, 3, 0), step_count=10, **done_kw), _ctx("solver")) == SA.DONE   # (waits 0 steps)
    goal = (5, 2, 255)
    assert SA.act(_view(ROOM, (4, 2, 0), target=goal, step_count=10), _ctx("laststep")) == SA.RIGHT   # look away
    assert SA.act(_view(ROOM, (4, 2, 1), target=goal, step_count=10), _ctx("laststep")) == SA.DROP    # wait
    assert SA.act(_view(ROOM, (4, 2, 1), target=goal, step_count=S2 - 2), _ctx("laststep")) == SA.LEFT
    assert SA.act(_view(ROOM, (4, 2, 0), target=goal, step_count=S2 - 1), _ctx("laststep")) == SA.FORWARD


def test_wanderer_never_plays_done():
    c = SA.AgentCtx(3, 3)
    v = _view(ROOM, (4, 2, 0), target=(5, 2, 255), mission_done=1)
    acts = {SA.act(v, c) for _ in range(400)}
    assert SA.DONE not in acts and acts >= {SA.LEFT, SA.RIGHT, SA.PICKUP, SA.DROP, SA.TOGGLE}
