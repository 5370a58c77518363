"""The C oracle (oracle/mgx_oracle.c) against the golden fixtures produced by
executing the reference's own custom_env.py / environment.py
(tests/golden/make_golden.py).  Bit-exact: obs, rewards (fp64), flags, full
grid + agent state after every step, RNG stream positions after every reset,
live-lock retry counts."""
import numpy as np
import pytest

import trajcheck as TC

FIXTURES = TC.fixtures()


def test_fixtures_present():
    assert len(FIXTURES) == 69                    # 53 random-action runs + 16 scripted-agent (deep_*) runs


def test_fixtures_pin_every_size():
    """Every size mgx_create accepts has a reference fixture; multi (one kernel instantiation per
    occupancy-mask width) has one at every size it accepts."""
    sizes, multi = set(), set()
    for p in FIXTURES:
        d = np.load(p)
        sizes.add(int(d["meta"][0]))
        if str(d["problem"]) == "multi":
            multi.add(int(d["meta"][0]))
    assert sizes == set(range(5, 17)) and multi == set(range(6, 17)), (sizes, multi)


def test_manual_fixtures_hold_premature_dones():
    """The manual=True fixtures (PlaygroundEnv(manual=True), custom_env.py:319-328) contain 'done'
    actions that end nothing (mission not complete) and 'done' actions that end a completed
    mission with its stored reward."""
    for name in ("manual_multi_all_s8", "manual_multi_pkp_s11"):
        d = dict(np.load(TC.GOLDEN + "/traj/%s.npz" % name))
        a, term = d["actions"], d["terminated"]
        assert ((a == 6) & (term == 0)).sum() > 100, name
        assert ((a == 6) & (term == 1) & (d["reward"] > 0)).sum() > 0, name


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: p.split("/")[-1][:-4])
def test_oracle_matches_reference_fixture(path):
    d = dict(np.load(path))
    cfg, T = TC.fixture_cfg(d)
    msg = TC.compare(TC.OracleSource(cfg), d)
    assert msg is None, msg


def test_fixture_covers_quirks():
    """The fixtures exercise the paths that matter.  Over the whole set: live-locks (S=8; multi_all_s6 and
    multi_all_s7 each hold abandoned attempts of their own, the common case on small grids), truncation,
    mission completion with stored reward, goal termination.  Per scripted-agent fixture (deep_*,
    tests/golden/scripted_agent.py) floors on the deep-episode events of TC.events -- conditions on the
    inputs, not measurements of the code under test: the time limit reached at every size, locked doors
    opened with the carried key, carried objects consumed by a same-colour door (Q4), paid rewards,
    truncations with a completed mission still stored (Q2), steps that terminate and truncate at once,
    a locked door toggled with the wrong key."""
    tot_ll = tot_trunc = tot_goal = tot_stored = 0
    trunc_md = trunc_md_s16 = wrong_key = n_deep = 0
    for p in FIXTURES:
        d = dict(np.load(p))
        name = p.split("/")[-1][:-4]
        tot_ll += int(d["livelock"].sum() + d["reset0_livelock"].sum())
        tot_trunc += int(d["truncated"].sum())
        tot_goal += int(((d["reward"] > 0) & (d["terminated"] == 1)).sum())
        tot_stored += int(np.isfinite(d["stored_reward"]).sum())
        if name in ("multi_all_s6", "multi_all_s7"):
            assert int(d["livelock"].sum() + d["reset0_livelock"].sum()) > 0, name
        if not name.startswith("deep_"):
            continue
        n_deep += 1
        assert str(d["agent_name"]) == "scripted" and int(d["meta"][2]) % 16 == 0, name
        e = TC.events(d)
        S = e["size"]
        multi, ado = "multi" in name, "ado_" in name
        assert e["max_step_count"] == S * S and e["truncations"] >= 10, (name, e)
        if multi and not ado:
            assert e["unlocks"] >= 20 and e["q4"] >= 20, (name, e)
        if "_mov_" not in name:
            assert e["paid"] >= 90, (name, e)
        if "_gtg_" not in name:                      # (every other mission pays on its `done`)
            assert e["done_paid"] >= 30, (name, e)
        assert e["term_and_trunc"] >= (3 if S == 8 else 1), (name, e)
        trunc_md += e["trunc_mission_done"]
        trunc_md_s16 += e["trunc_mission_done"] if S == 16 else 0
        wrong_key += e["wrong_key"]
    assert tot_ll > 0 and tot_goal > 0 and tot_stored > 0 and tot_trunc > 0
    assert n_deep == 16
    assert trunc_md >= 50 and trunc_md_s16 >= 1, (trunc_md, trunc_md_s16)
    assert wrong_key >= 1
