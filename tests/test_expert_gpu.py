"""mgx_expert_act on the GPU against its definition, mgx.expert.expert_reference on engine.dump_state(): actions and
costs of every env, in integers.

Shapes: 200 envs (three full waves and an 8-lane tail); sizes 5, 8, 11 and 16 (at 16 all 16 bits of a row and all 8
words of a board are live; 5 and 11 leave rows and bits unused; GS / 16 is 2, 4, 8, 16 -- the LDS grid stride is
made odd from each); multi with every mission and locked doors (the key routine, the held-back door layer, carried
keys), obstacles (lava), the single-room problems, `full` (target-less 'drop' and 'move' missions); int32 and int64
action outputs, with and without cost_dev, in every case; ring and inline reset modes.  Each env plays the expert's
action with probability 0.7 and else a uniform one, drawn on the host from a fixed seed: that reaches carried
objects, opened doors and dropped keys, which expert play alone never produces."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

N_ENVS, STEPS = 200, 40
MULTI = dict(problem="multi", mission=None, num_objects=4)
CASES = {
    "gtg5": (dict(problem="gtg", mission=5, size=5, num_objects=1), {}),
    "gto8": (dict(problem="gto", mission=0, size=8, num_objects=4), {}),
    "pkp11": (dict(problem="pkp", mission=2, size=11, num_objects=4), {}),
    "opn16": (dict(problem="opn", mission=1, size=16, num_objects=4), {}),
    "multi8": (dict(size=8, **MULTI), {}),
    "multi11": (dict(size=11, **MULTI), {}),
    "multi16": (dict(size=16, **MULTI), {}),
    "multi8-inline": (dict(size=8, **MULTI), dict(ring_depth=-1)),
    "multi16-inline": (dict(size=16, **MULTI), dict(ring_depth=-1)),
    "lava8": (dict(problem="multi", mission=5, size=8, num_objects=4, obstacles=True, percent_obstacles=0.1), {}),
    "full8": (dict(problem="full", mission=None, size=8, num_objects=4), {}),
}
STATE_KEYS = ("grid", "agent", "carrying", "step_count", "mission_done", "target", "mission_id", "pcg", "mtwords")


def _engine(cfg, extra, n=N_ENVS, **kw):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgx import MgxEngine
    return MgxEngine(n_envs=n, terminal_mode="truncated", mission_dtype=torch.uint8, reward64=True, **cfg, **extra,
                     **kw)


def _same_state(a, b):
    for k in STATE_KEYS:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("case", sorted(CASES))
def test_kernel_equals_reference(case):
    """At reset and after every one of 40 steps: the kernel's actions (int64 with costs, int32 without) and costs
    equal expert_reference's for every env; the call leaves the engine's state as it was."""
    from mgx import ExpertActor, expert_reference
    from mgx.compact import CompactBuffer
    cfg, extra = CASES[case]
    eng = _engine(cfg, extra)
    inline = extra.get("ring_depth") == -1
    eng.reset()
    buf = None
    if not inline:
        buf = CompactBuffer(eng, STEPS)
        buf.observe(0)
    expert = ExpertActor(eng)
    rng = np.random.default_rng(20251021)
    a32 = torch.zeros(N_ENVS, dtype=torch.int32, device=eng.device)
    seen, carried, bad = set(), 0, []
    for t in range(STEPS + 1):
        st = eng.dump_state()
        ra, rc = expert_reference(st)
        a64 = expert.expert_act()
        cost = expert.last_cost.clone()
        expert.last_cost.fill_(12345)
        a32.fill_(-7)
        expert.expert_act(out=a32, cost=False)
        assert int((expert.last_cost != 12345).sum()) == 0            # no cost_dev: nothing written
        ga, gc, g32 = a64.cpu().numpy(), cost.cpu().numpy(), a32.cpu().numpy()
        if t in (0, STEPS // 2):
            _same_state(st, eng.dump_state())
        miss = np.nonzero((ga != ra) | (gc != rc) | (g32 != ra))[0]
        for i in miss[:3]:
            bad.append((t, int(i), (int(ga[i]), int(gc[i]), int(g32[i])), (int(ra[i]), int(rc[i])),
                        st["agent"][i].tolist(), st["target"][i].tolist(), st["carrying"][i].tolist()))
        seen |= set(np.minimum(rc, 1).tolist())
        carried += int((st["carrying"][:, 0] != 0).sum())
        if t == STEPS:
            break
        play = np.where(rng.random(N_ENVS) < 0.7, ra, rng.integers(0, 7, N_ENVS)).astype(np.int64)
        act = torch.as_tensor(play, device=eng.device)
        if inline:
            eng.step(act)
        else:
            buf.step(t, act)
    eng.poll_error()
    print("%s: cost classes seen %s, carried-object states %d" % (case, sorted(seen), carried))
    assert not bad, bad[:6]
    assert 1 in seen                                                  # routed states
    if case.startswith("multi"):
        assert {-2, -3, 0} <= seen and carried > 0                    # the drop and key routines, completed missions
    if case == "full8":
        assert -1 in seen                                             # 'move': unsupported


@pytest.mark.parametrize("size", [8, 16])
def test_closed_loop_parity(size):
    """Engine + kernel against OracleVec + expert_reference at the same seed for 3 S^2 steps: rewards, dones and
    episode lengths step for step, and the same final state."""
    import oracle as O
    from mgx import ExpertActor, expert_reference
    from mgx.compact import CompactBuffer
    T = 3 * size * size
    eng = _engine(dict(size=size, **MULTI), {})
    ov = O.OracleVec("multi", None, size, 4, N_ENVS, 42)
    ov.reset()
    eng.reset()
    buf = CompactBuffer(eng, 16, ring=True)
    buf.observe(0)
    expert = ExpertActor(eng)
    bt = 0
    rew, done, lens, acts = [], [], [], []
    for t in range(T):
        a = expert.act(buf, bt)[0]
        buf.step(bt, a)
        acts.append(a.clone())
        rew.append(eng.reward64.clone())
        done.append(buf.dones[bt].clone())
        lens.append(eng.ep_len.clone())
        bt += 1
        if bt == buf.T:
            buf.carry_over()
            bt = 0
    eng.poll_error()
    rew, done, lens, acts = (torch.stack(x).cpu().numpy() for x in (rew, done, lens, acts))
    count = np.zeros(N_ENVS, np.int64)
    episodes = 0
    for t in range(T):
        st = ov.dump()
        ra, _ = expert_reference(st)
        assert np.array_equal(acts[t], ra), "actions differ at step %d" % t
        o = ov.step(ra)
        d = (o["terminated"] | o["truncated"]).astype(bool)
        count += 1
        assert np.array_equal(done[t].astype(bool), d), "dones differ at step %d" % t
        assert np.array_equal(rew[t], o["reward"]), "rewards differ at step %d" % t
        assert np.array_equal(lens[t][d], count[d]), "episode lengths differ at step %d" % t
        count[d] = 0
        episodes += int(d.sum())
    assert episodes > N_ENVS
    a, b = eng.dump_state(), ov.dump()
    for k in ("grid", "agent", "carrying", "step_count", "mission_done", "target", "pcg", "mtwords"):
        assert np.array_equal(a[k], b[k]), k


def test_evaluation_paths_agree():
    """evaluate_policy(expert, engine, 64, fused=expert) and GraphEvaluator(expert).evaluate(64) over two engines of
    equal seed return the same episode lists, and the expert solves what it should: every reward positive but for
    the few episodes the rules give up on."""
    from mgx import ExpertActor, GraphEvaluator, evaluate_policy
    cfg = dict(size=8, **MULTI)
    e1, e2 = _engine(cfg, {}, n=32, refill_every=16), _engine(cfg, {}, n=32, refill_every=16)
    x1, x2 = ExpertActor(e1), ExpertActor(e2)
    r1, l1 = evaluate_policy(x1, e1, 64, return_episode_rewards=True, fused=x1)
    ev = GraphEvaluator(x2)
    r2, l2 = ev.evaluate(64, return_episode_rewards=True)
    e1.poll_error()
    e2.poll_error()
    assert len(r1) == 64 and r1 == r2 and l1 == l2
    assert sum(r > 0 for r in r1) >= 48          # the CPU test holds the share to 0.95; 64 episodes are a small sample
    r3, l3 = ev.evaluate(64, return_episode_rewards=True)             # the captured graphs, replayed
    assert len(r3) == 64


def test_actor_preconditions():
    from mgx import ExpertActor
    from mgx.compact import CompactBuffer
    cfg = dict(problem="gtg", mission=5, size=8, num_objects=4)
    eng, other = _engine(cfg, {}, n=8), _engine(cfg, {}, n=8)
    eng.reset()
    other.reset()
    buf, obuf = CompactBuffer(eng, 4), CompactBuffer(other, 4)
    buf.observe(0)
    obuf.observe(0)
    x = ExpertActor(eng)
    assert x.policy is x and x.sync() is None
    with pytest.raises(TypeError, match="engine's state"):
        x.predict({})
    with pytest.raises(ValueError, match="another engine"):
        x.act(obuf, 0)
    a = x.act(buf, 0)
    assert a[1] is None and a[2] is None and a[0].dtype == torch.int64
    with pytest.raises(ValueError, match="current state"):
        x.act(buf, 1)                                                 # not stepped yet: row 1 is not the newest
    buf.step(0, a[0])
    with pytest.raises(ValueError, match="current state"):
        x.act(buf, 0)                                                 # stepped: row 0 is stale
    x.act(buf, 1)
    with pytest.raises(ValueError, match="int32/int64"):
        x.expert_act(out=torch.zeros(8, dtype=torch.float32, device=eng.device))
    L = eng.L
    assert L.mgx_expert_act(eng.h, None, 8, None, None) == 1 and b"mgx_expert_act" in L.mgx_last_error()
    assert L.mgx_expert_act(None, a[0].data_ptr(), 8, None, None) == 1
    assert L.mgx_expert_act(eng.h, a[0].data_ptr(), 2, None, None) == 1
    eng.poll_error()
