"""Graph-captured policy evaluation on the GPU: mgx_eval_record against its numpy restatement
(mgx.evaluation.eval_record_reference, itself pinned to evaluate_policy's loop body in tests/test_graph_eval_cpu.py),
GraphEvaluator against the eager evaluate_policy(..., fused=actor) loop, its reuse, and EvalCallback / learn() under
graph_collect.  Every comparison is exact: integers, or floats written by the same launches."""
import ctypes
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mgx.policy import ActorCriticPolicy  # noqa: E402

pytestmark = pytest.mark.gpu


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---------------------------------------------------------------- 1. the kernel alone
STEPS = 48
R_SENT, L_SENT, W_SENT, M_SENT = -7.25, -77, -5, 0xA5


def _n_evals(n):
    return sorted({0, 1, max(n - 1, 0), n, n + 1, 3 * n + 2})


@pytest.mark.parametrize("reward64", [True, False])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_eval_record_equals_reference(n, reward64):
    """48 steps per (n_envs, n_eval): done with probability 0.35, f64 rewards with exact zeros (or the f32 ep_return
    when the engine has no reward64), random lengths and mission ids over all of 0..255; the tables start as
    sentinels.  After EVERY step counts, the four tables -- sentinels included -- and remaining equal the
    reference.  base_dev differs from case to case and `when` carries it; steps 24.. use step_offset against an
    advanced base, as the second block of a captured evaluation does."""
    _gpu()
    from mgx.evaluation import EvalRecords, eval_record_reference
    dev = torch.device("cuda", torch.cuda.current_device())
    for n_eval in _n_evals(n):
        g = np.random.default_rng(1000 * n + n_eval)
        cap = max(1, -(-n_eval // n))
        base = int(g.integers(0, 2 ** 40)) if n_eval % 2 else 0
        rec = EvalRecords(n, cap, dev)
        rec.begin(n_eval, base=base)
        rec.rewards.fill_(R_SENT)
        rec.lengths.fill_(L_SENT)
        rec.when.fill_(W_SENT)
        rec.missions.fill_(M_SENT)
        ref = dict(counts=np.zeros(n, np.int32), rewards=np.full((n, cap), R_SENT), remaining=n_eval,
                   lengths=np.full((n, cap), L_SENT, np.int32), when=np.full((n, cap), W_SENT, np.int64),
                   missions=np.full((n, cap), M_SENT, np.uint8))
        for t in range(STEPS):
            done = (g.random(n) < 0.35).astype(np.uint8)
            r64 = np.where(g.random(n) < 0.4, 0.0, g.random(n))
            r32 = r64.astype(np.float32)
            ep_len = g.integers(1, 300, n).astype(np.int32)
            mids = g.integers(0, 256, n).astype(np.uint8)
            if t == 0:
                mids[0] = 200                                   # an id >= 128 in every case
            if t == STEPS // 2:
                rec.base.add_(STEPS // 2)                       # the block advance
            off = t % (STEPS // 2)
            rec.record(torch.as_tensor(done, device=dev), torch.as_tensor(r64, device=dev) if reward64 else None,
                       torch.as_tensor(r32, device=dev), torch.as_tensor(ep_len, device=dev),
                       torch.as_tensor(mids, device=dev), n_eval, step_offset=off)
            eval_record_reference(ref, done, r64 if reward64 else r32.astype(np.float64), ep_len, mids, n_eval,
                                  base + t)
            tag = (n, n_eval, t)
            assert np.array_equal(rec.counts.cpu().numpy(), ref["counts"]), tag
            assert np.array_equal(rec.rewards.cpu().numpy(), ref["rewards"]), tag
            assert np.array_equal(rec.lengths.cpu().numpy(), ref["lengths"]), tag
            assert np.array_equal(rec.when.cpu().numpy(), ref["when"]), tag
            assert np.array_equal(rec.missions.cpu().numpy(), ref["missions"]), tag
            assert int(rec.remaining) == ref["remaining"], tag
        assert int(rec.base) == base + STEPS // 2               # read, never written, by the launches
        if n_eval:
            assert ref["remaining"] < n_eval, "nothing was recorded"


def test_eval_record_invalid_arguments():
    """MGX_ERR_INVALID on live device pointers, nothing launched: the tables keep their sentinels."""
    _gpu()
    from mgx import _lib
    from mgx.evaluation import EvalRecords
    dev = torch.device("cuda", torch.cuda.current_device())
    n = 70
    rec = EvalRecords(n, 2, dev)
    rec.begin(2 * n)
    rec.when.fill_(W_SENT)
    done = torch.ones(n, dtype=torch.uint8, device=dev)
    r = torch.ones(n, dtype=torch.float64, device=dev)
    ln = torch.ones(n, dtype=torch.int32, device=dev)
    rec.record(done * 0, r, None, ln, done, 2 * n)                # fills the argument struct; records nothing
    L, a = _lib.load(), rec._args

    def call(n_envs=n, n_eval=2 * n, cap=2, **kw):
        b = _lib.MgxEvalRecordArgs.from_buffer_copy(a)
        for k, v in kw.items():
            setattr(b, k, v)
        return L.mgx_eval_record(n_envs, n_eval, cap, 0, ctypes.byref(b), None)

    for kw in (dict(n_envs=0), dict(n_envs=-1), dict(cap=0), dict(n_eval=-1), dict(n_eval=2 * n + 1),
               dict(done_dev=None), dict(reward64_dev=None), dict(ep_len_dev=None), dict(mission_id_dev=None),
               dict(base_dev=None), dict(counts_dev=None), dict(rewards_dev=None), dict(lengths_dev=None),
               dict(when_dev=None), dict(missions_dev=None), dict(remaining_dev=None)):
        st = call(**kw)
        assert st == 1 and b"mgx_eval_record" in L.mgx_last_error(), kw
    with pytest.raises(_lib.MgxError):
        _lib.check(call(cap=0), "mgx_eval_record")
    with pytest.raises(ValueError):                               # the wrapper's own tensor checks
        rec.record(done.bool(), r, None, ln, done, 2 * n)
    torch.cuda.synchronize()
    assert int(rec.counts.sum()) == 0 and int(rec.remaining) == 2 * n and bool((rec.when == W_SENT).all())


# ---------------------------------------------------------------- 2. graph against eager
def _engine(env, n_envs, k, refill_every, seed=42):
    from mgx import MgxEngine
    return MgxEngine(n_envs=n_envs, n_stack=k, seed=seed, terminal_mode="truncated", mission_dtype=torch.uint8,
                     refill_every=refill_every, reward64=True, **env)


def _policy(k, seed=0):
    """A randomly initialised policy under a fixed seed, every blob parameter redrawn as
    tests/test_graph_collect_gpu.py does (weights N(0, 1) / sqrt(fan-in), biases N(0, 0.5^2)): the greedy action
    varies with the observation, so episodes end at different steps."""
    from mgx.fused_policy import _params
    torch.manual_seed(seed)
    pol = ActorCriticPolicy(n_stack=k)
    g = torch.Generator().manual_seed(300 + seed)
    with torch.no_grad():
        for t in _params(pol)[1]:
            if t.dim() > 1:
                t.copy_(torch.randn(t.shape, generator=g) / math.sqrt(t[0].numel()))
            else:
                t.copy_(0.5 * torch.randn(t.shape, generator=g))
    return pol.cuda()


def _eager_with_missions(pol, eng, actor, n_eval, deterministic):
    """The loop of evaluate_policy(pol, eng, n_eval, fused=actor) on the host, one read per step: (rewards, lengths,
    mission ids, steps) with the mission of each recorded episode taken from buf.mids at the done step -- the
    observation the action was taken on."""
    from mgx.compact import CompactBuffer
    n = eng.n
    targets = [(n_eval + i) // n for i in range(n)]
    counts = [0] * n
    eng.reset()
    buf, bt = CompactBuffer(eng, max(2, eng.n_stack), ring=True), 0
    buf.observe(0)
    rewards, lengths, missions, t = [], [], [], 0
    while any(c < g for c, g in zip(counts, targets)):
        actions = actor.act(buf, bt, deterministic=deterministic)[0]
        mids = buf.mids[buf.row(bt)].cpu().tolist()
        buf.step(bt, actions)
        done = buf.dones[bt].cpu().tolist()
        r, ln = eng.reward64.cpu().tolist(), eng.ep_len.cpu().tolist()
        for i in range(n):
            if done[i] and counts[i] < targets[i]:
                rewards.append(round(r[i], 6))
                lengths.append(ln[i])
                missions.append(mids[i])
                counts[i] += 1
        bt += 1
        if bt == buf.T:
            buf.carry_over()
            bt = 0
        t += 1
    return rewards, lengths, missions, t


CONFIGS = [
    ("multi-any", dict(problem="multi", mission=None, size=8, num_objects=4), 16, 37, 4),
    ("pkp", dict(problem="pkp", mission=None, size=8, num_objects=4), 5, 12, 4),
    ("multi-toggle-11", dict(problem="multi", mission=1, size=11, num_objects=4), 16, 16, 4),
    ("multi-pickup-stack1", dict(problem="multi", mission=2, size=8, num_objects=4), 9, 20, 1),
]


@pytest.mark.parametrize("deterministic", [True, False])
@pytest.mark.parametrize("refill_every", [4, 16])
@pytest.mark.parametrize("name,env,n_envs,n_eval,k", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_graph_evaluation_equals_eager(name, env, n_envs, n_eval, k, refill_every, deterministic):
    """Fresh engines of equal seed, one randomly initialised policy, two FusedActors of equal sampling seed: the
    graph evaluator's episode lists equal evaluate_policy(..., fused=actor)'s element for element, mean and std
    are equal, steps_needed is the eager loop's step count, steps the next multiple of K, and the mission ids are
    those a host loop reads from buf.mids at the done steps."""
    _gpu()
    from mgx import GraphEvaluator, evaluate_policy
    from mgx.fused_policy import FusedActor
    pol = _policy(k)
    engs = [_engine(env, n_envs, k, refill_every) for _ in range(4)]
    actors = [FusedActor(pol, e, seed=9) for e in engs]
    want_r, want_l = evaluate_policy(pol, engs[0], n_eval, deterministic, return_episode_rewards=True,
                                     fused=actors[0])
    host_r, host_l, host_m, steps = _eager_with_missions(pol, engs[1], actors[1], n_eval, deterministic)
    assert (host_r, host_l) == (want_r, want_l) and len(want_r) == n_eval
    ev = GraphEvaluator(actors[2])
    assert ev.K == refill_every and ev.buf.T == refill_every
    got_r, got_l = evaluate_policy(pol, engs[2], n_eval, deterministic, return_episode_rewards=True,
                                   fused=actors[2], graph=ev)
    assert got_r == want_r and got_l == want_l
    last = ev.last
    assert last["steps_needed"] == steps
    assert last["steps"] == math.ceil(steps / ev.K) * ev.K == last["replays"] * ev.K
    assert last["mission_ids"] == host_m
    assert engs[2].calls == last["steps"]
    mean, std = evaluate_policy(pol, engs[3], n_eval, deterministic, fused=actors[3], graph=True)
    assert mean == float(np.mean(want_r)) and std == float(np.std(want_r))
    for e in engs:
        e.poll_error()


def test_graph_evaluation_block_of_two_epochs_and_errors():
    """block_steps = 2 refill epochs; a block that is no multiple of the epoch, an evaluator of another actor and a
    policy of another actor raise ValueError; n_eval = 0 replays nothing and returns NaNs as the eager loop does."""
    _gpu()
    from mgx import GraphEvaluator, evaluate_policy
    from mgx.fused_policy import FusedActor
    env = CONFIGS[0][1]
    pol = _policy(4)
    e1, e2 = _engine(env, 16, 4, 4), _engine(env, 16, 4, 4)
    a1, a2 = FusedActor(pol, e1, seed=9), FusedActor(pol, e2, seed=9)
    want = evaluate_policy(pol, e1, 20, return_episode_rewards=True, fused=a1)
    ev = GraphEvaluator(a2, block_steps=8)
    assert ev.evaluate(20, return_episode_rewards=True) == want
    assert ev.last["steps"] % 8 == 0 and ev.last["steps"] - ev.last["steps_needed"] < 8
    with pytest.raises(ValueError):
        GraphEvaluator(a2, block_steps=6)
    with pytest.raises(ValueError):
        evaluate_policy(pol, e1, 5, fused=a1, graph=ev)
    with pytest.raises(ValueError):
        evaluate_policy(_policy(4, seed=1), e2, 5, fused=a2, graph=ev)
    n_graphs = len(ev.graphs)
    mean, std = ev.evaluate(0)
    assert math.isnan(mean) and math.isnan(std) and len(ev.graphs) == n_graphs
    assert ev.last == dict(steps=0, steps_needed=0, replays=0, mission_ids=[])
    e2.poll_error()


# ---------------------------------------------------------------- 3. reuse
def _perturb(pol, i):
    g = torch.Generator().manual_seed(1000 + i)
    with torch.no_grad():
        for p in pol.parameters():
            p.add_((0.05 * torch.randn(p.shape, generator=g)).to(p.device))


@pytest.mark.parametrize("deterministic", [True, False])
def test_one_evaluator_evaluates_twice(deterministic):
    """The second evaluate() captures nothing, reads the changed weights (it syncs the actor itself) and, after
    engine.set_seed(seed) made its reset a seeded one, equals the eager fused loop on the new weights.

    The eager loop runs on a second engine taken through the same first graph evaluation and the same set_seed, not
    on a fresh one: a seeded reset after the first reseeds each env's PCG64 only -- the MT19937 cursor goes on and
    mission_done / the stored reward persist, as in the reference (mgx_reset, reset_mode 1) -- so no later
    evaluation on any engine equals one on a fresh engine.  That the two engines are in one state after equal
    graph evaluations is the determinism of the over-run continuation, checked at the end without any rewind: two
    evaluators on two fresh engines agree over both of their evaluations."""
    _gpu()
    from mgx import GraphEvaluator, evaluate_policy
    from mgx.fused_policy import FusedActor, pack_blob
    name, env, n_envs, n_eval, k = CONFIGS[0]
    pol = _policy(k)
    eng, twin = _engine(env, n_envs, k, 16), _engine(env, n_envs, k, 16)
    actor, twin_actor = FusedActor(pol, eng, seed=9), FusedActor(pol, twin, seed=9)
    ev = GraphEvaluator(actor)
    first = ev.evaluate(n_eval, deterministic, return_episode_rewards=True)
    first_last = dict(ev.last)
    assert GraphEvaluator(twin_actor).evaluate(n_eval, deterministic, return_episode_rewards=True) == first
    graphs = dict(ev.graphs)
    assert graphs
    if not deterministic:                                         # one draw per step, the over-run's included
        assert int(actor.counter[0]) == first_last["steps"] == int(twin_actor.counter[0])
    _perturb(pol, 1)
    assert not torch.equal(actor.blob, pack_blob(pol))
    eng.set_seed(42)
    twin.set_seed(42)
    second = ev.evaluate(n_eval, deterministic, return_episode_rewards=True)
    assert ev.graphs == graphs                                    # nothing captured anew
    assert torch.equal(actor.blob, pack_blob(pol))                # the evaluator synced the actor
    twin_actor.sync()
    want = evaluate_policy(pol, twin, n_eval, deterministic, return_episode_rewards=True, fused=twin_actor)
    assert second == want and len(second[0]) == n_eval
    assert twin.calls == ev.last["steps_needed"]                  # the eager loop's step count
    # two evaluators, two evaluations each, no rewind
    out = []
    for p in (_policy(k), _policy(k)):
        e = _engine(env, n_envs, k, 16)
        v = GraphEvaluator(FusedActor(p, e, seed=9))
        a = v.evaluate(n_eval, deterministic, return_episode_rewards=True)
        _perturb(p, 2)
        b = v.evaluate(n_eval, deterministic, return_episode_rewards=True)
        out.append((a, b, dict(v.last)))
        e.poll_error()
    assert out[0] == out[1]
    assert out[0][0] == first
    eng.poll_error()
    twin.poll_error()


# ---------------------------------------------------------------- 4. EvalCallback under graph_collect, learn()
ENV = dict(problem="multi", mission=2, size=8, num_objects=4)


def _cfg(**kw):
    """8 envs x 16 steps with fused_act -- and the fused update in minibatches of one 64-sample tile, the only
    update that is reproducible to the bit from run to run (tests/test_graph_collect_gpu.py), which comparing two
    learn() runs needs."""
    from mgx.ppo import PPOConfig
    return PPOConfig(n_envs=8, horizon=16, batch_size=64, n_epochs=2, fused_act=True, fused_train=True,
                     fused_mission=True, fused_update=True, n_eval_episodes=12, env=ENV, **kw)


def _callback(**kw):
    from mgx import EvalCallback
    ev = _engine(ENV, 6, 4, 16, seed=43)
    return EvalCallback(ev, fused=True, graph=True, eval_freq=24, n_eval_episodes=10, **kw)


def _same_history(ha, hb):
    assert len(ha) == len(hb)
    for a, b in zip(ha, hb):
        assert a.keys() == b.keys()
        for key in a:
            assert a[key] == b[key] or (math.isnan(a[key]) and math.isnan(b[key])), (key, a[key], b[key])


def test_learn_with_deferred_eval_callback_equals_per_step_callback():
    """3 rollouts of 8 envs x 16 steps, eval_freq 24: evaluations fall on step 8 of the second rollout and step 16
    of the third.  With graph_collect the callback runs after each replay; history and callback.evaluations equal
    those of the run that calls it inside the loop."""
    _gpu()
    from mgx.ppo import learn
    cb_e, cb_g = _callback(), _callback()
    pol_e, hist_e, eng_e = learn(_cfg(), 3 * 8 * 16, callback=cb_e)
    pol_g, hist_g, eng_g = learn(_cfg(graph_collect=True), 3 * 8 * 16, callback=cb_g)
    assert len(hist_g) == 3
    _same_history(hist_e, hist_g)
    assert [x[0] for x in cb_g.evaluations] == [24 * 8, 48 * 8]
    assert cb_e.evaluations == cb_g.evaluations
    assert cb_e.n_calls == cb_g.n_calls == 48
    assert cb_g.evaluator is not None and cb_g.evaluator.graphs
    for (name, a), (_, b) in zip(pol_e.named_parameters(), pol_g.named_parameters()):
        assert torch.equal(a.detach(), b.detach()), name
    eng_g.poll_error()
    cb_g.eval_engine.poll_error()


def test_learn_stops_at_the_same_evaluation():
    """StopTrainingOnRewardThreshold(-1.0) stops at the first evaluation (step 8 of the second rollout) either way:
    one history entry, the evaluation's num_timesteps equal."""
    _gpu()
    from mgx import StopTrainingOnRewardThreshold
    from mgx.ppo import learn
    cb_e = _callback(callback_on_new_best=StopTrainingOnRewardThreshold(-1.0))
    cb_g = _callback(callback_on_new_best=StopTrainingOnRewardThreshold(-1.0))
    _, hist_e, _ = learn(_cfg(), 3 * 8 * 16, callback=cb_e)
    _, hist_g, eng_g = learn(_cfg(graph_collect=True), 3 * 8 * 16, callback=cb_g)
    assert len(hist_e) == len(hist_g) == 1
    _same_history(hist_e, hist_g)
    assert cb_e.evaluations == cb_g.evaluations and len(cb_g.evaluations) == 1
    assert cb_g.evaluations[0][0] == 24 * 8
    assert cb_e.n_calls == cb_g.n_calls == 24                     # nothing was called after the stop
    eng_g.poll_error()


@pytest.mark.parametrize("graph_collect", [True, False])
def test_learn_final_evaluation_through_the_fused_actor(graph_collect):
    """learn(evaluate=True) evaluates through the collector's FusedActor with fused_act, and under graph_collect
    through a GraphEvaluator as well: the mean and std it reports are those of the eager fused loop on an engine in
    the training engine's post-training state (the same learn() without evaluate)."""
    _gpu()
    from mgx import evaluate_policy
    from mgx.fused_policy import FusedActor
    from mgx.ppo import learn
    cfg = _cfg(graph_collect=graph_collect)
    pol_a, hist_a, eng_a = learn(cfg, 2 * 8 * 16, evaluate=True)
    pol_b, hist_b, eng_b = learn(cfg, 2 * 8 * 16)
    for (name, a), (_, b) in zip(pol_a.named_parameters(), pol_b.named_parameters()):
        assert torch.equal(a.detach(), b.detach()), name
    mean, std = evaluate_policy(pol_b, eng_b, cfg.n_eval_episodes, fused=FusedActor(pol_b, eng_b, seed=cfg.seed))
    assert hist_a[-1]["mean_reward"] == mean and hist_a[-1]["std_reward"] == std
    assert "mean_reward" not in hist_b[-1]
    if graph_collect:                                             # stopped at a block boundary
        assert eng_a.calls % eng_a.refill_every == 0 and 0 <= eng_a.calls - eng_b.calls < eng_a.refill_every
    else:
        assert eng_a.calls == eng_b.calls
    eng_a.poll_error()
    eng_b.poll_error()
