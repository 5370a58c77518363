"""Carrying a run across a checkpoint on the fused update paths, on the GPU: a checkpoint loaded into a live
Trainer, into fresh objects and through learn(init=...), and a state_dict loaded under a live FusedActor /
GraphEvaluator.  Workload and helpers are tests/test_graph_train_gpu.py's (multi mission 2 at 8 x 8, 8 envs x 16
steps, minibatches 48 / 48 / 32, 2 epochs, n_stack 4: six Adam steps per round).

Every checkpoint goes through torch.save and torch.load(map_location="cuda", weights_only=True), as
tools/ppo_learn.py's --save / --resume do.  Every comparison is bit for bit: both sides run the same launches on the
same inputs, so there is no tolerance."""
import dataclasses
import math

import pytest

torch = pytest.importorskip("torch")

import test_graph_eval_gpu as E  # noqa: E402
import test_graph_train_gpu as G  # noqa: E402

pytestmark = pytest.mark.gpu

K = 4
GRAPH = pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])


def _checkpoint(pol, path, **extra):
    """tools/ppo_learn.py's checkpoint of `pol`, written to `path`."""
    torch.cuda.synchronize()
    torch.save(dict(policy=pol.state_dict(), optimizer=pol.optimizer.state_dict(), **extra), path)
    return path


def _load(path):
    return torch.load(path, map_location="cuda", weights_only=True)


def _load_in_place(pol, ck):
    pol.load_state_dict(ck["policy"])
    pol.optimizer.load_state_dict(ck["optimizer"])


@pytest.fixture(scope="module")
def after_round_0(tmp_path_factory):
    """The checkpoint of the reference run after its round 0: an eager leg of the reference's seeds run for that
    one round, which is the reference's round 0 bit for bit."""
    G._gpu()
    want = G._eager_rounds(K)
    col, tr = G._leg(G._cfg(K, False))
    G._assert_round(G._round(col, tr, G.PROGRESS[0]), want[0], "the checkpointed leg")
    col.engine.poll_error()
    return _checkpoint(tr.policy, tmp_path_factory.mktemp("resume") / "round0.pt")


@GRAPH
def test_live_in_place_resume(graph, after_round_0):
    """A leg runs round 0, so that its engine, collector, sampler counter and permutation generator are in the
    reference's state; its parameters, both moments and its step count are then scrambled (no generator touched) and
    the reference's round-0 checkpoint is loaded into the live policy and optimizer.  Rounds 1 and 2 equal the
    uninterrupted reference's: parameters, both moments, arena.step 12 then 18, statistics, state_dict steps.  With
    graph_train the captured epoch graphs and the Adam schedule's first step follow the import; either way the
    collector's FusedActor.sync() picks the loaded weights up."""
    G._gpu()
    want = G._eager_rounds(K)
    col, tr = G._leg(G._cfg(K, graph))
    G._assert_round(G._round(col, tr, G.PROGRESS[0]), want[0], (graph, 0))
    arena = tr.update.arena
    with torch.no_grad():
        for p in tr.policy.parameters():
            p.mul_(1.25)
    arena.exp_avg.fill_(0.5)
    arena.exp_avg_sq.fill_(0.25)
    arena.step = 99
    arena.export_state()
    assert not any(G._same(p, q) for p, q in zip(tr.policy.parameters(), want[0]["params"]) if p.dim() > 1)
    _load_in_place(tr.policy, _load(after_round_0))
    assert arena.attached()
    for i in (1, 2):
        got = G._round(col, tr, G.PROGRESS[i])
        G._assert_round(got, want[i], (graph, i))
        assert got["step"] == 6 * (i + 1)
        assert got["stats"]["lr"] == tr.lr_schedule(G.PROGRESS[i])
    assert tr.update.arena is arena
    if graph:
        assert tr.update._gbuf["cursor"].tolist() == [6, 0]
    col.engine.poll_error()


@GRAPH
def test_fresh_object_resume(graph, tmp_path):
    """Checkpoint after round 0, then one rollout: the leg trains on it, and a differently seeded fresh policy with a
    fresh Trainer that loaded the checkpoint trains on the same rollout object with the same progress and the same
    fixed permutations.  Parameters, both moments, the step (12), the statistics and the state_dict steps are
    equal."""
    G._gpu()
    from mgx.policy import ActorCriticPolicy
    from mgx.ppo import Trainer
    cfg = G._cfg(K, graph)
    col, tr = G._leg(cfg)
    G._round(col, tr, G.PROGRESS[0])
    path = _checkpoint(tr.policy, tmp_path / "round0.pt")
    ro = col.collect()
    g = torch.Generator().manual_seed(77)
    perms = [torch.randperm(ro.T * ro.N, generator=g).cuda() for _ in range(cfg.n_epochs)]

    def run(trainer):
        it = iter(perms)
        st = trainer.train(ro, G.PROGRESS[1], perm_fn=lambda n: next(it))
        torch.cuda.synchronize()
        a = trainer.update.arena
        sd = trainer.policy.optimizer.state_dict()["state"]
        return dict(params=[p.detach().clone() for p in a.tensors], exp_avg=a.exp_avg.clone(),
                    exp_avg_sq=a.exp_avg_sq.clone(), step=a.step, stats=st,
                    sd_steps=[int(s["step"]) for s in sd.values()])

    want = run(tr)
    torch.manual_seed(123)
    pol = ActorCriticPolicy(n_stack=K).cuda()
    assert not any(G._same(p, q) for p, q in zip(pol.parameters(), tr.policy.parameters()) if p.dim() > 1)
    _load_in_place(pol, _load(path))
    fresh = Trainer(pol, cfg)
    got = run(fresh)
    assert fresh.update is not tr.update and fresh.update.arena.attached()
    assert got["step"] == want["step"] == 12 and got["sd_steps"] == want["sd_steps"] == [12] * 25
    assert got["stats"] == want["stats"] and all(math.isfinite(x) for x in got["stats"].values()), (got, want)
    for i, (x, y) in enumerate(zip(got["params"], want["params"])):
        assert G._same(x, y), ("parameter", i)
    assert G._same(got["exp_avg"], want["exp_avg"]) and G._same(got["exp_avg_sq"], want["exp_avg_sq"])
    assert got["exp_avg"].any() and got["exp_avg_sq"].any()
    col.engine.poll_error()


def test_learn_init_continues_the_run(tmp_path):
    """learn() for two iterations with all six flags on, checkpointed as tools/ppo_learn.py does; learn(init=...)
    then continues it to four iterations twice with one seed_offset, with graph_collect + graph_train on and with
    both off.  Both return the iterations at 384 and 512 timesteps, the learning-rate schedule continues from the
    checkpoint's timesteps, histories, state_dicts and moments are equal, every step count is 24 (12 loaded + 12),
    every parameter moved, and neither engine reports an error."""
    G._gpu()
    from mgx.ppo import PPOConfig, learn, linear_schedule
    cfg = PPOConfig(n_envs=8, horizon=16, batch_size=48, n_epochs=2, fused_act=True, fused_train=True,
                    fused_mission=True, fused_update=True, graph_collect=True, graph_train=True, env=G.ENV)
    pol0, hist0, eng0 = learn(cfg, 2 * 128)
    assert [h["timesteps"] for h in hist0] == [128, 256]
    path = _checkpoint(pol0, tmp_path / "segment0.pt", timesteps=hist0[-1]["timesteps"], curve=[], train_seconds=0.0,
                       segment=0)
    eng0.poll_error()

    def resume(c):
        ck = _load(path)                                       # as a new process would: its own tensors
        init = {"policy": ck["policy"], "optimizer": ck["optimizer"], "timesteps": int(ck["timesteps"]),
                "seed_offset": 1000003 * (int(ck["segment"]) + 1)}
        return learn(c, 4 * 128, init=init)

    pol_g, hist_g, eng_g = resume(cfg)
    pol_e, hist_e, eng_e = resume(dataclasses.replace(cfg, graph_collect=False, graph_train=False))
    lr = linear_schedule(cfg.initial_learning_rate, cfg.final_learning_rate)
    for hist in (hist_g, hist_e):
        assert [h["timesteps"] for h in hist] == [384, 512]
        assert hist[0]["lr"] == lr(1.0 - 384.0 / 512.0) and hist[1]["lr"] == lr(0.0)
    for hg, he in zip(hist_g, hist_e):
        assert hg.keys() == he.keys()
        for key in hg:
            assert hg[key] == he[key] or (math.isnan(hg[key]) and math.isnan(he[key])), (key, hg[key], he[key])
    ck = _load(path)
    sg, se = pol_g.state_dict(), pol_e.state_dict()
    assert sg.keys() == se.keys() == ck["policy"].keys() and len(sg) >= 25
    for name in sg:
        assert G._same(sg[name], se[name]) if sg[name].dtype == torch.float32 else torch.equal(sg[name], se[name]), name
    for name, p in pol_g.named_parameters():
        assert not G._same(p, ck["policy"][name]), name
    og, oe = pol_g.optimizer.state_dict()["state"], pol_e.optimizer.state_dict()["state"]
    assert len(og) == len(oe) == 25
    for i in og:
        assert int(og[i]["step"]) == int(oe[i]["step"]) == 24
        assert int(ck["optimizer"]["state"][i]["step"]) == 12
        assert G._same(og[i]["exp_avg"], oe[i]["exp_avg"]) and G._same(og[i]["exp_avg_sq"], oe[i]["exp_avg_sq"]), i
    eng_g.poll_error()
    eng_e.poll_error()


@pytest.mark.parametrize("fused_mission", [False, True], ids=["table", "fused_mission"])
def test_inference_after_in_place_load(fused_mission, tmp_path):
    """A differently seeded policy's state_dict loaded into a policy that already has a FusedActor and a
    GraphEvaluator with captured blocks.  After actor.sync(), act(deterministic, logits) equals that of a fresh actor
    on a fresh policy holding the state, over six steps of two engines in one state; GraphEvaluator.evaluate(8) then
    returns the eager fused loop's episodes, replaying the blocks it captured before the load.

    The two engines are brought to one state as tests/test_graph_eval_gpu.py::test_one_evaluator_evaluates_twice
    does: the same first graph evaluation on both, then set_seed."""
    G._gpu()
    from mgx import GraphEvaluator, evaluate_policy
    from mgx.compact import CompactBuffer
    from mgx.fused_policy import FusedActor, pack_blob
    env, n_envs, n_eval = E.CONFIGS[0][1], 16, 8
    pol = E._policy(K, seed=0)
    eng, twin = E._engine(env, n_envs, K, 16), E._engine(env, n_envs, K, 16)
    actor = FusedActor(pol, eng, seed=9, fused_mission=fused_mission)
    ev = GraphEvaluator(actor)
    first = ev.evaluate(n_eval, return_episode_rewards=True)
    warm = GraphEvaluator(FusedActor(E._policy(K, seed=0), twin, seed=9, fused_mission=fused_mission))
    assert warm.evaluate(n_eval, return_episode_rewards=True) == first
    graphs = dict(ev.graphs)
    assert graphs
    eng.set_seed(42)
    twin.set_seed(42)
    path = tmp_path / "donor.pt"
    torch.save(E._policy(K, seed=1).state_dict(), path)
    old_blob, old_feat = actor.blob.clone(), actor.mission_feat.clone()
    pol.load_state_dict(_load(path))
    actor.sync()
    assert not torch.equal(actor.blob, old_blob) and not torch.equal(actor.mission_feat, old_feat)
    fresh_pol = E._policy(K, seed=2)
    fresh_pol.load_state_dict(_load(path))
    fresh = FusedActor(fresh_pol, twin, seed=9, fused_mission=fused_mission)
    assert torch.equal(actor.blob, pack_blob(fresh_pol)) and G._same(actor.blob, fresh.blob)
    assert G._same(actor.mission_feat, fresh.mission_feat)
    bufs = []
    for e in (eng, twin):
        e.reset()
        bufs.append(CompactBuffer(e, max(2, e.n_stack), ring=True))
        bufs[-1].observe(0)
    bt = 0
    for t in range(6):
        a = actor.act(bufs[0], bt, deterministic=True, logits=True)
        b = fresh.act(bufs[1], bt, deterministic=True, logits=True)
        assert torch.equal(a[0], b[0]), t
        for name, x, y in zip(("values", "log_probs", "logits"), a[1:], b[1:]):
            assert G._same(x, y) and bool(torch.isfinite(x).all()), (t, name)
        bufs[0].step(bt, a[0])
        bufs[1].step(bt, b[0])
        bt += 1
        if bt == bufs[0].T:
            bufs[0].carry_over()
            bufs[1].carry_over()
            bt = 0
    got = ev.evaluate(n_eval, return_episode_rewards=True)
    want = evaluate_policy(fresh_pol, twin, n_eval, return_episode_rewards=True, fused=fresh)
    assert got == want and len(got[0]) == n_eval
    assert twin.calls == ev.last["steps_needed"]
    assert all(ev.graphs[key] is g for key, g in graphs.items())       # the blocks captured before the load
    eng.poll_error()
    twin.poll_error()
