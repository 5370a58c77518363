"""Mission-routed mixture of experts on the GPU (mgx_policy_act_moe, mgx/moe.py).

Reference: the routed expert's own FusedActor (mgx_policy_act), run over the same index with the same seed and the
counter the mixture had before its call.  Every comparison is torch.equal per sample: the mixture runs the same
stage functions with the same weights, so no tolerance is introduced (the per-expert kernel is pinned to the fp64
module by tests/test_fused_policy_gpu.py).

Setup (that file's): multi 8x8, mission=None (dozens of mission ids per tile), a ring CompactBuffer of T = 3, 40
random-action steps over carried-over rollouts, action_net redrawn N(0, 1); 200 envs = three full tiles and a tail.
Each expert is a differently seeded policy."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mgx import _lib  # noqa: E402
from mgx.policy import ActorCriticPolicy  # noqa: E402

pytestmark = pytest.mark.gpu

N_ENVS, T_RING, STEPS, SEED = 200, 3, 40, 1234
MULTI = dict(problem="multi", mission=None, size=8, num_objects=4)
TASKS4 = ("GTO", "TGL", "PKP", "GTG")


def _policy(k, seed):
    torch.manual_seed(seed)
    pol = ActorCriticPolicy(n_stack=k)
    g = torch.Generator().manual_seed(100 + seed)
    with torch.no_grad():
        pol.action_net.weight.copy_(torch.randn(pol.action_net.weight.shape, generator=g))
        pol.action_net.bias.copy_(torch.randn(pol.action_net.bias.shape, generator=g))
    pol.train(False)
    return pol


def _task_route(n_experts):
    """Route by task over the ids of `multi`: task j of TASKS4 -> expert j % E."""
    from mgx.moe import route_by_task
    return route_by_task({t: j % n_experts for j, t in enumerate(TASKS4)}, ids=range(128))


class Run:
    pass


_RUNS = {}


def _run(k):
    """One 40-step trajectory per n_stack, 8 expert policies and their own FusedActors, made once."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if k in _RUNS:
        return _RUNS[k]
    from mgx import MgxEngine
    from mgx.compact import CompactBuffer
    from mgx.fused_policy import FusedActor
    r = Run()
    r.k = k
    r.eng = MgxEngine(n_envs=N_ENVS, n_stack=k, terminal_mode="truncated", mission_dtype=torch.uint8, **MULTI)
    r.buf = CompactBuffer(r.eng, T_RING, ring=True)
    r.pols = [_policy(k, s).cuda() for s in range(8)]
    r.refs = [FusedActor(p, r.eng, seed=SEED) for p in r.pols]
    r.eng.reset()
    r.buf.observe(0)
    g = torch.Generator().manual_seed(5)
    t = ends = 0
    for _ in range(STEPS):
        r.buf.step(t, torch.randint(0, 7, (N_ENVS,), generator=g).cuda())
        ends += int(r.buf.dones[t].sum())
        t += 1
        if t == T_RING:
            r.buf.carry_over()
            t = 0
    assert ends > 0                                       # episode starts fall inside stack windows
    r.t = t                                               # the buffer is left at observation t
    r.index = r.buf.index(t, r.buf._arange).contiguous()
    r.mids = r.buf.mids[r.buf.row(t)].cpu().numpy()
    r.eng.poll_error()
    _RUNS[k] = r
    return r


def _moe_actor(r, n_experts, route):
    from mgx.moe import FusedMoEActor, MoEPolicy
    moe = MoEPolicy(r.pols[:n_experts], route)
    return moe, FusedMoEActor(moe, r.eng, seed=SEED)


def _reference(r, index, which, mode, terminal, counter):
    """Per sample, the routed expert's own launch over the whole index: (actions, values, log_probs, logits)."""
    n = index.numel()
    dev = r.eng.device
    out = [torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev),
           torch.zeros((n, 7), device=dev)]
    for x in sorted(set(int(w) for w in which.tolist())):
        ref = r.refs[x]
        ref.counter[0] = counter
        got = ref._run(r.buf, index, mode, terminal=terminal, logits=True)
        assert int(ref.counter[0]) == counter + (mode == 2)
        sel = torch.as_tensor(which == x, device=dev)
        for o, gx in zip(out, got):
            if gx is not None:
                o[sel] = gx[sel]
    return out


def _assert_equals_experts(r, actor, route, index, mode, terminal=False):
    """One mixture call against the per-expert launches, bit for bit; returns the mixture's outputs."""
    mids = r.buf.mids.flatten()[index].cpu().numpy()
    which = np.asarray(route)[mids]
    c0 = int(actor.counter[0])
    a, v, lp, lg = actor._run(r.buf, index, mode, terminal=terminal, logits=True)
    assert int(actor.counter[0]) == c0 + (mode == 2)      # the pair of launches advances it by exactly one
    wa, wv, wlp, wlg = _reference(r, index, which, mode, terminal, c0)
    assert torch.equal(v, wv) and torch.equal(lg, wlg)
    if mode:
        assert torch.equal(a, wa) and torch.equal(lp, wlp)
    else:
        assert a is None and lp is None
    rec = actor.last_route.cpu().numpy()
    counts = np.bincount(which, minlength=8)
    assert rec[1:16:2].tolist() == counts.tolist() and rec[17] == 0
    return a, v, lp, lg


@pytest.mark.parametrize("n_experts", [1, 2, 4, 8])
@pytest.mark.parametrize("k", [1, 4, 8])
def test_mixture_equals_routed_experts_bit_for_bit(k, n_experts):
    """act (deterministic and sampled) and values(terminal=True) of the mixture equal, per sample, the routed
    expert's own FusedActor at the same seed and counter; the counter advances by one per sampled call."""
    r = _run(k)
    synthetic = torch.arange(256) % n_experts
    for route in (_task_route(n_experts), synthetic.to(torch.uint8)):
        moe, actor = _moe_actor(r, n_experts, route)
        actor.counter[0] = 7
        which = route.numpy()[r.mids]
        assert len(set(which.tolist())) >= min(n_experts, 2)          # the routing is not trivial
        for mode, terminal in ((1, False), (2, False), (2, False), (0, True), (0, False)):
            _assert_equals_experts(r, actor, route, r.index, mode, terminal)
        assert int(actor.counter[0]) == 9
        # the public methods are those calls
        a, v, lp = actor.act(r.buf, r.t, deterministic=True)
        a1, v1, lp1, lg1 = actor._run(r.buf, r.index, 1, logits=True)
        assert torch.equal(a, a1) and torch.equal(v, v1) and torch.equal(lp, lp1)
        assert torch.equal(actor.values(r.buf, r.t, terminal=True), actor._run(r.buf, r.index, 0, terminal=True)[1])
        lg, v0 = actor.logits(r.buf, r.t)
        assert torch.equal(lg, lg1) and torch.equal(v0, v1)
        # the torch restatement routes the gathered observation the same way
        obs = r.buf.gather_step(r.t, f32=False)
        assert moe.experts_of(obs).cpu().tolist() == which.tolist()
    r.eng.poll_error()


@pytest.mark.parametrize("k", [1, 4, 8])
def test_one_expert_is_the_plain_actor(k):
    """E = 1 with route = 0 everywhere: the plain FusedActor's outputs, bit for bit, in all three modes."""
    r = _run(k)
    _, actor = _moe_actor(r, 1, torch.zeros(256, dtype=torch.uint8))
    ref = r.refs[0]
    for mode, terminal in ((0, False), (0, True), (1, False), (2, False), (2, True)):
        actor.counter[0] = ref.counter[0] = 41
        got = actor._run(r.buf, r.index, mode, terminal=terminal, logits=True)
        want = ref._run(r.buf, r.index, mode, terminal=terminal, logits=True)
        for g, w in zip(got, want):
            assert (g is None and w is None) or torch.equal(g, w)
        assert int(actor.counter[0]) == int(ref.counter[0]) == 41 + (mode == 2)
    rec = actor.last_route.cpu().numpy()
    assert rec[:2].tolist() == [0, N_ENVS] and rec[16] == 4 and rec[17] == 0


CORNER_COUNTS = {0: 0, 1: 1, 2: 64, 3: 65, 4: 150, 5: 63, 6: 0, 7: 128}


def _corner_case(r):
    """An 8-expert table over the step's mission ids and an env list (with repeats) whose per-expert counts are
    CORNER_COUNTS: 0, 1, 64, 65 and > 128 at once."""
    ids, freq = np.unique(r.mids, return_counts=True)
    ids = ids[np.argsort(-freq, kind="stable")]
    assert ids.size >= 6
    route = np.zeros(256, np.uint8)                       # ids absent from the step -> expert 0, which stays empty
    targets = [e for e, c in CORNER_COUNTS.items() if c]
    for i, m in enumerate(ids):
        route[m] = targets[i % len(targets)]
    which = route[r.mids]
    envs = []
    for e, c in CORNER_COUNTS.items():
        mine = np.nonzero(which == e)[0]
        assert c == 0 or mine.size
        envs += np.resize(mine, c).tolist() if c else []
    return torch.from_numpy(route), np.sort(np.asarray(envs, dtype=np.int64))


@pytest.mark.parametrize("shuffled", [False, True], ids=["ascending", "shuffled"])
def test_segment_corners_match_the_reference(shuffled):
    """Counts of exactly 0, 1, 64, 65 and > 128 at once, over an env list with duplicates: the device lists, the
    segment records and the tile count equal moe_route_reference, and every position equals the per-expert launch."""
    from mgx.moe import moe_route_reference, scratch_views
    r = _run(4)
    route, envs = _corner_case(r)
    if shuffled:
        envs = envs[np.random.default_rng(11).permutation(envs.size)]
    assert np.unique(envs).size < envs.size               # duplicates
    _, actor = _moe_actor(r, 8, route)
    envs_dev = torch.from_numpy(envs).to(r.eng.device)
    index = r.buf.index(r.t, envs_dev).contiguous()
    n = index.numel()
    for mode, terminal in ((1, False), (2, False), (0, True)):
        _assert_equals_experts(r, actor, route, index, mode, terminal)
    a, v, lp = actor.act(r.buf, r.t, deterministic=True, envs=envs_dev)         # the envs= path: the same index
    a1, v1, lp1, _ = actor._run(r.buf, index, 1)
    assert torch.equal(a, a1) and torch.equal(v, v1) and torch.equal(lp, lp1)
    want = moe_route_reference(r.mids[envs], route.numpy(), 8, index=index.cpu().numpy())
    assert [int(c) for c in want["segments"][:, 1]] == list(CORNER_COUNTS.values())
    rec, lst, pos = (x.cpu().numpy() for x in scratch_views(actor.scratch, n, 8))
    assert rec[:16].reshape(8, 2).tolist() == want["segments"].tolist()
    assert rec[16] == want["tiles"] <= want["cap"] // 64 and rec[17] == want["unroutable"] == 0
    assert rec[20:].tolist() == [0] * 12
    for e in range(8):
        s, c = (int(x) for x in want["segments"][e])
        assert pos[s:s + c].tolist() == want["pos"][s:s + c].tolist()
        assert lst[s:s + c].tolist() == want["list"][s:s + c].tolist()
    r.eng.poll_error()


def test_unroutable_samples_are_counted_and_left_untouched():
    """Route bytes >= n_experts, through the raw call (MoEPolicy refuses such a table): pre-filled outputs keep
    their fill at those positions, the count is reported, every other position is the routed expert's."""
    from mgx.moe import moe_act, moe_route_reference, scratch_views, scratch_words
    r = _run(4)
    n, dev, E = N_ENVS, r.eng.device, 2
    route = (torch.arange(256) % 4).to(torch.uint8)       # experts 2 and 3 do not exist
    which = route.numpy()[r.mids]
    bad = which >= E
    assert 0 < bad.sum() < n
    scratch = torch.full((scratch_words(n, E),), -5, dtype=torch.int32, device=dev)      # need not be zeroed
    counter = torch.tensor([3, 0], dtype=torch.int64, device=dev)
    route_dev = route.to(dev)
    p = _lib.MgxPolicyMoe(n_experts=E, mode=2, route_dev=route_dev.data_ptr(), seed=SEED,
                          counter_dev=counter.data_ptr(), scratch_dev=scratch.data_ptr(),
                          scratch_words=scratch.numel())
    for x in range(E):
        p.blob_dev[x], p.mission_feat_dev[x] = r.refs[x].blob.data_ptr(), r.refs[x].mission_feat.data_ptr()
    a = torch.full((n,), -7, dtype=torch.int64, device=dev)
    v, lp, lg = (torch.full(s, 1234.5, device=dev) for s in ((n,), (n,), (n, 7)))
    moe_act(r.eng, r.buf, r.index, p, _lib.MgxActOut(), v, a, lp, lg)
    assert int(counter[0]) == 4
    rec, _, pos = (x.cpu().numpy() for x in scratch_views(scratch, n, E))
    want = moe_route_reference(r.mids, route.numpy(), E)
    assert rec[17] == want["unroutable"] == int(bad.sum())
    assert rec[:16].reshape(8, 2).tolist() == want["segments"].tolist() and rec[16] == want["tiles"]
    live = want["pos"] >= 0
    assert pos[live].tolist() == want["pos"][live].tolist()
    bad_dev = torch.as_tensor(bad, device=dev)
    assert bool((a[bad_dev] == -7).all()) and bool((v[bad_dev] == 1234.5).all())
    assert bool((lp[bad_dev] == 1234.5).all()) and bool((lg[bad_dev] == 1234.5).all())
    wa, wv, wlp, wlg = _reference(r, r.index, np.where(bad, 0, which), 2, False, 3)
    ok = ~bad_dev
    assert torch.equal(a[ok], wa[ok]) and torch.equal(v[ok], wv[ok])
    assert torch.equal(lp[ok], wlp[ok]) and torch.equal(lg[ok], wlg[ok])
    r.eng.poll_error()


def test_captured_act_draws_afresh_on_every_replay():
    """Two replays of a captured sampled act draw different actions, each the eager call's at the same counter."""
    r = _run(4)
    route = _task_route(4)
    _, actor = _moe_actor(r, 4, route)
    dev = r.eng.device
    out = (torch.zeros(N_ENVS, dtype=torch.int64, device=dev), torch.zeros(N_ENVS, device=dev),
           torch.zeros(N_ENVS, device=dev))
    actor.counter[0] = 20
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        actor._run(r.buf, r.index, 2, out=out)
    torch.cuda.synchronize()
    assert int(actor.counter[0]) == 20                    # captured, not run
    replays = []
    for i in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert int(actor.counter[0]) == 21 + i
        replays.append([x.clone() for x in out])
    assert not torch.equal(replays[0][0], replays[1][0])
    actor.counter[0] = 20
    for i in range(2):
        a, v, lp, _ = actor._run(r.buf, r.index, 2)
        assert torch.equal(a, replays[i][0]) and torch.equal(v, replays[i][1]) and torch.equal(lp, replays[i][2])
    _assert_equals_experts(r, actor, route, r.index, 2)
    r.eng.poll_error()


@pytest.mark.parametrize("deterministic", [True, False], ids=["deterministic", "sampled"])
def test_graph_evaluation_of_the_mixture_equals_eager(deterministic):
    """GraphEvaluator(moe_actor).evaluate equals evaluate_policy(moe, engine, fused=moe_actor) episode for episode
    (two engines of equal seed), evaluate_policy(..., graph=True) too, and summarize_missions' per-task episode
    counts sum to the total."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgx import GraphEvaluator, MgxEngine, evaluate_policy, summarize_missions
    from mgx.moe import FusedMoEActor, MoEPolicy
    k, n_envs, n_eval = 4, 16, 40
    pols = [_policy(k, s).cuda() for s in range(4)]
    moe = MoEPolicy(pols, _task_route(4))
    engs = [MgxEngine(n_envs=n_envs, n_stack=k, seed=42, terminal_mode="truncated", mission_dtype=torch.uint8,
                      refill_every=16, reward64=True, **MULTI) for _ in range(3)]
    actors = [FusedMoEActor(moe, e, seed=9) for e in engs]
    want = evaluate_policy(moe, engs[0], n_eval, deterministic, return_episode_rewards=True, fused=actors[0])
    ev = GraphEvaluator(actors[1])
    got = ev.evaluate(n_eval, deterministic, return_episode_rewards=True)
    assert got == want and len(got[0]) == n_eval
    assert evaluate_policy(moe, engs[2], n_eval, deterministic, return_episode_rewards=True, fused=actors[2],
                           graph=True) == want
    s = summarize_missions(got[0], got[1], ev.last["mission_ids"])
    assert s["overall"]["episodes"] == n_eval == sum(v["episodes"] for v in s["per_task"].values())
    assert set(s["per_task"]) <= set(TASKS4) and len(s["per_task"]) > 1
    counts = actors[1].last_route.cpu().numpy()[1:8:2]
    assert counts.sum() == n_envs                         # the last step's segment record: every env routed
    for e in engs:
        e.poll_error()
