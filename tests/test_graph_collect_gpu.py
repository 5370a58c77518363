"""Graph-captured PPO collect on the GPU: mgx_policy_bootstrap against the eager nonzero() + values + index_put_
sequence, and CompactRolloutCollector with PPOConfig.graph_collect against the eager fused_act collector -- bit for
bit throughout (both run the same kernels on the same buffers; the bootstrap's multiply and add are two fp32
operations, as torch's).

Workload: multi 8x8, mission 2 ('pick up'), 4 objects (config 3's PKP 8x8; max_steps 64), 200 envs = 3 full tiles of
64 samples and a tail of 8."""
import copy
import ctypes
import dataclasses
import math

import pytest

torch = pytest.importorskip("torch")

from mgx.policy import ActorCriticPolicy  # noqa: E402

pytestmark = pytest.mark.gpu

N_ENVS = 200
ENV = dict(problem="multi", mission=2, size=8, num_objects=4)
SENTINEL = 0x7FC12345                  # a NaN with a payload: any arithmetic on it, or a rewrite, changes the bits


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bits(x):
    return x.contiguous().view(torch.int32)


def _engine(k, refill_every=0):
    from mgx import MgxEngine
    return MgxEngine(n_envs=N_ENVS, n_stack=k, terminal_mode="truncated", mission_dtype=torch.uint8,
                     refill_every=refill_every, reward64=True, **ENV)


def _redrawn_policy(k, seed=0):
    """Every blob parameter redrawn as tests/test_fused_train_gpu.py does (weights N(0, 1) / sqrt(fan-in), biases
    N(0, 0.5^2)): no bias is zero."""
    from mgx.fused_policy import _params
    torch.manual_seed(seed)
    pol = ActorCriticPolicy(n_stack=k)
    g = torch.Generator().manual_seed(200 + seed)
    _, tensors = _params(pol)
    with torch.no_grad():
        for t in tensors:
            if t.dim() > 1:
                t.copy_(torch.randn(t.shape, generator=g) / math.sqrt(t[0].numel()))
            else:
                t.copy_(0.5 * torch.randn(t.shape, generator=g))
    return pol.cuda()


# ---------------------------------------------------------------- 1. the bootstrap kernel against the existing path
@pytest.mark.parametrize("k", range(1, 9))
def test_bootstrap_equals_eager_sequence_bitwise(k):
    """mgx_policy_bootstrap on a real ring buffer (T = 4) after 9 random-action steps -- 13 at n_stack >= 5, whose
    ring has three blocks -- so that the tested observation sits in the ring's first row and the walk-back of its
    terminal stack wraps.  Random actions rarely end a 'pick up' episode within 13 steps, so a quarter of the start
    flags are also set at random: episode starts fall inside the stack windows of many envs (both paths read the same
    buffer).  terminal_rows hold random bytes.  For every flag pattern: rewards bit-equal to the eager sequence,
    unselected rewards bit-untouched (a NaN-payload sentinel), list / count = nonzero(), the optional values output,
    and a second call on fresh copies gives the same bits."""
    _gpu()
    from mgx.compact import CompactBuffer
    from mgx.fused_policy import FusedActor
    eng = _engine(k)
    dev = eng.device
    buf = CompactBuffer(eng, 4, ring=True)
    fused = FusedActor(_redrawn_policy(k), eng, seed=3)
    g = torch.Generator().manual_seed(11 * k)
    eng.reset()
    buf.observe(0)
    steps = buf.blocks * buf.T + 1
    assert steps == (9 if k <= 4 else 13)
    for s in range(steps):
        if s and s % buf.T == 0:
            buf.carry_over()
        buf.step(s % buf.T, torch.randint(0, 7, (N_ENVS,), generator=g).to(dev))
    t = 1                                           # the observation the last step wrote
    assert buf.row(t) == 0 and buf.R >= k           # the older frames of its stack wrap to the ring's last rows
    buf.starts.bitwise_or_((torch.rand(buf.starts.shape, generator=g) < 0.25).to(torch.uint8).to(dev))
    window = buf.starts[[(buf.row(t) - j) % buf.R for j in range(max(k - 1, 1))]]
    assert bool(window.any()) and not bool(window.all())
    tr = torch.randint(0, 256, buf.terminal_rows.shape, generator=g).to(torch.uint8)
    tr[:, 0] %= 4
    buf.terminal_rows.copy_(tr)
    gamma = 0.8108071290665859
    gamma32 = torch.tensor(gamma, dtype=torch.float32).to(dev)
    sentinel = torch.tensor(SENTINEL, dtype=torch.int32).view(torch.float32).to(dev)

    def flags(trunc=(), term=()):
        a, b = torch.zeros(N_ENVS, dtype=torch.uint8), torch.zeros(N_ENVS, dtype=torch.uint8)
        a[torch.tensor(list(trunc), dtype=torch.int64)] = 1
        b[torch.tensor(list(term), dtype=torch.int64)] = 1
        return a, b

    perm = torch.randperm(N_ENVS, generator=g).tolist()
    patterns = {"none": flags(), "env 0": flags([0]), "env 199": flags([199]), "64": flags(perm[:64]),
                "65": flags(perm[:65]), "all": flags(range(N_ENVS)),
                "terminated too": flags(perm[:90], perm[60:120]),     # 30 of the truncated envs also terminated
                "terminated only": flags([], perm[:50])}
    want_count = {"none": 0, "env 0": 1, "env 199": 1, "64": 64, "65": 65, "all": N_ENVS, "terminated too": 60,
                  "terminated only": 0}
    base = torch.randn(N_ENVS, generator=g).to(dev)
    for name, (trunc, term) in patterns.items():
        buf.truncated[t].copy_(trunc)
        buf.terminated[t].copy_(term)
        sel = buf.truncated[t].bool() & ~buf.terminated[t].bool()
        boot = sel.nonzero().flatten()
        assert boot.numel() == want_count[name], name
        r0 = torch.where(sel, base, sentinel)
        want = r0.clone()
        tv = None
        if boot.numel():                            # the collector's eager sequence
            tv = fused.values(buf, t, terminal=True, envs=boot)
            want.index_put_((boot,), want.index_select(0, boot) + gamma32 * tv)
        got = []
        for rep in range(2):
            r = r0.clone()
            vals = torch.full((N_ENVS,), 7.0, device=dev)
            fused.boot_list.fill_(-1)
            fused.boot_count.fill_(-1)
            out = fused.bootstrap(buf, t, gamma, rewards=r, values=vals)
            assert out is r
            n = int(fused.boot_count)
            got.append((_bits(r).clone(), fused.boot_list[:n].clone(), n, _bits(vals).clone()))
        bits, lst, n, vb = got[0]
        assert n == boot.numel(), name
        assert torch.equal(lst, buf.row(t) * N_ENVS + boot), name
        assert torch.equal(bits, _bits(want)), name
        assert torch.equal(bits[~sel], _bits(r0)[~sel]), name          # untouched, to the bit
        if tv is not None:
            assert torch.equal(vb[:n], _bits(tv)), name
        assert bool((vb[n:] == _bits(torch.full((1,), 7.0, device=dev))).all()), name
        for a, b in zip(got[0], got[1]):
            assert (a == b) if isinstance(a, int) else torch.equal(a, b), name
    # in place in buf.rewards[t] by default
    buf.truncated[t].copy_(patterns["65"][0])
    buf.terminated[t].zero_()
    boot = buf.truncated[t].bool().nonzero().flatten()
    buf.rewards[t].copy_(base)
    want = base.clone()
    want.index_put_((boot,), want.index_select(0, boot) + gamma32 * fused.values(buf, t, terminal=True, envs=boot))
    fused.bootstrap(buf, t, gamma)
    assert torch.equal(_bits(buf.rewards[t]), _bits(want))
    eng.poll_error()


def test_bootstrap_rejects_a_ring_below_n_stack():
    """0 < ring_rows < n_stack reads the handle's n_stack: MGX_ERR_INVALID on a live handle, nothing launched."""
    _gpu()
    from mgx import _lib
    from mgx.compact import CompactBuffer
    from mgx.fused_policy import FusedActor
    eng = _engine(4)
    buf = CompactBuffer(eng, 4, ring=True)
    fused = FusedActor(_redrawn_policy(4), eng)
    eng.reset()
    buf.observe(0)
    fused.bootstrap(buf, 0, 0.5)                     # fills the argument structs
    P = ctypes.c_void_p
    st = eng.L.mgx_policy_bootstrap(eng.h, P(buf.rows.data_ptr()), P(buf.mids.data_ptr()), P(buf.starts.data_ptr()),
                                    N_ENVS, 3, 0, P(buf.terminal_rows.data_ptr()), ctypes.byref(fused._pol),
                                    ctypes.byref(fused._boot), eng._stream())
    assert st == 1 and b"mgx_policy_bootstrap" in eng.L.mgx_last_error()
    with pytest.raises(_lib.MgxError):
        _lib.check(st, "mgx_policy_bootstrap")
    eng.poll_error()


# ---------------------------------------------------------------- 2 - 5. graph collect against eager collect
def _collectors(k, horizon, refill_every, **cfg_kw):
    """(eager, graph) CompactRolloutCollectors with equal seeds, engines and weights; 'done' is rarely chosen
    (action_net.bias[6] = -30 as tests/test_ppo.py), so episodes end by truncation at step 64."""
    from mgx.ppo import CompactRolloutCollector, PPOConfig
    torch.manual_seed(0)
    pol_e = ActorCriticPolicy(n_stack=k).cuda()
    with torch.no_grad():
        pol_e.action_net.bias[6] = -30.0
    pol_g = copy.deepcopy(pol_e)
    cfg = PPOConfig(n_envs=N_ENVS, horizon=horizon, n_frames_stack=k, fused_act=True, env=ENV, seed=5, **cfg_kw)
    ce = CompactRolloutCollector(_engine(k, refill_every), pol_e, cfg)
    cg = CompactRolloutCollector(_engine(k, refill_every), pol_g, dataclasses.replace(cfg, graph_collect=True))
    assert ce.engine.refill_every == cg.engine.refill_every == refill_every
    return ce, cg


def _perturb(ce, cg, i):
    """The same in-place weight change on both policies (an optimiser phase stand-in)."""
    g = torch.Generator().manual_seed(1000 + i)
    with torch.no_grad():
        for a, b in zip(ce.policy.parameters(), cg.policy.parameters()):
            d = (0.02 * torch.randn(a.shape, generator=g)).to(a.device)
            a.add_(d)
            b.add_(d)


def _assert_same_rollout(ce, cg, re, rg, tag):
    be, bg = re.buf, rg.buf
    assert be.c == bg.c and be.block == bg.block, tag
    for name in ("actions", "values", "log_probs", "advantages", "returns", "adv_stats"):
        a, b = getattr(re, name), getattr(rg, name)
        assert torch.equal(a, b), (tag, name)
        if a.dtype == torch.float32:
            assert torch.equal(_bits(a), _bits(b)), (tag, name)
    assert torch.equal(_bits(be.rewards), _bits(bg.rewards)), (tag, "rewards")
    for name in ("terminated", "truncated", "dones"):
        assert torch.equal(getattr(be, name), getattr(bg, name)), (tag, name)
    blk = slice(be.block * be.T, (be.block + 1) * be.T)           # the block this rollout wrote
    assert torch.equal(be.rows[blk], bg.rows[blk]) and torch.equal(be.mids[blk], bg.mids[blk]), (tag, "rows")
    assert torch.equal(be.starts, bg.starts), (tag, "starts")
    assert torch.equal(be.terminal_rows, bg.terminal_rows), (tag, "terminal rows")
    assert torch.equal(_bits(ce.ep_returns), _bits(cg.ep_returns)), (tag, "ep_returns")
    assert torch.equal(_bits(ce.ep_lens), _bits(cg.ep_lens)), (tag, "ep_lens")
    assert ce.num_timesteps == cg.num_timesteps and ce.engine.calls == cg.engine.calls, tag
    assert torch.equal(ce.fused.counter, cg.fused.counter), (tag, "sampling counter")


def _run_pair(ce, cg, rollouts, tag=""):
    """`rollouts` collects of both, weights perturbed in between; ([actions per rollout], bootstraps seen)."""
    acts, boots = [], 0
    for i in range(rollouts):
        if i:
            _perturb(ce, cg, i)
        re, rg = ce.collect(), cg.collect()
        _assert_same_rollout(ce, cg, re, rg, (tag, i))
        acts.append((rg.buf.block, rg.actions.clone()))
        boots += int((rg.buf.truncated.bool() & ~rg.buf.terminated.bool()).sum())
    return acts, boots


def _assert_replays_draw_afresh(acts, blocks):
    for b in range(blocks):
        same = [a for blk, a in acts if blk == b]
        assert len(same) >= 2
        assert not torch.equal(same[0], same[1]), b


def test_graph_collect_equals_eager_collect():
    """n_stack 4, horizon 16, refill_every 16: two ring blocks, 6 rollouts (each graph replayed 3 times; the
    truncations of step 64 fall into the fourth)."""
    _gpu()
    ce, cg = _collectors(4, 16, 16)
    assert cg.rollout.buf.blocks == 2
    ce.start()
    cg.start()
    acts, boots = _run_pair(ce, cg, 6)
    assert len(cg.graphs) == 2
    assert boots > 0, "no truncation bootstrap exercised"
    _assert_replays_draw_afresh(acts, 2)
    ce.engine.poll_error()
    cg.engine.poll_error()


def _collect_before_the_shared_body(col, first):
    """The eager fused_act collect as it stood before the collector had one per-step body, on `col`'s engine, rollout
    and FusedActor: fresh act outputs copied into the rollout arrays, the truncation bootstrap through nonzero() +
    values(terminal=True, envs=boot) + index_put_, the episode statistics through lists of torch.where.  Returns
    (ep_returns, ep_lens, bootstraps)."""
    e, cfg, ro, fused = col.engine, col.cfg, col.rollout, col.fused
    buf = ro.buf
    fused.sync()
    if not first:
        buf.carry_over()
    col.policy.train(False)
    gamma32 = torch.tensor(cfg.gamma, dtype=torch.float32)
    ep_r, ep_l, boots = [], [], 0
    for t in range(cfg.horizon):
        actions, values, log_probs = fused.act(buf, t)
        buf.step(t, actions)
        boot = (buf.truncated[t].bool() & ~buf.terminated[t].bool()).nonzero().flatten()
        if boot.numel():
            boots += int(boot.numel())
            tv = fused.values(buf, t, terminal=True, envs=boot)
            r = buf.rewards[t]
            r.index_put_((boot,), r.index_select(0, boot) + gamma32.to(tv.device) * tv)
        ro.actions[t].copy_(actions)
        ro.values[t].copy_(values)
        ro.log_probs[t].copy_(log_probs)
        d = buf.dones[t].bool()
        ep_r.append(torch.where(d, e.ep_return, torch.nan))
        ep_l.append(torch.where(d, e.ep_len.float(), torch.nan))
    last_values = fused.values(buf, cfg.horizon)
    ro.compute_returns_and_advantage(last_values, cfg.gamma, cfg.gae_lambda)
    r, l = torch.stack(ep_r), torch.stack(ep_l)
    m = ~torch.isnan(r)
    return r[m], l[m], boots


def test_eager_collect_equals_the_sequence_before_the_shared_body():
    """collect() with fused_act on and graph_collect off, pinned to the arithmetic of the eager loop it replaced.
    n_stack 4, horizon 72: the truncations of step 64 fall into the first rollout, those of step 128 into the second,
    which also crosses the ring-block advance; the weights change in between.  Actions, values, log-probs, rewards,
    dones, advantages, returns, adv_stats and the episode statistics are equal bit for bit after each rollout."""
    _gpu()
    # `ref` only lends its engine, rollout and FusedActor: its collect() is never called, so that its config has
    # graph_collect on (a capture stream, the horizon checked against refill_every = 8) plays no part
    ce, ref = _collectors(4, 72, 8)
    ce.start()
    ref.start()
    boots = 0
    for i in range(2):
        if i:
            _perturb(ce, ref, i)
        got = ce.collect()
        ep_r, ep_l, n = _collect_before_the_shared_body(ref, first=(i == 0))
        boots += n
        want = ref.rollout
        assert n == int((got.buf.truncated.bool() & ~got.buf.terminated.bool()).sum()), i
        for name in ("actions", "values", "log_probs", "advantages", "returns", "adv_stats"):
            a, b = getattr(got, name), getattr(want, name)
            assert a.shape == b.shape and torch.equal(a, b), (i, name)
            if a.dtype == torch.float32:
                assert torch.equal(_bits(a), _bits(b)), (i, name)
        assert torch.equal(_bits(got.buf.rewards), _bits(want.buf.rewards)), (i, "rewards")
        for name in ("terminated", "truncated", "dones"):
            assert torch.equal(getattr(got.buf, name), getattr(want.buf, name)), (i, name)
        assert ce.ep_returns.numel() > 0 and ce.ep_returns.shape == ep_r.shape, i
        assert torch.equal(_bits(ce.ep_returns), _bits(ep_r)), (i, "ep_returns")
        assert torch.equal(_bits(ce.ep_lens), _bits(ep_l)), (i, "ep_lens")
        assert torch.equal(ce.fused.counter, ref.fused.counter), (i, "sampling counter")
    assert boots > 0, "no truncation bootstrap exercised"
    assert ce.num_timesteps == 2 * 72 * N_ENVS
    ce.engine.poll_error()
    ref.engine.poll_error()


def test_graph_collect_three_ring_blocks():
    """n_stack 8, horizon 4, refill_every 4: three ring blocks, 18 rollouts."""
    _gpu()
    ce, cg = _collectors(8, 4, 4)
    assert cg.engine.refill_every == 4 and cg.rollout.buf.blocks == 3
    ce.start()
    cg.start()
    acts, boots = _run_pair(ce, cg, 18)
    assert len(cg.graphs) == 3
    assert boots > 0, "no truncation bootstrap exercised"
    _assert_replays_draw_afresh(acts, 3)
    ce.engine.poll_error()
    cg.engine.poll_error()


def test_update_from_graph_collected_rollout():
    """Trainer.train (fused_train + fused_mission + fused_update, one fixed permutation) on the second rollout of
    each collector: the 25 parameters bit-equal -- the block bookkeeping minibatch_indices relies on (buf.c, and so
    buf.index / buf.dones) is that of the replayed block.  Minibatches of 64 samples = one tile each, 8 of them drawn
    from the whole rollout: mgx_policy_backward adds the mission-feature gradient with one fp32 atomic per tile and
    key, so only with one tile per minibatch is an update reproducible to the bit at all (include/mgx.h; with 800-sample
    minibatches two updates from equal rollouts differed by 1 ulp in direction.weight)."""
    _gpu()
    from mgx.ppo import Trainer
    ce, cg = _collectors(4, 16, 16, fused_train=True, fused_mission=True, fused_update=True, batch_size=64,
                         n_epochs=2)
    ce.start()
    cg.start()
    _run_pair(ce, cg, 2)
    assert cg.rollout.buf.block == 1
    perm = torch.randperm(N_ENVS * 16, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))[:256]
    Trainer(ce.policy, ce.cfg).train(ce.rollout, 1.0, perm_fn=lambda n: perm)
    Trainer(cg.policy, cg.cfg).train(cg.rollout, 1.0, perm_fn=lambda n: perm)
    pe, pg = list(ce.policy.named_parameters()), list(cg.policy.named_parameters())
    assert len(pe) == len(pg) == 25
    for (name, a), (_, b) in zip(pe, pg):
        assert torch.equal(_bits(a.detach()), _bits(b.detach())), name
    _run_pair(ce, cg, 1, "after the update")        # the replayed graphs read the updated weights
    cg.engine.poll_error()


def test_start_again_reuses_the_graphs():
    """start() after three graph rollouts, then three more: equal to the eager collector doing the same, with the
    graphs captured before the restart."""
    _gpu()
    ce, cg = _collectors(4, 16, 16)
    ce.start()
    cg.start()
    _run_pair(ce, cg, 3, "first")
    graphs = dict(cg.graphs)
    ce.start()
    cg.start()
    assert cg.engine.calls == 0
    _run_pair(ce, cg, 3, "second")
    assert cg.graphs == graphs                       # nothing captured anew
    cg.engine.poll_error()


def test_learn_with_graph_collect_equals_learn_without():
    """learn() for four iterations (two ring blocks, each graph replayed twice) with every fused flag on, with and
    without graph_collect: with the flag learn() creates the engine with refill_every = 4 for horizon 4 (without, the
    default epoch; transitions do not depend on it), and the 25 parameters and the histories come out bit-equal.
    Minibatches of 64 samples, one tile each: see test_update_from_graph_collected_rollout."""
    _gpu()
    from mgx.ppo import PPOConfig, learn
    cfg = PPOConfig(n_envs=70, horizon=4, batch_size=64, n_epochs=2, fused_act=True, fused_train=True,
                    fused_mission=True, fused_update=True, env=dict(problem="gtg", mission=5, size=6, num_objects=2))
    pol_e, hist_e, eng_e = learn(cfg, 4 * 70 * 4)
    pol_g, hist_g, eng_g = learn(dataclasses.replace(cfg, graph_collect=True), 4 * 70 * 4)
    assert eng_g.refill_every == 4 and eng_e.refill_every != 4
    assert len(hist_e) == len(hist_g) == 4
    for (name, a), (_, b) in zip(pol_e.named_parameters(), pol_g.named_parameters()):
        assert torch.equal(_bits(a.detach()), _bits(b.detach())), name
    for he, hg in zip(hist_e, hist_g):
        assert he.keys() == hg.keys()
        for key in he:
            assert he[key] == hg[key] or (math.isnan(he[key]) and math.isnan(hg[key])), (key, he[key], hg[key])
    eng_g.poll_error()


def test_alignment_and_callback_errors():
    _gpu()
    from mgx.ppo import CompactRolloutCollector, PPOConfig
    pol = ActorCriticPolicy(n_stack=4).cuda()
    cfg = PPOConfig(n_envs=N_ENVS, horizon=24, fused_act=True, graph_collect=True, env=ENV)
    with pytest.raises(ValueError):                  # 24 steps are not whole refill epochs of 16
        CompactRolloutCollector(_engine(4, 16), pol, cfg).collect()
    col = CompactRolloutCollector(_engine(4, 16), pol, dataclasses.replace(cfg, horizon=16))
    col.start()

    class Cb:
        def on_step(self, policy, num_timesteps):
            return True

    with pytest.raises(ValueError):                  # a callback is a host decision per step
        col.collect(callback=Cb())
    buf = col.rollout.buf
    buf.step(0, torch.zeros(N_ENVS, dtype=torch.int64, device=buf.engine.device))
    assert not col.engine.epoch_boundary()
    with pytest.raises(ValueError):                  # the first capture would start mid-epoch
        col.collect()
    assert not col.graphs
    col.engine.poll_error()
