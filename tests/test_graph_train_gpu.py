"""Graph-captured PPO update on the GPU (PPOConfig.graph_train): mgx_adam_step_sched against
mgx_adam_step, the mission _rows calls against forward + index_copy_ / index_select + backward, and Trainer.train /
learn() with the flag against the same without it.

Every comparison is bit for bit (torch.equal on the raw tensors, floats through their int32 view so that NaN and -0
count): both legs run the same arithmetic in the same order, so there is no tolerance.

Minibatches hold at most 64 samples (one tile of mgx_policy_backward) throughout: with more than one tile per
minibatch the mission-feature gradient is added by fp32 atomics and two eager updates already differ in the last bit
(tests/test_graph_collect_gpu.py::test_update_from_graph_collected_rollout)."""
import copy
import dataclasses
import math

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ENV = dict(problem="multi", mission=2, size=8, num_objects=4)
SENTINEL = 0x7FC12345                  # a NaN with a payload: any arithmetic on it, or a rewrite, changes the bits
BETAS, ADAM_EPS = (0.9, 0.999), 1e-8
MAX_NORM = 0.5215982006116593
LRS = (3e-4, 1.1e-4, 3e-6, 2.5e-4, 7e-5, 1e-5)
FIRST_STEP = 5
ADAM_WORDS = (1, 255, 1025, 110216, 300001)         # 300,001 > 256 workgroups x 1,024 words: the grid-stride case


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bits(x):
    return x.detach().contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------- mgx_adam_step_sched
def _adam_inputs(n, case):
    """(param, six gradients) on the GPU; gradient norm 4 x max_grad_norm (clip, off) or a quarter of it (noclip)."""
    g = torch.Generator().manual_seed(3000 + n)
    target = MAX_NORM * (0.25 if case == "noclip" else 4.0)
    param = torch.randn(n, generator=g).cuda()
    grads = []
    for _ in range(6):
        x = torch.randn(n, generator=g)
        grads.append((x * (target / max(float(x.norm()), 1e-30))).float().cuda())
    return param, grads


def _eager_adam(param, grads, lrs, first, max_norm, scale):
    """mgx_adam_step per gradient -> per step (param, grad, exp_avg, exp_avg_sq, total_norm)."""
    from mgx.fused_update import adam_step
    p = param.clone()
    m, v, norm = torch.zeros_like(p), torch.zeros_like(p), torch.zeros(1, device="cuda")
    out = []
    for i, (g, lr) in enumerate(zip(grads, lrs)):
        gg = g.clone()
        adam_step(p, gg, m, v, lr, first + i, betas=BETAS, eps=ADAM_EPS, max_grad_norm=max_norm, grad_scale=scale,
                  total_norm=norm)
        out.append(tuple(x.clone() for x in (p, gg, m, v, norm)))
    return out


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("case", ["clip", "noclip", "off"])
@pytest.mark.parametrize("n", ADAM_WORDS)
def test_adam_step_sched_equals_adam_step(n, case, scale):
    """Three consecutive steps with three lrs from one table: param, the written-back gradient, both moments and the
    total norm equal three mgx_adam_step calls after every step; the cursor ends at {3, 0}.  A fourth call on the
    3-entry table changes none of them and leaves the cursor at {4, 1}."""
    _gpu()
    from mgx.fused_update import adam_schedule, adam_step_sched
    max_norm = 0.0 if case == "off" else MAX_NORM
    param, grads = _adam_inputs(n, case)
    want = _eager_adam(param, grads[:3], LRS[:3], FIRST_STEP, max_norm, scale)
    clipped = float(want[0][1].norm()) < 0.99 * float(grads[0].norm()) * scale
    assert clipped == (case == "clip")
    table = adam_schedule(LRS[:3], FIRST_STEP, betas=BETAS, eps=ADAM_EPS).cuda()
    cursor = torch.zeros(2, dtype=torch.int32, device="cuda")
    p = param.clone()
    m, v, norm = torch.zeros_like(p), torch.zeros_like(p), torch.zeros(1, device="cuda")
    kw = dict(betas=BETAS, eps=ADAM_EPS, max_grad_norm=max_norm, grad_scale=scale, total_norm=norm)
    for i in range(3):
        gg = grads[i].clone()
        adam_step_sched(p, gg, m, v, table, cursor, **kw)
        for name, x, y in zip(("param", "grad", "exp_avg", "exp_avg_sq", "total_norm"), (p, gg, m, v, norm), want[i]):
            assert _same(x, y), (i, name)
        assert cursor.tolist() == [i + 1, 0]
    gg = grads[3].clone()
    before = tuple(x.clone() for x in (p, gg, m, v, norm))
    adam_step_sched(p, gg, m, v, table, cursor, **kw)
    for name, x, y in zip(("param", "grad", "exp_avg", "exp_avg_sq", "total_norm"), (p, gg, m, v, norm), before):
        assert _same(x, y), ("past the table", name)
    assert cursor.tolist() == [4, 1]
    assert not _same(p, param)


@pytest.mark.parametrize("n", ADAM_WORDS)
def test_adam_step_sched_captured_graph_replays(n):
    """The three calls captured once and replayed twice -- the table rewritten for the next three steps and lrs, the
    cursor zeroed and the gradients refilled in between -- equal six eager mgx_adam_step calls: nothing of (lr, step)
    is baked in.  Clip active, grad_scale 0.5."""
    _gpu()
    from mgx import _lib
    from mgx.fused_update import adam_schedule, adam_step_sched
    scale = 0.5
    param, grads = _adam_inputs(n, "clip")
    want = _eager_adam(param, grads, LRS, FIRST_STEP, MAX_NORM, scale)
    table = torch.zeros((3, 2), device="cuda")
    cursor = torch.zeros(2, dtype=torch.int32, device="cuda")
    p = param.clone()
    m, v, norm = torch.zeros_like(p), torch.zeros_like(p), torch.zeros(1, device="cuda")
    gbuf = [torch.zeros_like(p) for _ in range(3)]
    scratch = torch.empty(int(_lib.load().mgx_adam_scratch_words(n)), device="cuda")
    snap = tuple(x.clone() for x in (p, m, v))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(3):
            adam_step_sched(p, gbuf[i], m, v, table, cursor, betas=BETAS, eps=ADAM_EPS, max_grad_norm=MAX_NORM,
                            grad_scale=scale, total_norm=norm, scratch=scratch)
    torch.cuda.synchronize()
    for x, y in zip((p, m, v), snap):
        assert _same(x, y)                          # the capture executed nothing
    assert cursor.tolist() == [0, 0]
    for r in range(2):
        table.copy_(adam_schedule(LRS[3 * r:3 * r + 3], FIRST_STEP + 3 * r, betas=BETAS, eps=ADAM_EPS))
        cursor.zero_()
        for i in range(3):
            gbuf[i].copy_(grads[3 * r + i])
        graph.replay()
        torch.cuda.synchronize()
        last = want[3 * r + 2]
        for name, x, y in zip(("param", "grad", "exp_avg", "exp_avg_sq", "total_norm"), (p, gbuf[2], m, v, norm), last):
            assert _same(x, y), (r, name)
        for i in range(3):
            assert _same(gbuf[i], want[3 * r + i][1]), (r, i)
        assert cursor.tolist() == [3, 0]


# ---------------------------------------------------------------------------------------- mission _rows
@pytest.mark.parametrize("n_rows,seq_len", [(1, 1), (5, 32), (76, 128), (33, 7), (1900, 9)])
def test_mission_rows_equal_forward_index_copy_and_index_select_backward(n_rows, seq_len):
    """Shuffled, non-contiguous rows of a 1,024-row table (2 n_rows rows where that is more: 1,900 x 9 has the chunk
    count capped and empty trailing chunks) pre-filled with a NaN-payload sentinel: the named rows are
    mgx_mission_forward's features, the others still hold the sentinel, the step records are the same; the five
    gradients equal mgx_mission_backward on the index_select-ed cotangent with every unnamed g_table row NaN."""
    _gpu()
    from mgx.fused_mission import FusedMissionEncoder, mission_params
    from mgx.policy import ActorCriticPolicy
    torch.manual_seed(0)
    pol = ActorCriticPolicy(n_stack=1).cuda()
    enc = FusedMissionEncoder(pol, "cuda:0")
    params = tuple(p.detach().contiguous() for p in mission_params(pol))
    g = torch.Generator().manual_seed(100 * n_rows + seq_len)
    tokens = torch.randint(0, 32, (n_rows, seq_len), generator=g).to(torch.uint8).to(enc.device)
    table_rows = max(1024, 2 * n_rows)
    rows = torch.randperm(table_rows, generator=g)[:n_rows].to(enc.device)
    words = int(enc.L.mgx_mission_workspace_words(n_rows, seq_len))
    ws_a = torch.zeros(words, device=enc.device)
    ws_b = torch.zeros(words, device=enc.device)
    sentinel = torch.tensor(SENTINEL, dtype=torch.int32).view(torch.float32).to(enc.device)
    table = sentinel.expand(table_rows, 128).contiguous()
    feat = enc.forward_raw(tokens, params, ws_a)
    assert enc.forward_rows(tokens, params, table, rows, ws_b) is table
    torch.cuda.synchronize()
    assert torch.isfinite(feat).all() and feat.any()
    assert _same(table.index_select(0, rows), feat)
    named = torch.zeros(table_rows, dtype=torch.bool, device=enc.device)
    named[rows] = True
    assert bool((_bits(table)[~named] == SENTINEL).all())
    assert _same(ws_a[:n_rows * seq_len * 640], ws_b[:n_rows * seq_len * 640])
    cot = torch.randn((n_rows, 128), generator=g).to(enc.device)
    g_table = torch.full((table_rows, 128), float("nan"), device=enc.device)
    g_table.index_copy_(0, rows, cot)
    want = enc.backward_raw(tokens, params, g_table.index_select(0, rows), ws_a)
    got = enc.backward_rows(tokens, params, g_table, rows, ws_b)
    torch.cuda.synchronize()
    for name, x, y in zip(("embedding", "w_ih", "w_hh", "b_ih", "b_hh"), got, want):
        assert torch.isfinite(x).all(), name
        assert x.any() or (name == "w_hh" and seq_len == 1), name       # one step: h_0 = 0, so dW_hh = 0 exactly
        assert _same(x, y), name


# ---------------------------------------------------------------------------------------- Trainer.train
PROGRESS = (1.0, 0.6, 0.2)             # a different lr every round: nothing of it may be baked in


def _cfg(k, graph, **kw):
    from mgx.ppo import PPOConfig
    base = dict(n_envs=8, horizon=16, batch_size=48, n_epochs=2, n_frames_stack=k, fused_act=True, fused_train=True,
                fused_mission=True, fused_update=True, graph_train=graph, env=ENV, seed=5)
    base.update(kw)
    return PPOConfig(**base)


def _leg(cfg, policy_seed=0):
    """(collector, trainer) of one leg: its own engine and policy, everything seeded alike across legs."""
    from mgx import MgxEngine
    from mgx.policy import ActorCriticPolicy
    from mgx.ppo import CompactRolloutCollector, Trainer
    torch.manual_seed(policy_seed)
    pol = ActorCriticPolicy(n_stack=cfg.n_frames_stack).cuda()
    eng = MgxEngine(n_envs=cfg.n_envs, n_stack=cfg.n_frames_stack, terminal_mode="truncated",
                    mission_dtype=torch.uint8, reward64=True, seed=cfg.seed, **cfg.env)
    col = CompactRolloutCollector(eng, pol, cfg)
    col.start()
    return col, Trainer(pol, cfg)


def _round(col, tr, progress):
    """One collect + train -> everything the issue compares, cloned."""
    ro = col.collect()
    st = tr.train(ro, progress)
    arena = tr.update.arena
    torch.cuda.synchronize()
    sd = tr.policy.optimizer.state_dict()["state"]
    return dict(params=[p.detach().clone() for p in tr.policy.parameters()], exp_avg=arena.exp_avg.clone(),
                exp_avg_sq=arena.exp_avg_sq.clone(), step=arena.step, stats=st,
                sd_steps=[int(s["step"]) for s in sd.values()], block=ro.buf.block,
                rows=tuple(tr.update.ev._rows.tolist()))


def _assert_round(a, b, tag):
    assert a["step"] == b["step"] and a["sd_steps"] == b["sd_steps"] and len(a["sd_steps"]) == 25, tag
    assert a["stats"] == b["stats"], (tag, a["stats"], b["stats"])
    assert all(math.isfinite(x) for x in a["stats"].values()), tag
    assert a["block"] == b["block"] and a["rows"] == b["rows"], tag
    for i, (x, y) in enumerate(zip(a["params"], b["params"])):
        assert _same(x, y), (tag, "parameter", i)
    assert _same(a["exp_avg"], b["exp_avg"]) and _same(a["exp_avg_sq"], b["exp_avg_sq"]), tag


_EAGER = {}


def _eager_rounds(k, **kw):
    """Three all-eager rounds of (k, kw), run once and shared."""
    key = (k, tuple(sorted(kw.items())))
    if key not in _EAGER:
        col, tr = _leg(_cfg(k, False, **kw))
        _EAGER[key] = [_round(col, tr, p) for p in PROGRESS]
        col.engine.poll_error()
    return _EAGER[key]


VARIANTS = {"k4": (4, {}), "k1": (1, {}), "global": (4, dict(adv_norm="global")),
            "raw_adv": (4, dict(normalize_advantage=False)), "no_vclip": (4, dict(clip_range_vf=0.0))}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_trainer_graph_equals_eager(variant):
    """Two legs on the same seeds, 8 envs x 16 steps, minibatches 48 / 48 / 32, 2 epochs, three collect + train
    rounds at three learning rates: after every round every parameter, both moments, arena.step, the statistics dict
    and optimizer.state_dict()'s steps are equal.  The rounds cross ring blocks (n_stack 4: two blocks)."""
    _gpu()
    k, kw = VARIANTS[variant]
    want = _eager_rounds(k, **kw)
    col, tr = _leg(_cfg(k, True, **kw))
    assert tr.cfg.graph_train and not tr.cfg.graph_collect
    start = [p.detach().clone() for p in tr.policy.parameters()]
    for i, p in enumerate(PROGRESS):
        got = _round(col, tr, p)
        _assert_round(got, want[i], (variant, i))
        assert got["step"] == 6 * (i + 1)
        assert got["stats"]["lr"] == tr.lr_schedule(p)
    assert not any(_same(x, y) for x, y in zip(got["params"], start))
    if k == 4:
        assert {r["block"] for r in want} == {0, 1}
    up = tr.update
    assert 1 <= len(up._graphs) <= 8 and up._gbuf["shape"] == (128, (48, 48, 32), 2)
    assert up._gbuf["cursor"].tolist() == [6, 0]
    col.engine.poll_error()


PIN_SIZES = (48, 32, 1)                # one tile each (see the module docstring); one sample takes adv_mode 0
PIN_LRS = (3e-4, 1.1e-4, 3e-6)


def _sequence_before_the_shared_body(pol, eng, buf, cfg):
    """The eager minibatch step as it stood before FusedUpdate had one body, from the public raw calls:
    forward_raw + index_copy_ into a zeroed table, the policy forward with fresh logits / values, ppo_loss, the policy
    backward, index_select + backward_raw, adam_step by value.  Returns (arena, total_norm, step(index, sel, rollout,
    lr, adv_mode) -> statistics row)."""
    from mgx import _lib
    from mgx.fused_train import FusedEvaluator
    from mgx.fused_update import ParamArena, adam_step, ppo_loss
    L = _lib.load()
    ev = FusedEvaluator(pol, eng, fused_mission=True)
    enc, k = ev.mission, ev.K
    a = ParamArena(pol)
    ev.prepare(buf)
    f32 = dict(dtype=torch.float32, device=eng.device)
    table, g_table = torch.zeros((256 * k, 128), **f32), torch.empty((256, k, 128), **f32)
    norm = torch.zeros(1, **f32)
    loss_scratch = torch.empty(int(L.mgx_ppo_loss_scratch_words(1 << 30)), **f32)
    adam_scratch = torch.empty(int(L.mgx_adam_scratch_words(a.words)), **f32)
    blob, g_blob = a.param[:a.blob_words], a.grad[:a.blob_words]
    mission, g_mission = tuple(a.views(a.param, slice(20, 25))), tuple(a.views(a.grad, slice(20, 25)))
    stacks, rows = ev._stacks, ev._rows
    ws = torch.empty(int(L.mgx_mission_workspace_words(stacks.shape[0], stacks.shape[1])), **f32)
    pg = pol.optimizer.param_groups[0]

    def step(index, sel, rollout, lr, adv_mode):
        stats = torch.zeros(8, **f32)
        table.index_copy_(0, rows, enc.forward_raw(stacks, mission, ws))
        logits, values = ev.forward_raw(buf, index, blob, table)
        g_logits, g_values, _ = ppo_loss(logits, values, *rollout, cfg.clip_range, cfg.clip_range_vf, cfg.ent_coef,
                                         cfg.vf_coef, adv_mode=adv_mode, sel=sel, scratch=loss_scratch,
                                         out=(torch.empty_like(logits), torch.empty_like(values), stats))
        ev.backward_raw(buf, index, blob, table, g_logits, g_values, out=(g_blob, g_table))
        g_feat = g_table.view(-1, 128).index_select(0, rows)
        enc.backward_raw(stacks, mission, g_feat, ws, out=g_mission)
        a.step += 1
        adam_step(a.param, a.grad, a.exp_avg, a.exp_avg_sq, lr, a.step, betas=pg["betas"], eps=pg["eps"],
                  max_grad_norm=cfg.max_grad_norm, grad_scale=1.0, total_norm=norm, scratch=adam_scratch)
        return stats

    return a, norm, step


@pytest.mark.parametrize("k", [4, 1])
def test_step_equals_the_sequence_before_the_shared_body(k):
    """FusedUpdate.step pinned to the arithmetic of the eager step it replaced.  One collected rollout of 8 envs x 16
    steps; two policies of the same weights, each with its own arena; minibatches of 48, 32 and 1 sample of one
    permutation at three learning rates, stepped one after another (twice over: the per-size buffers are reused).
    After every step all 25 parameters, both moments, the gradient arena, total_norm and the statistics row are equal
    bit for bit."""
    _gpu()
    from mgx.fused_update import FusedUpdate
    from mgx.policy import ActorCriticPolicy
    cfg = _cfg(k, False)
    col, tr = _leg(cfg)
    ro = col.collect()
    pol_a = tr.policy
    torch.manual_seed(0)                            # _leg's policy seed
    pol_b = ActorCriticPolicy(n_stack=k).cuda()
    start = [p.detach().clone() for p in pol_a.parameters()]
    assert len(start) == 25 and all(_same(x, y) for x, y in zip(start, pol_b.parameters()))
    up = FusedUpdate(pol_a, col.engine)
    up.prepare(ro.buf)
    ref, ref_norm, ref_step = _sequence_before_the_shared_body(pol_b, col.engine, ro.buf, cfg)
    T, N = ro.T, ro.N
    perm = torch.randperm(T * N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))
    env, t = perm // T, perm % T
    index = ro.buf.index(t, env).to(torch.int64).contiguous()
    sel = (t * N + env).contiguous()
    rollout = (ro.actions, ro.values, ro.log_probs, ro.advantages, ro.returns)
    s = 0
    for i, m in enumerate(PIN_SIZES * 2):
        if i == 3:
            s = 10                                  # the second pass: other samples of the 128
        assert s + m <= T * N
        lr, mode = PIN_LRS[i % 3], 1 if m > 1 else 0
        got = torch.zeros(8, device="cuda")
        up.step(ro.buf, index[s:s + m], sel[s:s + m], rollout, cfg, lr, got, adv_mode=mode)
        want = ref_step(index[s:s + m], sel[s:s + m], rollout, lr, mode)
        torch.cuda.synchronize()
        tag = (k, i, m)
        assert up.arena.step == ref.step == i + 1, tag
        assert _same(got, want) and bool(torch.isfinite(got[:6]).all()), (tag, got.tolist(), want.tolist())
        for j, (x, y) in enumerate(zip(pol_a.parameters(), pol_b.parameters())):
            assert _same(x, y), (tag, "parameter", j)
        for name in ("param", "grad", "exp_avg", "exp_avg_sq"):
            assert _same(getattr(up.arena, name), getattr(ref, name)), (tag, name)
        assert _same(up.total_norm, ref_norm) and float(ref_norm) > 0, tag
        s += m
    assert not any(_same(x, y) for x, y in zip(pol_a.parameters(), start))
    col.engine.poll_error()


def test_hand_back_to_eager():
    """Two graph rounds, then one round with graph_train off on the same trainer (its generator goes on): equal to
    three all-eager rounds."""
    _gpu()
    want = _eager_rounds(4)
    col, tr = _leg(_cfg(4, True))
    for i in range(2):
        _assert_round(_round(col, tr, PROGRESS[i]), want[i], ("graph", i))
    tr.cfg = dataclasses.replace(tr.cfg, graph_train=False)
    _assert_round(_round(col, tr, PROGRESS[2]), want[2], "handed back")
    col.engine.poll_error()


@pytest.mark.parametrize("cap", [8, 1])
def test_mission_id_set_change_recaptures(cap, monkeypatch):
    """Rollouts of 2 envs x 4 steps until two different mission-id sets have occurred (at most 20): the graph of one
    set is not replayed for another -- equality with eager holds on both sides of the change.  cap 1: the cache holds
    one graph, so the change evicts and captures again, which is not an error."""
    _gpu()
    from mgx import fused_update
    monkeypatch.setattr(fused_update, "MAX_GRAPHS", cap)
    kw = dict(n_envs=2, horizon=4, batch_size=8, n_frames_stack=4)
    ce, te = _leg(_cfg(4, False, **kw))
    cg, tg = _leg(_cfg(4, True, **kw))
    seen, after = [], 0
    for i in range(20):
        p = 1.0 - 0.04 * i
        a, b = _round(ce, te, p), _round(cg, tg, p)
        _assert_round(b, a, i)
        if b["rows"] not in seen:
            seen.append(b["rows"])
        after += len(seen) >= 2
        if after >= 2:                              # one more round on the far side of the change
            break
    if len(seen) < 2:
        pytest.skip("the mission-id set never changed in 20 rollouts of 2 envs x 4 steps")
    assert len(tg.update._graphs) == min(cap, len(seen))
    cg.engine.poll_error()


def test_learn_with_graph_train_equals_learn_without():
    """learn() for 3 iterations of 8 envs x 16 steps with all six flags on against the same with graph_train off: the
    histories and the final state_dict are equal."""
    _gpu()
    from mgx.ppo import PPOConfig, learn
    cfg = PPOConfig(n_envs=8, horizon=16, batch_size=48, n_epochs=2, fused_act=True, fused_train=True,
                    fused_mission=True, fused_update=True, graph_collect=True, graph_train=True, env=ENV)
    pol_g, hist_g, eng_g = learn(cfg, 3 * 8 * 16)
    pol_e, hist_e, eng_e = learn(dataclasses.replace(cfg, graph_train=False), 3 * 8 * 16)
    assert len(hist_g) == len(hist_e) == 3
    for hg, he in zip(hist_g, hist_e):
        assert hg.keys() == he.keys()
        for key in hg:
            assert hg[key] == he[key] or (math.isnan(hg[key]) and math.isnan(he[key])), (key, hg[key], he[key])
    sg, se = pol_g.state_dict(), pol_e.state_dict()
    assert sg.keys() == se.keys() and len(sg) >= 25
    for name in sg:
        assert _same(sg[name], se[name]) if sg[name].dtype == torch.float32 else torch.equal(sg[name], se[name]), name
    og, oe = pol_g.optimizer.state_dict()["state"], pol_e.optimizer.state_dict()["state"]
    for i in og:
        assert int(og[i]["step"]) == int(oe[i]["step"]) == 18
        assert _same(og[i]["exp_avg"], oe[i]["exp_avg"]) and _same(og[i]["exp_avg_sq"], oe[i]["exp_avg_sq"]), i
    eng_g.poll_error()
    eng_e.poll_error()
