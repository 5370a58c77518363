"""Fused mission encoder on the GPU (mgx_mission_forward / mgx_mission_backward, mgx/fused_mission.py) against torch.

Reference: the fp64 CPU deep copy of the policy's Embedding + GRU, differentiated by autograd.  Yardstick (the one of
tests/test_fused_train_gpu.py), per tensor and measured in the same run: e_torch = max |torch fp32 GPU module - fp64|;
the kernels may deviate from fp64 by at most max(4 e_torch, 4 eps32 max|ref|).  Every check prints its ratios.

The Embedding and GRU parameters are redrawn (weights N(0, 1) / sqrt(fan-in), biases N(0, 0.5^2): no bias is zero).
Shapes: seq_len 32, 128 and 256 (n_stack 1, 4, 8) at n_rows 1 and one below, at and one above the kernel's tile of
3 rows per workgroup, and seq_len 32 at 256 rows (86 workgroups, the last one with a single live row).  Token sets:
real (mission id, v) stacks, uniform random tokens covering all 32 values, all zeros; from two rows on the three are
mixed in one input as well.

Those shapes leave paths of the weight-gradient kernels unrun (their chunks are 32, 48 or 64 pairs long and at most
152).  mission_ref.PLAN_SHAPES adds the shapes that run them -- seq_len 1, odd and unaligned seq_len, the tail loop of
mgx_mission_wgrad_kernel with 1, 2 and 3 steps, a half-filled last step, the chunk count capped at 256 with chunks
longer than 64 pairs and empty trailing chunks, 2,048 rows -- each named with its path there and checked against its
derived plan by tests/test_fused_mission_cpu.py.  Same reference, same yardstick; tokens random / zero / alternating
rows (mission_ref.plan_tokens: real stacks need seq_len to be a multiple of 32)."""
import copy
import math

import pytest

torch = pytest.importorskip("torch")

import mission_ref as R  # noqa: E402
from mgx.policy import ActorCriticPolicy  # noqa: E402

pytestmark = pytest.mark.gpu

EPS32 = float(torch.finfo(torch.float32).eps)
TILE = 3                                   # MS_ROWS (csrc/mgx_mission.h)
NAMES = ("embedding", "w_ih", "w_hh", "b_ih", "b_hh")
SHAPES = [(s, n) for s in (32, 128, 256) for n in (1, TILE - 1, TILE, TILE + 1)] + [(32, 256)]
KINDS = ("real", "random", "zero", "mixed")


class Ctx:
    pass


_CTX = {}


def _ctx():
    """One policy with redrawn mission parameters, its fp64 CPU copy and the encoder."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if _CTX:
        return _CTX["c"]
    from mgx.fused_mission import FusedMissionEncoder, mission_params
    c = Ctx()
    c.pol = R.redrawn_policy().cuda()
    c.pol.train(True)                      # MIOpen's RNN backward needs training mode
    c.seq32 = c.pol.features_extractor.extractors["mission"]
    c.seq64 = copy.deepcopy(c.seq32).cpu().double()
    c.enc = FusedMissionEncoder(c.pol, "cuda:0")
    c.params = mission_params(c.pol)
    _CTX["c"] = c
    return c


def _tokens(kind, n_rows, seq, seed=0):
    """u8 [n_rows, seq] (CPU)."""
    from mgx.fused_policy import mission_token_stacks
    g = torch.Generator().manual_seed(1000 * seq + 10 * n_rows + seed)
    k = seq // 32
    real = mission_token_stacks(k).reshape(256 * k, seq)
    real = real[real.any(1)]                                           # rows of missions that exist
    real = real[torch.randint(0, real.shape[0], (n_rows,), generator=g)]
    rnd = torch.randint(0, 32, (n_rows, seq), generator=g)
    rnd[0, :32] = torch.randperm(32, generator=g)                      # every value occurs
    zero = torch.zeros((n_rows, seq), dtype=torch.int64)
    if kind == "mixed":
        out = torch.stack([(real, rnd, zero)[i % 3][i] for i in range(n_rows)])
        if n_rows < 3:
            out[0, :32] = rnd[0, :32]
    else:
        out = dict(real=real, random=rnd, zero=zero)[kind]
    assert out.shape == (n_rows, seq)
    return out.to(torch.uint8)


def _module(seq, tokens, g):
    """(features, {name: grad}) of an Embedding + GRU Sequential on i64 tokens, cotangent g; f64 on the CPU."""
    _, h = seq(tokens)
    feat = h[-1]
    grads = torch.autograd.grad((feat * g.to(feat)).sum(), list(seq.parameters()))
    assert [tuple(x.shape) for x in grads] == [(32, 32), (384, 32), (384, 128), (384,), (384,)]
    return feat.detach().double().cpu(), {n: x.double().cpu() for n, x in zip(NAMES, grads)}


def _kernel(c, tokens, g, ws=None, params=None):
    """(features, {name: grad}) through forward_raw / backward_raw; raw f32 GPU tensors."""
    params = tuple(p.detach().contiguous() for p in (params or c.params))
    tok = tokens.cuda().contiguous()
    n, seq = tok.shape
    if ws is None:
        ws = torch.empty(int(c.enc.L.mgx_mission_workspace_words(n, seq)), dtype=torch.float32, device="cuda:0")
    feat = c.enc.forward_raw(tok, params, ws)
    grads = c.enc.backward_raw(tok, params, g.cuda(), ws)
    torch.cuda.synchronize()
    return feat, dict(zip(NAMES, grads))


def _bound_check(tag, got, ref, t32, need_signal=True):
    """Every tensor of got within max(4 e_torch, 4 eps32 max|ref|) of ref; prints the ratios.  -> {name: bound}"""
    bad, bounds = [], {}
    for n in ref:
        e_torch = float((t32[n] - ref[n]).abs().max())
        scale = float(ref[n].abs().max())
        bound = max(4.0 * e_torch, 4.0 * EPS32 * scale)
        dev = float((got[n].double().cpu() - ref[n]).abs().max())
        print("%s %s: kernel max |dev| %.3e, torch fp32 %.3e, bound %.3e, ratio %.2f"
              % (tag, n, dev, e_torch, bound, dev / bound if bound else float("inf")))
        if need_signal:
            assert scale > 0, n
        bounds[n] = bound
        if not dev <= bound:
            bad.append((n, dev, bound))
    assert not bad, bad
    return bounds


_CASES = {}


def _case(seq, n_rows, kind):
    """Everything the parity tests compare for one input, computed once."""
    key = (seq, n_rows, kind)
    if key in _CASES:
        return _CASES[key]
    c = _ctx()
    tok = _tokens(kind, n_rows, seq)
    g = torch.randn((n_rows, 128), generator=torch.Generator().manual_seed(seq + n_rows))
    r = Ctx()
    r.tok, r.g = tok, g
    r.ref = _module(c.seq64, tok.long(), g)
    r.t32 = _module(c.seq32, tok.long().cuda(), g.cuda())
    for p in c.seq32.parameters():
        p.grad = None
    r.got = _kernel(c, tok, g)
    _CASES[key] = r
    return r


def _kinds(n_rows):
    return KINDS if n_rows > 1 else KINDS[:3]


PARITY = [(s, n, kind) for s, n in SHAPES for kind in _kinds(n)]


@pytest.mark.parametrize("seq,n_rows,kind", PARITY)
def test_forward_parity(seq, n_rows, kind):
    r = _case(seq, n_rows, kind)
    assert r.got[0].shape == (n_rows, 128) and torch.isfinite(r.got[0]).all()
    _bound_check("seq %d rows %d %s" % (seq, n_rows, kind), {"features": r.got[0]}, {"features": r.ref[0]},
                 {"features": r.t32[0]})


@pytest.mark.parametrize("seq,n_rows,kind", PARITY)
def test_gradient_parity(seq, n_rows, kind):
    """All five gradients, N(0, 1) cotangent of the features."""
    r = _case(seq, n_rows, kind)
    _bound_check("seq %d rows %d %s" % (seq, n_rows, kind), r.got[1], r.ref[1], r.t32[1])


def _plan_case(n_rows, seq, kind):
    """_case for a mission_ref.PLAN_SHAPES entry: mission_ref's tokens and cotangent."""
    key = ("plan", seq, n_rows, kind)
    if key in _CASES:
        return _CASES[key]
    c = _ctx()
    r = Ctx()
    r.tok, r.g = R.plan_tokens(kind, n_rows, seq), R.plan_cotangent(n_rows, seq)
    r.ref = _module(c.seq64, r.tok.long(), r.g)
    r.t32 = _module(c.seq32, r.tok.long().cuda(), r.g.cuda())
    for p in c.seq32.parameters():
        p.grad = None
    r.got = _kernel(c, r.tok, r.g)
    _CASES[key] = r
    return r


def _plan_gradient_check(n_rows, seq, kind):
    """All five gradients of a plan case within the bound -> {name: bound}.  At seq_len 1 h_0 = 0 makes dW_hh zero:
    exactly zero from the kernels, and the other four must carry signal."""
    r = _plan_case(n_rows, seq, kind)
    got, ref, t32 = (dict(d) for d in (r.got[1], r.ref[1], r.t32[1]))
    if seq == 1:
        assert not got.pop("w_hh").any() and not ref.pop("w_hh").any()
        del t32["w_hh"]
    return _bound_check("plan rows %d seq %d %s" % (n_rows, seq, kind), got, ref, t32)


PLAN_PARITY = [(n, s, kind) for n, s in R.PLAN_SHAPES for kind in R.plan_kinds(n, s)]


@pytest.mark.parametrize("n_rows,seq,kind", PLAN_PARITY)
def test_forward_parity_plan_shapes(n_rows, seq, kind):
    r = _plan_case(n_rows, seq, kind)
    assert r.got[0].shape == (n_rows, 128) and torch.isfinite(r.got[0]).all()
    _bound_check("plan rows %d seq %d %s" % (n_rows, seq, kind), {"features": r.got[0]}, {"features": r.ref[0]},
                 {"features": r.t32[0]})


@pytest.mark.parametrize("n_rows,seq,kind", PLAN_PARITY)
def test_gradient_parity_plan_shapes(n_rows, seq, kind):
    """All five gradients, N(0, 1) cotangent of the features, at the shapes that run the weight-gradient kernels'
    tail loop, half-filled step, capped and empty chunks (mission_ref.PLAN_SHAPES names each shape's path)."""
    _plan_gradient_check(n_rows, seq, kind)


@pytest.mark.parametrize("n_rows,seq", R.PAIR_SHAPES)
def test_single_pair_would_be_seen(n_rows, seq):
    """A condition on the inputs that makes the parity test above a test of every (row, t) pair: by the explicit
    fp64 GRU (mission_ref.gru_reference), each pair's own contribution to db_ih -- its (da_r, da_z, da_n) -- and, for
    t > 0, to dW_hh -- its hidden-side cotangent (x) h_{t-1} -- has an entry above twice the bound the parity check
    applies to that tensor in this run.  A pair dropped or taken twice at a chunk boundary, in the half-filled step
    or in the tail loop then puts the gradient out of tolerance.  Random tokens; short seq_len only: over 64 steps
    the cotangent decays too far ((9, 65) reaches 5.5 times the floor on the CPU), and the long shapes are left to
    the parity test."""
    c = _ctx()
    bounds = _plan_gradient_check(n_rows, seq, "random")
    r = _plan_case(n_rows, seq, "random")
    ref = R.gru_reference(list(c.seq64.parameters()), r.tok, r.g)
    for name, (small, floor) in R.pair_floor_ratios(ref).items():
        print("plan rows %d seq %d %s: smallest pair contribution %.3e, bound %.3e (floor %.3e), factor %.1f"
              % (n_rows, seq, name, small, bounds[name], floor, small / bounds[name]))
        assert bounds[name] >= floor * (1.0 - 1e-12)
        assert small > 2.0 * bounds[name], (name, small, bounds[name])


@pytest.mark.parametrize("seq,n_rows", [(32, 1), (128, TILE + 1)])
def test_unused_tokens_have_exactly_zero_embedding_gradient(seq, n_rows):
    """An input of tokens 0, 1 and 2 only: rows 3..31 of the Embedding gradient are exactly zero, rows 0..2 are
    not, and all five gradients are within the bound."""
    c = _ctx()
    gen = torch.Generator().manual_seed(3)
    tok = torch.randint(0, 3, (n_rows, seq), generator=gen)
    tok[0, :3] = torch.arange(3)
    tok = tok.to(torch.uint8)
    g = torch.randn((n_rows, 128), generator=gen)
    _, ref = _module(c.seq64, tok.long(), g)
    _, t32 = _module(c.seq32, tok.long().cuda(), g.cuda())
    _, got = _kernel(c, tok, g)
    de = got["embedding"].cpu()
    assert not de[3:].any() and all(bool(de[i].any()) for i in range(3))
    _bound_check("tokens 0..2 seq %d rows %d" % (seq, n_rows), got, ref, t32)


def test_token_values_are_masked():
    """Token bytes above 31 index as their low five bits: no input reaches outside the tables."""
    c = _ctx()
    tok = _tokens("random", TILE + 1, 32)
    g = torch.randn((TILE + 1, 128), generator=torch.Generator().manual_seed(4))
    f0, g0 = _kernel(c, tok, g)
    f1, g1 = _kernel(c, tok | 0xE0, g)
    assert torch.equal(f0, f1) and all(torch.equal(g0[n], g1[n]) for n in NAMES)


@pytest.mark.parametrize("seq,n_rows", [(128, 76), (32, TILE + 1), (9, 1900), (256, 65)])
def test_reproducible_and_workspace_independent(seq, n_rows):
    """Two runs are bitwise equal in the features and all five gradients; a workspace prefilled with NaN gives the
    same bits (it need not be zeroed); the forward with and without a workspace gives the same features.  At 1,900
    x 9 and 65 x 256 the last 4 and 3 of the 256 chunks are empty: their slabs must come out as exact zeros, and no
    masked-out operand may leak a NaN through 0 * NaN."""
    c = _ctx()
    assert (R.chunk_plan(n_rows, seq)[4] > 0) == (n_rows * seq > 16384)
    tok = _tokens("mixed", n_rows, seq, seed=1) if seq % 32 == 0 else R.plan_tokens("mixed", n_rows, seq, seed=1)
    g = torch.randn((n_rows, 128), generator=torch.Generator().manual_seed(5))
    f0, g0 = _kernel(c, tok, g)
    f1, g1 = _kernel(c, tok, g)
    words = int(c.enc.L.mgx_mission_workspace_words(n_rows, seq))
    f2, g2 = _kernel(c, tok, g, ws=torch.full((words,), float("nan"), device="cuda:0"))
    f3 = c.enc.forward_raw(tok.cuda(), tuple(p.detach().contiguous() for p in c.params), None)
    assert torch.isfinite(f0).all() and bool(f0.any())
    assert torch.equal(f0, f1) and torch.equal(f0, f2) and torch.equal(f0, f3)
    for n in NAMES:
        assert torch.isfinite(g0[n]).all() and bool(g0[n].any()), n
        assert torch.equal(g0[n], g1[n]) and torch.equal(g0[n], g2[n]), n


def test_saturated_gates_stay_finite():
    """Every parameter scaled by 400: gate pre-activations beyond +-100 (asserted from the fp64 module's own
    arithmetic).  Features and gradients are finite, the features lie in [-1, 1]."""
    c = _ctx()
    params = tuple(400.0 * p.detach() for p in c.params)
    e, w_ih, w_hh, b_ih, b_hh = (p.double().cpu() for p in params)
    pre = e @ w_ih.T + b_ih                                            # the input side alone, per token
    assert float(pre.abs().max()) > 100.0 and float(pre.max()) > 100.0 and float(pre.min()) < -100.0
    tok = _tokens("mixed", TILE + 1, 128, seed=2)
    g = torch.randn((TILE + 1, 128), generator=torch.Generator().manual_seed(6))
    feat, grads = _kernel(c, tok, g, params=params)
    assert torch.isfinite(feat).all() and float(feat.abs().max()) <= 1.0
    for n in NAMES:
        assert torch.isfinite(grads[n]).all(), n


def test_encode_autograd_fills_the_five_gradients():
    """encode() under autograd: .grad of the five parameters equals backward_raw's gradients bit for bit, and a
    second backward through the same graph raises instead of reading clobbered records."""
    c = _ctx()
    tok = _tokens("mixed", 7, 64).cuda()
    g = torch.randn((7, 128), generator=torch.Generator().manual_seed(8)).cuda()
    _, want = _kernel(c, tok.cpu(), g.cpu())
    for p in c.params:
        p.grad = None
    feat = c.enc.encode(tok)
    assert feat.requires_grad
    (feat * g).sum().backward(retain_graph=True)
    for n, p in zip(NAMES, c.params):
        assert torch.equal(p.grad, want[n]), n
        p.grad = None
    with pytest.raises(RuntimeError):
        (feat * g).sum().backward()
    with torch.no_grad():
        assert torch.equal(c.enc.encode(tok), feat.detach())


def test_evaluator_ppo_loss_with_fused_mission():
    """test_fused_train_gpu.test_evaluate_actions_ppo_loss at n_stack 4 (gtg 6x6, 70 envs, 210 samples) with
    FusedEvaluator(fused_mission=True): p.grad of all 25 parameter tensors within the bound."""
    import test_fused_train_gpu as T
    from mgx.fused_train import FusedEvaluator
    from mgx.ppo import PPOConfig
    r = T._run(4)
    ev = FusedEvaluator(r.pol, r.eng, max_groups=2, fused_mission=True)
    ev.prepare(r.buf)
    assert ev._stacks.dtype == torch.uint8
    cfg = PPOConfig()
    n = r.index.numel()
    gen = torch.Generator().manual_seed(23)
    actions = torch.randint(0, 7, (n,), generator=gen)
    with torch.no_grad():
        lg64, v64 = T._out64(r.pol64, r.obs)
    lp64 = torch.log_softmax(lg64, 1).gather(1, actions[:, None])[:, 0]
    old_v = (v64 + 0.05 * torch.randn(n, generator=gen).double()).float()
    old_lp = (lp64 + 0.1 * torch.randn(n, generator=gen).double()).float()
    adv = torch.randn(n, generator=gen)
    ret = (v64 + 0.3 * torch.randn(n, generator=gen).double()).float()
    loss = T._ppo_loss(cfg, actions, old_v, old_lp, adv, ret)
    ref = T._module_grads(r.pol64, T._via(T._out64, actions), r.obs, loss)
    t32 = T._module_grads(r.pol, T._via(T._out32, actions), r.obs, loss)
    for p in r.pol.parameters():
        p.grad = None
    values, log_prob, entropy = ev.evaluate_actions(r.buf, r.index, actions.cuda())
    with torch.no_grad():
        assert float((values.double().cpu() - v64).abs().max()) < 1e-4
    loss(values, log_prob, entropy).backward()
    got = {nm: p.grad.double().cpu() for nm, p in r.pol.named_parameters()}
    for p in r.pol.parameters():
        p.grad = None
    T._check("fused_mission ppo", got, ref, t32)
    r.eng.poll_error()


def test_actor_table_with_fused_mission():
    """FusedActor(fused_mission=True).mission_feat at n_stack 2 (512 rows of 64 tokens, no workspace) against the
    fp64 module on every (mission id, v) stack; e_torch is fused_policy.mission_table(policy)."""
    from mgx import MgxEngine
    from mgx.fused_policy import FusedActor, mission_table, mission_token_stacks
    c = _ctx()
    pol = ActorCriticPolicy(n_stack=2).cuda()
    pol.features_extractor.extractors["mission"].load_state_dict(c.seq32.state_dict())
    eng = MgxEngine(n_envs=8, n_stack=2, terminal_mode="truncated", mission_dtype=torch.uint8, problem="gtg",
                    mission=5, size=6, num_objects=2)
    actor = FusedActor(pol, eng, fused_mission=True)
    assert actor.mission is not None and actor.mission_feat.shape == (256, 2, 128)
    with torch.no_grad():
        _, h = c.seq64(mission_token_stacks(2).reshape(512, 64))
        t32 = mission_table(pol)
    ref = h[-1].reshape(256, 2, 128)
    _bound_check("actor table", {"mission_feat": actor.mission_feat}, {"mission_feat": ref},
                 {"mission_feat": t32.double().cpu()})
    eng.poll_error()


def test_learn_smoke_with_fused_mission():
    """learn() with fused_act, fused_train and fused_mission on gtg 6x6 for one iteration: every history entry is
    finite, every parameter has moved, poll_error() is clean."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgx.ppo import PPOConfig, learn
    cfg = PPOConfig(n_envs=70, horizon=4, batch_size=64, n_epochs=2, fused_act=True, fused_train=True,
                    fused_mission=True, env=dict(problem="gtg", mission=5, size=6, num_objects=2))
    before = {}

    class Cb:
        def on_step(self, policy, num_timesteps):
            if not before:
                before.update({n: p.detach().clone() for n, p in policy.named_parameters()})
            return True

    pol, hist, eng = learn(cfg, 70 * 4, callback=Cb())
    assert len(hist) == 1
    for key in ("pg", "vf", "ent", "kl", "clipfrac", "lr", "adv_mean", "adv_std"):
        assert math.isfinite(hist[0][key]), (key, hist[0])
    for n, p in pol.named_parameters():
        assert torch.isfinite(p).all(), n
        assert not torch.equal(p.detach(), before[n]), n
    eng.poll_error()
