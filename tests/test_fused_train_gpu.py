"""Fused policy gradient on the GPU (mgx_policy_backward, mgx/fused_train.py) against torch autograd.

Reference: the fp64 CPU deep copy of the module on buf.gather of the same indices, differentiated by autograd.
Yardstick, per parameter tensor and measured in the same run: e_torch = max |torch fp32 GPU autograd - fp64|; the
kernel path may deviate from fp64 by at most max(4 e_torch, 4 eps32 max|ref|) -- the project's margin for fp32 sums
taken in another order, which is what these are.

Setup (as tests/test_fused_policy_gpu.py): gtg 6x6, 70 envs, a ring CompactBuffer of T = 3, 40 random-action steps
over carried-over rollouts, so episode starts fall inside stack windows and the walk-back wraps the ring.  Every
blob parameter is redrawn (weights N(0, 1) / sqrt(fan-in), biases N(0, 0.5^2): no bias is zero; action_net N(0, 1) as
in that file).  Samples: all 210 (t, env) pairs of the current block's three rows = three full tiles and an 18-lane
tail."""
import copy
import ctypes
import math

import pytest

torch = pytest.importorskip("torch")

from mgx.policy import ActorCriticPolicy  # noqa: E402

pytestmark = pytest.mark.gpu

N_ENVS, T_RING, STEPS = 70, 3, 40
ENV = dict(problem="gtg", mission=5, size=6, num_objects=2)
EPS32 = float(torch.finfo(torch.float32).eps)


def _policy(k, seed=0):
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
        pol.action_net.weight.copy_(torch.randn(pol.action_net.weight.shape, generator=g))
        pol.action_net.bias.copy_(torch.randn(pol.action_net.bias.shape, generator=g))
    pol.train(True)                    # MIOpen's RNN backward needs training mode (no layer behaves differently)
    return pol


def _out64(pol64, obs):
    o = {"image": obs["image"].cpu().double() / 255.0, "direction": obs["direction"].cpu().double(),
         "mission": obs["mission"].cpu()}
    f = pol64.features_extractor(o)
    return pol64.action_net(pol64.policy_net(f)), pol64.value_net(pol64.value_net_body(f)).flatten()


def _out32(pol, obs):
    pi, vf = pol._latent(obs)
    return pol.action_net(pi), pol.value_net(vf).flatten()


def _linear_loss(gl, gv):
    return lambda logits, values: (logits * gl.to(logits)).sum() + (values * gv.to(values)).sum()


def _module_grads(pol, outs, obs, loss):
    """{name: grad (f64, CPU)} of loss(logits, values) by autograd through the module."""
    names, ps = zip(*pol.named_parameters())
    gs = torch.autograd.grad(loss(*outs(pol, obs)), ps)
    return {n: g.detach().double().cpu() for n, g in zip(names, gs)}


class Run:
    pass


_RUNS = {}


def _run(k):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if k in _RUNS:
        return _RUNS[k]
    from mgx import MgxEngine
    from mgx.compact import CompactBuffer
    from mgx.fused_train import FusedEvaluator
    r = Run()
    r.k = k
    r.pol = _policy(k).cuda()
    r.pol64 = copy.deepcopy(r.pol).cpu().double()
    r.eng = MgxEngine(n_envs=N_ENVS, n_stack=k, terminal_mode="truncated", mission_dtype=torch.uint8, **ENV)
    r.buf = CompactBuffer(r.eng, T_RING, ring=True)
    r.eng.reset()
    r.buf.observe(0)
    g = torch.Generator().manual_seed(5)
    t, ends = 0, 0
    for _ in range(STEPS):
        r.buf.step(t, torch.randint(0, 7, (N_ENVS,), generator=g).cuda())
        ends += int(r.buf.dones[t].sum())
        t += 1
        if t == T_RING:
            r.buf.carry_over()
            t = 0
    assert ends > N_ENVS
    dev = r.eng.device
    tt = torch.arange(T_RING, device=dev).repeat_interleave(N_ENVS)
    ee = torch.arange(N_ENVS, device=dev).repeat(T_RING)
    r.index = r.buf.index(tt, ee).to(torch.int64).contiguous()        # 210 samples
    r.obs = {kk: v.clone() for kk, v in r.buf.gather(r.index, f32=False).items()}
    r.v = (r.obs["direction"].reshape(-1, k, 4).sum(2) > 0).sum(1).cpu()      # valid slots per sample
    r.mid = r.buf.mids.reshape(-1)[r.index].cpu().long()
    if k > 1:
        assert int((r.v < k).sum()) > 0                               # stacks with empty slots
    r.ev = FusedEvaluator(r.pol, r.eng, max_groups=2)
    r.ev.prepare(r.buf)
    gen = torch.Generator().manual_seed(17)
    r.gl = torch.randn((r.index.numel(), 7), generator=gen)
    r.gv = torch.randn(r.index.numel(), generator=gen)
    r.eng.poll_error()
    _RUNS[k] = r
    return r


def _kernel_grads(r, ev, index, gl, gv, scratch=None):
    """{name: grad (f64, CPU)} from mgx_policy_backward: the blob tensors sliced out of grad_blob, the Embedding and
    GRU gradients by autograd through the differentiable table; also the raw (grad_blob, grad_mission_feat)."""
    from mgx.fused_policy import _params, blob_offsets
    with torch.no_grad():
        blob, table = ev.inputs()
    gb, gm = ev.backward_raw(r.buf, index, blob.contiguous(), table.contiguous(), gl.cuda(), gv.cuda(), scratch=scratch)
    torch.cuda.synchronize()
    names = {id(p): n for n, p in r.pol.named_parameters()}
    _, tensors = _params(r.pol)
    out = {}
    for t, (o, shape) in zip(tensors, blob_offsets(r.k).values()):
        out[names[id(t)]] = gb[o:o + t.numel()].reshape(shape).double().cpu()
    mission = [(n, p) for n, p in r.pol.named_parameters() if ".mission." in n]
    assert len(mission) == 5 and len(out) == 20
    _, tab = ev.inputs()
    for (n, _), g in zip(mission, torch.autograd.grad(tab, [p for _, p in mission], grad_outputs=gm)):
        out[n] = g.double().cpu()
    return out, gb, gm


def _check(tag, got, ref, t32):
    """Every tensor within max(4 e_torch, 4 eps32 max|ref|) of the fp64 reference; prints the ratios."""
    assert set(got) == set(ref) == set(t32) and len(ref) == 25
    bad = []
    for n in ref:
        e_torch = float((t32[n] - ref[n]).abs().max())
        bound = max(4.0 * e_torch, 4.0 * EPS32 * float(ref[n].abs().max()))
        dev = float((got[n] - ref[n]).abs().max())
        print("%s %s: kernel max |dev| %.3e, torch fp32 %.3e, bound %.3e, ratio %.2f"
              % (tag, n, dev, e_torch, bound, dev / bound if bound else float("inf")))
        assert float(ref[n].abs().max()) > 0, n
        if not dev <= bound:
            bad.append((n, dev, bound))
    assert not bad, bad


def _refs(r, sel, loss):
    obs = {kk: v[sel] for kk, v in r.obs.items()}
    return _module_grads(r.pol64, _out64, obs, loss), _module_grads(r.pol, _out32, obs, loss)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7, 8])
def test_gradient_parity(k):
    """grad_blob's 20 tensors and the Embedding / GRU gradients through grad_mission_feat, N(0, 1) cotangents,
    max_groups = 2: each group walks two tiles, the 18-lane tail among them, and the fold adds two slabs."""
    r = _run(k)
    sel = slice(None)
    ref, t32 = _refs(r, sel, _linear_loss(r.gl, r.gv))
    got, _, _ = _kernel_grads(r, r.ev, r.index, r.gl, r.gv)
    _check("n_stack %d" % k, got, ref, t32)
    r.eng.poll_error()


def _ppo_loss(cfg, actions, old_v, old_lp, adv, ret):
    """Trainer.train's loss from (values, log_prob, entropy)."""
    def loss(values, log_prob, entropy):
        c = lambda x: x.to(values)  # noqa: E731
        a = (c(adv) - c(adv).mean()) / (c(adv).std() + 1e-8)
        ratio = torch.exp(log_prob - c(old_lp))
        policy_loss = -torch.min(a * ratio, a * torch.clamp(ratio, 1 - cfg.clip_range, 1 + cfg.clip_range)).mean()
        vp = c(old_v) + torch.clamp(values - c(old_v), -cfg.clip_range_vf, cfg.clip_range_vf)
        value_loss = torch.nn.functional.mse_loss(c(ret), vp)
        return policy_loss + cfg.ent_coef * -torch.mean(entropy) + cfg.vf_coef * value_loss
    return loss


@pytest.mark.parametrize("k", [1, 4, 8])
def test_evaluate_actions_ppo_loss(k):
    """p.grad of every parameter after loss.backward() through FusedEvaluator.evaluate_actions with Trainer.train's
    loss (clip 0.1, clip_range_vf, entropy and value coefficients of PPOConfig; random old values, log-probs and
    advantages) against the fp64 module's evaluate_actions: the log_prob / entropy cotangents and the autograd wiring."""
    from mgx.ppo import PPOConfig
    r = _run(k)
    cfg = PPOConfig()
    n = r.index.numel()
    gen = torch.Generator().manual_seed(23)
    actions = torch.randint(0, 7, (n,), generator=gen)
    with torch.no_grad():
        lg64, v64 = _out64(r.pol64, r.obs)
    lp64 = torch.log_softmax(lg64, 1).gather(1, actions[:, None])[:, 0]
    old_v = (v64 + 0.05 * torch.randn(n, generator=gen).double()).float()
    old_lp = (lp64 + 0.1 * torch.randn(n, generator=gen).double()).float()
    adv = torch.randn(n, generator=gen)
    ret = (v64 + 0.3 * torch.randn(n, generator=gen).double()).float()
    loss = _ppo_loss(cfg, actions, old_v, old_lp, adv, ret)

    def via(outs):
        def f(pol, obs):
            logits, values = outs(pol, obs)
            dist = torch.distributions.Categorical(logits=logits)
            return values, dist.log_prob(actions.to(logits.device)), dist.entropy()
        return f

    ref = _module_grads(r.pol64, via(_out64), r.obs, loss)
    t32 = _module_grads(r.pol, via(_out32), r.obs, loss)
    for p in r.pol.parameters():
        p.grad = None
    values, log_prob, entropy = r.ev.evaluate_actions(r.buf, r.index, actions.cuda())
    with torch.no_grad():
        assert float((values.double().cpu() - v64).abs().max()) < 1e-4
    loss(values, log_prob, entropy).backward()
    got = {nm: p.grad.double().cpu() for nm, p in r.pol.named_parameters()}
    for p in r.pol.parameters():
        p.grad = None
    _check("n_stack %d ppo" % k, got, ref, t32)
    r.eng.poll_error()


def test_reproducible_and_partition_independent():
    """n_stack 4: two identical calls give a bit-equal grad_blob; the default group count (one group per tile here)
    and a permutation of the samples (cotangents permuted alike) agree with the reference within test 1's bound."""
    from mgx.fused_train import FusedEvaluator
    r = _run(4)
    ref, t32 = _refs(r, slice(None), _linear_loss(r.gl, r.gv))
    _, gb0, _ = _kernel_grads(r, r.ev, r.index, r.gl, r.gv)
    _, gb1, _ = _kernel_grads(r, r.ev, r.index, r.gl, r.gv)
    assert torch.equal(gb0, gb1)
    ev0 = FusedEvaluator(r.pol, r.eng, max_groups=0)
    ev0.prepare(r.buf)
    got, _, _ = _kernel_grads(r, ev0, r.index, r.gl, r.gv)
    _check("default groups", got, ref, t32)
    perm = torch.randperm(r.index.numel(), generator=torch.Generator().manual_seed(3))
    got, _, _ = _kernel_grads(r, r.ev, r.index[perm.cuda()].contiguous(), r.gl[perm], r.gv[perm])
    _check("permuted", got, ref, t32)
    r.eng.poll_error()


@pytest.mark.parametrize("n", [1, 65])
def test_spare_lanes(n):
    """n_samples 1 (a tile with 63 empty lanes) and 65 (a full tile and a 1-lane tile) against the reference;
    grad_mission_feat is exactly zero on every (mid, v) row no sample has; a scratch pre-filled with NaN changes no
    output."""
    r = _run(4)
    sel = slice(0, n)
    gl, gv = r.gl[sel], r.gv[sel]
    ref, t32 = _refs(r, sel, _linear_loss(gl, gv))
    index = r.index[sel].contiguous()
    got, gb, gm = _kernel_grads(r, r.ev, index, gl, gv)
    _check("n_samples %d" % n, got, ref, t32)
    used = torch.zeros((256, 4), dtype=torch.bool)
    used[r.mid[sel], r.v[sel] - 1] = True
    gm = gm.cpu()
    assert not gm[~used].any()
    assert all(bool(gm[m, v].any()) for m, v in used.nonzero().tolist())
    words = int(r.eng.L.mgx_policy_grad_scratch_words(4, n, 2))
    scratch = torch.full((words,), float("nan"), device=r.eng.device)
    _, gb_nan, gm_nan = _kernel_grads(r, r.ev, index, gl, gv, scratch=scratch)
    assert torch.equal(gb, gb_nan) and not torch.isnan(gb_nan).any()
    if n == 1:
        assert torch.equal(gm, gm_nan.cpu())                          # one tile: one add per float, order-free
    r.eng.poll_error()


def test_bad_arguments_that_read_the_handle():
    """0 < ring_rows < n_stack and a scratch shorter than mgx_policy_grad_scratch_words are MGX_ERR_INVALID."""
    from mgx import _lib
    r = _run(4)
    e, buf, ev = r.eng, r.buf, r.ev
    with torch.no_grad():
        blob, table = ev.inputs()
    n = 130
    f32 = dict(dtype=torch.float32, device=e.device)
    need = int(e.L.mgx_policy_grad_scratch_words(4, n, 2))
    assert need == 2 * blob.numel()
    t = [torch.zeros((n, 7), **f32), torch.zeros(n, **f32), torch.zeros(blob.numel(), **f32),
         torch.zeros((256, 4, 128), **f32), torch.zeros(need, **f32)]
    P = ctypes.c_void_p

    def call(ring, words):
        g = _lib.MgxPolicyGrad(blob_dev=blob.data_ptr(), mission_feat_dev=table.data_ptr(), g_logits_dev=t[0].data_ptr(),
                               g_values_dev=t[1].data_ptr(), grad_blob_dev=t[2].data_ptr(),
                               grad_mission_feat_dev=t[3].data_ptr(), scratch_dev=t[4].data_ptr(),
                               scratch_words=words, max_groups=2)
        return e.L.mgx_policy_backward(e.h, P(buf.rows.data_ptr()), P(buf.mids.data_ptr()), P(buf.starts.data_ptr()),
                                       buf.N, ring, P(r.index.data_ptr()), n, ctypes.byref(g), None)

    for ring, words in ((3, need), (buf.R, need - 1)):
        assert call(ring, words) == 1 and b"mgx_policy_backward" in e.L.mgx_last_error()
    assert call(buf.R, need) == 0
    torch.cuda.synchronize()
    e.poll_error()


def test_learn_smoke():
    """learn() with fused_act and fused_train on gtg 6x6 for two iterations: 280 samples per epoch = four minibatches
    of 64 and one of 24.  Every history entry is finite, every parameter has moved, poll_error() is clean;
    fused_train with layout='sb3' raises ValueError."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgx.ppo import PPOConfig, learn
    cfg = PPOConfig(n_envs=70, horizon=4, batch_size=64, n_epochs=2, fused_act=True, fused_train=True, env=dict(ENV))
    before = {}

    class Cb:                                                          # the initial weights, before any update
        def on_step(self, policy, num_timesteps):
            if not before:
                before.update({n: p.detach().clone() for n, p in policy.named_parameters()})
            return True

    pol, hist, eng = learn(cfg, 2 * 70 * 4, callback=Cb())
    assert len(hist) == 2
    for st in hist:
        for key in ("pg", "vf", "ent", "kl", "clipfrac", "lr", "adv_mean", "adv_std"):
            assert math.isfinite(st[key]), (key, st)
    for n, p in pol.named_parameters():
        assert torch.isfinite(p).all(), n
        assert not torch.equal(p.detach(), before[n]), n
    eng.poll_error()
    with pytest.raises(ValueError):
        learn(PPOConfig(n_envs=70, horizon=4, batch_size=64, fused_train=True, layout="sb3", env=dict(ENV)), 280)
