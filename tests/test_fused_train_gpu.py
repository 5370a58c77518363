"""Fused policy gradient on the GPU (mgx_policy_backward, mgx/fused_train.py) against torch autograd.

Reference: the fp64 CPU deep copy of the module on buf.gather of the same indices, differentiated by autograd.
Yardstick, per parameter tensor and measured in the same run: e_torch = max |torch fp32 GPU autograd - fp64|; the
kernel path may deviate from fp64 by at most max(4 e_torch, 4 eps32 max|ref|) -- the project's margin for fp32 sums
taken in another order, which is what these are.

Setup (as tests/test_fused_policy_gpu.py): gtg 6x6, 70 envs, a ring CompactBuffer of T = 3, 40 random-action steps
over carried-over rollouts, so episode starts fall inside stack windows and the walk-back wraps the ring.  Every
blob parameter is redrawn (weights N(0, 1) / sqrt(fan-in), biases N(0, 0.5^2): no bias is zero; action_net N(0, 1) as
in that file).  Samples: all 210 (t, env) pairs of the current block's three rows = three full tiles and an 18-lane
tail.

Every gtg episode has mission id 3, so a tile there holds at most n_stack (mission id, v) keys.  The *_many_missions,
per-key, Trainer and non-ring tests run the same setup on MULTI (multi 8x8, mission=None: dozens of ids below 128 per
tile), the *_high_mission_ids tests on FULL (ids 128..132 next to ids below 128).  Their samples are the LAST three
observations (38, 39, 40): with more than one mission id, the block's third row -- written a ring cycle earlier, its
walk-back running into newer rows -- would be a stack over two missions, which no rollout holds; and they leave out
the 3 to 6 samples at which conv1's max-pool is tied within fp32 rounding (_ambiguous_pool).  With all 210 samples
kept, MULTI at n_stack 5 and 8 gave conv1.weight 3.1e-3 and 2.7e-3 off the fp64 gradient (bounds 1.0e-6, 1.4e-6; every
other tensor within its bound): the fp64 outputs hold windows whose two best positions are 3.8e-8 and 6.5e-8 apart."""
import copy
import ctypes
import dataclasses
import math

import pytest

torch = pytest.importorskip("torch")

from mgx.policy import ActorCriticPolicy  # noqa: E402

pytestmark = pytest.mark.gpu

N_ENVS, T_RING, STEPS = 70, 3, 40
ENV = dict(problem="gtg", mission=5, size=6, num_objects=2)
MULTI = dict(problem="multi", mission=None, size=8, num_objects=4)
FULL = dict(problem="full", mission=None, size=8, num_objects=4)
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


def _feat64(pol64, obs):
    o = {"image": obs["image"].cpu().double() / 255.0, "direction": obs["direction"].cpu().double(),
         "mission": obs["mission"].cpu()}
    return pol64.features_extractor(o)


def _feat32(pol, obs):
    from mgx.policy import preprocess
    return pol.features_extractor(preprocess(obs))


def _heads(pol, f):
    return pol.action_net(pol.policy_net(f)), pol.value_net(pol.value_net_body(f)).flatten()


def _out64(pol64, obs):
    return _heads(pol64, _feat64(pol64, obs))


def _out32(pol, obs):
    return _heads(pol, _feat32(pol, obs))


def _linear_loss(gl, gv):
    return lambda logits, values: (logits * gl.to(logits)).sum() + (values * gv.to(values)).sum()


def _module_grads(pol, outs, obs, loss):
    """{name: grad (f64, CPU)} of loss(logits, values) by autograd through the module."""
    names, ps = zip(*pol.named_parameters())
    gs = torch.autograd.grad(loss(*outs(pol, obs)), ps)
    return {n: g.detach().double().cpu() for n, g in zip(names, gs)}


def _ambiguous_pool(pol64, obs):
    """bool [B]: the samples at which conv1's ReLU + MaxPool has no gradient that fp32 can agree on with fp64.
    The pool hands a window's cotangent to its largest conv1 output.  Frames are drawn from a few dozen pixel
    values, so windows in which two positions with DIFFERENT input patches are within 1e-7 of each other turn up in
    every run; there the fp32 sum picks either position, and conv1.weight's gradient moves by the whole cotangent
    times the patch difference (1e-3, against a bound of 1e-6).  From the fp64 conv1 output alone: a sample is
    ambiguous if in some window a position whose patch differs from the winner's lies within G of the winner (and
    the winner is not below -G: ReLU stops those), or the winner lies within G of zero.  G = 16 eps32 max(1, |winner|):
    the fp32 value is a chain of 12 n_stack + 1 <= 97 multiply-adds of terms below 1, whose rounding errors add up
    to a few eps32 (a random walk of 97 steps of eps32 / 2: 5 eps32, 7 eps32 for the difference of two such values);
    16 eps32 is twice that.  It leaves out 3 to 6 of 210 samples."""
    x = obs["image"].cpu().double() / 255.0
    conv = pol64.features_extractor.extractors["image"][0]
    with torch.no_grad():
        y = conv(x)                                                    # [B, 16, 6, 6], before the ReLU
    B = y.shape[0]
    win = y.reshape(B, 16, 3, 2, 3, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, 16, 9, 4)      # [.., cell, position]
    pat = torch.nn.functional.unfold(x, 2).reshape(B, -1, 3, 2, 3, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, -1, 9, 4)
    same = (pat[:, :, :, :, None] == pat[:, :, :, None, :]).all(1)     # [B, cell, position, position]
    top, arg = win.max(3)
    g = 16.0 * EPS32 * top.abs().clamp_min(1.0)
    differs = ~same[:, None].expand(B, 16, 9, 4, 4).gather(3, arg[..., None, None].expand(B, 16, 9, 1, 4))[:, :, :, 0]
    tie = ((top[..., None] - win < g[..., None]) & differs).any(3) & (top > -g)
    return (tie | (top.abs() < g)).flatten(1).any(1)


class Run:
    pass


_RUNS = {}


def _run(k, env=ENV, ring=True):
    """One 40-step trajectory per (n_stack, env, buffer form), everything the tests compare recorded once."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    key = (k, tuple(sorted(env.items())), ring)
    if key in _RUNS:
        return _RUNS[key]
    from mgx import MgxEngine
    from mgx.compact import CompactBuffer
    from mgx.fused_train import FusedEvaluator
    r = Run()
    r.k = k
    r.pol = _policy(k).cuda()
    r.pol64 = copy.deepcopy(r.pol).cpu().double()
    r.eng = MgxEngine(n_envs=N_ENVS, n_stack=k, terminal_mode="truncated", mission_dtype=torch.uint8, **env)
    r.buf = CompactBuffer(r.eng, T_RING, ring=ring)
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
    if not ring:
        # observations 0..t of the rollout, rows H..H + t: with R = 0 the walk-back of k - 1 rows stays in the buffer
        # from row H = k - 1 on, and the rows after observation t are the previous rollout's
        obs_t = torch.arange(0, t + 1, device=dev)
        assert int(r.buf.row(0)) == k - 1 and obs_t.numel() == 2
    elif env == ENV:
        obs_t = torch.arange(T_RING, device=dev)
    else:
        obs_t = torch.arange(t + 1 - T_RING, t + 1, device=dev)        # the last three observations (module docstring)
    tt = obs_t.repeat_interleave(N_ENVS)
    ee = torch.arange(N_ENVS, device=dev).repeat(obs_t.numel())
    r.index = r.buf.index(tt, ee).to(torch.int64).contiguous()        # 210 samples (non-ring: 140)
    assert int(r.index.min()) >= 0 and int(r.index.max()) < r.buf.rows.shape[0] * N_ENVS
    if env != ENV:
        # less the few at which the reference has no gradient to compare with: the later samples move up a lane
        amb = _ambiguous_pool(r.pol64, r.buf.gather(r.index, f32=False))
        r.index = r.index[~amb.to(dev)].contiguous()
        print("%s n_stack %d%s: %d of %d samples left out (conv1 pool window tied within fp32 rounding)"
              % (env["problem"], k, "" if ring else " non-ring", int(amb.sum()), amb.numel()))
        assert r.index.numel() > 64 * (obs_t.numel() if ring else 2)  # still that many full tiles and a tail
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
    _RUNS[key] = r
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


def _tile_keys(mid, v, k):
    """[(mid, v)] in lane order for every 64-sample tile."""
    pairs = list(zip(mid.tolist(), v.tolist()))
    return [pairs[i:i + 64] for i in range(0, len(pairs), 64)]


def _assert_many_keys(tag, mid, v, k):
    """What keeps a many-mission test from passing vacuously, from the buffer itself: a full tile with >= 9 distinct
    (mid, v) keys (ordinals reach 8: every quarter of the workgroup owns a third key), >= 12 mission ids, a key whose
    samples are not contiguous in its tile, and at n_stack > 1 a tile with one mid at two v and one v at two mids."""
    tiles = _tile_keys(mid, v, k)
    print("%s: distinct (mid, v) keys per tile %s, mission ids per tile %s, %d ids and %d keys in all"
          % (tag, [len(set(t)) for t in tiles], [len({m for m, _ in t}) for t in tiles],
             len(set(mid.tolist())), len({p for t in tiles for p in t})))
    assert max(len(set(t)) for t in tiles if len(t) == 64) >= 9
    assert len(set(mid.tolist())) >= 12

    def split(t):
        pos = {}
        for i, p in enumerate(t):
            pos.setdefault(p, []).append(i)
        return any(q[-1] - q[0] + 1 != len(q) for q in pos.values())

    assert any(split(t) for t in tiles)
    if k > 1:
        def mixed(t):
            keys = set(t)
            by_mid, by_v = {}, {}
            for m, vv in keys:
                by_mid.setdefault(m, set()).add(vv)
                by_v.setdefault(vv, set()).add(m)
            return any(len(x) > 1 for x in by_mid.values()) and any(len(x) > 1 for x in by_v.values())

        assert any(mixed(t) for t in tiles)


def _assert_high_and_low_ids(tag, mid):
    """One tile holds mission ids >= 128 (MID_DROP, MID_MOVE + d) next to ids below 128."""
    tiles = [mid[i:i + 64] for i in range(0, mid.numel(), 64)]
    print("%s: samples with mission id >= 128 per tile %s, ids %s"
          % (tag, [int((t >= 128).sum()) for t in tiles], sorted(set(mid.tolist()))))
    assert any(bool((t >= 128).any()) and bool((t < 128).any()) for t in tiles)
    assert int(mid.max()) <= 132


@pytest.mark.parametrize("k", [1, 4, 5, 8])
def test_gradient_parity_many_missions(k):
    """test_gradient_parity on MULTI: dozens of (mid, v) keys per tile, so the leader ordinals pass 8, every quarter
    of the workgroup sums several keys, a key's sum skips foreign samples, every lane fetches its own table row
    and the Embedding / GRU gradient runs through a table with dozens of live rows."""
    r = _run(k, MULTI)
    _assert_many_keys("multi n_stack %d" % k, r.mid, r.v, k)
    ref, t32 = _refs(r, slice(None), _linear_loss(r.gl, r.gv))
    got, _, _ = _kernel_grads(r, r.ev, r.index, r.gl, r.gv)
    _check("multi n_stack %d" % k, got, ref, t32)
    r.eng.poll_error()


@pytest.mark.parametrize("k", [4, 8])
def test_gradient_parity_high_mission_ids(k):
    """test_gradient_parity on FULL: mission ids 128..132 (keys up to 132 * n_stack + n_stack - 1) next to ids
    below 128 in one tile."""
    r = _run(k, FULL)
    _assert_high_and_low_ids("full n_stack %d" % k, r.mid)
    ref, t32 = _refs(r, slice(None), _linear_loss(r.gl, r.gv))
    got, _, _ = _kernel_grads(r, r.ev, r.index, r.gl, r.gv)
    _check("full n_stack %d" % k, got, ref, t32)
    r.eng.poll_error()


def test_gradient_parity_non_ring_buffer():
    """n_stack 4 on MULTI over CompactBuffer(ring=False): ring_rows = 0, the walk-back does not wrap.  Samples:
    observations 0 and 1 of the current rollout (rows 3 and 4, whose history rows 0..2 carry_over copied) = two
    full tiles and a tail."""
    r = _run(4, MULTI, ring=False)
    assert not r.buf.ring and 128 < r.index.numel() <= 2 * N_ENVS
    _assert_many_keys("multi non-ring", r.mid, r.v, 4)
    ref, t32 = _refs(r, slice(None), _linear_loss(r.gl, r.gv))
    got, _, _ = _kernel_grads(r, r.ev, r.index, r.gl, r.gv)
    _check("multi non-ring", got, ref, t32)
    r.eng.poll_error()


@pytest.mark.parametrize("k", [4, 8])
def test_grad_mission_feat_per_key(k):
    """grad_mission_feat row by row on MULTI.  Reference: the fp64 module's cotangent of every sample's 128 mission
    features (autograd with respect to the extractor's output, columns 80..207), summed per (mid, v) in fp64.
    e_torch, per row: the same sums from the fp32 module on the GPU.  Every live row within max(4 e_torch, 4 eps32
    max|ref row|), every live row non-zero, every other row exactly zero: the right total in the wrong row fails
    here, where the Embedding / GRU gradients could average it away."""
    r = _run(k, MULTI)
    _assert_many_keys("multi n_stack %d" % k, r.mid, r.v, k)
    loss = _linear_loss(r.gl, r.gv)
    key = r.mid * k + r.v - 1

    def per_key(pol, feat, dev):
        f = feat(pol, r.obs)
        g = torch.autograd.grad(loss(*_heads(pol, f)), f)[0][:, 80:]
        assert g.shape == (key.numel(), 128)
        return torch.zeros((256 * k, 128), dtype=g.dtype, device=dev).index_add_(0, key.to(dev), g).double().cpu()

    ref = per_key(r.pol64, _feat64, "cpu")
    t32 = per_key(r.pol, _feat32, r.eng.device)
    _, _, gm = _kernel_grads(r, r.ev, r.index, r.gl, r.gv)
    gm = gm.reshape(256 * k, 128).double().cpu()
    live = torch.zeros(256 * k, dtype=torch.bool)
    live[key] = True
    assert int(live.sum()) >= 10
    assert not gm[~live].any()
    bad, worst = [], 0.0
    for row in live.nonzero().flatten().tolist():
        e_torch = float((t32[row] - ref[row]).abs().max())
        bound = max(4.0 * e_torch, 4.0 * EPS32 * float(ref[row].abs().max()))
        dev = float((gm[row] - ref[row]).abs().max())
        worst = max(worst, dev / bound)
        assert bool(gm[row].any()) and bound > 0, row
        if not dev <= bound:
            bad.append((row // k, row % k + 1, dev, bound))
    print("multi n_stack %d grad_mission_feat: %d live rows, worst row ratio %.2f" % (k, int(live.sum()), worst))
    assert not bad, bad
    r.eng.poll_error()


def _ppo_terms(cfg, actions, old_v, old_lp, adv, ret):
    """Trainer.train's (policy_loss, value_loss, entropy_loss) from (values, log_prob, entropy)."""
    def terms(values, log_prob, entropy):
        c = lambda x: x.to(values)  # noqa: E731
        a = (c(adv) - c(adv).mean()) / (c(adv).std() + 1e-8)
        ratio = torch.exp(log_prob - c(old_lp))
        policy_loss = -torch.min(a * ratio, a * torch.clamp(ratio, 1 - cfg.clip_range, 1 + cfg.clip_range)).mean()
        vp = c(old_v) + torch.clamp(values - c(old_v), -cfg.clip_range_vf, cfg.clip_range_vf)
        value_loss = torch.nn.functional.mse_loss(c(ret), vp)
        return policy_loss, value_loss, -torch.mean(entropy)
    return terms


def _ppo_loss(cfg, actions, old_v, old_lp, adv, ret):
    """Trainer.train's loss from (values, log_prob, entropy)."""
    terms = _ppo_terms(cfg, actions, old_v, old_lp, adv, ret)

    def loss(values, log_prob, entropy):
        pg, vf, ent = terms(values, log_prob, entropy)
        return pg + cfg.ent_coef * ent + cfg.vf_coef * vf
    return loss


def _via(outs, actions):
    """(pol, obs) -> (values, log_prob, entropy) of `actions`, as evaluate_actions, from outs' (logits, values)."""
    def f(pol, obs):
        logits, values = outs(pol, obs)
        dist = torch.distributions.Categorical(logits=logits)
        return values, dist.log_prob(actions.to(logits.device)), dist.entropy()
    return f


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
    ref = _module_grads(r.pol64, _via(_out64, actions), r.obs, loss)
    t32 = _module_grads(r.pol, _via(_out32, actions), r.obs, loss)
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


_TRAINER = {}


def _trainer_case():
    """One CompactRolloutCollector.collect (fused_act) on MULTI, 70 envs, horizon 4, n_stack 4, then Trainer.train
    from deep copies of the policy (optimiser included) with fused_train off and on and one fixed permutation:
    a whole epoch (four minibatches of 64 and one of 24) with everything minibatches / minibatch_indices yield
    recorded, and the first minibatch alone (p.grad as train() leaves it -- clipped, the step taken from it -- and
    the returned statistics, which are then that minibatch's)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if _TRAINER:
        return _TRAINER["r"]
    from mgx import MgxEngine
    from mgx.ppo import PPOConfig, Trainer, make_collector
    r = Run()
    r.cfg = cfg = PPOConfig(n_envs=N_ENVS, horizon=4, batch_size=64, n_epochs=1, n_frames_stack=4, fused_act=True,
                            env=dict(MULTI))
    r.pol = pol = _policy(4).cuda()
    r.pol64 = copy.deepcopy(pol).cpu().double()
    r.eng = eng = MgxEngine(n_envs=N_ENVS, seed=cfg.seed, n_stack=4, terminal_mode="truncated",
                            mission_dtype=torch.uint8, reward64=True, **MULTI)
    col = make_collector(eng, pol, cfg)
    col.start()
    r.ro = ro = col.collect()
    perm = torch.randperm(ro.T * ro.N, generator=torch.Generator().manual_seed(7)).to(eng.device)
    # the samples without a gradient to compare with (_ambiguous_pool) go last: none is in the first minibatch
    amb = _ambiguous_pool(r.pol64, ro.buf.gather(ro.buf.index(perm % ro.T, perm // ro.T), f32=False)).to(eng.device)
    assert int(amb.sum()) <= 24
    perm = torch.cat([perm[~amb], perm[amb]])
    log ={"minibatches": [], "minibatch_indices": []}

    def record(name):
        inner = getattr(ro, name)

        def batches(batch_size, p):
            for item in inner(batch_size, p):
                obs = item[0]
                obs = {kk: v.clone() for kk, v in obs.items()} if isinstance(obs, dict) else obs.clone()
                log[name].append((obs,) + tuple(x.clone() for x in item[1:]))
                yield item
        setattr(ro, name, batches)

    record("minibatches")
    record("minibatch_indices")

    def train(fused, p):
        q = copy.deepcopy(pol)
        assert q.optimizer.param_groups[0]["params"][0] is next(q.parameters())
        st = Trainer(q, dataclasses.replace(cfg, fused_train=fused)).train(ro, 1.0, perm_fn=lambda n: p)
        eng.poll_error()
        return q, st

    train(False, perm)
    train(True, perm)
    r.epoch = {kk: list(v) for kk, v in log.items()}
    for v in log.values():
        v.clear()
    r.first = {fused: train(fused, perm[:64]) for fused in (False, True)}
    r.first_batch = log["minibatch_indices"][0]
    assert len(log["minibatches"]) == len(log["minibatch_indices"]) == 1
    _TRAINER["r"] = r
    return r


def test_trainer_minibatch_pairing():
    """fused_train on and off see the same minibatches: actions, old values, old log-probs, advantages and returns
    bit-equal, and buf.gather(f32=True) of the indices minibatch_indices yields = the observation minibatches
    yields, bit for bit.  Both are pinned to the observation the collector acted on: the fp64 module's value of the
    gathered stack is the stored old value within 4 x e_torch (e_torch: the fp32 module on the same stacks), which
    a transposed (t, env) or a ring block off by one misses by the spread of the values."""
    r = _trainer_case()
    buf = r.ro.buf
    a, b = r.epoch["minibatches"], r.epoch["minibatch_indices"]
    assert [x[1].numel() for x in a] == [x[1].numel() for x in b] == [64, 64, 64, 64, 24]
    seen = []
    for i, (u, f) in enumerate(zip(a, b)):
        for j in range(1, 6):
            assert torch.equal(u[j], f[j]), (i, j)
        assert f[0].shape == (u[1].numel(),)
        obs = buf.gather(f[0], f32=True)
        for kk in ("image", "direction", "mission"):
            assert torch.equal(obs[kk], u[0][kk]), (i, kk)
        seen.append(f[0])
    index = torch.cat(seen)
    assert index.unique().numel() == r.ro.T * r.ro.N                    # every sample once
    assert buf.mids.reshape(-1)[index].unique().numel() >= 12
    stacks = buf.gather(index, f32=False)
    with torch.no_grad():
        v64 = _out64(r.pol64, stacks)[1]
        e_torch = float((_out32(r.pol, stacks)[1].double().cpu() - v64).abs().max())
    dev = float((torch.cat([f[2] for f in b]).double().cpu() - v64).abs().max())
    print("stored values of the yielded indices: max |dev| %.3e, torch fp32 %.3e; spread of the values %.3e"
          % (dev, e_torch, float(v64.std())))
    assert 0 < e_torch and dev <= 4.0 * e_torch
    r.eng.poll_error()


def _first_minibatch_refs(r):
    """The first minibatch's fp64 side: (evaluate_actions outputs -> PPO terms, loss, u8 stacks)."""
    index, actions, old_v, old_lp, adv, ret = r.first_batch
    stacks = r.ro.buf.gather(index, f32=False)
    args = (r.cfg, actions.cpu(), old_v.cpu(), old_lp.cpu(), adv.cpu(), ret.cpu())
    return stacks, actions.cpu(), _ppo_terms(*args), _ppo_loss(*args)


def test_trainer_first_step_gradients():
    """p.grad of the first optimiser step (as Trainer.train leaves it: after the gradient-norm clip) with
    fused_train on, against the fp64 module with the same loss on the same minibatch and the same clip; e_torch is
    the fused_train=False run's p.grad.  Gradients, not the weights after the step: Adam's first step is lr *
    sign(g), which turns a rounding difference in a near-zero gradient into 2 lr."""
    r = _trainer_case()
    stacks, actions, _, loss = _first_minibatch_refs(r)
    ref = _module_grads(r.pol64, _via(_out64, actions), stacks, loss)
    norm = math.sqrt(sum(float(g.pow(2).sum()) for g in ref.values()))
    coef = min(1.0, r.cfg.max_grad_norm / (norm + 1e-6))                 # torch.nn.utils.clip_grad_norm_
    ref = {n: g * coef for n, g in ref.items()}
    grads = {fused: {n: p.grad.double().cpu() for n, p in r.first[fused][0].named_parameters()}
             for fused in (False, True)}
    print("first step: fp64 gradient norm %.4f, clip coefficient %.4f" % (norm, coef))
    _check("trainer first step", grads[True], ref, grads[False])
    for n, p in r.first[True][0].named_parameters():
        assert not torch.equal(p.detach(), dict(r.pol.named_parameters())[n].detach()), n


def test_trainer_first_minibatch_statistics():
    """pg, vf and ent returned by Trainer.train for the first minibatch: fused_train on deviates from the fp64
    module's by at most 4 x the fused_train=False run's own deviation."""
    r = _trainer_case()
    stacks, actions, terms, _ = _first_minibatch_refs(r)
    with torch.no_grad():
        ref = dict(zip(("pg", "vf", "ent"), (float(x) for x in terms(*_via(_out64, actions)(r.pol64, stacks)))))
    bad = []
    for q in ("pg", "vf", "ent"):
        e_torch = abs(r.first[False][1][q] - ref[q])
        dev = abs(r.first[True][1][q] - ref[q])
        print("first minibatch %s: fp64 %.9f, fused |dev| %.3e, unfused |dev| %.3e, bound %.3e"
              % (q, ref[q], dev, e_torch, 4.0 * e_torch))
        if not dev <= 4.0 * e_torch:
            bad.append((q, dev, e_torch))
    assert not bad, bad
