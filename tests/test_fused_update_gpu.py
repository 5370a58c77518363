"""Fused PPO update on the GPU (mgx_ppo_loss, mgx_adam_step, mgx/fused_update.py) against torch.

Yardstick (the project's).  Reference: the fp64 CPU restatement of Trainer.train's formulas differentiated by
autograd, or fp64 clip_grad_norm_ + torch.optim.Adam, fed the same fp32 inputs cast up.  e_torch is the deviation of
the same torch code in fp32 on the GPU from that reference, measured in the same test.  A tensor may deviate by at most
max(4 e_torch, 4 eps32 max|ref|).  For a scalar statistic that is a mean over samples the floor is 4 eps32 mean_i |u_i|
with u the addends (policy loss: A r; value loss: (ret - vp)^2; entropy: H; kl: |r - 1| + |log r|; loss: the weighted sum
of the first three): a mean's rounding scales with its addends, not with a value that nearly cancels.  The advantage
mean is such a mean (u = a); the advantage std and the total gradient norm are roots of sums of squares whose rounding
is relative to the value itself: floor 4 eps32 |ref|.  Every comparison prints dev, e_torch and bound.

Synthetic loss inputs are constructed, not filtered: logits 2 N(0, 1), old_lp = fp64 lp - N(0, 0.1^2), old_v = v -
N(0, 0.08^2), c = 0.1, c_v the config's; a sample whose fp64 ratio lies within 1e-4 of 1 +- c, or whose |v - old_v|
lies within 1e-4 of c_v, is moved off by 5e-3 and the test asserts that none is left, so that every branch decision
is the same in fp32 and fp64 and clip_fraction can be compared exactly."""
import copy
import dataclasses
import math

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

EPS32 = float(torch.finfo(torch.float32).eps)
CLIP = 0.1
LOSS_B = (1, 2, 63, 64, 65, 257, 4099, 65793)      # 65793 > 256 workgroups x 256 samples: threads take a second sample
STAT_NAMES = ("pg", "vf", "ent", "kl", "clipfrac", "loss", "adv_mean", "adv_std")
ADV_STATS = (0.25, 1.4)                            # adv_mode 2


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _cfg():
    from mgx.ppo import PPOConfig
    return PPOConfig()


# ---------------------------------------------------------------------------------------- mgx_ppo_loss

_INPUTS = {}


def _loss_inputs(B):
    """The synthetic batch of size B (CPU tensors), built once."""
    if B in _INPUTS:
        return _INPUTS[B]
    cv = _cfg().clip_range_vf
    g = torch.Generator().manual_seed(1000 + B)
    logits = (2.0 * torch.randn((B, 7), generator=g)).float()
    values = torch.randn(B, generator=g).float()
    actions = torch.randint(0, 7, (B,), generator=g)
    lp64 = torch.log_softmax(logits.double(), 1).gather(1, actions[:, None])[:, 0]
    old_lp = (lp64 - 0.1 * torch.randn(B, generator=g).double()).float()
    old_v = (values.double() - 0.08 * torch.randn(B, generator=g).double()).float()
    if B <= 2:
        old_v[0] = values[0] - 0.02                                   # an unclipped value: g_values is not all zero
    adv = (0.3 + 1.5 * torch.randn(B, generator=g)).float()
    ret = (values.double() + 0.3 * torch.randn(B, generator=g).double()).float()

    def ratio():
        return torch.exp(lp64 - old_lp.double())

    def vdist():
        return (values.double() - old_v.double()).abs()

    near = ((ratio() - (1 + CLIP)).abs() < 1e-4) | ((ratio() - (1 - CLIP)).abs() < 1e-4)
    old_lp[near] -= 5e-3
    near_v = (vdist() - cv).abs() < 1e-4
    old_v[near_v] -= 5e-3 * torch.sign(values[near_v] - old_v[near_v])
    r = ratio()
    assert not (((r - (1 + CLIP)).abs() < 1e-4) | ((r - (1 - CLIP)).abs() < 1e-4)).any()
    assert not ((vdist() - cv).abs() < 1e-4).any()
    d = dict(B=B, logits=logits, values=values, actions=actions, old_lp=old_lp, old_v=old_v, adv=adv, ret=ret,
             nudged=(int(near.sum()), int(near_v.sum())))
    # the same samples scattered into arrays longer than B, addressed through a permutation
    L = B + 37
    sel = torch.randperm(L, generator=g)[:B]
    for name in ("actions", "old_lp", "old_v", "adv", "ret"):
        x = d[name]
        long = torch.full((L,), 3, dtype=x.dtype) if name == "actions" else torch.full((L,), float("nan"))
        long[sel] = x
        d[name + "_long"] = long
    d["sel"] = sel
    _INPUTS[B] = d
    return d


def _torch_loss(d, adv_mode, vclip, dtype, device):
    """Trainer.train's loss block on (logits, values) in `dtype` on `device` -> (g_logits, g_values, stats, u)."""
    cfg = _cfg()
    c = lambda x: x.to(device=device, dtype=dtype)  # noqa: E731
    z = c(d["logits"]).requires_grad_(True)
    v = c(d["values"]).requires_grad_(True)
    actions = d["actions"].to(device)
    old_v, old_lp, adv, ret = c(d["old_v"]), c(d["old_lp"]), c(d["adv"]), c(d["ret"])
    dist = torch.distributions.Categorical(logits=z)
    log_prob, entropy = dist.log_prob(actions), dist.entropy()
    mean, std = 0.0, 1.0
    if adv_mode == 1 and adv.numel() > 1:
        mean, std = adv.mean(), adv.std()
        adv = (adv - mean) / (std + 1e-8)
    elif adv_mode == 2:
        mean, std = (torch.tensor(x, dtype=torch.float32).to(device=device, dtype=dtype) for x in ADV_STATS)
        adv = (adv - mean) / (std + 1e-8)
    ratio = torch.exp(log_prob - old_lp)
    pl1 = adv * ratio
    pl2 = adv * torch.clamp(ratio, 1 - CLIP, 1 + CLIP)
    policy_loss = -torch.min(pl1, pl2).mean()
    vp = old_v + torch.clamp(v - old_v, -cfg.clip_range_vf, cfg.clip_range_vf) if vclip else v
    value_loss = torch.nn.functional.mse_loss(ret, vp)
    entropy_loss = -torch.mean(entropy)
    loss = policy_loss + cfg.ent_coef * entropy_loss + cfg.vf_coef * value_loss
    gz, gv = torch.autograd.grad(loss, (z, v))
    with torch.no_grad():
        log_ratio = log_prob - old_lp
        kl = torch.mean((torch.exp(log_ratio) - 1) - log_ratio)
        clipfrac = torch.mean((torch.abs(ratio - 1) > CLIP).to(dtype))
        stats = dict(pg=policy_loss, vf=value_loss, ent=entropy_loss, kl=kl, clipfrac=clipfrac, loss=loss,
                     adv_mean=mean, adv_std=std)
        stats = {k: float(x) for k, x in stats.items()}
        u_pg, u_vf, u_ent = (adv * ratio).abs().mean(), ((ret - vp) ** 2).mean(), entropy.abs().mean()
        u = dict(pg=float(u_pg), vf=float(u_vf), ent=float(u_ent),
                 kl=float(((ratio - 1).abs() + log_ratio.abs()).mean()),
                 loss=float(u_pg + cfg.ent_coef * u_ent + cfg.vf_coef * u_vf),
                 adv_mean=float(c(d["adv"]).abs().mean()), adv_std=abs(float(std)))
        branches = dict(A=adv.detach().cpu(), r=ratio.detach().cpu(), dv=(v - old_v).detach().abs().cpu())
    return gz.detach().double().cpu(), gv.detach().double().cpu(), stats, u, branches


_REFS = {}


def _loss_refs(B, adv_mode, vclip):
    """(fp64 CPU, fp32 GPU) results of _torch_loss, shared by the sel / no-sel cases."""
    key = (B, adv_mode, vclip)
    if key not in _REFS:
        d = _loss_inputs(B)
        _REFS[key] = (_torch_loss(d, adv_mode, vclip, torch.float64, "cpu"),
                      _torch_loss(d, adv_mode, vclip, torch.float32, "cuda"))
    return _REFS[key]


def _kernel_loss(d, adv_mode, vclip, use_sel):
    from mgx.fused_update import ppo_loss
    cfg = _cfg()
    suffix = "_long" if use_sel else ""
    arrays = [d[n + suffix].cuda().contiguous() for n in ("actions", "old_v", "old_lp", "adv", "ret")]
    out = ppo_loss(d["logits"].cuda(), d["values"].cuda(), *arrays, CLIP, cfg.clip_range_vf if vclip else 0.0,
                   cfg.ent_coef, cfg.vf_coef, adv_mode=adv_mode, sel=d["sel"].cuda() if use_sel else None,
                   adv_stats=torch.tensor(ADV_STATS, dtype=torch.float32).cuda() if adv_mode == 2 else None)
    torch.cuda.synchronize()
    return out


def _assert_branches(B, br, vclip):
    cv = _cfg().clip_range_vf
    A, r, dv = br["A"], br["r"], br["dv"]
    if B >= 63:
        for name, m in (("above", r > 1 + CLIP), ("below", r < 1 - CLIP), ("inside", (r >= 1 - CLIP) & (r <= 1 + CLIP))):
            assert int((m & (A > 0)).sum()) > 0 and int((m & (A < 0)).sum()) > 0, (B, name)
        assert int((dv > cv).sum()) > 0 and int((dv <= cv).sum()) > 0, B
    if B == 2:
        assert int((dv <= cv).sum()) > 0


def _loss_compare(B, adv_mode, vclip, use_sel):
    """One mgx_ppo_loss call against the yardstick -> ([(name, dev, e_torch, bound)] of g_logits, g_values and the
    seven statistics that are not clip_fraction, every line printed; the kernel's outputs; the fp64 statistics)."""
    d = _loss_inputs(B)
    (gz64, gv64, st64, u, br), (gz32, gv32, st32, _, _) = _loss_refs(B, adv_mode, vclip)
    _assert_branches(B, br, vclip)
    tag = "B %d adv_mode %d vclip %d sel %d" % (B, adv_mode, vclip, use_sel)
    out = _kernel_loss(d, adv_mode, vclip, use_sel)
    rows = []
    for name, got, ref, t32 in (("g_logits", out[0], gz64, gz32), ("g_values", out[1], gv64, gv32)):
        e_torch = float((t32 - ref).abs().max())
        bound = max(4.0 * e_torch, 4.0 * EPS32 * float(ref.abs().max()))
        dev = float((got.double().cpu() - ref).abs().max())
        print("%s %s: kernel max |dev| %.3e, torch fp32 %.3e, bound %.3e, ratio %.2f"
              % (tag, name, dev, e_torch, bound, dev / bound if bound else float("inf")))
        assert torch.isfinite(got).all()
        assert float(ref.abs().max()) > 0, name
        rows.append((name, dev, e_torch, bound))
    s = out[2].double().cpu().tolist()
    for i, name in enumerate(STAT_NAMES):
        if name == "clipfrac":
            continue
        e_torch = abs(st32[name] - st64[name])
        bound = max(4.0 * e_torch, 4.0 * EPS32 * u[name])
        dev = abs(s[i] - st64[name])
        print("%s %s: fp64 %.9f, kernel |dev| %.3e, torch fp32 %.3e, bound %.3e, ratio %.2f"
              % (tag, name, st64[name], dev, e_torch, bound, dev / bound if bound else 0.0))
        rows.append((name, dev, e_torch, bound))
    return rows, out, st64


@pytest.mark.parametrize("use_sel", [False, True])
@pytest.mark.parametrize("vclip", [True, False])
@pytest.mark.parametrize("adv_mode", [0, 1, 2])
@pytest.mark.parametrize("B", LOSS_B)
def test_ppo_loss_parity(B, adv_mode, vclip, use_sel):
    """g_logits, g_values and the eight statistics within the yardstick; clip_fraction exact; two calls bit-equal."""
    _gpu()
    rows, out, st64 = _loss_compare(B, adv_mode, vclip, use_sel)
    s = out[2].double().cpu().tolist()
    want = float(torch.tensor(st64["clipfrac"], dtype=torch.float64).float())
    print("clipfrac: kernel %.9f, fp64 %.9f" % (s[4], want))
    assert s[4] == want, (s[4], want)
    if adv_mode == 0 or (adv_mode == 1 and B == 1):
        assert s[6] == 0.0 and s[7] == 1.0
    if adv_mode == 2:
        assert s[6] == float(torch.tensor(ADV_STATS[0]).float()) and s[7] == float(torch.tensor(ADV_STATS[1]).float())
    again = _kernel_loss(_loss_inputs(B), adv_mode, vclip, use_sel)
    for x, y in zip(out, again):
        assert torch.equal(x, y)
    bad = [r for r in rows if not r[1] <= r[3]]
    assert not bad, bad


def test_ppo_loss_scratch_prefilled_with_nan():
    """The scratch need not be zeroed: a NaN-filled one gives the same bits."""
    _gpu()
    from mgx import _lib
    from mgx.fused_update import ppo_loss
    d = _loss_inputs(257)
    cfg = _cfg()
    arrays = [d[n].cuda() for n in ("actions", "old_v", "old_lp", "adv", "ret")]
    words = int(_lib.load().mgx_ppo_loss_scratch_words(257))
    outs = []
    for fill in (0.0, float("nan")):
        scratch = torch.full((words,), fill, device="cuda")
        outs.append(ppo_loss(d["logits"].cuda(), d["values"].cuda(), *arrays, CLIP, cfg.clip_range_vf, cfg.ent_coef,
                             cfg.vf_coef, adv_mode=1, scratch=scratch))
    torch.cuda.synchronize()
    for x, y in zip(*outs):
        assert torch.equal(x, y) and torch.isfinite(x).all()


# ---------------------------------------------------------------------------------------- mgx_adam_step

MAX_NORM = 0.5215982006116593
LR, BETAS, ADAM_EPS = 3e-4, (0.9, 0.999), 1e-8


def _adam_sizes():
    from mgx.fused_update import arena_layout
    return (1, 63, 64, 65, 1025, arena_layout(4)[1], 300001)   # the last: above 256 x 1,024 words, several per thread


def _adam_inputs(n, target_norm):
    """(param, three gradients), fp32 CPU; each gradient N(0, 1) scaled to the norm `target_norm`."""
    g = torch.Generator().manual_seed(2000 + n)
    param = torch.randn(n, generator=g)
    grads = []
    for _ in range(3):
        x = torch.randn(n, generator=g)
        grads.append((x * (target_norm / float(x.norm()))).float())
    return param, grads


def _torch_adam(param, grads, max_norm, dtype, device, state=None):
    """clip_grad_norm_ + torch.optim.Adam, three steps -> per step (param, exp_avg, exp_avg_sq, grad, total norm).
    state: (exp_avg, exp_avg_sq, first step) the optimizer starts from, as after load_state_dict."""
    p = torch.nn.Parameter(param.to(device=device, dtype=dtype).clone())
    opt = torch.optim.Adam([p], lr=LR, betas=BETAS, eps=ADAM_EPS)
    if state is not None:
        opt.state[p] = {"step": torch.tensor(float(state[2] - 1)),
                        "exp_avg": state[0].to(device=device, dtype=dtype).clone(),
                        "exp_avg_sq": state[1].to(device=device, dtype=dtype).clone()}
    out = []
    for g in grads:
        p.grad = g.to(device=device, dtype=dtype).clone()
        if max_norm > 0:
            total = torch.nn.utils.clip_grad_norm_([p], max_norm)
        else:
            total = p.grad.norm()
        opt.step()
        st = opt.state[p]
        out.append(tuple(x.detach().double().cpu().clone() for x in (p, st["exp_avg"], st["exp_avg_sq"], p.grad))
                   + (float(total),))
    return out


def _kernel_adam(param, grads, max_norm, grad_scale=1.0, state=None):
    from mgx.fused_update import adam_step
    n = param.numel()
    p = param.cuda().clone()
    m, v, first = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), 1
    if state is not None:
        m, v, first = state[0].cuda().clone(), state[1].cuda().clone(), state[2]
    norm = torch.zeros(1, device="cuda")
    out = []
    for i, g in enumerate(grads):
        gg = g.cuda().clone()
        adam_step(p, gg, m, v, LR, first + i, betas=BETAS, eps=ADAM_EPS, max_grad_norm=max_norm,
                  grad_scale=grad_scale, total_norm=norm)
        torch.cuda.synchronize()
        out.append((p.clone(), m.clone(), v.clone(), gg, norm.clone()))
    return out


RESUMED_STEP = 12345                               # a resumed run: Adam's bias corrections are all but 1


def _adam_state(n):
    """(exp_avg, exp_avg_sq >= 0, first step) of a run resumed at RESUMED_STEP: random moments of the size the
    clipped gradients of _adam_inputs leave behind."""
    g = torch.Generator().manual_seed(4000 + n)
    scale = MAX_NORM / math.sqrt(n)
    return scale * torch.randn(n, generator=g), (scale * torch.randn(n, generator=g)) ** 2, RESUMED_STEP


def _adam_compare(n, case):
    """Three consecutive mgx_adam_step calls against the yardstick -> ([(name, dev, e_torch, bound)], the kernel's
    outputs, the inputs).  clip: gradient norm 4 x max_grad_norm; noclip: a quarter of it; off: max_grad_norm = 0
    with the large gradients; resumed: clip, from _adam_state's moments and step in every path."""
    target = MAX_NORM * (0.25 if case == "noclip" else 4.0)
    max_norm = 0.0 if case == "off" else MAX_NORM
    state = _adam_state(n) if case == "resumed" else None
    param, grads = _adam_inputs(n, target)
    ref = _torch_adam(param, grads, max_norm, torch.float64, "cpu", state)
    t32 = _torch_adam(param, grads, max_norm, torch.float32, "cuda", state)
    got = _kernel_adam(param, grads, max_norm, state=state)
    rows = []
    for step in range(3):
        for j, name in enumerate(("param", "exp_avg", "exp_avg_sq", "grad")):
            e_torch = float((t32[step][j] - ref[step][j]).abs().max())
            bound = max(4.0 * e_torch, 4.0 * EPS32 * float(ref[step][j].abs().max()))
            dev = float((got[step][j].double().cpu() - ref[step][j]).abs().max())
            print("n %d %s step %d %s: kernel max |dev| %.3e, torch fp32 %.3e, bound %.3e, ratio %.2f"
                  % (n, case, step + 1 if state is None else state[2] + step, name, dev, e_torch, bound, dev / bound))
            rows.append(("step %d %s" % (step + 1, name), dev, e_torch, bound))
        e_torch = abs(t32[step][4] - ref[step][4])
        bound = max(4.0 * e_torch, 4.0 * EPS32 * abs(ref[step][4]))
        dev = abs(float(got[step][4]) - ref[step][4])
        print("n %d %s step %d total norm: fp64 %.9f, kernel |dev| %.3e, torch fp32 %.3e, bound %.3e"
              % (n, case, step + 1, ref[step][4], dev, e_torch, bound))
        rows.append(("step %d total_norm" % (step + 1), dev, e_torch, bound))
        clipped = float(ref[step][3].norm()) < 0.99 * target
        assert clipped == (case in ("clip", "resumed"))
    return rows, got, (param, grads, max_norm, 1.0, state)


@pytest.mark.parametrize("case", ["clip", "noclip", "off"])
@pytest.mark.parametrize("size", range(7))
def test_adam_step_parity(size, case):
    """Three consecutive steps, each path carrying its own state: param, both moments, the written-back clipped
    gradient and the total norm after every step, with the clip active, inactive and switched off.  Two runs are
    bit-equal."""
    _gpu()
    rows, got, inputs = _adam_compare(_adam_sizes()[size], case)
    again = _kernel_adam(*inputs)
    for a, b in zip(got, again):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    bad = [r for r in rows if not r[1] <= r[3]]
    assert not bad, bad


@pytest.mark.parametrize("size", [0, 5, 6])
def test_adam_step_parity_resumed(size):
    """What a resumed run asks of mgx_adam_step: three steps from imported non-zero moments (exp_avg_sq >= 0) at
    step 12,345, against fp64 clip_grad_norm_ + torch.optim.Adam whose state was set to the same moments and step,
    by the file's yardstick.  The same steps through adam_schedule(first_step=12345) + mgx_adam_step_sched equal the
    by-value calls bit for bit."""
    _gpu()
    from mgx.fused_update import adam_schedule, adam_step_sched
    n = _adam_sizes()[size]
    rows, got, inputs = _adam_compare(n, "resumed")
    param, grads, max_norm, _, state = inputs
    assert state[2] == RESUMED_STEP and state[0].any() and bool((state[1] >= 0).all()) and state[1].any()
    again = _kernel_adam(*inputs)
    for a, b in zip(got, again):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    table = adam_schedule([LR] * 3, first_step=RESUMED_STEP, betas=BETAS, eps=ADAM_EPS).cuda()
    cursor = torch.zeros(2, dtype=torch.int32, device="cuda")
    p, m, v = param.cuda().clone(), state[0].cuda().clone(), state[1].cuda().clone()
    norm = torch.zeros(1, device="cuda")
    for i, g in enumerate(grads):
        gg = g.cuda().clone()
        adam_step_sched(p, gg, m, v, table, cursor, betas=BETAS, eps=ADAM_EPS, max_grad_norm=max_norm,
                        total_norm=norm)
        torch.cuda.synchronize()
        for name, x, y in zip(("param", "exp_avg", "exp_avg_sq", "grad", "total_norm"), (p, m, v, gg, norm), got[i]):
            assert x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)), (i, name)
        assert cursor.tolist() == [i + 1, 0]
    assert not torch.equal(got[2][0], param.cuda()) and not torch.equal(got[2][1], state[0].cuda())
    bad = [r for r in rows if not r[1] <= r[3]]
    assert not bad, bad


@pytest.mark.parametrize("size", range(7))
def test_adam_grad_scale(size):
    """grad_scale = 0.5 equals pre-halved gradients with grad_scale = 1, bit for bit (halving is exact)."""
    _gpu()
    n = _adam_sizes()[size]
    param, grads = _adam_inputs(n, 4.0 * MAX_NORM)
    a = _kernel_adam(param, grads, MAX_NORM, grad_scale=0.5)
    b = _kernel_adam(param, [0.5 * g for g in grads], MAX_NORM)
    for x, y in zip(a, b):
        for s, t in zip(x, y):
            assert torch.equal(s, t)
    assert not torch.equal(a[2][0], param.cuda())


def test_adam_non_finite_gradients_propagate_as_in_torch():
    """One NaN gradient makes the norm, every written-back gradient and every parameter NaN; one +inf gradient gives
    coefficient 0: that gradient becomes NaN (inf * 0), the others 0 -- the NaN pattern of torch's fp32 path."""
    _gpu()
    param, grads = _adam_inputs(65, 4.0 * MAX_NORM)
    for bad_value in (float("nan"), float("inf")):
        g = grads[0].clone()
        g[7] = bad_value
        t32 = _torch_adam(param, [g], MAX_NORM, torch.float32, "cuda")[0]
        got = _kernel_adam(param, [g], MAX_NORM)[0]
        for j in range(4):
            assert torch.equal(torch.isnan(got[j].cpu()), torch.isnan(t32[j])), (bad_value, j)
            ok = ~torch.isnan(t32[j])
            assert torch.allclose(got[j].double().cpu()[ok], t32[j][ok], rtol=1e-5, atol=1e-7)
        assert math.isnan(float(got[4])) == math.isnan(t32[4]) and math.isinf(float(got[4])) == math.isinf(t32[4])
        assert torch.isnan(got[0]).any()


# ---------------------------------------------------------------------------------------- end to end

_E2E = {}


def _e2e():
    """test_fused_train_gpu._trainer_case's rollout and permutation; Trainer.train on the first minibatch and on the
    whole epoch from deep copies of the policy with fused_train + fused_mission and fused_update off / on."""
    _gpu()
    if _E2E:
        return _E2E["r"]
    import test_fused_train_gpu as T
    from mgx.ppo import Trainer
    r = T._trainer_case()
    ro, eng = r.ro, r.eng
    perm = torch.randperm(ro.T * ro.N, generator=torch.Generator().manual_seed(7)).to(eng.device)
    amb = T._ambiguous_pool(r.pol64, ro.buf.gather(ro.buf.index(perm % ro.T, perm // ro.T), f32=False)).to(eng.device)
    perm = torch.cat([perm[~amb], perm[amb]])
    first = perm[:64]
    assert torch.equal(ro.buf.index(first % ro.T, first // ro.T), r.first_batch[0])      # _trainer_case's minibatch
    base = dataclasses.replace(r.cfg, fused_train=True, fused_mission=True)

    def train(cfg, p):
        q = copy.deepcopy(r.pol)
        tr = Trainer(q, cfg)
        st = tr.train(ro, 1.0, perm_fn=lambda n: p)
        eng.poll_error()
        return q, st, tr

    e = T.Run()
    e.T, e.r, e.perm = T, r, perm
    e.off = train(dataclasses.replace(base, fused_update=False), first)
    e.off_again = train(dataclasses.replace(base, fused_update=False), first)
    e.untouched = train(base, first)
    e.on = train(dataclasses.replace(base, fused_update=True), first)
    e.toggle = train(dataclasses.replace(base, fused_update=True), first)      # test_trainer_flag_toggles_on_one_policy
    e.epoch_on = train(dataclasses.replace(base, fused_update=True), perm)
    e.epoch_off = train(base, perm)
    _E2E["r"] = e
    return e


def test_trainer_flag_off_is_the_parent_path():
    """With fused_update off Trainer.train is the parent's path: two runs and a run whose config never names the
    field give bit-equal parameters, gradients and statistics, and no arena is made."""
    e = _e2e()
    for other in (e.off_again, e.untouched):
        assert other[2].update is None and e.off[2].update is None
        assert other[1] == e.off[1]
        for (n, p), q in zip(e.off[0].named_parameters(), other[0].parameters()):
            assert torch.equal(p.detach(), q.detach()) and torch.equal(p.grad, q.grad), n


def test_trainer_first_step_gradients_fused_update():
    """p.grad of all 25 tensors after the first minibatch with fused_update on (the clipped gradient mgx_adam_step
    wrote back) against the fp64 module with the same loss and clip; e_torch is the fused_train + fused_mission run
    with fused_update off.  Gradients, not weights, for the reason test_trainer_first_step_gradients states.  Every
    parameter changed."""
    e = _e2e()
    T, r = e.T, e.r
    stacks, actions, _, loss = T._first_minibatch_refs(r)
    ref = T._module_grads(r.pol64, T._via(T._out64, actions), stacks, loss)
    norm = math.sqrt(sum(float(g.pow(2).sum()) for g in ref.values()))
    coef = min(1.0, r.cfg.max_grad_norm / (norm + 1e-6))
    ref = {n: g * coef for n, g in ref.items()}
    grads = {k: {n: p.grad.double().cpu() for n, p in run[0].named_parameters()} for k, run in
             (("on", e.on), ("off", e.off))}
    print("first step: fp64 gradient norm %.6f, clip coefficient %.4f, kernel norm %.6f"
          % (norm, coef, float(e.on[2].update.total_norm)))
    T._check("fused_update first step", grads["on"], ref, grads["off"])
    before = dict(r.pol.named_parameters())
    for n, p in e.on[0].named_parameters():
        assert torch.isfinite(p).all() and not torch.equal(p.detach(), before[n].detach()), n
    arena = e.on[2].update.arena
    assert arena.attached() and arena.step == 1
    assert int(e.on[0].optimizer.state_dict()["state"][0]["step"]) == 1


def test_trainer_first_minibatch_statistics_fused_update():
    """pg, vf and ent of the first minibatch within max(4 e_torch, 4 eps32 mean |u|) of the fp64 module's; the first
    minibatch has r = 1 up to rounding, so clipfrac is exactly 0 (its kl is rounding noise: the synthetic test
    covers kl)."""
    e = _e2e()
    T, r = e.T, e.r
    cfg = r.cfg
    stacks, actions, terms, _ = T._first_minibatch_refs(r)
    _, _, old_v, old_lp, adv, ret = (x.cpu() for x in r.first_batch)
    with torch.no_grad():
        values, log_prob, entropy = T._via(T._out64, actions)(r.pol64, stacks)
        ref = dict(zip(("pg", "vf", "ent"), (float(x) for x in terms(values, log_prob, entropy))))
        a = adv.double()
        a = (a - a.mean()) / (a.std() + 1e-8)
        ratio = torch.exp(log_prob - old_lp.double())
        vp = old_v.double() + torch.clamp(values - old_v.double(), -cfg.clip_range_vf, cfg.clip_range_vf)
        u = dict(pg=float((a * ratio).abs().mean()), vf=float(((ret.double() - vp) ** 2).mean()),
                 ent=float(entropy.abs().mean()))
    bad = []
    for q in ("pg", "vf", "ent"):
        e_torch = abs(e.off[1][q] - ref[q])
        bound = max(4.0 * e_torch, 4.0 * EPS32 * u[q])
        dev = abs(e.on[1][q] - ref[q])
        print("first minibatch %s: fp64 %.9f, fused_update |dev| %.3e, torch |dev| %.3e, bound %.3e"
              % (q, ref[q], dev, e_torch, bound))
        if not dev <= bound:
            bad.append((q, dev, bound))
    assert e.on[1]["clipfrac"] == 0.0 and e.off[1]["clipfrac"] == 0.0
    assert set(e.on[1]) == set(e.off[1]) == {"pg", "vf", "ent", "kl", "clipfrac", "lr"}
    assert not bad, bad


def test_trainer_epoch_fused_update():
    """A whole epoch (64, 64, 64, 64, 24) with fused_update on: no error bit, finite statistics close to the
    fused_update-off epoch's, five Adam steps counted, the parameters still views of the arena; FusedActor.sync()
    + logits on the updated weights match the updated module within 4 e_torch as the actor tests bound it."""
    e = _e2e()
    T, r = e.T, e.r
    q, st, tr = e.epoch_on
    arena = tr.update.arena
    assert arena.step == 5 and arena.attached()
    for key, val in st.items():
        assert math.isfinite(val), (key, st)
        print("epoch %s: fused_update on %.7f, off %.7f" % (key, val, e.epoch_off[1][key]))
    for key in ("vf", "ent"):
        assert abs(st[key] - e.epoch_off[1][key]) <= 1e-2 * abs(e.epoch_off[1][key]), key
    for n, p in q.named_parameters():
        assert torch.isfinite(p).all(), n
    from mgx.fused_policy import FusedActor
    actor = FusedActor(q, r.eng, fused_mission=True)
    actor.sync()
    assert torch.equal(actor.blob, arena.param[:arena.blob_words])
    buf = r.ro.buf
    q64 = copy.deepcopy(q).cpu().double()
    bad = []
    for t in (0, r.ro.T - 1):
        logits, values = actor.logits(buf, t)
        stacks = buf.gather_step(t, f32=False)
        with torch.no_grad():
            l64, v64 = T._out64(q64, stacks)
            l32, v32 = T._out32(q, stacks)
        for name, got, ref, t32 in (("logits", logits, l64, l32), ("values", values, v64, v32)):
            e_torch = float((t32.double().cpu() - ref).abs().max())
            dev = float((got.double().cpu() - ref).abs().max())
            print("updated weights t %d %s: kernel max |dev| %.3e, torch fp32 %.3e" % (t, name, dev, e_torch))
            assert e_torch > 0
            if not dev <= 4.0 * e_torch:
                bad.append((t, name, dev, e_torch))
    assert not bad, bad
    r.eng.poll_error()


def test_trainer_flag_toggles_on_one_policy():
    """A run continues with the flag off and on again on the same policy: torch's Adam steps on the exported state
    (moments that are the arena's views, the step count), its zero_grad detaches the gradient views, and the next
    fused_update train() re-attaches them and takes the step count back."""
    e = _e2e()
    from mgx.ppo import Trainer
    q, _, tr = e.toggle
    arena = tr.update.arena
    assert arena.step == 1
    first = e.perm[:64]
    m_before = arena.exp_avg.clone()
    Trainer(q, dataclasses.replace(tr.cfg, fused_update=False)).train(e.r.ro, 1.0, perm_fn=lambda n: first)
    assert int(q.optimizer.state[arena.tensors[0]]["step"]) == 2
    assert not torch.equal(arena.exp_avg, m_before)                     # torch updated the arena's moments in place
    assert not arena.attached()
    st = tr.train(e.r.ro, 1.0, perm_fn=lambda n: first)
    assert arena.attached() and arena.step == 3
    assert int(q.optimizer.state_dict()["state"][0]["step"]) == 3
    assert all(math.isfinite(v) for v in st.values())
    for n, p in q.named_parameters():
        assert torch.isfinite(p).all(), n
    e.r.eng.poll_error()


def test_trainer_group_path(tmp_path):
    """Trainer(group=...) with fused_update: the step all-reduces arena.grad once and passes grad_scale = 1 / world to
    mgx_adam_step.  In a one-rank gloo group the sum is the identity and the scale 1, so parameters, gradients and
    statistics are bit-equal to the run without a group (the scale itself: test_adam_grad_scale)."""
    e = _e2e()
    import torch.distributed as dist
    from mgx.ppo import Trainer
    assert not dist.is_initialized()
    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        q = copy.deepcopy(e.r.pol)
        tr = Trainer(q, e.on[2].cfg, group=dist.group.WORLD)
        assert tr.world == 1
        first = e.perm[:64]
        st = tr.train(e.r.ro, 1.0, perm_fn=lambda n: first)
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    assert st == e.on[1]
    for (n, p), ref in zip(q.named_parameters(), e.on[0].parameters()):
        assert torch.equal(p.detach(), ref.detach()) and torch.equal(p.grad, ref.grad), n
    e.r.eng.poll_error()


def test_learn_smoke_all_fused():
    """learn() with fused_act, fused_train, fused_mission and fused_update on gtg 6x6 for two iterations: every
    history entry is finite, every parameter has moved and is still an arena view, optimizer.state_dict() holds the
    step count, poll_error() is clean."""
    _gpu()
    from mgx.ppo import PPOConfig, learn
    cfg = PPOConfig(n_envs=70, horizon=4, batch_size=64, n_epochs=2, fused_act=True, fused_train=True,
                    fused_mission=True, fused_update=True, env=dict(problem="gtg", mission=5, size=6, num_objects=2))
    before = {}

    class Cb:
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
    sd = pol.optimizer.state_dict()["state"]
    assert len(sd) == 25 and all(int(s["step"]) == 2 * 2 * 5 for s in sd.values())
    eng.poll_error()
