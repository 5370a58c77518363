"""Behaviour cloning from the device expert on the GPU (mgx/imitation.py): the labels collect_demonstrations stores,
bc_loss through FusedEvaluator against the module, and BCTrainer on one fixed batch.

Loss and gradients (gtg 8x8, n_stack 1 and 4, 64 envs x 8 expert-played steps, 256 of the 512 samples): reference =
the fp64 CPU deep copy of the module on buf.gather of the same samples; yardstick, measured in the same run, e_torch
= |torch fp32 GPU module - fp64|; the fused path may deviate from fp64 by at most max(4 e_torch, 4 eps32 max|ref|),
the project's rule (tests/test_fused_train_gpu.py, whose policy, module evaluators and pool-tie filter are used
here).  bc_loss does not touch the value head: its parameters' gradients are exactly zero on every path."""
import copy

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import test_fused_train_gpu as F  # noqa: E402

pytestmark = pytest.mark.gpu

ENV = dict(problem="gtg", mission=5, size=8, num_objects=4)
N_ENVS, T, BATCH = 64, 8, 256
_RUNS = {}


def _engine(k, **kw):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgx import MgxEngine
    return MgxEngine(n_envs=N_ENVS, n_stack=k, terminal_mode="truncated", mission_dtype=torch.uint8, **ENV, **kw)


def _run(k):
    if k in _RUNS:
        return _RUNS[k]
    from mgx import ExpertActor, collect_demonstrations
    r = F.Run()
    r.k = k
    r.eng = _engine(k)
    r.pol = F._policy(k).cuda()
    r.pol64 = copy.deepcopy(r.pol).cpu().double()
    r.expert = ExpertActor(r.eng)
    r.demo = collect_demonstrations(r.eng, r.expert, T)
    r.eng.poll_error()
    every = torch.arange(T * N_ENVS, device=r.eng.device)
    every = every[r.demo.valid()]
    obs = r.demo.buf.gather(r.demo.buffer_index(every).contiguous(), f32=False)
    keep = every[~F._ambiguous_pool(r.pol64, obs).to(every.device)]
    assert keep.numel() >= BATCH
    perm = torch.randperm(keep.numel(), generator=torch.Generator().manual_seed(11))[:BATCH]
    r.index = keep[perm.to(keep.device)].sort().values.contiguous()
    r.obs = {kk: v.clone() for kk, v in r.demo.buf.gather(r.demo.buffer_index(r.index).contiguous(), f32=False).items()}
    r.labels = r.demo.labels.reshape(-1)[r.index]
    _RUNS[k] = r
    return r


def _bc(labels, ent_weight):
    def loss(values, log_prob, entropy):
        return -log_prob.mean() - ent_weight * entropy.mean()
    return loss


def _grads(pol, outs, obs, labels, loss):
    """(loss, {name: grad (f64, CPU)}); parameters the loss does not reach (the value head) get zeros."""
    names, ps = zip(*pol.named_parameters())
    val = loss(*F._via(outs, labels)(pol, obs))
    gs = torch.autograd.grad(val, ps, allow_unused=True)
    return float(val.detach().double()), {n: (torch.zeros_like(p) if g is None else g).detach().double().cpu()
                                          for n, p, g in zip(names, ps, gs)}


def test_labels_are_the_actions_stepped():
    """learner=None: the stored labels are the actions the buffer stepped -- a second engine of equal seed, stepped
    with them, reproduces the buffer's rows, dones and rewards, and an expert-only pass over it gives them back."""
    from mgx import ExpertActor
    from mgx.compact import CompactBuffer
    r = _run(4)
    d = r.demo
    assert d.actions is d.labels and tuple(d.labels.shape) == (T, N_ENVS) and d.cost.dtype == torch.int32
    e2 = _engine(4)
    x2 = ExpertActor(e2)
    e2.reset()
    b2 = CompactBuffer(e2, T)
    b2.observe(0)
    for t in range(T):
        assert torch.equal(x2.expert_act(), d.labels[t]), t
        assert torch.equal(x2.last_cost, d.cost[t]), t
        b2.step(t, d.labels[t])
    e2.poll_error()
    assert torch.equal(b2.rows, d.buf.rows) and torch.equal(b2.starts, d.buf.starts)
    assert torch.equal(b2.rewards, d.buf.rewards)
    assert int(d.buf.dones.sum()) > 0 and int((d.cost > 0).sum()) > T * N_ENVS // 2


def test_dagger_labels():
    """With a learner the learner's actions are played and the expert labels the states it reaches: equal to an
    expert-only pass over a second engine driven by the same actions."""
    from mgx import ExpertActor, collect_demonstrations
    from mgx.compact import CompactBuffer
    from mgx.fused_policy import FusedActor
    r = _run(4)
    eng = _engine(4)
    learner = FusedActor(r.pol, eng, seed=3)
    d = collect_demonstrations(eng, ExpertActor(eng), T, learner=learner)
    eng.poll_error()
    assert d.actions is not d.labels and int((d.actions != d.labels).sum()) > 0
    e2 = _engine(4)
    x2 = ExpertActor(e2)
    e2.reset()
    b2 = CompactBuffer(e2, T)
    b2.observe(0)
    for t in range(T):
        assert torch.equal(x2.expert_act(), d.labels[t]), t
        b2.step(t, d.actions[t])
    e2.poll_error()
    assert torch.equal(b2.rows, d.buf.rows)
    with pytest.raises(ValueError, match="another engine"):
        collect_demonstrations(e2, ExpertActor(e2), T, learner=learner)


@pytest.mark.parametrize("k", [1, 4])
def test_bc_loss_and_gradients(k):
    from mgx import bc_loss
    from mgx.fused_train import FusedEvaluator
    r = _run(k)
    ent_weight = 1e-3
    loss = _bc(r.labels, ent_weight)
    l64, ref = _grads(r.pol64, F._out64, r.obs, r.labels.cpu(), loss)
    l32, t32 = _grads(r.pol, F._out32, r.obs, r.labels, loss)
    ev = FusedEvaluator(r.pol, r.eng)
    for p in r.pol.parameters():
        p.grad = None
    got_loss = bc_loss(ev, r.demo, r.index, ent_weight)
    got_loss.backward()
    got = {n: (torch.zeros_like(p) if p.grad is None else p.grad).double().cpu() for n, p in r.pol.named_parameters()}
    for p in r.pol.parameters():
        p.grad = None
    lg = float(got_loss.detach().double())
    bound = max(4.0 * abs(l32 - l64), 4.0 * F.EPS32 * abs(l64))
    print("n_stack %d loss: fp64 %.9f, torch fp32 dev %.3e, fused dev %.3e, bound %.3e"
          % (k, l64, abs(l32 - l64), abs(lg - l64), bound))
    assert abs(lg - l64) <= bound
    bad, reached = [], 0
    for n in ref:
        e_torch = float((t32[n] - ref[n]).abs().max())
        b = max(4.0 * e_torch, 4.0 * F.EPS32 * float(ref[n].abs().max()))
        dev = float((got[n] - ref[n]).abs().max())
        print("n_stack %d %s: fused max |dev| %.3e, torch fp32 %.3e, bound %.3e" % (k, n, dev, e_torch, b))
        reached += float(ref[n].abs().max()) > 0
        if not dev <= b:
            bad.append((n, dev, b))
    assert not bad, bad
    assert len(ref) == 25 and reached == 19          # all but value_net_body (4 tensors) and value_net (2)
    r.eng.poll_error()


def test_masked_samples_are_left_out():
    """Samples whose cost is -4 or -1 do not enter the loss: marking some of the batch changes it to the loss of
    the rest."""
    from mgx import bc_loss
    from mgx.fused_train import FusedEvaluator
    from mgx.imitation import Demonstrations
    r = _run(4)
    ev = FusedEvaluator(r.pol, r.eng)
    cost = r.demo.cost.clone()
    flat = cost.reshape(-1)
    flat[r.index[:40]] = -4
    flat[r.index[40:64]] = -1
    d2 = Demonstrations(r.demo.buf, r.demo.labels, cost, r.demo.actions)
    with torch.no_grad():
        a = float(bc_loss(ev, d2, r.index))
        b = float(bc_loss(ev, r.demo, r.index[64:]))
        with pytest.raises(ValueError, match="no sample"):
            bc_loss(ev, d2, r.index[:64])
    assert a == b


def test_trainer_fits_one_batch():
    """50 Adam steps on one fixed batch of 256 samples: the loss falls and the label accuracy does not."""
    from mgx import BCTrainer
    r = _run(4)
    pol = copy.deepcopy(r.pol)
    tr = BCTrainer(pol, r.eng, batch_size=BATCH)
    before, acc0 = tr.loss(r.demo, r.index), tr.accuracy(r.demo, r.index)
    losses = tr.train(r.demo, 50, index=r.index)
    after, acc1 = tr.loss(r.demo, r.index), tr.accuracy(r.demo, r.index)
    print("BC on one batch: loss %.4f -> %.4f, accuracy %.3f -> %.3f" % (before, after, acc0, acc1))
    assert len(losses) == 50 and all(np.isfinite(losses))
    assert after < before and acc1 >= acc0
    r.eng.poll_error()
