"""mgx/imitation.py and ExpertActor without a GPU: argument checks, the sample bookkeeping of Demonstrations, and
bc_loss's formula and masking over a stand-in evaluator (the device paths: tests/test_imitation_gpu.py)."""
import types

import pytest

torch = pytest.importorskip("torch")

from mgx import BCTrainer, Demonstrations, ExpertActor, bc_loss, collect_demonstrations  # noqa: E402


class _Buf:
    """The two things Demonstrations asks of a CompactBuffer."""

    def __init__(self, n, h, engine=None):
        self.N, self.H, self.engine = n, h, engine

    def index(self, t, env):
        return (self.H + t) * self.N + env


class _Evaluator:
    """evaluate_actions from a table of logits per flat buffer index."""

    def __init__(self, logits):
        self.logits, self.calls = logits, []

    def evaluate_actions(self, buf, index, actions):
        self.calls.append(index.clone())
        dist = torch.distributions.Categorical(logits=self.logits[index])
        return torch.zeros(index.numel()), dist.log_prob(actions), dist.entropy()


def _demo(T=3, N=5, H=2):
    g = torch.Generator().manual_seed(0)
    labels = torch.randint(0, 7, (T, N), generator=g)
    cost = torch.randint(1, 9, (T, N), generator=g).to(torch.int32)
    cost[0, 1], cost[1, 2], cost[2, 4], cost[2, 0] = -4, -1, -4, -3
    return Demonstrations(_Buf(N, H), labels, cost, labels)


def test_demonstrations_bookkeeping():
    d = _demo()
    assert (d.T, d.N) == (3, 5)
    v = d.valid()
    assert v.dtype == torch.bool and v.numel() == 15 and int(v.sum()) == 12
    assert not v[1] and not v[7] and not v[14] and v[10]          # -3 (the key routine) is a label like any other
    idx = torch.tensor([0, 4, 5, 14])
    assert d.buffer_index(idx).tolist() == [10, 14, 15, 24]        # (H + t) * N + env


def test_bc_loss_formula_and_mask():
    d = _demo()
    logits = torch.randn((25, 7), generator=torch.Generator().manual_seed(1), requires_grad=True)
    ev = _Evaluator(logits)
    index = torch.arange(15)
    loss = bc_loss(ev, d, index, ent_weight=0.25)
    keep = index[d.valid()]
    assert ev.calls[0].tolist() == (keep + 10).tolist()            # only samples with a label reach the evaluator
    lp = torch.log_softmax(logits[keep + 10], 1)
    want = -lp.gather(1, d.labels.reshape(-1)[keep][:, None]).mean() - 0.25 * (-(lp.exp() * lp).sum(1)).mean()
    assert torch.allclose(loss, want, atol=1e-6)
    loss.backward()
    assert float(logits.grad[keep + 10].abs().sum()) > 0
    assert float(logits.grad[torch.tensor([11, 17, 24])].abs().sum()) == 0
    with pytest.raises(ValueError, match="no sample"):
        bc_loss(ev, d, torch.tensor([1, 7, 14]))


def test_argument_checks():
    eng, other = types.SimpleNamespace(n=4, device="cpu"), types.SimpleNamespace(n=4, device="cpu")
    expert = types.SimpleNamespace(engine=eng)
    with pytest.raises(ValueError, match="expert belongs to another engine"):
        collect_demonstrations(other, expert, 4)
    with pytest.raises(ValueError, match="learner belongs to another engine"):
        collect_demonstrations(eng, expert, 4, learner=types.SimpleNamespace(engine=other))
    with pytest.raises(ValueError, match="T must be"):
        collect_demonstrations(eng, expert, 0)
    with pytest.raises(ValueError, match="batch_size"):
        BCTrainer(None, eng, batch_size=0)


def test_expert_actor_refuses_observations():
    x = ExpertActor(types.SimpleNamespace(n=4, device="cpu"))
    assert x.policy is x and x.sync() is None and x.last_cost.dtype == torch.int32
    with pytest.raises(TypeError, match="engine's state, not an observation"):
        x.predict({"image": None})
    with pytest.raises(ValueError, match="another engine"):
        x.act(_Buf(4, 0, engine=object()), 0)
    with pytest.raises(ValueError, match="no values"):
        x._run(_Buf(4, 0, engine=x.engine), torch.arange(4), 0)
