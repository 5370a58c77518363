"""The two helpers the shared step bodies rest on, without a GPU: _lib.check_tensor (the one tensor check of every
library-call wrapper) and ppo.minibatch_env_t (the permutation slicing of the three minibatch iterators)."""
import pytest

torch = pytest.importorskip("torch")

from mgx import _lib  # noqa: E402
from mgx.ppo import CompactRollout, RolloutBuffer, minibatch_env_t  # noqa: E402


def test_check_tensor_accepts_and_returns_the_tensor():
    t = torch.zeros((3, 4), dtype=torch.float32)
    assert _lib.check_tensor(t, "t", torch.float32, 12) is t
    assert _lib.check_tensor(t, "t", torch.float32, 12, torch.device("cpu")) is t
    assert _lib.check_tensor(t, "t", torch.float32, 12, "cpu") is t
    row = t[1]                                       # a contiguous view
    assert _lib.check_tensor(row, "row", torch.float32, 4) is row


@pytest.mark.parametrize("case", ["dtype", "count", "contiguity", "device"])
def test_check_tensor_rejects(case):
    """Each of the four properties on its own; the message names the argument, the dtype, the count and the device."""
    t = torch.zeros((6, 4), dtype=torch.float32)
    bad = dict(dtype=(t.to(torch.float64), None), count=(t[:5], None), contiguity=(t.t(), None),
               device=(t, torch.device("cuda:0")))[case]
    if case == "contiguity":
        assert bad[0].numel() == 24 and not bad[0].is_contiguous()
    with pytest.raises(ValueError) as err:
        _lib.check_tensor(bad[0], "g_logits", torch.float32, 24, bad[1])
    text = str(err.value)
    assert "g_logits" in text and "torch.float32" in text and "24" in text
    if case == "device":
        assert "cuda:0" in text
    _lib.check_tensor(t, "g_logits", torch.float32, 24, torch.device("cpu"))


def test_check_tensor_missing_tensor_and_any_length():
    """A missing tensor is a ValueError that names the argument, not an AttributeError; numel None checks no count and
    promises none in the message."""
    with pytest.raises(ValueError, match="log_probs"):
        _lib.check_tensor(None, "log_probs", torch.float32, 8)
    t = torch.zeros(5, dtype=torch.float32)
    assert _lib.check_tensor(t, "returns", torch.float32, None) is t
    with pytest.raises(ValueError) as err:
        _lib.check_tensor(t.to(torch.int64), "returns", torch.float32, None)
    assert "returns" in str(err.value) and "elements" not in str(err.value)


def _pairs_by_hand(perm, batch_size, T):
    """The slicing each of the three iterators held before: idx = perm[s:s + batch_size]; env, t = idx // T, idx % T."""
    out = []
    for s in range(0, perm.numel(), batch_size):
        idx = perm[s:s + batch_size]
        out.append((idx // T, idx % T))
    return out


class _Buf:
    """Stands in for a CompactBuffer: index() and gather() hand back what they were asked for."""

    def index(self, t, env):
        return ("index", t, env)

    def gather(self, index, f32=False):
        return index


def test_minibatch_env_t_equals_the_three_iterators():
    """T = 5, N = 7: 35 samples in minibatches of 8 -> 8, 8, 8, 8, 3.  The helper's (env, t) are the hand slicing's, and
    RolloutBuffer.minibatches, CompactRollout.minibatches and CompactRollout.minibatch_indices each read exactly those
    elements."""
    T, N, bs = 5, 7, 8
    perm = torch.randperm(T * N, generator=torch.Generator().manual_seed(3))
    want = _pairs_by_hand(perm, bs, T)
    got = list(minibatch_env_t(perm, bs, T))
    assert [e.numel() for e, _ in got] == [8, 8, 8, 8, 3]
    assert len(got) == len(want)
    for (e, t), (we, wt) in zip(got, want):
        assert torch.equal(e, we) and torch.equal(t, wt)
    assert torch.equal(torch.cat([e * T + t for e, t in got]), perm)
    tag = torch.arange(T * N, dtype=torch.float32).view(T, N)          # element [t, env] names itself

    rb = RolloutBuffer(T, N, 1, "cpu")
    rb.values.copy_(tag)
    rb.log_probs.copy_(tag)
    rb.actions.copy_(tag.to(torch.int64))
    rb.advantages, rb.returns = tag.clone(), tag.clone()
    batches = list(rb.minibatches(bs, perm))
    assert len(batches) == len(want)
    for (obs, *arrays), (we, wt) in zip(batches, want):
        assert obs["image"].shape[0] == we.numel()
        for a in arrays:
            assert torch.equal(a.to(torch.float32), tag[wt, we])

    ro = CompactRollout.__new__(CompactRollout)                         # no engine: only the arrays and the slicing
    ro.T, ro.N, ro.buf = T, N, _Buf()
    ro.actions = tag.to(torch.int64)
    ro.values = ro.log_probs = ro.advantages = ro.returns = tag
    for it in (ro.minibatches, ro.minibatch_indices):
        batches = list(it(bs, perm))
        assert len(batches) == len(want)
        for (obs, *arrays), (we, wt) in zip(batches, want):
            kind, t, e = obs
            assert kind == "index" and torch.equal(t, wt) and torch.equal(e, we)
            for a in arrays:
                assert torch.equal(a.to(torch.float32), tag[wt, we])
