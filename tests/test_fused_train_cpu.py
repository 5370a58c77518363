"""Fused policy gradient (mgx_policy_backward, ABI 9): everything that can be checked without a GPU -- the scratch
size, the argument checks, and the two differentiable inputs of the autograd function (mgx/fused_train.py)."""
import ctypes

import pytest
import torch

from mgx import _lib
from mgx import fused_policy as fp
from mgx import fused_train as ft
from mgx.policy import ActorCriticPolicy


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_abi_version_and_exports(lib):
    assert _lib.ABI_VERSION == 9 and lib.mgx_abi_version() == 9
    assert "mgx_policy_backward" in _lib.EXPORTS and "mgx_policy_grad_scratch_words" in _lib.EXPORTS


def test_scratch_words(lib):
    """-1 for n_stack 0 and 9, n_samples 0, max_groups -1; else groups x blob words with groups = min(max_groups or
    the default of 256, tiles): positive, non-decreasing in max_groups, and 0 means the default."""
    f = lib.mgx_policy_grad_scratch_words
    for k, n, g in ((0, 100, 2), (9, 100, 2), (4, 0, 2), (4, -5, 0), (4, 100, -1)):
        assert int(f(k, n, g)) == -1
    for k in (1, 4, 8):
        words = int(lib.mgx_policy_blob_words(k))
        for n in (1, 64, 65, 210, 65536):
            tiles = (n + 63) // 64
            prev = 0
            for g in range(1, 300):
                w = int(f(k, n, g))
                assert w == min(g, tiles) * words and w >= prev > -1
                prev = w
            assert int(f(k, n, 0)) == min(256, tiles) * words


def test_policy_backward_rejects_bad_arguments_without_gpu(lib):
    """Every bad-argument case that needs no live handle returns MGX_ERR_INVALID before any HIP call and before
    any pointer is dereferenced (0 < ring_rows < n_stack and a short scratch read the handle's n_stack:
    tests/test_fused_train_gpu.py)."""
    d = ctypes.c_void_p(0x1000)

    def grad(**kw):
        g = _lib.MgxPolicyGrad(blob_dev=0x1000, mission_feat_dev=0x1000, g_logits_dev=0x1000, g_values_dev=0x1000,
                               grad_blob_dev=0x1000, grad_mission_feat_dev=0x1000, scratch_dev=0x1000,
                               scratch_words=1 << 40, max_groups=0)
        for k, v in kw.items():
            setattr(g, k, v)
        return g

    def call(g, n=16, h=d, rows=d, mids=d, starts=d, index=d, n_envs=64, ring=0):
        return lib.mgx_policy_backward(h, rows, mids, starts, n_envs, ring, index, n,
                                       None if g is None else ctypes.byref(g), None)

    cases = [dict(g=None)]
    cases += [dict(g=grad(**{name: None})) for name in ("blob_dev", "mission_feat_dev", "g_logits_dev", "g_values_dev",
                                                       "grad_blob_dev", "grad_mission_feat_dev", "scratch_dev")]
    cases += [dict(g=grad(), n=0), dict(g=grad(), n=-3), dict(g=grad(max_groups=-1)),
              dict(g=grad(scratch_words=0)), dict(g=grad(scratch_words=-1)),
              dict(g=grad(), h=None), dict(g=grad(), rows=None), dict(g=grad(), mids=None),
              dict(g=grad(), starts=None), dict(g=grad(), index=None)]
    for i, kw in enumerate(cases):
        st = call(**kw)
        assert st == 1, (i, st)                      # MGX_ERR_INVALID
        assert b"mgx_policy_backward" in lib.mgx_last_error()


@pytest.mark.parametrize("k", [1, 4, 8])
def test_blob_round_trip(k):
    """A random grad_blob back-propagated through the differentiable torch.cat lands in every parameter's .grad as
    the matching slice, bit for bit."""
    torch.manual_seed(k)
    pol = ActorCriticPolicy(n_stack=k)
    _, tensors = fp._params(pol)
    blob = ft.differentiable_blob(tensors)
    assert blob.requires_grad and blob.numel() == fp.blob_words(k)
    assert torch.equal(blob.detach(), fp.pack_blob(pol))
    g = torch.randn(blob.numel(), generator=torch.Generator().manual_seed(3))
    blob.backward(g)
    offs = fp.blob_offsets(k)
    assert len(tensors) == len(offs) == 20
    for t, (name, (o, shape)) in zip(tensors, offs.items()):
        assert t.grad is not None and tuple(t.grad.shape) == shape
        assert torch.equal(t.grad, g[o:o + t.numel()].reshape(shape)), name
    fe = pol.features_extractor.extractors["mission"]
    assert all(p.grad is None for p in fe.parameters())      # the blob holds no Embedding / GRU weight


def test_differentiable_table():
    """n_stack 2: d/dtheta sum(table * R), R non-zero on three (mid, v) rows, equals the extractor's own gradient
    on the three stacked token rows within 4 eps32 max|ref|, for the Embedding and the four GRU tensors; the table's
    values are mission_table's on those rows and zero elsewhere."""
    k = 2
    torch.manual_seed(11)
    pol = ActorCriticPolicy(n_stack=k)
    pol.train(False)
    keys = [(3, 1), (2 | (5 << 2) | (3 << 5), 2), (128, 2)]            # (mission id, v)
    rows = torch.tensor([mid * k + v - 1 for mid, v in keys])
    stacks_all = fp.mission_token_stacks(k).reshape(256 * k, 32 * k)
    stacks = stacks_all.index_select(0, rows)
    R = torch.zeros((256, k, 128))
    gen = torch.Generator().manual_seed(5)
    for mid, v in keys:
        R[mid, v - 1] = torch.randn(128, generator=gen)
    fe = pol.features_extractor
    params = dict(fe.extractors["mission"].named_parameters())
    assert len(params) == 5
    tab = ft.mission_table_rows(pol, rows, stacks)
    assert tab.shape == (256, k, 128) and tab.requires_grad
    full = fp.mission_table(pol)
    mask = torch.zeros(256 * k, dtype=torch.bool)
    mask[rows] = True
    assert torch.allclose(tab.detach().reshape(-1, 128)[mask], full.reshape(-1, 128)[mask], rtol=0,
                          atol=4 * torch.finfo(torch.float32).eps)
    assert not tab.detach().reshape(-1, 128)[~mask].any()
    got = torch.autograd.grad((tab * R).sum(), list(params.values()))
    obs = {"image": torch.zeros((3, 3 * k, 7, 7)), "direction": torch.zeros((3, 4 * k)), "mission": stacks}
    feat = fe(obs)[:, 80:]
    Rr = torch.stack([R[mid, v - 1] for mid, v in keys])
    want = torch.autograd.grad((feat * Rr).sum(), list(params.values()))
    eps = float(torch.finfo(torch.float32).eps)
    for name, a, b in zip(params, got, want):
        bound = 4 * eps * float(b.abs().max())
        dev = float((a - b).abs().max())
        print("%s: max |dev| %.3e, bound %.3e" % (name, dev, bound))
        assert float(b.abs().max()) > 0 and dev <= bound, name


class _HostEngine:
    """What FusedEvaluator.prepare / inputs and CompactRollout read of an engine, on the CPU."""

    def __init__(self, lib, n_envs, n_stack):
        self.L, self.n, self.n_stack, self.device = lib, n_envs, n_stack, torch.device("cpu")


def test_table_rows_of_mixed_mission_ids(lib):
    """n_stack 4, a buffer whose mission ids are 3, 37, 128, 132 and 255 (below and above 128, the last one unused:
    32 zero tokens): FusedEvaluator.prepare + inputs give fused_policy.mission_table on the rows mid * 4 + v - 1 of
    those ids at every v (within 4 eps32: the GRU runs on another batch) and exact zeros on the other 1,004 rows; the
    gradient of a cotangent that is non-zero on every row reaches only those 20 rows: the Embedding weight's
    gradient is non-zero on exactly the tokens those missions hold (0, the padding, among them)."""
    k = 4
    ids = [3, 37, 128, 132, 255]
    torch.manual_seed(13)
    pol = ActorCriticPolicy(n_stack=k)
    pol.train(False)
    ev = ft.FusedEvaluator(pol, _HostEngine(lib, 7, k))

    class Buf:
        mids = torch.tensor(ids * 3 + [37, 3], dtype=torch.uint8).reshape(1, 17)

    ev.prepare(Buf)
    blob, tab = ev.inputs()
    assert tab.shape == (256, k, 128) and tab.requires_grad and blob.numel() == fp.blob_words(k)
    full = fp.mission_table(pol)
    mask = torch.zeros((256, k), dtype=torch.bool)
    mask[ids] = True
    assert float(full[mask].abs().max()) > 0.1
    assert torch.allclose(tab.detach()[mask], full[mask], rtol=0, atol=4 * torch.finfo(torch.float32).eps)
    assert not tab.detach()[~mask].any()
    # rows of two ids differ by far more than that tolerance (the v rows of one id do not: after the mission's 32
    # tokens the GRU has all but forgotten the zero frames before them; the exact zeros pin those)
    rows = full[ids, k - 1]
    assert float(torch.cdist(rows, rows).fill_diagonal_(1.0).min()) > 1e-5
    R = torch.randn((256, k, 128), generator=torch.Generator().manual_seed(9))
    emb = pol.features_extractor.extractors["mission"][0].weight
    g = torch.autograd.grad((tab * R).sum(), emb)[0]
    tokens = torch.as_tensor(_lib.mission_tokens()).long()
    held = torch.zeros(32, dtype=torch.bool)
    held[tokens[ids].reshape(-1)] = True
    held[0] = True
    assert 3 < int(held.sum()) < 32
    assert g.shape == (32, 32) and not g[~held].any()
    assert all(bool(g[t].any()) for t in held.nonzero().flatten().tolist())


def test_minibatch_indices_pair_each_sample_with_its_own_row(lib):
    """CompactRollout.minibatch_indices, T = 4 and N = 5 in the third ring block: flat index i of the permutation is
    (env, t) = (i // T, i % T) (SB3's env-major flatten); the yielded compact index is ((block * T + t - 1) mod R) *
    N + env and the five tensors beside it are that (t, env)'s."""
    from mgx.ppo import CompactRollout
    T, N, k = 4, 5, 4
    ro = CompactRollout(_HostEngine(lib, N, k), T)
    ro.buf.carry_over()
    ro.buf.carry_over()
    assert (ro.buf.blocks, ro.buf.R, ro.buf.block) == (2, 8, 0)
    ro.buf.carry_over()                                       # block 1: observation 0 is the last row of block 0
    tag = (100 * torch.arange(T)[:, None] + torch.arange(N)[None, :])
    ro.actions.copy_(tag)
    for j, a in enumerate((ro.values, ro.log_probs, ro.advantages, ro.returns)):
        a.copy_(tag.float() + 0.125 * (j + 1))
    perm = torch.randperm(T * N, generator=torch.Generator().manual_seed(2))
    seen = 0
    for s, out in enumerate(ro.minibatch_indices(8, perm)):
        index, actions = out[0], out[1]
        for j in range(index.numel()):
            i = int(perm[8 * s + j])
            env, t = i // T, i % T
            assert int(index[j]) == ((1 * T + t - 1) % 8) * N + env
            assert int(actions[j]) == 100 * t + env
            for q in range(4):
                assert float(out[2 + q][j]) == 100 * t + env + 0.125 * (q + 1)
            seen += 1
    assert seen == T * N


def test_fused_evaluator_rejects_other_architectures():
    """The same ValueError as FusedActor, before the engine is touched."""
    for pol in (ActorCriticPolicy(n_stack=2, net_arch={"pi": [32, 32], "vf": [64, 64]}),
                ActorCriticPolicy(n_stack=2, n_actions=6)):
        with pytest.raises(ValueError, match="reference architecture"):
            ft.FusedEvaluator(pol, None)


def test_fused_train_needs_compact_layout():
    from mgx.ppo import PPOConfig, Trainer
    pol = ActorCriticPolicy(n_stack=4)
    with pytest.raises(ValueError):
        Trainer(pol, PPOConfig(fused_train=True, layout="sb3"))
    assert PPOConfig().fused_train is False
    Trainer(pol, PPOConfig(fused_train=True))            # compact: accepted
