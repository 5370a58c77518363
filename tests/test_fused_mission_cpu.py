"""Fused mission encoder (mgx_mission_forward / mgx_mission_backward, added within ABI 9): everything that can be
checked without a GPU -- the workspace size, the argument checks, the exports and the Python-side validation."""
import ctypes

import pytest
import torch

import mission_ref as R
from mgx import _lib
from mgx.policy import DEFAULT_ARCH, ActorCriticPolicy

NEW = ("mgx_mission_workspace_words", "mgx_mission_forward", "mgx_mission_backward")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_exports_and_abi_version(lib):
    assert _lib.ABI_VERSION == 9 and lib.mgx_abi_version() == 9
    for name in NEW:
        assert name in _lib.EXPORTS and getattr(lib, name) is not None


def test_workspace_words(lib):
    """-1 for n_rows 0 and 2049 and for seq_len 0 and 257; positive otherwise and non-decreasing in both arguments;
    at least the five 128-float records per (row, t) the backward needs."""
    f = lib.mgx_mission_workspace_words
    for n, t in ((0, 128), (2049, 128), (-1, 128), (76, 0), (76, 257), (76, -3)):
        assert int(f(n, t)) == -1, (n, t)
    rows = (1, 2, 3, 4, 5, 76, 77, 255, 256, 257, 1024, 2047, 2048)
    seqs = (1, 2, 31, 32, 33, 128, 255, 256)
    for t in seqs:
        prev = 0
        for n in rows:
            w = int(f(n, t))
            assert w >= prev and w >= 5 * 128 * n * t > 0, (n, t, w)
            prev = w
    for n in rows:
        prev = 0
        for t in seqs:
            w = int(f(n, t))
            assert w >= prev > -1, (n, t, w)
            prev = w


# ---------------------------------------------------------------------------------------- the chunk plan
SWEEP_ROWS = (1, 2, 3, 4, 5, 6, 7, 8, 65, 76, 257, 1024, 1900, 2047, 2048)


def test_chunk_plan_matches_the_library_and_partitions_the_pairs(lib):
    """mission_ref.chunk_plan against the library for every seq_len in 1..256 and a spread of n_rows, through the one
    value the host exposes: mgx_mission_workspace_words = pairs * 640 + chunks * MS_SLAB + 32 * 384.  Over the same
    sweep, what mgx_mission_wgrad_kernel relies on: L even and nsteps = L / 2, so every fetched operand 2 kk + h lies
    inside its chunk; chunks * L >= pairs; every pair in exactly one chunk [s L, min(K, (s + 1) L)); the used chunks
    come first and none of them is empty; k0 + L stays far inside an int."""
    f = lib.mgx_mission_workspace_words
    assert R.MS_SLAB == 384 * 128 + 32 * 384 + 128
    for T in range(1, R.MS_MAX_SEQ + 1):
        for n in SWEEP_ROWS:
            chunks, L, nsteps, used, empty, half = R.chunk_plan(n, T)
            K = n * T
            rest = int(f(n, T)) - K * 640 - 32 * 384
            assert rest == chunks * R.MS_SLAB and rest % R.MS_SLAB == 0, (n, T, rest, chunks)
            assert int(f(n, T)) == R.workspace_words(n, T)
            assert 1 <= chunks <= R.MS_MAX_CHUNKS and L % 2 == 0 and 2 * nsteps == L, (n, T)   # so 2 kk + h < L
            assert chunks * L >= K and (L <= R.MS_KCHUNK or chunks == R.MS_MAX_CHUNKS), (n, T)
            assert chunks * L + L < 2 ** 31
            starts, ends, live = [], [], 0
            for s in range(chunks):
                k0, k1 = s * L, min(K, (s + 1) * L)
                if k0 < K:
                    assert live == s and k1 > k0                       # used chunks first, none of them empty
                    live += 1
                    starts.append(k0)
                    ends.append(k1)
            assert live == used and empty == chunks - used and used >= 1, (n, T)
            cover = torch.bincount(torch.tensor(starts), minlength=K + 1) \
                - torch.bincount(torch.tensor(ends), minlength=K + 1)      # +1 where a chunk starts, -1 where it ends
            assert bool((torch.cumsum(cover, 0)[:K] == 1).all()), (n, T)
            assert half == ((K - (used - 1) * L) % 2 == 1), (n, T)


def test_plan_shapes_cover_every_class():
    """The shapes the GPU parity tests add (mission_ref.PLAN_SHAPES), by their derived plans, reach every path of
    the weight-gradient kernels that the earlier shapes (L in 32, 48, 64; at most 152 chunks) never did."""
    plans = {s: R.chunk_plan(*s) for s in R.PLAN_SHAPES}
    for s, p in plans.items():
        print(s, "pairs %d chunks %d L %d nsteps %d used %d empty %d half %s" % ((s[0] * s[1],) + p))
        assert 1 <= s[0] <= R.MS_MAX_ROWS and 1 <= s[1] <= R.MS_MAX_SEQ

    def some(pred):
        return [s for s, p in plans.items() if pred(s, *p)]

    assert some(lambda s, chunks, L, nsteps, used, empty, half: nsteps < 4)
    for tail in (1, 2, 3):
        assert some(lambda s, chunks, L, nsteps, used, empty, half: nsteps > 4 and nsteps % 4 == tail), tail
        assert some(lambda s, chunks, L, nsteps, used, empty, half: chunks > 1 and nsteps % 4 == tail), tail
    assert some(lambda s, chunks, L, nsteps, used, empty, half: half)
    assert some(lambda s, chunks, L, nsteps, used, empty, half: half and nsteps > 4)
    assert some(lambda s, chunks, L, nsteps, used, empty, half: 1 < chunks < 8)
    assert some(lambda s, chunks, L, nsteps, used, empty, half: chunks > 8 and chunks % 8)
    assert some(lambda s, chunks, L, nsteps, used, empty, half: chunks == 256 and L > 64 and not empty)
    assert some(lambda s, chunks, L, nsteps, used, empty, half: chunks == 256 and L > 64 and empty >= 1)
    for m in (0, 1, 2):
        assert some(lambda s, *p: s[1] % 2 == 1 and s[1] > 1 and s[0] % 3 == m), m
    assert some(lambda s, *p: s[0] == 2048)
    assert some(lambda s, *p: s[1] == 1)
    assert some(lambda s, *p: s[1] == 255)
    assert some(lambda s, chunks, L, *p: s[1] > 1 and L % s[1] != 0 and chunks > 1)    # a boundary inside a row
    assert set(R.PAIR_SHAPES) <= set(R.PLAN_SHAPES)
    # the table of the shapes' plans, as derived: (chunks, L, nsteps, empty chunks)
    assert {s: (p[0], p[1], p[2], p[4]) for s, p in plans.items()} == {
        (1, 1): (1, 2, 1, 0), (2, 1): (1, 2, 1, 0), (4, 1): (1, 4, 2, 0), (3, 7): (1, 22, 11, 0),
        (4, 33): (3, 44, 22, 0), (5, 37): (3, 62, 31, 0), (4, 100): (7, 58, 29, 0), (9, 65): (10, 60, 30, 0),
        (5, 255): (20, 64, 32, 0), (1900, 9): (256, 68, 34, 4), (65, 256): (256, 66, 33, 3), (2048, 9): (256, 72, 36, 0)}


# ---------------------------------------------------------------------------------------- the explicit fp64 GRU
@pytest.fixture(scope="module")
def seq64():
    """The fp64 Embedding + GRU of test_fused_mission_gpu._ctx: the one redrawn policy (mission_ref.redrawn_policy)."""
    import copy
    return copy.deepcopy(R.redrawn_policy().features_extractor.extractors["mission"]).double()


@pytest.mark.parametrize("n_rows,seq_len", [(2, 1), (4, 33), (5, 255)])
def test_explicit_gru_agrees_with_autograd(seq64, n_rows, seq_len):
    """mission_ref.gru_reference against fp64 nn.Embedding + nn.GRU under autograd: the features and the five
    gradients within 64 eps64 max|ref| per tensor (two fp64 evaluations that add up to 256 steps and 1,275 pairs in
    different orders).  The per-pair tensors are what the gradients were formed from: their sums are checked too."""
    tok = R.plan_tokens("random", n_rows, seq_len)
    g = R.plan_cotangent(n_rows, seq_len)
    _, h = seq64(tok.long())
    feat = h[-1]
    grads = torch.autograd.grad((feat * g.double()).sum(), list(seq64.parameters()))
    want = dict(zip(("embedding", "w_ih", "w_hh", "b_ih", "b_hh"), grads), features=feat.detach())
    ref = R.gru_reference(list(seq64.parameters()), tok, g)
    got = dict(ref.grads, features=ref.feat)
    bad = []
    for name, w in want.items():
        assert got[name].shape == w.shape and got[name].dtype == torch.float64, name
        dev = float((got[name] - w).abs().max())
        bound = 64.0 * R.EPS64 * float(w.abs().max())
        print("rows %d seq %d %s: |dev| %.3e, bound %.3e, ratio %.3f"
              % (n_rows, seq_len, name, dev, bound, dev / bound if bound else 0.0))
        if not dev <= bound:
            bad.append((name, dev, bound))
    assert not bad, bad
    assert ref.c_in.shape == ref.c_hid.shape == (n_rows, seq_len, 384) and ref.h_prev.shape == (n_rows, seq_len, 128)
    assert not ref.h_prev[:, 0].any() and (seq_len == 1 or bool(ref.h_prev[:, 1:].any()))
    assert torch.equal(ref.c_in[:, :, :256], ref.c_hid[:, :, :256])
    assert torch.equal(ref.c_in.reshape(-1, 384).sum(0), ref.grads["b_ih"])
    if seq_len == 1:
        assert not want["w_hh"].any() and not ref.grads["w_hh"].any()


@pytest.mark.parametrize("n_rows,seq_len", R.PAIR_SHAPES)
def test_every_pair_is_visible_in_the_pair_shapes_inputs(seq64, n_rows, seq_len):
    """The condition test_fused_mission_gpu.test_single_pair_would_be_seen puts on its inputs, with the floor
    4 eps32 max|gradient| in place of the measured bound: every pair's own contribution to db_ih, and for t > 0 to
    dW_hh, has an entry at least 16 times the floor (the GPU test needs 2 times the bound; the bound is the floor
    or 4 e_torch)."""
    ref = R.gru_reference(list(seq64.parameters()), R.plan_tokens("random", n_rows, seq_len),
                          R.plan_cotangent(n_rows, seq_len))
    ratios = R.pair_floor_ratios(ref)
    assert set(ratios) == {"b_ih", "w_hh"}
    for name, (small, floor) in ratios.items():
        print("rows %d seq %d %s: smallest pair contribution %.3e, floor %.3e, factor %.1f"
              % (n_rows, seq_len, name, small, floor, small / floor))
        assert small >= 16.0 * floor, (name, small, floor)


def test_long_sequences_hide_pairs_which_is_why_9_65_is_not_a_pair_shape(seq64):
    """The reason mission_ref.PAIR_SHAPES leaves (9, 65) out, computed: over 64 steps the cotangent decays until the
    smallest pair's contribution to db_ih is less than 16 times the floor (5.5 times, with these seeds)."""
    assert (9, 65) in R.PLAN_SHAPES and (9, 65) not in R.PAIR_SHAPES
    ref = R.gru_reference(list(seq64.parameters()), R.plan_tokens("random", 9, 65), R.plan_cotangent(9, 65))
    small, floor = R.pair_floor_ratios(ref)["b_ih"]
    print("rows 9 seq 65 b_ih: smallest pair contribution %.3e, floor %.3e, factor %.1f" % (small, floor, small / floor))
    assert small < 16.0 * floor


def _structs():
    p = _lib.MgxMissionParams(embedding_dev=0x1000, w_ih_dev=0x1000, w_hh_dev=0x1000, b_ih_dev=0x1000, b_hh_dev=0x1000)
    g = _lib.MgxMissionGrads(embedding_dev=0x1000, w_ih_dev=0x1000, w_hh_dev=0x1000, b_ih_dev=0x1000, b_hh_dev=0x1000)
    return p, g


FIELDS = ("embedding_dev", "w_ih_dev", "w_hh_dev", "b_ih_dev", "b_hh_dev")


def test_forward_rejects_bad_arguments_without_gpu(lib):
    """Every bad-argument case returns MGX_ERR_INVALID before any HIP call and before any pointer is dereferenced
    (the pointers are fake)."""
    d = ctypes.c_void_p(0x1000)
    need = int(lib.mgx_mission_workspace_words(76, 128))

    def call(tokens=d, n=76, t=128, p="ok", feat=d, ws=d, words=need, null=None):
        pp, _ = _structs()
        if null:
            setattr(pp, null, None)
        return lib.mgx_mission_forward(tokens, n, t, None if p is None else ctypes.byref(pp), feat, ws, words, None)

    cases = [dict(tokens=None), dict(feat=None), dict(p=None)]
    cases += [dict(null=name) for name in FIELDS]
    cases += [dict(n=0), dict(n=2049), dict(n=-1), dict(t=0), dict(t=257), dict(words=need - 1), dict(words=0),
              dict(words=-1), dict(ws=None, n=0), dict(ws=None, t=257)]
    for i, kw in enumerate(cases):
        st = call(**kw)
        assert st == 1, (i, kw, st)                  # MGX_ERR_INVALID
        assert b"mgx_mission_forward" in lib.mgx_last_error()


def test_backward_rejects_bad_arguments_without_gpu(lib):
    d = ctypes.c_void_p(0x1000)
    need = int(lib.mgx_mission_workspace_words(76, 128))

    def call(tokens=d, n=76, t=128, p="ok", gf=d, ws=d, words=need, g="ok", null_p=None, null_g=None):
        pp, gg = _structs()
        if null_p:
            setattr(pp, null_p, None)
        if null_g:
            setattr(gg, null_g, None)
        return lib.mgx_mission_backward(tokens, n, t, None if p is None else ctypes.byref(pp), gf, ws, words,
                                        None if g is None else ctypes.byref(gg), None)

    cases = [dict(tokens=None), dict(gf=None), dict(ws=None), dict(p=None), dict(g=None)]
    cases += [dict(null_p=name) for name in FIELDS] + [dict(null_g=name) for name in FIELDS]
    cases += [dict(n=0), dict(n=2049), dict(n=-1), dict(t=0), dict(t=257), dict(words=need - 1), dict(words=0),
              dict(words=-1)]
    for i, kw in enumerate(cases):
        st = call(**kw)
        assert st == 1, (i, kw, st)                  # MGX_ERR_INVALID
        assert b"mgx_mission_backward" in lib.mgx_last_error()


def test_fused_mission_needs_a_fused_path():
    from mgx.ppo import PPOConfig
    assert PPOConfig().fused_mission is False
    with pytest.raises(ValueError):
        PPOConfig(fused_mission=True)
    PPOConfig(fused_mission=True, fused_train=True)
    PPOConfig(fused_mission=True, fused_act=True)


def test_encoder_rejects_other_architectures():
    """A GRU with another hidden size (and an Embedding of another width) is the ValueError of FusedActor, before
    anything touches a device; the reference architecture is accepted."""
    from mgx.fused_mission import FusedMissionEncoder, mission_params
    for mission in ([["Embedding", [32, 32]], ["GRU", [32, 64, 1, True, True]]],
                    [["Embedding", [32, 16]], ["GRU", [16, 128, 1, True, True]]],
                    [["Embedding", [40, 32]], ["GRU", [32, 128, 1, True, True]]]):
        pol = ActorCriticPolicy(n_stack=2, arch=dict(DEFAULT_ARCH, mission=mission))
        with pytest.raises(ValueError, match="reference architecture"):
            FusedMissionEncoder(pol, "cpu")
    pol = ActorCriticPolicy(n_stack=2)
    enc = FusedMissionEncoder(pol, "cpu")
    shapes = [tuple(t.shape) for t in mission_params(pol)]
    assert shapes == [(32, 32), (384, 32), (384, 128), (384,), (384,)]
    with pytest.raises(ValueError):
        enc.encode(torch.zeros((3, 64), dtype=torch.int64))             # tokens are u8


def test_flag_off_keeps_the_token_stacks_and_the_table(lib):
    """FusedEvaluator without fused_mission holds the i64 stacks and no encoder, with it the same stacks as u8."""
    from mgx import fused_train as ft

    class Eng:
        L, n, n_stack, device = lib, 7, 2, torch.device("cpu")

    pol = ActorCriticPolicy(n_stack=2)
    off, on = ft.FusedEvaluator(pol, Eng), ft.FusedEvaluator(pol, Eng, fused_mission=True)
    assert off.mission is None and off._stacks_all.dtype == torch.int64
    assert on.mission is not None and on._stacks_all.dtype == torch.uint8
    assert torch.equal(off._stacks_all, on._stacks_all.to(torch.int64))
