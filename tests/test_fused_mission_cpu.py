"""Fused mission encoder (mgx_mission_forward / mgx_mission_backward, added within ABI 9): everything that can be
checked without a GPU -- the workspace size, the argument checks, the exports and the Python-side validation."""
import ctypes

import pytest
import torch

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
