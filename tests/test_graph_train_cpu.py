"""Graph-captured PPO update (PPOConfig.graph_train): everything that can be checked without a GPU
-- the exports, mgx_adam_schedule's entries, the argument checks of mgx_adam_step_sched and of the two mission _rows
calls (MGX_ERR_INVALID before any HIP call: the pointers are fake), and the flag's validation."""
import ctypes
import math

import numpy as np
import pytest
import torch

from mgx import _lib

NEW = ("mgx_adam_schedule", "mgx_adam_step_sched", "mgx_mission_forward_rows", "mgx_mission_backward_rows")
BETAS = (0.9, 0.999)
LRS = (3e-4, 1.234567e-5, 3e-6)
INVALID = 1                                          # MGX_ERR_INVALID


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_exports_and_abi_version(lib):
    assert _lib.ABI_VERSION == 9 and lib.mgx_abi_version() == 9
    for name in NEW:
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
    assert ctypes.sizeof(_lib.MgxAdamSched) == 8
    assert [f[0] for f in _lib.MgxAdamSched._fields_] == ["step_size", "bc2_sqrt"]


def _adam_args(**kw):
    a = _lib.MgxAdamArgs(lr=123.0, beta1=BETAS[0], beta2=BETAS[1], eps=1e-8, step=-7, max_grad_norm=0.5,
                         grad_scale=1.0)      # lr and step are ignored by the two new calls
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("step", [1, 2, 1000, 10 ** 6])
def test_adam_schedule_entries(lib, step):
    """Entry i is (float)(lr[i] / (1 - beta1^(first + i))) and (float)sqrt(1 - beta2^(first + i)), formed in double:
    one call per (step, lr), and one call of three consecutive steps with the three lrs."""
    from mgx.fused_update import adam_schedule
    b1, b2 = BETAS
    for lr in LRS:
        tab = adam_schedule([lr], step, betas=BETAS)
        assert tab.dtype == torch.float32 and tuple(tab.shape) == (1, 2)
        got = tab.numpy()
        assert got[0, 0] == np.float32(lr / (1 - b1 ** step)), (step, lr)
        assert got[0, 1] == np.float32(math.sqrt(1 - b2 ** step)), (step, lr)
    got = adam_schedule(LRS, step, betas=BETAS).numpy()
    assert got.shape == (3, 2)
    for i, lr in enumerate(LRS):
        assert got[i, 0] == np.float32(lr / (1 - b1 ** (step + i))), (step, i)
        assert got[i, 1] == np.float32(math.sqrt(1 - b2 ** (step + i))), (step, i)


def test_adam_schedule_rejects_bad_arguments(lib):
    out = (_lib.MgxAdamSched * 4)()
    lr = (ctypes.c_double * 4)(*([3e-4] * 4))

    def call(args="ok", lr=lr, first=1, n=4, out=out, **kw):
        a = _adam_args(**kw)
        return lib.mgx_adam_schedule(None if args is None else ctypes.byref(a), lr, first, n, out)

    assert call() == 0
    cases = [dict(args=None), dict(lr=None), dict(out=None), dict(first=0), dict(first=-5), dict(n=0), dict(n=-1),
             dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=float("nan")), dict(eps=-1e-8)]
    for i, kw in enumerate(cases):
        assert call(**kw) == INVALID, (i, kw)
        assert b"mgx_adam_schedule" in lib.mgx_last_error()


def test_adam_step_sched_rejects_bad_arguments_without_gpu(lib):
    n = 1025
    need = int(lib.mgx_adam_scratch_words(n))
    d = ctypes.c_void_p(0x1000)

    def call(param=d, grad=d, m=d, v=d, n=n, args="ok", table=d, table_len=3, cursor=d, norm=d, scratch=d,
             words=need, **kw):
        a = _adam_args(**kw)
        return lib.mgx_adam_step_sched(param, grad, m, v, n, None if args is None else ctypes.byref(a), table,
                                       table_len, cursor, norm, scratch, words, None)

    cases = [dict(param=None), dict(grad=None), dict(m=None), dict(v=None), dict(args=None), dict(scratch=None),
             dict(table=None), dict(cursor=None), dict(table_len=0), dict(table_len=-1), dict(n=0), dict(n=-1),
             dict(beta1=1.0), dict(beta2=1.5), dict(beta2=float("nan")), dict(eps=-1e-8), dict(words=need - 1),
             dict(words=0), dict(scratch=ctypes.c_void_p(0x1004))]
    for i, kw in enumerate(cases):
        assert call(**kw) == INVALID, (i, kw)
        assert b"mgx_adam_step_sched" in lib.mgx_last_error()


def _mission_structs(null=None, grads=False):
    s = (_lib.MgxMissionGrads if grads else _lib.MgxMissionParams)()
    for name, _ in s._fields_:
        setattr(s, name, None if name == null else 0x1000)
    return s


def test_mission_forward_rows_rejects_bad_arguments_without_gpu(lib):
    n, t = 5, 32
    need = int(lib.mgx_mission_workspace_words(n, t))
    d = ctypes.c_void_p(0x1000)

    def call(tokens=d, n=n, t=t, p="ok", null=None, table=d, rows=d, table_rows=1024, ws=d, words=need):
        ps = _mission_structs(null)
        return lib.mgx_mission_forward_rows(tokens, n, t, None if p is None else ctypes.byref(ps), table, rows,
                                            table_rows, ws, words, None)

    cases = [dict(tokens=None), dict(p=None), dict(table=None), dict(rows=None), dict(table_rows=0),
             dict(table_rows=-1), dict(words=need - 1), dict(words=0), dict(n=0), dict(n=2049), dict(t=0), dict(t=257)]
    cases += [dict(null=name) for name, _ in _lib.MgxMissionParams._fields_]
    for i, kw in enumerate(cases):
        assert call(**kw) == INVALID, (i, kw)
        assert b"mgx_mission_forward" in lib.mgx_last_error()


def test_mission_backward_rows_rejects_bad_arguments_without_gpu(lib):
    n, t = 5, 32
    need = int(lib.mgx_mission_workspace_words(n, t))
    d = ctypes.c_void_p(0x1000)

    def call(tokens=d, n=n, t=t, p="ok", null=None, g="ok", gnull=None, table=d, rows=d, table_rows=1024, ws=d,
             words=need):
        ps, gs = _mission_structs(null), _mission_structs(gnull, grads=True)
        return lib.mgx_mission_backward_rows(tokens, n, t, None if p is None else ctypes.byref(ps), table, rows,
                                             table_rows, ws, words, None if g is None else ctypes.byref(gs), None)

    cases = [dict(tokens=None), dict(p=None), dict(g=None), dict(table=None), dict(rows=None), dict(ws=None),
             dict(table_rows=0), dict(table_rows=-1), dict(words=need - 1), dict(words=0), dict(n=0), dict(n=2049),
             dict(t=0), dict(t=257)]
    cases += [dict(null=name) for name, _ in _lib.MgxMissionParams._fields_]
    cases += [dict(gnull=name) for name, _ in _lib.MgxMissionGrads._fields_]
    for i, kw in enumerate(cases):
        assert call(**kw) == INVALID, (i, kw)
        assert b"mgx_mission_backward" in lib.mgx_last_error()


def test_graph_train_flag_validation():
    from mgx.ppo import PPOConfig
    assert PPOConfig().graph_train is False
    for kw in (dict(), dict(fused_train=True, fused_mission=True), dict(fused_act=True, graph_collect=True)):
        with pytest.raises(ValueError):
            PPOConfig(graph_train=True, **kw)
    cfg = PPOConfig(graph_train=True, fused_update=True, fused_train=True, fused_mission=True)
    assert cfg.graph_train
    PPOConfig(graph_train=True, fused_update=True, fused_train=True, fused_mission=True, fused_act=True,
              graph_collect=True)


def test_trainer_rejects_a_group_with_graph_train():
    """The all-reduce is not captured: a data-parallel group with the flag is a ValueError, before the group is
    touched; without the flag the same constructor call is not this error."""
    from mgx.policy import ActorCriticPolicy
    from mgx.ppo import PPOConfig, Trainer, learn
    cfg = PPOConfig(graph_train=True, fused_update=True, fused_train=True, fused_mission=True, n_frames_stack=1)
    pol = ActorCriticPolicy(n_stack=1)
    with pytest.raises(ValueError, match="graph_train"):
        Trainer(pol, cfg, group=object())
    with pytest.raises(ValueError, match="graph_train"):
        learn(cfg, 16, device="cpu", group=object())
    assert Trainer(pol, cfg).group is None
