"""Graph-captured PPO collect (PPOConfig.graph_collect, mgx_policy_bootstrap): everything that can be checked
without a GPU -- the configuration rules, the refill-epoch helper and the entry point's argument checks."""
import ctypes

import pytest

from mgx import _lib
from mgx.ppo import PPOConfig, graph_refill_every


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_graph_collect_needs_fused_act_and_compact_layout():
    with pytest.raises(ValueError):
        PPOConfig(graph_collect=True)
    with pytest.raises(ValueError):
        PPOConfig(graph_collect=True, fused_act=True, layout="sb3")
    cfg = PPOConfig(graph_collect=True, fused_act=True)
    assert cfg.graph_collect and cfg.layout == "compact"
    assert PPOConfig().graph_collect is False


@pytest.mark.parametrize("horizon,want", [(16, 16), (1024, 64), (20, 20), (67, 1)])
def test_graph_refill_every(horizon, want):
    """The largest divisor of the horizon that is <= 64."""
    assert graph_refill_every(horizon) == want


def test_policy_bootstrap_rejects_bad_arguments_without_gpu(lib):
    """Every bad-argument case that needs no live handle returns MGX_ERR_INVALID before any HIP call and before any
    pointer is dereferenced (0 < ring_rows < n_stack reads the handle's n_stack: tests/test_graph_collect_gpu.py)."""
    d = ctypes.c_void_p(0x1000)                      # never dereferenced: the checks come first

    def policy(**kw):
        p = _lib.MgxPolicy(blob_dev=0x1000, mission_feat_dev=0x1000, mode=0, seed=1, counter_dev=0x1000)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def boot(**kw):
        b = _lib.MgxBootstrap(truncated_dev=0x1000, terminated_dev=0x1000, rewards_dev=0x1000, gamma=0.5,
                              list_dev=0x1000, count_dev=0x1000, values_dev=None)
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    def call(h=d, rows=d, mids=d, starts=d, n=64, ring=8, row=3, term=d, pol=policy(), b=boot()):
        return lib.mgx_policy_bootstrap(h, rows, mids, starts, n, ring, row, term,
                                        None if pol is None else ctypes.byref(pol),
                                        None if b is None else ctypes.byref(b), None)

    cases = [dict(h=None), dict(rows=None), dict(mids=None), dict(starts=None), dict(term=None), dict(pol=None),
             dict(b=None), dict(pol=policy(blob_dev=None)), dict(pol=policy(mission_feat_dev=None)),
             dict(b=boot(truncated_dev=None)), dict(b=boot(terminated_dev=None)), dict(b=boot(rewards_dev=None)),
             dict(b=boot(list_dev=None)), dict(b=boot(count_dev=None)),
             dict(n=0), dict(n=-4), dict(row=-1), dict(row=8), dict(row=9), dict(ring=0, row=-1), dict(ring=-1)]
    for kw in cases:
        st = call(**kw)
        assert st == 1, (kw, st)                     # MGX_ERR_INVALID
        assert b"mgx_policy_bootstrap" in lib.mgx_last_error()
