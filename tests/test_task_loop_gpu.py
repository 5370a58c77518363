"""The refill kernel's key / object task loop (mgx_device.h: gen_rooms' one loop over the placement draws' ten-word
passes) on the GPU against the C oracle, on RAGGED engines: the last refill wave holds a few lanes only, so lanes
without an env sit beside lanes that run out of tasks, are abandoned at the live-lock word cap or still place keys
and objects.  n = 130 at S = 8 (the 32-env S = 8 kernel, a last wave of 2 lanes; mission 5 and drawn missions), n = 70
at S = 11 (two 64-bit cell sets) and n = 40 at S = 16 (the LDS-grid path), rings that turn over several times
(refill every 8 steps, 160 steps of actions that are 'done' half the time), at the default live-lock word cap and at 64
words, where the cap fires inside the placement draws.  After every step every env's grid, agent, target, MT19937
cursor and PCG64 state, its mission tokens, `done` and the abandoned-attempt count of the fresh episodes must equal
the oracle's, and no device error bit may be set.  One configuration runs the same through the fused rollout
(mgx_rollout_compact).  The 64-env S = 8 kernel is what test_rollout.py::test_rollout_full_size_matches_oracle
[cfg2_65536] runs against the oracle."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

STATE_KEYS = ("grid", "agent", "carrying", "step_count", "mission_done", "mtwords", "pcg", "target")
T, K = 160, 8


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _actions(n):
    rng = np.random.default_rng(11)
    a = rng.integers(0, 7, (T, n), dtype=np.int32)
    return np.where(rng.random((T, n)) < 0.5, 6, a).astype(np.int32)


def _oracle(mission, size, n, llw):
    import oracle as O
    kw = {} if llw == 0 else dict(livelock_words=llw)
    return O.OracleVec("multi", mission, size, 4, n, 42, **kw)


CASES = [(5, 8, 130), (None, 8, 130), (2, 11, 70), (1, 16, 40)]


@pytest.mark.parametrize("llw", [64, 0], ids=["llw64", "llwdefault"])
@pytest.mark.parametrize("mission,size,n", CASES, ids=["m%s_s%d_n%d" % c for c in CASES])
def test_ragged_reset_episodes_match_oracle(mission, size, n, llw):
    _need_gpu()
    from mgx import MgxEngine
    from mgx._lib import mission_tokens
    ov = _oracle(mission, size, n, llw)
    eng = MgxEngine(problem="multi", mission=mission, size=size, n_envs=n, n_stack=4, terminal_mode="all",
                    livelock_words=llw, refill_every=K)
    assert eng.ring_depth > 0 and eng.refill_every == K
    tok = mission_tokens()
    r = ov.reset()
    eng.reset()
    assert np.array_equal(eng.livelock.cpu().numpy(), r["livelock"])
    acts = _actions(n)
    resets = abandoned = 0
    for t in range(T):
        o = ov.step(acts[t])
        eng.step(torch.as_tensor(acts[t], device=eng.device))
        done = eng.done.cpu().numpy().astype(bool)
        assert np.array_equal(done, (o["terminated"] | o["truncated"]).astype(bool)), t
        assert np.array_equal(eng.livelock.cpu().numpy()[done], o["livelock"][done]), t
        a, b = eng.dump_state(), ov.dump()
        for k in STATE_KEYS:
            assert np.array_equal(a[k], b[k]), (k, t)
        assert np.array_equal(tok[a["mission_id"]], np.where(done[:, None], o["r_mission"], o["mission"])), ("mission", t)
        resets += int(done.sum())
        abandoned += int(o["livelock"][done].sum())
    eng.poll_error()
    assert resets > 4 * n                                  # every ring turned over several times
    if llw == 64:
        assert abandoned > 0                               # the cap did fire


def test_ragged_reset_episodes_match_oracle_fused_rollout():
    _need_gpu()
    from mgx import MgxEngine
    from mgx.compact import CompactBuffer
    mission, size, n, llw = None, 8, 130, 64
    ov = _oracle(mission, size, n, llw)
    eng = MgxEngine(problem="multi", mission=mission, size=size, n_envs=n, terminal_mode="truncated",
                    mission_dtype=torch.uint8, livelock_words=llw, refill_every=K)
    buf = CompactBuffer(eng, K)
    ov.reset()
    eng.reset()
    buf.observe(0)
    acts = _actions(n)
    ad = torch.as_tensor(acts, device=eng.device)
    for c in range(T // K):
        if c:
            buf.carry_over()
        buf.rollout(0, ad[c * K:(c + 1) * K])              # 8 steps, one launch
        rows = buf.rows.cpu().numpy()
        dones = buf.dones.cpu().numpy().astype(bool)
        for j in range(K):
            o = ov.step(acts[c * K + j])
            done = (o["terminated"] | o["truncated"]).astype(bool)
            assert np.array_equal(dones[j], done), (c, j)
            row = rows[buf.row(j + 1)]
            img = row[:, 1:].reshape(n, 3, 7, 7).transpose(0, 2, 3, 1)
            assert np.array_equal(img, np.where(done[:, None, None, None], o["r_image"], o["image"])), (c, j)
            assert np.array_equal(row[:, 0], np.where(done, o["r_dir"], o["dir"])), (c, j)
        a, b = eng.dump_state(), ov.dump()
        for k in STATE_KEYS:
            assert np.array_equal(a[k], b[k]), (k, c)
    eng.poll_error()
