"""Deep episodes at block scale (needs an MI355X): the action scripts of tests/golden/actions -- the scripted
agent (tests/golden/scripted_agent.py) over hundreds of envs, so that many envs of one workgroup unlock doors,
consume carried objects, run into the time limit and end on their last step at once -- through every step
kernel, bit-exact against the C oracle:

  mgx_step                  SB3 layout, terminal mode `all`
  mgx_step_compact          terminal mode `truncated`, the terminal rows tracked on the host
  mgx_rollout_compact       whole 32-step epochs, terminal mode `truncated`
  mgx_rollout_compact_gae   the S = 16 script, GAE over episodes hundreds of steps long

The oracle's run of a script is computed once per session and shared (read-only)."""
import functools

import numpy as np
import pytest

from test_scripted_agent import SCRIPTS, load_script

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAMES = sorted(SCRIPTS)
E = 32                                              # refill epoch = fused chunk
STATE = ("grid", "agent", "carrying", "step_count", "mission_done", "mtwords", "pcg", "target")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class Trace:
    """The oracle's run of one action script: reset obs, every step's outputs, the events per (t, env), final state."""


@functools.lru_cache(maxsize=None)
def oracle_trace(name):
    import oracle as O
    acts, cfg, _ = load_script(name)
    T, n = acts.shape
    ov = O.OracleVec(cfg["problem"], cfg["mission"], cfg["size"], cfg["num_objects"], n, cfg["seed"])
    tr = Trace()
    tr.cfg, tr.n, tr.T, tr.acts = cfg, n, T, acts.astype(np.int32)
    tr.reset = ov.reset()
    tr.steps = []
    tr.unlock = np.zeros((T, n), bool)
    dv = np.array([(1, 0), (0, 1), (-1, 0), (0, -1)])
    ii = np.arange(n)
    for t in range(T):
        st = ov.dump()                                # the state the step starts from
        ag = st["agent"].astype(np.int64)
        front = st["grid"][ii, ag[:, 0] + dv[ag[:, 2], 0], ag[:, 1] + dv[ag[:, 2], 1]]
        tr.unlock[t] = ((tr.acts[t] == 5) & (front[:, 0] == 4) & (front[:, 2] == 2) & (st["carrying"][:, 0] == 5)
                        & (st["carrying"][:, 1] == front[:, 1]))
        tr.steps.append(ov.step(tr.acts[t]))
    tr.final = ov.dump()
    tr.term = np.stack([o["terminated"] for o in tr.steps]).astype(bool)
    tr.trunc = np.stack([o["truncated"] for o in tr.steps]).astype(bool)
    tr.done = tr.term | tr.trunc
    tr.reward = np.stack([o["reward"] for o in tr.steps])
    for a in [tr.acts, tr.unlock, tr.term, tr.trunc, tr.done, tr.reward] + list(tr.final.values()) + \
            [x for o in tr.steps + [tr.reset] for x in o.values()]:
        a.setflags(write=False)
    return tr


def _script_is_deep(tr):
    """Conditions on the script, from the oracle's run alone -- a quiet script must not pass vacuously: every
    64-env block (the tail block of eight included) holds a truncation, a truncation that is no termination and,
    where the config has locked doors at all (the multi-room problems), a door unlocked with the carried key; the
    script holds steps that terminate and truncate at once, and steps that pay a reward."""
    for b in range(0, tr.n, 64):
        s = slice(b, b + 64)
        assert tr.trunc[:, s].any() and (tr.trunc & ~tr.term)[:, s].any(), b
        if tr.cfg["problem"] == "multi":
            assert tr.unlock[:, s].any(), b
    assert (tr.trunc & tr.term).any() and (tr.reward > 0).sum() > tr.n


def _engine(tr, **kw):
    from mgx import MgxEngine
    c = tr.cfg
    return MgxEngine(problem=c["problem"], mission=c["mission"], size=c["size"], num_objects=c["num_objects"],
                     seed=c["seed"], n_envs=tr.n, n_stack=4, **kw)


def _same_state(eng, tr):
    a, b = eng.dump_state(), tr.final
    for k in STATE:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["stored_reward"], b["stored_reward"], equal_nan=True)


def _rows_of(img, dr):
    """Oracle frames (image HWC [n, 7, 7, 3], direction [n]) -> compact rows u8 [n, 148]."""
    n = img.shape[0]
    return np.concatenate([dr.reshape(n, 1), img.transpose(0, 3, 1, 2).reshape(n, 147)], axis=1)


def _want_row(o):
    done = (o["terminated"] | o["truncated"]).astype(bool)
    return _rows_of(np.where(done[:, None, None, None], o["r_image"], o["image"]), np.where(done, o["r_dir"], o["dir"]))


@pytest.mark.parametrize("name", NAMES)
def test_step_kernel_matches_oracle(name):
    """mgx_step, SB3 layout, terminal mode `all`: per step done / terminated / truncated, the f64 and f32 reward,
    the newest frame (the terminal frame where the episode ended), the new episode's frame and mission, the
    live-lock count; at the end every env's state."""
    _need_gpu()
    from test_gpu_parity import EngineSource
    tr = oracle_trace(name)
    _script_is_deep(tr)
    eng = _engine(tr, terminal_mode="all", reward64=True)
    obs = eng.reset()
    img, dr, mi = EngineSource.newest(obs)
    r = tr.reset
    assert np.array_equal(img, r["image"]) and np.array_equal(dr, r["dir"]) and np.array_equal(mi, r["mission"])
    acts = torch.tensor(np.array(tr.acts), device=eng.device)
    for t in range(tr.T):
        o = tr.steps[t]
        obs = eng.step(acts[t])
        done = eng.done.cpu().numpy().astype(bool)
        assert np.array_equal(done, tr.done[t]), t
        assert np.array_equal(eng.terminated.cpu().numpy().astype(bool), tr.term[t]), t
        assert np.array_equal(eng.truncated.cpu().numpy().astype(bool), tr.trunc[t]), t
        assert np.array_equal(eng.reward64.cpu().numpy(), o["reward"]), t
        assert np.array_equal(eng.reward.cpu().numpy(), o["reward"].astype(np.float32)), t
        img, dr, mi = EngineSource.newest(obs)
        timg, tdr, tmi = EngineSource.newest(eng.terminal_obs)
        assert np.array_equal(np.where(done[:, None, None, None], timg, img), o["image"]), t
        assert np.array_equal(np.where(done, tdr, dr), o["dir"]), t
        assert np.array_equal(np.where(done[:, None], tmi, mi), o["mission"]), t
        assert np.array_equal(img[done], o["r_image"][done]) and np.array_equal(dr[done], o["r_dir"][done]), t
        assert np.array_equal(mi[done], o["r_mission"][done]), t
        assert np.array_equal(eng.livelock.cpu().numpy()[done], o["livelock"][done]), t
    _same_state(eng, tr)
    eng.poll_error()


@pytest.mark.parametrize("name", NAMES)
def test_step_compact_terminal_rows_match_oracle(name):
    """mgx_step_compact, terminal mode `truncated`: per step the observation row, mission id, done / terminated /
    truncated flags and both rewards; terminal_rows[i] is the final frame exactly where the episode was truncated
    and not terminated, and keeps its content through every other ending -- the steps that terminate and truncate
    at once among them (the expected rows are tracked on the host from the first step on)."""
    _need_gpu()
    from mgx._lib import mission_tokens
    from mgx.compact import CompactBuffer
    tr = oracle_trace(name)
    _script_is_deep(tr)
    eng = _engine(tr, terminal_mode="truncated", reward64=True, mission_dtype=torch.uint8)
    buf = CompactBuffer(eng, tr.T)
    tok = mission_tokens()
    eng.reset()
    buf.observe(0)
    H = buf.H
    assert np.array_equal(buf.rows[H].cpu().numpy(), _rows_of(tr.reset["image"], tr.reset["dir"]))
    assert np.array_equal(tok[buf.mids[H].cpu().numpy()], tr.reset["mission"])
    want_term = buf.terminal_rows.cpu().numpy().copy()
    acts = torch.tensor(np.array(tr.acts), device=eng.device)
    for t in range(tr.T):
        o = tr.steps[t]
        buf.step(t, acts[t])
        r = H + 1 + t
        assert np.array_equal(buf.rows[r].cpu().numpy(), _want_row(o)), t
        assert np.array_equal(tok[buf.mids[r].cpu().numpy()], np.where(tr.done[t][:, None], o["r_mission"], o["mission"])), t
        assert np.array_equal(buf.starts[r].cpu().numpy().astype(bool), tr.done[t]), t
        assert np.array_equal(buf.terminated[t].cpu().numpy().astype(bool), tr.term[t]), t
        assert np.array_equal(buf.truncated[t].cpu().numpy().astype(bool), tr.trunc[t]), t
        assert np.array_equal(eng.reward64.cpu().numpy(), o["reward"]), t
        assert np.array_equal(buf.rewards[t].cpu().numpy(), o["reward"].astype(np.float32)), t
        assert np.array_equal(eng.livelock.cpu().numpy()[tr.done[t]], o["livelock"][tr.done[t]]), t
        only = tr.trunc[t] & ~tr.term[t]
        want_term[only] = _rows_of(o["image"], o["dir"])[only]
        assert np.array_equal(buf.terminal_rows.cpu().numpy(), want_term), t
    _same_state(eng, tr)
    eng.poll_error()


def _run_fused(tr, check_chunk, gae=None):
    """The script through the fused rollout in whole epochs of E steps; check_chunk(buf, t0) after each."""
    from mgx.compact import CompactBuffer
    eng = _engine(tr, terminal_mode="truncated", mission_dtype=torch.uint8, refill_every=E)
    assert eng.refill_every == E and tr.T % E == 0
    buf = CompactBuffer(eng, tr.T)
    eng.reset()
    buf.observe(0)
    acts = torch.tensor(np.array(tr.acts), device=eng.device)
    for t0 in range(0, tr.T, E):
        buf.rollout(t0, acts[t0:t0 + E].contiguous(), gae=None if gae is None else gae(t0))
        torch.cuda.synchronize()
        check_chunk(buf, t0)
    _same_state(eng, tr)
    eng.poll_error()


@pytest.mark.parametrize("name", NAMES)
def test_fused_rollout_matches_oracle(name):
    """mgx_rollout_compact in whole 32-step epochs, terminal mode `truncated` (32-env blocks at S = 16): every
    step's row, mission id, done / terminated / truncated flag and f32 reward; at each chunk end the terminal row
    of every env -- the final frame of its last truncated-only ending so far, untouched by any other ending; the
    state of every env at the end."""
    _need_gpu()
    from mgx._lib import mission_tokens
    tr = oracle_trace(name)
    _script_is_deep(tr)
    tok = mission_tokens()
    want_term = np.zeros((tr.n, 148), np.uint8)

    def check(buf, t0):
        H = buf.H
        rows, mids = buf.rows.cpu().numpy(), buf.mids.cpu().numpy()
        starts, rew = buf.starts.cpu().numpy().astype(bool), buf.rewards.cpu().numpy()
        trm, trc = buf.terminated.cpu().numpy().astype(bool), buf.truncated.cpu().numpy().astype(bool)
        for t in range(t0, t0 + E):
            o = tr.steps[t]
            r = H + 1 + t
            assert np.array_equal(starts[r], tr.done[t]), t
            assert np.array_equal(trm[t], tr.term[t]) and np.array_equal(trc[t], tr.trunc[t]), t
            assert np.array_equal(rows[r], _want_row(o)), t
            assert np.array_equal(tok[mids[r]], np.where(tr.done[t][:, None], o["r_mission"], o["mission"])), t
            assert np.array_equal(rew[t], o["reward"].astype(np.float32)), t
            only = tr.trunc[t] & ~tr.term[t]
            want_term[only] = _rows_of(o["image"], o["dir"])[only]
        assert np.array_equal(buf.terminal_rows.cpu().numpy(), want_term), t0

    _run_fused(tr, check)


def test_fused_rollout_gae_over_long_episodes():
    """mgx_rollout_compact_gae on the S = 16 script, random f32 values: the advantages and returns of every
    32-step launch equal the numpy GAE fed the oracle's rewards and dones.  Episodes run for up to 256 steps, so
    the recurrence crosses whole launches without a reset.  A condition of the test: at least a quarter of the
    (launch, env) pairs hold no reset at all -- under uniform random actions (6/7)^32 = 0.7 % of them would."""
    _need_gpu()
    import oracle as O
    tr = oracle_trace("multi_tgl_s16")
    _script_is_deep(tr)
    chunk_has_done = tr.done.reshape(tr.T // E, E, tr.n).any(1)
    assert (~chunk_has_done).mean() >= 0.25
    rng = np.random.default_rng(16)
    vals = rng.standard_normal((tr.T + 1, tr.n)).astype(np.float32)
    gamma, lam = 0.8108071290665859, 0.9452281119742252
    dev = torch.device("cuda")
    vd = torch.as_tensor(vals, device=dev)
    adv, ret = torch.empty((E, tr.n), device=dev), torch.empty((E, tr.n), device=dev)

    def gae(t0):
        return dict(values=vd[t0:t0 + E], last_values=vd[t0 + E], gamma=gamma, gae_lambda=lam, out=(adv, ret))

    def check(buf, t0):
        dn = tr.done[t0:t0 + E]
        es = np.zeros((E, tr.n), np.float32)
        es[1:] = dn[:-1]
        rew = tr.reward[t0:t0 + E].astype(np.float32)
        want_a, want_r = O.gae(rew, vals[t0:t0 + E], es, vals[t0 + E], dn[-1], gamma, lam)
        assert np.array_equal(buf.rewards[t0:t0 + E].cpu().numpy(), rew), t0
        assert np.array_equal(adv.cpu().numpy(), want_a), t0
        assert np.array_equal(ret.cpu().numpy(), want_r), t0

    _run_fused(tr, check, gae=gae)
