"""Fused actor-critic inference on the GPU (mgx_policy_act, mgx/fused_policy.py) against the torch module.

Reference: the same module in fp64 on the CPU, on the stacked observation mgx_gather_ring builds for the same
sample.  The tolerance is measured, per quantity and per n_stack, on the run itself: e_torch = max |torch fp32 on
the GPU - fp64| over the same samples, and the kernel may deviate from fp64 by at most 4 x e_torch (both are fp32
sums of <= 208 terms in different orders: headroom for order, not for another precision).

Setup: gtg 6x6, 70 envs (one full 64-sample tile + a 6-lane tail), a ring CompactBuffer of T = 3 (at n_stack 4 the
walk-back wraps the ring), 40 random-action steps over carried-over rollouts (episodes <= 36 steps, so episode starts
fall inside stack windows); action_net redrawn N(0, 1) (the initial gain of 0.01 makes every logit nearly tied).

n_stack 5..8 (mgx_policy_kernel<5..8>: X = 37 K rows of LDS, 16 direction bits, 15..24 conv1 trips, direction weight
columns up to 4 K - 1, mission_feat[mid][v-1] with v up to 8): the ring is 3 or 4 blocks of 3 rows and the walk-back
crosses up to three of them.  The reference observation there is still buf.gather_step, which tests/test_compact.py
pins to the FrameStackOracle at those depths; at n_stack 8 the run itself also compares the final gathered observation
with the C oracle's frames stacked by the FrameStackOracle (_oracle_stacks).

Every gtg episode has mission id 3: each lane of a tile reads the same mission-feature row.  The *_many_missions tests
run the same setup on MULTI (multi 8x8, mission=None: dozens of mission ids below 128 per tile), the *_high_mission_ids
tests on FULL (ids 128..132 next to ids below 128); both pin the n_stack 8 observation to the oracle as well."""
import copy
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mgx.policy import ActorCriticPolicy  # noqa: E402

pytestmark = pytest.mark.gpu

N_ENVS, T_RING, STEPS = 70, 3, 40
ENV = dict(problem="gtg", mission=5, size=6, num_objects=2)
MULTI = dict(problem="multi", mission=None, size=8, num_objects=4)
FULL = dict(problem="full", mission=None, size=8, num_objects=4)
M64 = (1 << 64) - 1


def _policy(k, seed=0):
    torch.manual_seed(seed)
    pol = ActorCriticPolicy(n_stack=k)
    g = torch.Generator().manual_seed(100 + seed)
    with torch.no_grad():
        pol.action_net.weight.copy_(torch.randn(pol.action_net.weight.shape, generator=g))
        pol.action_net.bias.copy_(torch.randn(pol.action_net.bias.shape, generator=g))
    pol.train(False)
    return pol


def _ref64(pol64, obs):
    """(logits, values) f64 of the fp64 CPU module on a u8 stacked observation (SB3 preprocess_obs in fp64)."""
    o = {"image": obs["image"].cpu().double() / 255.0, "direction": obs["direction"].cpu().double(),
         "mission": obs["mission"].cpu()}
    with torch.no_grad():
        f = pol64.features_extractor(o)
        return pol64.action_net(pol64.policy_net(f)), pol64.value_net(pol64.value_net_body(f)).flatten()


def _torch32(pol, obs):
    """(logits, values) of the fp32 module on the GPU, on the same u8 observation."""
    with torch.no_grad():
        pi, vf = pol._latent(obs)
        return pol.action_net(pi).double().cpu(), pol.value_net(vf).flatten().double().cpu()


def _cat(obs_list):
    return {k: torch.cat([o[k] for o in obs_list]) for k in obs_list[0]}


def _oracle_stacks(k, actions, env=ENV):
    """The stacked observation before every step and after the last one: the C oracle stepped with `actions`
    ([steps, N_ENVS]), its frames stacked by the numpy VecTransposeImage + VecFrameStack restatement."""
    import oracle as O
    ov = O.OracleVec(env["problem"], env["mission"], env["size"], env["num_objects"], N_ENVS, 42)
    fs = O.FrameStackOracle(N_ENVS, k)

    def raw(img, dr, mi):
        return dict(image=O.vec_transpose_image(img), direction=O.one_hot_dir(dr), mission=mi.astype(np.int64))

    r = ov.reset()
    out = [{kk: v.copy() for kk, v in fs.reset(raw(r["image"], r["dir"], r["mission"])).items()}]
    for a in actions:
        o = ov.step(np.asarray(a, dtype=np.int32))
        done = (o["terminated"] | o["truncated"]).astype(bool)
        cur = raw(np.where(done[:, None, None, None], o["r_image"], o["image"]), np.where(done, o["r_dir"], o["dir"]),
                  np.where(done[:, None], o["r_mission"], o["mission"]))
        st, _ = fs.step(cur, done, raw(o["image"], o["dir"], o["mission"]))
        out.append({kk: v.copy() for kk, v in st.items()})
    return out


class Run:
    pass


_RUNS = {}


def _run(k, env=ENV):
    """One 40-step trajectory per (n_stack, env), everything the tests compare recorded once."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    key = (k, tuple(sorted(env.items())))
    if key in _RUNS:
        return _RUNS[key]
    from mgx import MgxEngine
    from mgx.compact import CompactBuffer
    from mgx.fused_policy import FusedActor
    r = Run()
    r.pol = _policy(k).cuda()
    r.pol64 = copy.deepcopy(r.pol).cpu().double()
    r.eng = MgxEngine(n_envs=N_ENVS, n_stack=k, terminal_mode="truncated", mission_dtype=torch.uint8, **env)
    r.buf = CompactBuffer(r.eng, T_RING, ring=True)
    r.actor = FusedActor(r.pol, r.eng, seed=1234)
    r.eng.reset()
    r.buf.observe(0)
    g = torch.Generator().manual_seed(5)
    obs, lg, val, act, lp, starts, stepped, mids = [], [], [], [], [], 0, [], []
    t = 0
    for step in range(STEPS + 1):
        obs.append({kk: v.clone() for kk, v in r.buf.gather_step(t, f32=False).items()})
        mids.append(r.buf.mids[r.buf.row(t)].cpu().long())
        l, v = r.actor.logits(r.buf, t)
        a, v1, p = r.actor.act(r.buf, t, deterministic=True)
        assert torch.equal(v, v1)                          # modes 0 and 1: the same forward pass
        lg.append(l.double().cpu()); val.append(v.double().cpu()); act.append(a.cpu()); lp.append(p.double().cpu())
        if step == STEPS:
            break
        stepped.append(torch.randint(0, 7, (N_ENVS,), generator=g))
        r.buf.step(t, stepped[-1].cuda())
        starts += int(r.buf.dones[t].sum())
        t += 1
        if t == T_RING:
            r.buf.carry_over()
            t = 0
    r.t = t                                                # the buffer is left at observation t
    r.episode_ends = starts
    if k == 8:
        # the reference observation of this file is the gather's: pin it to the oracle here too (the final step, whose
        # stack was built across carried-over ring blocks)
        want = _oracle_stacks(k, torch.stack(stepped).numpy(), env)[-1]
        for kk in ("image", "direction", "mission"):
            assert np.array_equal(obs[-1][kk].cpu().numpy().astype(np.int64), want[kk].astype(np.int64)), kk
    r.obs = _cat(obs)
    r.mid = torch.cat(mids)                                # mission id of every sample, launch by launch
    r.v = (r.obs["direction"].reshape(-1, k, 4).sum(2) > 0).sum(1).cpu()
    r.logits, r.values, r.actions, r.log_probs = torch.cat(lg), torch.cat(val), torch.cat(act), torch.cat(lp)
    r.ref_logits, r.ref_values = _ref64(r.pol64, r.obs)
    r.ref_logp = torch.log_softmax(r.ref_logits, 1)
    t_logits, t_values = _torch32(r.pol, {kk: v.cuda() for kk, v in r.obs.items()})
    t_logp = torch.log_softmax(t_logits.float().cuda(), 1).double().cpu()     # fp32 log-softmax, as Categorical does
    r.e_torch = dict(logits=float((t_logits - r.ref_logits).abs().max()),
                     values=float((t_values - r.ref_values).abs().max()),
                     log_probs=float((t_logp - r.ref_logp).abs().max()))
    r.tol = {kk: 4.0 * v for kk, v in r.e_torch.items()}
    r.eng.poll_error()
    _RUNS[key] = r
    return r


def _forward_parity(r, k, tag=""):
    assert r.logits.shape == (N_ENVS * (STEPS + 1), 7)
    assert r.episode_ends > N_ENVS                         # starts inside the stack windows were exercised
    n_empty = int((r.obs["direction"].reshape(-1, k, 4).sum(2) == 0).any(1).sum())
    if k > 1:
        assert n_empty > N_ENVS                            # stacks with empty slots beyond the first observation
    dev = dict(logits=float((r.logits - r.ref_logits).abs().max()),
               values=float((r.values - r.ref_values).abs().max()))
    lp_ref = r.ref_logp.gather(1, r.actions[:, None])[:, 0]
    dev["log_probs"] = float((r.log_probs - lp_ref).abs().max())
    for q in ("logits", "values", "log_probs"):
        print("%sn_stack %d %s: kernel max |dev| %.3e, torch fp32 (GPU) max |dev| %.3e, bound %.3e"
              % (tag, k, q, dev[q], r.e_torch[q], r.tol[q]))
    for q in ("logits", "values", "log_probs"):
        assert r.e_torch[q] > 0
        assert dev[q] <= r.tol[q], (q, dev[q], r.e_torch[q])


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7, 8])
def test_forward_parity(k):
    """logits, values and mode-1 log-probs of every sample of every step within 4 x e_torch of the fp64 module."""
    _forward_parity(_run(k), k)


def _launch_tiles(r):
    """[(mid, v)] of the full 64-sample tile of every launch (70 envs: one full tile and a 6-lane tail)."""
    pairs = list(zip(r.mid.tolist(), r.v.tolist()))
    return [pairs[i:i + 64] for i in range(0, len(pairs), N_ENVS)]


def _assert_many_keys(r, k):
    """Some launch's full tile holds >= 9 distinct (mission id, v) keys, and >= 12 mission ids occur."""
    counts = [len(set(t)) for t in _launch_tiles(r)]
    print("multi n_stack %d: distinct (mid, v) keys per launch tile: min %d, max %d; %d mission ids in all"
          % (k, min(counts), max(counts), len(set(r.mid.tolist()))))
    assert max(counts) >= 9 and len(set(r.mid.tolist())) >= 12


@pytest.mark.parametrize("k", [4, 8])
def test_forward_parity_many_missions(k):
    """test_forward_parity on MULTI: every lane of a tile fetches its own mission-feature row."""
    r = _run(k, MULTI)
    _assert_many_keys(r, k)
    _forward_parity(r, k, "multi ")


@pytest.mark.parametrize("k", [4, 8])
def test_forward_parity_high_mission_ids(k):
    """test_forward_parity on FULL: one tile holds mission ids >= 128 (drop, move) next to ids below 128."""
    r = _run(k, FULL)
    tiles = _launch_tiles(r)
    high = [sum(m >= 128 for m, _ in t) for t in tiles]
    print("full n_stack %d: samples with mission id >= 128 per launch tile: min %d, max %d; ids %s"
          % (k, min(high), max(high), sorted(set(r.mid.tolist()))))
    assert any(0 < h < 64 for h in high) and int(r.mid.max()) <= 132
    _forward_parity(r, k, "full ")


@pytest.mark.parametrize("k", [1, 3, 4, 5, 8])
def test_deterministic_actions(k):
    """Mode 1 = the fp64 arg-max wherever the fp64 top-2 gap is >= 1e-3; such near-ties are <= 1 % of samples."""
    r = _run(k)
    top2 = r.ref_logits.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) >= 1e-3
    assert float((~clear).float().mean()) <= 0.01
    assert torch.equal(r.actions[clear], r.ref_logits.argmax(1)[clear])
    assert int(r.actions.min()) >= 0 and int(r.actions.max()) <= 6


@pytest.mark.parametrize("k", [1, 3, 4, 5, 8])
def test_subsets_and_terminal_rows(k):
    """values(terminal=True, envs=boot) on the steps where truncations occur ('done'-free actions for 36 steps
    force them), and single-env subsets, against the fp64 module on the matching gather_step."""
    r = _run(k)
    from mgx.compact import CompactBuffer
    eng, actor = r.eng, r.actor
    eng.reset()
    buf = CompactBuffer(eng, T_RING, ring=True)
    buf.observe(0)
    g = torch.Generator().manual_seed(9)
    t, n_boot, worst = 0, 0, 0.0
    for step in range(38):
        buf.step(t, torch.randint(0, 6, (N_ENVS,), generator=g).cuda())
        boot = (buf.truncated[t].bool() & ~buf.terminated[t].bool()).nonzero().flatten()
        if boot.numel():
            n_boot += int(boot.numel())
            for envs in (boot, boot[-1:]):
                got = actor.values(buf, t, terminal=True, envs=envs).double().cpu()
                _, want = _ref64(r.pol64, buf.gather_step(t, terminal=True, envs=envs, f32=False))
                assert got.shape == want.shape == (envs.numel(),)
                worst = max(worst, float((got - want).abs().max()))
        one = torch.tensor([(7 * step) % N_ENVS], device=eng.device)          # an `envs` subset of size 1
        got = actor.values(buf, t + 1, envs=one).double().cpu()
        _, want = _ref64(r.pol64, buf.gather_step(t + 1, envs=one, f32=False))
        worst = max(worst, float((got - want).abs().max()))
        lg1, _ = actor.logits(buf, t + 1, envs=one)
        want_l, _ = _ref64(r.pol64, buf.gather_step(t + 1, envs=one, f32=False))
        assert float((lg1.double().cpu() - want_l).abs().max()) <= r.tol["logits"]
        t += 1
        if t == T_RING:
            buf.carry_over()
            t = 0
    print("n_stack %d: %d truncation bootstraps, max |dev| %.3e (bound %.3e)" % (k, n_boot, worst, r.tol["values"]))
    assert n_boot > 0, "no truncation exercised"
    assert worst <= r.tol["values"]
    eng.poll_error()


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def _uniforms(seed, counter, n):
    key = _splitmix64((seed + counter * 0x9E3779B97F4A7C15) & M64)
    return np.array([(_splitmix64(key ^ ((b * 0xD1B54A32D192ED03) & M64)) >> 40) * 2.0 ** -24 for b in range(n)])


def test_splitmix_restatement_matches_random_actions():
    """The host restatement of the hash used below is mgx_random_actions' (its documented draw)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgx import _lib
    L = _lib.load()
    out = torch.zeros(256, dtype=torch.int32, device="cuda")
    ctr = torch.zeros(2, dtype=torch.int64, device="cuda")
    P = ctypes.c_void_p
    _lib.check(L.mgx_random_actions(P(out.data_ptr()), 256, 7, ctypes.c_uint64(77), P(ctr.data_ptr()), None))
    key = _splitmix64(77)
    want = [(((_splitmix64(key ^ ((i * 0xD1B54A32D192ED03) & M64)) >> 32) * 7) >> 32) for i in range(256)]
    assert out.cpu().tolist() == want


def _sampling(r):
    actor, buf, t = r.actor, r.buf, r.t
    actor.counter.zero_()
    a0, v0, lp0, lg0 = actor.act(buf, t, logits=True)
    assert actor.counter.cpu().tolist() == [1, 0]
    a1, _, _, _ = actor.act(buf, t, logits=True)
    assert actor.counter.cpu().tolist() == [2, 0]
    assert not torch.equal(a0, a1)                         # the next launch draws afresh
    actor.counter.zero_()
    a0b, v0b, lp0b, _ = actor.act(buf, t, logits=True)
    assert torch.equal(a0, a0b) and torch.equal(lp0, lp0b) and torch.equal(v0, v0b)
    l = lg0.double().cpu().numpy()
    p = np.exp(l - l.max(1, keepdims=True))
    cum = np.cumsum(p, axis=1)
    tot = cum[:, -1]
    n_near = 0
    for c, acts in ((0, a0), (1, a1)):
        u = _uniforms(actor.seed, c, N_ENVS)
        thr = u * tot
        near = (np.abs(cum - thr[:, None]) < 1e-5 * tot[:, None]).any(1)
        want = np.minimum((cum > thr[:, None]).argmax(1) + 7 * ~(cum > thr[:, None]).any(1), 6)
        got = acts.cpu().numpy()
        assert got.min() >= 0 and got.max() <= 6
        assert np.array_equal(got[~near], want[~near]), c
        n_near += int(near.sum())
    assert n_near <= 0.01 * 2 * N_ENVS
    lsm = torch.log_softmax(lg0.double().cpu(), 1).gather(1, a0.cpu()[:, None])[:, 0]
    assert float((lp0.double().cpu() - lsm).abs().max()) <= r.tol["log_probs"]
    assert torch.equal(lg0.double().cpu(), r.logits[-N_ENVS:]) and torch.equal(v0.double().cpu(), r.values[-N_ENVS:])
    assert len(set(a0.cpu().tolist())) > 1


@pytest.mark.parametrize("k", [1, 3, 4, 5, 8])
def test_sampling(k):
    """Mode 2: the action is the inverse-cdf choice of the documented u over the kernel's own logits; log-prob =
    log_softmax(logits)[action]; (seed, counter) reproduces; the launch advances the counter."""
    _sampling(_run(k))


@pytest.mark.parametrize("k", [4, 8])
def test_sampling_many_missions(k):
    """test_sampling on MULTI."""
    r = _run(k, MULTI)
    _assert_many_keys(r, k)
    _sampling(r)


def test_ring_shorter_than_stack_rejected():
    """0 < ring_rows < n_stack is MGX_ERR_INVALID (the one argument check that reads the handle)."""
    r = _run(4)
    from mgx import _lib
    e, buf, a = r.eng, r.buf, r.actor
    idx = torch.arange(4, device=e.device)
    out = torch.zeros(4, device=e.device)
    P = ctypes.c_void_p
    pol = _lib.MgxPolicy(blob_dev=a.blob.data_ptr(), mission_feat_dev=a.mission_feat.data_ptr(), mode=0)
    o = _lib.MgxActOut(values_dev=out.data_ptr())
    st = e.L.mgx_policy_act(e.h, P(buf.rows.data_ptr()), P(buf.mids.data_ptr()), P(buf.starts.data_ptr()), buf.N, 3,
                            P(idx.data_ptr()), 4, None, ctypes.byref(pol), ctypes.byref(o), None)
    assert st == 1 and b"mgx_policy_act" in e.L.mgx_last_error()


def _collector_case(k, horizon, rollouts):
    """`rollouts` collects of `horizon` steps at n_stack k with PPOConfig(fused_act=True), checked as
    test_collector_fused_act states; the bounds are _run(k)'s (4 x e_torch at that n_stack)."""
    r = _run(k)
    from mgx import MgxEngine
    from mgx.engine import gae_dones
    from mgx.ppo import PPOConfig, make_collector
    env = dict(problem="pkp", mission=None, size=6, num_objects=2)
    cfg = PPOConfig(fused_act=True, n_envs=N_ENVS, horizon=horizon, n_frames_stack=k, env=env)
    pol = _policy(k, seed=3).cuda()
    with torch.no_grad():
        pol.action_net.bias[6] = -30.0
    pol64 = copy.deepcopy(pol).cpu().double()
    eng = MgxEngine(n_envs=N_ENVS, seed=cfg.seed, n_stack=k, terminal_mode="truncated", mission_dtype=torch.uint8,
                    reward64=True, **env)
    col = make_collector(eng, pol, cfg)
    assert col.fused is not None
    col.start()
    gamma32 = torch.tensor(cfg.gamma, dtype=torch.float32)
    n_boot = 0
    for rollout in range(rollouts):
        seen = []

        class Cb:
            def __init__(self):
                self.t = 0

            def on_step(self, policy, num_timesteps):
                buf, t = col.rollout.buf, self.t
                boot = (buf.truncated[t].bool() & ~buf.terminated[t].bool()).nonzero().flatten()
                if boot.numel():
                    obs = {kk: v.clone() for kk, v in buf.gather_step(t, terminal=True, envs=boot, f32=False).items()}
                    seen.append((t, boot.clone(), obs, eng.reward64[boot].clone()))
                self.t += 1
                return True

        ro = col.collect(Cb())
        buf = ro.buf
        tt = torch.arange(cfg.horizon, device=eng.device).repeat_interleave(N_ENVS)
        ee = torch.arange(N_ENVS, device=eng.device).repeat(cfg.horizon)
        obs = buf.gather(buf.index(tt, ee), f32=False)
        logits, values = _ref64(pol64, obs)
        acts = ro.actions.reshape(-1).cpu()
        assert int(acts.min()) >= 0 and int(acts.max()) <= 6
        lp = torch.log_softmax(logits, 1).gather(1, acts[:, None])[:, 0]
        dv = float((ro.values.reshape(-1).double().cpu() - values).abs().max())
        dl = float((ro.log_probs.reshape(-1).double().cpu() - lp).abs().max())
        print("rollout %d: values max |dev| %.3e (bound %.3e), log-probs %.3e (bound %.3e)"
              % (rollout, dv, r.tol["values"], dl, r.tol["log_probs"]))
        assert dv <= r.tol["values"] and dl <= r.tol["log_probs"]
        for t, boot, tobs, raw in seen:
            _, tv = _ref64(pol64, tobs)
            want = raw.double().cpu() + float(gamma32) * tv
            got = ro.rewards[t, boot].double().cpu()
            # + the fp32 roundings of gamma * V and of the sum (half an ulp of the result each)
            slack = float(torch.finfo(torch.float32).eps) * max(1.0, float(want.abs().max()))
            assert float((got - want).abs().max()) <= float(gamma32) * r.tol["values"] + slack
            n_boot += int(boot.numel())
        last_values = col.fused.values(buf, cfg.horizon)
        adv, ret = gae_dones(ro.rewards, ro.values, buf.dones, last_values, cfg.gamma, cfg.gae_lambda)
        assert torch.equal(adv, ro.advantages) and torch.equal(ret, ro.returns)
    assert n_boot > 0, "no truncation exercised"
    eng.poll_error()


def test_collector_fused_act():
    """PPOConfig(fused_act=True): stored values / log-probs = the fp64 module's evaluate_actions on the stored
    observations and stored actions (teacher-forced), truncated steps carry gamma * V(terminal), advantages =
    gae_dones of the stored arrays bit for bit.  'done' is made improbable so that episodes run into the 36-step
    limit: four rollouts of 12 steps reach it."""
    _collector_case(4, 12, 4)


def test_collector_fused_act_stack_deeper_than_horizon():
    """The same at n_stack 6 with a horizon of 5: every stored observation's stack reaches into the previous
    rollout's ring block (the ring is 3 blocks of 5 rows), as does every truncation bootstrap's terminal stack.
    Eight rollouts pass the 36-step limit."""
    _collector_case(6, 5, 8)


def test_evaluate_policy_fused_loop():
    """The compact evaluation loop's bookkeeping: a fixed per-step action pattern gives identical (rewards,
    lengths) on the stacked path and on the path `fused=` uses; a policy evaluates to n_eval_episodes episodes."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgx import MgxEngine
    from mgx.evaluation import evaluate_policy
    from mgx.fused_policy import FusedActor
    pattern = [2, 2, 1, 2, 0, 2, 2, 6, 2, 1, 5]

    def scripted():
        state = {"i": 0}

        def fn(obs):
            assert obs["image"].shape == (N_ENVS, 12, 7, 7)          # both paths hand it the stacked observation
            a = pattern[state["i"] % len(pattern)]
            state["i"] += 1
            return torch.full((N_ENVS,), a, dtype=torch.int64, device="cuda")
        return fn

    pol = _policy(4).cuda()
    out = []
    for fused in (False, True):
        eng = MgxEngine(n_envs=N_ENVS, n_stack=4, terminal_mode="truncated", mission_dtype=torch.uint8,
                        reward64=True, **ENV)
        actor = FusedActor(pol, eng) if fused else None
        out.append(evaluate_policy(scripted(), eng, 90, return_episode_rewards=True, fused=actor))
        eng.poll_error()
    assert out[0] == out[1]
    assert len(out[0][0]) == 90 and len(set(out[0][1])) > 1
    rews, lens = evaluate_policy(pol, eng, 20, return_episode_rewards=True, fused=actor)
    assert len(rews) == len(lens) == 20
    mean_r, std_r = evaluate_policy(pol, eng, 20, fused=actor)
    assert np.isfinite(mean_r) and np.isfinite(std_r)
    eng.poll_error()
