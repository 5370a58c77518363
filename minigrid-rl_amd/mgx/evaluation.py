"""Device-resident policy evaluation over an MgxEngine: SB3's `evaluate_policy`
and `EvalCallback` as the reference calls them (src/ppo.py:145-150, 161-165;
SURVEY.md §8(f) rank 3).

SB3 2.x semantics restated (not vendored by the reference -> parity unpinned at
that boundary, pinned here against the C oracle, tests/test_evaluation.py):

  evaluate_policy(model, env, n_eval_episodes=10, deterministic=True)
    * observations = env.reset()  (SB3 VecEnv.reset: seeded on the first call,
      later calls unseeded -- MgxEngine.reset follows the same rule)
    * env i must finish episode_count_targets[i] = (n_eval_episodes + i) // n_envs
      episodes; the loop runs while any env is below its target
    * a done env below its target contributes Monitor's info["episode"]:
      r = round(sum(episode rewards), 6), l = episode length; rewards are
      appended in step order, env index order within a step
    * returns (np.mean(rewards), np.std(rewards)) or, with
      return_episode_rewards=True, (rewards, lengths) lists.

Nothing leaves the GPU per step except one bool (is any env still below its
target), the loop condition SB3 evaluates every iteration.  GraphEvaluator
 removes that read too: the accounting of a step is one launch
(mgx_eval_record), a block of steps one captured graph, and the host reads one
word per block.
"""
import ctypes
import os

import numpy as np
import torch


def _act_fn(model, deterministic):
    if hasattr(model, "predict"):
        return lambda obs: model.predict(obs, deterministic=deterministic)
    return model   # any callable obs -> actions [N] (int32/int64, on the engine's device)


def _episode_lists(rew, lens, when, extra=None):
    """The recorded episodes of [n, cap] host tables (when < 0: empty slot) in SB3's order -- by step, then env
    index: (rewards rounded as Monitor does, lengths[, extra's entries])."""
    sel = np.nonzero(when >= 0)
    order = np.lexsort((sel[0], when[sel]))              # by step, then env index
    env_i, k = sel[0][order], sel[1][order]
    episode_rewards = [round(float(rew[i, j]), 6) for i, j in zip(env_i, k)]
    episode_lengths = [int(lens[i, j]) for i, j in zip(env_i, k)]
    if extra is None:
        return episode_rewards, episode_lengths
    return episode_rewards, episode_lengths, [int(extra[i, j]) for i, j in zip(env_i, k)]


def _result(episode_rewards, episode_lengths, reward_threshold, return_episode_rewards):
    mean_reward = float(np.mean(episode_rewards)) if episode_rewards else float("nan")
    std_reward = float(np.std(episode_rewards)) if episode_rewards else float("nan")
    if reward_threshold is not None:
        assert mean_reward > reward_threshold, "Mean reward below threshold: %.2f < %.2f" % (
            mean_reward, reward_threshold)
    if return_episode_rewards:
        return episode_rewards, episode_lengths
    return mean_reward, std_reward


@torch.no_grad()
def evaluate_policy(model, engine, n_eval_episodes=10, deterministic=True, return_episode_rewards=False,
                    reward_threshold=None, fused=None, graph=None):
    """SB3 `evaluate_policy` over `engine` (an MgxEngine).  `model` is an
    ActorCriticPolicy (its predict(obs, deterministic)) or a callable obs -> actions.
    fused: a FusedActor of (model, engine) -- the same loop over a small ring CompactBuffer: per step one
    mgx_policy_act on the compact rows and one mgx_step_compact, no stacked observation (a callable `model`
    still gets the stacked observation, gathered from the rows).
    graph: with `fused`, run the loop as replays of captured blocks of steps (GraphEvaluator.evaluate): True
    builds a throwaway evaluator, a GraphEvaluator of `fused` is reused with its graphs.  The episodes returned
    are exactly this loop's, but the engine (and a sampled actor's counter) ends at a block boundary, up to
    block_steps - 1 steps further on -- see GraphEvaluator.  ValueError without `fused`, and for a callable
    `model` without predict (the stacked-observation callable cannot be captured).  None: the loop below."""
    if graph is not None and graph is not False:
        if fused is None:
            raise ValueError("graph= needs fused= (the captured block acts through mgx_policy_act)")
        if not hasattr(model, "predict"):
            raise ValueError("graph= needs a policy: a callable over stacked observations cannot be captured")
        ev = GraphEvaluator(fused) if graph is True else graph
        if getattr(ev, "actor", None) is not fused:
            raise ValueError("the GraphEvaluator belongs to another FusedActor")
        if fused.engine is not engine:
            raise ValueError("the FusedActor belongs to another engine")
        if fused.policy is not model:
            raise ValueError("the FusedActor belongs to another policy")
        return ev.evaluate(n_eval_episodes, deterministic, return_episode_rewards, reward_threshold)
    act = _act_fn(model, deterministic)
    n, dev = engine.n, engine.device
    idx = torch.arange(n, device=dev)
    targets = (n_eval_episodes + idx) // n            # episode_count_targets
    cap = max(1, (n_eval_episodes + n - 1) // n)
    counts = torch.zeros(n, dtype=torch.int64, device=dev)
    rew = torch.zeros((n, cap), dtype=torch.float64, device=dev)
    lens = torch.zeros((n, cap), dtype=torch.int64, device=dev)
    when = torch.full((n, cap), -1, dtype=torch.int64, device=dev)
    obs = engine.reset()
    if fused is not None:
        if fused.engine is not engine:
            raise ValueError("the FusedActor belongs to another engine")
        from .compact import CompactBuffer
        buf, bt = CompactBuffer(engine, max(2, engine.n_stack), ring=True), 0
        buf.observe(0)
    t = 0
    while bool((counts < targets).any()):
        if fused is None:
            actions = act(obs)
            obs = engine.step(actions)
            done = engine.done
        else:
            if hasattr(model, "predict"):
                actions = fused.act(buf, bt, deterministic=deterministic)[0]
            else:
                actions = model(buf.gather_step(bt, f32=False))
            buf.step(bt, actions)
            done = buf.dones[bt].bool()
            bt += 1
            if bt == buf.T:                              # next block of the ring (no rows move)
                buf.carry_over()
                bt = 0
        rec = done & (counts < targets)
        slot = counts.clamp(max=cap - 1)
        r = engine.reward64 if engine.reward64 is not None else engine.ep_return.double()
        # only the final step of an episode can pay (PlaygroundEnv.step), so the Monitor sum
        # of the episode's rewards is the last reward exactly
        rew[idx, slot] = torch.where(rec, r, rew[idx, slot])
        lens[idx, slot] = torch.where(rec, engine.ep_len.long(), lens[idx, slot])
        when[idx, slot] = torch.where(rec, torch.full_like(counts, t), when[idx, slot])
        counts += rec.long()
        t += 1
    episode_rewards, episode_lengths = _episode_lists(rew.cpu().numpy(), lens.cpu().numpy(), when.cpu().numpy())
    return _result(episode_rewards, episode_lengths, reward_threshold, return_episode_rewards)


def eval_record_reference(state, done, reward, ep_len, mission_id, n_eval_episodes, t):
    """mgx_eval_record (include/mgx.h) restated in numpy, in place on `state`: dict(counts i32 [n], rewards f64
    [n, cap], lengths i32 [n, cap], when i64 [n, cap], missions u8 [n, cap], remaining int).  done / reward /
    ep_len / mission_id: this step's per-env arrays; t: the step index (base + step_offset)."""
    n, cap = state["rewards"].shape
    for e in range(n):
        c = int(state["counts"][e])
        if done[e] and 0 <= c < (n_eval_episodes + e) // n and c < cap:
            state["rewards"][e, c] = reward[e]
            state["lengths"][e, c] = ep_len[e]
            state["when"][e, c] = t
            state["missions"][e, c] = mission_id[e]
            state["counts"][e] = c + 1
            state["remaining"] -= 1
    return state


class EvalRecords:
    """The device state of mgx_eval_record for the n envs of one evaluation: counts, the four [n, cap] record
    tables, the episodes still owed and the step counter the launches read."""

    def __init__(self, n, cap, device):
        from . import _lib
        self.n, self.cap, self.device = int(n), int(cap), torch.device(device)
        if self.n < 1 or self.cap < 1:
            raise ValueError("EvalRecords needs n >= 1 envs and cap >= 1 slots per env")
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.device)   # noqa: E731
        self.counts = z(self.n, torch.int32)
        self.rewards = z((self.n, self.cap), torch.float64)
        self.lengths = z((self.n, self.cap), torch.int32)
        self.when = z((self.n, self.cap), torch.int64)
        self.missions = z((self.n, self.cap), torch.uint8)
        self.remaining = z(1, torch.int32)
        self.base = z(1, torch.int64)
        self._args = _lib.MgxEvalRecordArgs()

    def begin(self, n_eval_episodes, base=0):
        """Before the first step: nothing recorded (when = -1 marks an empty slot), sum(targets) episodes owed."""
        self.counts.zero_()
        self.when.fill_(-1)
        self.remaining.fill_(int(n_eval_episodes))       # sum over e of (n_eval + e) // n
        self.base.fill_(int(base))

    def record(self, done, reward64, ep_return, ep_len, mission_id, n_eval_episodes, step_offset=0):
        """One mgx_eval_record launch on the current stream for this step's per-env arrays (reward64 f64 or None:
        ep_return f32); nothing is allocated and the host does not wait."""
        from . import _lib
        n, dev, a = self.n, self.device, self._args
        a.done_dev = _lib.check_tensor(done, "done", torch.uint8, n, dev).data_ptr()
        a.reward64_dev = None if reward64 is None else \
            _lib.check_tensor(reward64, "reward64", torch.float64, n, dev).data_ptr()
        a.ep_return_dev = None if ep_return is None else \
            _lib.check_tensor(ep_return, "ep_return", torch.float32, n, dev).data_ptr()
        a.ep_len_dev = _lib.check_tensor(ep_len, "ep_len", torch.int32, n, dev).data_ptr()
        a.mission_id_dev = _lib.check_tensor(mission_id, "mission_id", torch.uint8, n, dev).data_ptr()
        a.base_dev, a.counts_dev, a.remaining_dev = self.base.data_ptr(), self.counts.data_ptr(), \
            self.remaining.data_ptr()
        a.rewards_dev, a.lengths_dev = self.rewards.data_ptr(), self.lengths.data_ptr()
        a.when_dev, a.missions_dev = self.when.data_ptr(), self.missions.data_ptr()
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(_lib.load().mgx_eval_record(n, int(n_eval_episodes), self.cap, int(step_offset), ctypes.byref(a),
                                               stream), "mgx_eval_record")

    def episodes(self):
        """(rewards, lengths, mission ids, steps_needed) of the recorded episodes in SB3's order (one host read of
        each table); steps_needed = the last recording step + 1, the eager loop's step count."""
        when = self.when.cpu().numpy()
        r, l, m = _episode_lists(self.rewards.cpu().numpy(), self.lengths.cpu().numpy(), when,
                                 self.missions.cpu().numpy())
        return r, l, m, int(when.max()) + 1 if r else 0


class GraphEvaluator:
    """evaluate_policy(policy, engine, ..., fused=actor) as replays of captured graphs.

    One block is `block_steps` = K steps of (mgx_policy_act, mgx_step_compact, mgx_eval_record) on a ring
    CompactBuffer of K-step blocks, then `base += K` and the engine's join -- one graph per (ring block, action
    mode, n_eval_episodes), captured on first use and kept across evaluate() calls.  The host replays blocks in
    ring order and reads one word (the episodes still owed) after each; nothing else leaves the device until the
    records are read at the end.

    K must be a multiple of the engine's refill epoch (default: the epoch itself), and a block starts on an epoch
    boundary -- evaluate() resets the engine, which is one.  An evaluation engine therefore wants a small
    refill_every, e.g. MgxEngine(..., refill_every=16): episodes last at most size**2 steps, and the last block
    is run to its end.

    Over-run.  The loop stops at a block boundary, so the engine ends up to K - 1 steps past where the eager
    loop leaves it, and a sampled actor's counter with it.  The episodes recorded are exactly the eager loop's
    (the extra steps are masked by counts < target); a LATER evaluation on the same engine continues from a
    different state than the eager path's later evaluation would, deterministically for a given (seed, K)."""

    def __init__(self, actor, block_steps=None):
        from .compact import CompactBuffer
        e = actor.engine
        self.actor, self.engine = actor, e
        every = e.refill_every if e.ring_depth > 0 else 1
        self.K = int(every if block_steps is None else block_steps)
        if self.K < 1 or self.K % every:
            raise ValueError("GraphEvaluator: block_steps (%d) must be a positive multiple of the engine's refill "
                             "epoch (refill_every = %d)" % (self.K, every))
        self.buf = CompactBuffer(e, self.K, ring=True)
        n, dev = e.n, e.device
        # the flat indices of every row: a block's act launches index by a view of it (nothing allocated)
        self._index = torch.arange(self.buf.R * n, dtype=torch.int64, device=dev).view(self.buf.R, n)
        self._out = (torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.float32, device=dev),
                     torch.zeros(n, dtype=torch.float32, device=dev))
        self.records = {}                  # n_eval_episodes -> EvalRecords (the tables' size depends on it)
        self.graphs = {}                   # (ring block, mode, n_eval_episodes) -> captured graph
        self._stream = torch.cuda.Stream(dev)
        self.last = None

    def _block(self, rec, mode, n_eval):
        """The launches of the current ring block: K steps, the counter's advance, the refill's join."""
        e, buf, actor = self.engine, self.buf, self.actor
        for t in range(self.K):
            actor._run(buf, self._index[buf.row(t)], mode, out=self._out)
            buf.step(t, self._out[0])
            rec.record(buf.dones[t], e.reward64, e.ep_return, e.ep_len, buf.mids[buf.row(t)], n_eval, step_offset=t)
        rec.base.add_(self.K)
        e.join()                           # the graph is self-contained: the last epoch's refill ends inside it

    def _capture(self, rec, mode, n_eval):
        """Capture the current ring block, nothing executed; the Python bookkeeping of the captured calls
        (engine.calls) is redone by evaluate() on every replay."""
        e = self.engine
        e.join()
        torch.cuda.synchronize(e.device)
        calls = e.calls
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(self._stream):
            g.capture_begin()
            self._block(rec, mode, n_eval)
            g.capture_end()
        torch.cuda.synchronize(e.device)
        e.calls = calls
        return g

    @torch.no_grad()
    def evaluate(self, n_eval_episodes=10, deterministic=True, return_episode_rewards=False, reward_threshold=None):
        """evaluate_policy's result for the actor's policy; afterwards self.last = dict(steps: executed, a multiple
        of K; steps_needed: the eager loop's count; replays; mission_ids: per episode, in the returned order)."""
        from . import _lib
        e, buf, K = self.engine, self.buf, self.K
        n_eval = int(n_eval_episodes)
        if n_eval < 0:
            raise ValueError("n_eval_episodes must be >= 0")
        mode = 1 if deterministic else 2
        rec = self.records.get(n_eval)
        if rec is None:
            rec = self.records[n_eval] = EvalRecords(e.n, max(1, -(-n_eval // e.n)), e.device)
        self.actor.sync()
        e.reset()                          # calls = 0: an epoch boundary
        buf.c = 0
        buf.observe(0)                     # start flags set: the stale rows behind observation 0 stay masked
        rec.begin(n_eval)
        steps = replays = 0
        # every env finishes an episode within max_steps <= size**2 steps: far beyond this bound nothing can be owed
        bound = rec.cap * 16 * e.size ** 2 + K
        while n_eval > 0:
            key = (buf.block, mode, n_eval)
            g = self.graphs.get(key)
            if g is None:
                g = self.graphs[key] = self._capture(rec, mode, n_eval)
            g.replay()
            e.calls += K                   # what the replayed buf.step calls would have counted
            steps, replays = steps + K, replays + 1
            if int(rec.remaining) == 0:    # the one host read of the loop
                break
            if steps > bound:
                raise _lib.MgxError("GraphEvaluator: %d episodes still owed after %d steps"
                                    % (int(rec.remaining), steps))
            buf.carry_over()               # the next ring block (no rows move)
        rewards, lengths, missions, needed = rec.episodes()
        self.last = dict(steps=steps, steps_needed=needed, replays=replays, mission_ids=missions)
        return _result(rewards, lengths, reward_threshold, return_episode_rewards)


def summarize_missions(rewards, lengths, mission_ids):
    """Per-task and overall statistics of a vectorised evaluation's episodes -- rewards and lengths as
    evaluate_policy(..., return_episode_rewards=True) returns them, mission_ids as GraphEvaluator.last holds them:
    {"overall": stat, "per_task": {task: stat}} with stat = episodes, success_rate (reward > 0), mean_reward and
    mean_length, the shape of summarize_episodes()["per_task"] (tasks by task_of(mission_text(id)): README's
    columns).  The room count of an episode is not recorded on the device, so there is no per-cell table here:
    that remains evaluate_test_protocol's."""
    import collections
    from ._lib import mission_text
    if not len(rewards) == len(lengths) == len(mission_ids):
        raise ValueError("rewards, lengths and mission_ids must have one entry per episode")
    texts = {m: mission_text(m) for m in set(int(m) for m in mission_ids)}
    eps = [dict(reward=float(r), length=int(l), success=float(r) > 0, task=task_of(texts[int(m)]))
           for r, l, m in zip(rewards, lengths, mission_ids)]
    per_task = collections.defaultdict(list)
    for ep in eps:
        per_task[ep["task"]].append(ep)

    def stat(v):
        if not v:
            return {"episodes": 0, "success_rate": float("nan"), "mean_reward": float("nan"),
                    "mean_length": float("nan")}
        return {"episodes": len(v), "success_rate": float(np.mean([x["success"] for x in v])),
                "mean_reward": float(np.mean([x["reward"] for x in v])),
                "mean_length": float(np.mean([x["length"] for x in v]))}
    return {"overall": stat(eps), "per_task": {k: stat(v) for k, v in sorted(per_task.items())}}


# minigrid OBJECT_TO_IDX['door'] (the type byte of mgx_dump_state's grid); PlaygroundEnv's multi layouts place
# 1 / 3 / 4 doors for 2 / 3 / 4 rooms (custom_env.py:617-649, 857-928, 1299-1389)
_DOOR = 4
_ROOMS_BY_DOORS = {1: 2, 3: 3, 4: 4}
TASKS = (("go to goal", "GTG"), ("go to", "GTO"), ("pick up", "PKP"), ("toggle", "TGL"), ("drop", "DRP"),
         ("move", "MOV"))


def task_of(mission_text):
    """README.md:54-65's task columns from a mission text ('go to goal' before 'go to')."""
    for prefix, name in TASKS:
        if mission_text.startswith(prefix):
            return name
    return mission_text


@torch.no_grad()
def evaluate_test_protocol(model, engine, n_episodes=1000, deterministic=True, progress=None):
    """The reference's benchmark protocol, `test()` (src/ppo.py:185-230; README.md:54-65 "Benchmark (1k ep)"):
    ONE env, make_vec_env(make_env, n_envs=1, seed=cfg.seed, vec_env_cls=DummyVecEnv) + VecTransposeImage +
    VecFrameStack, and per episode

        obs = vec_env.reset(); while not done: action = model.predict(obs, deterministic); obs, r, done = step

    with the episode's reward summed.  `engine` must be a fresh 1-env MgxEngine of the tested config (its first
    reset is make_vec_env's seeded one: PCG64(seed), CPython random = MT19937(seed) from PlaygroundEnv.__init__,
    custom_env.py:82).  The single MT19937 stream advances across the episodes, so missions and room counts vary
    from episode to episode, and every episode skips one generated episode: DummyVecEnv auto-resets the env when
    it is done (one episode generated), and test()'s next vec_env.reset() -- unseeded, both streams continuing --
    generates another (MgxEngine.reset after the first is that unseeded reset).
    Returns one dict per episode: reward (f64 sum), length, success (reward > 0: the mission was completed),
    mission_id, mission text, task (README's column), rooms (multi: 2 / 3 / 4 from the door count; else 0).
    `progress(k)`, if given, is called after every episode (k episodes done)."""
    from ._lib import mission_text
    if engine.n != 1:
        raise ValueError("the test() protocol steps ONE env (src/ppo.py:201-206: n_envs=1)")
    act = _act_fn(model, deterministic)
    out, texts = [], {}
    for _ in range(n_episodes):
        obs = engine.reset()
        st = engine.dump_state()
        mid = int(st["mission_id"][0])
        doors = int((st["grid"][0, :, :, 0] == _DOOR).sum())
        if mid not in texts:
            texts[mid] = mission_text(mid)
        total, length = 0.0, 0
        while True:
            obs = engine.step(act(obs))
            length += 1
            r = engine.reward64 if engine.reward64 is not None else engine.reward.double()
            total += float(r[0])
            if bool(engine.done[0]):
                break
        out.append(dict(reward=total, length=length, success=total > 0, mission_id=mid, mission=texts[mid],
                        task=task_of(texts[mid]), rooms=_ROOMS_BY_DOORS.get(doors, 0)))
        if progress is not None:
            progress(len(out))
    return out


def summarize_episodes(eps):
    """Success rate overall and per (task, rooms) cell, and the cell histogram, of evaluate_test_protocol's
    episodes."""
    import collections
    cells = collections.defaultdict(list)
    for e in eps:
        cells["%s/%d rooms" % (e["task"], e["rooms"])].append(e)
    per_task = collections.defaultdict(list)
    for e in eps:
        per_task[e["task"]].append(e)

    def stat(v):
        return {"episodes": len(v), "success_rate": float(np.mean([x["success"] for x in v])),
                "mean_reward": float(np.mean([x["reward"] for x in v])),
                "mean_length": float(np.mean([x["length"] for x in v]))}
    return {"overall": stat(eps), "per_task": {k: stat(v) for k, v in sorted(per_task.items())},
            "per_cell": {k: stat(v) for k, v in sorted(cells.items())},
            "cell_histogram": {k: len(v) for k, v in sorted(cells.items())},
            "distinct_missions": len({e["mission_id"] for e in eps})}


class EvalCallback:
    """SB3 EvalCallback(eval_env, best_model_save_path, eval_freq, n_eval_episodes,
    deterministic=True) for mgx.ppo.learn: every `eval_freq` vectorised steps of the
    training engine, evaluate on `eval_engine` and keep the best policy weights.

    The reference passes its training vec_env as eval_env (src/ppo.py:145), which makes
    SB3 reset the training envs mid-rollout; here evaluation runs on its own engine
    (SB3's documented usage) so the training rollout is not disturbed.

    fused: evaluate through a FusedActor(policy, eval_engine, fused_mission=fused_mission), made on the first
    on_step and synced before every evaluation; graph (needs fused): through a GraphEvaluator of that actor as
    well -- the eval engine then wants a small refill_every (GraphEvaluator).

    deferrable: the callback reads only the policy's weights and its own eval engine, so a collector that cannot
    stop between steps (PPOConfig.graph_collect) may call on_step for every step of a rollout after the rollout:
    the weights do not change within one, and every evaluation returns what it would have returned mid-rollout."""

    deferrable = True

    def __init__(self, eval_engine, best_model_save_path=None, eval_freq=10000, n_eval_episodes=5,
                 deterministic=True, log=None, callback_on_new_best=None, fused=False, graph=False,
                 fused_mission=False):
        if graph and not fused:
            raise ValueError("EvalCallback: graph=True needs fused=True")
        self.fused, self.graph, self.fused_mission = bool(fused), bool(graph), bool(fused_mission)
        self.actor = self.evaluator = None     # made on the first on_step (they need the policy)
        self.eval_engine = eval_engine
        self.callback_on_new_best = callback_on_new_best   # SB3: its on_step() False stops training
        self.best_model_save_path = best_model_save_path
        self.eval_freq = int(eval_freq)
        self.n_eval_episodes = int(n_eval_episodes)
        self.deterministic = deterministic
        self.log = log
        self.n_calls = 0
        self.best_mean_reward = -float("inf")
        self.last_mean_reward = -float("inf")
        self.evaluations = []      # (num_timesteps, mean_reward, std_reward, mean_ep_length)

    def on_step(self, policy, num_timesteps):
        self.n_calls += 1
        if self.eval_freq <= 0 or self.n_calls % self.eval_freq != 0:
            return True
        was_training = policy.training
        policy.train(False)
        if self.fused and (self.actor is None or self.actor.policy is not policy):
            from .fused_policy import FusedActor
            self.actor = FusedActor(policy, self.eval_engine, fused_mission=self.fused_mission)
            self.evaluator = GraphEvaluator(self.actor) if self.graph else None
        elif self.fused and self.evaluator is None:
            self.actor.sync()              # the weights since the last evaluation (GraphEvaluator syncs itself)
        rews, lens = evaluate_policy(policy, self.eval_engine, self.n_eval_episodes, self.deterministic,
                                     return_episode_rewards=True, fused=self.actor, graph=self.evaluator)
        policy.train(was_training)
        mean_r, std_r = float(np.mean(rews)), float(np.std(rews))
        self.last_mean_reward = mean_r
        self.evaluations.append((num_timesteps, mean_r, std_r, float(np.mean(lens))))
        if self.log:
            self.log(dict(eval_timesteps=num_timesteps, eval_mean_reward=mean_r, eval_std_reward=std_r,
                          eval_mean_ep_length=float(np.mean(lens))))
        if mean_r > self.best_mean_reward:
            self.best_mean_reward = mean_r
            if self.best_model_save_path is not None:
                os.makedirs(self.best_model_save_path, exist_ok=True)
                torch.save(policy.state_dict(), os.path.join(self.best_model_save_path, "best_model.pt"))
            if self.callback_on_new_best is not None:
                return bool(self.callback_on_new_best.on_step(self))
        return True


class StopTrainingOnRewardThreshold:
    """SB3 StopTrainingOnRewardThreshold, used as EvalCallback(callback_on_new_best=...):
    training stops once the best mean evaluation reward reaches `reward_threshold`."""

    def __init__(self, reward_threshold):
        self.reward_threshold = float(reward_threshold)

    def on_step(self, parent):
        return bool(parent.best_mean_reward < self.reward_threshold)
