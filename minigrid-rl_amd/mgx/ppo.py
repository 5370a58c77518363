"""Device-resident PPO rollout + training loop over the engine (BASELINE config 3).

Mirrors what the reference runs through SB3 at src/ppo.py:83-159:
`PPO(CustomPPOPolicy, vec_env, **config).learn(total_timesteps)` with the
config of hydra_configs/algorithm/ppo.yaml.  The SB3 pieces restated here
(stable_baselines3 2.x, not vendored by the reference -> parity unpinned, see
DESIGN.md §6):

  OnPolicyAlgorithm.collect_rollouts   -> RolloutCollector.collect
      per step: policy(obs) -> actions/values/log_probs; env.step; for every
      done env with TimeLimit.truncated, reward += gamma * V(terminal_obs);
      buffer.add(last_obs, actions, rewards, last_episode_starts, values,
      log_probs); last_episode_starts = dones.  At the end: V(new_obs) and
      compute_returns_and_advantage(last_values, dones)  (-> mgx_gae).
  RolloutBuffer.get(batch_size)        -> minibatches over a random permutation
      of the env-major flattened (env, t) index (swap_and_flatten).
  PPO.train                            -> Trainer.train: per-minibatch advantage
      normalisation (A - mean) / (std_unbiased + 1e-8), clipped surrogate,
      clipped value loss, entropy bonus, grad-norm clip, Adam step.
  linear_schedule (ppo.py:35-40)       -> max(progress_remaining * lr0, lr_final).

Nothing leaves the GPU: observations stay in the engine's in-place stacks and
are copied into a compact uint8 buffer (image, direction, mission tokens < 32:
exact), actions are sampled on device and fed back to mgx_step directly.

Multi-GPU: pass `group` (a torch.distributed process group,
RCCL on GPUs, gloo on CPU).  Each rank owns its own env shard.  Per optimiser
step the gradients are all-reduced (mean) in one flat bucket; per rollout one
all-reduce of the f64 advantage statistics (sum A, sum A^2, n) produced by
mgx_gae gives the global advantage mean/std (logged; used for normalisation
only with adv_norm="global").
"""
import math
from dataclasses import dataclass, field

import numpy as np
import torch

from .compact import CompactBuffer
from .engine import MgxEngine, _stats_scratch, gae, gae_dones


@dataclass
class PPOConfig:
    """hydra_configs/algorithm/ppo.yaml (model_kwargs) + single.yaml network.optim_eps."""
    n_envs: int = 16
    horizon: int = 1024                 # n_steps
    batch_size: int = 256
    n_epochs: int = 4
    gamma: float = 0.8108071290665859
    gae_lambda: float = 0.9452281119742252
    clip_range: float = 0.1
    clip_range_vf: float = 0.08341734780140342     # <= 0 -> None
    normalize_advantage: bool = True
    ent_coef: float = 0.045732238989694494
    vf_coef: float = 0.8177283657817492
    max_grad_norm: float = 0.5215982006116593
    initial_learning_rate: float = 3e-4
    final_learning_rate: float = 3e-6
    optim_eps: float = 1e-8
    n_frames_stack: int = 4
    n_eval_episodes: int = 100          # algorithm/ppo.yaml: evaluate_policy after learn (src/ppo.py:161-165)
    seed: int = 42
    adv_norm: str = "minibatch"         # "minibatch" (reference) | "global" (all-reduced stats)
    mission_cache: bool = True          # policy.py: GRU once per distinct mission stack
    layout: str = "compact"             # rollout storage: "compact" (mgx/compact.py) | "sb3" (stacked obs)
    fused_act: bool = False             # compact layout: act / bootstrap / last values through mgx_policy_act
                                        # (mgx/fused_policy.py; own sampling stream) instead of pol(gathered obs)
    fused_train: bool = False           # compact layout: Trainer.train evaluates each minibatch through mgx_policy_act
                                        # + mgx_policy_backward (mgx/fused_train.py) instead of pol.evaluate_actions
    fused_mission: bool = False         # with fused_act / fused_train: the mission Embedding + GRU through
                                        # mgx_mission_forward / mgx_mission_backward (mgx/fused_mission.py)
    env: dict = field(default_factory=lambda: dict(problem="multi", mission=2, size=8, num_objects=4))
    fused_update: bool = False          # with fused_train + fused_mission: loss, gradient clip and Adam through
                                        # mgx_ppo_loss / mgx_adam_step on one flat parameter arena, no autograd
                                        # (mgx/fused_update.py)
    graph_collect: bool = False         # with fused_act, compact layout: a whole collect() -- act, step, truncation
                                        # bootstrap (mgx_policy_bootstrap), episode statistics, last values, GAE --
                                        # is one captured graph per ring block, replayed with no host decision
    graph_train: bool = False           # with fused_update: every epoch of Trainer.train is one captured graph of all
                                        # its minibatch steps (mgx_adam_step_sched: lr and Adam's bias corrections from
                                        # a device table), replayed after the permutation is copied in

    def __post_init__(self):
        if self.fused_train and self.layout != "compact":
            raise ValueError("fused_train needs layout='compact'")
        if self.graph_train and not self.fused_update:
            raise ValueError("graph_train needs fused_update")
        if self.graph_collect and not (self.fused_act and self.layout == "compact"):
            raise ValueError("graph_collect needs fused_act and layout='compact'")
        if self.fused_mission and not (self.fused_train or self.fused_act):
            raise ValueError("fused_mission needs fused_train or fused_act")
        if self.fused_update and not (self.fused_train and self.fused_mission and self.layout == "compact"):
            raise ValueError("fused_update needs fused_train, fused_mission and layout='compact'")


def graph_refill_every(horizon):
    """The engine's refill epoch for a graph-captured collect of `horizon` steps: the largest divisor of the
    horizon that is <= 64 (the engine's default epoch), so that every rollout holds whole epochs."""
    return max(d for d in range(1, 65) if horizon % d == 0)


def linear_schedule(initial_value, final_value):
    """src/ppo.py:35-40."""
    def func(progress_remaining):
        return max(progress_remaining * initial_value, final_value)
    return func


def check_group(cfg, group):
    """The one flag rule that needs a process group."""
    if cfg.graph_train and group is not None:
        raise ValueError("graph_train does not support a data-parallel group (the all-reduce is not captured)")


def check_graph_callback(callback):
    """graph_collect replays a whole rollout: only a callback that allows being called after it is accepted."""
    if callback is not None and not getattr(callback, "deferrable", False):
        raise ValueError("graph_collect: a callback needs a host decision every step (only a callback whose "
                         "`deferrable` attribute is true, such as EvalCallback, can be called after the replay)")


def deferred_on_steps(callback, policy, num_timesteps, n_envs, horizon):
    """The on_step calls of a rollout of `horizon` steps that started at `num_timesteps`, made after the rollout
    (a `deferrable` callback under graph_collect): once per step, in order, each with the step's own count
    num_timesteps + (t + 1) * n_envs.  Returns the count of the step whose call returned False (later steps are
    not called), else None."""
    for t in range(horizon):
        now = num_timesteps + (t + 1) * n_envs
        if callback.on_step(policy, now) is False:
            return now
        policy.train(False)
    return None


def minibatch_env_t(perm, batch_size, T):
    """(env, t) of every minibatch of `perm`, a permutation of the env-major flat index i = env * T + t (SB3
    swap_and_flatten), in slices of batch_size; the last one may be shorter."""
    for s in range(0, perm.numel(), batch_size):
        idx = perm[s:s + batch_size]
        yield idx // T, idx % T


class RolloutBuffer:
    """DictRolloutBuffer with compact integer observation storage, [T, N, ...]."""

    def __init__(self, T, N, n_stack, device):
        self.T, self.N = T, N
        u8 = torch.uint8
        self.image = torch.zeros((T, N, 3 * n_stack, 7, 7), dtype=u8, device=device)
        self.direction = torch.zeros((T, N, 4 * n_stack), dtype=u8, device=device)
        self.mission = torch.zeros((T, N, 32 * n_stack), dtype=u8, device=device)
        f32 = dict(dtype=torch.float32, device=device)
        self.actions = torch.zeros((T, N), dtype=torch.int64, device=device)
        self.rewards = torch.zeros((T, N), **f32)
        self.episode_starts = torch.zeros((T, N), **f32)
        self.values = torch.zeros((T, N), **f32)
        self.log_probs = torch.zeros((T, N), **f32)
        self.advantages = None
        self.returns = None
        self.adv_stats = torch.zeros(3, dtype=torch.float64, device=device)

    def add(self, t, obs, actions, rewards, episode_starts, values, log_probs):
        self.image[t].copy_(obs["image"])
        self.direction[t].copy_(obs["direction"])
        self.mission[t].copy_(obs["mission"])
        self.actions[t].copy_(actions)
        self.rewards[t].copy_(rewards)
        self.episode_starts[t].copy_(episode_starts)
        self.values[t].copy_(values)
        self.log_probs[t].copy_(log_probs)

    def compute_returns_and_advantage(self, last_values, dones, gamma, gae_lambda):
        self.adv_stats.zero_()
        self.advantages, self.returns = gae(self.rewards, self.values, self.episode_starts, last_values, dones,
                                            gamma, gae_lambda, stats=self.adv_stats)

    def minibatches(self, batch_size, perm):
        """perm: permutation of the env-major flat index i = env * T + t (SB3 swap_and_flatten)."""
        for env, t in minibatch_env_t(perm, batch_size, self.T):
            obs = {"image": self.image[t, env], "direction": self.direction[t, env], "mission": self.mission[t, env]}
            yield (obs, self.actions[t, env], self.values[t, env], self.log_probs[t, env],
                   self.advantages[t, env], self.returns[t, env])


class RolloutCollector:
    """OnPolicyAlgorithm.collect_rollouts over an MgxEngine, entirely on device."""

    def __init__(self, engine, policy, cfg):
        self.engine, self.policy, self.cfg = engine, policy, cfg
        self.buffer = RolloutBuffer(cfg.horizon, engine.n, cfg.n_frames_stack, engine.device)
        self.last_episode_starts = torch.ones(engine.n, dtype=torch.float32, device=engine.device)
        self.last_dones = torch.zeros(engine.n, dtype=torch.bool, device=engine.device)
        self.num_timesteps = 0
        self.ep_returns, self.ep_lens = [], []
        self.stopped = False           # a callback's on_step returned False (SB3 early stop)

    def start(self):
        self.engine.reset()
        self.last_episode_starts.fill_(1.0)

    @torch.no_grad()
    def collect(self, callback=None):
        e, pol, cfg, buf = self.engine, self.policy, self.cfg, self.buffer
        pol.train(False)
        gamma32 = torch.tensor(cfg.gamma, dtype=torch.float32)
        ep_r, ep_l = [], []
        for t in range(cfg.horizon):
            obs = e.obs
            actions, values, log_probs = pol(obs)
            # the engine updates the stacks in place: store the pre-step obs first
            buf.image[t].copy_(obs["image"])
            buf.direction[t].copy_(obs["direction"])
            buf.mission[t].copy_(obs["mission"])
            e.step(actions)
            self.num_timesteps += e.n
            rewards = e.reward.clone()
            boot = (e.truncated & ~e.terminated).nonzero().flatten()
            if boot.numel():
                t_obs = {k: v.index_select(0, boot) for k, v in e.terminal_obs.items()}
                tv = pol.predict_values(t_obs)
                rewards.index_put_((boot,), rewards.index_select(0, boot) + gamma32.to(tv.device) * tv)
            buf.actions[t].copy_(actions)
            buf.rewards[t].copy_(rewards)
            buf.episode_starts[t].copy_(self.last_episode_starts)
            buf.values[t].copy_(values)
            buf.log_probs[t].copy_(log_probs)
            self.last_episode_starts.copy_(e.done.float())
            d = e.done
            ep_r.append(torch.where(d, e.ep_return, torch.nan))
            ep_l.append(torch.where(d, e.ep_len.float(), torch.nan))
            if callback is not None:       # BaseCallback.on_step, once per vectorised step
                if callback.on_step(pol, self.num_timesteps) is False:
                    # SB3 collect_rollouts: return False at once (no GAE); learn() stops
                    self.stopped = True
                    return None
                pol.train(False)
        self.last_dones.copy_(e.done)
        last_values = pol.predict_values(e.obs)
        buf.compute_returns_and_advantage(last_values, self.last_dones, cfg.gamma, cfg.gae_lambda)
        r, l = torch.stack(ep_r), torch.stack(ep_l)
        m = ~torch.isnan(r)
        self.ep_returns, self.ep_lens = r[m], l[m]
        return buf


class CompactRollout:
    """The rollout of CompactRolloutCollector: observations in the compact layout (one 148-B row
    + mission id per env-step, stacks rebuilt by mgx_gather), per-step policy outputs, GAE."""

    def __init__(self, engine, T):
        self.buf = CompactBuffer(engine, T, ring=True)      # history rows read in place (no per-rollout copy)
        self.T, self.N = T, engine.n
        dev = engine.device
        self.actions = torch.zeros((T, self.N), dtype=torch.int64, device=dev)
        self.values = torch.zeros((T, self.N), dtype=torch.float32, device=dev)
        self.log_probs = torch.zeros((T, self.N), dtype=torch.float32, device=dev)
        self.advantages = torch.zeros((T, self.N), dtype=torch.float32, device=dev)
        self.returns = torch.zeros((T, self.N), dtype=torch.float32, device=dev)
        self.adv_stats = torch.zeros(3, dtype=torch.float64, device=dev)

    @property
    def rewards(self):
        return self.buf.rewards

    def compute_returns_and_advantage(self, last_values, gamma, gae_lambda):
        """SB3 GAE over the compact dones (mgx_gae_dones: next_non_terminal(t) = 1 - done(t))."""
        self.adv_stats.zero_()
        gae_dones(self.buf.rewards, self.values, self.buf.dones, last_values, gamma, gae_lambda,
                  stats=self.adv_stats, out=(self.advantages, self.returns))

    def minibatches(self, batch_size, perm):
        """perm: permutation of the env-major flat index i = env * T + t (SB3 swap_and_flatten);
        observations gathered straight into the policy's f32 input."""
        for env, t in minibatch_env_t(perm, batch_size, self.T):
            obs = self.buf.gather(self.buf.index(t, env), f32=True)
            yield (obs, self.actions[t, env], self.values[t, env], self.log_probs[t, env],
                   self.advantages[t, env], self.returns[t, env])

    def minibatch_indices(self, batch_size, perm):
        """minibatches() without the gather: the observations named by their flat compact-buffer indices
        (CompactBuffer.index), for FusedEvaluator.evaluate_actions."""
        for env, t in minibatch_env_t(perm, batch_size, self.T):
            yield (self.buf.index(t, env), self.actions[t, env], self.values[t, env], self.log_probs[t, env],
                   self.advantages[t, env], self.returns[t, env])


class CompactRolloutCollector:
    """OnPolicyAlgorithm.collect_rollouts over an MgxEngine with the compact layout: per step one
    gather builds the policy's f32 input (VecFrameStack + preprocess_obs fused), one
    mgx_step_compact writes the next observation row, reward and done straight into the rollout
    buffer (no stack roll, no buffer copy).  With cfg.fused_act the step is _fused_step, whether
    collect() runs it step by step or, with cfg.graph_collect, replays a captured horizon of it."""

    def __init__(self, engine, policy, cfg):
        self.engine, self.policy, self.cfg = engine, policy, cfg
        self.rollout = CompactRollout(engine, cfg.horizon)
        self.num_timesteps = 0
        self.ep_returns, self.ep_lens = [], []
        self.stopped = False
        self._n_rollouts = 0
        T, N, k, dev = cfg.horizon, engine.n, engine.n_stack, engine.device
        f32 = dict(dtype=torch.float32, device=dev)
        self.fused = None
        self.graphs = None                 # cfg.graph_collect: one captured collect per ring block, made on first use
        if cfg.fused_act:
            from .fused_policy import FusedActor
            self.fused = FusedActor(policy, engine, seed=cfg.seed, fused_mission=cfg.fused_mission)
            self._ep_r, self._ep_l = torch.zeros((T, N), **f32), torch.zeros((T, N), **f32)
            self._last_values = torch.zeros(N, **f32)
            self._nan = torch.full((), math.nan, **f32)     # torch.where(..., out=) takes no scalar
        if cfg.graph_collect:
            if engine.ring_depth > 0 and T % engine.refill_every:
                raise ValueError("graph_collect: the horizon (%d) must be a multiple of the engine's refill epoch "
                                 "(refill_every = %d)" % (T, engine.refill_every))
            self.graphs = {}
            self._stream = torch.cuda.Stream(dev)
        self._obs = dict(image=torch.empty((N, 3 * k, 7, 7), **f32), direction=torch.empty((N, 4 * k), **f32),
                         mission=torch.empty((N, 32 * k), dtype=torch.uint8, device=dev))

    def start(self):
        self.engine.reset()
        self.rollout.buf.observe(0)
        self._n_rollouts = 0

    @torch.no_grad()
    def collect(self, callback=None):
        if self.fused is not None:
            return self._collect_fused(callback)
        e, pol, cfg, ro = self.engine, self.policy, self.cfg, self.rollout
        buf = ro.buf
        if self._n_rollouts:
            buf.carry_over()
        self._n_rollouts += 1
        pol.train(False)
        gamma32 = torch.tensor(cfg.gamma, dtype=torch.float32)
        ep_r, ep_l = [], []
        for t in range(cfg.horizon):
            actions, values, log_probs = pol(buf.gather_step(t, f32=True, out=self._obs))
            buf.step(t, actions)
            self.num_timesteps += e.n              # next: the torch policy's bootstrap needs a host read
            boot = (buf.truncated[t].bool() & ~buf.terminated[t].bool()).nonzero().flatten()
            if boot.numel():
                tv = pol.predict_values(buf.gather_step(t, terminal=True, envs=boot))
                r = buf.rewards[t]
                r.index_put_((boot,), r.index_select(0, boot) + gamma32.to(tv.device) * tv)
            ro.actions[t].copy_(actions)
            ro.values[t].copy_(values)
            ro.log_probs[t].copy_(log_probs)
            d = buf.dones[t].bool()
            ep_r.append(torch.where(d, e.ep_return, torch.nan))
            ep_l.append(torch.where(d, e.ep_len.float(), torch.nan))
            if callback is not None:
                if callback.on_step(pol, self.num_timesteps) is False:
                    self.stopped = True
                    return None
                pol.train(False)
        last_values = pol.predict_values(buf.gather_step(cfg.horizon, f32=True, out=self._obs))
        ro.compute_returns_and_advantage(last_values, cfg.gamma, cfg.gae_lambda)
        r, l = torch.stack(ep_r), torch.stack(ep_l)
        m = ~torch.isnan(r)
        self.ep_returns, self.ep_lens = r[m], l[m]
        return ro

    def _fused_step(self, t):
        """Step t of a fused collect, no launch needing the host: act straight into row t of the rollout arrays, the
        engine step, the device-side truncation bootstrap, the statistics of the episodes that ended (NaN elsewhere)."""
        e, ro, fused = self.engine, self.rollout, self.fused
        buf = ro.buf
        actions, _, _ = fused.act(buf, t, out=(ro.actions[t], ro.values[t], ro.log_probs[t]))
        buf.step(t, actions)
        fused.bootstrap(buf, t, self.cfg.gamma)
        d = buf.dones[t].bool()
        torch.where(d, e.ep_return, self._nan, out=self._ep_r[t])
        torch.where(d, e.ep_len.float(), self._nan, out=self._ep_l[t])

    def _fused_finish(self):
        """After the last step: the values of the final observation, then GAE."""
        cfg, ro = self.cfg, self.rollout
        self.fused.values(ro.buf, cfg.horizon, out=self._last_values)
        ro.compute_returns_and_advantage(self._last_values, cfg.gamma, cfg.gae_lambda)

    def _capture(self):
        """Capture the collect of the current ring block: every launch of a rollout, none executed.  The Python
        bookkeeping the captured calls do (engine.calls) is redone by the caller on every replay."""
        e, cfg, ro = self.engine, self.cfg, self.rollout
        e.join()
        torch.cuda.synchronize(e.device)
        calls = e.calls
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(self._stream):
            _stats_scratch(ro.adv_stats)   # the GAE scratch of the capture stream: allocated outside the graph
            g.capture_begin()
            ro.adv_stats.zero_()
            for t in range(cfg.horizon):
                self._fused_step(t)
            self._fused_finish()
            e.join()                       # the graph is self-contained: the last epoch's refill ends inside it
            g.capture_end()
        torch.cuda.synchronize(e.device)
        e.calls = calls
        return g

    def _collect_fused(self, callback):
        """collect() with cfg.fused_act: sync the weights in place, then every step's body -- one by one, with the
        callback's say after each, or as one replay of the block's graph, a deferrable callback's steps after it
         -- and one read of the episode statistics."""
        e, cfg, ro = self.engine, self.cfg, self.rollout
        buf = ro.buf
        if self.graphs is not None:
            check_graph_callback(callback)
            if e.ring_depth > 0 and e.calls % e.refill_every:
                raise ValueError("graph_collect: a rollout must start on a refill-epoch boundary (engine.calls = %d, "
                                 "refill_every = %d)" % (e.calls, e.refill_every))
        self.fused.sync()                  # the optimiser phase since the last rollout changed the weights
        self.fused.index_table(buf)        # act / values over all envs index by a view: no launch, nothing allocated
        if self._n_rollouts:
            buf.carry_over()               # the block advance (ring: no device work)
        self._n_rollouts += 1
        self.policy.train(False)
        if self.graphs is not None:
            g = self.graphs.get(buf.block)
            if g is None:
                g = self.graphs[buf.block] = self._capture()
            g.replay()
            e.calls += cfg.horizon         # what the replayed buf.step calls would have counted
            before = self.num_timesteps
            self.num_timesteps += cfg.horizon * e.n
            if callback is not None:       # the weights were constant over the rollout: every step's call, now
                at = deferred_on_steps(callback, self.policy, before, e.n, cfg.horizon)
                if at is not None:
                    self.stopped = True
                    self.num_timesteps = at
                    return None
        else:
            for t in range(cfg.horizon):
                self._fused_step(t)
                self.num_timesteps += e.n
                if callback is not None:
                    if callback.on_step(self.policy, self.num_timesteps) is False:
                        self.stopped = True
                        return None
                    self.policy.train(False)
            self._fused_finish()
        m = ~torch.isnan(self._ep_r)
        self.ep_returns, self.ep_lens = self._ep_r[m], self._ep_l[m]
        return ro


class Trainer:
    """PPO.train (SB3) + the learn() loop; optional data-parallel group."""

    def __init__(self, policy, cfg, group=None):
        self.policy, self.cfg, self.group = policy, cfg, group
        check_group(cfg, group)
        self.lr_schedule = linear_schedule(cfg.initial_learning_rate, cfg.final_learning_rate)
        self.gen = torch.Generator(device=next(policy.parameters()).device)
        self.gen.manual_seed(cfg.seed)
        self.world = torch.distributed.get_world_size(group) if group is not None else 1
        self.fused = None              # FusedEvaluator of the rollout's engine (cfg.fused_train), made on first use
        self.update = None             # FusedUpdate of the rollout's engine (cfg.fused_update), made on first use

    def global_adv_stats(self, buf):
        s = buf.adv_stats.clone()
        if self.group is not None:
            torch.distributed.all_reduce(s, group=self.group)       # the one RCCL exchange per rollout
        n = s[2].clamp_min(1)
        mean = s[0] / n
        var = (s[1] - n * mean * mean) / (n - 1).clamp_min(1)
        return mean, var.clamp_min(0).sqrt(), s

    def _allreduce_grads(self):
        if self.group is None:
            return
        grads = [p.grad for p in self.policy.parameters() if p.grad is not None]
        flat = torch.cat([g.reshape(-1) for g in grads])
        torch.distributed.all_reduce(flat, group=self.group)
        flat /= self.world
        o = 0
        for g in grads:
            g.copy_(flat[o:o + g.numel()].view_as(g))
            o += g.numel()

    def train(self, buf, progress_remaining, perm_fn=None):
        cfg, pol = self.cfg, self.policy
        pol.train(True)
        lr = self.lr_schedule(progress_remaining)
        for g in pol.optimizer.param_groups:
            g["lr"] = lr
        clip = cfg.clip_range
        clip_vf = cfg.clip_range_vf if cfg.clip_range_vf > 0 else None
        g_mean = g_std = None
        if cfg.adv_norm == "global":
            g_mean, g_std, _ = self.global_adv_stats(buf)
        n = buf.T * buf.N
        if cfg.fused_update:
            return self._train_fused_update(buf, lr, g_mean, g_std, perm_fn)
        stats = dict(pg=[], vf=[], ent=[], kl=[], clipfrac=[])
        fused = None
        if cfg.fused_train:
            if self.fused is None or self.fused.engine is not buf.buf.engine:
                from .fused_train import FusedEvaluator
                self.fused = FusedEvaluator(pol, buf.buf.engine, fused_mission=cfg.fused_mission)
            fused = self.fused
            fused.prepare(buf.buf)         # the mission ids of this rollout: the table rows each minibatch computes
        for epoch in range(cfg.n_epochs):
            perm = perm_fn(n) if perm_fn else torch.randperm(n, generator=self.gen, device=self.gen.device)
            batches = buf.minibatches if fused is None else buf.minibatch_indices
            for obs, actions, old_v, old_lp, adv, ret in batches(cfg.batch_size, perm):
                if fused is None:
                    values, log_prob, entropy = pol.evaluate_actions(obs, actions)
                else:                      # obs: flat compact-buffer indices
                    values, log_prob, entropy = fused.evaluate_actions(buf.buf, obs, actions)
                if cfg.normalize_advantage and adv.numel() > 1:
                    if g_mean is not None:
                        adv = (adv - g_mean.float()) / (g_std.float() + 1e-8)
                    else:
                        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
                ratio = torch.exp(log_prob - old_lp)
                pl1 = adv * ratio
                pl2 = adv * torch.clamp(ratio, 1 - clip, 1 + clip)
                policy_loss = -torch.min(pl1, pl2).mean()
                values_pred = values if clip_vf is None else old_v + torch.clamp(values - old_v, -clip_vf, clip_vf)
                value_loss = torch.nn.functional.mse_loss(ret, values_pred)
                entropy_loss = -torch.mean(entropy)
                loss = policy_loss + cfg.ent_coef * entropy_loss + cfg.vf_coef * value_loss
                with torch.no_grad():
                    log_ratio = log_prob - old_lp
                    stats["kl"].append(torch.mean((torch.exp(log_ratio) - 1) - log_ratio))
                    stats["clipfrac"].append(torch.mean((torch.abs(ratio - 1) > clip).float()))
                stats["pg"].append(policy_loss.detach())
                stats["vf"].append(value_loss.detach())
                stats["ent"].append(entropy_loss.detach())
                pol.optimizer.zero_grad()
                loss.backward()
                self._allreduce_grads()
                torch.nn.utils.clip_grad_norm_(pol.parameters(), cfg.max_grad_norm)
                pol.optimizer.step()
        return {k: float(torch.stack(v).mean()) for k, v in stats.items()} | {"lr": lr}

    def _train_fused_update(self, buf, lr, g_mean, g_std, perm_fn):
        """train() with cfg.fused_update: every minibatch is FusedUpdate.step (mgx/fused_update.py) -- kernel
        launches from the compact rows to the updated weights, no autograd graph; the statistics of all minibatches
        stay in one device buffer that is read once."""
        cfg = self.cfg
        eng = buf.buf.engine
        if self.update is None or self.update.engine is not eng:
            from .fused_update import FusedUpdate
            self.update = FusedUpdate(self.policy, eng)
        up = self.update
        # prepare imports an optimizer state loaded since the last call (ParamArena.import_state); graph_begin below
        # starts the Adam schedule at arena.step + 1, so it must come after
        up.prepare(buf.buf)
        T, N, bs = buf.T, buf.N, cfg.batch_size
        rollout = (buf.actions, buf.values, buf.log_probs, buf.advantages, buf.returns)
        mode, adv_stats = (1 if cfg.normalize_advantage else 0), None
        if mode and g_mean is not None:                 # adv_norm="global": the statistics stay on the device
            mode, adv_stats = 2, torch.stack([g_mean, g_std]).float()
        rows = []
        graph = None
        if cfg.graph_train:                             # one captured graph per epoch
            graph = up.graph_begin(buf.buf, rollout, cfg, lr, T * N, adv_mode=mode, adv_stats=adv_stats)
        for epoch in range(cfg.n_epochs):
            perm = perm_fn(T * N) if perm_fn else torch.randperm(T * N, generator=self.gen, device=self.gen.device)
            env, t = perm // T, perm % T
            index = buf.buf.index(t, env).to(torch.int64).contiguous()
            sel = (t * N + env).contiguous()            # the sample's element of the [T, N] rollout arrays
            if graph is not None:
                rows.append(up.graph_epoch(graph, index, sel))
                continue
            stats = torch.zeros(((perm.numel() + bs - 1) // bs, 8), dtype=torch.float32, device=eng.device)
            for i, s in enumerate(range(0, perm.numel(), bs)):
                m = min(bs, perm.numel() - s)
                up.step(buf.buf, index[s:s + m], sel[s:s + m], rollout, cfg, lr, stats[i],
                        adv_mode=mode if m > 1 else 0, adv_stats=adv_stats, group=self.group)
            rows.append(stats)
        if graph is not None:
            st = up.graph_end(rows)                     # the one host read, the schedule cursor with it
        else:
            up.arena.export_state()
            st = torch.cat(rows).mean(0).tolist()       # the one host read
        return dict(pg=st[0], vf=st[1], ent=st[2], kl=st[3], clipfrac=st[4], lr=lr)


def make_collector(engine, policy, cfg):
    """The rollout collector of cfg.layout ("compact": CompactRolloutCollector, "sb3": RolloutCollector)."""
    if cfg.layout == "compact":
        return CompactRolloutCollector(engine, policy, cfg)
    if cfg.layout == "sb3":
        return RolloutCollector(engine, policy, cfg)
    raise ValueError("layout must be 'compact' or 'sb3'")


def learn(cfg, total_timesteps, device="cuda", group=None, rank=0, log=None, callback=None, evaluate=False,
          init=None):
    """PPO(...).learn(total_timesteps, callback=callback) for one rank's env shard; returns
    (policy, history, engine).  evaluate=True then runs evaluate_policy(model, vec_env,
    n_eval_episodes) on the training engine as src/ppo.py:161-165 does (history[-1]
    gets mean_reward / std_reward).  init: continue a run (SB3's PPO.load(...) then
    learn(..., reset_num_timesteps=False)): {"policy": state_dict, "optimizer": state_dict,
    "timesteps": int, "seed_offset": int} -- the envs restart from fresh episodes seeded
    cfg.seed + seed_offset; the learning-rate schedule continues from `timesteps`."""
    from .policy import ActorCriticPolicy
    init = init or {}
    check_group(cfg, group)            # before anything touches the device
    torch.manual_seed(cfg.seed + rank + init.get("seed_offset", 0))
    graph = dict(refill_every=graph_refill_every(cfg.horizon)) if cfg.graph_collect else {}
    eng = MgxEngine(n_envs=cfg.n_envs, seed=cfg.seed + init.get("seed_offset", 0), env_index_offset=rank * cfg.n_envs,
                    n_stack=cfg.n_frames_stack, terminal_mode="truncated", mission_dtype=torch.uint8,
                    device=device, reward64=True, **graph, **cfg.env)
    pol = ActorCriticPolicy(n_stack=cfg.n_frames_stack, optim_eps=cfg.optim_eps, lr=cfg.initial_learning_rate,
                            mission_cache=cfg.mission_cache).to(eng.device)
    if "policy" in init:
        pol.load_state_dict(init["policy"])
        pol.optimizer.load_state_dict(init["optimizer"])
    if group is not None:   # identical initial weights on every rank
        for p in pol.parameters():
            torch.distributed.broadcast(p.data, 0, group=group)
    col = make_collector(eng, pol, cfg)
    tr = Trainer(pol, cfg, group)
    col.start()
    hist = []
    world = tr.world
    col.num_timesteps = int(init.get("timesteps", 0)) // world
    while col.num_timesteps * world < total_timesteps:
        buf = col.collect(callback)
        if buf is None:                # callback asked to stop (SB3: continue_training False)
            break
        progress = 1.0 - float(col.num_timesteps * world) / float(total_timesteps)
        mean, std, s = tr.global_adv_stats(buf)
        st = tr.train(buf, progress)
        st.update(timesteps=col.num_timesteps * world, adv_mean=float(mean), adv_std=float(std),
                  ep_rew_mean=float(col.ep_returns.mean()) if col.ep_returns.numel() else math.nan,
                  ep_len_mean=float(col.ep_lens.mean()) if col.ep_lens.numel() else math.nan)
        hist.append(st)
        if log:
            log(st)
    if evaluate:
        from .evaluation import evaluate_policy
        # cfg.fused_act: through the collector's FusedActor; with cfg.graph_collect as captured blocks as well (the
        # training engine's refill epoch already divides them; GraphEvaluator syncs the actor itself)
        fused = getattr(col, "fused", None)
        graph = True if fused is not None and cfg.graph_collect else None
        if fused is not None and graph is None:
            fused.sync()                               # the last optimiser phase changed the weights
        mean_r, std_r = evaluate_policy(pol, eng, cfg.n_eval_episodes, fused=fused, graph=graph)
        if hist:
            hist[-1].update(mean_reward=mean_r, std_reward=std_r)
        if log:
            log(dict(mean_reward=mean_r, std_reward=std_r, n_eval_episodes=cfg.n_eval_episodes))
    eng.poll_error()
    return pol, hist, eng
