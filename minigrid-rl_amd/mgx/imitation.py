"""Behaviour cloning and DAgger from the device expert (mgx/expert.py): the reference's `algo: bc`
(src/hydra_configs/imitation.yaml: 20,000 expert episodes, batch_size 32, n_epochs 200; the `imitation` library's
BC: loss = -mean log pi(expert action | obs) - ent_weight * mean entropy, ent_weight 1e-3, Adam).

Demonstrations are collected at engine speed into a CompactBuffer: per step one mgx_expert_act (the labels and the
costs) and one mgx_step_compact -- with the expert's own action (BC) or a learner's (DAgger: the expert labels the
states the learner visits).  The loss goes through FusedEvaluator.evaluate_actions, so the forward is
mgx_policy_act on the compact rows and the gradient mgx_policy_backward (with fused_mission also the mission
kernels); the log-prob, the entropy, the mean and Adam stay in torch.  There is no fused BC loss kernel, and the
arena / graph update paths (mgx/fused_update.py) stay PPO-only.
"""
import torch

from .compact import CompactBuffer
from .expert import COST_GIVE_UP, COST_UNSUPPORTED


class Demonstrations:
    """T steps of N envs: buf (a CompactBuffer whose observation t is the state label t was given on), labels i64
    [T, N] (the expert's actions), cost i32 [T, N] (its costs), actions i64 [T, N] (what was played)."""

    def __init__(self, buf, labels, cost, actions):
        self.buf, self.labels, self.cost, self.actions = buf, labels, cost, actions
        self.T, self.N = labels.shape

    def valid(self):
        """bool [T * N]: the samples a loss may use -- the expert neither gave up nor met an unsupported mission."""
        c = self.cost.reshape(-1)
        return (c != COST_GIVE_UP) & (c != COST_UNSUPPORTED)

    def buffer_index(self, index):
        """Flat buffer indices (CompactBuffer.gather's) of the flat samples `index` (t * N + env)."""
        index = index.to(torch.int64)
        return self.buf.index(index // self.N, index % self.N)


@torch.no_grad()
def collect_demonstrations(engine, expert, T, learner=None, reset=True):
    """Step `engine` for T steps through a fresh CompactBuffer and label every state with `expert` (an ExpertActor of
    the engine).  learner None: the expert's action is played (behaviour cloning, as imitation.yaml's rollouts);
    a FusedActor of the engine: its sampled action is played and the expert only labels (DAgger).  reset: reset the
    engine first; else the rollout continues from the engine's current state (the stacks start empty).
    Returns Demonstrations."""
    if expert.engine is not engine:
        raise ValueError("the expert belongs to another engine")
    if learner is not None and getattr(learner, "engine", None) is not engine:
        raise ValueError("the learner belongs to another engine")
    T = int(T)
    if T < 1:
        raise ValueError("T must be >= 1")
    n, dev = engine.n, engine.device
    if reset:
        engine.reset()
    buf = CompactBuffer(engine, T)
    buf.observe(0)
    labels = torch.zeros((T, n), dtype=torch.int64, device=dev)
    cost = torch.zeros((T, n), dtype=torch.int32, device=dev)
    actions = labels if learner is None else torch.zeros((T, n), dtype=torch.int64, device=dev)
    for t in range(T):
        expert.expert_act(out=labels[t])
        cost[t].copy_(expert.last_cost)
        if learner is not None:
            actions[t].copy_(learner.act(buf, t, deterministic=False)[0])
        buf.step(t, actions[t])
    return Demonstrations(buf, labels, cost, actions)


def bc_loss(evaluator, demo, index, ent_weight=1e-3):
    """-mean(log_prob(label)) - ent_weight * mean(entropy) over the flat samples `index` (i64, t * N + env) of `demo`
    that the expert had an answer for (cost != -4 and != -1), through evaluator.evaluate_actions(buf, index, labels)
    (a FusedEvaluator: differentiable with respect to every parameter of its policy)."""
    index = index.to(torch.int64).reshape(-1)
    index = index[demo.valid()[index]]
    if index.numel() == 0:
        raise ValueError("bc_loss: no sample with an expert label among those given")
    labels = demo.labels.reshape(-1)[index]
    _, log_prob, entropy = evaluator.evaluate_actions(demo.buf, demo.buffer_index(index).contiguous(), labels)
    return -log_prob.mean() - ent_weight * entropy.mean()


class BCTrainer:
    """Behaviour cloning of `policy` on Demonstrations of `engine`: Adam over minibatches of bc_loss."""

    def __init__(self, policy, engine, batch_size=32, ent_weight=1e-3, lr=1e-3, fused_mission=False, seed=0):
        from .fused_train import FusedEvaluator
        if int(batch_size) < 1:
            raise ValueError("batch_size must be >= 1")
        self.policy, self.engine = policy, engine
        self.batch_size, self.ent_weight = int(batch_size), float(ent_weight)
        self.evaluator = FusedEvaluator(policy, engine, fused_mission=fused_mission)
        self.optimizer = torch.optim.Adam(policy.parameters(), lr=lr)
        self._gen = torch.Generator().manual_seed(int(seed))
        self.losses = []                  # one mean minibatch loss per epoch

    def _samples(self, demo, index):
        if demo.buf.engine is not self.engine:
            raise ValueError("the demonstrations belong to another engine")
        if index is None:
            index = torch.arange(demo.T * demo.N, device=self.engine.device)
        index = index.to(torch.int64).reshape(-1)
        return index[demo.valid()[index]]

    def loss(self, demo, index=None):
        """bc_loss of the policy as it stands on `index` (default: every sample), no gradient."""
        self.evaluator.prepare(demo.buf)
        with torch.no_grad():
            return float(bc_loss(self.evaluator, demo, self._samples(demo, index), self.ent_weight))

    @torch.no_grad()
    def accuracy(self, demo, index=None):
        """The share of `index` on which the policy's most likely action is the expert's."""
        ev = self.evaluator
        ev.prepare(demo.buf)
        index = self._samples(demo, index)
        blob, table = ev.inputs()
        logits, _ = ev.forward_raw(demo.buf, demo.buffer_index(index).contiguous(), blob.contiguous(),
                                   table.contiguous())
        return float((logits.argmax(1) == demo.labels.reshape(-1)[index]).float().mean())

    def train(self, demo, n_epochs=1, index=None):
        """n_epochs passes over `index` (default: every sample) in shuffled minibatches; returns the epochs' mean
        losses (also appended to self.losses)."""
        self.evaluator.prepare(demo.buf)
        index = self._samples(demo, index)
        if index.numel() == 0:
            raise ValueError("BCTrainer.train: no sample with an expert label")
        out = []
        for _ in range(int(n_epochs)):
            perm = torch.randperm(index.numel(), generator=self._gen).to(index.device)
            total, batches = 0.0, 0
            for lo in range(0, index.numel(), self.batch_size):
                mb = index[perm[lo:lo + self.batch_size]]
                self.optimizer.zero_grad(set_to_none=True)
                loss = bc_loss(self.evaluator, demo, mb, self.ent_weight)
                loss.backward()
                self.optimizer.step()
                total, batches = total + float(loss.detach()), batches + 1
            out.append(total / batches)
        self.losses += out
        return out
