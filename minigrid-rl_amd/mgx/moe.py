"""Mission-routed mixture of experts (mgx_policy_act_moe, include/mgx.h).

The reference's best ALL-task line is not one network but its mixture (src/policies.py MoeExtractor): a gate
reads the newest frame's 32 mission tokens, its arg-max picks one of the frozen per-task policies, and that
policy's action is played.  The gate's input is a function of the mission id alone, so here it is a table:
route[mission id] = expert.  MoEPolicy is the torch restatement on stacked observations (the readable
definition, and evaluate_policy's eager path); FusedMoEActor runs the mixture on compact rows in two launches
-- a device-side partition of the samples by expert, then one policy pass over the partition in which every
tile of 64 samples shares an expert -- so that it costs about what ONE policy costs, and fits a captured
evaluation block (GraphEvaluator).

Inference only, as in the reference: the experts are frozen, there is no bootstrap and no gradient.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .fused_policy import CompactActor, FusedActor, _params, fill_act_out, sample_addr

MAX_EXPERTS = _lib.MOE_MAX_EXPERTS
RECORD_WORDS = _lib.MOE_RECORD_WORDS
TILE = 64
REC_TILES, REC_UNROUTABLE, REC_COUNTER = 16, 17, 18     # words of the record after the 8 (start, count) pairs


def used_mission_ids():
    """The mission ids the engine can emit (those mgx_mission_text knows), ascending."""
    L, buf = _lib.load(), ctypes.create_string_buffer(64)
    return [m for m in range(256) if L.mgx_mission_text(m, buf, 64) == _lib.MGX_OK]


def check_route(route, n_experts):
    """`route` as a u8 [256] CPU tensor; ValueError unless it has 256 entries, all below n_experts."""
    r = torch.as_tensor(route).cpu()
    if r.dim() != 1 or r.numel() != 256 or r.is_floating_point() or r.dtype == torch.bool:
        raise ValueError("route must be an integer table of 256 entries (mission id -> expert)")
    r = r.to(torch.int64)
    bad = r[(r < 0) | (r >= n_experts)]
    if bad.numel():
        raise ValueError("route names expert %d, but there are %d experts" % (int(bad[0]), n_experts))
    return r.to(torch.uint8).contiguous()


def route_by_task(mapping, ids=None):
    """u8 [256]: route[id] = mapping[task_of(mission_text(id))] for every id of `ids` (default: every used id),
    e.g. {"GTG": 3, "GTO": 0, "TGL": 1, "PKP": 2} with ids=range(128), the ids of `multi`.  ValueError for an id
    of `ids` without a mission text or whose task `mapping` lacks; every other id maps to 0."""
    from .evaluation import task_of
    used = set(used_mission_ids())
    route = np.zeros(256, np.uint8)
    for m in (sorted(used) if ids is None else [int(i) for i in ids if int(i) in used]):
        task = task_of(_lib.mission_text(m))
        if task not in mapping:
            raise ValueError("mission id %d (%r) is task %s, which the mapping %s lacks"
                             % (m, _lib.mission_text(m), task, sorted(mapping)))
        route[m] = int(mapping[task])
    return torch.from_numpy(route)


@torch.no_grad()
def route_from_gate(module):
    """u8 [256] from a gating network: `module` maps tokens i64 [B, 32] to logits [B, E] (the reference's
    GatingNetwork on obs[:, -32:]); route[id] = the FIRST arg-max of its logits on row id of the 256-row token
    table (rows of unused ids are zeros)."""
    tok = torch.as_tensor(_lib.mission_tokens()).to(torch.int64)
    p = next(iter(module.parameters()), None) if hasattr(module, "parameters") else None
    logits = module(tok if p is None else tok.to(p.device))
    logits = np.asarray(logits.detach().cpu())
    if logits.ndim != 2 or logits.shape[0] != 256 or not 1 <= logits.shape[1] <= MAX_EXPERTS:
        raise ValueError("the gate must return logits [256, E] with 1 <= E <= %d, not %s"
                         % (MAX_EXPERTS, logits.shape))
    return torch.from_numpy(np.argmax(logits, axis=1).astype(np.uint8))     # numpy: the first maximum


class MoEPolicy:
    """The mixture on stacked observations: predict(obs) = the predict of expert route[mission id of the newest
    frame] -- what the reference's MoeExtractor.forward computes, with the gate tabulated per mission id.
    experts: 1..8 ActorCriticPolicy objects of equal n_stack; route: u8 [256] with values < len(experts)."""

    def __init__(self, experts, route):
        experts = list(experts)
        if not 1 <= len(experts) <= MAX_EXPERTS:
            raise ValueError("a mixture has 1..%d experts, not %d" % (MAX_EXPERTS, len(experts)))
        ks = [int(p.features_extractor.n_frames_stack) for p in experts]
        if len(set(ks)) != 1:
            raise ValueError("the experts must share one n_stack, not %s" % (ks,))
        self.experts, self.n_stack = experts, ks[0]
        self.route = check_route(route, len(experts))
        self._tokens = torch.as_tensor(_lib.mission_tokens()).to(torch.int64)      # [256, 32]
        self._dev = {}

    def _on(self, device):
        if device not in self._dev:
            self._dev[device] = (self._tokens.to(device), self.route.to(device).to(torch.int64))
        return self._dev[device]

    def mission_ids(self, obs):
        """i64 [B]: the mission id whose tokens the newest frame carries (the lowest such id)."""
        tok = obs["mission"][:, -32:].to(torch.int64)
        table, _ = self._on(tok.device)
        rows, inv = torch.unique(tok, dim=0, return_inverse=True)
        eq = (rows[:, None, :] == table[None]).all(-1)                            # [unique rows, 256]
        if not bool(eq.any(1).all()):
            raise ValueError("an observation's newest mission tokens belong to no mission id")
        return eq.to(torch.uint8).argmax(1)[inv] if eq.shape[0] else inv

    def experts_of(self, obs):
        """i64 [B]: the expert of every row of a stacked observation."""
        return self._on(obs["mission"].device)[1][self.mission_ids(obs)]

    @torch.no_grad()
    def predict(self, obs, deterministic=False):
        """i64 [B]: per row, the chosen expert's predict(row, deterministic)."""
        which = self.experts_of(obs)
        actions = torch.zeros(which.shape[0], dtype=torch.int64, device=which.device)
        for x, pol in enumerate(self.experts):
            sel = (which == x).nonzero().flatten()
            if sel.numel():
                actions[sel] = pol.predict({k: v[sel] for k, v in obs.items()}, deterministic=deterministic)
        return actions


def moe_route_reference(mids_of_samples, route, n_experts, index=None):
    """Launch 1 of mgx_policy_act_moe restated in numpy.  mids_of_samples: the mission id of every sample
    position's newest frame; route: [256].  Returns dict(pos i32 [cap]: the positions, expert after expert, -1 in
    the slots the launch never writes; list i64 [cap]: index[pos] (if index is given, else None); segments i32
    [8, 2]: (start, count) per expert; tiles; unroutable; cap = n + 63 * n_experts)."""
    mids = np.asarray(mids_of_samples).astype(np.int64).reshape(-1)
    route = np.asarray(route).astype(np.int64).reshape(-1)
    n, cap = mids.size, mids.size + (TILE - 1) * n_experts
    which = route[mids]
    pos = np.full(cap, -1, np.int32)
    seg = np.zeros((MAX_EXPERTS, 2), np.int32)
    start = tiles = 0
    for e in range(MAX_EXPERTS):
        p = np.nonzero(which == e)[0] if e < n_experts else np.zeros(0, np.int64)      # ascending: stable
        seg[e] = (start, p.size)
        pos[start:start + p.size] = p
        t = -(-p.size // TILE)
        tiles += t
        start += t * TILE
    lst = None
    if index is not None:
        idx = np.asarray(index).astype(np.int64).reshape(-1)
        lst = np.where(pos >= 0, idx[np.maximum(pos, 0)], -1)
    return dict(pos=pos, list=lst, segments=seg, tiles=tiles, unroutable=int((which >= n_experts).sum()), cap=cap,
                n=n)


def scratch_words(n_samples, n_experts):
    """mgx_policy_moe_scratch_words; ValueError where the library refuses the pair."""
    w = int(_lib.load().mgx_policy_moe_scratch_words(int(n_samples), int(n_experts)))
    if w < 0:
        raise ValueError("mgx_policy_moe_scratch_words(%d, %d) is out of range" % (n_samples, n_experts))
    return w


def scratch_views(scratch, n_samples, n_experts):
    """(record i32 [32], list i64 [cap], pos i32 [cap]): include/mgx.h's layout of a scratch tensor (views)."""
    cap = int(n_samples) + (TILE - 1) * int(n_experts)
    rec = scratch[:RECORD_WORDS]
    lst = scratch[RECORD_WORDS:RECORD_WORDS + 2 * cap].view(torch.int64)
    return rec, lst, scratch[RECORD_WORDS + 2 * cap:RECORD_WORDS + 3 * cap]


class FusedMoEActor(CompactActor):
    """FusedActor for a MoEPolicy: actions / values / log-probs of the mixture for observations of a CompactBuffer
    of `engine`, two launches each (the route, the policy pass).  Per sample bit-equal to the routed expert's own
    FusedActor at the same seed and counter.  act, values, logits, _run and index_table are CompactActor's, as
    FusedActor's are; engine, policy (= moe), sync and counter are as FusedActor's; there is no bootstrap.  After a
    call `last_route` (i32 [32], the record of include/mgx.h) holds (start, count) per expert, the live tile count
    and the unroutable count."""

    def __init__(self, moe, engine, seed=0, fused_mission=False):
        if not isinstance(moe, MoEPolicy):
            raise ValueError("FusedMoEActor needs a MoEPolicy")
        for p in moe.experts:
            _params(p)                               # ValueError before anything touches the device
        if engine is None or moe.n_stack != engine.n_stack:
            raise ValueError("the experts' n_stack %d does not match the engine's" % moe.n_stack)
        self.policy, self.engine = moe, engine
        self.K, self.E = moe.n_stack, len(moe.experts)
        self.seed = int(seed) & (2 ** 64 - 1)
        dev = engine.device
        # one packer per expert: its blob and mission table are that expert's FusedActor's
        self.experts = [FusedActor(p, engine, seed=seed, fused_mission=fused_mission) for p in moe.experts]
        self.counter = torch.zeros(2, dtype=torch.int64, device=dev)
        self.route = torch.zeros(256, dtype=torch.uint8, device=dev)
        self._pol = _lib.MgxPolicyMoe()
        self._out = _lib.MgxActOut()
        self._n = 0
        self._reserve(engine.n)
        self.sync(experts=False)

    def _reserve(self, n):
        if n > self._n:
            if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
                raise ValueError("FusedMoEActor: %d samples exceed the scratch reserved before the capture" % n)
            self.scratch = torch.zeros(scratch_words(n, self.E), dtype=torch.int32, device=self.engine.device)
            self._n = n

    @property
    def last_route(self):
        return self.scratch[:RECORD_WORDS]

    @torch.no_grad()
    def sync(self, experts=True):
        """Repack every expert's blob and mission table, and the route, from the mixture's current state."""
        if experts:
            for a in self.experts:
                a.sync()
        self.route.copy_(check_route(self.policy.route, self.E))

    def _launch(self, buf, idx, mode, values, actions, log_probs, lg, terminal):
        self._reserve(idx.numel())
        p = self._pol
        p.n_experts, p.mode, p.seed = self.E, int(mode), self.seed
        for x, a in enumerate(self.experts):
            p.blob_dev[x], p.mission_feat_dev[x] = a.blob.data_ptr(), a.mission_feat.data_ptr()
        p.route_dev, p.counter_dev = self.route.data_ptr(), self.counter.data_ptr()
        p.scratch_dev, p.scratch_words = self.scratch.data_ptr(), self.scratch.numel()
        moe_act(self.engine, buf, idx, p, self._out, values, actions, log_probs, lg, terminal=terminal)


def moe_act(engine, buf, index, p, o, values, actions=None, log_probs=None, logits=None, terminal=False):
    """mgx_policy_act_moe on the samples `index` (i64, contiguous) of `buf`; p: a filled MgxPolicyMoe; o: the
    MgxActOut to fill (policy_act's contract)."""
    fill_act_out(o, engine, index.numel(), p.mode, values, actions, log_probs, logits)
    _lib.check(engine.L.mgx_policy_act_moe(*sample_addr(engine, buf, index, bool(terminal)), ctypes.byref(p),
                                           ctypes.byref(o), engine._stream()), "mgx_policy_act_moe")
