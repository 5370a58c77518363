"""Fused actor-critic inference over compact rows (mgx_policy_act, include/mgx.h ABI 8).

`pol(obs)` in the rollout loop is a gather that expands every env's 150-byte observation into the
stacked fp32 tensor, a chain of library launches for a 47k-parameter net and a Categorical sample.
FusedActor replaces that line (and predict_values for the bootstrap / last-values passes) with ONE
HIP kernel that reads the compact rows in place and writes actions, values and log-probs: the
stacked observation is never built and nothing leaves the device.

Only the reference's own architecture is supported (policy.py DEFAULT_ARCH, net_arch 64/64 Tanh,
7 actions); anything else raises ValueError.  The kernel does not run the mission GRU: a stack's
valid slots are contiguous from the newest and share one mission id, so the mission features take
only (mission id, v = number of valid slots) values -- sync() tabulates them with the policy's own
Embedding + GRU (<= 256 * n_stack rows) next to the packed weights.  Call sync() after every
optimiser phase.

Sampling has its own documented stream (include/mgx.h): it is not torch's Categorical stream.
"""
import ctypes

import torch
from torch import nn

from . import _lib
from .policy import DEFAULT_ARCH, OBS_KEYS

N_ACTIONS = 7
FEATURES = 208            # direction 16 | image 64 | mission 128


def blob_layout(n_stack):
    """[(name, shape)] of the packed weight blob, in include/mgx.h's order."""
    k = int(n_stack)
    lay = [("direction.weight", (16, 4 * k)), ("direction.bias", (16,)),
           ("conv1.weight", (16, 3 * k, 2, 2)), ("conv1.bias", (16,)),
           ("conv2.weight", (32, 16, 2, 2)), ("conv2.bias", (32,)),
           ("conv3.weight", (64, 32, 2, 2)), ("conv3.bias", (64,))]
    for net in ("policy_net", "value_net_body"):
        lay += [(net + ".0.weight", (64, FEATURES)), (net + ".0.bias", (64,)),
                (net + ".1.weight", (64, 64)), (net + ".1.bias", (64,))]
    lay += [("action_net.weight", (N_ACTIONS, 64)), ("action_net.bias", (N_ACTIONS,)),
            ("value_net.weight", (1, 64)), ("value_net.bias", (1,))]
    return lay


def blob_offsets(n_stack):
    """{name: (offset, shape)} in fp32 words."""
    out, o = {}, 0
    for name, shape in blob_layout(n_stack):
        n = 1
        for s in shape:
            n *= s
        out[name] = (o, shape)
        o += n
    return out


def blob_words(n_stack):
    return sum(int(torch.Size(shape).numel()) for _, shape in blob_layout(n_stack))


def _bad(msg):
    raise ValueError("FusedActor supports only the reference architecture (policy.py DEFAULT_ARCH, net_arch "
                     "64/64 Tanh, %d actions): %s" % (N_ACTIONS, msg))


def _params(policy):
    """The policy's parameter tensors in blob order; ValueError for any other architecture."""
    fe = getattr(policy, "features_extractor", None)
    if fe is None or not hasattr(fe, "extractors"):
        _bad("no CustomExtractor")
    k = int(fe.n_frames_stack)
    if not 1 <= k <= 8:
        _bad("n_stack %d outside 1..8" % k)
    if tuple(fe.extractors.keys()) != OBS_KEYS:
        _bad("extractor keys %s" % (tuple(fe.extractors.keys()),))
    for key in OBS_KEYS:
        names = [type(m).__name__.replace("Conv2dGemm", "Conv2d") for m in fe.extractors[key]]
        if names != [n for n, _ in DEFAULT_ARCH[key]]:
            _bad("%s extractor is %s" % (key, names))
    img = [m for m in fe.extractors["image"] if isinstance(m, nn.Conv2d)]
    for c in img:
        if tuple(c.kernel_size) != (2, 2) or tuple(c.stride) != (1, 1) or any(c.padding) or \
                tuple(c.dilation) != (1, 1) or c.groups != 1 or c.bias is None:
            _bad("conv %s" % (c,))
    pool = [m for m in fe.extractors["image"] if isinstance(m, nn.MaxPool2d)][0]
    if pool.kernel_size not in (2, (2, 2)) or pool.stride not in (2, (2, 2)) or pool.padding not in (0, (0, 0)):
        _bad("pool %s" % (pool,))
    gru = fe.extractors["mission"][1]
    if gru.hidden_size != 128 or gru.num_layers != 1 or gru.bidirectional or not gru.batch_first:
        _bad("mission GRU %s" % (gru,))
    mods = [fe.extractors["direction"][0]] + img
    for net in (policy.policy_net, policy.value_net_body):
        kinds = [type(m) for m in net]
        if kinds != [nn.Linear, nn.Tanh, nn.Linear, nn.Tanh]:
            _bad("net_arch %s" % ([m.__name__ for m in kinds],))
        mods += [net[0], net[2]]
    mods += [policy.action_net, policy.value_net]
    tensors = []
    for m in mods:
        if m.bias is None:
            _bad("%s has no bias" % (m,))
        tensors += [m.weight, m.bias]
    for t, (name, shape) in zip(tensors, blob_layout(k)):
        if tuple(t.shape) != shape:
            _bad("%s is %s, not %s" % (name, tuple(t.shape), shape))
    return k, tensors


def pack_blob(policy):
    """f32 [mgx_policy_blob_words(n_stack)]: the policy's parameters in include/mgx.h's order."""
    _, tensors = _params(policy)
    return torch.cat([t.detach().to(torch.float32).reshape(-1) for t in tensors])


def mission_token_stacks(n_stack, tokens=None):
    """i64 [256, n_stack, 32 * n_stack]: entry [mid, v - 1] is the stacked mission input of a stack with v
    valid slots: n_stack - v zero frames, then v copies of mission mid's 32 tokens."""
    k = int(n_stack)
    tok = torch.as_tensor(_lib.mission_tokens() if tokens is None else tokens).to(torch.int64)   # [256, 32]
    out = torch.zeros((256, k, k, 32), dtype=torch.int64)
    for v in range(1, k + 1):
        out[:, v - 1, k - v:, :] = tok[:, None, :]
    return out.reshape(256, k, 32 * k)


@torch.no_grad()
def mission_table(policy, tokens=None):
    """f32 [256, n_stack, 128]: the policy's own Embedding + GRU on every (mission id, v) token stack."""
    k, _ = _params(policy)
    fe = policy.features_extractor
    dev = next(policy.parameters()).device
    st = mission_token_stacks(k, tokens).reshape(256 * k, 32 * k).to(dev)
    out = fe._mission_chunked(fe.extractors["mission"], st)
    return out.to(torch.float32).reshape(256, k, 128).contiguous()


def library_blob_words(engine, n_stack):
    """mgx_policy_blob_words(n_stack); MgxError unless the packer's layout has as many words."""
    words = int(engine.L.mgx_policy_blob_words(n_stack))
    if words != blob_words(n_stack):
        raise _lib.MgxError("blob layout mismatch: library %d words, packer %d" % (words, blob_words(n_stack)))
    return words


def sample_addr(engine, buf, index, terminal=None):
    """The leading arguments of mgx_policy_act / mgx_policy_backward: (handle, rows, mids, starts, N, ring_rows,
    index, n).  terminal False / True appends mgx_policy_act's terminal_rows (null / the buffer's)."""
    if buf.engine is not engine:
        raise ValueError("the buffer belongs to another engine")
    P = ctypes.c_void_p
    addr = (engine.h, P(buf.rows.data_ptr()), P(buf.mids.data_ptr()), P(buf.starts.data_ptr()), buf.N,
            buf.R if buf.ring else 0, P(index.data_ptr()), index.numel())
    if terminal is None:
        return addr
    return addr + (P(buf.terminal_rows.data_ptr()) if terminal else None,)


def fill_policy(p, blob, mission_feat, mode, seed=0, counter=None):
    """Fill the MgxPolicy `p`: the weights, the mode and, for the sampling mode, the stream's seed and counter."""
    p.blob_dev, p.mission_feat_dev = blob.data_ptr(), mission_feat.data_ptr()
    p.mode, p.seed, p.counter_dev = int(mode), seed, None if counter is None else counter.data_ptr()
    return p


def fill_act_out(o, engine, n, mode, values, actions=None, log_probs=None, logits=None):
    """Fill the MgxActOut `o` with the checked outputs of n samples: values f32 [n]; actions i64 [n] and log_probs
    f32 [n] only in modes 1 and 2; logits f32 [n, 7] optional."""
    dev, f32 = engine.device, torch.float32
    o.actions_dev = o.log_probs_dev = o.logits_dev = None
    o.values_dev = _lib.check_tensor(values, "values", f32, n, dev).data_ptr()
    if mode:
        o.actions_dev = _lib.check_tensor(actions, "actions", torch.int64, n, dev).data_ptr()
        o.log_probs_dev = _lib.check_tensor(log_probs, "log_probs", f32, n, dev).data_ptr()
    if logits is not None:
        o.logits_dev = _lib.check_tensor(logits, "logits", f32, n * N_ACTIONS, dev).data_ptr()
    return o


def policy_act(engine, buf, index, p, o, values, actions=None, log_probs=None, logits=None, terminal=False):
    """mgx_policy_act on the samples `index` (i64, contiguous) of `buf`; p: the MgxPolicy as fill_policy left it; o: the
    MgxActOut to fill (fill_act_out)."""
    fill_act_out(o, engine, index.numel(), p.mode, values, actions, log_probs, logits)
    _lib.check(engine.L.mgx_policy_act(*sample_addr(engine, buf, index, bool(terminal)), ctypes.byref(p),
                                       ctypes.byref(o), engine._stream()), "mgx_policy_act")


class CompactActor:
    """What the actors over compact rows share: act / values / logits for observations of a CompactBuffer of
    self.engine.  A subclass enqueues its kernels in _launch(buf, idx, mode, values, actions, log_probs, lg,
    terminal): idx i64 contiguous and not empty, the other tensors as fill_act_out takes them."""

    _table = None                                   # index_table()

    def _run(self, buf, index, mode, terminal=False, logits=False, out=None):
        """out: (actions, values, log_probs) tensors the kernel writes instead of fresh ones (actions and log_probs
        None in mode 0)."""
        e = self.engine
        if buf.engine is not e:            # also for an empty index, which launches nothing
            raise ValueError("the buffer belongs to another engine")
        idx = index.to(torch.int64).contiguous()
        n = idx.numel()
        f32 = dict(dtype=torch.float32, device=e.device)
        if out is not None:
            actions, values, log_probs = out
        else:
            values = torch.empty(n, **f32)
            actions = torch.empty(n, dtype=torch.int64, device=e.device) if mode else None
            log_probs = torch.empty(n, **f32) if mode else None
        lg = torch.empty((n, N_ACTIONS), **f32) if logits else None
        if n:
            self._launch(buf, idx, mode, values, actions, log_probs, lg, terminal)
        return actions, values, log_probs, lg

    def index_table(self, buf):
        """i64 [R, N]: row r holds the flat indices r * N + env of every env.  Once made for `buf`, act / values
        over all envs take their index from it (a view, no kernel): what every fused collect uses."""
        if self._table is None or self._table[0] is not buf:
            tab = torch.arange(buf.R * buf.N, dtype=torch.int64, device=self.engine.device).view(buf.R, buf.N)
            self._table = (buf, tab)
        return self._table[1]

    def _index(self, buf, t, envs):
        if envs is None and self._table is not None and self._table[0] is buf and isinstance(t, int):
            return self._table[1][buf.row(t)]
        return buf.index(t, buf._arange if envs is None else envs.to(torch.int64))

    def act(self, buf, t, deterministic=False, envs=None, logits=False, out=None):
        """(actions i64 [N], values f32 [N], log_probs f32 [N]) for observation t of `buf` -- what
        policy.forward(buf.gather_step(t), deterministic) returns, sampling aside (own stream).
        logits=True appends the action_net output f32 [N, 7].  out=(actions, values, log_probs): the kernel writes
        these tensors (e.g. row t of the rollout arrays) and they are what is returned."""
        a, v, lp, lg = self._run(buf, self._index(buf, t, envs), 1 if deterministic else 2, logits=logits, out=out)
        return (a, v, lp, lg) if logits else (a, v, lp)

    def values(self, buf, t, terminal=False, envs=None, out=None):
        """policy.predict_values(buf.gather_step(t, terminal=terminal, envs=envs)); out: the f32 tensor to write."""
        return self._run(buf, self._index(buf, t, envs), 0, terminal=terminal,
                         out=None if out is None else (None, out, None))[1]

    def logits(self, buf, t, terminal=False, envs=None):
        """(logits f32 [N, 7], values f32 [N]) of observation t (tests)."""
        _, v, _, lg = self._run(buf, self._index(buf, t, envs), 0, terminal=terminal, logits=True)
        return lg, v


class FusedActor(CompactActor):
    """actions / values / log-probs of `policy` for observations of a CompactBuffer of `engine`, one launch each."""

    def __init__(self, policy, engine, seed=0, fused_mission=False):
        k, _ = _params(policy)                       # ValueError before anything touches the device
        if engine is None or k != engine.n_stack:
            raise ValueError("policy n_stack %d does not match the engine's" % k)
        self.policy, self.engine = policy, engine
        self.K = k
        self.seed = int(seed) & (2 ** 64 - 1)
        dev = engine.device
        words = library_blob_words(engine, k)
        self.blob = torch.zeros(words, dtype=torch.float32, device=dev)
        self.mission_feat = torch.zeros((256, k, 128), dtype=torch.float32, device=dev)
        self.counter = torch.zeros(2, dtype=torch.int64, device=dev)      # u64 [2] (mgx_random_actions' contract)
        self._tokens = _lib.mission_tokens()
        self.mission = self._stacks = None
        if fused_mission:                            # the table through mgx_mission_forward (mgx/fused_mission.py)
            from .fused_mission import FusedMissionEncoder
            self.mission = FusedMissionEncoder(policy, dev)
            self._stacks = mission_token_stacks(k, self._tokens).reshape(256 * k, 32 * k).to(torch.uint8).to(dev)
        self._pol = _lib.MgxPolicy()
        self._out = _lib.MgxActOut()
        self._boot = _lib.MgxBootstrap()
        self.boot_list = torch.zeros(engine.n, dtype=torch.int64, device=dev)     # bootstrap()'s device work list
        self.boot_count = torch.zeros(1, dtype=torch.int32, device=dev)
        self.sync()

    @torch.no_grad()
    def sync(self):
        """Repack the blob and rebuild the mission-feature table from the policy's current parameters."""
        was = self.policy.training
        self.policy.train(False)
        self.blob.copy_(pack_blob(self.policy))
        if self.mission is not None:
            self.mission_feat.copy_(self.mission.encode(self._stacks).reshape(256, self.K, 128))
        else:
            self.mission_feat.copy_(mission_table(self.policy, self._tokens))
        self.policy.train(was)

    def _launch(self, buf, idx, mode, values, actions, log_probs, lg, terminal):
        p = fill_policy(self._pol, self.blob, self.mission_feat, mode, self.seed, self.counter)
        policy_act(self.engine, buf, idx, p, self._out, values, actions, log_probs, lg, terminal=terminal)

    def bootstrap(self, buf, t, gamma, rewards=None, values=None):
        """SB3's truncation bootstrap of step t on the device (mgx_policy_bootstrap): rewards[e] = rewards[e] +
        f32(gamma) * V(terminal observation of e) for every env with truncated & ~terminated at step t, in place in
        `rewards` (default buf.rewards[t]) -- no host read, so a captured graph can hold it.  Afterwards
        self.boot_count (i32 [1]) is the number of such envs and self.boot_list[:count] their flat indices
        (ascending env); values: optional f32 [N], V of list entry j at [j]."""
        e = self.engine
        if buf.engine is not e:
            raise ValueError("the buffer belongs to another engine")
        n = buf.N
        r = _lib.check_tensor(buf.rewards[t] if rewards is None else rewards, "rewards", torch.float32, n, e.device)
        if values is not None:
            _lib.check_tensor(values, "values", torch.float32, n, e.device)
        b, p = self._boot, fill_policy(self._pol, self.blob, self.mission_feat, 0, self.seed, self.counter)
        b.truncated_dev, b.terminated_dev = buf.truncated[t].data_ptr(), buf.terminated[t].data_ptr()
        b.rewards_dev, b.gamma = r.data_ptr(), float(gamma)
        b.list_dev, b.count_dev = self.boot_list.data_ptr(), self.boot_count.data_ptr()
        b.values_dev = None if values is None else values.data_ptr()
        P = ctypes.c_void_p
        _lib.check(e.L.mgx_policy_bootstrap(e.h, P(buf.rows.data_ptr()), P(buf.mids.data_ptr()),
                                            P(buf.starts.data_ptr()), n, buf.R if buf.ring else 0, int(buf.row(t)),
                                            P(buf.terminal_rows.data_ptr()), ctypes.byref(p), ctypes.byref(b),
                                            e._stream()), "mgx_policy_bootstrap")
        return r
