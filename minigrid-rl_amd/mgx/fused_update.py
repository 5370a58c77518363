"""Fused PPO update (mgx_ppo_loss / mgx_adam_step, include/mgx.h, added within ABI 9).

With fused_train and fused_mission the network's forward and backward are HIP kernels, but each minibatch still
pays a torch tail: the Categorical, a dozen elementwise loss ops and their autograd mirror images, five index
launches, torch.cat of the blob and its 20-slice backward, zero_grad, clip_grad_norm_ over 25 tensors and foreach
Adam.  FusedUpdate.step replaces all of it: every step from the compact rows to the updated weights is a kernel
launch and no autograd graph is built.

ParamArena is the storage that makes this possible: the 25 parameter tensors become views of ONE flat fp32 buffer
(the 20 blob tensors first, unpadded, so arena.param[:blob_words] IS the kernels' weight blob -- no torch.cat), their
.grad views of a second one, Adam's moments two more.  mgx_policy_backward and mgx_mission_backward write their
gradients straight into the gradient buffer; mgx_adam_step clips and steps the whole buffer in two launches.

The step exists once, as FusedUpdate._minibatch: six launches on persistent memory; its callers pass what differs
(index / sel, the statistics row, the mission workspace, the policy-gradient scratch, the Adam call).

Graph-captured update (PPOConfig.graph_train).  mgx_adam_step takes lr and the bias corrections by
value, so a captured graph would bake them in; mgx_adam_step_sched reads them from a device table at a device-side
cursor.  With it FusedUpdate captures one graph of a whole epoch -- _minibatch on fixed slices of persistent index /
sel buffers -- and Trainer.train replays it once per epoch: the host draws the permutation, copies it in and launches.
"""
import ctypes

import torch

from . import _lib
from .fused_mission import mission_params
from .fused_policy import N_ACTIONS, _params, blob_layout, blob_words

ALIGN = 4                              # words: mgx_mission_* read w_ih / w_hh as 16-byte vectors
STATS = ("pg", "vf", "ent", "kl", "clipfrac", "loss", "adv_mean", "adv_std")      # mgx_ppo_loss' stats_dev order
MISSION_NAMES = ("mission.embedding", "mission.weight_ih_l0", "mission.weight_hh_l0", "mission.bias_ih_l0",
                 "mission.bias_hh_l0")


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def arena_layout(n_stack):
    """[(name, offset in words, shape)]: the 20 blob tensors in blob_layout order without padding, then the five
    mission tensors, each on an ALIGN-word boundary; and the arena's size in words."""
    out, o = [], 0
    for name, shape in blob_layout(n_stack):
        out.append((name, o, shape))
        o += int(torch.Size(shape).numel())
    for name, shape in zip(MISSION_NAMES, ((32, 32), (384, 32), (384, 128), (384,), (384,))):
        o = (o + ALIGN - 1) // ALIGN * ALIGN
        out.append((name, o, shape))
        o += int(torch.Size(shape).numel())
    return out, (o + ALIGN - 1) // ALIGN * ALIGN


class ParamArena:
    """One flat f32 buffer each for the policy's parameters, gradients, exp_avg and exp_avg_sq.  Every p.data
    becomes a view of `param`, every p.grad a view of `grad`; an existing optimizer state (moments and step) is
    taken over.  Only the architecture _params / mission_params accept, and no parameter besides those 25."""

    def __init__(self, policy):
        k, blob = _params(policy)                                # ValueError for any other architecture
        tensors = list(blob) + list(mission_params(policy))
        if {id(p) for p in policy.parameters()} != {id(p) for p in tensors}:
            raise ValueError("ParamArena: the policy has parameters outside the 20 blob tensors and the mission "
                             "Embedding + GRU")
        if any(p.dtype != torch.float32 for p in tensors):
            raise ValueError("ParamArena: fp32 parameters only")
        self.policy, self.K = policy, k
        self.layout, self.words = arena_layout(k)
        self.blob_words = blob_words(k)
        self.tensors = tensors
        dev = tensors[0].device
        self.param, self.grad, self.exp_avg, self.exp_avg_sq = (
            torch.zeros(self.words, dtype=torch.float32, device=dev) for _ in range(4))
        self.step = 0
        for p, (_, o, shape) in zip(tensors, self.layout):
            if tuple(p.shape) != tuple(shape):
                raise ValueError("ParamArena: %s is not %s" % (tuple(p.shape), tuple(shape)))
        self._foreign_state()                                    # ValueError before a parameter is moved
        with torch.no_grad():
            for p, (_, o, shape) in zip(tensors, self.layout):
                self._view(self.param, o, shape).copy_(p.data)
                if p.grad is not None:
                    self._view(self.grad, o, shape).copy_(p.grad)
                p.data = self._view(self.param, o, shape)
                p.grad = self._view(self.grad, o, shape)
        self.import_state()

    @staticmethod
    def _view(flat, o, shape):
        return flat[o:o + int(torch.Size(shape).numel())].view(shape)

    def _foreign_state(self):
        """(the optimizer's state entry of each of the 25 tensors or None, whether any of them holds a moment that
        is not the arena's own view).  ValueError for a foreign moment of the wrong shape or dtype.  Host only: 25
        pointer comparisons."""
        opt = getattr(self.policy, "optimizer", None)
        state = opt.state if opt is not None else {}
        entries = [state.get(p) or None for p in self.tensors]
        foreign = False
        for st, (name, o, shape) in zip(entries, self.layout):
            for key, flat in (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)):
                t = st.get(key) if st else None
                if t is None or (t.data_ptr() == flat.data_ptr() + 4 * o and tuple(t.shape) == tuple(shape)
                                 and t.dtype == flat.dtype):
                    continue
                if tuple(t.shape) != tuple(shape) or t.dtype != torch.float32:
                    raise ValueError("ParamArena: the optimizer's %s of %s is %s %s, not %s %s"
                                     % (key, name, t.dtype, tuple(t.shape), torch.float32, tuple(shape)))
                foreign = True
        return entries, foreign

    def import_state(self):
        """Take policy.optimizer's state over; returns whether it was foreign.  The arena owns the moments: the
        optimizer's state is either empty (the arena stays as it is), made of the arena's own views (export_state;
        the moments stay, the step count is the state's, which torch's Adam may have advanced) or foreign -- some
        exp_avg / exp_avg_sq is another tensor, as after optimizer.load_state_dict, which replaces the state's
        tensors where nn.Module.load_state_dict copies in place.  A foreign state is copied in whole: the moments of
        every tensor that has an entry, zeros for the others, the largest step count; export_state() then makes the
        optimizer's state views again.  No device work unless the state is foreign."""
        entries, foreign = self._foreign_state()
        steps = [int(st["step"]) for st in entries if st and "step" in st]
        if steps:
            self.step = max(steps)
        if not foreign:
            return False
        with torch.no_grad():
            for st, m, v in zip(entries, self.views(self.exp_avg), self.views(self.exp_avg_sq)):
                for key, view in (("exp_avg", m), ("exp_avg_sq", v)):
                    if st and st.get(key) is not None:
                        view.copy_(st[key])
                    else:
                        view.zero_()
        self.export_state()
        return True

    def views(self, flat, which=slice(None)):
        """The tensors of `flat` (one of the four buffers) in layout order."""
        return [self._view(flat, o, shape) for _, o, shape in self.layout[which]]

    def attached(self):
        """Whether every parameter and gradient is still the arena's view (the policy's load_state_dict keeps them;
        an optimizer.zero_grad(set_to_none=True) or p.data = ... elsewhere does not).  Parameters and gradients
        only: the optimizer's load_state_dict replaces the moments' tensors, which import_state() takes back."""
        for p, (_, o, _) in zip(self.tensors, self.layout):
            if p.data_ptr() != self.param.data_ptr() + 4 * o or p.grad is None or \
                    p.grad.data_ptr() != self.grad.data_ptr() + 4 * o:
                return False
        return True

    def attach_grads(self):
        """Make every p.grad the arena's view again (the torch path's zero_grad sets it to None)."""
        for p, (_, o, shape) in zip(self.tensors, self.layout):
            p.grad = self._view(self.grad, o, shape)

    def export_state(self):
        """Write the moments and the step count into policy.optimizer's state (as views of the arena: no copy), so
        that optimizer.state_dict() holds them and torch's Adam continues the run with fused_update off."""
        opt = self.policy.optimizer
        for p, (_, o, shape) in zip(self.tensors, self.layout):
            opt.state[p] = {"step": torch.tensor(float(self.step)), "exp_avg": self._view(self.exp_avg, o, shape),
                            "exp_avg_sq": self._view(self.exp_avg_sq, o, shape)}


def ppo_loss(logits, values, actions, old_values, old_log_probs, advantages, returns, clip_range, clip_range_vf,
             ent_coef, vf_coef, adv_mode=1, sel=None, adv_stats=None, out=None, scratch=None):
    """mgx_ppo_loss on torch tensors -> (g_logits f32 [B, 7], g_values f32 [B], stats f32 [8]).  logits f32 [B, 7] and
    values f32 [B] as mgx_policy_act mode 0 wrote them; the five rollout arrays (i64 actions, f32 others, contiguous)
    are read at sel[i] (i64 [B]) or at i.  out: that triple to write into.  scratch: f32, at least
    mgx_ppo_loss_scratch_words(B) words."""
    L = _lib.load()
    n = values.numel()
    dev = logits.device
    f32, check = torch.float32, _lib.check_tensor
    check(logits, "logits", f32, n * N_ACTIONS)
    check(values, "values", f32, n)
    for t in (old_values, old_log_probs, advantages, returns):
        check(t, "a rollout array", f32, None)
    check(actions, "actions", torch.int64, None)
    if sel is not None:
        check(sel, "sel", torch.int64, n)
    if sel is None and min(t.numel() for t in (actions, old_values, old_log_probs, advantages, returns)) < n:
        raise ValueError("the rollout arrays are shorter than the batch")
    if out is None:
        out = (torch.empty((n, N_ACTIONS), dtype=torch.float32, device=dev),
               torch.empty(n, dtype=torch.float32, device=dev), torch.empty(8, dtype=torch.float32, device=dev))
    g_logits, g_values, stats = out
    check(g_logits, "g_logits", f32, n * N_ACTIONS)
    check(g_values, "g_values", f32, n)
    check(stats, "stats", f32, 8)
    if scratch is None:
        scratch = torch.empty(max(int(L.mgx_ppo_loss_scratch_words(n)), 2), dtype=torch.float32, device=dev)
    a = _lib.MgxPpoLossArgs(
        logits_dev=logits.data_ptr(), values_dev=values.data_ptr(), sel_dev=None if sel is None else sel.data_ptr(),
        actions_dev=actions.data_ptr(), old_values_dev=old_values.data_ptr(),
        old_log_probs_dev=old_log_probs.data_ptr(), advantages_dev=advantages.data_ptr(),
        returns_dev=returns.data_ptr(), adv_stats_dev=None if adv_stats is None else adv_stats.data_ptr(),
        g_logits_dev=g_logits.data_ptr(), g_values_dev=g_values.data_ptr(), stats_dev=stats.data_ptr(),
        scratch_dev=scratch.data_ptr(), scratch_words=scratch.numel(), clip_range=float(clip_range),
        clip_range_vf=float(clip_range_vf) if clip_range_vf else 0.0, ent_coef=float(ent_coef),
        vf_coef=float(vf_coef), adv_mode=int(adv_mode))
    _lib.check(L.mgx_ppo_loss(n, ctypes.byref(a), _stream(dev)), "mgx_ppo_loss")
    return out


def _adam(param, grad, exp_avg, exp_avg_sq, lr, step, sched, betas, eps, max_grad_norm, grad_scale, total_norm,
          scratch):
    """mgx_adam_step with (lr, step) by value, or with sched = (table, cursor) mgx_adam_step_sched."""
    L = _lib.load()
    n, dev = param.numel(), param.device
    for t, what in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _lib.check_tensor(t, what, torch.float32, n)
    if scratch is None:
        scratch = torch.empty(max(int(L.mgx_adam_scratch_words(n)), 2), dtype=torch.float32, device=dev)
    a = _lib.MgxAdamArgs(lr=float(lr), beta1=float(betas[0]), beta2=float(betas[1]), eps=float(eps), step=int(step),
                         max_grad_norm=float(max_grad_norm) if max_grad_norm else 0.0, grad_scale=float(grad_scale))
    head = (_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), n, ctypes.byref(a))
    tail = (_ptr(total_norm), _ptr(scratch), scratch.numel(), _stream(dev))
    if sched is None:
        _lib.check(L.mgx_adam_step(*head, *tail), "mgx_adam_step")
        return
    table, cursor = sched
    if table.dim() != 2 or table.shape[1] != 2:
        raise ValueError("table must be a f32 [len, 2] tensor")
    _lib.check_tensor(table, "table", torch.float32, None, dev)
    _lib.check_tensor(cursor, "cursor", torch.int32, 2, dev)
    _lib.check(L.mgx_adam_step_sched(*head, _ptr(table), table.shape[0], _ptr(cursor), *tail), "mgx_adam_step_sched")


def adam_step(param, grad, exp_avg, exp_avg_sq, lr, step, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=0.0,
              grad_scale=1.0, total_norm=None, scratch=None):
    """mgx_adam_step on four flat contiguous f32 tensors of one length, in place; `step` counts from 1.
    total_norm: optional f32 [1] for the norm before the clip."""
    _adam(param, grad, exp_avg, exp_avg_sq, lr, step, None, betas, eps, max_grad_norm, grad_scale, total_norm, scratch)


def adam_schedule(lrs, first_step, betas=(0.9, 0.999), eps=1e-8):
    """mgx_adam_schedule -> f32 [n, 2] on the host: row i = (step_size, bc2_sqrt) of step first_step + i at learning
    rate lrs[i], formed as mgx_adam_step forms them."""
    L = _lib.load()
    lrs = [float(x) for x in lrs]
    n = len(lrs)
    a = _lib.MgxAdamArgs(lr=0.0, beta1=float(betas[0]), beta2=float(betas[1]), eps=float(eps), step=0,
                         max_grad_norm=0.0, grad_scale=1.0)
    out = (_lib.MgxAdamSched * max(n, 1))()
    _lib.check(L.mgx_adam_schedule(ctypes.byref(a), (ctypes.c_double * max(n, 1))(*lrs), int(first_step), n, out),
               "mgx_adam_schedule")
    return torch.tensor([[e.step_size, e.bc2_sqrt] for e in out[:n]], dtype=torch.float64).to(torch.float32)


def adam_step_sched(param, grad, exp_avg, exp_avg_sq, table, cursor, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=0.0,
                    grad_scale=1.0, total_norm=None, scratch=None):
    """mgx_adam_step_sched: adam_step whose (lr, step) come from the device: table f32 [len, 2] as adam_schedule
    returns it, cursor i32 [2] = {next entry, overrun count}.  Past the table's end nothing is updated and cursor[1]
    counts the call."""
    _adam(param, grad, exp_avg, exp_avg_sq, 0.0, 0, (table, cursor), betas, eps, max_grad_norm, grad_scale,
          total_norm, scratch)


MAX_GRAPHS = 8                         # captured epoch graphs kept per FusedUpdate; the oldest is evicted


class FusedUpdate:
    """One PPO minibatch step of `policy` on samples of a CompactBuffer of `engine` without torch.autograd:
    mgx_mission_forward_rows, mgx_policy_act (mode 0), mgx_ppo_loss, mgx_policy_backward, mgx_mission_backward_rows
    and Adam on a ParamArena -- _minibatch, which step() runs at once and _capture_epoch captures.  Adam's betas and
    eps are policy.optimizer's; weight decay, amsgrad and maximize are not supported (ValueError)."""

    def __init__(self, policy, engine, max_groups=0):
        from .fused_train import FusedEvaluator
        mission_params(policy)                           # ValueError before anything touches the device
        self.ev = FusedEvaluator(policy, engine, max_groups=max_groups, fused_mission=True)   # ValueError first
        g = policy.optimizer.param_groups
        if len(g) != 1 or g[0].get("weight_decay", 0) or g[0].get("amsgrad", False) or g[0].get("maximize", False):
            raise ValueError("FusedUpdate supports torch.optim.Adam's default update in one parameter group only")
        self.policy, self.engine = policy, engine
        self.arena = ParamArena(policy)
        dev, k = engine.device, self.ev.K
        L = engine.L
        self.table = torch.zeros((256 * k, 128), dtype=torch.float32, device=dev)
        self.g_table = torch.empty((256, k, 128), dtype=torch.float32, device=dev)
        self.total_norm = torch.zeros(1, dtype=torch.float32, device=dev)
        self._adam_scratch = torch.empty(int(L.mgx_adam_scratch_words(self.arena.words)), dtype=torch.float32,
                                         device=dev)
        self._loss_scratch = torch.empty(int(L.mgx_ppo_loss_scratch_words(1 << 30)), dtype=torch.float32, device=dev)
        self._batch = {}               # B -> (logits, values, g_logits, g_values), see _buffers
        self._graphs = {}              # graph_train: cache key -> (graph, stacks, rows, workspace), oldest first
        self._gbuf = None              # graph_train: the persistent buffers of one (T * N, minibatch sizes, epochs)
        self._gstream = None
        a = self.arena
        self._blob, self._g_blob = a.param[:a.blob_words], a.grad[:a.blob_words]
        self._mission = tuple(a.views(a.param, slice(20, 25)))
        self._g_mission = tuple(a.views(a.grad, slice(20, 25)))

    def prepare(self, buf):
        """FusedEvaluator.prepare: the mission ids of this rollout (one host sync); rows of other ids are zero."""
        self.ev.prepare(buf)
        self.table.zero_()
        if not self.arena.attached():
            self.arena.attach_grads()  # a torch step in between (optimizer.zero_grad) set them to None
        # torch's Adam stepped on the exported state (views: only the step count moves), or a checkpoint was loaded
        # into the live optimizer (foreign tensors: moments and step are copied in).  graph_begin reads arena.step
        # for the schedule's first step, so it runs after this.
        self.arena.import_state()
        if not self.arena.attached():
            raise RuntimeError("FusedUpdate: the policy's parameters are no longer views of the arena")

    def _buffers(self, n):
        """(logits, values, g_logits, g_values) of n samples: made once per size and kept (graphs address them)."""
        if n not in self._batch:
            f32 = dict(dtype=torch.float32, device=self.engine.device)
            self._batch[n] = (torch.empty((n, N_ACTIONS), **f32), torch.empty(n, **f32),
                              torch.empty((n, N_ACTIONS), **f32), torch.empty(n, **f32))
        return self._batch[n]

    def _minibatch(self, buf, index, sel, rollout, cfg, adv_mode, adv_stats, *, stats_out, workspace, scratch, adam):
        """The six launches of one minibatch, the same whether they run now or are being captured.  workspace: the
        mission step records; scratch: mgx_policy_backward's (None: the evaluator's own, grown on demand); adam: the
        sixth launch as a call without arguments, _adam_by_value or _adam_by_schedule bound to what it needs."""
        ev, enc = self.ev, self.ev.mission
        logits, values, g_logits, g_values = self._buffers(index.numel())
        stacks, rows = ev._stacks, ev._rows
        enc.forward_rows(stacks, self._mission, self.table, rows, workspace)
        ev.forward_raw(buf, index, self._blob, self.table, out=(logits, values))
        ppo_loss(logits, values, *rollout, cfg.clip_range, cfg.clip_range_vf, cfg.ent_coef, cfg.vf_coef,
                 adv_mode=adv_mode, sel=sel, adv_stats=adv_stats, out=(g_logits, g_values, stats_out),
                 scratch=self._loss_scratch)
        ev.backward_raw(buf, index, self._blob, self.table, g_logits, g_values, scratch=scratch,
                        out=(self._g_blob, self.g_table))
        enc.backward_rows(stacks, self._mission, self.g_table.view(-1, 128), rows, workspace, out=self._g_mission)
        adam()

    def _adam_args(self, cfg):
        a, pg = self.arena, self.policy.optimizer.param_groups[0]
        return (a.param, a.grad, a.exp_avg, a.exp_avg_sq), dict(
            betas=pg["betas"], eps=pg["eps"], max_grad_norm=cfg.max_grad_norm, total_norm=self.total_norm,
            scratch=self._adam_scratch)

    def _adam_by_value(self, cfg, lr, group):
        """All-reduce the gradient arena over `group` (the mean, through grad_scale), count arena.step, step at lr."""
        scale = 1.0
        if group is not None:
            torch.distributed.all_reduce(self.arena.grad, group=group)
            scale = 1.0 / torch.distributed.get_world_size(group)
        self.arena.step += 1
        bufs, kw = self._adam_args(cfg)
        adam_step(*bufs, lr, self.arena.step, grad_scale=scale, **kw)

    def _adam_by_schedule(self, cfg, table, cursor):
        """(lr, step) from `table` at `cursor` on the device; graph_end counts the steps."""
        bufs, kw = self._adam_args(cfg)
        adam_step_sched(*bufs, table, cursor, **kw)

    def step(self, buf, index, sel, rollout, cfg, lr, stats_out, adv_mode=1, adv_stats=None, group=None):
        """One minibatch, now.  index: i64 [B] flat compact-buffer indices (CompactBuffer.index); sel: i64 [B], the
        element of the rollout arrays each sample reads; rollout: (actions, old_values, old_log_probs, advantages,
        returns); cfg: clip_range, clip_range_vf, ent_coef, vf_coef, max_grad_norm; stats_out: f32 [8] row that
        receives mgx_ppo_loss' statistics; group: all-reduce the gradient arena (mean) before the step."""
        enc, stacks = self.ev.mission, self.ev._stacks
        ws = enc._workspace(stacks.shape[0], stacks.shape[1])
        enc._ticket += 1               # a pending autograd encode() of this encoder loses the workspace
        self._minibatch(buf, index, sel, rollout, cfg, adv_mode, adv_stats, stats_out=stats_out, workspace=ws,
                        scratch=None, adam=lambda: self._adam_by_value(cfg, lr, group))

    # ---- graph_train: one captured graph per epoch
    def _graph_buffers(self, n, sizes, n_epochs):
        """The persistent buffers the captured graphs address, for n samples in minibatches of `sizes`."""
        shape = (n, sizes, n_epochs)
        if self._gbuf is not None and self._gbuf["shape"] == shape:
            return self._gbuf
        self._graphs.clear()           # they address the old buffers
        dev, L, top = self.engine.device, self.engine.L, max(sizes)
        f32 = dict(dtype=torch.float32, device=dev)
        self._gbuf = dict(
            shape=shape,
            index=torch.zeros(n, dtype=torch.int64, device=dev), sel=torch.zeros(n, dtype=torch.int64, device=dev),
            stats=torch.zeros((len(sizes), 8), **f32), adv_stats=torch.zeros(2, **f32),
            sched=torch.zeros((n_epochs * len(sizes), 2), **f32), cursor=torch.zeros(2, dtype=torch.int32, device=dev),
            scratch=torch.empty(int(L.mgx_policy_grad_scratch_words(self.ev.K, top, self.ev.max_groups)), **f32))
        if self._gstream is None:
            self._gstream = torch.cuda.Stream(dev)
        return self._gbuf

    def _capture_epoch(self, b, buf, rollout, cfg, adv_mode):
        """Capture one epoch -- every minibatch's launches in order on one stream, none executed: _minibatch on the
        fixed slices [s, s + m) of the persistent index / sel."""
        enc, dev = self.ev.mission, self.engine.device
        stacks, rows = self.ev._stacks, self.ev._rows
        ws = torch.empty(int(enc.L.mgx_mission_workspace_words(stacks.shape[0], stacks.shape[1])),
                         dtype=torch.float32, device=dev)          # the graph's own: enc's is reallocated as it grows
        for m in set(b["shape"][1]):
            self._buffers(m)           # nothing is allocated under capture
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(self._gstream):
            g.capture_begin()
            try:
                s = 0
                for i, m in enumerate(b["shape"][1]):
                    mode = adv_mode if m > 1 else 0
                    self._minibatch(buf, b["index"][s:s + m], b["sel"][s:s + m], rollout, cfg, mode,
                                    b["adv_stats"] if mode == 2 else None, stats_out=b["stats"][i], workspace=ws,
                                    scratch=b["scratch"],
                                    adam=lambda: self._adam_by_schedule(cfg, b["sched"], b["cursor"]))
                    s += m
            finally:
                g.capture_end()
        torch.cuda.synchronize(dev)
        return g, stacks, rows, ws

    def graph_begin(self, buf, rollout, cfg, lr, n_samples, adv_mode=1, adv_stats=None):
        """After prepare(): the schedule of this train() call's n_epochs * n_minibatches steps at `lr`, from
        arena.step + 1, and a zeroed cursor, to the device; returns the epoch graph of this call's by-value
        arguments, captured now if the cache does not hold it."""
        sizes = tuple(min(cfg.batch_size, n_samples - s) for s in range(0, n_samples, cfg.batch_size))
        b = self._graph_buffers(n_samples, sizes, cfg.n_epochs)
        pg = self.policy.optimizer.param_groups[0]
        steps = cfg.n_epochs * len(sizes)
        b["sched"].copy_(adam_schedule([lr] * steps, self.arena.step + 1, betas=pg["betas"], eps=pg["eps"]))
        b["cursor"].zero_()
        if adv_mode == 2:
            b["adv_stats"].copy_(adv_stats)
        self.ev.mission._ticket += 1   # a pending autograd encode() of this encoder loses the workspace
        # everything the launches take by value: sizes and scalars, and the addresses that are not this object's own
        # (sample_addr passes the buffer's base addresses, N and R: nothing of the ring block -- that is in `index`)
        key = (tuple(self.ev._rows.tolist()), sizes, adv_mode, float(cfg.clip_range), float(cfg.clip_range_vf),
               float(cfg.ent_coef), float(cfg.vf_coef), float(cfg.max_grad_norm), tuple(pg["betas"]), float(pg["eps"]),
               id(buf), buf.rows.data_ptr(), buf.mids.data_ptr(), buf.starts.data_ptr(), buf.N, buf.R, buf.ring,
               tuple(t.data_ptr() for t in rollout))
        hit = self._graphs.get(key)
        if hit is None:
            while len(self._graphs) >= MAX_GRAPHS:
                del self._graphs[next(iter(self._graphs))]
            hit = self._graphs[key] = self._capture_epoch(b, buf, rollout, cfg, adv_mode)
        return hit[0]

    def graph_epoch(self, graph, index, sel):
        """One epoch: the permutation's index / sel into the persistent buffers, one replay -> stats f32 [n_mb, 8]."""
        b = self._gbuf
        b["index"].copy_(index)
        b["sel"].copy_(sel)
        graph.replay()
        return b["stats"].clone()

    def graph_end(self, rows):
        """After the last epoch: the step count, the optimizer state, and the one host read -> the mean statistics
        row.  MgxError if the device ran past the schedule or did not take every entry."""
        b = self._gbuf
        steps = b["sched"].shape[0]
        self.arena.step += steps
        self.arena.export_state()
        st = torch.cat([torch.cat(rows).mean(0), b["cursor"].to(torch.float32)]).tolist()
        if st[9] != 0 or st[8] != steps:
            raise _lib.MgxError("graph_train: the Adam schedule cursor ended at {%d, %d} after %d steps"
                                % (st[8], st[9], steps))
        return st[:8]
