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


def _f32(t, numel, what):
    if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != numel:
        raise ValueError("%s must be a contiguous f32 tensor of %d elements" % (what, numel))
    return t


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
        state = getattr(policy, "optimizer", None)
        state = state.state if state is not None else {}
        self.step = 0
        with torch.no_grad():
            for p, (_, o, shape) in zip(tensors, self.layout):
                if tuple(p.shape) != tuple(shape):
                    raise ValueError("ParamArena: %s is not %s" % (tuple(p.shape), tuple(shape)))
                self._view(self.param, o, shape).copy_(p.data)
                if p.grad is not None:
                    self._view(self.grad, o, shape).copy_(p.grad)
                st = state.get(p)
                if st:
                    self._view(self.exp_avg, o, shape).copy_(st["exp_avg"])
                    self._view(self.exp_avg_sq, o, shape).copy_(st["exp_avg_sq"])
                    self.step = max(self.step, int(st["step"]))
                p.data = self._view(self.param, o, shape)
                p.grad = self._view(self.grad, o, shape)

    @staticmethod
    def _view(flat, o, shape):
        return flat[o:o + int(torch.Size(shape).numel())].view(shape)

    def views(self, flat, which=slice(None)):
        """The tensors of `flat` (one of the four buffers) in layout order."""
        return [self._view(flat, o, shape) for _, o, shape in self.layout[which]]

    def attached(self):
        """Whether every parameter and gradient is still the arena's view (load_state_dict keeps them; an
        optimizer.zero_grad(set_to_none=True) or p.data = ... elsewhere does not)."""
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
    _f32(logits, n * N_ACTIONS, "logits")
    _f32(values, n, "values")
    for t in (old_values, old_log_probs, advantages, returns):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("the rollout arrays must be contiguous f32 tensors")
    if actions.dtype != torch.int64 or not actions.is_contiguous():
        raise ValueError("actions must be a contiguous i64 tensor")
    if sel is not None and (sel.dtype != torch.int64 or not sel.is_contiguous() or sel.numel() != n):
        raise ValueError("sel must be a contiguous i64 tensor of %d elements" % n)
    if sel is None and min(t.numel() for t in (actions, old_values, old_log_probs, advantages, returns)) < n:
        raise ValueError("the rollout arrays are shorter than the batch")
    if out is None:
        out = (torch.empty((n, N_ACTIONS), dtype=torch.float32, device=dev),
               torch.empty(n, dtype=torch.float32, device=dev), torch.empty(8, dtype=torch.float32, device=dev))
    g_logits, g_values, stats = out
    _f32(g_logits, n * N_ACTIONS, "g_logits")
    _f32(g_values, n, "g_values")
    _f32(stats, 8, "stats")
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


def adam_step(param, grad, exp_avg, exp_avg_sq, lr, step, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=0.0,
              grad_scale=1.0, total_norm=None, scratch=None):
    """mgx_adam_step on four flat contiguous f32 tensors of one length, in place; `step` counts from 1.
    total_norm: optional f32 [1] for the norm before the clip."""
    L = _lib.load()
    n = param.numel()
    for t, what in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _f32(t, n, what)
    dev = param.device
    if scratch is None:
        scratch = torch.empty(max(int(L.mgx_adam_scratch_words(n)), 2), dtype=torch.float32, device=dev)
    a = _lib.MgxAdamArgs(lr=float(lr), beta1=float(betas[0]), beta2=float(betas[1]), eps=float(eps), step=int(step),
                         max_grad_norm=float(max_grad_norm) if max_grad_norm else 0.0, grad_scale=float(grad_scale))
    _lib.check(L.mgx_adam_step(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), n, ctypes.byref(a),
                               _ptr(total_norm), _ptr(scratch), scratch.numel(), _stream(dev)), "mgx_adam_step")


class FusedUpdate:
    """One PPO minibatch step of `policy` on samples of a CompactBuffer of `engine` without torch.autograd:
    mgx_mission_forward, mgx_policy_act (mode 0), mgx_ppo_loss, mgx_policy_backward, mgx_mission_backward,
    mgx_adam_step on a ParamArena.  Adam's betas and eps are policy.optimizer's; weight decay, amsgrad and
    maximize are not supported (ValueError)."""

    def __init__(self, policy, engine, max_groups=0):
        from .fused_train import FusedEvaluator
        mission_params(policy)                           # ValueError before anything touches the device
        self.ev =FusedEvaluator(policy, engine, max_groups=max_groups, fused_mission=True)   # ValueError first
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
        self._batch = {}               # B -> (g_logits, g_values)
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
        st = self.policy.optimizer.state.get(self.arena.tensors[0])
        if st and "step" in st:        # torch's Adam stepped on the exported state (its moments are the arena's views)
            self.arena.step = int(st["step"])
        if not self.arena.attached():
            raise RuntimeError("FusedUpdate: the policy's parameters are no longer views of the arena")

    def step(self, buf, index, sel, rollout, cfg, lr, stats_out, adv_mode=1, adv_stats=None, group=None):
        """One minibatch.  index: i64 [B] flat compact-buffer indices (CompactBuffer.index); sel: i64 [B], the
        element of the rollout arrays each sample reads; rollout: (actions, old_values, old_log_probs, advantages,
        returns); cfg: clip_range, clip_range_vf, ent_coef, vf_coef, max_grad_norm; stats_out: f32 [8] row that
        receives mgx_ppo_loss' statistics; group: all-reduce the gradient arena (mean) before the step."""
        ev, a, enc = self.ev, self.arena, self.ev.mission
        n = index.numel()
        if n not in self._batch:
            dev = self.engine.device
            self._batch[n] = (torch.empty((n, N_ACTIONS), dtype=torch.float32, device=dev),
                              torch.empty(n, dtype=torch.float32, device=dev))
        g_logits, g_values = self._batch[n]
        stacks, rows = ev._stacks, ev._rows
        ws = enc._workspace(stacks.shape[0], stacks.shape[1])
        enc._ticket += 1               # a pending autograd encode() of this encoder loses the workspace
        feat = enc.forward_raw(stacks, self._mission, ws)
        self.table.index_copy_(0, rows, feat)
        logits, values = ev.forward_raw(buf, index, self._blob, self.table)
        ppo_loss(logits, values, *rollout, cfg.clip_range, cfg.clip_range_vf, cfg.ent_coef, cfg.vf_coef,
                 adv_mode=adv_mode, sel=sel, adv_stats=adv_stats, out=(g_logits, g_values, stats_out),
                 scratch=self._loss_scratch)
        ev.backward_raw(buf, index, self._blob, self.table, g_logits, g_values, out=(self._g_blob, self.g_table))
        g_feat = self.g_table.view(-1, 128).index_select(0, rows)
        enc.backward_raw(stacks, self._mission, g_feat, ws, out=self._g_mission)
        scale = 1.0
        if group is not None:
            torch.distributed.all_reduce(a.grad, group=group)
            scale = 1.0 / torch.distributed.get_world_size(group)
        a.step += 1
        pg = self.policy.optimizer.param_groups[0]
        adam_step(a.param, a.grad, a.exp_avg, a.exp_avg_sq, lr, a.step, betas=pg["betas"], eps=pg["eps"],
                  max_grad_norm=cfg.max_grad_norm, grad_scale=scale, total_norm=self.total_norm,
                  scratch=self._adam_scratch)
