"""Fused policy gradient for the PPO update (mgx_policy_backward, include/mgx.h ABI 9).

`pol.evaluate_actions(gathered obs, actions)` in Trainer.train expands every sampled observation into
the stacked fp32 tensor and runs the net as a chain of library launches, forwards and backwards.
FusedEvaluator replaces that call and its autograd graph: the forward is mgx_policy_act (mode 0, logits)
on the compact rows in place, the backward is mgx_policy_backward, both inside one
torch.autograd.Function whose inputs are the packed weight blob and the mission-feature table.  Both
inputs are built differentiably -- the blob as torch.cat of the parameters in blob_layout order, the
table by the policy's own Embedding + GRU -- so autograd delivers p.grad for every parameter, Embedding
and GRU included.  The Categorical on the logits, the loss, the clipping and Adam stay in torch (mgx/fused_update.py
replaces them too, and the autograd graph with them, on the raw calls below).

The table is computed only for the mission ids that occur in the buffer (prepare(), once per train()
call); the other rows stay zero and are never read for a sample.  The blob and the table are rebuilt
for every evaluate_actions call: the weights change at every optimiser step.
"""
import ctypes

import torch

from . import _lib
from .fused_policy import (N_ACTIONS, _params, fill_policy, library_blob_words, mission_token_stacks, policy_act,
                           sample_addr)


def differentiable_blob(tensors):
    """f32 [blob words]: torch.cat of the parameters in blob order, connected to them by autograd."""
    return torch.cat([t.to(torch.float32).reshape(-1) for t in tensors])


def mission_table_rows(policy, rows, stacks, encoder=None):
    """f32 [256, n_stack, 128]: fused_policy.mission_table restricted to the flat rows `rows` (i64 [r], row =
    mid * n_stack + v - 1; `stacks` i64 [r, 32 * n_stack] their token stacks), the rest zero -- with autograd.
    With `encoder` (a FusedMissionEncoder; `stacks` then u8) the rows come from the fused mission kernels."""
    k, _ = _params(policy)
    fe = policy.features_extractor
    if encoder is not None:
        out = encoder.encode(stacks)
    else:
        out = fe._mission_chunked(fe.extractors["mission"], stacks).to(torch.float32)
    tab = torch.zeros((256 * k, 128), dtype=torch.float32, device=out.device)
    return tab.index_copy(0, rows, out).reshape(256, k, 128)


class _PolicyFn(torch.autograd.Function):
    """(blob, mission_feat) -> (logits [B, 7], values [B]) of the samples `index` of `buf`."""

    @staticmethod
    def forward(ctx, blob, mission_feat, ev, buf, index):
        blob, mission_feat = blob.detach().contiguous(), mission_feat.detach().contiguous()
        ctx.ev, ctx.buf, ctx.index = ev, buf, index
        ctx.save_for_backward(blob, mission_feat)
        logits, values = ev.forward_raw(buf, index, blob, mission_feat)
        return logits, values

    @staticmethod
    def backward(ctx, g_logits, g_values):
        blob, mission_feat = ctx.saved_tensors
        n = ctx.index.numel()
        dev = blob.device
        if g_logits is None:
            g_logits = torch.zeros((n, N_ACTIONS), dtype=torch.float32, device=dev)
        if g_values is None:
            g_values = torch.zeros(n, dtype=torch.float32, device=dev)
        gb, gm = ctx.ev.backward_raw(ctx.buf, ctx.index, blob, mission_feat, g_logits, g_values)
        return gb, gm, None, None, None


class FusedEvaluator:
    """evaluate_actions of `policy` for samples of a CompactBuffer of `engine`, differentiable with respect to
    every parameter.  max_groups: mgx_policy_grad.max_groups (0: the library's default).  fused_mission: the table's
    rows come from mgx_mission_forward / mgx_mission_backward (mgx/fused_mission.py), not from MIOpen's GRU."""

    def __init__(self, policy, engine, max_groups=0, fused_mission=False):
        k, _ = _params(policy)                       # ValueError before anything touches the device
        if engine is None or k != engine.n_stack:
            raise ValueError("policy n_stack %d does not match the engine's" % k)
        self.policy, self.engine, self.K = policy, engine, k
        self.max_groups = int(max_groups)
        self.words = library_blob_words(engine, k)
        self._stacks_all = mission_token_stacks(k, _lib.mission_tokens()).reshape(256 * k, 32 * k)
        self.mission = None
        if fused_mission:
            from .fused_mission import FusedMissionEncoder
            self.mission = FusedMissionEncoder(policy, engine.device)
            self._stacks_all = self._stacks_all.to(torch.uint8)       # the kernels read the token stacks as u8
        self._stacks_all = self._stacks_all.to(engine.device)
        self._rows = self._stacks = None
        self._scratch = None
        self._pol, self._out, self._grad = _lib.MgxPolicy(), _lib.MgxActOut(), _lib.MgxPolicyGrad()

    def prepare(self, buf):
        """Find the mission ids held by `buf` (one host sync): the table rows later calls compute."""
        mids = torch.unique(buf.mids).to(torch.int64)
        k = self.K
        self._rows = (mids[:, None] * k + torch.arange(k, device=mids.device)[None, :]).reshape(-1)
        self._stacks = self._stacks_all.index_select(0, self._rows).contiguous()

    def inputs(self):
        """(blob, mission_feat): the kernel's two differentiable inputs from the policy's current parameters."""
        _, tensors = _params(self.policy)
        return differentiable_blob(tensors), mission_table_rows(self.policy, self._rows, self._stacks, self.mission)

    def forward_raw(self, buf, index, blob, mission_feat, out=None):
        """mgx_policy_act mode 0 -> (logits f32 [B, 7], values f32 [B]); out: that pair as contiguous f32 tensors to
        write into (a captured graph's persistent buffers)."""
        e, n = self.engine, index.numel()
        if out is None:
            logits = torch.empty((n, N_ACTIONS), dtype=torch.float32, device=e.device)
            values = torch.empty(n, dtype=torch.float32, device=e.device)
        else:
            logits, values = out
        policy_act(e, buf, index, fill_policy(self._pol, blob, mission_feat, 0), self._out, values, logits=logits)
        return logits, values

    def backward_raw(self, buf, index, blob, mission_feat, g_logits, g_values, scratch=None, out=None):
        """mgx_policy_backward -> (grad_blob f32 [words], grad_mission_feat f32 [256, n_stack, 128]); out: that pair
        as contiguous f32 tensors to write into (mgx/fused_update.py: a slice of the gradient arena)."""
        e, n, k = self.engine, index.numel(), self.K
        need = int(e.L.mgx_policy_grad_scratch_words(k, n, self.max_groups))
        if scratch is None:
            if self._scratch is None or self._scratch.numel() < need:
                self._scratch = torch.empty(need, dtype=torch.float32, device=e.device)
            scratch = self._scratch
        gl = g_logits.to(torch.float32).contiguous()
        gv = g_values.to(torch.float32).contiguous()
        if out is None:
            gb = torch.empty(self.words, dtype=torch.float32, device=e.device)
            gm = torch.empty((256, k, 128), dtype=torch.float32, device=e.device)
        else:
            gb, gm = out
            _lib.check_tensor(gb, "out: grad_blob", torch.float32, self.words, e.device)
            _lib.check_tensor(gm, "out: grad_mission_feat", torch.float32, 256 * k * 128, e.device)
        g = self._grad
        g.blob_dev, g.mission_feat_dev = blob.data_ptr(), mission_feat.data_ptr()
        g.g_logits_dev, g.g_values_dev = gl.data_ptr(), gv.data_ptr()
        g.grad_blob_dev, g.grad_mission_feat_dev = gb.data_ptr(), gm.data_ptr()
        g.scratch_dev, g.scratch_words = scratch.data_ptr(), scratch.numel()
        g.max_groups, g.reserved0 = self.max_groups, 0
        _lib.check(e.L.mgx_policy_backward(*sample_addr(e, buf, index), ctypes.byref(g), e._stream()),
                   "mgx_policy_backward")
        return gb, gm

    def evaluate_actions(self, buf, index, actions):
        """(values, log_prob, entropy) as ActorCriticPolicy.evaluate_actions on buf.gather(index)."""
        if self._rows is None:
            self.prepare(buf)
        index = index.to(torch.int64).contiguous()
        blob, table = self.inputs()
        logits, values = _PolicyFn.apply(blob, table, self, buf, index)
        dist = torch.distributions.Categorical(logits=logits)
        return values, dist.log_prob(actions), dist.entropy()
