"""Fused mission encoder (mgx_mission_forward / mgx_mission_backward, include/mgx.h, added within ABI 9).

The policy's mission extractor -- Embedding(32, 32) -> GRU(32, 128), last hidden state -- runs through MIOpen as
seq_len sequential time steps of small launches in each direction.  FusedMissionEncoder runs it as one persistent HIP
kernel per direction that keeps W_hh in registers (csrc/mgx_mission.h): encode() is a
torch.autograd.Function whose inputs are the five parameter tensors and whose backward returns their five gradients,
so p.grad of the Embedding and the GRU comes out of loss.backward() as before.

Only the reference's own extractor is supported (policy.py DEFAULT_ARCH); anything else raises ValueError.  The
workspace that carries the step records from the forward to the backward is cached and grown on demand: one encode()
may be pending a backward at a time (a later encode() with autograd takes the workspace over, and the earlier graph's
backward then raises instead of reading another call's records).
"""
import ctypes

import torch

from . import _lib
from .fused_policy import _bad, _params

HIDDEN, EMBED, VOCAB = 128, 32, 32
MAX_ROWS, MAX_SEQ = 2048, 256
_P = ctypes.c_void_p


def mission_params(policy):
    """(Embedding.weight, weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0) of the policy's mission extractor;
    ValueError for any other architecture."""
    _params(policy)
    emb, gru = policy.features_extractor.extractors["mission"]
    if emb.num_embeddings != VOCAB or emb.embedding_dim != EMBED or emb.padding_idx is not None or \
            emb.max_norm is not None:
        _bad("mission Embedding %s" % (emb,))
    if gru.input_size != EMBED or gru.hidden_size != HIDDEN or not gru.bias or gru.dropout:
        _bad("mission GRU %s" % (gru,))
    return emb.weight, gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0


class _MissionFn(torch.autograd.Function):
    """(embedding, w_ih, w_hh, b_ih, b_hh) -> features f32 [n_rows, 128] of the token rows `tokens`."""

    @staticmethod
    def forward(ctx, emb, w_ih, w_hh, b_ih, b_hh, enc, tokens):
        params = tuple(t.detach().to(torch.float32).contiguous() for t in (emb, w_ih, w_hh, b_ih, b_hh))
        ws = enc._workspace(tokens.shape[0], tokens.shape[1])
        enc._ticket += 1
        ctx.enc, ctx.tokens, ctx.ws, ctx.ticket = enc, tokens, ws, enc._ticket
        ctx.save_for_backward(*params)
        return enc.forward_raw(tokens, params, ws)

    @staticmethod
    def backward(ctx, g_features):
        enc = ctx.enc
        if ctx.ticket != enc._ticket or ctx.ws is not enc._ws:
            raise RuntimeError("FusedMissionEncoder: the step records of this encode() are gone (a later encode() "
                               "or an earlier backward took the workspace)")
        enc._ticket += 1                                 # the backward clobbers the records: once only
        grads = enc.backward_raw(ctx.tokens, ctx.saved_tensors, g_features, ctx.ws)
        return grads + (None, None)


class FusedMissionEncoder:
    """The mission features of u8 token rows through the fused kernels, differentiable with respect to the policy's
    Embedding and GRU parameters."""

    def __init__(self, policy, device):
        mission_params(policy)                           # ValueError before anything touches the device
        self.policy, self.device = policy, torch.device(device)
        self.L = _lib.load()
        self._ws = None
        self._ticket = 0
        self._p, self._g = _lib.MgxMissionParams(), _lib.MgxMissionGrads()

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check_tokens(self, tokens):
        if tokens.dtype != torch.uint8 or tokens.dim() != 2 or not tokens.is_contiguous() or \
                tokens.device != self.device:
            raise ValueError("tokens must be a contiguous u8 [n_rows, seq_len] tensor on %s" % (self.device,))
        n, t = tokens.shape
        if not (1 <= n <= MAX_ROWS and 1 <= t <= MAX_SEQ):
            raise ValueError("n_rows must be in 1..%d and seq_len in 1..%d" % (MAX_ROWS, MAX_SEQ))
        return n, t

    def _workspace(self, n_rows, seq_len):
        need = int(self.L.mgx_mission_workspace_words(n_rows, seq_len))
        if need < 0:
            raise ValueError("n_rows must be in 1..%d and seq_len in 1..%d" % (MAX_ROWS, MAX_SEQ))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.float32, device=self.device)
        return self._ws

    def _fill(self, s, tensors):
        s.embedding_dev, s.w_ih_dev, s.w_hh_dev, s.b_ih_dev, s.b_hh_dev = (t.data_ptr() for t in tensors)

    def _table_args(self, table, rows, n):
        if table.dim() != 2 or table.shape[1] != HIDDEN:
            raise ValueError("the table must be a f32 [table_rows, %d] tensor" % HIDDEN)
        _lib.check_tensor(table, "the table", torch.float32, None, self.device)
        _lib.check_tensor(rows, "rows", torch.int64, n, self.device)
        return _P(table.data_ptr()), _P(rows.data_ptr()), table.shape[0]

    def _forward(self, tokens, params, workspace, table=None, rows=None):
        """mgx_mission_forward, or with (table, rows) mgx_mission_forward_rows."""
        n, t = self._check_tokens(tokens)
        self._fill(self._p, params)
        head = (_P(tokens.data_ptr()), n, t, ctypes.byref(self._p))
        tail = (None, 0) if workspace is None else (_P(workspace.data_ptr()), workspace.numel())
        if table is None:
            feat = torch.empty((n, HIDDEN), dtype=torch.float32, device=self.device)
            _lib.check(self.L.mgx_mission_forward(*head, _P(feat.data_ptr()), *tail, self._stream()),
                       "mgx_mission_forward")
            return feat
        _lib.check(self.L.mgx_mission_forward_rows(*head, *self._table_args(table, rows, n), *tail, self._stream()),
                   "mgx_mission_forward_rows")
        return table

    def _backward(self, tokens, params, g, workspace, out, rows=None):
        """mgx_mission_backward on g f32 [n_rows, 128], or with `rows` mgx_mission_backward_rows on the table g."""
        n, t = self._check_tokens(tokens)
        if out is None:
            grads = tuple(torch.empty_like(p) for p in params)
        else:
            grads = tuple(out)
            if len(grads) != 5 or any(o.shape != p.shape for o, p in zip(grads, params)):
                raise ValueError("out must be five contiguous f32 tensors shaped as params")
            for i, (o, p) in enumerate(zip(grads, params)):
                _lib.check_tensor(o, "out[%d]" % i, torch.float32, p.numel(), p.device)
        self._fill(self._p, params)
        self._fill(self._g, grads)
        head = (_P(tokens.data_ptr()), n, t, ctypes.byref(self._p))
        tail = (_P(workspace.data_ptr()), workspace.numel(), ctypes.byref(self._g), self._stream())
        if rows is None:
            _lib.check(self.L.mgx_mission_backward(*head, _P(g.data_ptr()), *tail), "mgx_mission_backward")
        else:
            _lib.check(self.L.mgx_mission_backward_rows(*head, *self._table_args(g, rows, n), *tail),
                       "mgx_mission_backward_rows")
        return grads

    def forward_raw(self, tokens, params, workspace=None):
        """mgx_mission_forward -> features f32 [n_rows, 128]; params: five contiguous f32 tensors."""
        return self._forward(tokens, params, workspace)

    def backward_raw(self, tokens, params, g_features, workspace, out=None):
        """mgx_mission_backward -> the five gradients, shaped as params; `workspace` as forward_raw left it.
        out: five contiguous f32 tensors of those shapes to write into (mgx/fused_update.py)."""
        return self._backward(tokens, params, g_features.to(torch.float32).contiguous(), workspace, out)

    def forward_rows(self, tokens, params, table, rows, workspace=None):
        """mgx_mission_forward_rows: row r's feature into table[rows[r]] (table f32 [table_rows, 128], rows i64
        [n_rows]) -- forward_raw + table.index_copy_(0, rows, .) bit for bit, in one launch.  Indices outside the
        table are the caller's error."""
        return self._forward(tokens, params, workspace, table, rows)

    def backward_rows(self, tokens, params, g_table, rows, workspace, out=None):
        """mgx_mission_backward_rows: backward_raw on g_table.index_select(0, rows) bit for bit, without the
        index_select (g_table f32 [table_rows, 128]); rows it does not name are not read."""
        return self._backward(tokens, params, g_table, workspace, out, rows)

    def encode(self, tokens_u8):
        """f32 [n_rows, 128]: the extractor's output on u8 [n_rows, seq_len] token rows.  Under autograd the result
        is connected to the five parameters; without it the forward runs with no workspace."""
        params = mission_params(self.policy)
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return _MissionFn.apply(*params, self, tokens_u8)
        return self.forward_raw(tokens_u8, tuple(p.detach().to(torch.float32).contiguous() for p in params))
