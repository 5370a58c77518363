"""Helpers of the mission-encoder tests (tests/test_fused_mission_cpu.py, tests/test_fused_mission_gpu.py): the
weight-gradient chunk plan of mgx_mission_backward restated in Python, the shapes the GPU tests run because of it,
and an explicit fp64 Embedding + GRU whose backward through time hands out what autograd keeps to itself, the
per-(row, t) gate cotangents the kernels record."""
import math

import torch

# csrc/mgx_mission.h
MS_H, MS_G, MS_V = 128, 384, 32
MS_REC = 5 * MS_H
MS_KCHUNK, MS_MAX_CHUNKS = 64, 256
MS_SLAB = MS_G * MS_H + MS_V * MS_G + MS_H
MS_MAX_ROWS, MS_MAX_SEQ = 2048, 256


def chunk_plan(n_rows, seq_len):
    """(chunks, L, nsteps, used_chunks, empty_chunks, last_step_half) of mgx_mission_backward at (n_rows, seq_len):
    mission_chunks() and mission_backward() of csrc/mgx_engine.hip.  Chunk s of mgx_mission_wgrad_kernel covers the
    pairs k = row * seq_len + t in [s L, min(K, (s + 1) L)) in nsteps MFMA steps of two pairs each; a chunk with
    s L >= K is empty; last_step_half: the last used chunk's last live step holds one pair and one masked-out one."""
    pairs = n_rows * seq_len
    chunks = max(1, min(MS_MAX_CHUNKS, (pairs + MS_KCHUNK - 1) // MS_KCHUNK))
    L = (pairs + chunks - 1) // chunks
    L += L & 1
    used = (pairs + L - 1) // L
    return chunks, L, L // 2, used, chunks - used, bool(pairs & 1)


def workspace_words(n_rows, seq_len):
    """mgx_mission_workspace_words: the step records, one slab per chunk, dG."""
    return n_rows * seq_len * MS_REC + chunk_plan(n_rows, seq_len)[0] * MS_SLAB + MS_V * MS_G


# (n_rows, seq_len) the GPU parity tests add, and the code path each one exists for.  test_fused_mission_cpu.py
# derives the plan of every entry and asserts that the classes named here are all present.
PLAN_SHAPES = (
    (1, 1),       # T = 1, one pair: one MFMA step, half filled; the main loop of four steps is skipped
    (2, 1),       # T = 1, one full step
    (4, 1),       # T = 1, two steps, more rows than a workgroup's three
    (3, 7),       # 21 pairs in one chunk: 11 steps = two groups of four + a tail of 3, the last step half filled
    (4, 33),      # 3 chunks of 44: 22 steps, tail of 2, both chunk boundaries inside a row
    (5, 37),      # 3 chunks of 62: 31 steps, tail of 3 in every chunk, boundaries inside rows, last step half filled
    (4, 100),     # 7 chunks of 58: tail of 1; the fold's short-group path alone (chunks < 8)
    (9, 65),      # 10 chunks of 60: tail of 2; the fold takes one group of eight and a short group of two
    (5, 255),     # the longest odd T, an odd pair count, 20 chunks of 64
    (1900, 9),    # 17,100 pairs: the chunk count capped at 256, L = 68 > 64, tail of 2, 4 empty trailing chunks
    (65, 256),    # 16,640 pairs: capped, L = 66, tail of 1, 3 empty trailing chunks
    (2048, 9),    # n_rows at its maximum: capped, L = 72, no empty chunk; the last workgroup has 2 live rows
)
# The per-pair sensitivity test's shapes.  (9, 65) is not among them: over 64 steps the cotangent decays until the
# smallest pair's contribution to db_ih is 5.5 times the floor 4 eps32 max|db_ih|, where 16 times is asked.
PAIR_SHAPES = ((1900, 9), (2048, 9), (3, 7), (4, 33), (5, 37))
EPS32 = float(torch.finfo(torch.float32).eps)
EPS64 = float(torch.finfo(torch.float64).eps)


def redrawn_policy():
    """The policy of the mission-encoder tests, on the CPU: ActorCriticPolicy(n_stack=4) from seed 0 with the
    Embedding and GRU parameters redrawn (weights N(0, 1) / sqrt(fan-in), biases N(0, 0.5^2): no bias is zero)."""
    from mgx.fused_mission import mission_params
    from mgx.policy import ActorCriticPolicy
    torch.manual_seed(0)
    pol = ActorCriticPolicy(n_stack=4)
    g = torch.Generator().manual_seed(77)
    with torch.no_grad():
        for t in mission_params(pol):
            if t.dim() > 1:
                t.copy_(torch.randn(t.shape, generator=g) / math.sqrt(t.shape[1]))
            else:
                t.copy_(0.5 * torch.randn(t.shape, generator=g))
    return pol


def plan_kinds(n_rows, seq_len):
    """Token kinds of the parity tests at a PLAN_SHAPES entry."""
    return ("random",) if seq_len == 1 else ("random", "zero", "mixed")


def plan_tokens(kind, n_rows, seq_len, seed=0):
    """u8 [n_rows, seq_len] for any seq_len.  random: uniform over the 32 values, row 0 starting with a permutation
    (every value that fits occurs); zero; mixed: random and zero rows alternating."""
    g = torch.Generator().manual_seed(1000 * seq_len + 10 * n_rows + seed)
    rnd = torch.randint(0, MS_V, (n_rows, seq_len), generator=g)
    m = min(MS_V, seq_len)
    rnd[0, :m] = torch.randperm(MS_V, generator=g)[:m]
    if kind == "mixed":
        rnd[1::2] = 0
    elif kind == "zero":
        rnd.zero_()
    else:
        assert kind == "random", kind
    return rnd.to(torch.uint8)


def plan_cotangent(n_rows, seq_len):
    """The N(0, 1) feature cotangent of the parity tests, f32 [n_rows, 128]."""
    return torch.randn((n_rows, MS_H), generator=torch.Generator().manual_seed(seq_len + n_rows))


class GruRef:
    """feat [n, 128]; grads {name: tensor}; per pair (row, t): c_in [n, T, 384] = (da_r, da_z, da_n), c_hid
    [n, T, 384] = (da_r, da_z, da_n r), h_prev [n, T, 128] = h_{t-1} (zeros at t = 0).  All fp64."""


def gru_reference(params, tokens, g_feat):
    """Embedding + GRU (h_0 = 0, output the last hidden state) forward and backward through time as an explicit
    fp64 loop over t, the formulas of csrc/mgx_mission.h:
        a = G[tok_t] + W_hh h + b_hh, G[tok] = W_ih E[tok] + b_ih;  r = sigmoid(a_r), z = sigmoid(a_z),
        q = a_hn, n = tanh(G_n + r q), h' = (1 - z) n + z h
        da_n = dh (1 - z)(1 - n^2), da_z = dh (h - n) z (1 - z), da_r = da_n q r (1 - r), dh <- dh z + W_hh^T c_hid
    params: (embedding, w_ih, w_hh, b_ih, b_hh); tokens: integer [n, T]; g_feat: [n, 128]."""
    emb, w_ih, w_hh, b_ih, b_hh = (p.detach().double().cpu() for p in params)
    tok = tokens.long().cpu()
    n_rows, T = tok.shape
    H = MS_H
    G = emb @ w_ih.T + b_ih                                            # [32, 384]
    h = torch.zeros((n_rows, H), dtype=torch.float64)
    hs, rs, zs, ns, qs = [], [], [], [], []
    for t in range(T):
        a = h @ w_hh.T + b_hh
        gi = G[tok[:, t]]
        r = torch.sigmoid(gi[:, :H] + a[:, :H])
        z = torch.sigmoid(gi[:, H:2 * H] + a[:, H:2 * H])
        q = a[:, 2 * H:]
        n = torch.tanh(gi[:, 2 * H:] + r * q)
        hs.append(h)
        h = (1.0 - z) * n + z * h
        rs.append(r); zs.append(z); ns.append(n); qs.append(q)
    out = GruRef()
    out.feat = h
    dh = g_feat.detach().double().cpu().clone()
    c_in = torch.zeros((n_rows, T, 3 * H), dtype=torch.float64)
    c_hid = torch.zeros((n_rows, T, 3 * H), dtype=torch.float64)
    for t in range(T - 1, -1, -1):
        r, z, n, q, hp = rs[t], zs[t], ns[t], qs[t], hs[t]
        da_n = dh * (1.0 - z) * (1.0 - n * n)
        da_z = dh * (hp - n) * (z * (1.0 - z))
        da_r = da_n * q * (r * (1.0 - r))
        c_in[:, t] = torch.cat((da_r, da_z, da_n), 1)
        c_hid[:, t] = torch.cat((da_r, da_z, da_n * r), 1)
        dh = dh * z + c_hid[:, t] @ w_hh
    out.c_in, out.c_hid, out.h_prev = c_in, c_hid, torch.stack(hs, 1)
    ci, ch = c_in.reshape(-1, 3 * H), c_hid.reshape(-1, 3 * H)
    dG = torch.zeros((MS_V, 3 * H), dtype=torch.float64).index_add_(0, tok.reshape(-1), ci)
    out.grads = {"embedding": dG @ w_ih, "w_ih": dG.T @ emb, "w_hh": ch.T @ out.h_prev.reshape(-1, H),
                 "b_ih": ci.sum(0), "b_hh": ch.sum(0)}
    return out


def pair_floor_ratios(ref):
    """For db_ih and dW_hh: (the smallest, over pairs, of the largest |entry| of the pair's own contribution, the
    floor 4 eps32 max|gradient|).  db_ih: the pair's (da_r, da_z, da_n), every pair; dW_hh: the outer product of its
    hidden-side cotangent with h_{t-1}, pairs with t > 0 (left out at T = 1, where dW_hh = 0)."""
    small = {"b_ih": float(ref.c_in.abs().amax(2).min())}
    if ref.c_hid.shape[1] > 1:
        small["w_hh"] = float((ref.c_hid.abs().amax(2) * ref.h_prev.abs().amax(2))[:, 1:].min())
    return {n: (s, 4.0 * EPS32 * float(ref.grads[n].abs().max())) for n, s in small.items()}
