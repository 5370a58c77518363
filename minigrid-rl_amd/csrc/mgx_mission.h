// mgx_mission.h -- mgx_mission_forward / mgx_mission_backward: the reference's mission extractor, Embedding(32, 32) ->
// GRU(32, 128, one layer, bias, batch_first), h0 = 0, output = last hidden state, forward and backward through time,
// for n_rows independent token sequences.  Included by mgx_engine.hip after mgx_policy_grad.h (pg_f16).
//
// Mapping.  The input side takes 32 values: G[tok] = W_ih E[tok] + b_ih is a [32][384] table every
// workgroup builds in LDS in its prologue (1,024 multiply-adds per thread), so a time step is G[tok_t] + W_hh h + b_hh
// and the gate math.  A workgroup of 384 threads owns MS_ROWS = 3 rows for all seq_len steps; rows are independent:
// no cross-workgroup synchronisation.  W_hh (196,608 B) lives in registers:
//   forward   thread j holds row j of W_hh (128 VGPRs); per step it forms a[i][j] = W_hh[j] . h_i + b_hh[j] for the
//             three rows, h broadcast from LDS as float4; after a barrier thread (i, u) = (tid / 128, tid % 128) does
//             row i's gate math for unit u and writes h' to the other half of a double-buffered LDS h.  Two barriers
//             per step.
//   backward  thread (part, u) holds column u of gate block `part` of W_hh, W_hh[part * 128 + k][u] (128 VGPRs: W_hh
//             transposed); thread (i, u) carries dh[i][u] in a register, forms the gate cotangents of its unit from
//             the step record, writes them to the workspace and to LDS; after a barrier thread (part, u) forms the
//             partial sum_k W_hh[part * 128 + k][u] c_i[part * 128 + k] for the three rows; after a second barrier
//             dh = dh z + ((P0 + P1) + P2).  The next step's record is loaded before this step's arithmetic.
// The weight gradients are off the serial chain: mgx_mission_wgrad_kernel is an fp32-input MFMA GEMM over k = (row, t)
// split into S chunks of k (S and the chunk length depend on (n_rows, seq_len) only), one 32 x 32 block per wave, into
// per-chunk slabs; mgx_mission_fold_kernel adds the slabs in chunk order; mgx_mission_input_grad_kernel forms dW_ih,
// db_ih, dE and the r / z part of db_hh from dG.  No float atomics anywhere: every output is bitwise reproducible.
// fp32 throughout, every multiply-add an explicit fmaf or an MFMA (a k-ordered fmaf chain); contraction stays off.
#ifndef MGX_MISSION_H_
#define MGX_MISSION_H_

constexpr int MS_H = 128;                   // hidden units
constexpr int MS_G = 3 * MS_H;              // gate rows: r | z | n
constexpr int MS_E = 32;                    // embedding width
constexpr int MS_V = 32;                    // vocabulary
constexpr int MS_ROWS = 3;                  // rows per workgroup: MS_ROWS * MS_H (row, unit) pairs = one per thread
constexpr int MS_THREADS = MS_G;
constexpr int MS_MAX_ROWS = 2048, MS_MAX_SEQ = 256;
constexpr int MS_REC = 5 * MS_H;            // workspace words per (row, t): h_t | r | z | n | W_hn h + b_hn
constexpr int MS_KCHUNK = 64;               // (row, t) pairs per weight-gradient chunk, until MS_MAX_CHUNKS chunks
constexpr int MS_MAX_CHUNKS = 256;
constexpr int MS_SLAB_G = MS_G * MS_H;              // slab: dW_hh [384][128] | dG [32][384] | db_hn [128]
constexpr int MS_SLAB_B = MS_SLAB_G + MS_V * MS_G;
constexpr int MS_SLAB = MS_SLAB_B + MS_H;
static_assert(MS_ROWS * MS_H == MS_THREADS, "one (row, unit) pair per thread");

struct MissionArgs {
    const uint8_t *tokens;                  // [n_rows][T]
    int64_t n_rows;
    int T;
    const float *emb, *w_ih, *w_hh, *b_ih, *b_hh;
    float *feat;                            // forward: [n_rows][128]
    const float *g_feat;                    // backward: [n_rows][128]
    float *ws;                              // step records [n_rows][T][MS_REC]; forward: may be null
    const int64_t *rows;                    // ROWS: row r's feature / cotangent is row rows[r] of feat / g_feat
};

// 0 and 1 for large |x| (expf gives inf or 0), never NaN
__device__ __forceinline__ float ms_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// acc[i] += w . x_i for the workgroup's rows.  Summation order: eight partial sums, partial p taking k = p mod 8 in
// ascending k (acc[i]'s initial value starts partial 0), then the pairwise tree ((0+1)+(2+3))+((4+5)+(6+7)).  One chain
// of 128 put the features 2 to 2.5 times further from fp64 than torch's GRU; eight chains of 16 are level with it.
template <class LH>
__device__ __forceinline__ void ms_matvec(const float (&w)[MS_H], float (&acc)[MS_ROWS], LH xrow) {
    float p[MS_ROWS][8];
#pragma unroll
    for (int i = 0; i < MS_ROWS; i++) {
        p[i][0] = acc[i];
#pragma unroll
        for (int c = 1; c < 8; c++) p[i][c] = 0.0f;
    }
#pragma unroll
    for (int k4 = 0; k4 < MS_H / 4; k4++)
#pragma unroll
        for (int i = 0; i < MS_ROWS; i++) {
            const float4 xv = xrow(i)[k4];                            // one address for the whole wave: a broadcast
            const int c = (k4 & 1) * 4;
            p[i][c + 0] = __builtin_fmaf(w[4 * k4 + 0], xv.x, p[i][c + 0]);
            p[i][c + 1] = __builtin_fmaf(w[4 * k4 + 1], xv.y, p[i][c + 1]);
            p[i][c + 2] = __builtin_fmaf(w[4 * k4 + 2], xv.z, p[i][c + 2]);
            p[i][c + 3] = __builtin_fmaf(w[4 * k4 + 3], xv.w, p[i][c + 3]);
        }
#pragma unroll
    for (int i = 0; i < MS_ROWS; i++)
        acc[i] = ((p[i][0] + p[i][1]) + (p[i][2] + p[i][3])) + ((p[i][4] + p[i][5]) + (p[i][6] + p[i][7]));
}

// ROWS (mgx_mission_forward_rows): the one store below goes to row a.rows[myrow] of a table, nothing else differs.
template <bool ROWS>
__global__ __launch_bounds__(MS_THREADS) void mgx_mission_forward_kernel(MissionArgs a) {
    __shared__ float sG[MS_V * MS_G];                                 // G[tok][j]
    __shared__ __align__(16) float sH[2][MS_ROWS][MS_H];
    __shared__ float sA[MS_ROWS][MS_G];                               // W_hh h + b_hh
    __shared__ uint8_t sTok[MS_ROWS][MS_MAX_SEQ];
    const int tid = threadIdx.x;
    const int T = a.T;
    const int64_t row0 = (int64_t)blockIdx.x * MS_ROWS;
    for (int i = tid; i < MS_ROWS * T; i += MS_THREADS) {
        const int r = i / T, t = i - r * T;
        const int64_t row = row0 + r;
        sTok[r][t] = row < a.n_rows ? (uint8_t)(a.tokens[row * T + t] & (MS_V - 1)) : (uint8_t)0;
    }
    {
        float wi[MS_E];
        const float4 *w4 = reinterpret_cast<const float4 *>(a.w_ih + (size_t)tid * MS_E);
#pragma unroll
        for (int e4 = 0; e4 < MS_E / 4; e4++) {
            const float4 x = w4[e4];
            wi[4 * e4] = x.x; wi[4 * e4 + 1] = x.y; wi[4 * e4 + 2] = x.z; wi[4 * e4 + 3] = x.w;
        }
        const float bi = a.b_ih[tid];
#pragma nounroll
        for (int tok = 0; tok < MS_V; tok++) {
            float acc = bi;
#pragma unroll
            for (int e = 0; e < MS_E; e++) acc = __builtin_fmaf(wi[e], a.emb[tok * MS_E + e], acc);
            sG[tok * MS_G + tid] = acc;
        }
    }
    float w[MS_H];
    {
        const float4 *w4 = reinterpret_cast<const float4 *>(a.w_hh + (size_t)tid * MS_H);
#pragma unroll
        for (int k4 = 0; k4 < MS_H / 4; k4++) {
            const float4 x = w4[k4];
            w[4 * k4] = x.x; w[4 * k4 + 1] = x.y; w[4 * k4 + 2] = x.z; w[4 * k4 + 3] = x.w;
        }
    }
    const float bh = a.b_hh[tid];
    for (int i = tid; i < 2 * MS_ROWS * MS_H; i += MS_THREADS) (&sH[0][0][0])[i] = 0.0f;
    const int ri = tid >> 7, u = tid & (MS_H - 1);                    // the gate math's (row, unit)
    const int64_t myrow = row0 + ri;
    const bool live = myrow < a.n_rows;
    float *rec = a.ws ? a.ws + (size_t)(live ? myrow : 0) * T * MS_REC + u : nullptr;
    __syncthreads();
    int cur = 0;
#pragma nounroll
    for (int t = 0; t < T; t++) {
        float acc[MS_ROWS];
#pragma unroll
        for (int i = 0; i < MS_ROWS; i++) acc[i] = bh;
        ms_matvec(w, acc, [&](int i) { return reinterpret_cast<const float4 *>(&sH[cur][i][0]); });
#pragma unroll
        for (int i = 0; i < MS_ROWS; i++) sA[i][tid] = acc[i];
        __syncthreads();
        const float *g = sG + (int)sTok[ri][t] * MS_G + u;
        const float q = sA[ri][2 * MS_H + u];
        const float r = ms_sigmoid(g[0] + sA[ri][u]);
        const float z = ms_sigmoid(g[MS_H] + sA[ri][MS_H + u]);
        const float n = tanhf(__builtin_fmaf(r, q, g[2 * MS_H]));
        const float hn = __builtin_fmaf(z, sH[cur][ri][u] - n, n);    // (1 - z) n + z h
        sH[cur ^ 1][ri][u] = hn;
        if (rec && live) {
            float *p = rec + (size_t)t * MS_REC;
            p[0] = hn; p[MS_H] = r; p[2 * MS_H] = z; p[3 * MS_H] = n; p[4 * MS_H] = q;
        }
        cur ^= 1;
        __syncthreads();
    }
    if (live) a.feat[(ROWS ? a.rows[myrow] : myrow) * MS_H + u] = sH[cur][ri][u];
}

// Backward through time.  Record slots on return: h_t | da_r | da_z | da_n | da_n r  (a_* the gate pre-activations;
// slots 1..3 are the input-side cotangents, 1, 2 and 4 the hidden-side ones).
// ROWS (mgx_mission_backward_rows): the one load of the cotangent reads row a.rows[myrow] of a table.
template <bool ROWS>
__global__ __launch_bounds__(MS_THREADS) void mgx_mission_bptt_kernel(MissionArgs a) {
    __shared__ __align__(16) float sC[MS_ROWS][MS_G];                 // hidden-side cotangents of this step
    __shared__ float sP[MS_ROWS][3][MS_H];                            // the three partial products per (row, unit)
    const int tid = threadIdx.x;
    const int T = a.T;
    const int part = tid >> 7, u = tid & (MS_H - 1);
    const int ri = part;
    const int64_t myrow = (int64_t)blockIdx.x * MS_ROWS + ri;
    const bool live = myrow < a.n_rows;
    float wt[MS_H];
#pragma unroll
    for (int k = 0; k < MS_H; k++) wt[k] = a.w_hh[(size_t)(part * MS_H + k) * MS_H + u];
    float *rec = a.ws + (size_t)(live ? myrow : 0) * T * MS_REC + u;
    float dh = live ? a.g_feat[(ROWS ? a.rows[myrow] : myrow) * MS_H + u] : 0.0f;
    float r = 0.0f, z = 0.0f, n = 0.0f, q = 0.0f, hp = 0.0f;
    const auto load = [&](int t, float &r_, float &z_, float &n_, float &q_, float &hp_) {
        r_ = z_ = n_ = q_ = hp_ = 0.0f;
        if (live) {
            const float *p = rec + (size_t)t * MS_REC;
            r_ = p[MS_H]; z_ = p[2 * MS_H]; n_ = p[3 * MS_H]; q_ = p[4 * MS_H];
            if (t > 0) hp_ = p[-MS_REC];
        }
    };
    load(T - 1, r, z, n, q, hp);
#pragma nounroll
    for (int t = T - 1; t >= 0; t--) {
        float r2 = 0.0f, z2 = 0.0f, n2 = 0.0f, q2 = 0.0f, hp2 = 0.0f;
        if (t > 0) load(t - 1, r2, z2, n2, q2, hp2);
        const float da_n = dh * (1.0f - z) * __builtin_fmaf(-n, n, 1.0f);
        const float da_z = dh * (hp - n) * (z * (1.0f - z));
        const float da_r = da_n * q * (r * (1.0f - r));
        const float dhn = da_n * r;
        if (live) {
            float *p = rec + (size_t)t * MS_REC;
            p[MS_H] = da_r; p[2 * MS_H] = da_z; p[3 * MS_H] = da_n; p[4 * MS_H] = dhn;
        }
        sC[ri][u] = da_r; sC[ri][MS_H + u] = da_z; sC[ri][2 * MS_H + u] = dhn;
        __syncthreads();
        float acc[MS_ROWS];
#pragma unroll
        for (int i = 0; i < MS_ROWS; i++) acc[i] = 0.0f;
        ms_matvec(wt, acc, [&](int i) { return reinterpret_cast<const float4 *>(&sC[i][part * MS_H]); });
#pragma unroll
        for (int i = 0; i < MS_ROWS; i++) sP[i][part][u] = acc[i];
        __syncthreads();
        dh = __builtin_fmaf(dh, z, (sP[ri][0][u] + sP[ri][1][u]) + sP[ri][2][u]);
        r = r2; z = z2; n = n2; q = q2; hp = hp2;
    }
}

struct MissionWArgs {
    const uint8_t *tokens;
    const float *ws;
    int K, T, L;                            // K = n_rows * T pairs; chunk s covers k in [s L, min(K, (s + 1) L)), L even
    float *part;                            // [chunks][MS_SLAB]
};

// grid (12, chunks): workgroup (b, s) forms the 32 gate rows j0 = 32 b of chunk s's slab.  Waves 0..3: dW_hh[j][32 w ..]
// = sum_k c_hidden[k][j] h_{t-1}[k][.]; wave 4: dG[tok][j] = sum_k c_input[k][j] [tok_k == tok]; wave 5 (n gate only):
// db_hn[j] = sum_k c_hidden[k][j].  Summation order within a chunk: four accumulators, MFMA step kk (pairs 2 kk and
// 2 kk + 1) into accumulator kk mod 4 while whole groups of four steps last, the rest into accumulator 0, then
// (0 + 1) + (2 + 3).  Pairs past the chunk's end enter as exact zeros.
__global__ __launch_bounds__(MS_THREADS) void mgx_mission_wgrad_kernel(MissionWArgs a) {
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j0 = blockIdx.x * 32, gate = j0 >> 7, jj = j0 & (MS_H - 1);
    if (wv == 5 && gate < 2) return;
    const int k0 = blockIdx.y * a.L, k1 = min(a.K, k0 + a.L);
    float *slab = a.part + (size_t)blockIdx.y * MS_SLAB;
    const int slot = (wv == 4 || gate < 2) ? 1 + gate : 4;
    const int r = lane & 31, h = lane >> 5;
    const float *pa = a.ws + slot * MS_H + jj + r;
    const float *pb = a.ws + (wv & 3) * 32 + r;
    pg_f16 acc[4];
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int i = 0; i < 16; i++) acc[q][i] = 0.0f;
    const int nsteps = a.L >> 1;
    // this lane's operands of MFMA step kk: pair k = k0 + 2 kk + h; the loads are unconditional (clamped addresses)
    const auto fetch = [&](int kk, float &av, float &bv) {
        const int k = k0 + 2 * kk + h;
        const bool in = k < k1;
        const int kc = min(k, a.K - 1);
        av = pa[(size_t)kc * MS_REC];
        if (wv < 4) {
            const float hv = pb[(size_t)max(kc - 1, 0) * MS_REC];
            bv = (unsigned)kc % (unsigned)a.T ? hv : 0.0f;            // h_{-1} = 0
        } else if (wv == 4) {
            bv = (a.tokens[kc] & (MS_V - 1)) == r ? 1.0f : 0.0f;
        } else {
            bv = r == 0 ? 1.0f : 0.0f;
        }
        av = in ? av : 0.0f;
        bv = in ? bv : 0.0f;
    };
    int kk = 0;
    for (; kk + 4 <= nsteps; kk += 4) {                               // four steps' loads in flight at a time
        float av[4], bv[4];
#pragma unroll
        for (int q = 0; q < 4; q++) fetch(kk + q, av[q], bv[q]);
#pragma unroll
        for (int q = 0; q < 4; q++) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q], bv[q], acc[q], 0, 0, 0);
    }
    for (; kk < nsteps; kk++) {
        float av, bv;
        fetch(kk, av, bv);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[0], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int m = (i & 3) + 8 * (i >> 2) + 4 * h;
        const float x = (acc[0][i] + acc[1][i]) + (acc[2][i] + acc[3][i]);
        if (wv < 4) slab[(j0 + m) * MS_H + wv * 32 + r] = x;
        else if (wv == 4) slab[MS_SLAB_G + r * MS_G + j0 + m] = x;
        else if (r == 0) slab[MS_SLAB_B + jj + m] = x;
    }
}

// The slabs added in chunk order, eight at a time as ((0+1)+(2+3))+((4+5)+(6+7)) (a short last group: its slabs in
// order), the groups' sums then in order -> dW_hh, dG (scratch), db_hh[256..383]
__global__ __launch_bounds__(256) void mgx_mission_fold_kernel(const float *__restrict__ part, int chunks,
                                                               float *__restrict__ dw_hh, float *__restrict__ dG,
                                                               float *__restrict__ db_hh) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= MS_SLAB) return;
    const float *p = part + i;
    float s = 0.0f;
    int c = 0;
    for (; c + 8 <= chunks; c += 8) {
        float x[8];
#pragma unroll
        for (int q = 0; q < 8; q++) x[q] = p[(size_t)(c + q) * MS_SLAB];
        const float g = ((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7]));
        s = c ? s + g : g;
    }
    if (c < chunks) {
        float g = p[(size_t)c * MS_SLAB];
        for (int q = c + 1; q < chunks; q++) g = g + p[(size_t)q * MS_SLAB];
        s = c ? s + g : g;
    }
    if (i < MS_SLAB_G) dw_hh[i] = s;
    else if (i < MS_SLAB_B) dG[i - MS_SLAB_G] = s;
    else db_hh[2 * MS_H + i - MS_SLAB_B] = s;
}

// From dG [32][384], one output per 32 lanes: dW_ih[j][e] = sum_tok dG[tok][j] E[tok][e]; db_ih[j] = sum_tok dG[tok][j]
// (= db_hh[j] for the r and z gates, whose two sides share a cotangent); dE[tok][e] = sum_j W_ih[j][e] dG[tok][j].
// Lane l takes the terms l, l + 32, ... in ascending order, then a butterfly over the 32 lanes (a tree: dE's 384
// terms cancel heavily, and one chain over them was 7 times further from fp64 than torch).  A token that never occurs
// has dG[tok] = 0 exactly (its one-hot column is all zeros), hence dE[tok] = 0 exactly.
constexpr int MS_INPUT_GRAD_OUTPUTS = MS_G * MS_E + MS_G + MS_V * MS_E;
__global__ __launch_bounds__(256) void mgx_mission_input_grad_kernel(const float *__restrict__ dG,
                                                                     const float *__restrict__ emb,
                                                                     const float *__restrict__ w_ih,
                                                                     float *__restrict__ d_emb, float *__restrict__ dw_ih,
                                                                     float *__restrict__ db_ih, float *__restrict__ db_hh) {
    int o = blockIdx.x * 8 + (threadIdx.x >> 5);                      // uniform over the 32 lanes
    const int l = threadIdx.x & 31;
    if (o >= MS_INPUT_GRAD_OUTPUTS) return;
    float x = 0.0f;
    float *out, *out2 = nullptr;
    if (o < MS_G * MS_E) {
        const int j = o / MS_E, e = o - j * MS_E;
        x = dG[l * MS_G + j] * emb[l * MS_E + e];
        out = dw_ih + o;
    } else if ((o -= MS_G * MS_E) < MS_G) {
        x = dG[l * MS_G + o];
        out = db_ih + o;
        if (o < 2 * MS_H) out2 = db_hh + o;
    } else {
        o -= MS_G;
        const int tok = o / MS_E, e = o - tok * MS_E;
        for (int j = l; j < MS_G; j += 32) x = __builtin_fmaf(w_ih[j * MS_E + e], dG[tok * MS_G + j], x);
        out = d_emb + o;
    }
#pragma unroll
    for (int sh = 1; sh < 32; sh <<= 1) x = x + __shfl_xor(x, sh, 64);
    if (l == 0) {
        *out = x;
        if (out2) *out2 = x;
    }
}

#endif  // MGX_MISSION_H_
