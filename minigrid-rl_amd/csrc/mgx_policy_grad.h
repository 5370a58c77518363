// mgx_policy_grad.h -- mgx_policy_backward: the gradient of mgx_policy_act's network (mgx_policy.h) with respect to
// the weight blob and the mission-feature table, straight from compact rows.  Included by mgx_engine.hip after
// mgx_policy.h, whose constants, blob layout and dot helpers it uses.
//
// Mapping: one workgroup of 8 waves per tile of 64 samples, LANE = SAMPLE, as mgx_policy_kernel<K>.
// At most `groups` workgroups run; workgroup g walks tiles g, g + groups, ... and adds every tile's weight gradient
// into its own slab scratch[g][blob words] with plain loads and stores (the first tile stores, so the scratch need
// not be zeroed); mgx_policy_fold_kernel then adds the slabs in group order: grad_blob is bitwise reproducible.
// Three passes per tile:
//   (a) forward   stages A-F of mgx_policy_kernel: the same pol_trunk (mgx_policy.h) with this kernel's six LDS
//                 regions, every activation kept in LDS as [feature][sample], row stride 65 dwords
//   (b) backward  lane = sample, waves split a layer's INPUTS: dX[i] = sum_o W[o][i] dZ[o] with wave-uniform scalar
//                 weight loads, written in place over the activation it replaces (Tanh' and ReLU' from the outputs)
//   (c) weights   dW[o][i] = sum_s dZ[o][s] A[i][s] on v_mfma_f32_32x32x2_f32 (exact fp32, k = sample ascending):
//                 both operands are already sample-minor in LDS, one 32x32 block of dW per wave at a time.
//                 conv1 is the exception: its pooled gradient sits at a per-sample position, so it runs on the VALU
//                 as the forward's stage B does (lane = sample, then a fixed-order butterfly over the wave).
// LDS rows (65 dwords each): P 144 | C2 128 | F 80 | H1 128 | H2 128 = 608 rows = 158,080 B for every n_stack.  The
// input rows (37 K <= 296) lie over C2.. while those are unwritten and are staged again for conv1's backward once
// they are dead; the mission features are staged over H2 once its gradient has been consumed, and their gradient
// replaces them; the direction one-hot is staged over H1.  One workgroup per CU.
// fp32 throughout, every multiply-add an explicit fmaf or an MFMA (a k-ordered fmaf chain).
#ifndef MGX_POLICY_GRAD_H_
#define MGX_POLICY_GRAD_H_

constexpr int PG_DEFAULT_GROUPS = 256;     // workgroups (= slabs) when max_groups is 0: one per CU of an MI355X
constexpr int PG_P = 0, PG_C2 = 144, PG_F = 272, PG_H1 = 352, PG_H2 = 480, PG_ROWS = 608;
constexpr int PG_POS = PG_C2 + 8 * POL_RW;  // conv1 backward: arg-max position bytes [36][65] dwords, after the rows
constexpr int PG_IDX = PG_POS + 36;         // stage A's (sample, slot) arrays: 12 B each, <= 24 rows
static_assert(PG_IDX * POL_LS * 4 % 8 == 0 && PG_IDX + 24 <= PG_ROWS, "stage-A arrays");
constexpr size_t pg_lds_bytes() { return (size_t)PG_ROWS * POL_LS * 4; }

typedef float pg_f16 __attribute__((ext_vector_type(16)));

struct PolGradArgs {
    SampleAddr s;
    const float *blob, *mfeat, *g_logits, *g_values;
    float *gmf, *scratch;
    int groups;
};

// acc[j] += sum_o w[o * ldw + j] * z(o), o ascending: the transposed product, accumulators indexed by input
template <int NI, class LZ>
__device__ __forceinline__ void pg_dot_t(float (&acc)[NI], const float *__restrict__ w, int ldw, int nout, LZ z) {
#pragma nounroll
    for (int o = 0; o < nout; o++) {
        const float zo = z(o);
#pragma unroll
        for (int j = 0; j < NI; j++) acc[j] = __builtin_fmaf(w[o * ldw + j], zo, acc[j]);
    }
}

// One 32x32 block of D[m][n] = sum_k A[m][k] B[k][n], k = 0 .. 2 * nsteps - 1 ascending.  la(r, k) is A[r][k] and
// lb(r, k) is B[k][r] for this lane's r = lane & 31; st(m, n, value) receives the block.
template <class LA, class LB, class ST>
__device__ __forceinline__ void pg_mfma_block(int lane, int nsteps, LA la, LB lb, ST st) {
    const int r = lane & 31, h = lane >> 5;
    pg_f16 acc;
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = 0.0f;
#pragma unroll 4
    for (int kk = 0; kk < nsteps; kk++)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(la(r, 2 * kk + h), lb(r, 2 * kk + h), acc, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 16; i++) st((i & 3) + 8 * (i >> 2) + 4 * h, r, acc[i]);
}

template <int K>
__global__ __launch_bounds__(POL_THREADS, 2) void mgx_policy_grad_kernel(PolGradArgs a) {
    extern __shared__ __align__(16) uint8_t smem[];
    constexpr PolBlob L = pol_blob(K);
    constexpr int LS = POL_LS;
    constexpr int NF = POL_NF;
    float *S = reinterpret_cast<float *>(smem);
    float *P = S + PG_P * LS, *C2 = S + PG_C2 * LS, *F = S + PG_F * LS, *H1 = S + PG_H1 * LS, *H2 = S + PG_H2 * LS;
    float *Y = C2;                                                    // the input rows: [K * 37][65]
    uint8_t *PosB = reinterpret_cast<uint8_t *>(S + PG_POS * LS);
    const uint8_t **s_src = reinterpret_cast<const uint8_t **>(S + PG_IDX * LS);   // [64 * K], nullptr: empty slot
    int *s_mid = reinterpret_cast<int *>(s_src + POL_TILE * K);       // [64 * K], -1: empty slot
    __shared__ float s_g[8 * POL_LS];                                 // cotangents: rows 0..6 logits, 7 value
    __shared__ int s_key[POL_TILE];                                   // mid * K + v - 1; -1: spare lane
    __shared__ int s_lead[POL_TILE];                                  // ordinal among the tile's distinct keys, or -1
    float *slab = a.scratch + (size_t)blockIdx.x * L.words;
    const int64_t ntiles = (a.s.B + POL_TILE - 1) / POL_TILE;

    for (int64_t tile = blockIdx.x; tile < ntiles; tile += a.groups) {
        // the thread id is made opaque once per tile: hoisted out of this loop, the per-lane LDS addresses of every
        // stage would stay live across the whole body and spill
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const float *Wt = a.blob;                                     // likewise the weight base: its per-tensor
        asm volatile("" : "+s"(Wt));                                  // addresses would be hoisted and spilt
        const float *__restrict__ W = Wt;
        const int lane = tid & 63;
        const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform: weight addresses stay scalar
        const bool first = tile == (int64_t)blockIdx.x;
        const int64_t b0 = tile * POL_TILE;
        const int nb = (int)min<int64_t>(POL_TILE, a.s.B - b0);
        // slab[off] (+)= v
        const auto put = [&](int off, float v) { slab[off] = first ? v : slab[off] + v; };
        // sums of `per` consecutive LDS rows over the 64 samples -> n bias gradients: a lane adds its sample's `per`
        // values, then a fixed-order butterfly over the wave (a tree: shorter rounding chains than a serial sum)
        const auto bias = [&](const float *Z, int n, int per, int off) {
            for (int o = wv; o < n; o += POL_NW) {
                float x = 0.0f;
                for (int q = 0; q < per; q++) x = x + Z[(o * per + q) * LS + lane];
#pragma unroll
                for (int sh = 1; sh < 64; sh <<= 1) x = x + __shfl_xor(x, sh, 64);
                if (lane == 0) put(off + o, x);
            }
        };
        // ---- A, A2 again, for conv1's backward: source row of every (sample, slot), then the rows -> Y
        const auto stage_rows = [&]() {
            pol_stage_src<K>(a.s, nullptr, b0, nb, tid, s_src, s_mid);
            __syncthreads();
            pol_stage_rows<K>(s_src, tid, Y);
        };
        const uint8_t *xb = reinterpret_cast<const uint8_t *>(Y) + lane * 4;

        // =============================================================== (a) forward: mgx_policy.h's pol_trunk, no
        // terminal rows; the rows lie over C2.  Beside the rows it stages the cotangents and the table keys
        const PolLane pl = pol_trunk<K>(a.s, nullptr, b0, nb, tid, lane, wv, W, a.mfeat, s_src, s_mid,
                                        PolLds{Y, P, C2, F, H1, H2}, [&](int my_key) {
            for (int i = tid; i < 8 * POL_TILE; i += POL_THREADS) {  // the cotangents; spare lanes: exactly zero
                const int o = i >> 6, s = i & 63;
                float g = 0.0f;
                if (s < nb) g = o < POL_NA ? a.g_logits[(b0 + s) * POL_NA + o] : a.g_values[b0 + s];
                s_g[o * LS + s] = g;
            }
            if (wv == 0) {                                            // a key's first sample leads its table sum
                const int kreg = lane < nb ? my_key : -1;
                bool lead = lane < nb;
                for (int q = 0; q < POL_TILE - 1; q++) {
                    const int kq = __shfl(kreg, q, 64);
                    if (q < lane && kq == kreg) lead = false;
                }
                const unsigned long long leaders = __ballot(lead);
                s_key[lane] = kreg;
                s_lead[lane] = lead ? __popcll(leaders & ((1ull << lane) - 1ull)) : -1;
            }
        });
        const int v = pl.v;
        const uint32_t dsel = pl.dsel;

        // =============================================================== (b), (c) backward, heads first
        // ---- heads: dWa[o][i] = sum_s g[o][s] H2p[i][s], dWvn[i] = sum_s gv[s] H2v[i][s]; biases = row sums of g
        if (wv < 4) {
            const int half = wv >> 1, i0 = (wv & 1) * 32;             // half 0: action_net, 1: value_net
            pg_mfma_block(lane, 32,
                          [&](int r, int k) { return half ? (r == 0 ? s_g[7 * LS + k] : 0.0f) : (r < POL_NA ? s_g[r * LS + k] : 0.0f); },
                          [&](int r, int k) { return H2[(half * 64 + i0 + r) * LS + k]; },
                          [&](int m, int n, float x) {
                              if (m < (half ? 1 : POL_NA)) put((half ? L.vn_w : L.a_w) + m * 64 + i0 + n, x);
                          });
        }
        bias(s_g, POL_NA, 1, L.a_b);
        bias(s_g + 7 * LS, 1, 1, L.vn_b);
        __syncthreads();
        // dZ2 = (Wa^T g | wvn gv) * (1 - H2^2), in place over H2
        {
            const int i0 = wv * NF;
            float dp[NF], dv[NF];
#pragma unroll
            for (int j = 0; j < NF; j++) { dp[j] = 0.0f; dv[j] = 0.0f; }
            pg_dot_t<NF>(dp, W + L.a_w + i0, 64, POL_NA, [&](int o) { return s_g[o * LS + lane]; });
            pg_dot_t<NF>(dv, W + L.vn_w + i0, 64, 1, [&](int) { return s_g[7 * LS + lane]; });
#pragma unroll
            for (int j = 0; j < NF; j++) {
                const float tp = H2[(i0 + j) * LS + lane], tv = H2[(64 + i0 + j) * LS + lane];
                H2[(i0 + j) * LS + lane] = dp[j] * __builtin_fmaf(-tp, tp, 1.0f);
                H2[(64 + i0 + j) * LS + lane] = dv[j] * __builtin_fmaf(-tv, tv, 1.0f);
            }
        }
        __syncthreads();
        // ---- L1: dW1[o][i] = sum_s dZ2[o][s] H1[i][s]: 2 nets x 2 x 2 blocks, one per wave
        {
            const int net = wv >> 2, o0 = ((wv >> 1) & 1) * 32, i0 = (wv & 1) * 32;
            pg_mfma_block(lane, 32, [&](int r, int k) { return H2[(net * 64 + o0 + r) * LS + k]; },
                          [&](int r, int k) { return H1[(net * 64 + i0 + r) * LS + k]; },
                          [&](int m, int n, float x) { put((net ? L.v1_w : L.p1_w) + (o0 + m) * 64 + i0 + n, x); });
        }
        bias(H2, 64, 1, L.p1_b);
        bias(H2 + 64 * LS, 64, 1, L.v1_b);
        __syncthreads();
        // dZ1 = (W1^T dZ2) * (1 - H1^2), in place over H1
        {
            const int i0 = wv * NF;
            float dp[NF], dv[NF];
#pragma unroll
            for (int j = 0; j < NF; j++) { dp[j] = 0.0f; dv[j] = 0.0f; }
            pg_dot_t<NF>(dp, W + L.p1_w + i0, 64, 64, [&](int o) { return H2[o * LS + lane]; });
            pg_dot_t<NF>(dv, W + L.v1_w + i0, 64, 64, [&](int o) { return H2[(64 + o) * LS + lane]; });
#pragma unroll
            for (int j = 0; j < NF; j++) {
                const float tp = H1[(i0 + j) * LS + lane], tv = H1[(64 + i0 + j) * LS + lane];
                H1[(i0 + j) * LS + lane] = dp[j] * __builtin_fmaf(-tp, tp, 1.0f);
                H1[(64 + i0 + j) * LS + lane] = dv[j] * __builtin_fmaf(-tv, tv, 1.0f);
            }
        }
        __syncthreads();
        // ---- the mission features of every sample -> M = H2 (dZ2 is dead): M[f][s] = mission_feat[key(s)][f]
        float *M = H2;
        for (int i = tid; i < 128 * POL_TILE; i += POL_THREADS) {
            const int f = i & 127, s = i >> 7;
            const int key = s_key[s];
            M[f * LS + s] = a.mfeat[(size_t)(key < 0 ? 0 : key) * 128 + f];
        }
        __syncthreads();
        // ---- L0: dW0[o][i] = sum_s dZ1[o][s] (F | M)[i][s]: 4 x 7 blocks (rows 0..63 policy_net, 64..127 value_net_body)
        for (int t = wv; t < 28; t += POL_NW) {
            const int mt = t / 7, nt = t - mt * 7;
            const int o0 = (mt & 1) * 32, i0 = nt * 32;
            const int woff = mt >> 1 ? L.v0_w : L.p0_w;
            pg_mfma_block(lane, 32, [&](int r, int k) { return H1[(mt * 32 + r) * LS + k]; },
                          [&](int r, int k) {
                              const int i = i0 + r;
                              return i < 80 ? F[i * LS + k] : i < POL_FEAT ? M[(i - 80) * LS + k] : 0.0f;
                          },
                          [&](int m, int n, float x) {
                              if (i0 + n < POL_FEAT) put(woff + (o0 + m) * POL_FEAT + i0 + n, x);
                          });
        }
        bias(H1, 64, 1, L.p0_b);
        bias(H1 + 64 * LS, 64, 1, L.v0_b);
        __syncthreads();
        // dFeat = W0p^T dZ1p + W0v^T dZ1v: 26 inputs per wave.  [0, 16) -> F (direction output), [16, 80) -> F through
        // conv3's ReLU, [80, 208) -> M (the per-sample table gradient)
        {
            constexpr int NI = POL_FEAT / POL_NW;
            static_assert(NI * POL_NW == POL_FEAT, "L0 inputs per wave");
            const int i0 = wv * NI;
            float d[NI];
#pragma unroll
            for (int j = 0; j < NI; j++) d[j] = 0.0f;
            const float *__restrict__ wp = W + L.p0_w + i0, *__restrict__ wq = W + L.v0_w + i0;
#pragma nounroll
            for (int o = 0; o < 64; o++) {
                const float zp = H1[o * LS + lane], zv = H1[(64 + o) * LS + lane];
#pragma unroll
                for (int j = 0; j < NI; j++) {
                    d[j] = __builtin_fmaf(wp[o * POL_FEAT + j], zp, d[j]);
                    d[j] = __builtin_fmaf(wq[o * POL_FEAT + j], zv, d[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < NI; j++) {
                const int i = i0 + j;                                  // wave-uniform
                if (i < 16) F[i * LS + lane] = d[j];
                else if (i < 80) F[i * LS + lane] = F[i * LS + lane] > 0.0f ? d[j] : 0.0f;
                else M[(i - 80) * LS + lane] = d[j];
            }
        }
        __syncthreads();
        // ---- the table gradient: the samples of one (mission id, v) key summed in sample order, then one atomic
        // add per float (64 consecutive floats per wave instruction).  The first sample of a key does its sum.
        {
            const int f = tid & 127, part = tid >> 7;
            for (int s = 0; s < nb; s++) {
                const int ord = s_lead[s];
                if (ord < 0 || (ord & 3) != part) continue;
                const int key = s_key[s];
                float sum = 0.0f;
                for (int q = s; q < nb; q++)
                    if (s_key[q] == key) sum = sum + M[f * LS + q];
                atomicAdd(a.gmf + (size_t)key * 128 + f, sum);
            }
        }
        // ---- direction one-hot -> H1 rows [0, 4K) (dZ1 is dead)
        for (int j = wv; j < 4 * K; j += POL_NW) {
            const int k = j >> 2, dd = j & 3;
            H1[j * LS + lane] = (k >= K - v && ((dsel >> (2 * k)) & 3) == (uint32_t)dd) ? 1.0f : 0.0f;
        }
        __syncthreads();
        // ---- direction Linear (wave 0) and conv3 (waves 0..7): dW = sum_s dZ[o][s] In[i][s]
        if (wv == 0)
            pg_mfma_block(lane, 32, [&](int r, int k) { return r < 16 ? F[r * LS + k] : 0.0f; },
                          [&](int r, int k) { return r < 4 * K ? H1[r * LS + k] : 0.0f; },
                          [&](int m, int n, float x) {
                              if (m < 16 && n < 4 * K) put(L.dir_w + m * 4 * K + n, x);
                          });
        {
            const int o0 = (wv >> 2) * 32, i0 = (wv & 3) * 32;
            pg_mfma_block(lane, 32, [&](int r, int k) { return F[(16 + o0 + r) * LS + k]; },
                          [&](int r, int k) { return C2[(i0 + r) * LS + k]; },
                          [&](int m, int n, float x) { put(L.c3_w + (o0 + m) * 128 + i0 + n, x); });
        }
        bias(F, 16, 1, L.dir_b);
        bias(F + 16 * LS, 64, 1, L.c3_b);
        __syncthreads();
        // dC2 = (W3^T dZ3) through conv2's ReLU, in place over C2: 16 inputs per wave
        {
            const int i0 = wv * 16;
            float d[16];
#pragma unroll
            for (int j = 0; j < 16; j++) d[j] = 0.0f;
            pg_dot_t<16>(d, W + L.c3_w + i0, 128, 64, [&](int o) { return F[(16 + o) * LS + lane]; });
#pragma unroll
            for (int j = 0; j < 16; j++) C2[(i0 + j) * LS + lane] = C2[(i0 + j) * LS + lane] > 0.0f ? d[j] : 0.0f;
        }
        __syncthreads();
        // ---- conv2: dW2[oc][ic][dy][dx] = sum_{pos, s} dC2[oc][pos][s] P[ic][pos + (dy, dx)][s]: 2 blocks, k = (pos, s)
        if (wv < 2) {
            const int j0 = wv * 32;
            pg_mfma_block(lane, 128, [&](int r, int k) { return C2[(r * 4 + (k >> 6)) * LS + (k & 63)]; },
                          [&](int r, int k) {
                              const int j = j0 + r, ic = j >> 2, dy = (j >> 1) & 1, dx = j & 1;
                              const int pos = k >> 6, oy = pos >> 1, ox = pos & 1;
                              return P[(ic * 9 + (oy + dy) * 3 + ox + dx) * LS + (k & 63)];
                          },
                          [&](int m, int n, float x) { put(L.c2_w + m * 64 + j0 + n, x); });
        }
        bias(C2, 32, 4, L.c2_b);
        __syncthreads();
        // dP = conv2's transposed product through the pool's ReLU, in place over P: 2 input channels per wave
        {
            const int ic0 = wv * 2;
            float d[2][9];
#pragma unroll
            for (int q = 0; q < 2; q++)
#pragma unroll
                for (int j = 0; j < 9; j++) d[q][j] = 0.0f;
#pragma nounroll
            for (int oc = 0; oc < 32; oc++) {
                float z[4];
#pragma unroll
                for (int p = 0; p < 4; p++) z[p] = C2[(oc * 4 + p) * LS + lane];
#pragma unroll
                for (int q = 0; q < 2; q++) {
                    const float *__restrict__ wq = W + L.c2_w + (oc * 16 + ic0 + q) * 4;
#pragma unroll
                    for (int dy = 0; dy < 2; dy++)
#pragma unroll
                        for (int dx = 0; dx < 2; dx++) {
                            const float wt = wq[dy * 2 + dx];
#pragma unroll
                            for (int oy = 0; oy < 2; oy++)
#pragma unroll
                                for (int ox = 0; ox < 2; ox++)
                                    d[q][(oy + dy) * 3 + ox + dx] = __builtin_fmaf(wt, z[oy * 2 + ox], d[q][(oy + dy) * 3 + ox + dx]);
                        }
                }
            }
#pragma unroll
            for (int q = 0; q < 2; q++)
#pragma unroll
                for (int j = 0; j < 9; j++) {
                    float *p = P + ((ic0 + q) * 9 + j) * LS + lane;
                    *p = *p > 0.0f ? d[q][j] : 0.0f;
                }
        }
        __syncthreads();                                              // C2 .. H2 are dead: the rows come back
        // ---- conv1: stage the rows again; find every pooled cell's first maximum (window order) as stage B computes
        // it; then dW1[oc][c][dy][dx] = sum_{cell, s} dP[oc][cell][s] x[c][argmax + (dy, dx)][s]
        bias(P, 16, 9, L.c1_b);
        stage_rows();
        __syncthreads();
        {
            int oc0, cell0, cell1;
            pol_conv1_share(wv, oc0, cell0, cell1);
            for (int cell = cell0; cell < cell1; cell++) {
                float acc[4][4];
                pol_conv1_cell<K>(W, xb, oc0, cell, acc);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    int pos = 0;
                    float m = acc[q][0];
#pragma unroll
                    for (int p = 1; p < 4; p++)
                        if (acc[q][p] > m) { m = acc[q][p]; pos = p; }
                    const int idx = (oc0 + q) * 9 + cell;
                    PosB[((idx >> 2) * LS + lane) * 4 + (idx & 3)] = (uint8_t)pos;
                }
            }
        }
        __syncthreads();
        {
            const int oc0 = (wv & 3) * 4;
            for (int c = wv >> 2; c < 3 * K; c += 2) {
                float acc[4][4];
#pragma unroll
                for (int q = 0; q < 4; q++)
#pragma unroll
                    for (int p = 0; p < 4; p++) acc[q][p] = 0.0f;
#pragma nounroll
                for (int cell = 0; cell < 9; cell++) {
                    const int py = cell / 3, px = cell - py * 3;
                    float pix[9];
                    pol_conv1_patch(xb, c, py, px, pix);
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int idx = (oc0 + q) * 9 + cell;
                        const float g = P[idx * LS + lane];
                        const int pos = PosB[((idx >> 2) * LS + lane) * 4 + (idx & 3)];
#pragma unroll
                        for (int p = 0; p < 4; p++) {
                            const float gp = pos == p ? g : 0.0f;
#pragma unroll
                            for (int dy = 0; dy < 2; dy++)
#pragma unroll
                                for (int dx = 0; dx < 2; dx++)
                                    acc[q][dy * 2 + dx] =
                                        __builtin_fmaf(gp, pix[((p >> 1) + dy) * 3 + (p & 1) + dx], acc[q][dy * 2 + dx]);
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; q++)
#pragma unroll
                    for (int p = 0; p < 4; p++) {
                        float x = acc[q][p];
#pragma unroll
                        for (int sh = 1; sh < 64; sh <<= 1) x = x + __shfl_xor(x, sh, 64);
                        if (lane == 0) put(L.c1_w + ((oc0 + q) * 3 * K + c) * 4 + p, x);
                    }
            }
        }
        __syncthreads();                                              // the next tile overwrites everything
    }
}

// grad_blob[w] = slab 0 + slab 1 + ... in group order
__global__ __launch_bounds__(256) void mgx_policy_fold_kernel(const float *__restrict__ scratch, int groups, int words,
                                                              float *__restrict__ out) {
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w >= words) return;
    float s = scratch[w];
    for (int g = 1; g < groups; g++) s = s + scratch[(size_t)g * words + w];
    out[w] = s;
}

#endif  // MGX_POLICY_GRAD_H_
