// mgx_policy.h -- mgx_policy_act: the reference actor-critic's forward pass (policy.py DEFAULT_ARCH, net_arch 64/64
// Tanh, 7 actions) straight from compact rows: actions, values, log-probs and logits of n samples in ONE launch, the
// stacked observation never materialised.  Included by mgx_engine.hip (after splitmix64 and FROW).
//
// Mapping (DESIGN.md "Fused actor-critic kernel"): one workgroup of 8 waves per tile of 64 samples.  LANE = SAMPLE in
// every stage; the 8 waves split each layer's OUTPUT channels.  A lane keeps 8..16 fp32 accumulators in registers;
// the weight of an (output, input) pair is the same for all 64 lanes, so its address is wave-uniform and it is read
// from the blob through the scalar cache (L2-resident, 188 KB at n_stack 4; nothing but the input rows and the
// activations is staged).  Activations live in LDS as [feature][sample] with a row stride of 65 dwords: a lane reads
// feature i of its own sample, consecutive lanes hit consecutive banks.  All 64 lanes are busy in every stage of a
// full tile; a tail tile computes zeros in its spare lanes and writes nothing for them.
//
//   A   per (sample, slot): source row / validity (mgx_gather's walk-back, ring wrap and terminal rows included)
//   A2  rows -> LDS as dwords [slot][37][65] (coalesced along a row; empty slot = zeros)
//   B   conv1 2x2 + ReLU + MaxPool 2: rows (X) -> P[144]; each lane keeps its K direction bytes in a register
//   C   conv2 2x2 + ReLU: P -> C2[128] in X (the rows are dead)
//   D   conv3 2x2 + ReLU: C2 -> F[16..80) in P (dead after C); direction Linear (one weight column per valid
//       slot) -> F[0..16)
//   E   policy_net L0 | value_net_body L0 (208 -> 64 each, Tanh): F + mission_feat[mid][v-1][128] (global) -> H1[128] in X
//   F   policy_net L1 | value_net_body L1 (64 -> 64 each, Tanh): H1 -> H2[128] in P
//   G   action_net (7) and value_net (1), arg-max / inverse-cdf sample, log-prob: wave 0
// Two LDS regions in all, X = max(37 K, 128) rows and P = 144 rows of 65 dwords: 79 KB at n_stack 4, two workgroups
// per CU.
// fp32 throughout, every multiply-add an explicit fmaf (the library is built with -ffp-contract=off).
#ifndef MGX_POLICY_H_
#define MGX_POLICY_H_

constexpr int POL_TILE = 64;               // samples per workgroup (= lanes of a wave)
constexpr int POL_NW = 8;                  // waves per workgroup: they split every layer's outputs
constexpr int POL_THREADS = 64 * POL_NW;
constexpr int POL_LS = 65;                 // LDS row stride in dwords (64 samples + 1: conflict-free staging writes)
constexpr int POL_RW = FROW / 4;           // 37 dwords per compact row
constexpr int POL_FEAT = 208;              // direction 16 | image 64 | mission 128
constexpr int POL_NA = 7;

// Offsets (fp32 words) of the packed weight blob, in include/mgx.h's order.
struct PolBlob {
    int dir_w, dir_b, c1_w, c1_b, c2_w, c2_b, c3_w, c3_b, p0_w, p0_b, p1_w, p1_b, v0_w, v0_b, v1_w, v1_b, a_w, a_b,
        vn_w, vn_b, words;
};
__host__ __device__ constexpr PolBlob pol_blob(int K) {
    PolBlob b{};
    int o = 0;
    b.dir_w = o; o += 16 * 4 * K;  b.dir_b = o; o += 16;
    b.c1_w = o;  o += 16 * 3 * K * 4; b.c1_b = o; o += 16;
    b.c2_w = o;  o += 32 * 16 * 4; b.c2_b = o; o += 32;
    b.c3_w = o;  o += 64 * 32 * 4; b.c3_b = o; o += 64;
    b.p0_w = o;  o += 64 * POL_FEAT; b.p0_b = o; o += 64;
    b.p1_w = o;  o += 64 * 64; b.p1_b = o; o += 64;
    b.v0_w = o;  o += 64 * POL_FEAT; b.v0_b = o; o += 64;
    b.v1_w = o;  o += 64 * 64; b.v1_b = o; o += 64;
    b.a_w = o;   o += POL_NA * 64; b.a_b = o; o += POL_NA;
    b.vn_w = o;  o += 64; b.vn_b = o; o += 1;
    b.words = o;
    return b;
}
static_assert(pol_blob(4).words == 46984, "blob layout");

// dynamic LDS of mgx_policy_kernel<K>: X (rows, then C2, then H1) | P (pooled conv1, then F = direction | image, then H2)
__host__ __device__ constexpr int pol_x_rows(int K) { return K * POL_RW > 128 ? K * POL_RW : 128; }
__host__ __device__ constexpr size_t pol_lds_bytes(int K) { return (size_t)(pol_x_rows(K) + 144) * POL_LS * 4; }

struct PolArgs {
    const uint8_t *rows, *mids, *starts;
    int64_t N, R;
    const int64_t *index;
    int64_t B;
    const uint8_t *newest;
    const float *blob, *mfeat;
    int mode;
    uint64_t seed;
    unsigned long long *ctr;
    long long *actions;
    float *values, *log_probs, *logits;
};

// acc[o] += sum_i w[o * ldw + i] * x(i), i ascending, x four at a time through `load4` (each value feeds NO chains)
template <int NO, class L4>
__device__ __forceinline__ void pol_dot(float (&acc)[NO], const float *__restrict__ w, int ldw, int nin, L4 load4) {
#pragma nounroll                       // (unrolled, the scalar weight loads of many iterations are hoisted and spill)
    for (int i0 = 0; i0 < nin; i0 += 4) {
        float x[4];
        load4(i0, x);
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int o = 0; o < NO; o++) acc[o] = __builtin_fmaf(x[j], w[o * ldw + i0 + j], acc[o]);
    }
}
// the same for two layers that share their input (policy_net L0 and value_net_body L0)
template <int NO, class L4>
__device__ __forceinline__ void pol_dot2(float (&a)[NO], float (&b)[NO], const float *__restrict__ wa,
                                         const float *__restrict__ wb, int ldw, int nin, L4 load4) {
#pragma nounroll                       // (unrolled, the scalar weight loads of many iterations are hoisted and spill)
    for (int i0 = 0; i0 < nin; i0 += 4) {
        float x[4];
        load4(i0, x);
#pragma unroll
        for (int j = 0; j < 4; j++) {
#pragma unroll
            for (int o = 0; o < NO; o++) a[o] = __builtin_fmaf(x[j], wa[o * ldw + i0 + j], a[o]);
#pragma unroll
            for (int o = 0; o < NO; o++) b[o] = __builtin_fmaf(x[j], wb[o * ldw + i0 + j], b[o]);
        }
    }
}

template <int K>
__global__ __launch_bounds__(POL_THREADS, 4) void mgx_policy_kernel(PolArgs a) {
    extern __shared__ __align__(16) uint8_t smem[];
    constexpr PolBlob L = pol_blob(K);
    constexpr int LS = POL_LS;
    float *X = reinterpret_cast<float *>(smem);                       // [pol_x_rows][65]
    float *P = X + pol_x_rows(K) * LS;                                // [144][65]
    float *F = P;                                                     // [80][65], once the pooled maps are dead
    __shared__ const uint8_t *s_src[POL_TILE * K];
    __shared__ int s_mid[POL_TILE * K];                               // -1: empty slot
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);          // wave-uniform: weight addresses stay scalar
    const int64_t b0 = (int64_t)blockIdx.x * POL_TILE;
    const int nb = (int)min<int64_t>(POL_TILE, a.B - b0);
    const float *__restrict__ W = a.blob;

    // ---- A: source row and validity of every (sample, slot); slot K-1 is the newest (mgx_gather_kernel's rules)
    for (int pr = tid; pr < POL_TILE * K; pr += POL_THREADS) {
        const int bi = pr / K, k = pr - bi * K;
        const uint8_t *src = nullptr;
        int mid = -1;
        if (bi < nb) {
            const int64_t idx = a.index[b0 + bi];
            const int64_t row0 = idx / a.N, env = idx - row0 * a.N;
            const int64_t R = a.R;
            const auto back_idx = [&](int j) -> int64_t {
                int64_t r = row0 - j;
                if (R > 0 && r < 0) r += ((-r + R - 1) / R) * R;
                return r * a.N + env;
            };
            const int back = K - 1 - k;
            if (a.newest) {
                if (back == 0) { src = a.newest + env * FROW; mid = a.mids[idx]; }
                else {
                    bool ok = true;
                    for (int j = 0; j < back - 1 && ok; j++) ok = !a.starts[back_idx(j)];
                    if (ok) { const int64_t r = back_idx(back - 1); src = a.rows + r * FROW; mid = a.mids[r]; }
                }
            } else {
                bool ok = true;
                for (int j = 0; j < back && ok; j++) ok = !a.starts[back_idx(j)];
                if (ok) { const int64_t r = back_idx(back); src = a.rows + r * FROW; mid = a.mids[r]; }
            }
        }
        s_src[pr] = src;
        s_mid[pr] = mid;
    }
    __syncthreads();
    // ---- A2: stage the rows: X[(k * 37 + w) * 65 + sample] = dword w of slot k
    {
        uint32_t *Xu = reinterpret_cast<uint32_t *>(X);
        for (int i = tid; i < POL_TILE * K * POL_RW; i += POL_THREADS) {
            const int pr = i / POL_RW, w = i - pr * POL_RW;
            const int bi = pr / K, k = pr - bi * K;
            const uint8_t *src = s_src[pr];
            Xu[(k * POL_RW + w) * LS + bi] = src ? reinterpret_cast<const uint32_t *>(src)[w] : 0u;
        }
    }
    // valid slots are contiguous from the newest and share its mission id: v = their count
    int v = 0;
#pragma unroll
    for (int k = 0; k < K; k++) v += s_mid[lane * K + k] >= 0;
    const int my_mid = lane < nb ? s_mid[lane * K + K - 1] : 0;
    const float *__restrict__ mf = a.mfeat + ((size_t)my_mid * K + (v > 0 ? v - 1 : 0)) * 128;
    __syncthreads();
    const uint8_t *xb = reinterpret_cast<const uint8_t *>(X) + lane * 4;

    uint32_t dsel = 0;                                                // direction (row byte 0) of slot k at bits 2k
#pragma unroll
    for (int k = 0; k < K; k++) dsel |= (uint32_t)(xb[(k * POL_RW) * LS * 4] & 3) << (2 * k);
    // ---- B: conv1 (3K -> 16, 2x2) + ReLU + MaxPool 2: wave = 4 output channels x 5 or 4 of the 9 pooled cells;
    // per pooled cell the 2x2 conv outputs under it from a 3x3 input patch per channel (16 accumulators, 64 fmaf
    // per 9 pixels)
    {
        const int oc0 = (wv & 3) * 4;
        const int cell0 = (wv >> 2) ? 5 : 0, cell1 = (wv >> 2) ? 9 : 5;
        for (int cell = cell0; cell < cell1; cell++) {
            const int py = cell / 3, px = cell - py * 3;
            float acc[4][4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float bq = W[L.c1_b + oc0 + q];
#pragma unroll
                for (int p = 0; p < 4; p++) acc[q][p] = bq;
            }
#pragma nounroll                       // (at n_stack 2 the 6 trips were unrolled: 284 scalar registers spilled)
            for (int c = 0; c < 3 * K; c++) {
                const int k = c / 3, ch = c - k * 3;
                float pix[9];
#pragma unroll
                for (int i = 0; i < 3; i++)
#pragma unroll
                    for (int j = 0; j < 3; j++) {
                        const int bp = 1 + ch * 49 + (2 * py + i) * 7 + 2 * px + j;      // byte of the row
                        pix[i * 3 + j] = (float)xb[((k * POL_RW + (bp >> 2)) * LS) * 4 + (bp & 3)] * (1.0f / 255.0f);
                    }
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const float *__restrict__ wq = W + L.c1_w + ((oc0 + q) * 3 * K + c) * 4;
#pragma unroll
                    for (int dy = 0; dy < 2; dy++)
#pragma unroll
                        for (int dx = 0; dx < 2; dx++) {
                            const float wt = wq[dy * 2 + dx];
#pragma unroll
                            for (int oy = 0; oy < 2; oy++)
#pragma unroll
                                for (int ox = 0; ox < 2; ox++)
                                    acc[q][oy * 2 + ox] = __builtin_fmaf(pix[(oy + dy) * 3 + ox + dx], wt, acc[q][oy * 2 + ox]);
                        }
                }
            }
#pragma unroll
            for (int q = 0; q < 4; q++)
                P[((oc0 + q) * 9 + cell) * LS + lane] =
                    fmaxf(fmaxf(fmaxf(acc[q][0], acc[q][1]), fmaxf(acc[q][2], acc[q][3])), 0.0f);
        }
    }
    __syncthreads();                                                  // rows dead from here: X becomes C2
    // ---- C: conv2 (16 -> 32, 2x2 on 3x3) + ReLU: wave = 4 output channels x 4 positions (16 accumulators)
    {
        constexpr int NQ = 32 / POL_NW;
        const int oc0 = wv * NQ;
        float acc[NQ][4];
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const float bq = W[L.c2_b + oc0 + q];
#pragma unroll
            for (int p = 0; p < 4; p++) acc[q][p] = bq;
        }
        for (int ic = 0; ic < 16; ic++) {
            float in[9];
#pragma unroll
            for (int j = 0; j < 9; j++) in[j] = P[(ic * 9 + j) * LS + lane];
#pragma unroll
            for (int q = 0; q < NQ; q++) {
                const float *__restrict__ wq = W + L.c2_w + ((oc0 + q) * 16 + ic) * 4;
#pragma unroll
                for (int dy = 0; dy < 2; dy++)
#pragma unroll
                    for (int dx = 0; dx < 2; dx++) {
                        const float wt = wq[dy * 2 + dx];
#pragma unroll
                        for (int oy = 0; oy < 2; oy++)
#pragma unroll
                            for (int ox = 0; ox < 2; ox++)
                                acc[q][oy * 2 + ox] = __builtin_fmaf(in[(oy + dy) * 3 + ox + dx], wt, acc[q][oy * 2 + ox]);
                    }
            }
        }
#pragma unroll
        for (int q = 0; q < NQ; q++)
#pragma unroll
            for (int p = 0; p < 4; p++) X[((oc0 + q) * 4 + p) * LS + lane] = fmaxf(acc[q][p], 0.0f);
    }
    __syncthreads();
    // ---- D: conv3 (32 -> 64, 2x2 on 2x2 = a 128 -> 64 dot) + ReLU -> F[16 .. 80): wave = 8 output channels
    constexpr int NF = 64 / POL_NW;                                   // outputs per wave of a 64-wide layer
    {
        const int o0 = wv * NF;
        float acc[NF];
#pragma unroll
        for (int o = 0; o < NF; o++) acc[o] = W[L.c3_b + o0 + o];
        const float *xin = X + lane;
        pol_dot<NF>(acc, W + L.c3_w + o0 * 128, 128, 128, [&](int i0, float (&x)[4]) {
#pragma unroll
            for (int j = 0; j < 4; j++) x[j] = xin[(i0 + j) * LS];
        });
#pragma unroll
        for (int o = 0; o < NF; o++) F[(16 + o0 + o) * LS + lane] = fmaxf(acc[o], 0.0f);
        // direction Linear(4K -> 16): bias + one weight column per valid slot (one-hot input); wave = 2 outputs
#pragma unroll
        for (int q = 0; q < 16 / POL_NW; q++) {
            const int o = wv * (16 / POL_NW) + q;
            float acc1 = W[L.dir_b + o];
#pragma unroll
            for (int k = 0; k < K; k++) {
                const float wt = W[L.dir_w + o * 4 * K + 4 * k + ((dsel >> (2 * k)) & 3)];
                acc1 = __builtin_fmaf(k >= K - v ? 1.0f : 0.0f, wt, acc1);
            }
            F[o * LS + lane] = acc1;
        }
    }
    __syncthreads();
    // ---- E: policy_net L0 | value_net_body L0: 208 -> 64 each, Tanh; wave = 8 + 8 outputs sharing every input.
    // Inputs 0..79 from F, 80..207 the (mission, v) feature row, read by each lane from the table (float4)
    float hp[NF], hv[NF];
    {
        const int o0 = wv * NF;
#pragma unroll
        for (int o = 0; o < NF; o++) { hp[o] = W[L.p0_b + o0 + o]; hv[o] = W[L.v0_b + o0 + o]; }
        const float *xin = F + lane;
        pol_dot2<NF>(hp, hv, W + L.p0_w + o0 * POL_FEAT, W + L.v0_w + o0 * POL_FEAT, POL_FEAT, 80,
                     [&](int i0, float (&x)[4]) {
#pragma unroll
                         for (int j = 0; j < 4; j++) x[j] = xin[(i0 + j) * LS];
                     });
        pol_dot2<NF>(hp, hv, W + L.p0_w + o0 * POL_FEAT + 80, W + L.v0_w + o0 * POL_FEAT + 80, POL_FEAT, 128,
                     [&](int i0, float (&x)[4]) {
                         const float4 m = *reinterpret_cast<const float4 *>(mf + i0);
                         x[0] = m.x; x[1] = m.y; x[2] = m.z; x[3] = m.w;
                     });
#pragma unroll
        for (int o = 0; o < NF; o++) {                                // H1 = X: [0..64) policy, [64..128) value
            X[(o0 + o) * LS + lane] = tanhf(hp[o]);
            X[(64 + o0 + o) * LS + lane] = tanhf(hv[o]);
        }
    }
    __syncthreads();
    // ---- F: policy_net L1 | value_net_body L1: 64 -> 64 each, Tanh -> H2 = P
    {
        const int o0 = wv * NF;
#pragma unroll
        for (int o = 0; o < NF; o++) { hp[o] = W[L.p1_b + o0 + o]; hv[o] = W[L.v1_b + o0 + o]; }
        const float *xp = X + lane, *xv = X + 64 * LS + lane;
        pol_dot<NF>(hp, W + L.p1_w + o0 * 64, 64, 64, [&](int i0, float (&x)[4]) {
#pragma unroll
            for (int j = 0; j < 4; j++) x[j] = xp[(i0 + j) * LS];
        });
        pol_dot<NF>(hv, W + L.v1_w + o0 * 64, 64, 64, [&](int i0, float (&x)[4]) {
#pragma unroll
            for (int j = 0; j < 4; j++) x[j] = xv[(i0 + j) * LS];
        });
#pragma unroll
        for (int o = 0; o < NF; o++) {
            P[(o0 + o) * LS + lane] = tanhf(hp[o]);
            P[(64 + o0 + o) * LS + lane] = tanhf(hv[o]);
        }
    }
    __syncthreads();
    // ---- G: heads, action choice and outputs: wave 0, one sample per lane
    if (wv != 0) return;
    float lg[POL_NA], val[1];
#pragma unroll
    for (int o = 0; o < POL_NA; o++) lg[o] = W[L.a_b + o];
    val[0] = W[L.vn_b];
    {
        const float *xp = P + lane, *xv = P + 64 * LS + lane;
        pol_dot<POL_NA>(lg, W + L.a_w, 64, 64, [&](int i0, float (&x)[4]) {
#pragma unroll
            for (int j = 0; j < 4; j++) x[j] = xp[(i0 + j) * LS];
        });
        pol_dot<1>(val, W + L.vn_w, 64, 64, [&](int i0, float (&x)[4]) {
#pragma unroll
            for (int j = 0; j < 4; j++) x[j] = xv[(i0 + j) * LS];
        });
    }
    unsigned long long c = 0;
    if (a.mode == 2) c = *reinterpret_cast<volatile unsigned long long *>(a.ctr);
    if (lane < nb) {
        const int64_t b = b0 + lane;
        if (a.values) a.values[b] = val[0];
        if (a.logits) {
#pragma unroll
            for (int o = 0; o < POL_NA; o++) a.logits[b * POL_NA + o] = lg[o];
        }
        if (a.mode != 0) {
            float mx = lg[0];
            int am = 0;
#pragma unroll
            for (int o = 1; o < POL_NA; o++)
                if (lg[o] > mx) { mx = lg[o]; am = o; }              // first index of the maximum
            float cum[POL_NA], tot = 0.0f;
#pragma unroll
            for (int o = 0; o < POL_NA; o++) { tot = tot + expf(lg[o] - mx); cum[o] = tot; }
            int act = am;
            if (a.mode == 2) {
                const uint64_t key = splitmix64(a.seed + (uint64_t)c * 0x9E3779B97F4A7C15ull);
                const uint64_t h = splitmix64(key ^ ((uint64_t)b * 0xD1B54A32D192ED03ull));
                const float u = (float)(uint32_t)(h >> 40) * (1.0f / 16777216.0f);
                const float thr = u * tot;
                act = POL_NA - 1;
#pragma unroll
                for (int o = POL_NA - 2; o >= 0; o--)
                    if (cum[o] > thr) act = o;                        // ends at the smallest such index
            }
            float la = lg[0];
#pragma unroll
            for (int o = 1; o < POL_NA; o++) la = act == o ? lg[o] : la;
            a.actions[b] = act;
            a.log_probs[b] = (la - mx) - logf(tot);
        }
    }
    // the launch counter, as mgx_random_actions_kernel: every workgroup has read it (above, the whole wave) before its
    // own tally add; the last one to arrive advances it
    if (a.mode == 2 && tid == 0) {
        __threadfence();
        if (atomicAdd(reinterpret_cast<unsigned int *>(a.ctr + 1), 1u) == gridDim.x - 1) {
            *reinterpret_cast<volatile unsigned long long *>(a.ctr) = c + 1ull;
            *reinterpret_cast<volatile unsigned int *>(a.ctr + 1) = 0u;
            __threadfence();
        }
    }
}

#endif  // MGX_POLICY_H_
