// mgx_policy.h -- mgx_policy_act: the reference actor-critic's forward pass (policy.py DEFAULT_ARCH, net_arch 64/64
// Tanh, 7 actions) straight from compact rows: actions, values, log-probs and logits of n samples in ONE launch, the
// stacked observation never materialised.  Included by mgx_engine.hip (after splitmix64, FROW and stack_slot).
//
// Mapping (DESIGN.md "Fused actor-critic kernel"): one workgroup of 8 waves per tile of 64 samples.  LANE = SAMPLE in
// every stage; the 8 waves split each layer's OUTPUT channels.  A lane keeps 8..16 fp32 accumulators in registers;
// the weight of an (output, input) pair is the same for all 64 lanes, so its address is wave-uniform and it is read
// from the blob through the scalar cache (L2-resident, 188 KB at n_stack 4; nothing but the input rows and the
// activations is staged).  Activations live in LDS as [feature][sample] with a row stride of 65 dwords: a lane reads
// feature i of its own sample, consecutive lanes hit consecutive banks.  All 64 lanes are busy in every stage of a
// full tile; a tail tile computes zeros in its spare lanes and writes nothing for them.
//
// Stages A to F are the pol_* function templates below, each taking its source and destination LDS regions; pol_trunk
// is their sequence, the one place that defines their order, the barrier after each and which region (PolLds) becomes
// which.  It is the network's one forward pass, run by the three act-side kernels here and by pass (a) of
// mgx_policy_grad_kernel (mgx_policy_grad.h): bootstrap, mixture and gradient are those of what mgx_policy_act returns.
//
//   A   pol_stage_src   per (sample, slot): source row / validity (stack_slot: mgx_gather's walk-back, ring wrap and
//                       terminal rows included)
//   A2  pol_stage_rows  rows -> LDS as dwords [slot][37][65] (coalesced along a row; empty slot = zeros); then each
//                       lane's row of the mission-feature table (pol_feat_row) and the caller's after_rows
//   B   pol_conv1       conv1 2x2 + ReLU + MaxPool 2: rows -> P[144]; before it each lane packs its K direction bytes
//                       into a register (pol_dsel)
//   C   pol_conv2       conv2 2x2 + ReLU: P -> C2[128]
//   D   pol_conv3_dir   conv3 2x2 + ReLU: C2 -> F[16..80); direction Linear (one weight column per valid slot) -> F[0..16)
//   E   pol_l0          policy_net L0 | value_net_body L0 (208 -> 64 each, Tanh): F + mission_feat[mid][v-1][128]
//                       (global) -> H1[128]
//   F   pol_l1          policy_net L1 | value_net_body L1 (64 -> 64 each, Tanh): H1 -> H2[128]
//   G   pol_heads       action_net (7) and value_net (1), arg-max / inverse-cdf sample, log-prob: wave 0 of
//                       mgx_policy_kernel and mgx_policy_moe_kernel (mgx_policy_boot_kernel: the value head alone);
//                       not part of pol_trunk
// The three act-side kernels have two LDS regions in all (pol_act_lds), X = max(37 K, 128) rows (the rows, then C2,
// then H1) and P = 144 rows (the pooled maps, then F, then H2) of 65 dwords: 79 KB at n_stack 4, two workgroups per CU.
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
constexpr int POL_NF = 64 / POL_NW;        // outputs per wave of a 64-wide layer

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

// Which samples a launch works on: sample b's newest frame is row index[b] (flat row * N + env) of a compact buffer
// of N envs, linear (R = 0) or a ring of R rows.  The leading arguments of mgx_gather_ring, mgx_policy_act and
// mgx_policy_backward (sample_addr in mgx_engine.hip checks and fills it).
struct SampleAddr {
    const uint8_t *rows, *mids, *starts;
    int64_t N, R;
    const int64_t *index;
    int64_t B;
};

// The outputs of mgx_policy_act and mgx_policy_act_moe (an mgx_act_out; pol_out in mgx_engine.hip checks and fills it)
struct PolOut {
    long long *actions;
    float *values, *log_probs, *logits;
};

struct PolArgs {
    SampleAddr s;
    const uint8_t *newest;
    const float *blob, *mfeat;
    int mode;
    uint64_t seed;
    unsigned long long *ctr;
    PolOut out;
};

// The forward pass's LDS regions, [feature][POL_LS] floats; one may lie over another that is dead when it is written
struct PolLds {
    float *rows, *P, *C2, *F, *H1, *H2;
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
// pol_dot's load4 for an input in LDS: features i0 .. i0 + 3 of the lane's sample (xin = the region + lane)
__device__ __forceinline__ auto pol_lds4(const float *xin) {
    return [xin](int i0, float (&x)[4]) {
#pragma unroll
        for (int j = 0; j < 4; j++) x[j] = xin[(i0 + j) * POL_LS];
    };
}
// the four outputs of a 2x2 convolution over a 3x3 input, one input channel: acc[oy][ox] += in[oy + dy][ox + dx] *
// wq[dy][dx], the taps (dy, dx) in row order
__device__ __forceinline__ void pol_conv2x2(const float (&in)[9], const float *__restrict__ wq, float (&acc)[4]) {
#pragma unroll
    for (int dy = 0; dy < 2; dy++)
#pragma unroll
        for (int dx = 0; dx < 2; dx++) {
            const float wt = wq[dy * 2 + dx];
#pragma unroll
            for (int oy = 0; oy < 2; oy++)
#pragma unroll
                for (int ox = 0; ox < 2; ox++)
                    acc[oy * 2 + ox] = __builtin_fmaf(in[(oy + dy) * 3 + ox + dx], wt, acc[oy * 2 + ox]);
        }
}

// ---- The forward pass, stage by stage.  Common arguments: tid = thread of the workgroup, lane = tid & 63 = the
// sample, wv = the wave (wave-uniform, so that weight addresses stay scalar), W = the weight blob; activations are
// [feature][POL_LS] floats in LDS.  pol_trunk, after them, puts a barrier between two stages.

// ---- A: source row (nullptr: empty slot) and mission id (-1) of every (sample, slot) of the tile of nb samples at b0;
// slot K-1 is the newest (mgx_gather_kernel's rules)
template <int K>
__device__ __forceinline__ void pol_stage_src(const SampleAddr &s, const uint8_t *newest, int64_t b0, int nb, int tid,
                                              const uint8_t **s_src, int *s_mid) {
    for (int pr = tid; pr < POL_TILE * K; pr += POL_THREADS) {
        const int bi = pr / K, k = pr - bi * K;
        const uint8_t *src = nullptr;
        int mid = -1;
        if (bi < nb) src = stack_slot(s.rows, s.mids, s.starts, s.N, s.R, newest, s.index[b0 + bi], K - 1 - k, mid);
        s_src[pr] = src;
        s_mid[pr] = mid;
    }
}
// ---- A2: stage the rows: X[(k * 37 + w) * 65 + sample] = dword w of slot k
template <int K>
__device__ __forceinline__ void pol_stage_rows(const uint8_t *const *s_src, int tid, float *X) {
    uint32_t *Xu = reinterpret_cast<uint32_t *>(X);
    for (int i = tid; i < POL_TILE * K * POL_RW; i += POL_THREADS) {
        const int pr = i / POL_RW, w = i - pr * POL_RW;
        const int bi = pr / K, k = pr - bi * K;
        const uint8_t *src = s_src[pr];
        Xu[(k * POL_RW + w) * POL_LS + bi] = src ? reinterpret_cast<const uint32_t *>(src)[w] : 0u;
    }
}
// valid slots are contiguous from the newest and share its mission id: v = their count.  Returns the lane's row of the
// mission-feature table [256][K][128], mid * K + v - 1 (row 0 for a spare lane, whose slots are all empty)
template <int K>
__device__ __forceinline__ int pol_feat_row(const int *s_mid, int lane, int nb, int &v) {
    v = 0;
#pragma unroll
    for (int k = 0; k < K; k++) v += s_mid[lane * K + k] >= 0;
    const int my_mid = lane < nb ? s_mid[lane * K + K - 1] : 0;
    return my_mid * K + (v > 0 ? v - 1 : 0);
}
// direction (row byte 0) of slot k at bits 2k; xb = the staged rows + lane * 4
template <int K>
__device__ __forceinline__ uint32_t pol_dsel(const uint8_t *xb) {
    uint32_t dsel = 0;
#pragma unroll
    for (int k = 0; k < K; k++) dsel |= (uint32_t)(xb[(k * POL_RW) * POL_LS * 4] & 3) << (2 * k);
    return dsel;
}
// conv1's 3x3 input patch under pooled cell (py, px) of input channel c (slot c / 3, colour c % 3); pixel = u8 / 255
__device__ __forceinline__ void pol_conv1_patch(const uint8_t *xb, int c, int py, int px, float (&pix)[9]) {
    const int k = c / 3, ch = c - k * 3;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int bp = 1 + ch * 49 + (2 * py + i) * 7 + 2 * px + j;      // byte of the row
            pix[i * 3 + j] = (float)xb[((k * POL_RW + (bp >> 2)) * POL_LS) * 4 + (bp & 3)] * (1.0f / 255.0f);
        }
}
// conv1's four outputs under pooled cell `cell` for output channels oc0 .. oc0 + 3, from a 3x3 patch per input channel
// (16 accumulators, 64 fmaf per 9 pixels)
template <int K>
__device__ __forceinline__ void pol_conv1_cell(const float *__restrict__ W, const uint8_t *xb, int oc0, int cell,
                                               float (&acc)[4][4]) {
    constexpr PolBlob L = pol_blob(K);
    const int py = cell / 3, px = cell - py * 3;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const float bq = W[L.c1_b + oc0 + q];
#pragma unroll
        for (int p = 0; p < 4; p++) acc[q][p] = bq;
    }
#pragma nounroll                       // (at n_stack 2 the 6 trips were unrolled: 284 scalar registers spilled)
    for (int c = 0; c < 3 * K; c++) {
        float pix[9];
        pol_conv1_patch(xb, c, py, px, pix);
#pragma unroll
        for (int q = 0; q < 4; q++) pol_conv2x2(pix, W + L.c1_w + ((oc0 + q) * 3 * K + c) * 4, acc[q]);
    }
}
// a wave's share of conv1's (output channel, pooled cell) pairs: 4 output channels x 5 or 4 of the 9 cells
__device__ __forceinline__ void pol_conv1_share(int wv, int &oc0, int &cell0, int &cell1) {
    oc0 = (wv & 3) * 4;
    cell0 = (wv >> 2) ? 5 : 0;
    cell1 = (wv >> 2) ? 9 : 5;
}
// ---- B: conv1 (3K -> 16, 2x2) + ReLU + MaxPool 2: the rows -> P[144]
template <int K>
__device__ __forceinline__ void pol_conv1(const float *__restrict__ W, int wv, int lane, const uint8_t *xb, float *P) {
    int oc0, cell0, cell1;
    pol_conv1_share(wv, oc0, cell0, cell1);
    for (int cell = cell0; cell < cell1; cell++) {
        float acc[4][4];
        pol_conv1_cell<K>(W, xb, oc0, cell, acc);
#pragma unroll
        for (int q = 0; q < 4; q++)
            P[((oc0 + q) * 9 + cell) * POL_LS + lane] =
                fmaxf(fmaxf(fmaxf(acc[q][0], acc[q][1]), fmaxf(acc[q][2], acc[q][3])), 0.0f);
    }
}
// ---- C: conv2 (16 -> 32, 2x2 on 3x3) + ReLU: P -> C2[128]; wave = 4 output channels x 4 positions (16 accumulators)
template <int K>
__device__ __forceinline__ void pol_conv2(const float *__restrict__ W, int wv, int lane, const float *P, float *C2) {
    constexpr PolBlob L = pol_blob(K);
    constexpr int LS = POL_LS;
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
        for (int q = 0; q < NQ; q++) pol_conv2x2(in, W + L.c2_w + ((oc0 + q) * 16 + ic) * 4, acc[q]);
    }
#pragma unroll
    for (int q = 0; q < NQ; q++)
#pragma unroll
        for (int p = 0; p < 4; p++) C2[((oc0 + q) * 4 + p) * LS + lane] = fmaxf(acc[q][p], 0.0f);
}
// ---- D: conv3 (32 -> 64, 2x2 on 2x2 = a 128 -> 64 dot) + ReLU: C2 -> F[16 .. 80), wave = 8 output channels; direction
// Linear(4K -> 16): bias + one weight column per valid slot (one-hot input) -> F[0 .. 16), wave = 2 outputs
template <int K>
__device__ __forceinline__ void pol_conv3_dir(const float *__restrict__ W, int wv, int lane, uint32_t dsel, int v,
                                              const float *C2, float *F) {
    constexpr PolBlob L = pol_blob(K);
    constexpr int LS = POL_LS, NF = POL_NF;
    const int o0 = wv * NF;
    float acc[NF];
#pragma unroll
    for (int o = 0; o < NF; o++) acc[o] = W[L.c3_b + o0 + o];
    pol_dot<NF>(acc, W + L.c3_w + o0 * 128, 128, 128, pol_lds4(C2 + lane));
#pragma unroll
    for (int o = 0; o < NF; o++) F[(16 + o0 + o) * LS + lane] = fmaxf(acc[o], 0.0f);
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
// ---- E: policy_net L0 | value_net_body L0: 208 -> 64 each, Tanh; wave = 8 + 8 outputs sharing every input.
// Inputs 0..79 from F, 80..207 the (mission, v) feature row mf, read by each lane from the table (float4).
// H1: [0..64) policy, [64..128) value
template <int K>
__device__ __forceinline__ void pol_l0(const float *__restrict__ W, int wv, int lane, const float *__restrict__ mf,
                                       const float *F, float *H1) {
    constexpr PolBlob L = pol_blob(K);
    constexpr int LS = POL_LS, NF = POL_NF;
    float hp[NF], hv[NF];
    const int o0 = wv * NF;
#pragma unroll
    for (int o = 0; o < NF; o++) { hp[o] = W[L.p0_b + o0 + o]; hv[o] = W[L.v0_b + o0 + o]; }
    pol_dot2<NF>(hp, hv, W + L.p0_w + o0 * POL_FEAT, W + L.v0_w + o0 * POL_FEAT, POL_FEAT, 80, pol_lds4(F + lane));
    pol_dot2<NF>(hp, hv, W + L.p0_w + o0 * POL_FEAT + 80, W + L.v0_w + o0 * POL_FEAT + 80, POL_FEAT, 128,
                 [&](int i0, float (&x)[4]) {
                     const float4 m = *reinterpret_cast<const float4 *>(mf + i0);
                     x[0] = m.x; x[1] = m.y; x[2] = m.z; x[3] = m.w;
                 });
#pragma unroll
    for (int o = 0; o < NF; o++) {
        H1[(o0 + o) * LS + lane] = tanhf(hp[o]);
        H1[(64 + o0 + o) * LS + lane] = tanhf(hv[o]);
    }
}
// ---- F: policy_net L1 | value_net_body L1: 64 -> 64 each, Tanh: H1 -> H2[128]
template <int K>
__device__ __forceinline__ void pol_l1(const float *__restrict__ W, int wv, int lane, const float *H1, float *H2) {
    constexpr PolBlob L = pol_blob(K);
    constexpr int LS = POL_LS, NF = POL_NF;
    float hp[NF], hv[NF];
    const int o0 = wv * NF;
#pragma unroll
    for (int o = 0; o < NF; o++) { hp[o] = W[L.p1_b + o0 + o]; hv[o] = W[L.v1_b + o0 + o]; }
    pol_dot<NF>(hp, W + L.p1_w + o0 * 64, 64, 64, pol_lds4(H1 + lane));
    pol_dot<NF>(hv, W + L.v1_w + o0 * 64, 64, 64, pol_lds4(H1 + 64 * LS + lane));
#pragma unroll
    for (int o = 0; o < NF; o++) {
        H2[(o0 + o) * LS + lane] = tanhf(hp[o]);
        H2[(64 + o0 + o) * LS + lane] = tanhf(hv[o]);
    }
}

// ---- A to F in order, with the barrier after each: the forward pass of the tile of nb samples at b0 of s.index, from
// compact rows to r.H2; written here and nowhere else.  s_src / s_mid: stage A's [64 K] arrays in LDS; mfeat: the table
// [256][K][128]; after_rows(feature row): the caller's own work between A2 and its barrier (mgx_policy_grad_kernel
// stages its cotangents there).  Returns what a lane keeps of its sample once the rows are dead.
struct PolLane { int v; uint32_t dsel; };  // valid slots; pol_dsel
template <int K, class AfterRows>
__device__ __forceinline__ PolLane pol_trunk(const SampleAddr &s, const uint8_t *newest, int64_t b0, int nb, int tid,
                                             int lane, int wv, const float *__restrict__ W, const float *mfeat,
                                             const uint8_t **s_src, int *s_mid, const PolLds &r,
                                             AfterRows after_rows) {
    PolLane l;
    pol_stage_src<K>(s, newest, b0, nb, tid, s_src, s_mid);           // A
    __syncthreads();
    pol_stage_rows<K>(s_src, tid, r.rows);                            // A2
    const int frow = pol_feat_row<K>(s_mid, lane, nb, l.v);
    const float *__restrict__ mf = mfeat + (size_t)frow * 128;
    after_rows(frow);
    __syncthreads();
    const uint8_t *xb = reinterpret_cast<const uint8_t *>(r.rows) + lane * 4;
    l.dsel = pol_dsel<K>(xb);
    pol_conv1<K>(W, wv, lane, xb, r.P);                               // B
    __syncthreads();                                                  // rows dead from here
    pol_conv2<K>(W, wv, lane, r.P, r.C2);                             // C
    __syncthreads();
    pol_conv3_dir<K>(W, wv, lane, l.dsel, l.v, r.C2, r.F);            // D
    __syncthreads();
    pol_l0<K>(W, wv, lane, mf, r.F, r.H1);                            // E
    __syncthreads();
    pol_l1<K>(W, wv, lane, r.H1, r.H2);                               // F
    __syncthreads();
    return l;
}
// The act-side kernels' regions, two in all (pol_lds_bytes): X = the rows, then C2, then H1; P = P, then F, then H2
template <int K>
__device__ __forceinline__ PolLds pol_act_lds(uint8_t *smem) {
    float *X = reinterpret_cast<float *>(smem);                       // [pol_x_rows][65]
    float *P = X + pol_x_rows(K) * POL_LS;                            // [144][65]
    return PolLds{X, P, X, P, X, P};
}

// ---- G: action_net and value_net on H2 = P, then the action choice and the outputs of sample b (= the lane's, if
// `live`): wave 0 of mgx_policy_kernel and of mgx_policy_moe_kernel, one sample per lane.  b is the sample's position
// in the caller's index: where its outputs go and what keys its draw.  read_ctr() loads the launch counter (mode 2
// only, by the whole wave, after the heads' dots); the value is returned (0 in the other modes).
template <int K, class ReadCtr>
__device__ __forceinline__ unsigned long long pol_heads(const float *__restrict__ W, const float *P, int lane, bool live,
                                                        int64_t b, int mode, uint64_t seed, ReadCtr read_ctr,
                                                        const PolOut &out) {
    constexpr PolBlob L = pol_blob(K);
    constexpr int LS = POL_LS;
    float lg[POL_NA], val[1];
#pragma unroll
    for (int o = 0; o < POL_NA; o++) lg[o] = W[L.a_b + o];
    val[0] = W[L.vn_b];
    pol_dot<POL_NA>(lg, W + L.a_w, 64, 64, pol_lds4(P + lane));
    pol_dot<1>(val, W + L.vn_w, 64, 64, pol_lds4(P + 64 * LS + lane));
    unsigned long long c = 0;
    if (mode == 2) c = read_ctr();
    if (live) {
        if (out.values) out.values[b] = val[0];
        if (out.logits) {
#pragma unroll
            for (int o = 0; o < POL_NA; o++) out.logits[b * POL_NA + o] = lg[o];
        }
        if (mode != 0) {
            float mx = lg[0];
            int am = 0;
#pragma unroll
            for (int o = 1; o < POL_NA; o++)
                if (lg[o] > mx) { mx = lg[o]; am = o; }              // first index of the maximum
            float cum[POL_NA], tot = 0.0f;
#pragma unroll
            for (int o = 0; o < POL_NA; o++) { tot = tot + expf(lg[o] - mx); cum[o] = tot; }
            int act = am;
            if (mode == 2) {
                const uint64_t key = splitmix64(seed + (uint64_t)c * 0x9E3779B97F4A7C15ull);
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
            out.actions[b] = act;
            out.log_probs[b] = (la - mx) - logf(tot);
        }
    }
    return c;
}

template <int K>
__global__ __launch_bounds__(POL_THREADS, 4) void mgx_policy_kernel(PolArgs a) {
    extern __shared__ __align__(16) uint8_t smem[];
    __shared__ const uint8_t *s_src[POL_TILE * K];
    __shared__ int s_mid[POL_TILE * K];                               // -1: empty slot
    const PolLds r = pol_act_lds<K>(smem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);          // wave-uniform: weight addresses stay scalar
    const int64_t b0 = (int64_t)blockIdx.x * POL_TILE;
    const int nb = (int)min<int64_t>(POL_TILE, a.s.B - b0);
    const float *__restrict__ W = a.blob;
    pol_trunk<K>(a.s, a.newest, b0, nb, tid, lane, wv, W, a.mfeat, s_src, s_mid, r, [](int) {});   // A to F
    // ---- G: heads, action choice and outputs: wave 0, one sample per lane
    if (wv != 0) return;
    const unsigned long long c = pol_heads<K>(
        W, r.H2, lane, lane < nb, b0 + lane, a.mode, a.seed,
        [&] { return *reinterpret_cast<volatile unsigned long long *>(a.ctr); }, a.out);
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

// ---- mgx_policy_bootstrap: rewards[e] += gamma * V(terminal observation of e) for every env with truncated & !terminated
// at one step, the work list built on the device (DESIGN.md "Graph-captured collect").  Two launches.
struct PolBootArgs {
    SampleAddr s;                          // the buffer; index = the list, B unused (the count is on the device)
    int64_t row;                           // sample of env e: flat index row * N + e
    const uint8_t *newest;                 // the terminal rows [N][FROW]
    const float *blob, *mfeat;
    const uint8_t *truncated, *terminated;
    float *rewards;
    float gamma;
    int64_t *list;                         // [N]: flat indices of the selected envs, ascending env
    int *count;                            // [1]
    float *values;                         // optional [N]: V of list entry j at [j]
};

// Launch 1: ordered compaction by ONE workgroup: per chunk of BOOT_THREADS envs a ballot per wave, popcounts below
// the lane, an exclusive scan of the wave totals in LDS.  Entry j of the list is the j-th selected env in ascending
// order (torch's nonzero()); every list entry below the count and the count itself are written, nothing is read back.
constexpr int BOOT_THREADS = 1024;
__global__ __launch_bounds__(BOOT_THREADS) void mgx_boot_list_kernel(PolBootArgs a) {
    constexpr int NWV = BOOT_THREADS / 64;
    __shared__ int s_tot[NWV];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int base = 0;                                                     // selected envs before this chunk (uniform)
    for (int64_t e0 = 0; e0 < a.s.N; e0 += BOOT_THREADS) {
        const int64_t e = e0 + tid;
        const bool sel = e < a.s.N && a.truncated[e] != 0 && a.terminated[e] == 0;
        const unsigned long long m = __ballot(sel);
        if (lane == 0) s_tot[wv] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < NWV; w++) {
            const int c = s_tot[w];
            before += w < wv ? c : 0;
            total += c;
        }
        if (sel) a.list[base + before + __popcll(m & ((1ull << lane) - 1ull))] = a.row * a.s.N + e;
        base += total;
        __syncthreads();                                              // s_tot is rewritten by the next chunk
    }
    if (tid == 0) *a.count = base;
}

// Launch 2: the value pass over the list: the forward pass (pol_trunk) and the value head on the terminal stack of
// every listed sample, then rewards[e] = rewards[e] + gamma * v as two fp32 operations (what the eager index_put_ of
// r[boot] + gamma * V computes).  The count is read from the device, so the grid is sized for the worst case, one
// workgroup per tile of the N envs; a workgroup whose tile lies past the count exits after that one load, and with count
// 0 nothing is stored.  One tile per workgroup, as mgx_policy_kernel: with a loop over tiles around the stages the
// compiler hoists the weight loads out of it (95..127 VGPRs, 20 spilled SGPRs, scratch at n_stack 2).
template <int K>
__global__ __launch_bounds__(POL_THREADS, 4) void mgx_policy_boot_kernel(PolBootArgs a) {
    extern __shared__ __align__(16) uint8_t smem[];
    constexpr PolBlob L = pol_blob(K);
    __shared__ const uint8_t *s_src[POL_TILE * K];
    __shared__ int s_mid[POL_TILE * K];
    const PolLds r = pol_act_lds<K>(smem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float *__restrict__ W = a.blob;
    const int64_t cnt = min<int64_t>(*a.count, a.s.N);                // (a list never holds more than N entries)
    const int64_t b0 = (int64_t)blockIdx.x * POL_TILE;
    if (b0 >= cnt) return;                                            // the whole workgroup: no barrier is skipped
    SampleAddr s = a.s;                                               // the buffer, with the list as the index
    s.index = a.list, s.B = cnt;
    const int nb = (int)min<int64_t>(POL_TILE, cnt - b0);
    pol_trunk<K>(s, a.newest, b0, nb, tid, lane, wv, W, a.mfeat, s_src, s_mid, r, [](int) {});     // A to F
    if (wv != 0) return;                                              // the value head: wave 0, one sample per lane
    float val[1];
    val[0] = W[L.vn_b];
    pol_dot<1>(val, W + L.vn_w, 64, 64, pol_lds4(r.H2 + 64 * POL_LS + lane));
    if (lane < nb) {
        const int64_t e = a.list[b0 + lane] % a.s.N;
        const float gv = __fmul_rn(a.gamma, val[0]);
        a.rewards[e] = __fadd_rn(a.rewards[e], gv);
        if (a.values) a.values[b0 + lane] = val[0];
    }
}

// ---- mgx_policy_act_moe: mgx_policy_act with the weights of expert route[mission id of the newest frame] per sample
// (DESIGN.md "Mission-routed mixture of experts").  Two launches, the shape of the bootstrap's pair above.
constexpr int MOE_MAX = MGX_MOE_MAX_EXPERTS;
constexpr int MOE_REC = MGX_MOE_RECORD_WORDS;  // the record's words; [2e], [2e + 1] = start, count of expert e
constexpr int MOE_REC_TILES = 16, MOE_REC_UNROUTABLE = 17, MOE_REC_CTR = 18;
struct PolMoeArgs {
    SampleAddr s;                          // the caller's index and n_samples
    const uint8_t *newest;
    const float *blob[MOE_MAX], *mfeat[MOE_MAX];
    const uint8_t *route;                  // [256]
    int n_experts, mode;
    uint64_t seed;
    unsigned long long *ctr;
    int *rec;                              // [MOE_REC]
    int64_t *list;                         // [n_samples + 63 n_experts]: SampleAddr.index of launch 2
    int *pos;                              // the same length: the position p of each list entry
    PolOut out;
};

// Launch 1: a stable partition of the positions by expert, by ONE workgroup (mgx_boot_list_kernel's compaction, once
// per expert).  Pass 1 counts every expert's samples (per wave, in registers) and lays the segments out; pass 2 places
// the entries: per chunk of MOE_THREADS positions a ballot per expert and wave, the wave totals in LDS (two buffers
// by chunk parity, so the running segment cursors are updated without a third barrier).  The expert of a position is
// route[mids[index[p]]]: stack_slot's newest slot reads mids[index[p]] with and without terminal rows.
constexpr int MOE_THREADS = 1024;
__global__ __launch_bounds__(MOE_THREADS) void mgx_moe_route_kernel(PolMoeArgs a) {
    constexpr int NWV = MOE_THREADS / 64;
    __shared__ int s_tot[2][NWV][MOE_MAX + 1];                        // [.][.][MOE_MAX]: unroutable (pass 1 only)
    __shared__ int s_cur[MOE_MAX];                                    // next free list slot of every expert
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t n = a.s.B;
    const int E = a.n_experts;
    // mode 2: this launch owns the counter: the snapshot is what every draw of launch 2 uses
    if (tid == 0) {
        unsigned long long c = 0;
        if (a.mode == 2) {
            c = *reinterpret_cast<volatile unsigned long long *>(a.ctr);
            *reinterpret_cast<volatile unsigned long long *>(a.ctr) = c + 1ull;
        }
        a.rec[MOE_REC_CTR] = (int)(uint32_t)c;
        a.rec[MOE_REC_CTR + 1] = (int)(uint32_t)(c >> 32);
    }
    if (tid >= MOE_REC_CTR + 2 && tid < MOE_REC) a.rec[tid] = 0;
    // ---- pass 1: counts (wave-uniform registers: a ballot's popcount per expert)
    int cnt[MOE_MAX + 1];
#pragma unroll
    for (int x = 0; x <= MOE_MAX; x++) cnt[x] = 0;
    for (int64_t p0 = 0; p0 < n; p0 += MOE_THREADS) {
        const int64_t p = p0 + tid;
        const int e = p < n ? (int)a.route[a.s.mids[a.s.index[p]]] : -1;
#pragma unroll
        for (int x = 0; x < MOE_MAX; x++) cnt[x] += __popcll(__ballot(e == x && x < E));
        cnt[MOE_MAX] += __popcll(__ballot(e >= E));
    }
    if (lane == 0) {
#pragma unroll
        for (int x = 0; x <= MOE_MAX; x++) s_tot[0][wv][x] = cnt[x];
    }
    __syncthreads();
    if (tid == 0) {
        int start = 0, tiles = 0;
        for (int x = 0; x < MOE_MAX; x++) {
            int c = 0;
            for (int w = 0; w < NWV; w++) c += s_tot[0][w][x];
            a.rec[2 * x] = start;
            a.rec[2 * x + 1] = c;
            s_cur[x] = start;
            const int t = (c + POL_TILE - 1) / POL_TILE;
            tiles += t;
            start += t * POL_TILE;
        }
        int bad = 0;
        for (int w = 0; w < NWV; w++) bad += s_tot[0][w][MOE_MAX];
        a.rec[MOE_REC_TILES] = tiles;
        a.rec[MOE_REC_UNROUTABLE] = bad;
    }
    __syncthreads();
    // ---- pass 2: placement.  Slots stay below n + 63 E: segment e ends at start_e + count_e <= the padded total
    int par = 1;                                                      // (buffer 0 was read by thread 0 above)
    for (int64_t p0 = 0; p0 < n; p0 += MOE_THREADS, par ^= 1) {
        const int64_t p = p0 + tid;
        int64_t idx = 0;
        int e = -1;
        if (p < n) {
            idx = a.s.index[p];
            e = (int)a.route[a.s.mids[idx]];
        }
        const bool sel = e >= 0 && e < E;
        unsigned long long mine = 0;
#pragma unroll
        for (int x = 0; x < MOE_MAX; x++) {
            const unsigned long long m = __ballot(sel && e == x);
            if (e == x) mine = m;
            if (lane == x) s_tot[par][wv][x] = __popcll(m);
        }
        __syncthreads();
        if (sel) {
            int before = 0;
            for (int w = 0; w < wv; w++) before += s_tot[par][w][e];
            const int slot = s_cur[e] + before + __popcll(mine & ((1ull << lane) - 1ull));
            a.list[slot] = idx;
            a.pos[slot] = (int)p;
        }
        __syncthreads();                                              // s_cur was read by everyone
        if (tid < MOE_MAX) {
            int total = 0;
            for (int w = 0; w < NWV; w++) total += s_tot[par][w][tid];
            s_cur[tid] += total;                                      // read next after the next chunk's first barrier
        }
    }
}

// Launch 2: the policy pass over the partition.  Tile t of the lists (entries 64 t .. 64 t + 63) belongs to the expert
// whose segment holds it; a segment starts at a multiple of 64, so no tile has two experts.  The live tiles number
// sum_e ceil(c_e / 64) <= sum_e (c_e + 63) / 64 <= (n_samples + 63 E) / 64, rounded down because the left side is an
// integer: that is the grid.  A workgroup past the live tile count exits after that one load.  One tile per
// workgroup, as mgx_policy_kernel.
template <int K>
__global__ __launch_bounds__(POL_THREADS, 4) void mgx_policy_moe_kernel(PolMoeArgs a) {
    extern __shared__ __align__(16) uint8_t smem[];
    __shared__ const uint8_t *s_src[POL_TILE * K];
    __shared__ int s_mid[POL_TILE * K];
    const PolLds r = pol_act_lds<K>(smem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = (int)blockIdx.x;
    if (tile >= a.rec[MOE_REC_TILES]) return;                         // the whole workgroup: no barrier is skipped
    int e = 0, nb = 0;
    for (int x = 0; x < a.n_experts; x++) {                           // <= 8 records; exactly one holds a live tile
        const int t0 = a.rec[2 * x] / POL_TILE, c = a.rec[2 * x + 1];
        if (tile >= t0 && (tile - t0) * POL_TILE < c) {
            e = x;
            nb = min(POL_TILE, c - (tile - t0) * POL_TILE);
        }
    }
    e = __builtin_amdgcn_readfirstlane(e);                            // wave-uniform: weight addresses stay scalar
    nb = __builtin_amdgcn_readfirstlane(nb);
    const float *__restrict__ W = a.blob[e];
    const int64_t b0 = (int64_t)tile * POL_TILE;                      // the tile's first list slot
    SampleAddr s = a.s;                                               // the buffer, with the partition as the index
    s.index = a.list, s.B = b0 + nb;
    pol_trunk<K>(s, a.newest, b0, nb, tid, lane, wv, W, a.mfeat[e], s_src, s_mid, r, [](int) {});  // A to F
    if (wv != 0) return;                                              // G: wave 0; outputs and the draw's key at p
    const int64_t p = lane < nb ? a.pos[b0 + lane] : 0;
    pol_heads<K>(W, r.H2, lane, lane < nb, p, a.mode, a.seed,
                 [&] { return *reinterpret_cast<const unsigned long long *>(a.rec + MOE_REC_CTR); }, a.out);
}

#endif  // MGX_POLICY_H_
