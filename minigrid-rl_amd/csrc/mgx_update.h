// The PPO update's tail (include/mgx.h, added within ABI 9): mgx_ppo_loss and mgx_adam_step, and
// mgx_adam_step_sched, the same step with its per-step scalars read from a device table (§4.11).
//
// mgx_ppo_loss   PPO.train's loss block on the (logits, values) mgx_policy_act mode 0 wrote: the loss, its
//                statistics and the cotangents mgx_policy_backward consumes, lane = sample, fp32 with expf / logf.
// mgx_adam_step  clip_grad_norm_ + Adam.step over one flat array, lane = word.
//
// Reductions.  Every sum over samples or words is taken the same way: a thread adds its elements in index order
// (i, i + grid, ...) into fp64, the 256 threads of a workgroup are added by a fixed LDS tree, the workgroup's
// partial goes to the caller's scratch, and the NEXT launch on the stream adds the <= 256 partials by the same
// tree (one partial per thread).  No float atomics, no counter, no workgroup waits for another: the order of
// every addition is a function of the element count alone, so every output is bitwise reproducible.
#pragma once

#define UP_THREADS 256
#define UP_MAX_GROUPS 256          // partials per reduction: one per thread of the workgroup that folds them
#define UP_LOSS_PER_GROUP 256      // samples per workgroup and pass while the grid is below UP_MAX_GROUPS
#define UP_ADAM_PER_GROUP 1024     // words per workgroup likewise (~110 k words: 108 workgroups)
#define UP_STATS 5                 // per-sample sums: min(A r, A clamp r), (ret - vp)^2, H, (r - 1) - log r, clipped

// v[j] <- sum over the workgroup's threads of v[j], the same tree for every call; lds: N * UP_THREADS doubles
template <int N>
__device__ inline void up_block_sum(double (&v)[N], double *lds) {
    const int t = threadIdx.x;
#pragma unroll
    for (int j = 0; j < N; j++) lds[j * UP_THREADS + t] = v[j];
    __syncthreads();
    for (int s = UP_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int j = 0; j < N; j++) lds[j * UP_THREADS + t] = lds[j * UP_THREADS + t] + lds[j * UP_THREADS + t + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < N; j++) v[j] = lds[j * UP_THREADS];
    __syncthreads();               // the caller may fill lds again
}

struct PpoLossArgs {
    const float *logits, *values;
    const int64_t *sel, *actions;
    const float *old_values, *old_log_probs, *advantages, *returns, *adv_stats;
    float *g_logits, *g_values, *stats;
    double *adv_part;              // [groups][2]: sum (a - a0), sum (a - a0)^2
    double *stat_part;             // [groups][UP_STATS]
    int64_t B;
    int groups, adv_mode;
    float lo, hi, clip, clip_vf, ent_coef, vf_coef, inv_b;
};

__device__ inline int64_t up_sel(const PpoLossArgs &a, int64_t i) { return a.sel ? a.sel[i] : i; }

// adv_mode 1, pass 1: the advantage sums, shifted by the first sample's advantage (no cancellation in the variance)
__global__ __launch_bounds__(UP_THREADS) void mgx_ppo_adv_kernel(PpoLossArgs a) {
    __shared__ double lds[2 * UP_THREADS];
    const double a0 = (double)a.advantages[up_sel(a, 0)];
    double v[2] = {0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * UP_THREADS + threadIdx.x; i < a.B; i += (int64_t)gridDim.x * UP_THREADS) {
        const double x = (double)a.advantages[up_sel(a, i)] - a0;
        v[0] = v[0] + x;
        v[1] = v[1] + x * x;
    }
    up_block_sum<2>(v, lds);
    if (threadIdx.x == 0) {
        a.adv_part[2 * blockIdx.x] = v[0];
        a.adv_part[2 * blockIdx.x + 1] = v[1];
    }
}

__global__ __launch_bounds__(UP_THREADS) void mgx_ppo_loss_kernel(PpoLossArgs a) {
    __shared__ double lds[UP_STATS * UP_THREADS];
    const int t = threadIdx.x;
    float mean = 0.f, sd = 1.f;
    if (a.adv_mode == 1) {         // every workgroup folds the same partials in the same order
        double v[2] = {0.0, 0.0};
        if (t < a.groups) {
            v[0] = a.adv_part[2 * t];
            v[1] = a.adv_part[2 * t + 1];
        }
        up_block_sum<2>(v, lds);
        const double n = (double)a.B;
        const double m = v[0] / n;
        double var = (v[1] - v[0] * m) / (n - 1.0);         // unbiased, as Tensor.std()
        if (var < 0.0) var = 0.0;
        mean = (float)((double)a.advantages[up_sel(a, 0)] + m);
        sd = (float)sqrt(var);
    } else if (a.adv_mode == 2) {
        mean = a.adv_stats[0];
        sd = a.adv_stats[1];
    }
    const float den = sd + 1e-8f;
    if (blockIdx.x == 0 && t == 0) {
        a.stats[6] = mean;
        a.stats[7] = sd;
    }
    double acc[UP_STATS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const float ent_b = a.ent_coef * a.inv_b;
    for (int64_t i = (int64_t)blockIdx.x * UP_THREADS + t; i < a.B; i += (int64_t)gridDim.x * UP_THREADS) {
        const int64_t e = up_sel(a, i);
        float z[7], p[7], logp[7];
        float zmax = -INFINITY;
#pragma unroll
        for (int j = 0; j < 7; j++) {
            z[j] = a.logits[i * 7 + j];
            zmax = fmaxf(zmax, z[j]);
        }
        float total = 0.f;
#pragma unroll
        for (int j = 0; j < 7; j++) {
            z[j] = z[j] - zmax;
            p[j] = expf(z[j]);
            total = total + p[j];
        }
        const float log_total = logf(total);
        int64_t act = a.actions[e];
        act = act < 0 ? 0 : (act > 6 ? 6 : act);
        float H = 0.f, lp = 0.f;
#pragma unroll
        for (int j = 0; j < 7; j++) {
            logp[j] = z[j] - log_total;
            p[j] = p[j] / total;
            H = H - p[j] * logp[j];
            lp = (j == (int)act) ? logp[j] : lp;
        }
        float A = a.advantages[e];
        if (a.adv_mode != 0) A = (A - mean) / den;
        const float log_r = lp - a.old_log_probs[e];
        const float r = expf(log_r);
        const float rc = fminf(fmaxf(r, a.lo), a.hi);
        const float pl1 = A * r, pl2 = A * rc;
        // torch.min ties inside the range and splits the gradient, the clamp passes its half: the full gradient
        const bool pass = (r >= a.lo && r <= a.hi) || pl1 < pl2;
        const float g_lp = pass ? -(pl1 * a.inv_b) : 0.f;
#pragma unroll
        for (int j = 0; j < 7; j++) {
            const float onehot = (j == (int)act) ? 1.f : 0.f;
            a.g_logits[i * 7 + j] = g_lp * (onehot - p[j]) + ent_b * (p[j] * (logp[j] + H));
        }
        const float v = a.values[i], ov = a.old_values[e];
        float vp = v;
        bool inside = true;
        if (a.clip_vf > 0.f) {
            const float d = v - ov;
            inside = d >= -a.clip_vf && d <= a.clip_vf;
            vp = ov + fminf(fmaxf(d, -a.clip_vf), a.clip_vf);
        }
        const float diff = vp - a.returns[e];
        a.g_values[i] = inside ? a.vf_coef * (2.f * diff * a.inv_b) : 0.f;
        acc[0] = acc[0] + (double)fminf(pl1, pl2);
        acc[1] = acc[1] + (double)(diff * diff);
        acc[2] = acc[2] + (double)H;
        acc[3] = acc[3] + (double)(expm1f(log_r) - log_r);   // (r - 1) - log r without r's rounding against 1
        acc[4] = acc[4] + (fabsf(r - 1.f) > a.clip ? 1.0 : 0.0);
    }
    up_block_sum<UP_STATS>(acc, lds);
    if (t == 0) {
#pragma unroll
        for (int j = 0; j < UP_STATS; j++) a.stat_part[UP_STATS * blockIdx.x + j] = acc[j];
    }
}

// one workgroup: the statistics from the per-workgroup partials
__global__ __launch_bounds__(UP_THREADS) void mgx_ppo_stats_kernel(PpoLossArgs a) {
    __shared__ double lds[UP_STATS * UP_THREADS];
    const int t = threadIdx.x;
    double acc[UP_STATS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (t < a.groups) {
#pragma unroll
        for (int j = 0; j < UP_STATS; j++) acc[j] = a.stat_part[UP_STATS * t + j];
    }
    up_block_sum<UP_STATS>(acc, lds);
    if (t == 0) {
        const double n = (double)a.B;
        const double pl = -acc[0] / n, vl = acc[1] / n, el = -acc[2] / n;
        a.stats[0] = (float)pl;
        a.stats[1] = (float)vl;
        a.stats[2] = (float)el;
        a.stats[3] = (float)(acc[3] / n);
        a.stats[4] = (float)(acc[4] / n);
        a.stats[5] = (float)(pl + (double)a.ent_coef * el + (double)a.vf_coef * vl);
    }
}

struct AdamArgs {
    float *param, *grad, *exp_avg, *exp_avg_sq, *norm_out;
    double *part;                  // [groups]: sum (grad * grad_scale)^2
    int64_t n;
    int groups;
    float grad_scale, max_norm, w1, beta2, w2, step_size, bc2_sqrt, eps;
    const mgx_adam_sched *sched;   // SCHED: [sched_len] (step_size, bc2_sqrt) per step; the two by-value ones unused
    int32_t *cursor;               // SCHED: {next entry, overrun count}
    int sched_len;
};

// SCHED (mgx_adam_step_sched): the two per-step scalars come from a device table, so a captured graph bakes in
// nothing that changes from step to step.  Thread 0 of workgroup 0 of the norm launch is the cursor's only writer;
// the step launch of the same call reads entry cursor[0] - 1 (stream order: the norm launch has finished, and the
// next call's norm launch has not begun).  Arithmetic, summation order and grid are those of SCHED = false.

template <bool SCHED>
__global__ __launch_bounds__(UP_THREADS) void mgx_adam_norm_kernel(AdamArgs a) {
    __shared__ double lds[UP_THREADS];
    if (SCHED && blockIdx.x == 0 && threadIdx.x == 0) a.cursor[0] = a.cursor[0] + 1;
    double v[1] = {0.0};
    for (int64_t i = (int64_t)blockIdx.x * UP_THREADS + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * UP_THREADS) {
        const double x = (double)(a.grad[i] * a.grad_scale);
        v[0] = v[0] + x * x;
    }
    up_block_sum<1>(v, lds);
    if (threadIdx.x == 0) a.part[blockIdx.x] = v[0];
}

template <bool SCHED>
__global__ __launch_bounds__(UP_THREADS) void mgx_adam_step_kernel(AdamArgs a) {
    __shared__ double lds[UP_THREADS];
    const int t = threadIdx.x;
    float step_size = a.step_size, bc2_sqrt = a.bc2_sqrt;
    if (SCHED) {
        const int e = a.cursor[0] - 1;
        if (e < 0 || e >= a.sched_len) {                      // past the table: nothing is updated, the overrun counted
            if (blockIdx.x == 0 && t == 0) a.cursor[1] = a.cursor[1] + 1;
            return;                                           // uniform over the grid
        }
        step_size = a.sched[e].step_size;
        bc2_sqrt = a.sched[e].bc2_sqrt;
    }
    double v[1] = {t < a.groups ? a.part[t] : 0.0};
    up_block_sum<1>(v, lds);
    const float total = (float)sqrt(v[0]);
    if (blockIdx.x == 0 && t == 0 && a.norm_out) a.norm_out[0] = total;
    float coef = 1.f;
    if (a.max_norm > 0.f) {        // clip_grad_norm_: a NaN norm stays a NaN coefficient (no fminf)
        const float c = a.max_norm / (total + 1e-6f);
        coef = c > 1.f ? 1.f : c;
    }
    for (int64_t i = (int64_t)blockIdx.x * UP_THREADS + t; i < a.n; i += (int64_t)gridDim.x * UP_THREADS) {
        const float g = (a.grad[i] * a.grad_scale) * coef;
        a.grad[i] = g;
        float m = a.exp_avg[i], s = a.exp_avg_sq[i];
        m = m + a.w1 * (g - m);                               // lerp_(grad, 1 - beta1)
        s = s * a.beta2 + a.w2 * (g * g);                     // mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        a.exp_avg[i] = m;
        a.exp_avg_sq[i] = s;
        const float denom = sqrtf(s) / bc2_sqrt + a.eps;
        a.param[i] = a.param[i] - step_size * (m / denom);  // addcdiv_(exp_avg, denom, value=-step_size)
    }
}
