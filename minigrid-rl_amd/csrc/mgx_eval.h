// mgx_eval_record (include/mgx.h, added within ABI 9): SB3 evaluate_policy's per-step episode
// accounting for every env of one vector step, in one launch, so that a captured graph can hold an evaluation.
//
// Lane = env, one wave per workgroup: the recorded envs of a workgroup are one ballot's popcount, and the
// workgroup's first lane takes them off remaining_dev with one integer atomic -- none when nothing was recorded.
// Every other store is an env's own slot: no LDS, no float atomics, no workgroup waits for another.  The step
// counter base_dev is only read, so the launches of a captured block share it without an order between them.
#pragma once

#define EVAL_THREADS 64            // one wave: the ballot covers the workgroup

struct EvalRecordArgs {
    const uint8_t *done;
    const double *reward64;        // or null: ep_return
    const float *ep_return;
    const int32_t *ep_len;
    const uint8_t *mission_id;
    const int64_t *base;
    int32_t *counts;
    double *rewards;
    int32_t *lengths;
    int64_t *when;
    uint8_t *missions;
    int32_t *remaining;
    int64_t n, n_eval, cap, step_offset;
};

__global__ __launch_bounds__(EVAL_THREADS) void mgx_eval_record_kernel(EvalRecordArgs a) {
    const int64_t e = (int64_t)blockIdx.x * EVAL_THREADS + threadIdx.x;
    bool rec = false;
    if (e < a.n) {
        const int64_t target = (a.n_eval + e) / a.n;        // SB3's episode_count_targets
        const int64_t c = a.counts[e];
        rec = a.done[e] != 0 && c >= 0 && c < target && c < a.cap;
        if (rec) {
            const int64_t slot = e * a.cap + c;
            a.rewards[slot] = a.reward64 ? a.reward64[e] : (double)a.ep_return[e];
            a.lengths[slot] = a.ep_len[e];
            a.when[slot] = a.base[0] + a.step_offset;
            a.missions[slot] = a.mission_id[e];
            a.counts[e] = (int32_t)(c + 1);
        }
    }
    const int recorded = __popcll(__ballot(rec));
    if (threadIdx.x == 0 && recorded > 0) atomicSub(a.remaining, recorded);
}
