/*
 * mgx.h -- C ABI of the MI355X-native vectorised MiniGrid engine (libmgx.so).
 *
 * Drop-in boundary.  The reference reaches this path through Python objects,
 * not an FFI; each entry point below replaces one of them:
 *
 *   mgx_create   <- make_vec_env(make_env, n_envs, seed, SubprocVecEnv)  src/ppo.py:118-122
 *                   + PlaygroundEnv.__init__                              src/custom_env.py:74-116
 *                   + VecTransposeImage / VecFrameStack(n_stack,'first')  src/ppo.py:124-126
 *   mgx_reset    <- VecEnv.reset() -> env_i.reset(seed=seed+i)
 *                   -> PlaygroundEnv._gen_grid                            src/custom_env.py:122-267
 *                   -> TokenizeVocabWrapper / Discrete2BoxWrapper         src/environment.py:69-149
 *   mgx_step     <- VecEnv.step(actions): PlaygroundEnv.step              src/custom_env.py:269-330
 *                   + SubprocVecEnv auto-reset, Monitor episode stats,
 *                   terminal_observation, TimeLimit.truncated (SB3, via ppo.py:159)
 *   mgx_gae      <- DictRolloutBuffer.compute_returns_and_advantage (SB3, via ppo.py:159)
 *   mgx_destroy  <- VecEnv.close()                                        src/ppo.py:169
 *
 * Conventions: plain C, no exceptions cross the ABI; every call returns an
 * mgx_status (0 = OK) and mgx_last_error() describes the last failure of the
 * calling thread.  All buffers named *_dev are caller-owned DEVICE pointers
 * (e.g. torch.Tensor.data_ptr()); `stream` is a hipStream_t (NULL = default).
 * mgx_reset / mgx_step / mgx_gae only enqueue work on `stream` (no host sync,
 * no allocation) and are therefore hipGraph-capturable.  A handle is not
 * thread-safe; use one handle per device (per rank).
 */
#ifndef MGX_H_
#define MGX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGX_ABI_VERSION 9

/* Live-lock cap (engine policy; the reference hangs): a
 * reset attempt may consume at most this many MT19937 words; the attempt that
 * would take one more is abandoned and the reset re-runs unseeded with both
 * RNG streams continuing. */
#define MGX_LIVELOCK_WORDS 4096

typedef enum {
    MGX_OK = 0,
    MGX_ERR_INVALID = 1,      /* bad argument / unsupported configuration */
    MGX_ERR_HIP = 2,          /* a HIP runtime call failed */
    MGX_ERR_DEVICE = 3,       /* the device reported an error (see mgx_poll_error) */
    MGX_ERR_OOM = 4
} mgx_status;

/* PlaygroundEnv problems (custom_env.py:134-152) */
typedef enum {
    MGX_PROBLEM_MULTI = 0, MGX_PROBLEM_FULL = 1, MGX_PROBLEM_GTO = 2, MGX_PROBLEM_GTG = 3,
    MGX_PROBLEM_OPN = 4, MGX_PROBLEM_PKP = 5, MGX_PROBLEM_DRP = 6, MGX_PROBLEM_MOV = 7
} mgx_problem;

/* which done envs get a stacked terminal observation written */
typedef enum { MGX_TERMINAL_NONE = 0, MGX_TERMINAL_TRUNCATED = 1, MGX_TERMINAL_ALL = 2 } mgx_terminal_mode;

/* Device error bits reported by mgx_poll_error */
#define MGX_DEVERR_MT_TABLE   1u   /* an env's MT19937 cursor left the window of the stream the device holds
                                      (live cursors spread over more than mt_table_words) */
#define MGX_DEVERR_BAD_ACTION 2u   /* action outside 0..6 (minigrid raises ValueError) */
#define MGX_DEVERR_PCG_LOOP   4u   /* a PCG64 rejection loop exceeded its safety bound */
#define MGX_DEVERR_OBJECTS    8u   /* generator ran out of objects (AssertionError / IndexError in the reference) */
#define MGX_DEVERR_RING_EMPTY 16u  /* an env found its episode ring empty (engine invariant broken) */

typedef struct mgx_config {
    int32_t problem;           /* mgx_problem; `env.problem` */
    int32_t mission;           /* `env.mission` (problem multi): 0 'go to', 1 'toggle', 2 'pick up',
                                  5 'go to goal'; -1 = None */
    int32_t size;              /* `env.size` (5..16); max_steps = size^2 (custom_env.py:114).  Problem multi
                                  needs 6..16: at 5 the reference's goal placement in a 4-room layout never
                                  ends (every free cell is next to a door), so mgx_create refuses it */
    int32_t num_objects;       /* `env.num_objects` */
    int32_t see_through_walls; /* `env.see_through_walls`; 0 = minigrid Grid.process_vis occlusion */
    int32_t all_doors_open;    /* `env.all_doors_open` */
    int32_t obstacles;         /* `env.obstacles`: floor((size-2)^2 * percent_obstacles) lava (multi) or
                                  lava/wall (single room) cells (custom_env.py:154-172) */
    int32_t n_stack;           /* `algorithm.n_frames_stack` (1..8) */
    int64_t n_envs;            /* envs owned by this handle */
    int64_t base_seed;         /* `seed`; env i: PCG64(SeedSequence(base_seed + env_index_offset + i)), MT19937(base_seed) */
    int64_t env_index_offset;  /* global index of env 0 (rank * n_envs when sharding) */
    int32_t livelock_words;    /* 0 -> MGX_LIVELOCK_WORDS */
    int32_t terminal_mode;     /* mgx_terminal_mode */
    int32_t mission_int64;     /* 1: mission tokens int64 (TokenizeVocabWrapper dtype), 0: uint8 */
    int32_t refill_cap;        /* > 0 (0 -> max(2, round(0.19 * refill_every))): a refill epoch's production
                                  per env follows the consumption of its 64-env wave since the previous
                                  refill (the mean, rounded up), beyond what keeps the ring from running
                                  dry; < 0 -> fill the ring every epoch.  mgx_reset fills every ring */
    int64_t mt_table_words;    /* 0 -> default (2^26): MT19937 output words the device keeps (rounded up to a
                                  power of two of 10-word groups, >= 5,120).  The stream is extended on the
                                  device as cursors advance -- no lifetime limit; only the spread between
                                  the oldest live cursor and the newest must stay below it */
    int32_t ring_depth;        /* pre-generated episodes per env (0 -> 512 since ABI 7, 256 before; rounded up to a power of two
                                  <= 4096, ring positions are mod 2^16; -1 = no ring: every auto-reset
                                  generated inline) */
    int32_t refill_every;      /* steps per refill epoch K (0 -> min(ring_depth/4, 64); clamped to <= ring_depth/2:
                                  each epoch keeps >= K queued, and a step pops <= 1 episode) */
    double percent_obstacles;  /* `env.percent_obstacles` (single.yaml:28: 0.05); used when obstacles */
    int32_t manual;            /* PlaygroundEnv(manual=True) (make_env(manual=True), environment.py:10-20):
                                  a 'done' before the mission is complete is a no-op -- no termination,
                                  no reset (custom_env.py:319-328 `elif not self.manual`) */
    int32_t reserved0;         /* 0 */
} mgx_config;

/* Stacked observation in the layout SB3's VecFrameStack(VecTransposeImage(.))
 * hands the policy: image u8 [N][3*n_stack][7][7] ([c][vx][vy] per frame,
 * newest frame last), direction u8 [N][4*n_stack] (one-hot per frame),
 * mission [N][32*n_stack] (int64 or uint8 tokens per frame). */
typedef struct mgx_obs {
    void *image_dev;
    void *direction_dev;
    void *mission_dev;
} mgx_obs;

typedef struct mgx_step_out {
    mgx_obs obs;               /* updated in place (the stacks roll) */
    mgx_obs terminal;          /* stacked terminal obs, valid where written (terminal_mode) */
    float *reward_dev;         /* f32 [N] */
    double *reward64_dev;      /* f64 [N] (optional): the env's Python-float reward */
    uint8_t *terminated_dev;   /* u8 [N] */
    uint8_t *truncated_dev;    /* u8 [N] (gymnasium truncated; TimeLimit.truncated = trunc & !term) */
    uint8_t *done_dev;         /* u8 [N] = term | trunc (SB3 `dones`) */
    float *ep_return_dev;      /* f32 [N] Monitor 'r', valid where done (optional) */
    int32_t *ep_len_dev;       /* i32 [N] Monitor 'l', valid where done (optional) */
    int32_t *livelock_dev;     /* i32 [N] abandoned reset attempts where done (optional) */
} mgx_step_out;

typedef struct mgx_handle mgx_handle;

const char *mgx_last_error(void);
int mgx_abi_version(void);

mgx_status mgx_create(const mgx_config *cfg, int device, mgx_handle **out);
mgx_status mgx_destroy(mgx_handle *h);

/* VecEnv.reset() of every env; writes the stacked first observation (zeros +
 * newest frame).  The first call after mgx_create is the seeded reset of
 * make_vec_env (PCG64 <- base_seed + env_index_offset + i, MT cursor 0).  Later
 * calls follow SB3: seeded (PCG64 only) if mgx_set_seed was called since the
 * last reset, else unseeded; both streams continue from each env's current
 * episode, and mission_done / the stored reward persist.
 * It also pre-generates ring_depth episodes per env (on `stream`; ~26 ms at
 * 65,536 envs, S = 8, D = 512).  `livelock_dev` (optional i32 [N]). */
mgx_status mgx_reset(mgx_handle *h, const mgx_obs *obs, int32_t *livelock_dev, void *stream);

/* VecEnv.seed(seed) (SB3): the NEXT mgx_reset seeds env i's PCG64 with
 * seed + env_index_offset + i.  The MT19937 stream keeps cfg.base_seed: the
 * reference seeds CPython `random` once, in PlaygroundEnv.__init__
 * (custom_env.py:82), from the config, not from reset(seed). */
mgx_status mgx_set_seed(mgx_handle *h, int64_t seed);

/* One vectorised step.  actions_dev: [N] int32 (action_bytes = 4) or int64 (8).
 * Episode pre-generation runs CONCURRENTLY with the steps on a handle-owned
 * side stream, in epochs of K = refill_every calls: the first call of an epoch
 * joins the previous epoch's refill (and the slide that publishes its episodes) and
 * forks the next refill off `stream`.  Whatever the caller enqueues between two
 * epochs (GAE, the policy) overlaps the refill's tail.  The launch sequence
 * depends only on the call count; end a stream capture (hipGraph) with mgx_join
 * to make it self-contained. */
mgx_status mgx_step(mgx_handle *h, const void *actions_dev, int action_bytes,
                    const mgx_step_out *out, void *stream);

/* ---- Compact rollout layout ------------------------------
 * One observation = one 148-B ROW (byte 0: agent direction 0..3; bytes 1..147: the
 * [c][vx][vy] frame, VecTransposeImage order) + one mission-id byte (mgx_mission_text;
 * tokens = TokenizeVocabWrapper of that text).  A rollout buffer is [T][N] rows; the
 * SB3 stacked observation of any (t, env) is rebuilt by mgx_gather from rows t-n_stack+1..t
 * and the episode-start flags (VecFrameStack zero-fills before an episode's first obs).
 * 150 B per env-step instead of 588 + 16 + 32*n_stack*(1|8) B; no stack roll per step. */
typedef struct mgx_compact_out {
    uint8_t *row_dev;             /* u8 [N][148]: the observation after this step (the new
                                     episode's first one where done) */
    uint8_t *mission_id_dev;      /* u8 [N]: its mission id */
    uint8_t *terminal_row_dev;    /* u8 [N][148]: the final observation of each episode that ended
                                     (written where terminal_mode selects; its mission id is the
                                     previous row's) */
    float *reward_dev;            /* as mgx_step_out */
    double *reward64_dev;
    uint8_t *terminated_dev;
    uint8_t *truncated_dev;
    uint8_t *done_dev;            /* u8 [N]: done of this step = start flag of the row written */
    float *ep_return_dev;
    int32_t *ep_len_dev;
    int32_t *livelock_dev;
} mgx_compact_out;

/* mgx_step with compact outputs (same transition, RNG, auto-reset and refill epochs as
 * mgx_step; the two may not be mixed on one handle between resets).  Needs the ring. */
mgx_status mgx_step_compact(mgx_handle *h, const void *actions_dev, int action_bytes, const mgx_compact_out *out,
                            void *stream);

/* K consecutive mgx_step_compact calls fused into ONE launch, for a rollout whose actions are
 * known up front (random-action or scripted rollouts: BASELINE config 2's workload; a policy in the
 * loop needs mgx_step_compact per step).  actions_dev: int32 [K][N].  The outputs of step t go to
 * row t of the [K][N] arrays below; terminal rows, ep_return, ep_len and livelock are left as
 * after the last step.  Transitions, RNG streams, auto-resets, refill epochs and counters are
 * those of the K calls, bit for bit.  The K steps must lie within one refill epoch:
 * (mgx_step calls so far % refill_every) + K <= refill_every.  Needs the ring. */
typedef struct mgx_rollout_out {
    uint8_t *rows_dev;            /* u8 [K][N][148]: the observation after step t at row t */
    uint8_t *mission_ids_dev;     /* u8 [K][N] */
    uint8_t *terminal_row_dev;    /* u8 [N][148] (as mgx_compact_out) */
    float *rewards_dev;           /* f32 [K][N] */
    double *rewards64_dev;        /* f64 [K][N] (optional) */
    uint8_t *terminated_dev;      /* u8 [K][N] */
    uint8_t *truncated_dev;       /* u8 [K][N] */
    uint8_t *dones_dev;           /* u8 [K][N] */
    float *ep_return_dev;         /* f32 [N] (optional) */
    int32_t *ep_len_dev;          /* i32 [N] (optional) */
    int32_t *livelock_dev;        /* i32 [N] (optional) */
} mgx_rollout_out;
mgx_status mgx_rollout_compact(mgx_handle *h, const int32_t *actions_dev, int K, const mgx_rollout_out *out,
                               void *stream);

/* The current observation of every env as compact rows (e.g. row 0 after mgx_reset). */
mgx_status mgx_observe_compact(mgx_handle *h, uint8_t *row_dev, uint8_t *mission_id_dev, void *stream);

/* Stacked observations (VecFrameStack(n_stack) of the handle) of n_samples (t, env) pairs from
 * a compact buffer: rows_dev u8 [R][n_envs][148], mission_ids_dev / starts_dev u8 [R][n_envs]
 * (start = the row is an episode's first observation); index_dev i64 [n_samples] = t*n_envs +
 * env of the newest row, which must have n_stack-1 rows before it.  terminal_rows_dev (u8
 * [n_envs][148], optional): the newest frame is env's terminal row and the older ones start at
 * row index (SB3's stacked terminal_observation).  Outputs (device): image [n][3*n_stack][7][7]
 * u8 or f32 (= u8 / 255, SB3 preprocess_obs), direction [n][4*n_stack] u8 or f32 one-hot,
 * mission [n][32*n_stack] u8 tokens. */
mgx_status mgx_gather(const mgx_handle *h, const uint8_t *rows_dev, const uint8_t *mission_ids_dev,
                      const uint8_t *starts_dev, int64_t n_envs, const int64_t *index_dev, int64_t n_samples,
                      const uint8_t *terminal_rows_dev, void *image_dev, int image_f32, void *direction_dev,
                      int direction_f32, uint8_t *mission_dev, void *stream);

/* mgx_gather over a RING of ring_rows rows (ABI 6): walking back from a sample's newest row wraps
 * from row 0 to row ring_rows - 1, so a rollout that starts where the previous one ended reads its
 * n_stack - 1 history rows in place -- no per-rollout copy of them (mgx/compact.py ring mode).
 * ring_rows = 0 is mgx_gather; else ring_rows >= n_stack. */
mgx_status mgx_gather_ring(const mgx_handle *h, const uint8_t *rows_dev, const uint8_t *mission_ids_dev,
                           const uint8_t *starts_dev, int64_t n_envs, int64_t ring_rows, const int64_t *index_dev,
                           int64_t n_samples, const uint8_t *terminal_rows_dev, void *image_dev, int image_f32,
                           void *direction_dev, int direction_f32, uint8_t *mission_dev, void *stream);

/* ---- Fused actor-critic inference over compact rows (ABI 8) ------------------------------------
 * The forward pass of the reference's policy (CustomPPOPolicy with the default `arch`: policy.py
 * DEFAULT_ARCH, net_arch pi = vf = [64, 64] Tanh, 7 actions) for n_samples (t, env) pairs of a compact
 * buffer, in ONE launch: what ActorCriticPolicy.forward / predict_values compute on the observation
 * mgx_gather_ring would build for the same sample -- same slot validity, walk-back, ring wrap and
 * terminal-row case; empty slots are zeros, image = u8 * (1/255), direction = one-hot of row byte 0 --
 * without materialising that observation.  fp32 with fp32 accumulation.
 *
 * Weight blob (fp32, mgx_policy_blob_words(n_stack) words; K = n_stack): every tensor in its torch
 * row-major layout, concatenated in this order:
 *    1. direction Linear        W[16][4K], b[16]
 *    2. image conv1             W[16][3K][2][2], b[16]
 *    3. image conv2             W[32][16][2][2], b[32]
 *    4. image conv3             W[64][32][2][2], b[64]
 *    5. policy_net L0           W[64][208], b[64]     (features: direction 16 | image 64 | mission 128)
 *    6. policy_net L1           W[64][64], b[64]
 *    7. value_net_body L0, L1   as 5 and 6
 *    8. action_net              W[7][64], b[7]
 *    9. value_net               W[1][64], b[1]
 * (46,984 words at K = 4).  The mission GRU does not run in this kernel: the valid slots of a stack are
 * contiguous from the newest and share one mission id, so the mission features take only (mission id,
 * v = number of valid slots) values, and the caller tabulates them with the policy's own Embedding + GRU
 * (in torch, or with mgx_mission_forward below):
 * mission_feat[mid][v-1][:] = features of K - v zero frames followed by v copies of mid's 32 tokens. */
int64_t mgx_policy_blob_words(int n_stack);   /* host only; -1 unless 1 <= n_stack <= 8 */

typedef struct mgx_policy {
    const float *blob_dev;          /* f32 [mgx_policy_blob_words(n_stack)]; 4-byte aligned */
    const float *mission_feat_dev;  /* f32 [256][n_stack][128]; 16-byte aligned (read as float4) */
    int32_t mode;                   /* 0: values (and logits) only, 1: deterministic action, 2: sampled action */
    int32_t reserved0;              /* 0 */
    uint64_t seed;                  /* mode 2 */
    uint64_t *counter_dev;          /* mode 2: u64 [2], the contract of mgx_random_actions' counter_dev */
} mgx_policy;

typedef struct mgx_act_out {        /* each optional; actions_dev and log_probs_dev required when mode != 0 */
    int64_t *actions_dev;           /* i64 [n_samples] */
    float *values_dev;              /* f32 [n_samples]: value_net output */
    float *log_probs_dev;           /* f32 [n_samples]: l[action] - max l - log(total) */
    float *logits_dev;              /* f32 [n_samples][7]: action_net output l */
} mgx_act_out;

/* rows_dev .. terminal_rows_dev: exactly mgx_gather_ring's sample addressing.  Mode 1: action = the first
 * index of the maximum logit.  Mode 2: u = (h >> 40) * 2^-24 with h = mgx_random_actions' hash of (seed,
 * counter_dev[0], sample index b); p_a = exp(l_a - max l) accumulated in fp32 in index order (cum_a, total =
 * cum_6); action = the smallest a with cum_a > u * total, 6 if there is none; the launch then advances
 * counter_dev[0] by one on the device (a replayed graph draws afresh; launches sharing a counter must not
 * overlap).  Only enqueues on `stream` (no allocation, no host sync).  MGX_ERR_INVALID before any HIP call
 * for: null pol / out / blob / feature table, n_samples <= 0, mode outside 0..2, a null counter_dev in
 * mode 2, missing actions_dev / log_probs_dev when mode != 0, 0 < ring_rows < n_stack. */
mgx_status mgx_policy_act(const mgx_handle *h, const uint8_t *rows_dev, const uint8_t *mission_ids_dev,
                          const uint8_t *starts_dev, int64_t n_envs, int64_t ring_rows, const int64_t *index_dev,
                          int64_t n_samples, const uint8_t *terminal_rows_dev, const mgx_policy *pol,
                          const mgx_act_out *out, void *stream);

/* ---- Truncation bootstrap on the device (added within ABI 9) ---------------------------------------
 * SB3's `rewards[idx] += gamma * V(terminal_observation)` for every env with truncated & !terminated at one
 * step of a compact buffer, the work list built on the device: what
 *    boot = (truncated & ~terminated).nonzero();  r[boot] = r[boot] + gamma * V
 * computes with V = mgx_policy_act (mode 0, terminal_rows_dev) on the samples row * n_envs + boot -- bit for bit
 * (the multiply and the add are two fp32 operations), with no host decision, so a captured graph can hold it.
 * Two launches: (1) one workgroup compacts the selected envs in ascending order into list_dev (flat indices
 * row * n_envs + e, nonzero()'s order) and writes count_dev; every entry below the count and the count are
 * written, so neither needs zeroing, and both stay readable afterwards; (2) a grid of ceil(n_envs / 64)
 * workgroups, one per possible tile of 64 list entries, reads the count on the device: mgx_policy_act's
 * forward pass and value head on each listed env's terminal stack, then the reward update; a workgroup past
 * the count exits after that one load.  Deterministic (no float atomics); with nothing selected launch 2
 * stores nothing and rewards_dev is untouched. */
typedef struct mgx_bootstrap {
    const uint8_t *truncated_dev;   /* u8 [n_envs]: this step's flags */
    const uint8_t *terminated_dev;  /* u8 [n_envs] */
    float *rewards_dev;             /* f32 [n_envs]: r[e] = r[e] + gamma * V(e) where selected, else untouched */
    float gamma;
    int32_t reserved0;              /* 0 */
    int64_t *list_dev;              /* i64 [n_envs], caller-owned scratch: the selected samples' flat indices */
    int32_t *count_dev;             /* i32 [1], caller-owned: the number selected */
    float *values_dev;              /* optional f32 [n_envs]: V of list entry j at [j] */
} mgx_bootstrap;

/* rows_dev .. ring_rows, terminal_rows_dev: mgx_policy_act's sample addressing; row = the buffer row of the
 * observation the step left (the terminal stack's older frames start there).  pol: blob_dev and
 * mission_feat_dev are read (mode, seed and counter_dev are not).  Only enqueues on `stream` (no allocation,
 * no host sync; capturable).  MGX_ERR_INVALID before any HIP call for: a null pointer (values_dev aside),
 * n_envs <= 0, row < 0 or, in a ring, row >= ring_rows, 0 < ring_rows < n_stack. */
mgx_status mgx_policy_bootstrap(const mgx_handle *h, const uint8_t *rows_dev, const uint8_t *mission_ids_dev,
                                const uint8_t *starts_dev, int64_t n_envs, int64_t ring_rows, int64_t row,
                                const uint8_t *terminal_rows_dev, const mgx_policy *pol, const mgx_bootstrap *b,
                                void *stream);

/* ---- Mission-routed mixture of experts (added within ABI 9) ------------------------------------------
 * mgx_policy_act over up to MGX_MOE_MAX_EXPERTS frozen policies of one n_stack: sample b (position b of
 * index_dev) is computed with the weight blob and the mission-feature table of expert
 *    e(b) = route_dev[mission_ids_dev[index_dev[b]]]
 * -- the mission id of the sample's newest frame, terminal case included -- and is, bit for bit, what
 * mgx_policy_act returns for it with that expert's mgx_policy, the same seed and the same counter value.  The
 * reference's mixture (src/policies.py MoeExtractor: the arg-max of a gate over the newest frame's mission
 * tokens picks one of the per-task policies) with the gate tabulated per mission id.  Two launches:
 *
 * (1) the route: ONE workgroup partitions the positions p in [0, n_samples) by expert, stably.  Expert e's
 *     segment of the lists starts at start_e = 64 * sum over e' < e of ceil(count_e' / 64) and holds count_e
 *     entries with ascending p.  A sample whose route byte is >= n_experts is unroutable: it is counted, left out
 *     of every list, and none of its outputs is written.  In mode 2 this launch also snapshots counter_dev[0]
 *     into the record and advances it by one (launch 2's grid holds idle workgroups, so mgx_policy_act's
 *     arrival tally is not used; every draw uses the snapshot, the value before the advance).
 * (2) the policy pass: a grid of (n_samples + 63 * n_experts) / 64 workgroups, the bound on the live tiles
 *     sum_e ceil(count_e / 64); a workgroup past the live tile count exits after one load; a live one finds its
 *     expert among the <= 8 segment records and runs mgx_policy_act's forward pass and heads on its tile of 64
 *     list entries with that expert's weights.  Outputs go to position p, and the sampling hash is keyed by p.
 *
 * scratch_dev: caller-owned, 8-byte aligned, mgx_policy_moe_scratch_words(n_samples, n_experts) i32 words, not
 * zeroed by anyone: every word launch 2 reads is written by launch 1, and all of it stays readable afterwards.
 * With cap = n_samples + 63 * n_experts (the most entries a list can hold):
 *    words [0, 32)               the record: [2e] = start_e, [2e + 1] = count_e for e < 8 (experts >= n_experts:
 *                                start = the end of the last segment, count 0), [16] = live tiles, [17] = unroutable
 *                                samples, [18..19] = the u64 counter snapshot (0 unless mode 2), [20..31] = 0
 *    words [32, 32 + 2 cap)      i64 list[cap]: list[start_e + j] = index_dev[p] of the j-th position p of expert e
 *    words [32 + 2 cap, 32 + 3 cap)  i32 pos[cap]: that p
 * List entries outside [start_e, start_e + count_e) (the padding up to a multiple of 64) are never written. */
#define MGX_MOE_MAX_EXPERTS 8
#define MGX_MOE_RECORD_WORDS 32

/* host only: 32 + 3 * (n_samples + 63 * n_experts); -1 unless n_samples > 0, 1 <= n_experts <= 8 and
 * n_samples + 63 * n_experts < 2^31 */
int64_t mgx_policy_moe_scratch_words(int64_t n_samples, int n_experts);

typedef struct mgx_policy_moe {
    int32_t n_experts;              /* 1 .. MGX_MOE_MAX_EXPERTS */
    int32_t mode;                   /* as mgx_policy */
    const float *blob_dev[MGX_MOE_MAX_EXPERTS];          /* the first n_experts: as mgx_policy.blob_dev */
    const float *mission_feat_dev[MGX_MOE_MAX_EXPERTS];  /* the first n_experts: as mgx_policy.mission_feat_dev */
    const uint8_t *route_dev;       /* u8 [256]: mission id -> expert */
    uint64_t seed;                  /* mode 2 */
    uint64_t *counter_dev;          /* mode 2: as mgx_policy; the PAIR of launches advances counter_dev[0] by one */
    int32_t *scratch_dev;           /* i32 [scratch_words], 8-byte aligned (layout above) */
    int64_t scratch_words;          /* >= mgx_policy_moe_scratch_words(n_samples, n_experts) */
} mgx_policy_moe;

/* rows_dev .. terminal_rows_dev and out: exactly mgx_policy_act's.  Only enqueues on `stream` (no allocation, no
 * host sync; capturable).  MGX_ERR_INVALID before any HIP call for: null pol / out / route_dev / scratch_dev or
 * one of the first n_experts blob or table pointers, n_experts outside 1..8, a misaligned scratch_dev,
 * scratch_words below mgx_policy_moe_scratch_words (or n_samples beyond its range), and every case
 * mgx_policy_act rejects. */
mgx_status mgx_policy_act_moe(const mgx_handle *h, const uint8_t *rows_dev, const uint8_t *mission_ids_dev,
                              const uint8_t *starts_dev, int64_t n_envs, int64_t ring_rows,
                              const int64_t *index_dev, int64_t n_samples, const uint8_t *terminal_rows_dev,
                              const mgx_policy_moe *pol, const mgx_act_out *out, void *stream);

/* ---- Fused policy gradient over compact rows (ABI 9) ---------------------------------------------
 * The backward pass of the network above for the same kind of samples, for the PPO update: given the
 * cotangents of action_net's and value_net's outputs it recomputes the forward pass from the compact rows
 * and writes
 *    grad_blob         = sum over samples of d(g_logits . logits + g_values * value) / d blob
 *    grad_mission_feat = the same derivative with respect to the mission-feature table
 * (the forward half of a training step is mgx_policy_act in mode 0 with logits_dev set).  The Embedding
 * and the GRU do not run in this call: the caller back-propagates grad_mission_feat through its own
 * differentiable table (in torch, or with mgx_mission_backward below).  fp32 with fp32 accumulation; MaxPool's gradient goes to the first maximum in
 * window order, ReLU's where the pre-activation is positive.
 *
 * Summation order.  At most `groups` workgroups run (max_groups, or 256 -- one per CU of an MI355X -- when
 * it is 0; never more than the ceil(n_samples / 64) tiles).  Workgroup g walks tiles g, g + groups, ...
 * and adds each tile's weight gradient into its own slab of scratch_dev; a second kernel adds the slabs
 * in group order.  grad_blob is therefore bitwise reproducible for a given (n_samples, groups).
 * grad_mission_feat is summed per tile over the samples that share a (mission id, v) row and then added
 * with fp32 atomics: its summation order across tiles is run-dependent (as torch's index_select backward
 * is), and rows no sample names stay exactly zero.
 * scratch_dev needs mgx_policy_grad_scratch_words(n_stack, n_samples, max_groups) words = groups x
 * mgx_policy_blob_words(n_stack); it is caller-owned and need not be zeroed. */
int64_t mgx_policy_grad_scratch_words(int n_stack, int64_t n_samples, int max_groups);
                                    /* host only; -1 unless 1 <= n_stack <= 8, n_samples > 0, max_groups >= 0 */

typedef struct mgx_policy_grad {
    const float *blob_dev;          /* as mgx_policy */
    const float *mission_feat_dev;  /* as mgx_policy; only rows some sample names are read (and row 0) */
    const float *g_logits_dev;      /* f32 [n_samples][7]: dL/d(action_net output) */
    const float *g_values_dev;      /* f32 [n_samples]:    dL/d(value_net output) */
    float *grad_blob_dev;           /* f32 [mgx_policy_blob_words(n_stack)], blob order; OVERWRITTEN */
    float *grad_mission_feat_dev;   /* f32 [256][n_stack][128]; OVERWRITTEN (zero where no sample has that (mid, v)) */
    float *scratch_dev;             /* f32 [scratch_words], caller-owned, need not be zeroed */
    int64_t scratch_words;
    int32_t max_groups;             /* 0: default; else the number of workgroups that share the tiles */
    int32_t reserved0;              /* 0 */
} mgx_policy_grad;

/* rows_dev .. index_dev: exactly mgx_policy_act's sample addressing without the terminal-row case.  Only
 * enqueues on `stream` (the outputs are zeroed on the stream; no allocation, no host sync; capturable).
 * MGX_ERR_INVALID before any HIP call for: any null pointer, n_samples <= 0, scratch_words below
 * mgx_policy_grad_scratch_words(...), max_groups < 0, 0 < ring_rows < n_stack. */
mgx_status mgx_policy_backward(const mgx_handle *h, const uint8_t *rows_dev, const uint8_t *mission_ids_dev,
                               const uint8_t *starts_dev, int64_t n_envs, int64_t ring_rows,
                               const int64_t *index_dev, int64_t n_samples, const mgx_policy_grad *g,
                               void *stream);

/* ---- Mission encoder: Embedding + GRU forward and backward (added within ABI 9) --------------------
 * The reference's mission extractor for n_rows independent token sequences of length seq_len:
 * Embedding(32, 32) -> GRU(32, 128, one layer, bias, batch_first), h0 = 0, output = the last hidden state.
 * Gate order and bias placement are torch's: r = sigmoid(W_ir x + b_ir + W_hr h + b_hr), z likewise,
 * n = tanh(W_in x + b_in + r * (W_hn h + b_hn)), h' = (1 - z) * n + z * h.  fp32 with fp32 accumulation.
 * Token values are masked with & 31.  These calls take no engine handle: they read nothing of an engine.
 *
 * One persistent kernel per direction keeps W_hh in registers over all seq_len steps.  With a workspace
 * the forward records, per (row, t), what the backward needs; the backward walks the steps in reverse,
 * replaces the records by the gate cotangents and then forms the weight gradients from them off the
 * serial chain (an fp32 MFMA product over (row, t) in chunks whose number and length depend on (n_rows,
 * seq_len) only, added in chunk order).  No float atomics: every output is bitwise reproducible for a
 * given (n_rows, seq_len).  Embedding-gradient rows of tokens that never occur are exactly zero.
 * The workspace is caller-owned and need not be zeroed. */
int64_t mgx_mission_workspace_words(int64_t n_rows, int seq_len);
                                    /* host only; -1 unless 1 <= n_rows <= 2048, 1 <= seq_len <= 256 */

typedef struct mgx_mission_params { /* fp32, torch's row-major layouts; w_ih_dev and w_hh_dev 16-byte aligned */
    const float *embedding_dev;     /* [32][32]   Embedding.weight */
    const float *w_ih_dev;          /* [384][32]  GRU.weight_ih_l0 (r | z | n) */
    const float *w_hh_dev;          /* [384][128] GRU.weight_hh_l0 */
    const float *b_ih_dev;          /* [384]      GRU.bias_ih_l0 */
    const float *b_hh_dev;          /* [384]      GRU.bias_hh_l0 */
} mgx_mission_params;

typedef struct mgx_mission_grads {  /* the same shapes; every one OVERWRITTEN */
    float *embedding_dev;
    float *w_ih_dev;
    float *w_hh_dev;
    float *b_ih_dev;
    float *b_hh_dev;
} mgx_mission_grads;

/* features_dev f32 [n_rows][128].  workspace_dev NULL: inference only; else f32 [workspace_words] with
 * workspace_words >= mgx_mission_workspace_words(n_rows, seq_len).  The features are bitwise the same
 * with and without a workspace.  Only enqueues on `stream` (no allocation, no host sync; capturable).
 * MGX_ERR_INVALID before any HIP call for: a null pointer (workspace_dev excepted), sizes out of range,
 * a workspace that is too short. */
mgx_status mgx_mission_forward(const uint8_t *tokens_dev /* u8 [n_rows][seq_len] */, int64_t n_rows, int seq_len,
                               const mgx_mission_params *p, float *features_dev, float *workspace_dev,
                               int64_t workspace_words, void *stream);

/* g_features_dev f32 [n_rows][128]: the cotangent of the forward's features.  workspace_dev: as the forward
 * of the same tokens and parameters left it; clobbered.  Writes the five gradients of g.  Only enqueues
 * on `stream` (four launches; no allocation, no host sync; capturable).  MGX_ERR_INVALID before any HIP
 * call for: any null pointer, sizes out of range, a workspace that is too short. */
mgx_status mgx_mission_backward(const uint8_t *tokens_dev, int64_t n_rows, int seq_len, const mgx_mission_params *p,
                                const float *g_features_dev, float *workspace_dev, int64_t workspace_words,
                                const mgx_mission_grads *g, void *stream);

/* The same two calls reading and writing rows of a table in place (added within ABI 9): row r's feature goes
 * to table_dev[rows_dev[r]][128] instead of features_dev[r], and row r's cotangent is read from
 * g_table_dev[rows_dev[r]][128] -- what forward + index_copy_ and index_select + backward do, bit for bit,
 * without the two torch launches.  table_dev / g_table_dev f32 [table_rows][128]; rows_dev i64 [n_rows] on the
 * device.  Table rows that rows_dev does not name are neither read nor written.  An index outside
 * [0, table_rows) is the caller's error (the host cannot see it).  Everything else as above; additionally
 * MGX_ERR_INVALID for a null rows_dev and table_rows < 1. */
mgx_status mgx_mission_forward_rows(const uint8_t *tokens_dev, int64_t n_rows, int seq_len,
                                    const mgx_mission_params *p, float *table_dev, const int64_t *rows_dev,
                                    int64_t table_rows, float *workspace_dev, int64_t workspace_words, void *stream);
mgx_status mgx_mission_backward_rows(const uint8_t *tokens_dev, int64_t n_rows, int seq_len,
                                     const mgx_mission_params *p, const float *g_table_dev, const int64_t *rows_dev,
                                     int64_t table_rows, float *workspace_dev, int64_t workspace_words,
                                     const mgx_mission_grads *g, void *stream);

/* ---- PPO loss: statistics and cotangents (added within ABI 9) ----------------------------------------
 * Replaces the loss block of SB3's PPO.train (stable_baselines3/ppo/ppo.py; mgx/ppo.py Trainer.train) and its
 * autograd graph down to the network outputs: from the logits and values mgx_policy_act (mode 0) wrote and
 * the rollout's arrays it writes the loss statistics and dL/dlogits, dL/dvalues -- exactly what
 * mgx_policy_backward consumes.  fp32, expf / logf; sums over samples in fp64 (below).  With p = softmax(z),
 * lp = log p[a], H = -sum p log p, r = exp(lp - old_lp), A the (normalised) advantage, c = clip_range:
 *    policy_loss  = -mean min(A r, A clamp(r, 1 - c, 1 + c))      value_loss = mean (ret - vp)^2
 *    entropy_loss = -mean H        approx_kl = mean (r - 1) - log r        clip_fraction = mean [|r - 1| > c]
 *    loss         = policy_loss + ent_coef entropy_loss + vf_coef value_loss
 *    vp           = old_v + clamp(v - old_v, -c_v, c_v), or v when clip_range_vf <= 0
 *    dL/dlp  = -A r / B where 1 - c <= r <= 1 + c or A r < A clamp(r), else 0
 *    dL/dz_j = dL/dlp ([j = a] - p_j) + ent_coef / B p_j (log p_j + H)
 *    dL/dv   = vf_coef 2 (vp - ret) / B where |v - old_v| <= c_v (or no value clipping), else 0
 * The rollout's arrays are read at element sel_dev[i] for sample i (sel_dev NULL: element i); logits, values
 * and the outputs are indexed by i.  Actions outside 0..6 are clamped into that range.
 * adv_mode 0: A = advantage.  1: A = (a - mean) / (std + 1e-8) over the n_samples advantages, std unbiased as
 * Tensor.std(); not applied when n_samples = 1 (as PPO.train).  2: mean and std read from adv_stats_dev.
 * stats_dev f32 [8] = policy_loss, value_loss, entropy_loss, approx_kl, clip_fraction, loss, the advantage mean
 * and std used (0 and 1 where none were).
 *
 * Summation order.  ceil(n_samples / 256) workgroups, at most 256; a thread adds its samples in index order
 * into fp64, a workgroup's threads are added by a fixed tree, the partials go to scratch_dev and the next
 * launch adds them by the same tree.  adv_mode 1 is a pass of its own in front (the advantage sums, shifted
 * by the first sample's).  Two or three launches, no float atomics: every output is bitwise reproducible
 * for a given n_samples.  clip_range .. vf_coef are by-value arguments: a captured graph bakes them in. */
int64_t mgx_ppo_loss_scratch_words(int64_t n_samples);      /* host only; -1 unless n_samples > 0 */

typedef struct mgx_ppo_loss_args {
    const float *logits_dev;        /* f32 [n_samples][7], as mgx_act_out.logits_dev */
    const float *values_dev;        /* f32 [n_samples] */
    const int64_t *sel_dev;         /* i64 [n_samples] or NULL: the element of the five arrays below sample i reads */
    const int64_t *actions_dev;     /* i64 */
    const float *old_values_dev;    /* f32, as the four below */
    const float *old_log_probs_dev;
    const float *advantages_dev;
    const float *returns_dev;
    const float *adv_stats_dev;     /* f32 [2] mean, std: adv_mode 2 only */
    float *g_logits_dev;            /* f32 [n_samples][7]; OVERWRITTEN */
    float *g_values_dev;            /* f32 [n_samples]; OVERWRITTEN */
    float *stats_dev;               /* f32 [8]; OVERWRITTEN */
    float *scratch_dev;             /* f32 [scratch_words], 8-byte aligned, caller-owned, need not be zeroed */
    int64_t scratch_words;
    double clip_range;              /* > 0 */
    double clip_range_vf;           /* <= 0: no value clipping */
    double ent_coef;
    double vf_coef;
    int32_t adv_mode;               /* 0 raw, 1 minibatch statistics, 2 adv_stats_dev */
    int32_t reserved0;              /* 0 */
} mgx_ppo_loss_args;

/* Takes no engine handle.  Only enqueues on `stream` (no allocation, no host sync; capturable).
 * MGX_ERR_INVALID before any HIP call for: a null pointer (sel_dev excepted; adv_stats_dev unless adv_mode 2),
 * n_samples <= 0, adv_mode outside 0..2, clip_range <= 0, scratch_words below mgx_ppo_loss_scratch_words(...),
 * a scratch that is not 8-byte aligned. */
mgx_status mgx_ppo_loss(int64_t n_samples, const mgx_ppo_loss_args *a, void *stream);

/* ---- Gradient-norm clip + Adam over one flat array (added within ABI 9) ---------------------------------
 * Replaces torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm) followed by torch.optim.Adam.step()
 * (defaults: no weight decay, no amsgrad) for parameters, gradients and moments that each live in one flat
 * fp32 array:
 *    g = grad * grad_scale                (the data-parallel mean after one summing all-reduce)
 *    total = ||g||_2,  coef = min(1, max_grad_norm / (total + 1e-6))   (1 when max_grad_norm <= 0)
 *    grad <- g * coef                     (WRITTEN BACK: the clipped gradient stays inspectable, as p.grad)
 *    exp_avg <- exp_avg + (1 - beta1) (grad - exp_avg),  exp_avg_sq <- beta2 exp_avg_sq + (1 - beta2) grad^2
 *    param <- param - lr / (1 - beta1^step) * exp_avg / (sqrt(exp_avg_sq) / sqrt(1 - beta2^step) + eps)
 * The bias corrections are formed on the host in double from `step`, as torch forms them.  lr and the
 * corrections are therefore by-value arguments of mgx_adam_step: a captured graph bakes them in.
 * mgx_adam_step_sched (below) reads them from a device table instead, so one captured graph serves every step
 * of a schedule; betas, eps, max_grad_norm and grad_scale stay by value in both (constant over a run).  Non-finite gradients propagate exactly as in
 * torch (a NaN norm makes every gradient NaN); there is no special case.
 *
 * Summation order.  The norm is summed as mgx_ppo_loss sums: ceil(n_words / 1024) workgroups, at most 256,
 * fp64, fixed order, partials in scratch_dev, folded by every workgroup of the second launch.  Two launches,
 * no float atomics: bitwise reproducible for a given n_words. */
int64_t mgx_adam_scratch_words(int64_t n_words);            /* host only; -1 unless n_words > 0 */

typedef struct mgx_adam_args {
    double lr;
    double beta1, beta2;            /* each in [0, 1) */
    double eps;                     /* >= 0 */
    int64_t step;                   /* 1-based count of this step */
    double max_grad_norm;           /* <= 0: no clip */
    double grad_scale;              /* 1: none */
} mgx_adam_args;

/* param_dev .. exp_avg_sq_dev f32 [n_words], caller-owned, each updated in place.  total_norm_dev: optional
 * f32 [1], the norm before the clip.  scratch_dev f32 [scratch_words], 8-byte aligned, need not be zeroed.
 * Only enqueues on `stream` (no allocation, no host sync; capturable).  MGX_ERR_INVALID before any HIP call
 * for: a null pointer (total_norm_dev excepted), n_words <= 0, step < 1, a beta outside [0, 1), eps < 0,
 * scratch_words below mgx_adam_scratch_words(n_words), a scratch that is not 8-byte aligned. */
mgx_status mgx_adam_step(float *param_dev, float *grad_dev, float *exp_avg_dev, float *exp_avg_sq_dev,
                         int64_t n_words, const mgx_adam_args *a, float *total_norm_dev, float *scratch_dev,
                         int64_t scratch_words, void *stream);

/* Device-scheduled Adam (added within ABI 9): the two scalars of a step that change from step to step. */
typedef struct mgx_adam_sched {
    float step_size;                /* (float)(lr / (1 - beta1^step)) */
    float bc2_sqrt;                 /* (float)sqrt(1 - beta2^step) */
} mgx_adam_sched;

/* Host only, no HIP call: out_host[i] = the entry of step first_step + i at learning rate lr[i], i < n, by the
 * very function mgx_adam_step forms them with (double precision, then cast).  a->lr and a->step are ignored.
 * MGX_ERR_INVALID for: a null pointer, first_step < 1, n < 1, a beta outside [0, 1), eps < 0. */
mgx_status mgx_adam_schedule(const mgx_adam_args *a, const double *lr, int64_t first_step, int32_t n,
                             mgx_adam_sched *out_host);

/* mgx_adam_step with step_size and bc2_sqrt read from table_dev (mgx_adam_sched [table_len], on the device)
 * at a device-side cursor; a->lr and a->step are ignored, the rest of `a` is by value.  cursor_dev int32 [2] =
 * {next entry, overrun count}: thread 0 of the norm launch's first workgroup reads c = cursor[0] and writes
 * c + 1 (the only writer); the step launch of the same call uses entry cursor[0] - 1 (stream order).  With
 * that entry >= table_len the call updates nothing (total_norm_dev included) and adds 1 to cursor[1].  Plain
 * stores, no atomics.  The same kernels, arithmetic, summation order and grid as mgx_adam_step: every output is
 * bitwise what mgx_adam_step writes for the entry's (lr, step).  Calls that share a cursor must be on one
 * stream.  Validation as mgx_adam_step (step excepted), and MGX_ERR_INVALID for a null table_dev or
 * cursor_dev and table_len < 1, before any HIP call. */
mgx_status mgx_adam_step_sched(float *param_dev, float *grad_dev, float *exp_avg_dev, float *exp_avg_sq_dev,
                               int64_t n_words, const mgx_adam_args *a, const mgx_adam_sched *table_dev,
                               int32_t table_len, int32_t *cursor_dev, float *total_norm_dev, float *scratch_dev,
                               int64_t scratch_words, void *stream);

/* ---- Evaluation records on the device (added within ABI 9) -------------------------------------------
 * SB3 evaluate_policy's per-step episode accounting (stable_baselines3/common/evaluation.py; the loop body of
 * mgx/evaluation.py evaluate_policy) for every env of ONE vector step, in one launch and with no host decision,
 * so a captured graph can hold a block of evaluation steps (mgx/evaluation.py GraphEvaluator).
 * For env e, with target = (n_eval_episodes + e) / n_envs in integer arithmetic (episode_count_targets), the
 * step index t = base_dev[0] + step_offset and c = counts_dev[e]:
 *    rec = done[e] != 0 && c < target
 *    if rec: rewards[e][c] = reward64[e] (or (double) ep_return[e]),  lengths[e][c] = ep_len[e],
 *            when[e][c] = t,  missions[e][c] = mission_id[e],  counts[e] = c + 1
 *    remaining_dev[0] -= the number of envs with rec, one integer atomic per workgroup of 64 envs that recorded
 *    anything (a ballot's popcount); no float atomics, every output is reproducible.
 * Slots at or beyond an env's count and envs that record nothing are NOT written.  base_dev is only read: a
 * captured block of K steps bakes step_offset = 0 .. K-1 into its launches and advances base_dev by K once at
 * its end, so no launch orders against another through the counter.  The host sets remaining_dev to the sum of
 * the targets (= n_eval_episodes) before the first step; the evaluation is over when it reads 0.  A count
 * outside [0, cap) records nothing (the tables are never written out of bounds). */
typedef struct mgx_eval_record_args {
    const uint8_t *done_dev;        /* u8 [n_envs]: this step's done flags */
    const double *reward64_dev;     /* f64 [n_envs]: this step's reward (only an episode's last step pays, so it */
    const float *ep_return_dev;     /*   is the Monitor sum), or NULL: f32 [n_envs] ep_return_dev is read instead */
    const int32_t *ep_len_dev;      /* i32 [n_envs]: the length of the episode that just ended */
    const uint8_t *mission_id_dev;  /* u8 [n_envs]: the mission id of the observation the action was taken on */
    const int64_t *base_dev;        /* i64 [1]: step index of step_offset 0; READ only */
    int32_t *counts_dev;            /* i32 [n_envs]: episodes recorded so far; updated in place */
    double *rewards_dev;            /* f64 [n_envs][cap] */
    int32_t *lengths_dev;           /* i32 [n_envs][cap] */
    int64_t *when_dev;              /* i64 [n_envs][cap] */
    uint8_t *missions_dev;          /* u8 [n_envs][cap] */
    int32_t *remaining_dev;         /* i32 [1]: episodes still owed */
} mgx_eval_record_args;

/* Takes no engine handle.  Only enqueues on `stream` (no allocation, no host sync; capturable).
 * MGX_ERR_INVALID before any HIP call for: a null pointer (one of reward64_dev / ep_return_dev may be null),
 * n_envs <= 0, n_eval_episodes < 0, cap < 1, cap below the largest target ceil(n_eval_episodes / n_envs). */
mgx_status mgx_eval_record(int64_t n_envs, int64_t n_eval_episodes, int64_t cap, int64_t step_offset,
                           const mgx_eval_record_args *a, void *stream);

/* ---- The shortest-path expert on the device (added within ABI 9) ----------------------------------------
 * A stateless expert for demonstrations (behaviour cloning, DAgger) and as an optimal-length yardstick: the action
 * and the remaining cost of every env, from the env's current state alone (EnvState and the grid).  The reference's
 * counterpart is src/experts.py (a per-env Python A* over a full-grid observation, no locked doors), cloned by
 * `algo: bc` (src/hydra_configs/imitation.yaml).  mgx/expert.py expert_reference is the normative definition; this
 * call returns the same integers for the same state.
 *
 * Cost model over states (x, y, dir): LEFT / RIGHT cost 1; FORWARD into an empty cell or an open door costs 1;
 * entering a closed door costs 2 (TOGGLE, then FORWARD); entering a locked door costs 2, but only while carrying
 * the key of its colour; everything else is impassable (lava, walls, objects, any goal that is not the final
 * cell).  The agent's own cell is always a valid start.  D(s) is the cost-to-go to a goal set G.  The first action
 * is the argmin over [the forward move, LEFT, RIGHT] of edge cost + D(successor), ties in that order; the forward
 * move is TOGGLE when the front cell is a door that must be opened first.
 *
 * Rules, the first that applies decides (action, cost):
 *   1. mission_done: DONE, 0.
 *   2. no target cell (tx == 255): the target action if there is one, cost 1 ('drop' completes on the action
 *      alone); else ('move' missions) DONE, -1: unsupported.
 *   3. needed = the hand holds a key whose colour some locked door of the grid has.  Target action PICKUP with a
 *      full hand that is not needed: the drop routine, -2.
 *   4. route to the mission.  At-cell missions (target action 255 or 0): G = the target cell in any direction,
 *      which may be entered as the final move; cost D (standing on it already: DONE, 0).  Facing missions: G =
 *      every neighbour of the target, facing it; cost D + 1; at D == 0 the action is the target action, or (PICKUP
 *      with a full hand) the drop routine, -2.
 *   5. unreachable with a full hand that is not needed: the drop routine, -2.
 *   6. unreachable with an empty hand: G = every state facing a key, or a key-holding box, whose colour some
 *      locked door has; the route's first action, at D == 0 PICKUP for a key and TOGGLE for a box; cost -3.
 *   7. otherwise DONE, -4: give up.
 * Drop routine: the first empty cell among front, right, left, behind decides: DROP, RIGHT, LEFT, RIGHT; none: DONE.
 *
 * actions_dev: [N] int32 (action_bytes = 4) or int64 (8); cost_dev: optional i32 [N].  Reads the handle's state and
 * grids and nothing else of it, writes only its outputs; one launch (one lane per env, one wave per 64 envs, a
 * layered search bounded by 8 size^2 layers).  Only enqueues on `stream` (no allocation, no host sync): it can sit
 * in a captured graph between two mgx_step_compact calls.  MGX_ERR_INVALID before any HIP call for: a null handle
 * or actions_dev, action_bytes other than 4 or 8. */
mgx_status mgx_expert_act(mgx_handle *h, void *actions_dev, int action_bytes, int32_t *cost_dev /* optional */,
                          void *stream);

/* Makes `stream` wait for the in-flight refill, if any (no host sync). */
mgx_status mgx_join(mgx_handle *h, void *stream);

/* The effective configuration (defaults resolved: ring_depth, refill_every, ...). */
mgx_status mgx_get_config(const mgx_handle *h, mgx_config *out);

/* GAE over a [T][N] f32 rollout (DictRolloutBuffer.compute_returns_and_advantage):
 * episode_starts_dev f32 [T][N], last_values f32 [N], last_dones u8 [N];
 * writes advantages/returns f32 [T][N].  adv_stats_dev (optional, f64 [3]):
 * accumulates (sum A, sum A^2, count) for RCCL advantage-stat reduction, through per-workgroup
 * partials in stats_scratch_dev (f64 [MGX_GAE_SCRATCH_WORDS], caller-owned, zeroed before its first
 * use; every call leaves it zeroed).  Calls that may overlap (two collectors on two streams) pass
 * scratches of their own; NULL = one device-global scratch (such calls must then not overlap). */
#define MGX_GAE_SCRATCH_WORDS 512
mgx_status mgx_gae(const float *rewards_dev, const float *values_dev, const float *episode_starts_dev,
                   const float *last_values_dev, const uint8_t *last_dones_dev, int64_t T, int64_t N,
                   float gamma, float gamma_lambda, float *advantages_dev, float *returns_dev,
                   double *adv_stats_dev, double *stats_scratch_dev, void *stream);

/* GAE over the compact rollout layout: dones_dev u8 [T][N] is the `done` output of
 * step t (what mgx_step writes to done_dev), so next_non_terminal(t) = 1 - dones[t]
 * -- SB3's episode_starts[t+1] for t < T-1 and its last_dones at T-1.  Same fp32
 * op order, outputs and adv_stats_dev as mgx_gae; 17 B of traffic per element. */
mgx_status mgx_gae_dones(const float *rewards_dev, const float *values_dev, const uint8_t *dones_dev,
                         const float *last_values_dev, int64_t T, int64_t N, float gamma, float gamma_lambda,
                         float *advantages_dev, float *returns_dev, double *adv_stats_dev,
                         double *stats_scratch_dev, void *stream);

/* mgx_rollout_compact followed by mgx_gae_dones over the K steps it runs (its rewards_dev and dones_dev,
 * T = K), the GAE fused into the launch: each workgroup runs the recurrence of its 64 envs as soon as its
 * own K steps are done, reading back the rewards and dones it wrote (no second kernel over the rollout).
 * Same fp32 op order and outputs as mgx_gae_dones (bit for bit); adv_stats_dev / stats_scratch_dev as
 * there (the fold of the per-workgroup partials is a second, one-workgroup launch).  Replaces the
 * reference's collect_rollouts + compute_returns_and_advantage pair for a rollout whose actions are
 * known up front and whose horizon is this launch (ppo.py:159; SB3 OnPolicyAlgorithm.collect_rollouts). */
typedef struct mgx_gae_args {
    const float *values_dev;       /* f32 [K][N] */
    const float *last_values_dev;  /* f32 [N]: V(observation after step K-1) */
    float gamma, gamma_lambda;     /* gamma_lambda = float(gamma * gae_lambda), as mgx_gae_dones */
    float *advantages_dev;         /* f32 [K][N] */
    float *returns_dev;            /* f32 [K][N] */
    double *adv_stats_dev;         /* f64 [3] (optional) */
    double *stats_scratch_dev;     /* f64 [MGX_GAE_SCRATCH_WORDS] (optional) */
} mgx_gae_args;
mgx_status mgx_rollout_compact_gae(mgx_handle *h, const int32_t *actions_dev, int K, const mgx_rollout_out *out,
                                   const mgx_gae_args *gae, void *stream);

/* Scene record of env `env`'s current episode, for PlaygroundEnv.llm_description /
 * LLMDescriptionWrapper (environment.py:152-195; manual mode, one env): the episode is
 * regenerated on the device from the RNG state its generation started from, which only the
 * inline reset mode keeps (ring_depth = -1).  record (HOST, MGX_SCENE_WORDS u32):
 *   [0] number of objs entries, [1] agent x | y<<8 | dir<<16, [2] mission id | tx<<8 | ty<<16 |
 *   target action<<24, [3] abandoned attempts, [4] error bits, [8 .. 8+32) objs entries in
 *   placement order (type | COLOR_NAMES index<<4 | x<<8 | y<<16 | 1<<24 for a door's key or key
 *   box), [40 ..) the generated grid, one cell code byte per cell (y*S + x; S <= 16).
 * Synchronises `stream`. */
#define MGX_SCENE_WORDS 104
mgx_status mgx_scene(mgx_handle *h, int64_t env, uint32_t *record, void *stream);

/* Kernel clocks (measurement; ABI 6).  With clock_dev set, every workgroup of every launch of the step
 * kernels (mgx_step, mgx_step_compact, mgx_rollout_compact[_gae]: class 0) and of the refill kernel
 * (class 1) and the MT slide after it (class 2) records its start and end on the device (wall-clock ticks; *tick_khz, optional, receives
 * their rate), so that a caller can time the kernels INSIDE a replayed hipGraph, beside whatever runs
 * concurrently (bench.py: the timed region's own launches); a launch's span is the min start to the
 * max end over its workgroups.  clock_dev: u64 [mgx_clock_words(h, slots)], caller-owned, zeroed;
 * per class c (G = mgx_clock_groups(h, c) workgroups per launch), in order: cnt u64 [G] (launches so
 * far, per workgroup), then rec u64 [slots][G][2] {start, end} of launches 0 .. slots-1 (later
 * launches are counted, not recorded).  Kernel parameters are captured at launch: set the clock
 * before capturing a graph.  NULL clock_dev: off (the default). */
#define MGX_CLOCK_CLASSES 4   /* 0 step kernels (64-env blocks), 1 refill, 2 MT slide (the kernel that follows each
                                 refill), 3 (ABI 7) the fused rollout's 32-env blocks at S = 16 (0 groups otherwise):
                                 every launch of a class has its class's grid */
int64_t mgx_clock_words(const mgx_handle *h, int slots);
int mgx_clock_groups(const mgx_handle *h, int cls);
mgx_status mgx_set_clock(mgx_handle *h, uint64_t *clock_dev, int slots, int *tick_khz);

/* Synchronises `stream`, returns the device error bits (MGX_DEVERR_*) and clears them. */
mgx_status mgx_poll_error(mgx_handle *h, void *stream, uint32_t *bits);

/* Counters since create: [0] env-steps, [1] resets (incl. first), [2] abandoned
 * (live-locked) reset attempts, [3] max MT cursor, [4] pre-generated episodes
 * queued in the rings now (between two mgx_reset calls, episodes produced by
 * the refill = resets consumed + change of [4]), [5] refill launches enqueued (incl. the
 * synchronous fills of mgx_reset), [6] mgx_step calls since the last mgx_reset,
 * [7] MT19937 words generated so far (the device ring holds the last mt_table_words of them).
 * Synchronises `stream` and the refill stream. */
mgx_status mgx_stats(mgx_handle *h, void *stream, uint64_t out[8]);

/* The fused rollout's own random policy (ABI 7): once set, mgx_rollout_compact[_gae] may be called with
 * actions_dev = NULL, and each launch then draws its K x N actions on the device, in the DMA wave that would have
 * loaded them -- exactly mgx_random_actions' draws (n_actions 7) over a [K][N] buffer at counter c = the number of
 * such launches since this call (no actions buffer, nothing read).  enable = 0 turns it off.  Synchronises. */
mgx_status mgx_set_random_policy(mgx_handle *h, int enable, uint64_t seed);

/* Synthetic random policy (ABI 7; env.action_space.sample() for a whole batch -- the benchmark's random-action
 * rollouts, a random agent's evaluation): out_dev i32 [count] = uniform draws on {0 .. n_actions-1}
 * (1 <= n_actions <= 65536) from a counter-based hash of (seed, counter, i): key = splitmix64(seed + c *
 * 0x9E3779B97F4A7C15), h = splitmix64(key ^ (i * 0xD1B54A32D192ED03)), out = ((h >> 32) * n_actions) >> 32
 * (mod 2^64; c = counter_dev[0]).  The launch then advances counter_dev[0] by one on the device, so the same launch
 * captured in a hipGraph draws fresh actions at every replay.  counter_dev: u64 [2], caller-owned, zeroed before
 * the first use (word 1 is the launch's own workgroup tally; launches sharing a counter must not overlap). */
mgx_status mgx_random_actions(int32_t *out_dev, int64_t count, int n_actions, uint64_t seed, uint64_t *counter_dev,
                              void *stream);

/* Diagnostics (ABI 7): the episodes queued in each env's ring now, (tail - head) mod 2^16, into a HOST
 * array levels[N] (what mgx_stats [4] sums).  Synchronises `stream` and the refill stream.  Measurement
 * only, no reference counterpart (tools/diag_ring_levels.py: the ring-level distribution over long runs). */
mgx_status mgx_ring_levels(mgx_handle *h, void *stream, uint16_t *levels);

/* Diagnostics: the first n (<= 32) raw device counters.  [0..2], in every build, say how the refill used the
 * prefix records of the MT19937 stream (multi-room problems with the ring; zero otherwise): [0] lookups -- episode
 * generation attempts the refill started with the records on, since mgx_create; [1] hits -- those whose record
 * matched, so that the attempt took its MT-only prefix from it instead of drawing it; [2] the record frontier:
 * every stream word below it has had its record computed (mgx_stats [7] is the words generated, the frontier
 * follows it by what the last MT slide generated).  [3] unused; [4..31] phase / section clocks of -DMGX_STAMPS /
 * -DMGX_GEN_STAMPS / -DMGX_REFILL_CLOCK builds (zero otherwise).  Synchronises. */
mgx_status mgx_debug_counters(mgx_handle *h, void *stream, uint64_t *out, int n);

/* Test/debug: copy env state to HOST buffers (any may be NULL); synchronises.
 * grid u8 [N][S][S][4] (x-major (type,colour,state,box-holds-key)), agent u8 [N][3],
 * carrying u8 [N][4], step_count i32 [N], mission_done u8 [N], stored_reward f64 [N]
 * (NaN = None), mt_words i64 [N], pcg u64 [N][6] (state hi/lo, inc hi/lo,
 * has_uint32, uinteger), target u8 [N][3], mission_id u8 [N]. */
mgx_status mgx_dump_state(mgx_handle *h, void *stream, uint8_t *grid, uint8_t *agent, uint8_t *carrying,
                          int32_t *step_count, uint8_t *mission_done, double *stored_reward,
                          int64_t *mt_words, uint64_t *pcg, uint8_t *target, uint8_t *mission_id);

/* Mission text / tokens for a mission_id (host side, no device access). */
mgx_status mgx_mission_text(int mission_id, char *buf, size_t buflen);

#ifdef __cplusplus
}
#endif
#endif /* MGX_H_ */
