/*
 * sac_engine.h — C ABI of the MI355X (gfx950) SAC update engine.
 *
 * This is the drop-in boundary for the reference's hot path: the SAC gradient
 * step and the replay buffer it samples from.  The reference has no native or
 * FFI layer (pure Python/PyTorch); each entry point below replaces a Python
 * method of the reference and is bound from Python with ctypes by
 * soft-actor-critic_amd/sac/_engine.py (the host-side mirror of the reference
 * API; binding recipe in INTEGRATION.md).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless named *_host;
 *   - all launches are asynchronous on the given HIP stream (hipStream_t passed
 *     as void*; NULL = legacy default stream); no entry point synchronises the
 *     device except sac_engine_create (one-off table upload) and the profiling
 *     entry point;
 *   - parameters, Adam moments and replay storage are owned by the caller (the
 *     PyTorch caching allocator); the engine keeps raw pointers only;
 *   - return 0 on success, a negative SAC_E* code on error; sac_last_error()
 *     returns a description of the last error of the calling thread.
 *
 * Layouts
 *   - network parameters: one flat fp32 buffer per network, Linear layers in
 *     order, each as weight [out][in] (nn.Linear layout) followed by bias [out]
 *     — i.e. the concatenation of reference state_dict() values
 *     (net.0.weight, net.0.bias, net.2.weight, ...; sac/models.py:141-149);
 *   - Adam exp_avg / exp_avg_sq buffers use the same flat layout;
 *   - replay storage is fp32, ring-ordered, in one of two layouts (row_stride):
 *     struct-of-arrays obs[cap][obs_dim], act[cap][act_dim], rew[cap],
 *     next_obs[cap][obs_dim], done[cap] (row_stride = 0), or transition
 *     records [cap][row_stride] holding each row's fields at the field
 *     pointers' offsets (the default of sac/replay_buffer.py: obs | next_obs |
 *     act | rew | done, padded to whole 128-B lines, so a sampled row is 2
 *     cache lines at C2 instead of ~6.5);
 *     state[0] = number of valid rows, state[1] = next write slot
 *     (the oldest row once full), state[2] = push generation (incremented by
 *     every push and by ReplayBuffer.clear(); a batch the engine staged for
 *     the next step is used only while it matches).
 *
 * The done word
 *   - a stored row's done is a float d that every path of the gradient step
 *     reads as y = r + (gamma (1 - d)) (...).  By default d = terminated |
 *     truncated.  enum sac_done_mode / sac_engine_set_done_mode choose what the
 *     fused rollout step stores instead: terminated alone, or, for the staging
 *     table of n-step returns, the END CODE c = terminated + 2 * truncated in
 *     {0, 1, 2, 3}.  sac_replay_emit_nstep_codes turns a window of end codes
 *     into a row whose d is 0, 1, or 1 - gamma^k / gamma^n (<= 0) for a window
 *     the time limit closed after k of n steps.
 */
#ifndef SAC_ENGINE_H
#define SAC_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAC_MAX_LAYERS 8   /* slots of q_dims / pi_dims: the struct's layout.  The kernels take fewer: q_layers, pi_layers */

enum sac_status {
  SAC_OK = 0,
  SAC_E_INVALID = -1,     /* bad argument / unsupported shape */
  SAC_E_HIP = -2,         /* HIP runtime error */
  SAC_E_NOT_ENOUGH = -3,  /* replay holds fewer rows than the batch (ValueError in Python) */
};

enum sac_activation {     /* reference sac/models.py:104-112 _ACTIVATIONS */
  SAC_ACT_IDENTITY = 0, SAC_ACT_RELU = 1, SAC_ACT_TANH = 2, SAC_ACT_ELU = 3,
  SAC_ACT_LEAKY_RELU = 4, SAC_ACT_GELU = 5, SAC_ACT_SELU = 6
};

enum sac_precision {
  SAC_PREC_FP32 = 0,      /* v_mfma_f32_16x16x4_f32: exact-fp32 products (parity mode) */
  SAC_PREC_BF16 = 1       /* v_mfma_f32_16x16x32_bf16, fp32 accumulate, fp32 master weights */
};

/* Shape + hyper-parameters.  Mirrors the YAML keys the reference reads
 * (sac.*, q_net.*, policy_net.*, train.batch_size; sac/agent.py:22-115). */
typedef struct sac_engine_config {
  int32_t obs_dim, act_dim, batch;
  int32_t q_layers;                         /* number of Linear layers of Q: 2..6 (one to five hidden layers);
                                               anything else fails with SAC_E_INVALID, as for pi_layers */
  int32_t q_dims[SAC_MAX_LAYERS + 1];       /* q_dims[0]=obs+act ... q_dims[q_layers]=1 */
  int32_t q_hidden_act, q_out_act;
  int32_t pi_layers;                        /* number of Linear layers of pi: 2..6, independent of q_layers */
  int32_t pi_dims[SAC_MAX_LAYERS + 1];      /* pi_dims[0]=obs ... pi_dims[pi_layers]=2*act */
  int32_t pi_hidden_act, pi_out_act;
  float gamma, tau;
  float log_std_min, log_std_max, action_scale;
  double actor_lr, critic_lr, alpha_lr;      /* Python floats in the reference: kept in double */
  float beta1, beta2, adam_eps;             /* torch.optim.Adam defaults 0.9, 0.999, 1e-8 */
  int32_t auto_entropy;                     /* sac.auto_entropy_tuning */
  float target_entropy;                     /* -act_dim (agent.py:43) */
  int32_t precision;                        /* enum sac_precision */
  uint64_t seed;                            /* device RNG (replay indices, eps) */
  /* Kernel layout overrides.  0 everywhere = the engine's own choice: what the
   * drop-in classes pass and what every measured number uses.  The other
   * values exist for the parity tests and A/B runs; every setting computes the
   * same step (fp32 summation order aside).  The library reads no environment. */
  int32_t layout;        /* enum sac_layout */
  int32_t stage_path;    /* 0: only where the phase kernels' LDS layout does not fit;
                            1: force the layer-synchronous stage path; -1: refuse it (create fails).
                            1 is honoured only where the stage path applies: the hidden split was not
                            chosen, both nets have at least two hidden layers and act_dim <= 8.  Anywhere
                            else it is ignored without an error and the shape runs the kernels it would
                            run at 0.  A shape past the LDS layout with act_dim > 8 has no path: create
                            fails with the LDS figure. */
  int32_t stage_batch;   /* 0: phase C gathers the next step's batch; -1: phase A gathers its own */
  int32_t upd_parts;     /* 0: cost model; 1..4: batch parts of the large-batch (B > 1024) update tiles */
  int32_t upd_threads;   /* 0: auto; 512 / 1024: workgroup size of phase B's large-batch update tiles */
} sac_engine_config;

enum sac_layout {         /* phase A / C workgroup layouts (sac_engine_config.layout) */
  SAC_LAYOUT_AUTO = 0,    /* hidden-split role kernels where they apply, else roles, else pair tiles
                             (row tiles where the pair layout's LDS does not fit) */
  SAC_LAYOUT_ROLES = 1,   /* one workgroup per (network role, row tile): no hidden split */
  SAC_LAYOUT_ROWS = 2,    /* one workgroup per row tile running every network */
  SAC_LAYOUT_PAIRS = 3    /* one workgroup per (pair of row tiles, group of networks): large batches */
};

/* Caller-owned device state of one learner. */
typedef struct sac_engine_buffers {
  float *pi, *q1, *q2, *q1t, *q2t;          /* flat fp32 parameters */
  float *pi_m, *pi_v, *q1_m, *q1_v, *q2_m, *q2_v;  /* Adam exp_avg / exp_avg_sq */
  double *alpha_state;   /* [4]: log_alpha, alpha, adam m, adam v (fp64, agent.py:45-55) */
  double *opt_steps;     /* [4]: Adam step of policy, q1, q2, alpha optimizers */
  uint64_t *rng_step;    /* [1]: device RNG step counter */
  float *stats;          /* [4 + 2*batch]: losses Lq1,Lq2,Lpi,Lalpha; y[batch]; log_pi[batch] */
  void *workspace;       /* sac_engine_workspace_bytes() bytes, 256-B aligned */
  size_t workspace_bytes;
} sac_engine_buffers;

typedef struct sac_replay {
  float *obs, *act, *rew, *next_obs, *done;
  int64_t capacity;
  int32_t obs_dim, act_dim;
  int64_t *state;        /* device [3]: size, next write slot, push generation */
  int64_t row_stride;    /* 0: struct-of-arrays (each field its own dense [cap][width] array);
                            > 0: transition records -- every field is a column of ONE
                            [cap][row_stride] fp32 table (floats between consecutive rows) */
} sac_replay;

typedef struct sac_engine sac_engine;

const char *sac_last_error(void);
const char *sac_version(void);

/* Workspace the engine needs for this config (activations, packed compute
 * copies of the weights, split-K partials, tile tables). */
size_t sac_engine_workspace_bytes(const sac_engine_config *cfg);

/* Validates cfg, lays out the workspace, uploads the tile tables and writes the
 * packed compute copies of the weights (one synchronous call).
 * Replaces: SAC.__init__ network/optimizer setup, sac/agent.py:22-124. */
int sac_engine_create(const sac_engine_config *cfg, const sac_engine_buffers *buf,
                      void *stream, sac_engine **out);
void sac_engine_destroy(sac_engine *e);

/* Re-derive the packed compute copies after the host changed parameters
 * (load_state_dict, load_agent: sac/agent.py:538-554). */
int sac_engine_sync_params(sac_engine *e, void *stream);

/* n_steps consecutive SAC gradient steps (sample -> target -> critic -> actor ->
 * alpha -> Polyak), each exactly sac/agent.py:302-327.
 *   indices : NULL => device sampler (Philox-keyed Feistel permutation:
 *             distinct uniform rows, as random.sample, replay_buffer.py:39);
 *             else [n_steps][batch] int32 LOGICAL positions (0 = oldest row,
 *             the deque order of the reference).
 *   eps     : NULL => device Philox normals; else [n_steps][2][batch][act_dim]
 *             fp32 (target eps, then actor eps: the two rsample draws,
 *             sac/models.py:83).
 * Replaces: SAC.training_step (sac/agent.py:302-327) and the methods it calls
 * (sample_batch 166, compute_target_q_values 195, update_q_networks 213,
 * update_policy_network 238, update_entropy_temperature 263,
 * soft_update_target_networks 282). */
int sac_engine_train(sac_engine *e, const sac_replay *rb, int32_t n_steps,
                     const int32_t *indices, const float *eps, void *stream);

/* Same, replayed from a captured hipGraph of `chunk` steps (device sampler and
 * device eps only).  n_steps need not be a multiple of chunk; n_steps = 0
 * only captures the graph (no step runs). */
int sac_engine_train_graph(sac_engine *e, const sac_replay *rb, int32_t n_steps,
                           int32_t chunk, void *stream);

/* Policy action for n observations [n][obs_dim].  eps == NULL => deterministic
 * tanh(mu)*scale (models.py:89-92); else eps [n][act_dim] and the squashed
 * Gaussian sample (models.py:79-87).  log_pi may be NULL.
 * Replaces: SAC.select_action (sac/agent.py:149-156). */
int sac_policy_act(sac_engine *e, const float *obs, int32_t n, const float *eps,
                   float *action, float *log_pi, void *stream);

/* Q1 and Q2 of n (state, action) rows: q[n][2].  Rows i at obs + i*obs_stride,
 * act + i*act_stride (strides in floats, >= obs_dim / act_dim).  target != 0
 * evaluates the target critics.  Replaces: the critic forwards of
 * SAC._log_q_values (sac/agent.py:493-500). */
int sac_q_values(sac_engine *e, const float *obs, int64_t obs_stride, const float *act, int64_t act_stride,
                 int32_t n, int32_t target, float *q, void *stream);

/* The same for n consecutive ring slots of a replay buffer, starting at
 * first_slot and wrapping at capacity: (next_obs if use_next_obs else obs, act). */
int sac_q_values_replay(sac_engine *e, const sac_replay *rb, int64_t first_slot, int32_t n,
                        int32_t use_next_obs, int32_t target, float *q, void *stream);

/* Append n transitions (packed rows [n][2*obs+act+2] = s|a|r|s'|d, device) at
 * host-tracked (size, pos); writes the new (size, pos) to rb->state.
 * Replaces: ReplayBuffer.push (sac/replay_buffer.py:21-30). */
int sac_replay_push(const sac_replay *rb, const float *rows, int64_t n,
                    int64_t size_host, int64_t pos_host, void *stream);

/* ---- n-step returns (train.n_step) ---------------------------
 * `stage` is a replay table of capacity exactly n * num_envs, with rb's obs_dim
 * and act_dim, that holds the last n vector steps' one-step rows (o, a, r, o',
 * d) -- d = terminated | truncated, as sac_rollout_step and sac_replay_push
 * store them.  `newest` is the staging slot of environment 0's row of the newest
 * vector step; the row of environment i at age a (0 = newest) is slot (newest -
 * a * num_envs + i) mod (n * num_envs), and the window scanned is ages n - 1
 * down to 0, i.e. window steps j = 0 (oldest) .. n - 1.
 *
 * One launch writes num_envs n-step rows (o_0, a_0, R, o'_{k-1}, d_{k-1}) into
 * rb at slots (pos_host + i) % capacity: k is the smallest j + 1 with d_j = 1,
 * or n if there is none, and R = gpow[0] r_0 + gpow[1] r_1 + ... + gpow[k-1]
 * r_{k-1}, accumulated in float64 in that order starting from the first
 * product (so n = 1 copies every reward bit for bit, -0.0 included), without
 * fused multiply-adds, and rounded to fp32 once.  It also writes rb->state =
 * {min(capacity, size_host + num_envs), (pos_host + num_envs) % capacity,
 * generation + 1}, as sac_replay_push and sac_rollout_step do.  A window an
 * episode end closes never bootstraps (its done is 1) and an open one spans
 * exactly n steps, so the rows train as ordinary replay rows on an engine
 * created with gamma = gpow[n].
 *
 * gpow_host[0..n-1] (host memory, gpow[0] = 1, gpow[j] = gpow[j-1] * gamma) is
 * copied into the kernel arguments by value: the call keeps no host state, is
 * asynchronous on `stream` and can be captured.  Every argument is checked
 * before any HIP call; SAC_E_INVALID for a null table or field, n outside
 * 1..SAC_NSTEP_MAX, num_envs < 1, a staging capacity other than n * num_envs,
 * differing dims, num_envs > rb->capacity, newest / size_host / pos_host out of
 * range, and stage and rb the same table.  Both replay layouts work, for stage
 * and rb independently.
 * Replaces: nothing in the reference (one-step targets only, agent.py:195-211). */
#define SAC_NSTEP_MAX 8
int sac_replay_emit_nstep(const sac_replay *stage, const sac_replay *rb, int32_t n, int32_t num_envs,
                          int64_t newest, const double *gpow_host, int64_t size_host, int64_t pos_host,
                          void *stream);

/* ---- n-step rows from end codes (train.bootstrap_truncated) ---
 * sac_replay_emit_nstep with a staging table whose done column holds END CODES:
 * c = terminated + 2 * truncated as a float in {0, 1, 2, 3}, which the rollout
 * step stores in the mode SAC_DONE_END_CODE (sac_engine_set_done_mode).  k is
 * the smallest j + 1 with c_j != 0, or n; R, o'_{k-1}, the slots, rb->state and
 * the validation are sac_replay_emit_nstep's.  The stored done is
 *   +0.0f                                  if no row of the window ended,
 *   1.0f                                   if c_{k-1} is 1 or 3 (the closing step terminated),
 *   (float)(1.0 - gpow[k] / gpow[n])       if c_{k-1} is 2 (truncated only):
 * one float64 division, one float64 subtraction, one rounding; +0.0f at k = n,
 * negative for k < n.  The gradient step computes y = r + (gamma_eff (1 - d))
 * (...) with d read as a float, so on an engine created with gamma = gpow[n]
 * a window a truncation closed after k steps bootstraps with gamma^k (to within
 * 4 fp32 ulps) from the true next state, and one a termination closed does not
 * bootstrap.  gpow_host has n + 1 entries here (gpow[n] is read).  A table that
 * holds only 0 and 1 gives exactly sac_replay_emit_nstep's rows.
 * Replaces: nothing in the reference (it stores terminated | truncated,
 * agent.py:343-356, and one-step targets only). */
int sac_replay_emit_nstep_codes(const sac_replay *stage, const sac_replay *rb, int32_t n, int32_t num_envs,
                                int64_t newest, const double *gpow_host, int64_t size_host, int64_t pos_host,
                                void *stream);

/* Gather rows by LOGICAL index into SoA outputs (s[B][obs], a[B][act], r[B],
 * s2[B][obs], d[B]).  Replaces: ReplayBuffer.sample + SAC.sample_batch's
 * stacking (replay_buffer.py:32-39, agent.py:166-193). */
int sac_replay_gather(const sac_replay *rb, const int32_t *logical_idx, int32_t batch,
                      float *s, float *a, float *r, float *s2, float *d, void *stream);

/* Device sampler alone: `batch` distinct logical indices in [0, size) for RNG
 * (seed, step).  size is read from rb->state. */
int sac_replay_sample_indices(const sac_replay *rb, int32_t batch, uint64_t seed,
                              uint64_t step, int32_t *out, void *stream);

/* Device sampler + gather in ONE kernel: the sampler's `batch` distinct rows
 * for (seed, step) gathered into SoA outputs as sac_replay_gather does (the
 * indices are also written to idx_out unless it is NULL).  The caller
 * guarantees batch <= size (Python raises the reference's ValueError first).
 * Replaces: ReplayBuffer.sample + SAC.sample_batch (replay_buffer.py:32-39,
 * agent.py:166-193) with the device RNG in place of random.sample. */
int sac_replay_sample_gather(const sac_replay *rb, int32_t batch, uint64_t seed,
                             uint64_t step, int32_t *idx_out, float *s, float *a,
                             float *r, float *s2, float *d, void *stream);

/* Profiling: runs n_steps with hipEvents after each launch and returns the
 * mean event interval per phase launch in ms (ms_host holds 5 floats):
 * [0]=A target+critic-backward, [1]=B critic dW+Adam+Polyak, [2]=C actor,
 * [3]=D actor dW+Adam+alpha, [4]=the same interval for an empty kernel launched
 * the same way (diagnostic: an event + dispatch pair alone).  Each interval
 * includes its event's cost; bench.py removes it using the event-free graph
 * step time.  The sequence is queued behind a spin kernel, so the intervals are
 * device time, not host-submission time.  Synchronises the stream. */
int sac_engine_time_phases(sac_engine *e, const sac_replay *rb, int32_t n_steps,
                           float *ms_host, void *stream);

/* Temperature updates on (default) or off.  Off reproduces the reference
 * after SAC.load_agent with auto_entropy_tuning: it rebinds log_alpha to the
 * checkpoint's tensor but leaves alpha_optimizer bound to the old one
 * (sac/agent.py:550-554), so later steps still compute and report L_alpha while
 * log_alpha, alpha, its Adam moments and step count stay as loaded.  Takes
 * effect for launches (and graph replays) after this point on `stream`. */
int sac_engine_set_alpha_update(sac_engine *e, int32_t enabled, void *stream);

/* What the fused rollout step stores in a row's done word
 * (train.bootstrap_truncated). */
enum sac_done_mode {
  SAC_DONE_ANY_END = 0,     /* terminated | truncated (default; the reference's rows) */
  SAC_DONE_TERMINATED = 1,  /* terminated alone: a row the time limit ended bootstraps from its final_obs */
  SAC_DONE_END_CODE = 2     /* terminated + 2 * truncated in {0, 1, 2, 3}: rows of a staging table
                               (sac_replay_emit_nstep_codes), never of a replay the gradient step reads */
};

/* Sets the mode (default SAC_DONE_ANY_END).  Host state of the engine, no HIP
 * call: sac_rollout_step, sac_rollout_step_dev and the capture inside
 * sac_engine_loop_graph read it when they are called; the mode is part of the
 * loop graph's cache key, so a call in another mode captures again.  The
 * `store` argument of those calls keeps its meaning (non-zero = store);
 * nothing else in a stored row changes with the mode.  SAC_E_INVALID outside
 * 0..2. */
int sac_engine_set_done_mode(sac_engine *e, int32_t mode);

/* Where a sampled rollout step's actions come from (train.random_steps;
 * DESIGN.md §3.13). */
enum sac_action_source {
  SAC_ACTIONS_POLICY = 0,   /* the squashed-Gaussian sample of the policy (default) */
  SAC_ACTIONS_UNIFORM = 1   /* uniform in [-action_scale, action_scale): no policy forward (below) */
};

/* Sets the source (default SAC_ACTIONS_POLICY).  Host state of the engine, no
 * HIP call, exactly like sac_engine_set_done_mode: sac_rollout_step,
 * sac_rollout_step_dev and the capture inside sac_engine_loop_graph read it
 * when they are called, and it is part of the loop graph's cache key.  With
 * SAC_ACTIONS_UNIFORM a step with deterministic = 0 is one launch of a kernel
 * with one thread per environment row that reads nothing of the policy:
 * component j of env row i at RNG step t is word j % 4 of the Philox4x32-10
 * block with key = the engine's seed and counter (t lo, t hi, i, 5 << 16 | j /
 * 4) (which = 5), u = (float)(word >> 8) * 2^-24, a = action_scale * (2.0f * u
 * - 1.0f): 2u - 1 is exact, the product is the one rounding, the range is
 * [-action_scale, action_scale).  The environment step, the stored row, the
 * done word, rb->state and the cursor are the fused step's.  deterministic !=
 * 0 is the policy mean whatever the source.  The entry points validate as
 * before (the engine must still be able to run the policy).  SAC_E_INVALID
 * outside 0..1.
 * Replaces: env.action_space.sample() of SAC.warmup_replay_buffer
 * (sac/agent.py:137-147 of the reference), over the policy's own range. */
int sac_engine_set_action_source(sac_engine *e, int32_t source);

/* The same draws on the host: out_host[n][act_dim], row i component j as above
 * for (seed, t) and `scale`.  Needs no device and no engine.  SAC_E_INVALID,
 * with nothing written, for a null out_host, n < 1, act_dim outside 1..32 or a
 * scale that is not finite and positive. */
int sac_uniform_actions_host(uint64_t seed, uint64_t t, int32_t n, int32_t act_dim, float scale, float *out_host);

/* Health check (synchronises the stream): SAC_E_HIP if an in-launch
 * workgroup hand-off of the role-split phase kernels gave up waiting (the
 * affected steps are invalid), else 0.  Replaces: nothing (diagnostic). */
int sac_engine_check(sac_engine *e, void *stream);

/* Asynchronous status read: copies the engine's two status words [launch
 * epoch, hand-off timeout flag] into host_dst (pinned host memory; valid once
 * the stream has reached this point).  A non-zero timeout flag means a step's
 * results are invalid; the Python API raises RuntimeError on it (lazily, with
 * no per-step synchronisation).  sac_engine_clear_status resets the flag. */
int sac_engine_read_status(sac_engine *e, uint32_t *host_dst, void *stream);
int sac_engine_clear_status(sac_engine *e, void *stream);

/* Phase kernel names as they appear in rocprofv3 kernel traces. */
const char *sac_phase_kernel_name(int32_t phase);

/* ---- device-resident environments (sac/envs.py and sac/control_envs.py on the device)
 * N copies of one environment stepped in lockstep with SAME-STEP autoreset,
 * exactly as sac.vector_env.SyncVectorEnv drives the host classes: an
 * environment whose episode ended is reset inside the step, and the transition
 * of a step is (obs, action, reward, final_obs, terminated | truncated).  Values
 * the host classes keep as Python floats are doubles here, so the fp32-rounded
 * observations and rewards are the host's.
 *
 * Per-kind widths (the macros below the enum; sac_envs.pos / .vel are
 * component-major blocks [rows][num_envs] of doubles):
 *                          SAC_ENV_ACT_DIM  SAC_ENV_OBS_DIM   SAC_ENV_POS_ROWS  SAC_ENV_VEL_ROWS
 *   the probes (0..3)             1         1 (kind 2: any)          1          0 (vel may be NULL)
 *   SAC_ENV_PENDULUM              1               3                  1                 1
 *   SAC_ENV_REACHER               2              10                  4                 2
 *   SAC_ENV_CARTPOLE              1               4                  2                 2
 * Codes 4..7, 9..15 and 17..31 are not assigned.
 *
 * RNG (Philox4x32-10, key = seed, counter (t, env row, which << 16 | block)):
 * which = 2 the action noise of sac_rollout_step (key = the engine's seed,
 * block = action pair, Box-Muller as the training draws, which use 0 / 1);
 * which = 5 its uniform actions under SAC_ACTIONS_UNIFORM (key = the engine's
 * seed, block = four action components; sac_engine_set_action_source);
 * which = 3 the observation a SAC_ENV_RANDOM_OBS environment steps to at t,
 * which = 4 a reset draw at t (key = the environment seed; four draws per
 * block, u = (word >> 8) * 2^-24): the reset observation 2u - 1 of
 * SAC_ENV_RANDOM_OBS, block by block, and the reset state of a control task,
 * which is block 0's uniforms u0..u3 in double.  The initial reset is t = 0; the
 * k-th step (k = 0, 1, ...) is t = k + 1.
 *
 * The probes (sac/envs.py; see the enum).  One action component, one
 * observation (SAC_ENV_RANDOM_OBS: its obs_dim argument).
 *
 * The control tasks (sac/control_envs.py).  Each keeps its state in float64,
 * clips every action component to [action_low, action_high], observes the NEW
 * state in fp32, is truncated at max_steps, and restarts an episode that ended
 * at t from the reset draw of t.
 *
 * SAC_ENV_PENDULUM: the classic pendulum swing-up (PendulumEnv; g = 10, m = l =
 * 1, speed limit 8).  State (th, thdot): pos (th), vel (thdot).  With u the
 * clipped torque and an = ((th + pi) mod 2 pi) - pi, a step gives reward -(an^2
 * + 0.1 thdot^2 + 0.001 u^2) of the PRE-step state, thdot' = clip(thdot + (15
 * sin th + 3 u) dt, -8, 8), th' = th + thdot' dt; never terminated.
 * Observation (cos th, sin th, thdot).  Reset: th = pi (2 u0 - 1), thdot = 2 u1
 * - 1.
 *
 * SAC_ENV_REACHER: a planar two-link arm reaching for a target (ReacherEnv;
 * links L1 = L2 = 0.1, GAIN = 10, DAMP = 2, CTRL_COST = 0.1, target half side
 * 0.14).  State (th1, th2, w1, w2, tx, ty): pos (th1, th2, tx, ty), vel (w1,
 * w2).  The joints are decoupled first-order rotors: with u_j the j-th clipped
 * torque, dx = (L1 cos th1 + L2 cos(th1 + th2)) - tx and dy the same with sin
 * and ty, a step gives reward -sqrt(dx^2 + dy^2) - 0.1 (u0^2 + u1^2) of the
 * PRE-step state, w_j' = w_j + (10 u_j - 2 w_j) dt, th_j' = th_j + w_j' dt;
 * never terminated.  Observation (cos th1, cos th2, sin th1, sin th2, tx, ty,
 * w1, w2, dx, dy).  Reset: tx = 0.14 (2 u0 - 1), ty = 0.14 (2 u1 - 1), th1 = pi
 * (2 u2 - 1), th2 = pi (2 u3 - 1), w = 0.
 *
 * SAC_ENV_CARTPOLE: the classic balancing cart-pole (CartPoleEnv; G = 9.8,
 * M_CART = 1, M_POLE = 0.1, HALF_LEN = 0.5, FORCE_MAG = 10, X_LIMIT = 2.4,
 * TH_LIMIT = 12 degrees, all compile-time constants).  State (x, xdot, th,
 * thdot): pos (x, th), vel (xdot, thdot).  With u the clipped action, F = 10 u,
 * c = cos th, s = sin th, M = 1.1, temp = (F + 0.05 thdot^2 s) / M, thacc = (G s
 * - c temp) / (0.5 (4/3 - 0.1 c^2 / M)), xacc = temp - 0.05 thacc c / M, an
 * explicit Euler step x' = x + dt xdot, xdot' = xdot + dt xacc, th' = th + dt
 * thdot, thdot' = thdot + dt thacc.  Reward 1.0 on every step; terminated when
 * |x'| > X_LIMIT or |th'| > TH_LIMIT, independently of truncation: both may be
 * set, and rows end at different steps.  Observation (x, xdot, th, thdot).
 * Reset: x, xdot, th, thdot = 0.05 (2 u_k - 1), k = 0..3.  sin th and cos th
 * feed back into the state, so the device's trajectory follows the host class's
 * to a few float64 ulps, not to the bit. */
enum sac_env_kind {
  SAC_ENV_CONSTANT_REWARD = 0,  /* envs.py ConstantRewardEnv: r = reward, terminated at max_steps */
  SAC_ENV_QUADRATIC_ACTION = 1, /* QuadraticActionRewardEnv: r = -(clip(a) - target)^2 in fp32 */
  SAC_ENV_RANDOM_OBS = 2,       /* RandomObsBinaryRewardEnv: uniform obs, r = +1 iff |a| <= threshold */
  SAC_ENV_POINT_MASS = 3,       /* OneDPointMassReachEnv: pos += clip(a) * dt, reach goal_pos */
  SAC_ENV_PENDULUM = 8,         /* control_envs.py PendulumEnv: swing-up, obs (cos th, sin th, thdot) */
  SAC_ENV_REACHER = 16,         /* control_envs.py ReacherEnv: two-link arm, two torques, obs_dim 10 */
  SAC_ENV_CARTPOLE = 32         /* control_envs.py CartPoleEnv: balance, +1 per step, ends by failure, obs_dim 4 */
};

/* The width table above.  SAC_ENV_ACT_DIM: action components, the act_dim the replay buffer and the engine must
 * have.  SAC_ENV_OBS_DIM: the obs_dim the kind fixes; 0 where it is the caller's (SAC_ENV_RANDOM_OBS).
 * SAC_ENV_POS_ROWS / SAC_ENV_VEL_ROWS: rows of sac_envs.pos / .vel. */
#define SAC_ENV_ACT_DIM(kind) ((kind) == SAC_ENV_REACHER ? 2 : 1)
#define SAC_ENV_OBS_DIM(kind)                                                                         \
  ((kind) == SAC_ENV_PENDULUM ? 3 : (kind) == SAC_ENV_REACHER ? 10 : (kind) == SAC_ENV_CARTPOLE ? 4 : \
   (kind) == SAC_ENV_RANDOM_OBS ? 0 : 1)
#define SAC_ENV_POS_ROWS(kind) ((kind) == SAC_ENV_REACHER ? 4 : (kind) == SAC_ENV_CARTPOLE ? 2 : 1)
#define SAC_ENV_VEL_ROWS(kind) \
  ((kind) == SAC_ENV_REACHER || (kind) == SAC_ENV_CARTPOLE ? 2 : (kind) == SAC_ENV_PENDULUM ? 1 : 0)

/* The constructor arguments of the sac/envs.py class of `kind` (the others are
 * ignored); action bounds are rounded to fp32 as its Box stores them. */
typedef struct sac_env_config {
  int32_t kind;                 /* enum sac_env_kind */
  int32_t num_envs;
  int32_t obs_dim;              /* SAC_ENV_OBS_DIM(kind); SAC_ENV_RANDOM_OBS: its obs_dim argument */
  int32_t max_steps;
  double reward;                              /* SAC_ENV_CONSTANT_REWARD */
  double target;                              /* SAC_ENV_QUADRATIC_ACTION */
  double action_low, action_high;             /* SAC_ENV_QUADRATIC_ACTION, SAC_ENV_POINT_MASS and the control
                                                 tasks (the host class's bound, every component) */
  double threshold;                           /* SAC_ENV_RANDOM_OBS */
  double start_pos, goal_pos, dt, step_penalty, goal_reward, goal_tolerance;  /* SAC_ENV_POINT_MASS; dt also
                                                                                 the control tasks */
  uint64_t seed;                /* observation draws of SAC_ENV_RANDOM_OBS, reset draws of the control tasks */
} sac_env_config;

/* One cell of the episode record: written by every environment on every step. */
typedef struct sac_env_episode {
  double ret;                   /* return of the episode so far (sum of the double rewards) */
  int32_t length;               /* steps of the episode so far */
  int32_t ended;                /* 1 if the episode ended on this step (then ret / length are final) */
} sac_env_episode;

/* Caller-owned device state of num_envs environments. */
typedef struct sac_envs {
  sac_env_config cfg;
  float *obs;                   /* [num_envs][obs_dim] current observations */
  int32_t *step;                /* [num_envs] step in the episode (envs.py current_step) */
  int32_t *ep_length;           /* [num_envs] length of the running episode */
  double *pos;                  /* [SAC_ENV_POS_ROWS(kind)][num_envs]: SAC_ENV_POINT_MASS position; a control
                                   task's pos components, in the order of its section above */
  double *ep_return;            /* [num_envs] return of the running episode */
  sac_env_episode *episodes;    /* [ring_steps][num_envs] dense ring indexed by t % ring_steps and env row;
                                   NULL: no record (sac_envs_step only) */
  int64_t ring_steps;
  double *vel;                  /* [SAC_ENV_VEL_ROWS(kind)][num_envs]: a control task's vel components; may be
                                   NULL for the probes */
} sac_envs;

/* Reset every environment: step and episode counters to 0, the initial
 * observation (draws of SAC_ENV_RANDOM_OBS and the control tasks: which = 4, t = 0,
 * key `seed`).
 * Replaces: SyncVectorEnv.reset (sac/vector_env.py:39-46). */
int sac_envs_reset(const sac_envs *envs, uint64_t seed, void *stream);

/* Vector step t (>= 1) with the caller's actions [num_envs][SAC_ENV_ACT_DIM(kind)]: obs
 * [num_envs][obs_dim] (after autoreset), final_obs [num_envs][obs_dim] (the
 * true next state of every environment), reward [num_envs] fp32, terminated /
 * truncated [num_envs] bytes (0 / 1).
 * Replaces: SyncVectorEnv.step (sac/vector_env.py:55-71) over sac/envs.py. */
int sac_envs_step(const sac_envs *envs, const float *actions, uint64_t t, float *obs, float *final_obs,
                  float *reward, uint8_t *terminated, uint8_t *truncated, void *stream);

/* Act -> step -> store in ONE kernel: the policy forward on the environments'
 * current observations, the squashed-Gaussian sample (tanh(mu) * scale when
 * deterministic), the environment step, and the num_envs transitions written
 * into the replay ring at slots (pos_host + i) % capacity, with the new (size,
 * pos) and the push generation written to rb->state as sac_replay_push does.
 * store = 0 leaves the replay untouched (evaluation).  The done word of a
 * stored row follows the engine's sac_done_mode (default: terminated |
 * truncated); a sampled step's actions follow its sac_action_source (default:
 * the policy).  Needs envs->episodes and num_envs <= capacity.
 * Replaces: one iteration of SAC.run_vectorized_training_loop up to the
 * updates (select_actions, env.step, store_transitions; sac/agent.py:343-356
 * of the reference per environment). */
int sac_rollout_step(sac_engine *e, const sac_envs *envs, const sac_replay *rb, int64_t size_host,
                     int64_t pos_host, uint64_t t, int32_t deterministic, int32_t store, void *stream);

/* ---- device loop cursor ----------------------------------------------------
 * A caller-owned device array int64 cursor[2][4]; slot p holds {replay size,
 * next write slot, vector steps taken t, reserved 0}.  A launch that takes
 * (cursor, parity) reads slot `parity`; the rollout step also writes the
 * advanced cursor to slot parity ^ 1, so consecutive vector steps alternate
 * parity and no launch reads a word it writes.  The caller seeds slot 0 (or the
 * slot of its first parity) from its host mirrors; nothing else on the host
 * has to follow the loop, which is what lets sac_engine_loop_graph replay whole
 * iterations from one hipGraph. */

/* sac_rollout_step with (size, pos, t) read from cursor[parity]: the vector
 * step's RNG step is t + 1.  Writes cursor[parity ^ 1] = {min(capacity, size +
 * num_envs), (pos + num_envs) % capacity, t + 1, 0} and rb->state as
 * sac_rollout_step does; store = 0 writes {size, pos, t + 1, 0} and leaves the
 * replay alone.  A slot whose (size, pos) lie outside the ring (never seeded)
 * makes the launch a no-op. */
int sac_rollout_step_dev(sac_engine *e, const sac_envs *envs, const sac_replay *rb, int64_t *cursor,
                         int32_t parity, int32_t deterministic, int32_t store, void *stream);

/* sac_q_values_replay over the n rows written by the vector step whose
 * pre-step cursor is cursor[parity] (first slot = that slot's pos, wrapping at
 * capacity), into cell (t + 1) % q_ring_steps of q_ring[q_ring_steps][n][2]. */
int sac_q_values_replay_dev(sac_engine *e, const sac_replay *rb, const int64_t *cursor, int32_t parity,
                            int32_t n, int32_t use_next_obs, int32_t target, float *q_ring,
                            int32_t q_ring_steps, void *stream);

/* k_steps (even, >= 2) iterations of the device-resident loop as ONE hipGraph,
 * replayed n_replays times (0: capture only).  Iteration j is the rollout step
 * at parity j & 1 (sampled actions, store = 1), grad_steps_host[j] gradient
 * steps (device sampler and device eps, as sac_engine_train_graph; the caller
 * guarantees batch <= size by then), and, if q_ring is not NULL, the critic
 * evaluation of (next_obs, act) of the step's num_envs rows into its cell of
 * q_ring[q_ring_steps][num_envs][2].  Every replay starts at parity 0: the
 * caller seeds cursor[0] before the first replay of a run, and after any vector
 * step it issued another way.  The graph is cached on (envs, rb, cursor,
 * k_steps, the gradient-step counts, q_ring, q_ring_steps, the done mode, the
 * action source) -- a call with another key captures again -- apart from
 * sac_engine_train_graph's cache.
 * Replaces: k_steps iterations of SAC.run_vectorized_training_loop
 * (sac/agent.py:343-364 of the reference per environment). */
int sac_engine_loop_graph(sac_engine *e, const sac_envs *envs, const sac_replay *rb, int64_t *cursor,
                          int32_t k_steps, const int32_t *grad_steps_host, float *q_ring,
                          int32_t q_ring_steps, int32_t n_replays, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SAC_ENGINE_H */
