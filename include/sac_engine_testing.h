/*
 * sac_engine_testing.h — diagnostic exports of libsac_engine.so (not part of
 * the drop-in boundary; used by tools/ and tests/ only).
 */
#ifndef SAC_ENGINE_TESTING_H
#define SAC_ENGINE_TESTING_H
#include "sac_engine.h"
#ifdef __cplusplus
extern "C" {
#endif
/* Point the phase kernels at a device buffer of int64 s_memtime stamps
 * ([grid][64]); only builds with -DSAC_STAMPS write them. */
int sac_engine_debug_stamps(sac_engine *e, long long *dev_buf, void *stream);
int sac_engine_debug_stamped(void);
/* Launch ONE phase kernel of the current step (kind: 0 A, 1 B, 2 C, 3 D) on
 * the stream.  Timing experiments only:
 * re-running a phase out of sequence advances or corrupts the training state. */
int sac_engine_debug_launch(sac_engine* e, const sac_replay* rb, int32_t kind, void* stream);
/* The last step whose phase A took its batch from the record phase C staged
 * (0: none yet); synchronises the stream. */
int sac_engine_debug_staged_step(sac_engine* e, uint64_t* step_out, void* stream);
/* 1 if phases A/C run role-split (per-network workgroups with in-launch
 * hand-offs), 0 if one workgroup per row tile runs all networks. */
int sac_engine_uses_roles(const sac_engine *e);
/* 1 if phases A/C run the hidden-split role kernels (sac_split.h: two
 * workgroups per role and row tile, each with half of the 256-wide layer 1). */
int sac_engine_uses_split(const sac_engine *e);
/* 1 if phases A/C run the pair-tile kernels (sac_pairs.h: one workgroup per
 * pair of row tiles and group of networks; config.layout = SAC_LAYOUT_PAIRS). */
int sac_engine_uses_pairs(const sac_engine *e);
/* Launches per gradient step of the large-batch stage path (sac_wide.h:
 * layer-synchronous GEMM stages for phases A and C, used where the per-network
 * role kernels do not fit), else 0. */
int sac_engine_uses_wide(const sac_engine *e);
/* Launches per step of each phase A, B, C, D into out[4] (the stage path runs
   several per phase; its first-step gather is not counted); returns 0. */
int sac_engine_phase_launches(const sac_engine *e, int32_t *out);
/* Host evaluation of the device sampler (the same inline code as the sampler
 * inside sac_engine_train and sac_replay_sample_indices): out[b] = b-th element
 * of the Philox-keyed Feistel permutation of [0, size) for RNG (seed, step). */
int sac_debug_sample_indices_host(int64_t size, int32_t batch, uint64_t seed, uint64_t step, int32_t *out);
/* Host evaluation of the device eps draws of one step (the same inline
 * philox_normal2 the phase kernels call in their default device-RNG mode, compiled
 * for the host): out[which][b][j], which = 0 the target rsample (agent.py:204),
 * 1 the actor rsample (agent.py:241), rows b < batch, action dims j < act_dim
 * (models.py:83: eps of rsample).  Counter (step, b, which << 16 | j / 2), key
 * seed; Box-Muller gives dims 2p and 2p + 1. */
int sac_debug_eps_host(uint64_t seed, uint64_t step, int32_t batch, int32_t act_dim, float *out);
/* Host evaluation of csrc/sac_math.h, the acting head, target, seed and min-Q
 * arithmetic that sac_policy_act_kernel, the rollout step and the stage path
 * call, compiled for the host (so exp / tanh / log1p are the host libm's).
 * in[SAC_HEAD_NIN][n] holds n independent elements, row k = input k;
 * out[SAC_HEAD_NOUT][n] receives, per element: head_act(mu, lsr, e) (LS = the
 * clamped log sigma, ACT_Z, ACT_ACT), head_act_mean (ACT_MEAN), head_act_lp and
 * head_corr (ACT_LP, ACT_CORR: one action dim's log pi terms); Y = td_target(r,
 * d, gamma, q1, q2, alpha, lp) with q1, q2 as the target critics and lp as
 * log pi'; critic_seed(q1, Y, B) (SEED_D, SEED); minq_weights(q1, q2, -1 / B)
 * (MINQ, W1, W2) and PI_TERM = alpha lp - MINQ. */
enum { SAC_HEAD_IN_MU, SAC_HEAD_IN_LSR, SAC_HEAD_IN_E, SAC_HEAD_IN_Q1, SAC_HEAD_IN_Q2, SAC_HEAD_IN_R, SAC_HEAD_IN_D,
       SAC_HEAD_IN_LP, SAC_HEAD_NIN };
enum { SAC_HEAD_LS, SAC_HEAD_ACT_Z, SAC_HEAD_ACT_ACT, SAC_HEAD_ACT_MEAN, SAC_HEAD_ACT_LP, SAC_HEAD_ACT_CORR,
       SAC_HEAD_Y, SAC_HEAD_SEED_D, SAC_HEAD_SEED, SAC_HEAD_MINQ, SAC_HEAD_W1, SAC_HEAD_W2, SAC_HEAD_PI_TERM,
       SAC_HEAD_NOUT };
int sac_debug_head_host(int32_t n, const float *in, float lo, float hi, float scale, float gamma, float alpha,
                        int32_t B, float *out);
/* The same draws computed on the device (out: device [2][batch][act_dim]). */
int sac_debug_eps_device(uint64_t seed, uint64_t step, int32_t batch, int32_t act_dim, float *out, void *stream);
/* Polls a hand-off wait makes before it gives up and sets the timeout flag
 * (default 1 << 22, about 0.3 s); synchronises the stream.  A bound of 0
 * forces the timeout path (tests/test_gpu_engine.py): the API must raise. */
int sac_engine_debug_set_spin_limit(sac_engine *e, int32_t polls, void *stream);
/* Host evaluation of the action noise sac_rollout_step draws at vector step t
 * (the same inline philox_normal2, which = 2): out[i][j], env rows i < n,
 * action dims j < act_dim.  Counter (t, i, 2 << 16 | j / 2), key seed (the
 * engine's); Box-Muller gives dims 2p and 2p + 1. */
int sac_debug_rollout_eps_host(uint64_t seed, uint64_t t, int32_t n, int32_t act_dim, float *out);
/* The same draws computed on the device (out: device [n][act_dim]), with the
 * device library's logf / sincosf: what the fused step adds to mu, to the bit. */
int sac_debug_rollout_eps_device(uint64_t seed, uint64_t t, int32_t n, int32_t act_dim, float *out, void *stream);
/* Host evaluation of the observation draws of SAC_ENV_RANDOM_OBS (the same
 * inline code as the device's): out[i][k], env rows i < n, k < obs_dim, for
 * which = 3 (the observation stepped to at t) or 4 (the reset observation at
 * t).  Counter (t, i, which << 16 | k / 4), key seed (the environments');
 * output word k % 4: u = (word >> 8) * 2^-24, obs = 2u - 1 in [-1, 1). */
int sac_debug_env_obs_host(uint64_t seed, uint64_t t, int32_t which, int32_t n, int32_t obs_dim, float *out);
/* One step of SAC_ENV_PENDULUM on the host: the inline dynamics the device
 * kernels call (csrc/sac_envs.h EnvTask<ENV_CLASS_PENDULUM>::dynamics), compiled for the host, so
 * sin / cos are the host libm's.  cfg supplies action_low, action_high, dt and
 * max_steps (kind must be SAC_ENV_PENDULUM); state = (th, thdot) is advanced in
 * place; `step` is the step in the episode before this one.  Outputs: the
 * observation stepped to, the reward of the pre-step state, truncated = step +
 * 1 >= max_steps.  No autoreset: the caller applies the reset draw below. */
int sac_debug_env_step_host(const sac_env_config *cfg, double state[2], int32_t step, float action,
                            float obs_out[3], double *reward, int32_t *truncated);
/* The reset state (th, thdot) of SAC_ENV_PENDULUM row `row` at vector step t
 * (t = 0: the initial reset) for environment seed `seed`: the same inline code
 * as the device's, state_out = {pi (2 u0 - 1), 2 u1 - 1} with u0, u1 the first
 * two uniforms of sac_debug_env_obs_host's which = 4 block 0. */
int sac_debug_env_reset_host(uint64_t seed, uint64_t t, int32_t row, double state_out[2]);
/* One step of SAC_ENV_REACHER on the host: the inline dynamics the device
 * kernels call (csrc/sac_envs.h EnvTask<ENV_CLASS_REACHER>::dynamics), compiled for the host, so
 * sin / cos / sqrt are the host libm's.  cfg supplies action_low, action_high,
 * dt and max_steps (kind must be SAC_ENV_REACHER); state = (th1, th2, w1, w2,
 * tx, ty), the order of ReacherEnv.state, is advanced in place; `step` is the
 * step in the episode before this one.  Outputs: the observation stepped to,
 * the reward of the pre-step state, truncated = step + 1 >= max_steps.  No
 * autoreset: the caller applies the reset draw below. */
int sac_debug_reacher_step_host(const sac_env_config *cfg, double state[6], int32_t step, const float action[2],
                                float obs_out[10], double *reward, int32_t *truncated);
/* The reset state of SAC_ENV_REACHER row `row` at vector step t (t = 0: the
 * initial reset) for environment seed `seed`, in the same order: the same
 * inline code as the device's, (th1, th2) = pi (2 u - 1) of the third and
 * fourth uniform of sac_debug_env_obs_host's which = 4 block 0, w1 = w2 = 0,
 * (tx, ty) = 0.14 (2 u - 1) of its first and second. */
int sac_debug_reacher_reset_host(uint64_t seed, uint64_t t, int32_t row, double state_out[6]);
/* One step of SAC_ENV_CARTPOLE on the host: the inline dynamics the device
 * kernels call (csrc/sac_envs.h EnvTask<ENV_CLASS_CARTPOLE>::dynamics), compiled for the host, so
 * sin / cos are the host libm's.  cfg supplies action_low, action_high, dt and
 * max_steps (kind must be SAC_ENV_CARTPOLE); state = (x, xdot, th, thdot), the
 * order of CartPoleEnv.state, is advanced in place; `step` is the step in the
 * episode before this one.  Outputs: the observation stepped to, the reward
 * (1.0), terminated = the new state is outside a limit, truncated = step + 1 >=
 * max_steps (both may be set).  No autoreset: the caller applies the reset draw
 * below. */
int sac_debug_cartpole_step_host(const sac_env_config *cfg, double state[4], int32_t step, const float action[1],
                                 float obs_out[4], double *reward, int32_t *terminated, int32_t *truncated);
/* The reset state of SAC_ENV_CARTPOLE row `row` at vector step t (t = 0: the
 * initial reset) for environment seed `seed`, in the same order: the same
 * inline code as the device's, 0.05 (2 u_k - 1) of the four uniforms of
 * sac_debug_env_obs_host's which = 4 block 0. */
int sac_debug_cartpole_reset_host(uint64_t seed, uint64_t t, int32_t row, double state_out[4]);
/* A host-only engine: the validated config and no device state (no HIP call is
 * made).  For the argument checks of the forward-only entry points --
 * sac_q_values, sac_q_values_replay, sac_policy_act and sac_rollout_step -- on
 * a machine without a device: with valid arguments they return SAC_E_INVALID
 * ("no device state") where the launch would be.  Pass it to no other entry
 * point but sac_engine_destroy. */
int sac_debug_engine_host(const sac_engine_config *cfg, sac_engine **out);
/* The plan sac_engine_create would make of cfg on a device of ncu compute
 * units, as one JSON object in out[cap]; no HIP call is made and nothing is
 * dereferenced.  The config is validated and planned as create does it, and
 * refused (SAC_E_INVALID, sac_last_error()) where and as create refuses it
 * before its first HIP call; also when cap is too small.  Fields: "path"
 * ("split" | "roles" | "pairs" | "rows" | "wide"), the scalars workspace_bytes,
 * lds_bytes, upd_lds, upd_lds_b, upd_threads_b, nB, nD, nrt, xs, role_xcd,
 * stage, upd_slots; "launch": grid, threads and dynamic LDS bytes of phases A,
 * B, C, D (the stage path: B, D and "stages", its launch list: kind, j0, j1,
 * grid, phase, last, lds); "hash": FNV-1a 64 of the bytes of the device
 * descriptor, the update-tile arrays of phases B and D, and the stage path's
 * descriptor and job array (of no bytes off the stage path).
 * Device addresses in the hashed descriptors are these fake ones: the
 * workspace at SAC_PLAN_FAKE_WORKSPACE, buffer i of sac_engine_buffers (pi,
 * q1, ... stats: the fifteen pointers before workspace, in struct order) at
 * SAC_PLAN_FAKE_BUFFER0 + i * SAC_PLAN_FAKE_BUFFER_STEP: 256-byte aligned and
 * 1 TiB apart, further than any buffer or workspace reaches. */
#define SAC_PLAN_FAKE_WORKSPACE 0x200000000000ull
#define SAC_PLAN_FAKE_BUFFER0 0x010000000000ull
#define SAC_PLAN_FAKE_BUFFER_STEP 0x010000000000ull
int sac_debug_plan_host(const sac_engine_config *cfg, int32_t ncu, char *out, size_t cap);
#ifdef __cplusplus
}
#endif
#endif
