// sac_envs.h — the probe environments of sac/envs.py and the Pendulum swing-up
// two-link reacher and balancing cart-pole of sac/control_envs.py on the
// device, and the fused rollout step (act -> step -> store in one launch).
//
//   * pendulum_dynamics: one step of the swing-up in float64, host-callable;
//   * reacher_dynamics: one step of the reacher (two action components), likewise;
//   * cartpole_dynamics: one step of the cart-pole (the kind that terminates by failure), likewise;
//   * env_step: ONE statement of the environments' dynamics, with the semantics
//     sac.vector_env.SyncVectorEnv gives the host classes (same-step autoreset;
//     the transition is (obs, action, reward, final_obs, terminated | truncated)).
//     Whatever sac/envs.py keeps as a Python float is a double here, so the
//     fp32-rounded observations and rewards are the host's bit for bit;
//   * sac_envs_step_kernel: N environments stepped with the caller's actions;
//   * sac_rollout_step_kernel<T, KC>: sibling of sac_policy_act_kernel<T>
//     (same workgroup shape, LDS layout and mlp_forward call); the thread that
//     owns environment row i samples its action, steps the environment and
//     writes the transition into the replay ring.  Compiled once per kind class
//     KC (the probes, the pendulum, the reacher, the cart-pole); the host picks by the
//     environments' kind;
//   * sac_rollout_step_dev_kernel<T, KC>: the same body with (size, pos,
//     t) read from a two-slot cursor in device memory, so whole loop iterations
//     replay from one hipGraph (sac_engine_loop_graph).
//
// State is caller-owned global memory (include/sac_engine.h sac_envs).  Every
// environment row is read and written by exactly one thread of one launch, and
// every episode-ring cell by its own row: no atomics, no hand-offs, nothing
// depends on the order workgroups run in.
#pragma once
#include "../../include/sac_engine.h"
#include "sac_phases.h"

// Action components an environment of `kind` takes: 1 (envs.py: every probe's action_space has shape
// (1,), and so has the pendulum's) except the reacher's 2.
__host__ __device__ inline int env_act_dim(int kind) { return SAC_ENV_ACT_DIM(kind); }
// The rollout kernels are compiled once per kind class, so no class holds another's code.
enum EnvClass { ENV_CLASS_PROBES = 0, ENV_CLASS_PENDULUM = 1, ENV_CLASS_REACHER = 2, ENV_CLASS_CARTPOLE = 3 };
inline int env_class(int kind) {
  return kind == SAC_ENV_PENDULUM   ? ENV_CLASS_PENDULUM
         : kind == SAC_ENV_REACHER  ? ENV_CLASS_REACHER
         : kind == SAC_ENV_CARTPOLE ? ENV_CLASS_CARTPOLE
                                    : ENV_CLASS_PROBES;
}
// Philox `which` values of the rollout (0 / 1 are the training draws)
#define ENV_WHICH_NOISE 2u  // action noise of a rollout step, key = engine seed
#define ENV_WHICH_STEP 3u   // observation an environment steps to at t, key = env seed
#define ENV_WHICH_RESET 4u  // its reset observation at t

// Four uniforms in [0, 1) for (t, row, which, block): counter (t, row,
// which << 16 | block), key = seed; the top 24 bits of each output word.
// Host-callable so the C ABI exports the same inline code (sac_debug_env_obs_host).
__host__ __device__ inline void philox_uniform4(uint64_t seed, uint64_t t, uint32_t row, uint32_t which,
                                                uint32_t block, float u[4]) {
  uint32_t c[4] = {(uint32_t)t, (uint32_t)(t >> 32), row, (which << 16) | block};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
  for (int k = 0; k < 4; ++k) u[k] = (float)(c[k] >> 8) * 5.9604644775390625e-8f;
}
// 2u - 1 is exact in fp32 (u is a multiple of 2^-24 below 1): obs in [-1, 1)
__host__ __device__ inline float env_uniform_obs(float u) { return 2.0f * u - 1.0f; }

// np.clip on float32: min(max(x, lo), hi) with NaN passed through
__host__ __device__ inline float clip_f32(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

// ---- Pendulum swing-up (sac/control_envs.py PendulumEnv) --------------------
// State (th, thdot) in float64; g = 10, m = l = 1, so 3 g / (2 l) = 15 and
// 3 / (m l^2) = 3 exactly.  Every operation below is the host class's, in its
// order (the library is built with -ffp-contract=off: no fused multiply-adds).
#define SAC_PENDULUM_OBS_DIM 3
#define SAC_PENDULUM_MAX_SPEED 8.0
#define SAC_PI 3.141592653589793

// Python's ((th + pi) % (2 pi)) - pi: the angle in [-pi, pi)
__host__ __device__ inline double pendulum_angle(double th) {
  double an = fmod(th + SAC_PI, 2.0 * SAC_PI);
  if (an < 0.0) an += 2.0 * SAC_PI;
  return an - SAC_PI;
}

// The observation of a state, in fp32
__host__ __device__ inline void pendulum_obs(double th, double thdot, float obs[SAC_PENDULUM_OBS_DIM]) {
  obs[0] = (float)cos(th);
  obs[1] = (float)sin(th);
  obs[2] = (float)thdot;
}

// One step from (th, thdot) with action a: the reward of the PRE-step state,
// the new state in place and its observation (cos th', sin th', thdot') in fp32.
__host__ __device__ inline double pendulum_dynamics(double& th, double& thdot, float a, double action_low,
                                                    double action_high, double dt, float obs[SAC_PENDULUM_OBS_DIM]) {
  const double u = (double)clip_f32(a, (float)action_low, (float)action_high);
  const double an = pendulum_angle(th);
  const double reward = -(an * an + 0.1 * thdot * thdot + 0.001 * u * u);
  double v = thdot + (15.0 * sin(th) + 3.0 * u) * dt;
  v = v < -SAC_PENDULUM_MAX_SPEED ? -SAC_PENDULUM_MAX_SPEED : (v > SAC_PENDULUM_MAX_SPEED ? SAC_PENDULUM_MAX_SPEED : v);
  th = th + v * dt;
  thdot = v;
  pendulum_obs(th, thdot, obs);
  return reward;
}

// The reset draw of env row `row` at vector step t: th ~ U[-pi, pi), thdot ~
// U[-1, 1) from the first two uniforms of the row's ENV_WHICH_RESET block 0.
__host__ __device__ inline void pendulum_reset_draw(uint64_t seed, uint64_t t, uint32_t row, double& th,
                                                    double& thdot) {
  float u[4];
  philox_uniform4(seed, t, row, ENV_WHICH_RESET, 0, u);
  th = SAC_PI * (2.0 * (double)u[0] - 1.0);
  thdot = 2.0 * (double)u[1] - 1.0;
}

// ---- Two-link reacher (sac/control_envs.py ReacherEnv) ----------------------
// State s = (th1, th2, w1, w2, tx, ty) in float64, the order of ReacherEnv.state.
// Sine and cosine enter the reward and the observation only, never the state:
// the state trajectory is the host's bit for bit whatever library they come from.
#define SAC_REACHER_OBS_DIM 10
#define SAC_REACHER_L1 0.1
#define SAC_REACHER_L2 0.1
#define SAC_REACHER_GAIN 10.0
#define SAC_REACHER_DAMP 2.0
#define SAC_REACHER_CTRL_COST 0.1
#define SAC_REACHER_TARGET_HALF_SIDE 0.14

// Fingertip minus target
__host__ __device__ inline void reacher_tip(const double s[6], double& dx, double& dy) {
  dx = (SAC_REACHER_L1 * cos(s[0]) + SAC_REACHER_L2 * cos(s[0] + s[1])) - s[4];
  dy = (SAC_REACHER_L1 * sin(s[0]) + SAC_REACHER_L2 * sin(s[0] + s[1])) - s[5];
}

// The observation of a state, in fp32
__host__ __device__ inline void reacher_obs(const double s[6], float obs[SAC_REACHER_OBS_DIM]) {
  double dx, dy;
  reacher_tip(s, dx, dy);
  obs[0] = (float)cos(s[0]);
  obs[1] = (float)cos(s[1]);
  obs[2] = (float)sin(s[0]);
  obs[3] = (float)sin(s[1]);
  obs[4] = (float)s[4];
  obs[5] = (float)s[5];
  obs[6] = (float)s[2];
  obs[7] = (float)s[3];
  obs[8] = (float)dx;
  obs[9] = (float)dy;
}

// One step from s with actions (a0, a1): the reward of the PRE-step state, the
// new state in place and its observation in fp32.
__host__ __device__ inline double reacher_dynamics(double s[6], float a0, float a1, double action_low,
                                                   double action_high, double dt, float obs[SAC_REACHER_OBS_DIM]) {
  const double u0 = (double)clip_f32(a0, (float)action_low, (float)action_high);
  const double u1 = (double)clip_f32(a1, (float)action_low, (float)action_high);
  double dx, dy;
  reacher_tip(s, dx, dy);
  const double reward = -sqrt(dx * dx + dy * dy) - SAC_REACHER_CTRL_COST * (u0 * u0 + u1 * u1);
  s[2] = s[2] + (SAC_REACHER_GAIN * u0 - SAC_REACHER_DAMP * s[2]) * dt;
  s[3] = s[3] + (SAC_REACHER_GAIN * u1 - SAC_REACHER_DAMP * s[3]) * dt;
  s[0] = s[0] + s[2] * dt;
  s[1] = s[1] + s[3] * dt;
  reacher_obs(s, obs);
  return reward;
}

// The reset draw of env row `row` at vector step t: the four uniforms of the
// row's ENV_WHICH_RESET block 0 give the target in the square of half side 0.14
// and both angles in [-pi, pi); the arm starts at rest.
__host__ __device__ inline void reacher_reset_draw(uint64_t seed, uint64_t t, uint32_t row, double s[6]) {
  float u[4];
  philox_uniform4(seed, t, row, ENV_WHICH_RESET, 0, u);
  s[4] = SAC_REACHER_TARGET_HALF_SIDE * (2.0 * (double)u[0] - 1.0);
  s[5] = SAC_REACHER_TARGET_HALF_SIDE * (2.0 * (double)u[1] - 1.0);
  s[0] = SAC_PI * (2.0 * (double)u[2] - 1.0);
  s[1] = SAC_PI * (2.0 * (double)u[3] - 1.0);
  s[2] = 0.0;
  s[3] = 0.0;
}

// Row i's state in the component-major blocks ev.pos [4][N] (th1, th2, tx, ty) and ev.vel [2][N] (w1, w2)
__device__ __forceinline__ void reacher_load(const sac_envs& ev, int i, double s[6]) {
  const size_t n = (size_t)ev.cfg.num_envs;
  s[0] = ev.pos[i];
  s[1] = ev.pos[n + i];
  s[2] = ev.vel[i];
  s[3] = ev.vel[n + i];
  s[4] = ev.pos[2 * n + i];
  s[5] = ev.pos[3 * n + i];
}
__device__ __forceinline__ void reacher_store(const sac_envs& ev, int i, const double s[6]) {
  const size_t n = (size_t)ev.cfg.num_envs;
  ev.pos[i] = s[0];
  ev.pos[n + i] = s[1];
  ev.vel[i] = s[2];
  ev.vel[n + i] = s[3];
  ev.pos[2 * n + i] = s[4];
  ev.pos[3 * n + i] = s[5];
}

// ---- Balancing cart-pole (sac/control_envs.py CartPoleEnv) ------------------
// State s = (x, xdot, th, thdot) in float64, the order of CartPoleEnv.state.
// Every operation is the host class's, in its order.  sin th and cos th feed
// back into the state, so the trajectory follows the host's to the library's
// few float64 ulps, not to the bit.
#define SAC_CARTPOLE_OBS_DIM 4
#define SAC_CARTPOLE_G 9.8
#define SAC_CARTPOLE_M_CART 1.0
#define SAC_CARTPOLE_M_POLE 0.1
#define SAC_CARTPOLE_HALF_LEN 0.5
#define SAC_CARTPOLE_FORCE_MAG 10.0
#define SAC_CARTPOLE_X_LIMIT 2.4
#define SAC_CARTPOLE_TH_LIMIT (12.0 * 2.0 * SAC_PI / 360.0)
#define SAC_CARTPOLE_RESET_HALF_SIDE 0.05

// The observation of a state, in fp32
__host__ __device__ inline void cartpole_obs(const double s[4], float obs[SAC_CARTPOLE_OBS_DIM]) {
  for (int k = 0; k < SAC_CARTPOLE_OBS_DIM; ++k) obs[k] = (float)s[k];
}

// One Euler step from s with action a: the new state in place, its observation
// in fp32; returns terminated (the new state is outside a limit).  The reward
// is 1.0 on every step, the failing one included.
__host__ __device__ inline bool cartpole_dynamics(double s[4], float a, double action_low, double action_high,
                                                  double dt, float obs[SAC_CARTPOLE_OBS_DIM]) {
  const double u = (double)clip_f32(a, (float)action_low, (float)action_high);
  const double x = s[0], xdot = s[1], th = s[2], thdot = s[3];
  const double F = SAC_CARTPOLE_FORCE_MAG * u, c = cos(th), sn = sin(th);
  const double M = SAC_CARTPOLE_M_CART + SAC_CARTPOLE_M_POLE;
  const double temp = (F + SAC_CARTPOLE_M_POLE * SAC_CARTPOLE_HALF_LEN * thdot * thdot * sn) / M;
  const double thacc =
      (SAC_CARTPOLE_G * sn - c * temp) / (SAC_CARTPOLE_HALF_LEN * (4.0 / 3.0 - SAC_CARTPOLE_M_POLE * c * c / M));
  const double xacc = temp - SAC_CARTPOLE_M_POLE * SAC_CARTPOLE_HALF_LEN * thacc * c / M;
  s[0] = x + dt * xdot;
  s[1] = xdot + dt * xacc;
  s[2] = th + dt * thdot;
  s[3] = thdot + dt * thacc;
  cartpole_obs(s, obs);
  return fabs(s[0]) > SAC_CARTPOLE_X_LIMIT || fabs(s[2]) > SAC_CARTPOLE_TH_LIMIT;
}

// The reset draw of env row `row` at vector step t: the four uniforms of the
// row's ENV_WHICH_RESET block 0 give x, xdot, th, thdot in [-0.05, 0.05).
__host__ __device__ inline void cartpole_reset_draw(uint64_t seed, uint64_t t, uint32_t row, double s[4]) {
  float u[4];
  philox_uniform4(seed, t, row, ENV_WHICH_RESET, 0, u);
  for (int k = 0; k < 4; ++k) s[k] = SAC_CARTPOLE_RESET_HALF_SIDE * (2.0 * (double)u[k] - 1.0);
}

// Row i's state in the component-major blocks ev.pos [2][N] (x, th) and ev.vel [2][N] (xdot, thdot)
__device__ __forceinline__ void cartpole_load(const sac_envs& ev, int i, double s[4]) {
  const size_t n = (size_t)ev.cfg.num_envs;
  s[0] = ev.pos[i];
  s[1] = ev.vel[i];
  s[2] = ev.pos[n + i];
  s[3] = ev.vel[n + i];
}
__device__ __forceinline__ void cartpole_store(const sac_envs& ev, int i, const double s[4]) {
  const size_t n = (size_t)ev.cfg.num_envs;
  ev.pos[i] = s[0];
  ev.vel[i] = s[1];
  ev.pos[n + i] = s[2];
  ev.vel[n + i] = s[3];
}

struct EnvOut {
  double reward;  // as the host class returns it (probe 1's fp32 reward widened, as float(r) does)
  bool terminated, truncated;
};

// The pendulum's step of env_step: state (th, thdot) in ev.pos / ev.vel, three
// observation components, no termination, truncation at max_steps; a truncated
// row takes its reset draw of this t as its current state and observation.
// Inlined: a noinline call costs the rollout kernels 192 B of scratch per lane
// (profiles/pendulum_rollout_resources.txt).
__device__ __forceinline__ EnvOut env_step_pendulum(const sac_envs& ev, int i, uint64_t t, float action,
                                                    float* final_obs) {
  const sac_env_config& c = ev.cfg;
  const int step = ev.step[i] + 1;
  float* cur = ev.obs + (size_t)i * SAC_PENDULUM_OBS_DIM;
  double th = ev.pos[i], thdot = ev.vel[i];
  float fo[SAC_PENDULUM_OBS_DIM];
  EnvOut o;
  o.reward = pendulum_dynamics(th, thdot, action, c.action_low, c.action_high, c.dt, fo);
  o.terminated = false;
  o.truncated = step >= c.max_steps;
  if (final_obs)
    for (int k = 0; k < SAC_PENDULUM_OBS_DIM; ++k) final_obs[k] = fo[k];
  if (o.truncated) {
    pendulum_reset_draw(c.seed, t, (uint32_t)i, th, thdot);
    pendulum_obs(th, thdot, fo);
  }
  for (int k = 0; k < SAC_PENDULUM_OBS_DIM; ++k) cur[k] = fo[k];
  ev.step[i] = o.truncated ? 0 : step;
  ev.pos[i] = th;
  ev.vel[i] = thdot;
  return o;
}

// The reacher's step of env_step: as the pendulum's, with two action components, ten observation
// components and the state of reacher_load.
__device__ __forceinline__ EnvOut env_step_reacher(const sac_envs& ev, int i, uint64_t t, float a0, float a1,
                                                   float* final_obs) {
  const sac_env_config& c = ev.cfg;
  const int step = ev.step[i] + 1;
  float* cur = ev.obs + (size_t)i * SAC_REACHER_OBS_DIM;
  double s[6];
  reacher_load(ev, i, s);
  float fo[SAC_REACHER_OBS_DIM];
  EnvOut o;
  o.reward = reacher_dynamics(s, a0, a1, c.action_low, c.action_high, c.dt, fo);
  o.terminated = false;
  o.truncated = step >= c.max_steps;
  if (final_obs)
    for (int k = 0; k < SAC_REACHER_OBS_DIM; ++k) final_obs[k] = fo[k];
  if (o.truncated) {
    reacher_reset_draw(c.seed, t, (uint32_t)i, s);
    reacher_obs(s, fo);
  }
  for (int k = 0; k < SAC_REACHER_OBS_DIM; ++k) cur[k] = fo[k];
  ev.step[i] = o.truncated ? 0 : step;
  reacher_store(ev, i, s);
  return o;
}

// The cart-pole's step of env_step: the one kind whose rows end by failure, each at its own step;
// terminated and truncated are independent, and a row that ended either way takes its reset draw of
// this t.
__device__ __forceinline__ EnvOut env_step_cartpole(const sac_envs& ev, int i, uint64_t t, float action,
                                                    float* final_obs) {
  const sac_env_config& c = ev.cfg;
  const int step = ev.step[i] + 1;
  float* cur = ev.obs + (size_t)i * SAC_CARTPOLE_OBS_DIM;
  double s[4];
  cartpole_load(ev, i, s);
  float fo[SAC_CARTPOLE_OBS_DIM];
  EnvOut o;
  o.terminated = cartpole_dynamics(s, action, c.action_low, c.action_high, c.dt, fo);
  o.reward = 1.0;
  o.truncated = step >= c.max_steps;
  const bool done = o.terminated || o.truncated;
  if (final_obs)
    for (int k = 0; k < SAC_CARTPOLE_OBS_DIM; ++k) final_obs[k] = fo[k];
  if (done) {
    cartpole_reset_draw(c.seed, t, (uint32_t)i, s);
    cartpole_obs(s, fo);
  }
  for (int k = 0; k < SAC_CARTPOLE_OBS_DIM; ++k) cur[k] = fo[k];
  ev.step[i] = done ? 0 : step;
  cartpole_store(ev, i, s);
  return o;
}

// One step of environment row i at vector step t with the action's first
// component `action` (and its second, a1, for the one kind that takes two).
// Writes the observation stepped to into final_obs[obs_dim] (unless NULL), the
// environment's new current observation (the reset observation where the
// episode ended) into ev.obs, and its step counter / position.
// KC is the kind class (EnvClass), decided by the launch: the rollout kernels are
// compiled once per class, so the probes' kernels hold none of the pendulum's, the
// reacher's or the cart-pole's code (behind a run-time branch the pendulum cost them 16 more
// spilled SGPRs and 1-2 % per launch).
template <int KC>
__device__ __forceinline__ EnvOut env_step(const sac_envs& ev, int i, uint64_t t, float action, float a1,
                                           float* final_obs) {
  if (KC == ENV_CLASS_PENDULUM) return env_step_pendulum(ev, i, t, action, final_obs);
  if (KC == ENV_CLASS_REACHER) return env_step_reacher(ev, i, t, action, a1, final_obs);
  if (KC == ENV_CLASS_CARTPOLE) return env_step_cartpole(ev, i, t, action, final_obs);
  const sac_env_config& c = ev.cfg;
  const int O = c.obs_dim;
  const int step = ev.step[i] + 1;
  float* cur = ev.obs + (size_t)i * O;
  EnvOut o;
  o.terminated = o.truncated = false;
  float fo = 0.f, ro = 0.f;  // observation stepped to / after a reset (the probes with one observation)
  double pos = 0.0;
  switch (c.kind) {
    case SAC_ENV_CONSTANT_REWARD:
      o.reward = c.reward;
      o.terminated = step >= c.max_steps;
      break;
    case SAC_ENV_QUADRATIC_ACTION: {
      // np.float32 - Python float stays fp32 (the float is a weak scalar).  d * d is the correctly
      // rounded square; numpy's scalar ** 2 is powf and misses it by an ulp for ~0.07 % of arguments.
      const float a = clip_f32(action, (float)c.action_low, (float)c.action_high);
      const float d = a - (float)c.target;
      o.reward = (double)(-(d * d));
      o.terminated = step >= c.max_steps;
      break;
    }
    case SAC_ENV_RANDOM_OBS:
      o.reward = fabs((double)action) <= c.threshold ? 1.0 : -1.0;
      o.terminated = step >= c.max_steps;
      break;
    default: {  // SAC_ENV_POINT_MASS
      const double a = (double)clip_f32(action, (float)c.action_low, (float)c.action_high);
      pos = ev.pos[i] + a * c.dt;
      const bool reached = fabs(pos - c.goal_pos) <= c.goal_tolerance;
      o.reward = reached ? c.step_penalty + c.goal_reward : c.step_penalty;
      o.terminated = reached;
      o.truncated = step >= c.max_steps;
      fo = (float)pos;
      ro = (float)c.start_pos;
      break;
    }
  }
  const bool done = o.terminated || o.truncated;
  if (c.kind == SAC_ENV_RANDOM_OBS) {
    for (int b = 0; 4 * b < O; ++b) {
      float u[4], v[4] = {0.f, 0.f, 0.f, 0.f};
      philox_uniform4(c.seed, t, (uint32_t)i, ENV_WHICH_STEP, (uint32_t)b, u);
      if (done) philox_uniform4(c.seed, t, (uint32_t)i, ENV_WHICH_RESET, (uint32_t)b, v);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int j = 4 * b + k;
        if (j >= O) break;
        const float f = env_uniform_obs(u[k]);
        if (final_obs) final_obs[j] = f;
        cur[j] = done ? env_uniform_obs(v[k]) : f;
      }
    }
  } else {
    if (final_obs) final_obs[0] = fo;
    cur[0] = done ? ro : fo;
  }
  ev.step[i] = done ? 0 : step;
  if (c.kind == SAC_ENV_POINT_MASS) ev.pos[i] = done ? c.start_pos : pos;
  return o;
}

// The loop's episode bookkeeping (agent.py run_vectorized_training_loop:
// ep_ret += rewards in float64, ep_len += 1, both zeroed where the episode
// ended) and this step's cell of the episode ring.
__device__ __forceinline__ void env_account(const sac_envs& ev, int i, uint64_t t, const EnvOut& o) {
  const bool done = o.terminated || o.truncated;
  const double ret = ev.ep_return[i] + o.reward;
  const int len = ev.ep_length[i] + 1;
  if (ev.episodes) {
    sac_env_episode* cell = ev.episodes + (size_t)(t % (uint64_t)ev.ring_steps) * ev.cfg.num_envs + i;
    cell->ret = ret;
    cell->length = len;
    cell->ended = done ? 1 : 0;
  }
  ev.ep_return[i] = done ? 0.0 : ret;
  ev.ep_length[i] = done ? 0 : len;
}

__global__ void sac_envs_reset_kernel(sac_envs ev, uint64_t seed) {
  const sac_env_config& c = ev.cfg;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c.num_envs) return;
  const int O = c.obs_dim;
  float* cur = ev.obs + (size_t)i * O;
  if (c.kind == SAC_ENV_RANDOM_OBS) {
    for (int b = 0; 4 * b < O; ++b) {
      float u[4];
      philox_uniform4(seed, 0, (uint32_t)i, ENV_WHICH_RESET, (uint32_t)b, u);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (4 * b + k < O) cur[4 * b + k] = env_uniform_obs(u[k]);
    }
  } else if (c.kind != SAC_ENV_PENDULUM && c.kind != SAC_ENV_REACHER && c.kind != SAC_ENV_CARTPOLE) {
    cur[0] = c.kind == SAC_ENV_POINT_MASS ? (float)c.start_pos : 0.f;
  }
  ev.step[i] = 0;
  ev.ep_length[i] = 0;
  if (c.kind == SAC_ENV_CARTPOLE) {
    double s[4];
    cartpole_reset_draw(seed, 0, (uint32_t)i, s);
    cartpole_obs(s, cur);
    cartpole_store(ev, i, s);
  } else if (c.kind == SAC_ENV_REACHER) {
    double s[6];
    reacher_reset_draw(seed, 0, (uint32_t)i, s);
    reacher_obs(s, cur);
    reacher_store(ev, i, s);
  } else if (c.kind == SAC_ENV_PENDULUM) {
    double th, thdot;
    pendulum_reset_draw(seed, 0, (uint32_t)i, th, thdot);
    pendulum_obs(th, thdot, cur);
    ev.pos[i] = th;
    ev.vel[i] = thdot;
  } else {
    ev.pos[i] = c.kind == SAC_ENV_POINT_MASS ? c.start_pos : 0.0;
  }
  ev.ep_return[i] = 0.0;
}

__global__ void sac_envs_step_kernel(sac_envs ev, const float* __restrict__ actions, uint64_t t,
                                     float* __restrict__ obs, float* __restrict__ final_obs,
                                     float* __restrict__ reward, uint8_t* __restrict__ terminated,
                                     uint8_t* __restrict__ truncated) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ev.cfg.num_envs) return;
  const int O = ev.cfg.obs_dim;
  const int A = env_act_dim(ev.cfg.kind);
  const float a = actions[(size_t)i * A];
  float* fin = final_obs + (size_t)i * O;
  EnvOut o;
  if (ev.cfg.kind == SAC_ENV_REACHER)
    o = env_step<ENV_CLASS_REACHER>(ev, i, t, a, actions[(size_t)i * A + 1], fin);
  else if (ev.cfg.kind == SAC_ENV_CARTPOLE)
    o = env_step<ENV_CLASS_CARTPOLE>(ev, i, t, a, 0.f, fin);
  else if (ev.cfg.kind == SAC_ENV_PENDULUM)
    o = env_step<ENV_CLASS_PENDULUM>(ev, i, t, a, 0.f, fin);
  else
    o = env_step<ENV_CLASS_PROBES>(ev, i, t, a, 0.f, fin);
  env_account(ev, i, t, o);
  for (int k = 0; k < O; ++k) obs[(size_t)i * O + k] = ev.obs[(size_t)i * O + k];
  reward[i] = (float)o.reward;
  terminated[i] = o.terminated ? 1 : 0;
  truncated[i] = o.truncated ? 1 : 0;
}

// The fused step of one workgroup (SAC_ROWS environments) at RNG step t, its
// rows going to ring slots (pos + i) % capacity.  new_size / new_pos: the
// replay's (size, write slot) after this step, as sac_replay_push computes
// them.  Both kernels below are this body; they differ in where (pos, t) come
// from.
template <typename T, int KC>
__device__ __forceinline__ void rollout_step_body(const EngineDev* __restrict__ Ep, const sac_envs& ev,
                                                  const sac_replay& rb, int64_t pos, int64_t new_size, int64_t new_pos,
                                                  uint64_t t, int deterministic, int store) {
  PREFETCH_ARG(Ep);
  const AS_C EngineDev& E = *(const AS_C EngineDev*)Ep;
  extern __shared__ float lds_raw[];
  lf* lds = (lf*)lds_raw;
  constexpr int R = SAC_ROWS;
  const int tid = threadIdx.x, O = E.O, A = E.A, ld = E.ld, ldo = E.ldo;
  const int n = ev.cfg.num_envs;
  const int r0 = blockIdx.x * R;
  const int nvalid = min(R, n - r0);
  const AS_G float* obs = GPC(float, ev.obs);
  lf* Xb = lds + E.o_X;
  lf* Yb = lds + E.o_Y;
  lf* outB = lds + E.o_out;
  lf* outP = lds + E.o_outp;
  const AS_C NetDev& pi = E.net[NET_PI];
  const int Kp0 = pi.l[0].Kp;
  for (int i = tid; i < R * Kp0; i += SAC_THREADS) {
    const int r = i / Kp0, k = i % Kp0;
    Xb[r * ld + k] = (k < O && r < nvalid) ? obs[(size_t)(r0 + r) * O + k] : 0.f;
  }
  __syncthreads();
  mlp_forward<T, R>(pi, Xb, Yb, ld, outP, outB, ldo, E.o_P1, E.ldp1, lds, false, false, 0, 0, 0);
  // every read of ev.obs above is behind mlp_forward's barriers: row owners may now overwrite their rows
  if (tid < nvalid) {
    const int i = r0 + tid;
    const lf* o = outB + tid * ldo;
    const float lo = E.ls_min, hi = E.ls_max, scale = E.scale;
    const RowStrides rs = row_strides(rb.row_stride, O, A);
    const int64_t slot = (pos + i) % rb.capacity;
    if (store)
      for (int k = 0; k < O; ++k) rb.obs[slot * rs.obs + k] = ev.obs[(size_t)i * O + k];
    float a0 = 0.f, a1 = 0.f;  // what the environment takes: registers, not a re-read of the replay row
    for (int p = 0; 2 * p < A; ++p) {
      float e2[2] = {0.f, 0.f};
      if (!deterministic) philox_normal2(E.seed, t, (uint32_t)i, ENV_WHICH_NOISE, (uint32_t)p, e2[0], e2[1]);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int j = 2 * p + q;
        if (j >= A) break;
        float a;
        if (deterministic) {
          a = tanhf(o[j]) * scale;
        } else {  // the head arithmetic of sac_policy_act_kernel
          const float mu = o[j], lsr = o[A + j], e = e2[q];
          const float ls = lsr < lo ? lo : (lsr > hi ? hi : lsr);
          const float sd = expf(ls);
          const float z = mu + e * sd;
          a = tanhf(z) * scale;
        }
        if (j == 0) a0 = a;
        if (KC == ENV_CLASS_REACHER && j == 1) a1 = a;
        if (store) rb.act[slot * rs.act + j] = a;
      }
    }
    const EnvOut eo = env_step<KC>(ev, i, t, a0, a1, store ? rb.next_obs + slot * rs.obs : nullptr);
    env_account(ev, i, t, eo);
    if (store) {
      rb.rew[slot * rs.one] = (float)eo.reward;
      rb.done[slot * rs.one] = (eo.terminated || eo.truncated) ? 1.f : 0.f;
    }
  }
  if (store && blockIdx.x == 0 && tid == 0) {  // as replay_push_kernel
    rb.state[0] = new_size;
    rb.state[1] = new_pos;
    rb.state[2] += 1;  // push generation: a batch phase C staged before this step is stale
  }
}

// One workgroup per SAC_ROWS environments; (size, pos, t) are host arguments,
// new_size / new_pos computed by the host as sac_replay_push does.  KC:
// env_class(ev.cfg.kind) (the host picks the instantiation).
template <typename T, int KC>
__global__ void __launch_bounds__(SAC_THREADS) sac_rollout_step_kernel(const EngineDev* __restrict__ Ep, sac_envs ev,
                                                                      sac_replay rb, int64_t pos, int64_t new_size,
                                                                      int64_t new_pos, uint64_t t, int deterministic,
                                                                      int store) {
  rollout_step_body<T, KC>(Ep, ev, rb, pos, new_size, new_pos, t, deterministic, store);
}

// The same step with the loop cursor on the device (include/sac_engine.h
// sac_rollout_step_dev): every workgroup reads {size, pos, t} from `cur`, one
// slot of the caller's cursor[2][4], and block 0's thread 0 writes the
// advanced cursor to `nxt`, the other slot.  No workgroup reads a word another
// workgroup of the launch writes (cur is only read, nxt and rb.state only
// written), so nothing depends on the order workgroups run in and the launch
// can be replayed from a hipGraph with the slots alternating.  A cursor outside
// the ring (never seeded) stores nothing and does not advance.
template <typename T, int KC>
__global__ void __launch_bounds__(SAC_THREADS) sac_rollout_step_dev_kernel(const EngineDev* __restrict__ Ep, sac_envs ev,
                                                                          sac_replay rb,
                                                                          const int64_t* __restrict__ cur,
                                                                          int64_t* __restrict__ nxt, int deterministic,
                                                                          int store) {
  const int64_t size = cur[0], pos = cur[1], cap = rb.capacity, n = ev.cfg.num_envs;
  const uint64_t t = (uint64_t)cur[2] + 1;  // the k-th step (k = 0, 1, ...) is RNG step k + 1
  if (size < 0 || size > cap || pos < 0 || pos >= cap) return;
  const int64_t new_size = store ? (size + n < cap ? size + n : cap) : size;
  const int64_t new_pos = store ? (pos + n) % cap : pos;
  rollout_step_body<T, KC>(Ep, ev, rb, pos, new_size, new_pos, t, deterministic, store);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    nxt[0] = new_size;
    nxt[1] = new_pos;
    nxt[2] = (int64_t)t;
    nxt[3] = 0;
  }
}
