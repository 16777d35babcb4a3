// sac_envs.h — the environments of sac/envs.py (the probes) and sac/control_envs.py
// (the control tasks) on the device, and the fused rollout step (act -> step ->
// store in one launch).
//
//   class (EnvClass)       kinds                    described by
//   ENV_CLASS_PROBES       SAC_ENV_* 0..3           the switch in env_step (one class on purpose)
//   ENV_CLASS_PENDULUM     SAC_ENV_PENDULUM         EnvTask<ENV_CLASS_PENDULUM>
//   ENV_CLASS_REACHER      SAC_ENV_REACHER          EnvTask<ENV_CLASS_REACHER>
//   ENV_CLASS_CARTPOLE     SAC_ENV_CARTPOLE         EnvTask<ENV_CLASS_CARTPOLE>
//
//   * EnvTask<KC>: everything the kernels know about one control task: its widths,
//     where each float64 state component lives, its observation, dynamics and
//     reset draw (host-callable: the C ABI exports the same inline code);
//   * task_load / task_store / env_step_task / task_reset: the code every task
//     shares, written once over an EnvTask;
//   * env_step<KC>: ONE statement of the environments' dynamics, with the semantics
//     sac.vector_env.SyncVectorEnv gives the host classes (same-step autoreset;
//     the transition is (obs, action, reward, final_obs, terminated | truncated)).
//     Whatever the host classes keep as a Python float is a double here, so the
//     fp32-rounded observations and rewards are the host's bit for bit;
//   * with_env_class: the one map from a kind to its class;
//   * sac_envs_step_kernel: N environments stepped with the caller's actions;
//   * sac_rollout_step_kernel<T, KC>: sibling of sac_policy_act_kernel<T>
//     (same workgroup shape, LDS layout and mlp_forward call); the thread that
//     owns environment row i samples its action, steps the environment and
//     writes the transition into the replay ring.  Compiled once per class KC, so
//     that no class carries another's code; the host picks by the environments' kind;
//   * sac_rollout_step_dev_kernel<T, KC>: the same body with (size, pos,
//     t) read from a two-slot cursor in device memory, so whole loop iterations
//     replay from one hipGraph (sac_engine_loop_graph);
//   * rollout_row_tail<KC>: what a row owner does once it holds its action (copy
//     the observation, store the action, step, account, reward and done word),
//     shared by the fused body and the uniform kernels;
//   * sac_rollout_uniform_kernel<KC> / sac_rollout_uniform_dev_kernel<KC>: the
//     rollout step with uniform-random actions (train.random_steps): one thread
//     per environment row, no policy forward, no LDS.
//
// State is caller-owned global memory (include/sac_engine.h sac_envs).  Every
// environment row is read and written by exactly one thread of one launch, and
// every episode-ring cell by its own row: no atomics, no hand-offs, nothing
// depends on the order workgroups run in.
#pragma once
#include <type_traits>

#include "../../include/sac_engine.h"
#include "sac_phases.h"

// Action components an environment of `kind` takes
__host__ __device__ inline int env_act_dim(int kind) { return SAC_ENV_ACT_DIM(kind); }
enum EnvClass { ENV_CLASS_PROBES = 0, ENV_CLASS_PENDULUM = 1, ENV_CLASS_REACHER = 2, ENV_CLASS_CARTPOLE = 3 };
// Philox `which` values of the rollout (0 / 1 are the training draws)
#define ENV_WHICH_NOISE 2u  // action noise of a rollout step, key = engine seed
#define ENV_WHICH_STEP 3u   // observation an environment steps to at t, key = env seed
#define ENV_WHICH_RESET 4u  // its reset observation at t
#define ENV_WHICH_UNIFORM 5u  // uniform warm-up actions of a rollout step (train.random_steps), key = engine seed

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

// The uniform warm-up action components 0..n-1 of env row `row` at RNG step t
// (DESIGN.md §3.13): component j is word j % 4 of the row's ENV_WHICH_UNIFORM
// block j / 4, a = scale * (2u - 1) in [-scale, scale).  2u - 1 is exact, the
// product is the one rounding.  Host-callable: sac_uniform_actions_host is this.
__host__ __device__ inline void uniform_actions_row(uint64_t seed, uint64_t t, uint32_t row, float scale, int n,
                                                    float* a) {
  for (int b = 0; 4 * b < n; ++b) {
    float u[4];
    philox_uniform4(seed, t, row, ENV_WHICH_UNIFORM, (uint32_t)b, u);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (4 * b + k < n) a[4 * b + k] = scale * env_uniform_obs(u[k]);
  }
}

// np.clip on float32: min(max(x, lo), hi) with NaN passed through
__host__ __device__ inline float clip_f32(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

struct EnvOut {
  double reward;  // as the host class returns it (probe 1's fp32 reward widened, as float(r) does)
  bool terminated, truncated;
};

// ---- The control tasks -------------------------------------------------------
// EnvTask<KC> describes the task of class KC:
//   KIND, NAME           its sac_env_kind and that enumerator's spelling;
//   OBS, ACT             observation and action components;
//   NS                   float64 state components, in the order of the host class's .state;
//   POS_ROWS, VEL_ROWS   rows of the component-major blocks sac_envs.pos [POS_ROWS][N] and .vel [VEL_ROWS][N];
//   home(k)              where state component k lives: a row of .vel or of .pos;
//   obs(s, o)            the fp32 observation of a state;
//   dynamics(s, a, cfg, obs_out, out)   one step from s with actions a[ACT]: the new state in place, its
//                        observation, and out.reward / out.terminated;
//   reset_draw(seed, t, row, s)   the state row `row` restarts from at vector step t, from the four uniforms
//                        of the row's ENV_WHICH_RESET block 0.
// Every operation is the host class's, in its order (the library is built with
// -ffp-contract=off: no fused multiply-adds).
template <int KC>
struct EnvTask;
struct EnvHome {
  int vel, row;  // row `row` of sac_envs.vel (vel = 1) or of sac_envs.pos (vel = 0)
};
#define SAC_PI 3.141592653589793

// The probes share one class and have no description; their one action component is all the rollout asks.
template <>
struct EnvTask<ENV_CLASS_PROBES> {
  static constexpr int ACT = 1;
};

// Pendulum swing-up (sac/control_envs.py PendulumEnv).  State (th, thdot); g =
// 10, m = l = 1, so 3 g / (2 l) = 15 and 3 / (m l^2) = 3 exactly.
template <>
struct EnvTask<ENV_CLASS_PENDULUM> {
  static constexpr int KIND = SAC_ENV_PENDULUM, OBS = 3, ACT = 1, NS = 2, POS_ROWS = 1, VEL_ROWS = 1;
  static constexpr const char* NAME = "SAC_ENV_PENDULUM";
  static constexpr double MAX_SPEED = 8.0;
  static constexpr EnvHome home(int k) { return EnvHome{k, 0}; }

  // Python's ((th + pi) % (2 pi)) - pi: the angle in [-pi, pi)
  __host__ __device__ static inline double angle(double th) {
    double an = fmod(th + SAC_PI, 2.0 * SAC_PI);
    if (an < 0.0) an += 2.0 * SAC_PI;
    return an - SAC_PI;
  }
  __host__ __device__ static inline void obs(const double s[NS], float o[OBS]) {
    o[0] = (float)cos(s[0]);
    o[1] = (float)sin(s[0]);
    o[2] = (float)s[1];
  }
  // The reward is the PRE-step state's; never terminated.
  __host__ __device__ static inline void dynamics(double s[NS], const float a[ACT], const sac_env_config& c,
                                                  float obs_out[OBS], EnvOut& out) {
    const double u = (double)clip_f32(a[0], (float)c.action_low, (float)c.action_high);
    const double an = angle(s[0]);
    out.reward = -(an * an + 0.1 * s[1] * s[1] + 0.001 * u * u);
    out.terminated = false;
    double v = s[1] + (15.0 * sin(s[0]) + 3.0 * u) * c.dt;
    v = v < -MAX_SPEED ? -MAX_SPEED : (v > MAX_SPEED ? MAX_SPEED : v);
    s[0] = s[0] + v * c.dt;
    s[1] = v;
    obs(s, obs_out);
  }
  // th ~ U[-pi, pi), thdot ~ U[-1, 1) from the block's first two uniforms
  __host__ __device__ static inline void reset_draw(uint64_t seed, uint64_t t, uint32_t row, double s[NS]) {
    float u[4];
    philox_uniform4(seed, t, row, ENV_WHICH_RESET, 0, u);
    s[0] = SAC_PI * (2.0 * (double)u[0] - 1.0);
    s[1] = 2.0 * (double)u[1] - 1.0;
  }
};

// Two-link reacher (sac/control_envs.py ReacherEnv).  State (th1, th2, w1, w2,
// tx, ty).  Sine and cosine enter the reward and the observation only, never the
// state: the state trajectory is the host's bit for bit whatever library they
// come from.
template <>
struct EnvTask<ENV_CLASS_REACHER> {
  static constexpr int KIND = SAC_ENV_REACHER, OBS = 10, ACT = 2, NS = 6, POS_ROWS = 4, VEL_ROWS = 2;
  static constexpr const char* NAME = "SAC_ENV_REACHER";
  static constexpr double L1 = 0.1, L2 = 0.1, GAIN = 10.0, DAMP = 2.0, CTRL_COST = 0.1, TARGET_HALF_SIDE = 0.14;
  // pos: th1, th2, tx, ty; vel: w1, w2
  static constexpr EnvHome home(int k) { return k < 2 ? EnvHome{0, k} : k < 4 ? EnvHome{1, k - 2} : EnvHome{0, k - 2}; }

  // Fingertip minus target
  __host__ __device__ static inline void tip(const double s[NS], double& dx, double& dy) {
    dx = (L1 * cos(s[0]) + L2 * cos(s[0] + s[1])) - s[4];
    dy = (L1 * sin(s[0]) + L2 * sin(s[0] + s[1])) - s[5];
  }
  __host__ __device__ static inline void obs(const double s[NS], float o[OBS]) {
    double dx, dy;
    tip(s, dx, dy);
    o[0] = (float)cos(s[0]);
    o[1] = (float)cos(s[1]);
    o[2] = (float)sin(s[0]);
    o[3] = (float)sin(s[1]);
    o[4] = (float)s[4];
    o[5] = (float)s[5];
    o[6] = (float)s[2];
    o[7] = (float)s[3];
    o[8] = (float)dx;
    o[9] = (float)dy;
  }
  // The reward is the PRE-step state's; never terminated.
  __host__ __device__ static inline void dynamics(double s[NS], const float a[ACT], const sac_env_config& c,
                                                  float obs_out[OBS], EnvOut& out) {
    const double u0 = (double)clip_f32(a[0], (float)c.action_low, (float)c.action_high);
    const double u1 = (double)clip_f32(a[1], (float)c.action_low, (float)c.action_high);
    double dx, dy;
    tip(s, dx, dy);
    out.reward = -sqrt(dx * dx + dy * dy) - CTRL_COST * (u0 * u0 + u1 * u1);
    out.terminated = false;
    s[2] = s[2] + (GAIN * u0 - DAMP * s[2]) * c.dt;
    s[3] = s[3] + (GAIN * u1 - DAMP * s[3]) * c.dt;
    s[0] = s[0] + s[2] * c.dt;
    s[1] = s[1] + s[3] * c.dt;
    obs(s, obs_out);
  }
  // The target in the square of half side 0.14, both angles in [-pi, pi); the arm starts at rest.
  __host__ __device__ static inline void reset_draw(uint64_t seed, uint64_t t, uint32_t row, double s[NS]) {
    float u[4];
    philox_uniform4(seed, t, row, ENV_WHICH_RESET, 0, u);
    s[4] = TARGET_HALF_SIDE * (2.0 * (double)u[0] - 1.0);
    s[5] = TARGET_HALF_SIDE * (2.0 * (double)u[1] - 1.0);
    s[0] = SAC_PI * (2.0 * (double)u[2] - 1.0);
    s[1] = SAC_PI * (2.0 * (double)u[3] - 1.0);
    s[2] = 0.0;
    s[3] = 0.0;
  }
};

// Balancing cart-pole (sac/control_envs.py CartPoleEnv).  State (x, xdot, th,
// thdot).  sin th and cos th feed back into the state, so the trajectory follows
// the host's to the library's few float64 ulps, not to the bit.
template <>
struct EnvTask<ENV_CLASS_CARTPOLE> {
  static constexpr int KIND = SAC_ENV_CARTPOLE, OBS = 4, ACT = 1, NS = 4, POS_ROWS = 2, VEL_ROWS = 2;
  static constexpr const char* NAME = "SAC_ENV_CARTPOLE";
  static constexpr double G = 9.8, M_CART = 1.0, M_POLE = 0.1, HALF_LEN = 0.5, FORCE_MAG = 10.0, X_LIMIT = 2.4,
                          TH_LIMIT = 12.0 * 2.0 * SAC_PI / 360.0, RESET_HALF_SIDE = 0.05;
  // pos: x, th; vel: xdot, thdot
  static constexpr EnvHome home(int k) { return EnvHome{k & 1, k >> 1}; }

  __host__ __device__ static inline void obs(const double s[NS], float o[OBS]) {
    for (int k = 0; k < OBS; ++k) o[k] = (float)s[k];
  }
  // One Euler step; terminated: the new state is outside a limit.  The reward
  // is 1.0 on every step, the failing one included.
  __host__ __device__ static inline void dynamics(double s[NS], const float a[ACT], const sac_env_config& cfg,
                                                  float obs_out[OBS], EnvOut& out) {
    const double dt = cfg.dt;
    const double u = (double)clip_f32(a[0], (float)cfg.action_low, (float)cfg.action_high);
    const double x = s[0], xdot = s[1], th = s[2], thdot = s[3];
    const double F = FORCE_MAG * u, c = cos(th), sn = sin(th);
    const double M = M_CART + M_POLE;
    const double temp = (F + M_POLE * HALF_LEN * thdot * thdot * sn) / M;
    const double thacc = (G * sn - c * temp) / (HALF_LEN * (4.0 / 3.0 - M_POLE * c * c / M));
    const double xacc = temp - M_POLE * HALF_LEN * thacc * c / M;
    s[0] = x + dt * xdot;
    s[1] = xdot + dt * xacc;
    s[2] = th + dt * thdot;
    s[3] = thdot + dt * thacc;
    obs(s, obs_out);
    out.terminated = fabs(s[0]) > X_LIMIT || fabs(s[2]) > TH_LIMIT;
    out.reward = 1.0;
  }
  // x, xdot, th, thdot in [-0.05, 0.05)
  __host__ __device__ static inline void reset_draw(uint64_t seed, uint64_t t, uint32_t row, double s[NS]) {
    float u[4];
    philox_uniform4(seed, t, row, ENV_WHICH_RESET, 0, u);
    for (int k = 0; k < 4; ++k) s[k] = RESET_HALF_SIDE * (2.0 * (double)u[k] - 1.0);
  }
};

// Rows of .vel (vel = 1) or .pos (vel = 0) the map of a task names: one past its highest
template <typename Task>
constexpr int task_rows(int vel) {
  int rows = 0;
  for (int k = 0; k < Task::NS; ++k)
    if (Task::home(k).vel == vel && Task::home(k).row >= rows) rows = Task::home(k).row + 1;
  return rows;
}
// Every description agrees with the width table of include/sac_engine.h and with its own map
template <typename Task>
constexpr bool task_matches_header() {
  return Task::OBS == SAC_ENV_OBS_DIM(Task::KIND) && Task::ACT == SAC_ENV_ACT_DIM(Task::KIND) &&
         Task::POS_ROWS == SAC_ENV_POS_ROWS(Task::KIND) && Task::VEL_ROWS == SAC_ENV_VEL_ROWS(Task::KIND) &&
         Task::POS_ROWS == task_rows<Task>(0) && Task::VEL_ROWS == task_rows<Task>(1);
}
static_assert(task_matches_header<EnvTask<ENV_CLASS_PENDULUM>>(), "the pendulum's widths");
static_assert(task_matches_header<EnvTask<ENV_CLASS_REACHER>>(), "the reacher's widths");
static_assert(task_matches_header<EnvTask<ENV_CLASS_CARTPOLE>>(), "the cart-pole's widths");

// The one map from a kind to its class: f(std::integral_constant<int, KC>) with KC the class of `kind`
// (whatever is no task's kind is a probe's).
template <typename F>
__host__ __device__ __forceinline__ decltype(auto) with_env_class(int kind, F&& f) {
  if (kind == SAC_ENV_PENDULUM) return f(std::integral_constant<int, ENV_CLASS_PENDULUM>{});
  if (kind == SAC_ENV_REACHER) return f(std::integral_constant<int, ENV_CLASS_REACHER>{});
  if (kind == SAC_ENV_CARTPOLE) return f(std::integral_constant<int, ENV_CLASS_CARTPOLE>{});
  return f(std::integral_constant<int, ENV_CLASS_PROBES>{});
}
// One kind of every class, for what must touch every instantiation
constexpr int ENV_CLASS_KINDS[] = {SAC_ENV_POINT_MASS, SAC_ENV_PENDULUM, SAC_ENV_REACHER, SAC_ENV_CARTPOLE};

// Row i's state from / to the component-major blocks ev.pos and ev.vel, in state component order
template <typename Task>
__device__ __forceinline__ void task_load(const sac_envs& ev, int i, double s[Task::NS]) {
  const size_t n = (size_t)ev.cfg.num_envs;
#pragma unroll
  for (int k = 0; k < Task::NS; ++k) s[k] = (Task::home(k).vel ? ev.vel : ev.pos)[Task::home(k).row * n + i];
}
template <typename Task>
__device__ __forceinline__ void task_store(const sac_envs& ev, int i, const double s[Task::NS]) {
  const size_t n = (size_t)ev.cfg.num_envs;
#pragma unroll
  for (int k = 0; k < Task::NS; ++k) (Task::home(k).vel ? ev.vel : ev.pos)[Task::home(k).row * n + i] = s[k];
}

// A control task's step of env_step: truncation at max_steps, independent of
// the task's own termination; a row that ended either way takes its reset draw
// of this t as its current state and observation.
// Inlined: a noinline call costs the rollout kernels 192 B of scratch per lane
// (profiles/pendulum_rollout_resources.txt).
template <typename Task>
__device__ __forceinline__ EnvOut env_step_task(const sac_envs& ev, int i, uint64_t t, const float* act,
                                                float* final_obs) {
  const sac_env_config& c = ev.cfg;
  const int step = ev.step[i] + 1;
  float* cur = ev.obs + (size_t)i * Task::OBS;
  double s[Task::NS];
  task_load<Task>(ev, i, s);
  float fo[Task::OBS];
  EnvOut o;
  Task::dynamics(s, act, c, fo, o);
  o.truncated = step >= c.max_steps;
  const bool done = o.terminated || o.truncated;
  if (final_obs)
    for (int k = 0; k < Task::OBS; ++k) final_obs[k] = fo[k];
  if (done) {
    Task::reset_draw(c.seed, t, (uint32_t)i, s);
    Task::obs(s, fo);
  }
  for (int k = 0; k < Task::OBS; ++k) cur[k] = fo[k];
  ev.step[i] = done ? 0 : step;
  task_store<Task>(ev, i, s);
  return o;
}

// A control task's part of sac_envs_reset_kernel: the reset draw of t = 0, its observation, the state
template <typename Task>
__device__ __forceinline__ void task_reset(const sac_envs& ev, int i, uint64_t seed, float* cur) {
  double s[Task::NS];
  Task::reset_draw(seed, 0, (uint32_t)i, s);
  Task::obs(s, cur);
  task_store<Task>(ev, i, s);
}

// One step of environment row i at vector step t with the action components
// act[ACT of the class].  Writes the observation stepped to into
// final_obs[obs_dim] (unless NULL), the environment's new current observation
// (the reset observation where the episode ended) into ev.obs, and its step
// counter / state.
// KC is the kind class (EnvClass), decided by the launch: the rollout kernels are
// compiled once per class, so no class's kernels hold another's code (behind a
// run-time branch the pendulum cost the probes 16 more spilled SGPRs and 1-2 %
// per launch).
template <int KC>
__device__ __forceinline__ EnvOut env_step(const sac_envs& ev, int i, uint64_t t, const float* act, float* final_obs) {
  if constexpr (KC != ENV_CLASS_PROBES) return env_step_task<EnvTask<KC>>(ev, i, t, act, final_obs);
  const float action = act[0];
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
  } else if (!SAC_ENV_VEL_ROWS(c.kind)) {
    cur[0] = c.kind == SAC_ENV_POINT_MASS ? (float)c.start_pos : 0.f;
  }
  ev.step[i] = 0;
  ev.ep_length[i] = 0;
  with_env_class(c.kind, [&](auto kc) {
    if constexpr (decltype(kc)::value != ENV_CLASS_PROBES)
      task_reset<EnvTask<decltype(kc)::value>>(ev, i, seed, cur);
    else
      ev.pos[i] = c.kind == SAC_ENV_POINT_MASS ? c.start_pos : 0.0;
  });
  ev.ep_return[i] = 0.0;
}

__global__ void sac_envs_step_kernel(sac_envs ev, const float* __restrict__ actions, uint64_t t,
                                     float* __restrict__ obs, float* __restrict__ final_obs,
                                     float* __restrict__ reward, uint8_t* __restrict__ terminated,
                                     uint8_t* __restrict__ truncated) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ev.cfg.num_envs) return;
  const int O = ev.cfg.obs_dim;
  const float* act = actions + (size_t)i * env_act_dim(ev.cfg.kind);
  float* fin = final_obs + (size_t)i * O;
  const EnvOut o =
      with_env_class(ev.cfg.kind, [&](auto kc) { return env_step<decltype(kc)::value>(ev, i, t, act, fin); });
  env_account(ev, i, t, o);
  for (int k = 0; k < O; ++k) obs[(size_t)i * O + k] = ev.obs[(size_t)i * O + k];
  reward[i] = (float)o.reward;
  terminated[i] = o.terminated ? 1 : 0;
  truncated[i] = o.truncated ? 1 : 0;
}

// The row owner's tail: environment row i, holding the action components act[ACT
// of the class] it takes at RNG step t, copies its observation and action to
// ring slot `slot` (store != 0), steps, accounts the episode and writes the
// reward and the done word.  store: as rollout_step_body's.
template <int KC>
__device__ __forceinline__ void rollout_row_tail(const sac_envs& ev, const sac_replay& rb, const RowStrides& rs, int O,
                                                 int i, int64_t slot, uint64_t t,
                                                 const float (&act)[EnvTask<KC>::ACT], int store) {
  if (store) {
    for (int k = 0; k < O; ++k) rb.obs[slot * rs.obs + k] = ev.obs[(size_t)i * O + k];
#pragma unroll
    for (int k = 0; k < EnvTask<KC>::ACT; ++k) rb.act[slot * rs.act + k] = act[k];
  }
  const EnvOut eo = env_step<KC>(ev, i, t, act, store ? rb.next_obs + slot * rs.obs : nullptr);
  env_account(ev, i, t, eo);
  if (store) {
    rb.rew[slot * rs.one] = (float)eo.reward;
    // the done word by `store`: any end, terminated alone, or the end code of a staging table
    const int code = (eo.terminated ? 1 : 0) + (eo.truncated ? 2 : 0);
    rb.done[slot * rs.one] = (float)(store == 3 ? code : store == 2 ? (code & 1) : (code != 0));
  }
}

// The fused step of one workgroup (SAC_ROWS environments) at RNG step t, its
// rows going to ring slots (pos + i) % capacity.  new_size / new_pos: the
// replay's (size, write slot) after this step, as sac_replay_push computes
// them.  store: 0 stores nothing; 1 / 2 / 3 store the rows with done =
// terminated | truncated / terminated / terminated + 2 * truncated (the engine's
// sac_done_mode + 1: rollout_store).  Both kernels below are
// this body; they differ in where (pos, t) come from.
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
    // what the environment takes: registers (so never indexed by a run-time j).  A is the class's ACT
    // (check_rollout_dims), so these are all the components the tail stores.
    constexpr int NA = EnvTask<KC>::ACT;
    float act[NA] = {};
    for (int p = 0; 2 * p < A; ++p) {
      float e2[2] = {0.f, 0.f};
      if (!deterministic) philox_normal2(E.seed, t, (uint32_t)i, ENV_WHICH_NOISE, (uint32_t)p, e2[0], e2[1]);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int j = 2 * p + q;
        if (j >= A) break;
        float a;
        if (deterministic) a = head_act_mean(o[j], scale);  // the acting head of sac_math.h, as sac_policy_act_kernel
        else a = head_act(o[j], o[A + j], e2[q], lo, hi, scale).act;
#pragma unroll
        for (int k = 0; k < NA; ++k)
          if (j == k) act[k] = a;
      }
    }
    rollout_row_tail<KC>(ev, rb, rs, O, i, slot, t, act, store);
  }
  if (store && blockIdx.x == 0 && tid == 0) {  // as replay_push_kernel
    rb.state[0] = new_size;
    rb.state[1] = new_pos;
    rb.state[2] += 1;  // push generation: a batch phase C staged before this step is stale
  }
}

// One workgroup per SAC_ROWS environments; (size, pos, t) are host arguments,
// new_size / new_pos computed by the host as sac_replay_push does.  KC:
// the class of ev.cfg.kind (the host picks the instantiation: with_env_class).
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

// ---- The rollout step with uniform-random actions (train.random_steps)
// One thread per environment row, 256 per workgroup: row i draws its actions
// (uniform_actions_row, key = the engine's seed, scale = its action_scale, both
// kernel arguments: nothing of the engine's device state is read) and runs the
// row owner's tail.  No LDS, no barrier, no atomic.  (pos, new_size, new_pos, t,
// store) as rollout_step_body's.
#define SAC_UNIFORM_THREADS 256
template <int KC>
__device__ __forceinline__ void rollout_uniform_body(uint64_t seed, float scale, const sac_envs& ev,
                                                     const sac_replay& rb, int64_t pos, int64_t new_size,
                                                     int64_t new_pos, uint64_t t, int store) {
  const int i = blockIdx.x * SAC_UNIFORM_THREADS + threadIdx.x;
  if (i < ev.cfg.num_envs) {
    constexpr int NA = EnvTask<KC>::ACT;
    const int O = ev.cfg.obs_dim;
    float act[NA];
    uniform_actions_row(seed, t, (uint32_t)i, scale, NA, act);
    rollout_row_tail<KC>(ev, rb, row_strides(rb.row_stride, O, NA), O, i, (pos + i) % rb.capacity, t, act, store);
  }
  if (store && blockIdx.x == 0 && threadIdx.x == 0) {  // as replay_push_kernel
    rb.state[0] = new_size;
    rb.state[1] = new_pos;
    rb.state[2] += 1;
  }
}

template <int KC>
__global__ void __launch_bounds__(SAC_UNIFORM_THREADS) sac_rollout_uniform_kernel(uint64_t seed, float scale,
                                                                                 sac_envs ev, sac_replay rb,
                                                                                 int64_t pos, int64_t new_size,
                                                                                 int64_t new_pos, uint64_t t,
                                                                                 int store) {
  rollout_uniform_body<KC>(seed, scale, ev, rb, pos, new_size, new_pos, t, store);
}

// The cursor form, exactly as sac_rollout_step_dev_kernel: cur is only read, nxt and rb.state only written.
template <int KC>
__global__ void __launch_bounds__(SAC_UNIFORM_THREADS) sac_rollout_uniform_dev_kernel(uint64_t seed, float scale,
                                                                                     sac_envs ev, sac_replay rb,
                                                                                     const int64_t* __restrict__ cur,
                                                                                     int64_t* __restrict__ nxt,
                                                                                     int store) {
  const int64_t size = cur[0], pos = cur[1], cap = rb.capacity, n = ev.cfg.num_envs;
  const uint64_t t = (uint64_t)cur[2] + 1;
  if (size < 0 || size > cap || pos < 0 || pos >= cap) return;
  const int64_t new_size = store ? (size + n < cap ? size + n : cap) : size;
  const int64_t new_pos = store ? (pos + n) % cap : pos;
  rollout_uniform_body<KC>(seed, scale, ev, rb, pos, new_size, new_pos, t, store);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    nxt[0] = new_size;
    nxt[1] = new_pos;
    nxt[2] = (int64_t)t;
    nxt[3] = 0;
  }
}
