// sac_torch_ops.cpp — PyTorch-ROCm custom ops over the C ABI (include/sac_engine.h).
//
// TORCH_LIBRARY(sac_hip): the operator boundary SURVEY.md §8(b) names for the
// hot path.  Every op launches on the caller's CURRENT HIP stream
// (torch.cuda.current_stream(): ROCm PyTorch's HIP stream masquerading as the
// "cuda" device type), never synchronises the host, allocates its
// outputs from the PyTorch caching allocator, and is capturable by
// torch.cuda.graph.  Meta kernels give the output shapes (fake tensors).
//
//   replay_push          ReplayBuffer.push            (reference sac/replay_buffer.py:21-30)
//   replay_gather        ReplayBuffer.sample +        (replay_buffer.py:32-39,
//                        SAC.sample_batch stacking     sac/agent.py:166-193)
//   replay_sample        the index draw of random.sample (replay_buffer.py:39)
//   replay_sample_gather sampler + gather in one kernel
//   replay_emit_nstep    the n-step rows of the last n vector steps, staging table -> replay ring (train.n_step)
//   replay_emit_nstep_codes  the same from a staging table of end codes (train.bootstrap_truncated)
//   engine_set_done_mode what the rollout step stores as done (enum sac_done_mode); host state, no launch
//   engine_set_action_source  where its sampled actions come from (enum sac_action_source); host state, no launch
//   train_step           SAC.training_step            (sac/agent.py:302-327)
//   train_graph          a loop of training_step      (sac/agent.py:361-364), hipGraph-replayed
//   policy_act           SAC.select_action            (sac/agent.py:149-156; models.py:79-92)
//   q_values             the critic forwards of SAC._log_q_values (sac/agent.py:493-500), ONE kernel
//   q_values_replay      the same on ring slots of a replay buffer (no gather, no copy)
//   envs_reset           SyncVectorEnv.reset          (sac/vector_env.py:39-46 over sac/envs.py)
//   envs_step            SyncVectorEnv.step           (sac/vector_env.py:55-71 over sac/envs.py)
//   rollout_step         select_actions + env.step + store_transitions of one vector step, ONE kernel
//   rollout_step_dev     the same with (size, pos, t) read from a device loop cursor
//   q_values_replay_dev  q_values_replay on the rows of the vector step a cursor slot describes
//   loop_graph           K iterations of the device-resident loop, ONE hipGraph replay
//
// Replay storage is ONE fp32 tensor per buffer; `layout` = [capacity, obs_dim,
// act_dim, row_stride, off_obs, off_act, off_rew, off_next_obs, off_done]
// (offsets in floats from storage.data_ptr(); row_stride 0 = struct-of-arrays).
// Environment state (envs_*, rollout_step): `obs` [N][O] fp32, `counters`
// int32 [2][N] (step in episode, episode length), `dstate` float64
// [SAC_ENV_POS_ROWS + 1 + SAC_ENV_VEL_ROWS][N] (the kind's sac_envs.pos rows,
// the episode return, its sac_envs.vel rows: include/sac_engine.h has the
// widths and each task's components), `ring` float64 [S][N][2] (the sac_env_episode
// cells: return, then length and ended as two int32); `icfg` = [kind, num_envs,
// obs_dim, max_steps], `params` = the 11 doubles of sac_env_config in order.
// Engine state: `engine` is the sac_engine* handle (int64) from
// sac_engine_create; `state` lists the 16 caller-owned tensors the step reads
// and writes (sac_engine_buffers order) so the op's mutation is declared.
//
// The ops do not link libsac_engine.so: bind_engine_library(path) dlopens the
// library the Python side loaded (the same file, hence the same instance as the
// ctypes handle's owner, also for the diagnostic -DSAC_STAMPS build) and
// resolves the entry points once.
#include <dlfcn.h>

#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/library.h>

#include "sac_engine.h"

namespace {

constexpr int64_t kStateTensors = 16;
using Guard = c10::hip::HIPGuardMasqueradingAsCUDA;

// the C ABI entry points the ops call, resolved by bind_engine_library
struct EngineApi {
  decltype(&sac_last_error) last_error = nullptr;
  decltype(&sac_replay_push) replay_push = nullptr;
  decltype(&sac_replay_gather) replay_gather = nullptr;
  decltype(&sac_replay_sample_indices) replay_sample_indices = nullptr;
  decltype(&sac_replay_sample_gather) replay_sample_gather = nullptr;
  decltype(&sac_replay_emit_nstep) replay_emit_nstep = nullptr;
  decltype(&sac_replay_emit_nstep_codes) replay_emit_nstep_codes = nullptr;
  decltype(&sac_engine_set_done_mode) engine_set_done_mode = nullptr;
  decltype(&sac_engine_set_action_source) engine_set_action_source = nullptr;
  decltype(&sac_engine_train) engine_train = nullptr;
  decltype(&sac_engine_train_graph) engine_train_graph = nullptr;
  decltype(&sac_policy_act) policy_act = nullptr;
  decltype(&sac_q_values) q_values = nullptr;
  decltype(&sac_q_values_replay) q_values_replay = nullptr;
  decltype(&sac_envs_reset) envs_reset = nullptr;
  decltype(&sac_envs_step) envs_step = nullptr;
  decltype(&sac_rollout_step) rollout_step = nullptr;
  decltype(&sac_rollout_step_dev) rollout_step_dev = nullptr;
  decltype(&sac_q_values_replay_dev) q_values_replay_dev = nullptr;
  decltype(&sac_engine_loop_graph) engine_loop_graph = nullptr;
};
EngineApi g_api;
std::string g_bound_path;

template <typename F>
void resolve(void* h, const char* name, F& f) {
  f = reinterpret_cast<F>(dlsym(h, name));
  TORCH_CHECK(f != nullptr, "libsac_engine lacks ", name);
}

void bind_engine_library(c10::string_view path_) {
  const std::string path(path_.data(), path_.size());
  if (g_api.engine_train && path == g_bound_path) return;
  void* h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
  TORCH_CHECK(h != nullptr, "cannot load ", path, ": ", dlerror());
  EngineApi a;
  resolve(h, "sac_last_error", a.last_error);
  resolve(h, "sac_replay_push", a.replay_push);
  resolve(h, "sac_replay_gather", a.replay_gather);
  resolve(h, "sac_replay_sample_indices", a.replay_sample_indices);
  resolve(h, "sac_replay_sample_gather", a.replay_sample_gather);
  resolve(h, "sac_replay_emit_nstep", a.replay_emit_nstep);
  resolve(h, "sac_replay_emit_nstep_codes", a.replay_emit_nstep_codes);
  resolve(h, "sac_engine_set_done_mode", a.engine_set_done_mode);
  resolve(h, "sac_engine_set_action_source", a.engine_set_action_source);
  resolve(h, "sac_engine_train", a.engine_train);
  resolve(h, "sac_engine_train_graph", a.engine_train_graph);
  resolve(h, "sac_policy_act", a.policy_act);
  resolve(h, "sac_q_values", a.q_values);
  resolve(h, "sac_q_values_replay", a.q_values_replay);
  resolve(h, "sac_envs_reset", a.envs_reset);
  resolve(h, "sac_envs_step", a.envs_step);
  resolve(h, "sac_rollout_step", a.rollout_step);
  resolve(h, "sac_rollout_step_dev", a.rollout_step_dev);
  resolve(h, "sac_q_values_replay_dev", a.q_values_replay_dev);
  resolve(h, "sac_engine_loop_graph", a.engine_loop_graph);
  g_api = a;
  g_bound_path = path;
}

const EngineApi& api() {
  TORCH_CHECK(g_api.engine_train != nullptr,
              "torch.ops.sac_hip: engine library not bound (call sac._engine.ops(), which binds libsac_engine.so)");
  return g_api;
}

void* stream_of(const at::Tensor& t) {
  return static_cast<void*>(c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream());
}

void check_rc(int rc) {
  // SAC_E_NOT_ENOUGH is the reference's ValueError (replay_buffer.py:35-38)
  if (rc == SAC_OK) return;
  TORCH_CHECK_VALUE(rc != SAC_E_NOT_ENOUGH, api().last_error());
  TORCH_CHECK(false, "libsac_engine error ", rc, ": ", api().last_error());
}

void check_f32(const at::Tensor& t, const char* what) {
  TORCH_CHECK(t.is_cuda(), what, " must be a HIP device tensor");
  TORCH_CHECK(t.scalar_type() == at::kFloat, what, " must be float32");
  TORCH_CHECK(t.is_contiguous(), what, " must be contiguous");
}

struct Replay {
  sac_replay d;
  int64_t obs, act;
};

Replay make_replay(const at::Tensor& storage, const at::Tensor& state, at::IntArrayRef layout) {
  TORCH_CHECK(layout.size() == 9, "replay layout must have 9 entries");
  check_f32(storage, "replay storage");
  TORCH_CHECK(state.is_cuda() && state.scalar_type() == at::kLong && state.numel() >= 3 && state.is_contiguous(),
              "replay state must be a contiguous int64 device tensor of >= 3 entries");
  TORCH_CHECK(state.device() == storage.device(), "replay state and storage on different devices");
  const int64_t cap = layout[0], O = layout[1], A = layout[2], stride = layout[3];
  TORCH_CHECK(cap >= 1 && O >= 1 && A >= 1 && stride >= 0, "bad replay layout");
  const int64_t width[5] = {O, A, 1, O, 1};
  const int64_t n = storage.numel();
  for (int f = 0; f < 5; ++f) {
    const int64_t off = layout[4 + f];
    const int64_t end = stride ? off + (cap - 1) * stride + width[f] : off + cap * width[f];
    TORCH_CHECK(off >= 0 && end <= n, "replay field ", f, " exceeds the storage tensor");
    if (stride) TORCH_CHECK(width[f] <= stride, "record stride narrower than a field");
  }
  float* base = storage.data_ptr<float>();
  Replay r;
  r.d.obs = base + layout[4];
  r.d.act = base + layout[5];
  r.d.rew = base + layout[6];
  r.d.next_obs = base + layout[7];
  r.d.done = base + layout[8];
  r.d.capacity = cap;
  r.d.obs_dim = static_cast<int32_t>(O);
  r.d.act_dim = static_cast<int32_t>(A);
  r.d.state = state.data_ptr<int64_t>();
  r.d.row_stride = stride;
  r.obs = O;
  r.act = A;
  return r;
}

sac_engine* engine_of(int64_t handle, const at::TensorList& state, const at::Tensor& like) {
  TORCH_CHECK(handle != 0, "null engine handle");
  TORCH_CHECK(static_cast<int64_t>(state.size()) == kStateTensors, "engine state must list ", kStateTensors,
              " tensors (sac_engine_buffers order)");
  for (const auto& t : state)
    TORCH_CHECK(t.is_cuda() && t.device() == like.device(), "engine state tensor not on the replay's device");
  return reinterpret_cast<sac_engine*>(handle);
}

// ---------------------------------------------------------------- replay
void replay_push(at::Tensor& storage, at::Tensor& state, at::IntArrayRef layout, const at::Tensor& rows,
                 int64_t size, int64_t pos) {
  Replay r = make_replay(storage, state, layout);
  check_f32(rows, "rows");
  TORCH_CHECK(rows.dim() == 2 && rows.size(1) == 2 * r.obs + r.act + 2, "rows must be [n][2*obs+act+2]");
  TORCH_CHECK(rows.device() == storage.device(), "rows on a different device");
  if (rows.size(0) == 0) return;
  Guard g(storage.device());
  check_rc(api().replay_push(&r.d, rows.data_ptr<float>(), rows.size(0), size, pos, stream_of(storage)));
}

std::vector<at::Tensor> empty_batch(const at::Tensor& like, int64_t B, int64_t O, int64_t A) {
  auto o = like.options().dtype(at::kFloat);
  return {at::empty({B, O}, o), at::empty({B, A}, o), at::empty({B}, o), at::empty({B, O}, o), at::empty({B}, o)};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> replay_gather(
    const at::Tensor& storage, const at::Tensor& state, at::IntArrayRef layout, const at::Tensor& indices) {
  Replay r = make_replay(storage, state, layout);
  TORCH_CHECK(indices.is_cuda() && indices.scalar_type() == at::kInt && indices.dim() == 1 && indices.is_contiguous(),
              "indices must be a contiguous 1-D int32 device tensor");
  const int64_t B = indices.size(0);
  auto out = empty_batch(storage, B, r.obs, r.act);
  if (B) {
    Guard g(storage.device());
    check_rc(api().replay_gather(&r.d, indices.data_ptr<int32_t>(), static_cast<int32_t>(B), out[0].data_ptr<float>(),
                               out[1].data_ptr<float>(), out[2].data_ptr<float>(), out[3].data_ptr<float>(),
                               out[4].data_ptr<float>(), stream_of(storage)));
  }
  return {out[0], out[1], out[2], out[3], out[4]};
}

at::Tensor replay_sample(const at::Tensor& storage, const at::Tensor& state, at::IntArrayRef layout, int64_t batch,
                         int64_t seed, int64_t step) {
  Replay r = make_replay(storage, state, layout);
  TORCH_CHECK(batch >= 1 && batch <= r.d.capacity, "batch must be in [1, capacity]");
  auto idx = at::empty({batch}, storage.options().dtype(at::kInt));
  Guard g(storage.device());
  check_rc(api().replay_sample_indices(&r.d, static_cast<int32_t>(batch), static_cast<uint64_t>(seed),
                                     static_cast<uint64_t>(step), idx.data_ptr<int32_t>(), stream_of(storage)));
  return idx;
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> replay_sample_gather(
    const at::Tensor& storage, const at::Tensor& state, at::IntArrayRef layout, int64_t batch, int64_t seed,
    int64_t step) {
  Replay r = make_replay(storage, state, layout);
  TORCH_CHECK(batch >= 1 && batch <= r.d.capacity, "batch must be in [1, capacity]");
  auto idx = at::empty({batch}, storage.options().dtype(at::kInt));
  auto out = empty_batch(storage, batch, r.obs, r.act);
  Guard g(storage.device());
  check_rc(api().replay_sample_gather(&r.d, static_cast<int32_t>(batch), static_cast<uint64_t>(seed),
                                    static_cast<uint64_t>(step), idx.data_ptr<int32_t>(), out[0].data_ptr<float>(),
                                    out[1].data_ptr<float>(), out[2].data_ptr<float>(), out[3].data_ptr<float>(),
                                    out[4].data_ptr<float>(), stream_of(storage)));
  return {idx, out[0], out[1], out[2], out[3], out[4]};
}

// The n-step rows of the last n vector steps: reads the staging table, writes num_envs rows and the state
// words of the destination (include/sac_engine.h sac_replay_emit_nstep).  gpow = [1, g, g^2, ...], at least n long.
void replay_emit_nstep(at::Tensor& storage, at::Tensor& state, at::IntArrayRef layout, const at::Tensor& stage_storage,
                       const at::Tensor& stage_state, at::IntArrayRef stage_layout, int64_t n, int64_t num_envs,
                       int64_t newest, at::ArrayRef<double> gpow, int64_t size, int64_t pos) {
  Replay r = make_replay(storage, state, layout);
  Replay st = make_replay(stage_storage, stage_state, stage_layout);
  TORCH_CHECK(stage_storage.device() == storage.device(), "staging table and replay on different devices");
  TORCH_CHECK(n >= 1 && n <= SAC_NSTEP_MAX, "n must be in [1, ", SAC_NSTEP_MAX, "]");
  TORCH_CHECK(num_envs >= 1 && num_envs <= INT32_MAX, "num_envs must be >= 1");
  TORCH_CHECK(static_cast<int64_t>(gpow.size()) >= n, "gpow must hold at least n discount powers");
  Guard g(storage.device());
  check_rc(api().replay_emit_nstep(&st.d, &r.d, static_cast<int32_t>(n), static_cast<int32_t>(num_envs), newest,
                                   gpow.data(), size, pos, stream_of(storage)));
}

// The same from end codes (include/sac_engine.h sac_replay_emit_nstep_codes): gpow at least n + 1 long.
void replay_emit_nstep_codes(at::Tensor& storage, at::Tensor& state, at::IntArrayRef layout,
                             const at::Tensor& stage_storage, const at::Tensor& stage_state,
                             at::IntArrayRef stage_layout, int64_t n, int64_t num_envs, int64_t newest,
                             at::ArrayRef<double> gpow, int64_t size, int64_t pos) {
  Replay r = make_replay(storage, state, layout);
  Replay st = make_replay(stage_storage, stage_state, stage_layout);
  TORCH_CHECK(stage_storage.device() == storage.device(), "staging table and replay on different devices");
  TORCH_CHECK(n >= 1 && n <= SAC_NSTEP_MAX, "n must be in [1, ", SAC_NSTEP_MAX, "]");
  TORCH_CHECK(num_envs >= 1 && num_envs <= INT32_MAX, "num_envs must be >= 1");
  TORCH_CHECK(static_cast<int64_t>(gpow.size()) >= n + 1, "gpow must hold at least n + 1 discount powers");
  Guard g(storage.device());
  check_rc(api().replay_emit_nstep_codes(&st.d, &r.d, static_cast<int32_t>(n), static_cast<int32_t>(num_envs), newest,
                                         gpow.data(), size, pos, stream_of(storage)));
}

// ---------------------------------------------------------------- learner
void engine_set_done_mode(int64_t engine, int64_t mode) {
  TORCH_CHECK(engine != 0, "null engine handle");
  TORCH_CHECK_VALUE(mode >= 0 && mode <= 2, "done mode must be 0 (any end), 1 (terminated) or 2 (end code)");
  check_rc(api().engine_set_done_mode(reinterpret_cast<sac_engine*>(engine), static_cast<int32_t>(mode)));
}

void engine_set_action_source(int64_t engine, int64_t source) {
  TORCH_CHECK(engine != 0, "null engine handle");
  TORCH_CHECK_VALUE(source >= 0 && source <= 1, "action source must be 0 (policy) or 1 (uniform)");
  check_rc(api().engine_set_action_source(reinterpret_cast<sac_engine*>(engine), static_cast<int32_t>(source)));
}

void train_step(int64_t engine, at::TensorList state, const at::Tensor& storage, const at::Tensor& rstate,
                at::IntArrayRef layout, int64_t n_steps, const std::optional<at::Tensor>& indices,
                const std::optional<at::Tensor>& eps) {
  Replay r = make_replay(storage, rstate, layout);
  sac_engine* e = engine_of(engine, state, storage);
  TORCH_CHECK(n_steps >= 0, "n_steps must be >= 0");
  const int32_t* ip = nullptr;
  const float* ep = nullptr;
  if (indices && indices->defined()) {
    const auto& t = *indices;
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kInt && t.is_contiguous() && t.dim() == 2 &&
                    t.size(0) >= n_steps,
                "indices must be a contiguous [n_steps][batch] int32 device tensor");
    ip = t.data_ptr<int32_t>();
  }
  if (eps && eps->defined()) {
    const auto& t = *eps;
    check_f32(t, "eps");
    TORCH_CHECK(t.dim() == 4 && t.size(0) >= n_steps && t.size(1) == 2 && t.size(3) == r.act,
                "eps must be [n_steps][2][batch][act_dim]");
    ep = t.data_ptr<float>();
  }
  if (!n_steps) return;
  Guard g(storage.device());
  check_rc(api().engine_train(e, &r.d, static_cast<int32_t>(n_steps), ip, ep, stream_of(storage)));
}

void train_graph(int64_t engine, at::TensorList state, const at::Tensor& storage, const at::Tensor& rstate,
                 at::IntArrayRef layout, int64_t n_steps, int64_t chunk) {
  Replay r = make_replay(storage, rstate, layout);
  sac_engine* e = engine_of(engine, state, storage);
  TORCH_CHECK(n_steps >= 0 && chunk >= 1, "n_steps >= 0 and chunk >= 1");
  Guard g(storage.device());
  check_rc(api().engine_train_graph(e, &r.d, static_cast<int32_t>(n_steps), static_cast<int32_t>(chunk),
                                  stream_of(storage)));
}

std::tuple<at::Tensor, at::Tensor> policy_act(int64_t engine, const at::Tensor& obs, const std::optional<at::Tensor>& eps,
                                              int64_t act_dim, bool want_log_pi) {
  TORCH_CHECK(engine != 0, "null engine handle");
  check_f32(obs, "obs");
  TORCH_CHECK(obs.dim() == 2, "obs must be [n][obs_dim]");
  const int64_t n = obs.size(0);
  const float* ep = nullptr;
  if (eps && eps->defined()) {
    check_f32(*eps, "eps");
    TORCH_CHECK(eps->dim() == 2 && eps->size(0) == n && eps->size(1) == act_dim, "eps must be [n][act_dim]");
    ep = eps->data_ptr<float>();
  }
  auto o = obs.options();
  at::Tensor act = at::empty({n, act_dim}, o);
  at::Tensor lp = at::empty({(want_log_pi && ep) ? n : 0}, o);
  if (n) {
    Guard g(obs.device());
    check_rc(api().policy_act(reinterpret_cast<sac_engine*>(engine), obs.data_ptr<float>(), static_cast<int32_t>(n), ep,
                            act.data_ptr<float>(), lp.numel() ? lp.data_ptr<float>() : nullptr, stream_of(obs)));
  }
  return {act, lp};
}

// rows of a [n][width] fp32 device tensor addressed by (data_ptr, stride(0)): a
// column view of a wider table works without a copy
void check_rows(const at::Tensor& t, const char* what) {
  TORCH_CHECK(t.is_cuda(), what, " must be a HIP device tensor");
  TORCH_CHECK(t.scalar_type() == at::kFloat, what, " must be float32");
  TORCH_CHECK(t.dim() == 2 && t.size(1) >= 1, what, " must be [n][width]");
  TORCH_CHECK(t.size(1) == 1 || t.stride(1) == 1, what, " must have unit inner stride");
  TORCH_CHECK(t.size(0) <= 1 || t.stride(0) >= t.size(1), what, " rows overlap (row stride below the width)");
}

at::Tensor q_values(int64_t engine, const at::Tensor& obs, const at::Tensor& act, bool target) {
  TORCH_CHECK(engine != 0, "null engine handle");
  check_rows(obs, "obs");
  check_rows(act, "act");
  TORCH_CHECK(obs.size(0) == act.size(0) && obs.device() == act.device(),
              "obs and act must hold the same number of rows on one device");
  const int64_t n = obs.size(0);
  TORCH_CHECK(n <= INT32_MAX, "too many rows");
  at::Tensor q = at::empty({n, 2}, obs.options());
  if (n) {
    Guard g(obs.device());
    // one row: any stride addresses it; pass the width
    const int64_t so = n > 1 ? obs.stride(0) : obs.size(1), sa = n > 1 ? act.stride(0) : act.size(1);
    check_rc(api().q_values(reinterpret_cast<sac_engine*>(engine), obs.data_ptr<float>(), so, act.data_ptr<float>(), sa,
                            static_cast<int32_t>(n), target ? 1 : 0, q.data_ptr<float>(), stream_of(obs)));
  }
  return q;
}

at::Tensor q_values_replay(int64_t engine, const at::Tensor& storage, const at::Tensor& rstate, at::IntArrayRef layout,
                           int64_t first_slot, int64_t n, bool next_obs, bool target) {
  TORCH_CHECK(engine != 0, "null engine handle");
  Replay r = make_replay(storage, rstate, layout);
  TORCH_CHECK(n >= 1 && n <= r.d.capacity, "n must be in [1, capacity]");
  at::Tensor q = at::empty({n, 2}, storage.options());
  Guard g(storage.device());
  check_rc(api().q_values_replay(reinterpret_cast<sac_engine*>(engine), &r.d, first_slot, static_cast<int32_t>(n),
                                 next_obs ? 1 : 0, target ? 1 : 0, q.data_ptr<float>(), stream_of(storage)));
  return q;
}

// ---------------------------------------------------------------- environments
sac_envs make_envs(const at::Tensor& obs, const at::Tensor& counters, const at::Tensor& dstate,
                   const std::optional<at::Tensor>& ring, at::IntArrayRef icfg, at::ArrayRef<double> params,
                   int64_t seed) {
  TORCH_CHECK(icfg.size() == 4, "icfg must be [kind, num_envs, obs_dim, max_steps]");
  TORCH_CHECK(params.size() == 11, "params must hold the 11 doubles of sac_env_config");
  const int64_t N = icfg[1], O = icfg[2];
  // the kind's sac_envs.pos / .vel
  const int64_t pos_rows = SAC_ENV_POS_ROWS(icfg[0]), vel_rows = SAC_ENV_VEL_ROWS(icfg[0]);
  TORCH_CHECK(N >= 1 && N <= INT32_MAX && O >= 1 && O <= INT32_MAX, "num_envs and obs_dim must be >= 1");
  check_f32(obs, "env obs");
  TORCH_CHECK(obs.dim() == 2 && obs.size(0) == N && obs.size(1) == O, "env obs must be [num_envs][obs_dim]");
  TORCH_CHECK(counters.is_cuda() && counters.scalar_type() == at::kInt && counters.is_contiguous() &&
                  counters.dim() == 2 && counters.size(0) == 2 && counters.size(1) == N,
              "env counters must be a contiguous int32 [2][num_envs] device tensor");
  TORCH_CHECK(dstate.is_cuda() && dstate.scalar_type() == at::kDouble && dstate.is_contiguous() && dstate.dim() == 2 &&
                  dstate.size(0) == pos_rows + 1 + vel_rows && dstate.size(1) == N,
              "env dstate must be a contiguous float64 [2][num_envs] device tensor ([3][num_envs] for the pendulum, "
              "[7][num_envs] for the reacher, [5][num_envs] for the cart-pole)");
  TORCH_CHECK(counters.device() == obs.device() && dstate.device() == obs.device(), "env state on different devices");
  sac_envs ev{};
  ev.cfg.kind = static_cast<int32_t>(icfg[0]);
  ev.cfg.num_envs = static_cast<int32_t>(N);
  ev.cfg.obs_dim = static_cast<int32_t>(O);
  ev.cfg.max_steps = static_cast<int32_t>(std::min<int64_t>(std::max<int64_t>(icfg[3], INT32_MIN), INT32_MAX));
  ev.cfg.reward = params[0];
  ev.cfg.target = params[1];
  ev.cfg.action_low = params[2];
  ev.cfg.action_high = params[3];
  ev.cfg.threshold = params[4];
  ev.cfg.start_pos = params[5];
  ev.cfg.goal_pos = params[6];
  ev.cfg.dt = params[7];
  ev.cfg.step_penalty = params[8];
  ev.cfg.goal_reward = params[9];
  ev.cfg.goal_tolerance = params[10];
  ev.cfg.seed = static_cast<uint64_t>(seed);
  ev.obs = obs.data_ptr<float>();
  ev.step = counters.data_ptr<int32_t>();
  ev.ep_length = ev.step + N;
  ev.pos = dstate.data_ptr<double>();
  ev.ep_return = ev.pos + pos_rows * N;
  ev.vel = vel_rows ? ev.ep_return + N : nullptr;
  if (ring && ring->defined()) {
    const auto& r = *ring;
    TORCH_CHECK(r.is_cuda() && r.scalar_type() == at::kDouble && r.is_contiguous() && r.dim() == 3 && r.size(0) >= 1 &&
                    r.size(1) == N && r.size(2) == 2 && r.device() == obs.device(),
                "episode ring must be a contiguous float64 [ring_steps][num_envs][2] device tensor");
    static_assert(sizeof(sac_env_episode) == 2 * sizeof(double), "ring cell layout");
    ev.episodes = reinterpret_cast<sac_env_episode*>(r.data_ptr<double>());
    ev.ring_steps = r.size(0);
  }
  return ev;
}

void envs_reset(at::Tensor& obs, at::Tensor& counters, at::Tensor& dstate, at::IntArrayRef icfg,
                at::ArrayRef<double> params, int64_t seed) {
  sac_envs ev = make_envs(obs, counters, dstate, std::nullopt, icfg, params, seed);
  Guard g(obs.device());
  check_rc(api().envs_reset(&ev, static_cast<uint64_t>(seed), stream_of(obs)));
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> envs_step(
    at::Tensor& obs, at::Tensor& counters, at::Tensor& dstate, const std::optional<at::Tensor>& ring,
    at::IntArrayRef icfg, at::ArrayRef<double> params, int64_t seed, const at::Tensor& actions, int64_t t) {
  sac_envs ev = make_envs(obs, counters, dstate, ring, icfg, params, seed);
  check_f32(actions, "actions");
  const int64_t A = SAC_ENV_ACT_DIM(ev.cfg.kind);
  TORCH_CHECK(actions.dim() == 2 && actions.size(0) == obs.size(0) && actions.size(1) == A &&
                  actions.device() == obs.device(),
              "actions must be [num_envs][", A, "] on the environments' device");
  TORCH_CHECK(t >= 1, "vector step t must be >= 1 (0 is the reset)");
  const int64_t N = obs.size(0), O = obs.size(1);
  auto o = obs.options();
  at::Tensor obs_out = at::empty({N, O}, o), final_obs = at::empty({N, O}, o), reward = at::empty({N}, o);
  at::Tensor term = at::empty({N}, o.dtype(at::kBool)), trunc = at::empty({N}, o.dtype(at::kBool));
  Guard g(obs.device());
  check_rc(api().envs_step(&ev, actions.data_ptr<float>(), static_cast<uint64_t>(t), obs_out.data_ptr<float>(),
                           final_obs.data_ptr<float>(), reward.data_ptr<float>(),
                           reinterpret_cast<uint8_t*>(term.data_ptr<bool>()),
                           reinterpret_cast<uint8_t*>(trunc.data_ptr<bool>()), stream_of(obs)));
  return {obs_out, final_obs, reward, term, trunc};
}

void rollout_step(int64_t engine, at::Tensor& obs, at::Tensor& counters, at::Tensor& dstate, at::Tensor& ring,
                  at::IntArrayRef icfg, at::ArrayRef<double> params, int64_t seed, at::Tensor& storage,
                  at::Tensor& rstate, at::IntArrayRef layout, int64_t size, int64_t pos, int64_t t, bool deterministic,
                  bool store) {
  TORCH_CHECK(engine != 0, "null engine handle");
  sac_envs ev = make_envs(obs, counters, dstate, ring, icfg, params, seed);
  Replay r = make_replay(storage, rstate, layout);
  TORCH_CHECK(storage.device() == obs.device(), "replay and environments on different devices");
  TORCH_CHECK(t >= 1, "vector step t must be >= 1 (0 is the reset)");
  Guard g(obs.device());
  check_rc(api().rollout_step(reinterpret_cast<sac_engine*>(engine), &ev, &r.d, size, pos, static_cast<uint64_t>(t),
                              deterministic ? 1 : 0, store ? 1 : 0, stream_of(obs)));
}

// ---------------------------------------------------------------- device loop cursor
int64_t* cursor_of(const at::Tensor& cursor, const at::Tensor& like) {
  TORCH_CHECK(cursor.is_cuda() && cursor.scalar_type() == at::kLong && cursor.is_contiguous() && cursor.dim() == 2 &&
                  cursor.size(0) == 2 && cursor.size(1) == 4 && cursor.device() == like.device(),
              "cursor must be a contiguous int64 [2][4] tensor on the replay's device");
  return cursor.data_ptr<int64_t>();
}

float* q_ring_of(const at::Tensor& q_ring, int64_t n, const at::Tensor& like) {
  check_f32(q_ring, "q_ring");
  TORCH_CHECK(q_ring.dim() == 3 && q_ring.size(0) >= 1 && q_ring.size(0) <= INT32_MAX && q_ring.size(1) == n &&
                  q_ring.size(2) == 2 && q_ring.device() == like.device(),
              "q_ring must be [steps][", n, "][2] on the replay's device");
  return q_ring.data_ptr<float>();
}

void rollout_step_dev(int64_t engine, at::Tensor& obs, at::Tensor& counters, at::Tensor& dstate, at::Tensor& ring,
                      at::IntArrayRef icfg, at::ArrayRef<double> params, int64_t seed, at::Tensor& storage,
                      at::Tensor& rstate, at::IntArrayRef layout, at::Tensor& cursor, int64_t parity, bool deterministic,
                      bool store) {
  TORCH_CHECK(engine != 0, "null engine handle");
  sac_envs ev = make_envs(obs, counters, dstate, ring, icfg, params, seed);
  Replay r = make_replay(storage, rstate, layout);
  TORCH_CHECK(storage.device() == obs.device(), "replay and environments on different devices");
  int64_t* cur = cursor_of(cursor, storage);
  TORCH_CHECK(parity == 0 || parity == 1, "parity must be 0 or 1");
  Guard g(obs.device());
  check_rc(api().rollout_step_dev(reinterpret_cast<sac_engine*>(engine), &ev, &r.d, cur, static_cast<int32_t>(parity),
                                  deterministic ? 1 : 0, store ? 1 : 0, stream_of(obs)));
}

void q_values_replay_dev(int64_t engine, const at::Tensor& storage, const at::Tensor& rstate, at::IntArrayRef layout,
                         const at::Tensor& cursor, int64_t parity, int64_t n, bool next_obs, bool target,
                         at::Tensor& q_ring) {
  TORCH_CHECK(engine != 0, "null engine handle");
  Replay r = make_replay(storage, rstate, layout);
  TORCH_CHECK(n >= 1 && n <= r.d.capacity, "n must be in [1, capacity]");
  const int64_t* cur = cursor_of(cursor, storage);
  TORCH_CHECK(parity == 0 || parity == 1, "parity must be 0 or 1");
  float* q = q_ring_of(q_ring, n, storage);
  Guard g(storage.device());
  check_rc(api().q_values_replay_dev(reinterpret_cast<sac_engine*>(engine), &r.d, cur, static_cast<int32_t>(parity),
                                     static_cast<int32_t>(n), next_obs ? 1 : 0, target ? 1 : 0, q,
                                     static_cast<int32_t>(q_ring.size(0)), stream_of(storage)));
}

void loop_graph(int64_t engine, at::TensorList state, at::Tensor& obs, at::Tensor& counters, at::Tensor& dstate,
                at::Tensor& ring, at::IntArrayRef icfg, at::ArrayRef<double> params, int64_t seed, at::Tensor& storage,
                at::Tensor& rstate, at::IntArrayRef layout, at::Tensor& cursor, at::IntArrayRef grad_steps,
                int64_t n_replays, const std::optional<at::Tensor>& q_ring) {
  sac_envs ev = make_envs(obs, counters, dstate, ring, icfg, params, seed);
  Replay r = make_replay(storage, rstate, layout);
  sac_engine* e = engine_of(engine, state, storage);
  TORCH_CHECK(storage.device() == obs.device(), "replay and environments on different devices");
  int64_t* cur = cursor_of(cursor, storage);
  TORCH_CHECK(grad_steps.size() <= INT32_MAX && n_replays >= 0 && n_replays <= INT32_MAX,
              "grad_steps / n_replays out of range");
  std::vector<int32_t> g32;
  for (int64_t v : grad_steps) {
    TORCH_CHECK(v >= 0 && v <= INT32_MAX, "gradient-step counts must be >= 0");
    g32.push_back(static_cast<int32_t>(v));
  }
  float* q = nullptr;
  int32_t q_steps = 0;
  if (q_ring && q_ring->defined()) {
    q = q_ring_of(*q_ring, ev.cfg.num_envs, storage);
    q_steps = static_cast<int32_t>(q_ring->size(0));
  }
  Guard g(storage.device());
  check_rc(api().engine_loop_graph(e, &ev, &r.d, cur, static_cast<int32_t>(g32.size()), g32.data(), q, q_steps,
                                   static_cast<int32_t>(n_replays), stream_of(storage)));
}

// ---------------------------------------------------------------- meta (shapes only)
void replay_push_meta(at::Tensor&, at::Tensor&, at::IntArrayRef, const at::Tensor&, int64_t, int64_t) {}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> replay_gather_meta(
    const at::Tensor& storage, const at::Tensor&, at::IntArrayRef layout, const at::Tensor& indices) {
  auto o = empty_batch(storage, indices.size(0), layout[1], layout[2]);
  return {o[0], o[1], o[2], o[3], o[4]};
}

at::Tensor replay_sample_meta(const at::Tensor& storage, const at::Tensor&, at::IntArrayRef, int64_t batch, int64_t,
                              int64_t) {
  return at::empty({batch}, storage.options().dtype(at::kInt));
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> replay_sample_gather_meta(
    const at::Tensor& storage, const at::Tensor&, at::IntArrayRef layout, int64_t batch, int64_t, int64_t) {
  auto o = empty_batch(storage, batch, layout[1], layout[2]);
  return {at::empty({batch}, storage.options().dtype(at::kInt)), o[0], o[1], o[2], o[3], o[4]};
}

void replay_emit_nstep_meta(at::Tensor&, at::Tensor&, at::IntArrayRef, const at::Tensor&, const at::Tensor&,
                            at::IntArrayRef, int64_t, int64_t, int64_t, at::ArrayRef<double>, int64_t, int64_t) {}

void train_step_meta(int64_t, at::TensorList, const at::Tensor&, const at::Tensor&, at::IntArrayRef, int64_t,
                     const std::optional<at::Tensor>&, const std::optional<at::Tensor>&) {}

void train_graph_meta(int64_t, at::TensorList, const at::Tensor&, const at::Tensor&, at::IntArrayRef, int64_t,
                      int64_t) {}

std::tuple<at::Tensor, at::Tensor> policy_act_meta(int64_t, const at::Tensor& obs, const std::optional<at::Tensor>& eps,
                                                   int64_t act_dim, bool want_log_pi) {
  const int64_t n = obs.size(0);
  const bool lp = want_log_pi && eps && eps->defined();
  return {at::empty({n, act_dim}, obs.options()), at::empty({lp ? n : 0}, obs.options())};
}

at::Tensor q_values_meta(int64_t, const at::Tensor& obs, const at::Tensor&, bool) {
  return at::empty({obs.size(0), 2}, obs.options());
}

at::Tensor q_values_replay_meta(int64_t, const at::Tensor& storage, const at::Tensor&, at::IntArrayRef, int64_t,
                                int64_t n, bool, bool) {
  return at::empty({n, 2}, storage.options());
}

void envs_reset_meta(at::Tensor&, at::Tensor&, at::Tensor&, at::IntArrayRef, at::ArrayRef<double>, int64_t) {}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> envs_step_meta(
    at::Tensor& obs, at::Tensor&, at::Tensor&, const std::optional<at::Tensor>&, at::IntArrayRef, at::ArrayRef<double>,
    int64_t, const at::Tensor&, int64_t) {
  const int64_t N = obs.size(0), O = obs.size(1);
  auto o = obs.options();
  return {at::empty({N, O}, o), at::empty({N, O}, o), at::empty({N}, o), at::empty({N}, o.dtype(at::kBool)),
          at::empty({N}, o.dtype(at::kBool))};
}

void rollout_step_meta(int64_t, at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&, at::IntArrayRef,
                       at::ArrayRef<double>, int64_t, at::Tensor&, at::Tensor&, at::IntArrayRef, int64_t, int64_t,
                       int64_t, bool, bool) {}

void rollout_step_dev_meta(int64_t, at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&, at::IntArrayRef,
                           at::ArrayRef<double>, int64_t, at::Tensor&, at::Tensor&, at::IntArrayRef, at::Tensor&, int64_t,
                           bool, bool) {}

void q_values_replay_dev_meta(int64_t, const at::Tensor&, const at::Tensor&, at::IntArrayRef, const at::Tensor&, int64_t,
                              int64_t, bool, bool, at::Tensor&) {}

void loop_graph_meta(int64_t, at::TensorList, at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&, at::IntArrayRef,
                     at::ArrayRef<double>, int64_t, at::Tensor&, at::Tensor&, at::IntArrayRef, at::Tensor&,
                     at::IntArrayRef, int64_t, const std::optional<at::Tensor>&) {}

}  // namespace

TORCH_LIBRARY(sac_hip, m) {
  m.def("bind_engine_library(str path) -> ()", &bind_engine_library);
  m.def("replay_push(Tensor(a!) storage, Tensor(b!) state, int[] layout, Tensor rows, int size, int pos) -> ()");
  m.def("replay_gather(Tensor storage, Tensor state, int[] layout, Tensor indices) "
        "-> (Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("replay_sample(Tensor storage, Tensor state, int[] layout, int batch, int seed, int step) -> Tensor");
  m.def("replay_sample_gather(Tensor storage, Tensor state, int[] layout, int batch, int seed, int step) "
        "-> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("replay_emit_nstep(Tensor(a!) storage, Tensor(b!) state, int[] layout, Tensor stage_storage, "
        "Tensor stage_state, int[] stage_layout, int n, int num_envs, int newest, float[] gpow, int size, int pos) "
        "-> ()");
  m.def("replay_emit_nstep_codes(Tensor(a!) storage, Tensor(b!) state, int[] layout, Tensor stage_storage, "
        "Tensor stage_state, int[] stage_layout, int n, int num_envs, int newest, float[] gpow, int size, int pos) "
        "-> ()");
  m.def("engine_set_done_mode(int engine, int mode) -> ()", &engine_set_done_mode);
  m.def("engine_set_action_source(int engine, int source) -> ()", &engine_set_action_source);
  m.def("train_step(int engine, Tensor(a!)[] state, Tensor storage, Tensor replay_state, int[] layout, "
        "int n_steps, Tensor? indices=None, Tensor? eps=None) -> ()");
  m.def("train_graph(int engine, Tensor(a!)[] state, Tensor storage, Tensor replay_state, int[] layout, "
        "int n_steps, int chunk) -> ()");
  m.def("policy_act(int engine, Tensor obs, Tensor? eps, int act_dim, bool want_log_pi=False) -> (Tensor, Tensor)");
  m.def("q_values(int engine, Tensor obs, Tensor act, bool target=False) -> Tensor");
  m.def("q_values_replay(int engine, Tensor storage, Tensor replay_state, int[] layout, int first_slot, int n, "
        "bool next_obs=True, bool target=False) -> Tensor");
  m.def("envs_reset(Tensor(a!) obs, Tensor(b!) counters, Tensor(c!) dstate, int[] icfg, float[] params, int seed) "
        "-> ()");
  m.def("envs_step(Tensor(a!) obs, Tensor(b!) counters, Tensor(c!) dstate, Tensor(d!)? ring, int[] icfg, "
        "float[] params, int seed, Tensor actions, int t) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("rollout_step(int engine, Tensor(a!) obs, Tensor(b!) counters, Tensor(c!) dstate, Tensor(d!) ring, "
        "int[] icfg, float[] params, int seed, Tensor(e!) storage, Tensor(f!) replay_state, int[] layout, "
        "int size, int pos, int t, bool deterministic=False, bool store=True) -> ()");
  m.def("rollout_step_dev(int engine, Tensor(a!) obs, Tensor(b!) counters, Tensor(c!) dstate, Tensor(d!) ring, "
        "int[] icfg, float[] params, int seed, Tensor(e!) storage, Tensor(f!) replay_state, int[] layout, "
        "Tensor(g!) cursor, int parity, bool deterministic=False, bool store=True) -> ()");
  m.def("q_values_replay_dev(int engine, Tensor storage, Tensor replay_state, int[] layout, Tensor cursor, "
        "int parity, int n, bool next_obs, bool target, Tensor(a!) q_ring) -> ()");
  m.def("loop_graph(int engine, Tensor(a!)[] state, Tensor(b!) obs, Tensor(c!) counters, Tensor(d!) dstate, "
        "Tensor(e!) ring, int[] icfg, float[] params, int seed, Tensor(f!) storage, Tensor(g!) replay_state, "
        "int[] layout, Tensor(h!) cursor, int[] grad_steps, int n_replays, Tensor(i!)? q_ring=None) -> ()");
}

TORCH_LIBRARY_IMPL(sac_hip, CUDA, m) {
  m.impl("replay_push", &replay_push);
  m.impl("replay_gather", &replay_gather);
  m.impl("replay_sample", &replay_sample);
  m.impl("replay_sample_gather", &replay_sample_gather);
  m.impl("replay_emit_nstep", &replay_emit_nstep);
  m.impl("replay_emit_nstep_codes", &replay_emit_nstep_codes);
  m.impl("train_step", &train_step);
  m.impl("train_graph", &train_graph);
  m.impl("policy_act", &policy_act);
  m.impl("q_values", &q_values);
  m.impl("q_values_replay", &q_values_replay);
  m.impl("envs_reset", &envs_reset);
  m.impl("envs_step", &envs_step);
  m.impl("rollout_step", &rollout_step);
  m.impl("rollout_step_dev", &rollout_step_dev);
  m.impl("q_values_replay_dev", &q_values_replay_dev);
  m.impl("loop_graph", &loop_graph);
}

TORCH_LIBRARY_IMPL(sac_hip, Meta, m) {
  m.impl("replay_push", &replay_push_meta);
  m.impl("replay_gather", &replay_gather_meta);
  m.impl("replay_sample", &replay_sample_meta);
  m.impl("replay_sample_gather", &replay_sample_gather_meta);
  m.impl("replay_emit_nstep", &replay_emit_nstep_meta);
  m.impl("replay_emit_nstep_codes", &replay_emit_nstep_meta);
  m.impl("train_step", &train_step_meta);
  m.impl("train_graph", &train_graph_meta);
  m.impl("policy_act", &policy_act_meta);
  m.impl("q_values", &q_values_meta);
  m.impl("q_values_replay", &q_values_replay_meta);
  m.impl("envs_reset", &envs_reset_meta);
  m.impl("envs_step", &envs_step_meta);
  m.impl("rollout_step", &rollout_step_meta);
  m.impl("rollout_step_dev", &rollout_step_dev_meta);
  m.impl("q_values_replay_dev", &q_values_replay_dev_meta);
  m.impl("loop_graph", &loop_graph_meta);
}
