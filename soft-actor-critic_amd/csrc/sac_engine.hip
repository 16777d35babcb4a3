// sac_engine.hip — MI355X (gfx950) SAC gradient-step engine, C ABI in
// include/sac_engine.h.  Design notes: DESIGN.md.
//
// One gradient step (reference sac/agent.py:302-327) = 4 launches:
//
//   A  sac_target_critic  row tiles of 16 batch rows, 8 waves.  Device sampler
//                         + replay gather (agent.py:166-193), pi forward on s' and s
//                         (models.py:79-87), target twin-Q and y (agent.py:195-211),
//                         Q1/Q2 forward + backward to every layer's pre-activation
//                         gradient (agent.py:221-234).  Writes X^T / dY^T tiles.
//   B  sac_critic_update  32x32 weight tiles: dW = dY^T X (MFMA over the batch),
//                         Adam (torch single-tensor math), Polyak (agent.py:282-300),
//                         packed compute copies of the new weights.
//   C  sac_actor          row tiles: Q1/Q2 forward on (s, a~) with the UPDATED
//                         critics, min-Q, backward to d a~, squashed-Gaussian head
//                         backward, pi backward (agent.py:238-260).
//   D  sac_actor_update   pi weight tiles + Adam; one extra block runs the float64
//                         alpha update (agent.py:263-280) and reduces the losses.
//
// Weights stay fp32 masters (the nn.Parameter storage); GEMM operands are packed
// compute copies in the MFMA dtype ([out][in] and [in][out], 32-padded) that the
// update kernels rewrite in place, so nothing is re-packed per step.
#include "../../include/sac_engine.h"
#include "../../include/sac_engine_testing.h"

#include <algorithm>
#include <cmath>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#define SAC_VERSION "sac-mi355x 0.1.0"

#include "sac_device.h"
#include "sac_math.h"
#include "sac_phases.h"
#include "sac_split.h"
#include "sac_wide.h"
#include "sac_pairs.h"
#include "sac_envs.h"
#include "sac_nstep.h"
#include "sac_plan.h"

// ============================================================================ params / replay
template <typename T>
__global__ void pack_weights(const float* __restrict__ W, int K, int N, int Kp, int Np, T* __restrict__ Wc,
                             T* __restrict__ WTc) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < Np * Kp; i += gridDim.x * blockDim.x) {
    const int n = i / Kp, k = i % Kp;
    const float v = (n < N && k < K) ? W[(size_t)n * K + k] : 0.f;
    Wc[packed_off<T>(n, k, Kp)] = MM<T>::cvt(v);
    if (WTc) WTc[packed_off<T>(k, n, Np)] = MM<T>::cvt(v);
  }
}

__global__ void replay_push_kernel(sac_replay rb, const float* __restrict__ rows, int64_t n, int64_t skip, int64_t pos,
                                   int64_t new_size, int64_t new_pos) {
  const int O = rb.obs_dim, A = rb.act_dim, W = 2 * O + A + 2;
  const RowStrides rs = row_strides(rb.row_stride, O, A);
  const int64_t total = (n - skip) * W;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t rr = i / W;
    const int c = (int)(i % W);
    const int64_t src = skip + rr;
    const int64_t slot = (pos + src) % rb.capacity;
    const float v = rows[src * W + c];
    if (c < O)
      rb.obs[slot * rs.obs + c] = v;
    else if (c < O + A)
      rb.act[slot * rs.act + (c - O)] = v;
    else if (c == O + A)
      rb.rew[slot * rs.one] = v;
    else if (c < 2 * O + A + 1)
      rb.next_obs[slot * rs.obs + (c - O - A - 1)] = v;
    else
      rb.done[slot * rs.one] = v;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    rb.state[0] = new_size;
    rb.state[1] = new_pos;
    rb.state[2] += 1;  // push generation (a staged batch record of an older generation is stale)
  }
}

// Replay gather by LOGICAL index (reference replay_buffer.py:32-39 +
// agent.py:166-193), one wave per 64 batch rows.  Lane l resolves row b0+l's
// ring slot ONCE (32-bit index load or the device sampler, one conditional
// subtract instead of a 64-bit modulo); then each field is copied
// row-vectorised: the wave's 64 output rows of a field are one contiguous span
// of the SoA output, swept 16 B per lane (4 B when the field width is not a
// multiple of 4 floats), each lane taking its source row's slot from the
// owner lane by a shuffle.  Loads are issued in batches of GATHER_GB before
// their stores (memory-level parallelism: a batch's rows are independent).
#define GATHER_GB 8
template <typename V>
__device__ __forceinline__ void gather_field(const float* __restrict__ src, int W, int64_t stride,
                                             float* __restrict__ dst, int nrow, int64_t slot, int lane) {
  constexpr int EV = sizeof(V) / 4;  // floats per access
  const int Q = W / EV;              // accesses per row
  const int64_t SV = stride / EV;    // accesses between consecutive source rows
  const int total = nrow * Q;
  const V* __restrict__ sv = (const V*)src;
  V* __restrict__ dv = (V*)dst;
  for (int i0 = 0; i0 < total; i0 += 64 * GATHER_GB) {
    V v[GATHER_GB];
    int64_t sl[GATHER_GB];
    int qq[GATHER_GB];
#pragma unroll
    for (int u = 0; u < GATHER_GB; ++u) {
      const int i = min(i0 + u * 64 + lane, total - 1);  // past the end: the last access again
      const int row = (unsigned)i / (unsigned)Q;
      qq[u] = i - row * Q;
      sl[u] = __shfl(slot, row < 64 ? row : 63, 64);  // every lane joins the shuffle
    }
    // loads unconditional: under a per-lane branch each one waited for the one before
#pragma unroll
    for (int u = 0; u < GATHER_GB; ++u)
      if (i0 + u * 64 < total) v[u] = sv[sl[u] * SV + qq[u]];  // wave-uniform test
#pragma unroll
    for (int u = 0; u < GATHER_GB; ++u) {
      const int i = i0 + u * 64 + lane;
      if (i < total) dv[i] = v[u];
    }
  }
}

// Transition-record layout with the standard field order (obs | next_obs |
// act | rew | done at offsets 0, O, 2O, 2O+A, 2O+A+1; O, A multiples of 4;
// row_stride = 4P floats with P | 64): ONE sweep reads each sampled record
// once, 16 B per lane (P lanes per record, 64 / P records per wave
// instruction, padding pieces skipped), and every 16-B piece lands whole in
// one output field.  The field of a lane's piece is the same in every
// iteration (piece = lane % P).
template <bool SAMPLE>
__global__ void __launch_bounds__(256) replay_gather_records_kernel(
    sac_replay rb, const int32_t* __restrict__ idx, int B, FeistelKeys fk, int32_t* __restrict__ idx_out,
    float* __restrict__ s, float* __restrict__ a, float* __restrict__ r, float* __restrict__ s2, float* __restrict__ d,
    int rpw) {
  // rpw rows per wave (64, or 16 for smaller batches: 4x the waves in flight)
  const int lane = threadIdx.x & 63;
  const int b0 = (int)(((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * rpw;
  if (b0 >= B) return;  // whole waves
  const int nrow = B - b0 < rpw ? B - b0 : rpw;
  const int O = rb.obs_dim, A = rb.act_dim;
  const int64_t size = rb.state[0], pos = rb.state[1], cap = rb.capacity;
  int64_t slot = 0;
  if (lane < nrow) {
    int64_t li;
    if (SAMPLE) {
      const Feistel f = feistel_from_keys(fk, size);
      li = feistel_sample(f, b0 + lane, size);
      if (idx_out) idx_out[b0 + lane] = (int32_t)li;
    } else {
      li = idx[b0 + lane];
    }
    const int64_t p = pos + li;
    slot = size < cap ? li : (p >= cap ? p - cap : p);
  }
  const int P = (int)(rb.row_stride >> 2);  // 16-B pieces per record
  const int RPI = 64 / P;                   // records per wave instruction
  const int piece = lane % P, sub = lane / P;
  const int f = 4 * piece;                  // first float of this lane's piece
  const int live = (2 * O + A + 2 + 3) >> 2;  // pieces holding data
  // this lane's destination: field base + column (fixed over the iterations)
  float* dst;
  int dw, col;
  if (f < O) { dst = s; dw = O; col = f; }
  else if (f < 2 * O) { dst = s2; dw = O; col = f - O; }
  else if (f < 2 * O + A) { dst = a; dw = A; col = f - 2 * O; }
  else { dst = nullptr; dw = 0; col = 0; }  // the rew | done piece
  const f32x4* __restrict__ rec = (const f32x4*)rb.obs;
  const int64_t SV = rb.row_stride >> 2;
  const int iters = (nrow + RPI - 1) / RPI;
  const int pcl = piece < live ? piece : live - 1;  // padding pieces re-read the row's last live one
  for (int i0 = 0; i0 < iters; i0 += GATHER_GB) {
    f32x4 v[GATHER_GB];
    int64_t sl[GATHER_GB];
#pragma unroll
    for (int u = 0; u < GATHER_GB; ++u) {
      const int row = (i0 + u) * RPI + sub;
      sl[u] = __shfl(slot, row < 64 ? row : 63, 64);  // rows past nrow: slot 0
    }
    // loads unconditional (no per-lane branch: under one each load waited for the
    // one before, so a wave's rows were fetched one round trip after another)
#pragma unroll
    for (int u = 0; u < GATHER_GB; ++u)
      if (i0 + u < iters) v[u] = rec[sl[u] * SV + pcl];  // wave-uniform test
#pragma unroll
    for (int u = 0; u < GATHER_GB; ++u) {
      const int row = (i0 + u) * RPI + sub;
      if (row < nrow && piece < live) {
        const int b = b0 + row;
        if (dst) {
          // nontemporal output stores: 2.41 -> 3.01 TB/s at B = 1,048,576 (records)
          __builtin_nontemporal_store(v[u], (f32x4*)(dst + (size_t)b * dw + col));
        } else if (f == 2 * O + A) {
          r[b] = v[u][0];
          d[b] = v[u][1];
        }
      }
    }
  }
}

static bool standard_records(const sac_replay* rb) {
  const int64_t W = rb->row_stride;
  const int O = rb->obs_dim, A = rb->act_dim;
  return W > 0 && W <= 256 && (W & (W - 1)) == 0 && W >= 2 * O + A + 2 && (O & 3) == 0 && (A & 3) == 0 &&
         ((uintptr_t)rb->obs & 15) == 0 && rb->next_obs == rb->obs + O && rb->act == rb->obs + 2 * O &&
         rb->rew == rb->act + A && rb->done == rb->rew + 1;
}

template <bool SAMPLE>
__global__ void __launch_bounds__(256) replay_gather_kernel(sac_replay rb, const int32_t* __restrict__ idx, int B,
                                                            FeistelKeys fk, int32_t* __restrict__ idx_out,
                                                            float* __restrict__ s, float* __restrict__ a,
                                                            float* __restrict__ r, float* __restrict__ s2,
                                                            float* __restrict__ d) {
  const int lane = threadIdx.x & 63;
  const int b0 = (int)(((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * 64;
  if (b0 >= B) return;  // whole waves
  const int nrow = B - b0 < 64 ? B - b0 : 64;
  const int O = rb.obs_dim, A = rb.act_dim;
  const int64_t size = rb.state[0], pos = rb.state[1], cap = rb.capacity;
  int64_t slot = 0;
  if (lane < nrow) {
    int64_t li;
    if (SAMPLE) {
      const Feistel f = feistel_from_keys(fk, size);
      li = feistel_sample(f, b0 + lane, size);
      if (idx_out) idx_out[b0 + lane] = (int32_t)li;
    } else {
      li = idx[b0 + lane];
    }
    const int64_t p = pos + li;  // li < size <= cap, pos < cap
    slot = size < cap ? li : (p >= cap ? p - cap : p);
  }
  // transition records: the five sweeps read the same 64 records, so after the
  // first sweep's misses the others hit the lines in L2
  const RowStrides rs = row_strides(rb.row_stride, O, A);
  auto a16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  if ((O & 3) == 0 && (rs.obs & 3) == 0 && a16(rb.obs) && a16(rb.next_obs)) {
    gather_field<f32x4>(rb.obs, O, rs.obs, s + (size_t)b0 * O, nrow, slot, lane);
    gather_field<f32x4>(rb.next_obs, O, rs.obs, s2 + (size_t)b0 * O, nrow, slot, lane);
  } else {
    gather_field<float>(rb.obs, O, rs.obs, s + (size_t)b0 * O, nrow, slot, lane);
    gather_field<float>(rb.next_obs, O, rs.obs, s2 + (size_t)b0 * O, nrow, slot, lane);
  }
  if ((A & 3) == 0 && (rs.act & 3) == 0 && a16(rb.act))
    gather_field<f32x4>(rb.act, A, rs.act, a + (size_t)b0 * A, nrow, slot, lane);
  else
    gather_field<float>(rb.act, A, rs.act, a + (size_t)b0 * A, nrow, slot, lane);
  if (lane < nrow) {
    r[b0 + lane] = rb.rew[slot * rs.one];
    d[b0 + lane] = rb.done[slot * rs.one];
  }
}

// The eps draws of one step exactly as the fused step makes them in its default
// (device RNG) mode: out[which][b][j] = philox_normal2(seed, step, b, which,
// j / 2), component j % 2 (sac_phases.h / sac_split.h eps loops).
__host__ __device__ inline void eps_pair(uint64_t seed, uint64_t step, int b, int which, int p, int B, int A,
                                         float* out) {
  float n0, n1;
  philox_normal2(seed, step, (uint32_t)b, (uint32_t)which, (uint32_t)p, n0, n1);
  float* o = out + ((size_t)which * B + b) * A;
  o[2 * p] = n0;
  if (2 * p + 1 < A) o[2 * p + 1] = n1;
}
__global__ void eps_draw_kernel(uint64_t seed, uint64_t step, int B, int A, float* __restrict__ out) {
  const int NP = (A + 1) / 2;
  const int64_t n = 2LL * B * NP;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int p = (int)(i % NP);
    const int64_t rw = i / NP;
    eps_pair(seed, step, (int)(rw % B), (int)(rw / B), p, B, A, out);
  }
}

__global__ void replay_sample_kernel(const int64_t* __restrict__ state, int B, FeistelKeys fk, int32_t* __restrict__ out) {
  const int64_t size = state[0];
  const Feistel f = feistel_from_keys(fk, size);
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x)
    out[b] = (int32_t)feistel_sample(f, b, size);
}

// ============================================================================ host side
static thread_local std::string g_err;
static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
#define HIPCHK(x)                                                                                  \
  do {                                                                                             \
    hipError_t _e = (x);                                                                           \
    if (_e != hipSuccess) return fail(SAC_E_HIP, std::string(#x ": ") + hipGetErrorString(_e));    \
  } while (0)

static int validate(const sac_engine_config* c) {
  if (!c) return fail(SAC_E_INVALID, "null config");
  if (c->obs_dim < 1 || c->act_dim < 1 || c->act_dim > 32) return fail(SAC_E_INVALID, "obs_dim >= 1, 1 <= act_dim <= 32");
  if (c->batch < 1 || c->batch > (1 << 20)) return fail(SAC_E_INVALID, "batch out of range");
  if (c->q_layers < 2 || c->q_layers > SAC_DEV_LAYERS || c->pi_layers < 2 || c->pi_layers > SAC_DEV_LAYERS)
    return fail(SAC_E_INVALID, "networks need 1..5 hidden layers");
  if (c->q_dims[0] != c->obs_dim + c->act_dim || c->q_dims[c->q_layers] != 1)
    return fail(SAC_E_INVALID, "q_dims must run obs+act -> ... -> 1");
  if (c->pi_dims[0] != c->obs_dim || c->pi_dims[c->pi_layers] != 2 * c->act_dim)
    return fail(SAC_E_INVALID, "pi_dims must run obs -> ... -> 2*act");
  for (int i = 0; i <= c->q_layers; ++i)
    if (c->q_dims[i] < 1) return fail(SAC_E_INVALID, "bad q dim");
  for (int i = 0; i <= c->pi_layers; ++i)
    if (c->pi_dims[i] < 1) return fail(SAC_E_INVALID, "bad pi dim");
  const int acts[4] = {c->q_hidden_act, c->q_out_act, c->pi_hidden_act, c->pi_out_act};
  for (int a : acts)
    if (a < 0 || a > 6) return fail(SAC_E_INVALID, "bad activation code");
  if (c->precision != SAC_PREC_FP32 && c->precision != SAC_PREC_BF16) return fail(SAC_E_INVALID, "bad precision");
  if (c->layout < SAC_LAYOUT_AUTO || c->layout > SAC_LAYOUT_PAIRS || c->stage_path < -1 || c->stage_path > 1 ||
      c->stage_batch < -1 || c->stage_batch > 0 || c->upd_parts < 0 || c->upd_parts > 4 ||
      (c->upd_threads != 0 && c->upd_threads != 512 && c->upd_threads != 1024))
    return fail(SAC_E_INVALID, "bad layout override (layout 0..3, stage_path -1..1, stage_batch -1..0, "
                               "upd_parts 0..4, upd_threads 0 / 512 / 1024)");
  return SAC_OK;
}

// The rollout kernels' instantiation for the class of a kind (sac_envs.h with_env_class)
template <typename T>
static auto rollout_kernel(int kind) {
  return with_env_class(kind, [](auto kc) { return sac_rollout_step_kernel<T, decltype(kc)::value>; });
}
template <typename T>
static auto rollout_dev_kernel(int kind) {
  return with_env_class(kind, [](auto kc) { return sac_rollout_step_dev_kernel<T, decltype(kc)::value>; });
}

static auto rollout_uniform_kernel(int kind) {
  return with_env_class(kind, [](auto kc) { return sac_rollout_uniform_kernel<decltype(kc)::value>; });
}
static auto rollout_uniform_dev_kernel(int kind) {
  return with_env_class(kind, [](auto kc) { return sac_rollout_uniform_dev_kernel<decltype(kc)::value>; });
}

template <typename T>
static void set_lds_attrs(size_t bytes) {
  (void)bytes;
  const int b = 160 * 1024;  // the launch passes what it needs; the attribute is the cap
  (void)hipFuncSetAttribute((const void*)sac_target_critic<T, false>, hipFuncAttributeMaxDynamicSharedMemorySize, b);
  (void)hipFuncSetAttribute((const void*)sac_target_critic<T, true>, hipFuncAttributeMaxDynamicSharedMemorySize, b);
  (void)hipFuncSetAttribute((const void*)sac_actor<T, false>, hipFuncAttributeMaxDynamicSharedMemorySize, b);
  (void)hipFuncSetAttribute((const void*)sac_actor<T, true>, hipFuncAttributeMaxDynamicSharedMemorySize, b);
  (void)hipFuncSetAttribute((const void*)sac_policy_act_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, b);
  for (int kind : ENV_CLASS_KINDS) {
    (void)hipFuncSetAttribute((const void*)rollout_kernel<T>(kind), hipFuncAttributeMaxDynamicSharedMemorySize, b);
    (void)hipFuncSetAttribute((const void*)rollout_dev_kernel<T>(kind), hipFuncAttributeMaxDynamicSharedMemorySize, b);
  }
  (void)hipFuncSetAttribute((const void*)sac_q_values_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, b);
  (void)hipFuncSetAttribute((const void*)sac_target_critic_split<T>, hipFuncAttributeMaxDynamicSharedMemorySize, b);
  (void)hipFuncSetAttribute((const void*)sac_target_critic_pairs<T>, hipFuncAttributeMaxDynamicSharedMemorySize, b);
  (void)hipFuncSetAttribute((const void*)sac_actor_pairs<T>, hipFuncAttributeMaxDynamicSharedMemorySize, b);
  (void)hipFuncSetAttribute((const void*)sac_actor_split<T>, hipFuncAttributeMaxDynamicSharedMemorySize, b);
  // the 1024-thread update kernels hold the K-quarter partials in static LDS: the cap is on the dynamic block
  const int bu = b - SAC_UPD_PART_BYTES;
  (void)hipFuncSetAttribute((const void*)sac_critic_update<T>, hipFuncAttributeMaxDynamicSharedMemorySize, bu);
  (void)hipFuncSetAttribute((const void*)sac_critic_update<T, 512>, hipFuncAttributeMaxDynamicSharedMemorySize, b);
  (void)hipFuncSetAttribute((const void*)sac_actor_update<T>, hipFuncAttributeMaxDynamicSharedMemorySize, bu);
  (void)hipFuncSetAttribute((const void*)sac_wide_stage<T, WA_PLAIN, false>, hipFuncAttributeMaxDynamicSharedMemorySize, b);
  (void)hipFuncSetAttribute((const void*)sac_wide_stage<T, WA_ACT, false>, hipFuncAttributeMaxDynamicSharedMemorySize, b);
  (void)hipFuncSetAttribute((const void*)sac_wide_stage<T, WA_OUTBWD, false>, hipFuncAttributeMaxDynamicSharedMemorySize, b);
  (void)hipFuncSetAttribute((const void*)sac_wide_stage<T, WA_PLAIN, true>, hipFuncAttributeMaxDynamicSharedMemorySize, b);
  (void)hipFuncSetAttribute((const void*)sac_wide_stage<T, WA_ACT, true>, hipFuncAttributeMaxDynamicSharedMemorySize, b);
  (void)hipFuncSetAttribute((const void*)sac_wide_stage<T, WA_OUTBWD, true>, hipFuncAttributeMaxDynamicSharedMemorySize, b);
  (void)hipFuncSetAttribute((const void*)sac_wide_gather<T>, hipFuncAttributeMaxDynamicSharedMemorySize, b);
  (void)hipFuncSetAttribute((const void*)sac_wide_head<T>, hipFuncAttributeMaxDynamicSharedMemorySize, b);
}

// empty kernel: the dispatch + event gap of sac_engine_time_phases
__global__ void sac_noop_kernel() {}
// one wave spinning `ticks` of the 100 MHz realtime clock: holds the stream
// while the host enqueues a timed sequence, so its launches run back to back
// at device speed instead of host-submission speed
__global__ void sac_spin_kernel(long long ticks) {
  const long long t0 = __builtin_amdgcn_s_memrealtime();
  while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}

// fn<T>(args) with T the engine's MFMA operand type: the one precision fork of
// the step's launches.  (A macro, not a template over a generic lambda: the
// kernels are instantiated in the order these forks name them, and the code
// object lists them in that order.)
#define BY_PRECISION(e, fn, ...) \
  ((e)->cfg.precision == SAC_PREC_BF16 ? fn<bf16>(__VA_ARGS__) : fn<float>(__VA_ARGS__))

// One phase launch of the row-tile / role / pair paths (and B, D of the stage
// path): the kernel of the engine's path on the geometry plan_launches() made.
template <typename T>
static void launch_kind(sac_engine* e, int kind, const sac_replay* rb, const int32_t* idx, const float* eps,
                        hipStream_t s) {
  const PhaseLaunch& L = e->launch[kind];
  switch (kind) {
    case L_A:
      switch (e->path) {
        case PATH_SPLIT: sac_target_critic_split<T><<<L.grid, L.threads, L.lds, s>>>(e->d, *rb, idx, eps); break;
        case PATH_ROLES: sac_target_critic<T, true><<<L.grid, L.threads, L.lds, s>>>(e->d, *rb, idx, eps); break;
        case PATH_PAIRS: sac_target_critic_pairs<T><<<L.grid, L.threads, L.lds, s>>>(e->d, *rb, idx, eps); break;
        case PATH_ROWS: sac_target_critic<T, false><<<L.grid, L.threads, L.lds, s>>>(e->d, *rb, idx, eps); break;
        case PATH_WIDE: break;  // its stages: launch_wide
      }
      break;
    case L_B:
      if (L.threads == 512)
        sac_critic_update<T, 512><<<L.grid, 512, L.lds, s>>>(e->d, e->tilesB);
      else
        sac_critic_update<T><<<L.grid, L.threads, L.lds, s>>>(e->d, e->tilesB);
      break;
    case L_C:
      switch (e->path) {
        case PATH_SPLIT: sac_actor_split<T><<<L.grid, L.threads, L.lds, s>>>(e->d, *rb); break;
        case PATH_ROLES: sac_actor<T, true><<<L.grid, L.threads, L.lds, s>>>(e->d, *rb); break;
        case PATH_PAIRS: sac_actor_pairs<T><<<L.grid, L.threads, L.lds, s>>>(e->d, *rb); break;
        case PATH_ROWS: sac_actor<T, false><<<L.grid, L.threads, L.lds, s>>>(e->d, *rb); break;
        case PATH_WIDE: break;
      }
      break;
    case L_D:
      sac_actor_update<T><<<L.grid, L.threads, L.lds, s>>>(e->d, e->tilesD, e->nD);
      break;
  }
}

// One launch of the large-batch stage path (sac_wide.h).
template <typename T>
static void launch_wide_stage(sac_engine* e, const sac_engine::WStage& st, const sac_replay* rb, const int32_t* idx,
                              const float* eps, hipStream_t s, bool stage_next, const int32_t* next_idx) {
  const size_t glds = (size_t)((WGR * (e->cfg.obs_dim + e->cfg.act_dim) + 1) & ~1) * 4 + WGR * 8;
  switch (st.kind) {
    case 0:
      sac_wide_gather<T><<<st.grid, WG_T, glds, s>>>(e->d, e->wdd, *rb, idx);
      break;
    case 1: {
      // the last phase-C stage also gathers the next step's batch (when there is one in this call)
      const int ng = st.last && stage_next ? (e->cfg.batch + WGR - 1) / WGR : 0;
      const int flags = st.last | (&st == &e->wst[1] ? 2 : 0) | (ng ? 4 : 0) | (int)((&st - e->wst.data()) << 8);
      const bool relu = e->cfg.q_hidden_act == ACT_RELU && e->cfg.pi_hidden_act == ACT_RELU;
      const int am = e->hostW[st.j0].amode;  // one A-operand mode per stage (build_wide)
      auto k = relu ? (am == WA_PLAIN ? sac_wide_stage<T, WA_PLAIN, true>
                       : am == WA_ACT ? sac_wide_stage<T, WA_ACT, true> : sac_wide_stage<T, WA_OUTBWD, true>)
                    : (am == WA_PLAIN ? sac_wide_stage<T, WA_PLAIN, false>
                       : am == WA_ACT ? sac_wide_stage<T, WA_ACT, false> : sac_wide_stage<T, WA_OUTBWD, false>);
      k<<<st.grid + ng, WG_T, std::max(st.lds, ng ? glds : 0), s>>>(e->d, e->wdd, e->wjobs + st.j0, st.j1 - st.j0,
                                                                    flags, st.grid, *rb, next_idx);
      break;
    }
    case 2:
      sac_wide_head<T><<<st.grid, WG_T, 0, s>>>(e->d, e->wdd, eps);
      break;
    case 3:
      launch_kind<T>(e, L_B, rb, idx, eps, s);
      break;
    case 4:
      launch_kind<T>(e, L_D, rb, idx, eps, s);
      break;
  }
}
static void launch_wide(sac_engine* e, const sac_engine::WStage& st, const sac_replay* rb, const int32_t* idx,
                        const float* eps, hipStream_t s, bool stage_next = false, const int32_t* next_idx = nullptr) {
  BY_PRECISION(e, launch_wide_stage, e, st, rb, idx, eps, s, stage_next, next_idx);
}

// What time_phases keeps of a launch: its phase and an event after it.
static void after_launch(int phase, hipStream_t s, std::vector<int>* kinds, std::vector<hipEvent_t>* ev) {
  if (kinds) kinds->push_back(phase);
  if (ev) {
    hipEvent_t x;
    (void)hipEventCreate(&x);
    (void)hipEventRecord(x, s);
    ev->push_back(x);
  }
}

// The launches of n consecutive steps (and, per launch, its kind in *kinds).
static void launch_steps(sac_engine* e, const sac_replay* rb, int n, const int32_t* indices, const float* eps,
                         hipStream_t s, std::vector<int>* kinds = nullptr, std::vector<hipEvent_t>* ev = nullptr) {
  const size_t B = e->cfg.batch, A = e->cfg.act_dim;
  for (int i = 0; i < n; ++i) {
    const int32_t* ix = indices ? indices + (size_t)i * B : nullptr;
    const float* ep = eps ? eps + (size_t)i * 2 * B * A : nullptr;
    if (e->path != PATH_WIDE) {
      for (int k = L_A; k <= L_D; ++k) {
        BY_PRECISION(e, launch_kind, e, k, rb, ix, ep, s);
        after_launch(k, s, kinds, ev);
      }
      continue;
    }
    // the stage sequence of sac_wide.h: step i > 0 of the call uses the batch
    // step i - 1 gathered in its last phase-C stage
    const bool next = i + 1 < n;
    const int32_t* nix = indices && next ? indices + (size_t)(i + 1) * B : nullptr;
    for (const sac_engine::WStage& st : e->wst) {
      if (st.kind == 0 && i > 0) continue;
      launch_wide(e, st, rb, ix, ep, s, next, nix);
      after_launch(st.phase, s, kinds, ev);
    }
  }
}

static int check_replay(sac_engine* e, const sac_replay* rb) {
  if (!rb || !rb->obs || !rb->act || !rb->rew || !rb->next_obs || !rb->done || !rb->state)
    return fail(SAC_E_INVALID, "null replay buffer");
  if (rb->obs_dim != e->cfg.obs_dim || rb->act_dim != e->cfg.act_dim)
    return fail(SAC_E_INVALID, "replay dims do not match the engine");
  if (rb->capacity < e->cfg.batch) return fail(SAC_E_NOT_ENOUGH, "replay capacity smaller than the batch");
  return SAC_OK;
}

// Configuration first, then pointers: the messages of a bad configuration do not
// depend on the state being allocated.
static int check_envs(const sac_envs* ev, bool need_ring) {
  if (!ev) return fail(SAC_E_INVALID, "null environments");
  const sac_env_config& c = ev->cfg;
  // a control task's enumerator (sac_envs.h EnvTask), NULL for the probes and for an unknown kind
  const char* task = with_env_class(c.kind, [](auto kc) -> const char* {
    if constexpr (decltype(kc)::value != ENV_CLASS_PROBES) return EnvTask<decltype(kc)::value>::NAME;
    return nullptr;
  });
  if ((c.kind < SAC_ENV_CONSTANT_REWARD || c.kind > SAC_ENV_POINT_MASS) && !task)
    return fail(SAC_E_INVALID, "unknown environment kind " + std::to_string(c.kind));
  if (c.num_envs < 1) return fail(SAC_E_INVALID, "num_envs >= 1");
  if (c.max_steps < 1) return fail(SAC_E_INVALID, "max_steps >= 1");
  const int obs_dim = SAC_ENV_OBS_DIM(c.kind);  // 0: the caller's
  if (task && c.obs_dim != obs_dim)
    return fail(SAC_E_INVALID, "obs_dim must be " + std::to_string(obs_dim) + " for " + task);
  if (!task && (obs_dim ? c.obs_dim != obs_dim : (c.obs_dim < 1 || c.obs_dim > 4 * 65536)))
    return fail(SAC_E_INVALID, "obs_dim must be 1 (SAC_ENV_RANDOM_OBS: 1..262144)");
  if (!ev->obs || !ev->step || !ev->ep_length || !ev->pos || !ev->ep_return ||
      (SAC_ENV_VEL_ROWS(c.kind) && !ev->vel))
    return fail(SAC_E_INVALID, "null environment state");
  if (need_ring ? (!ev->episodes || ev->ring_steps < 1) : (ev->episodes && ev->ring_steps < 1))
    return fail(SAC_E_INVALID, "episode ring needs episodes != NULL and ring_steps >= 1");
  return SAC_OK;
}

// An explicit layout override the planner could not honour (choose_path).
static int fail_refused(const char* refused) {
  return fail(SAC_E_INVALID, std::string("layout override cannot be honoured: ") + refused);
}

// What sac_engine_create refuses of a finished plan, before its first HIP call.
static int check_plan(const sac_engine* e) {
  const sac_engine_config* c = &e->cfg;
  if (std::max(e->lds_bytes, e->upd_lds) > 160 * 1024) {
    const size_t lb = e->lds_bytes;
    return fail(SAC_E_INVALID, "layer widths need " + std::to_string(lb) + " B of LDS per workgroup (max 163840)");
  }
  if (e->path == PATH_WIDE) {
    // the stage launches' LDS, and the batch gather's [WGR][obs + act] rows + slots
    size_t mx = (size_t)((WGR * (c->obs_dim + c->act_dim) + 1) & ~1) * 4 + WGR * 8;
    for (const sac_engine::WStage& st : e->wst) mx = std::max(mx, st.lds);
    if (e->hostW.size() > WIDE_MAX_JOBS || mx > 160 * 1024) {
      const std::string m = "internal: stage path plans " + std::to_string(e->hostW.size()) + " jobs, " +
                            std::to_string(mx) + " B of LDS";
      return fail(SAC_E_INVALID, m);
    }
  }
  if ((int)e->hostB.size() != e->nB || (int)e->hostD.size() != e->nD) {  // the grids launch nB / nD tiles
    const std::string m = "internal: update tiles planned " + std::to_string(e->nB) + " / " + std::to_string(e->nD) +
                          ", built " + std::to_string(e->hostB.size()) + " / " + std::to_string(e->hostD.size());
    return fail(SAC_E_INVALID, m);
  }
  return SAC_OK;
}

// What the control tasks' sac_debug_*_step_host / *_reset_host exports share, behind each one's own null
// checks; `terminated` may be NULL
template <int KC>
static int task_step_host(const std::string& who, const sac_env_config* cfg, double* state, int32_t step,
                          const float* action, float* obs_out, double* reward, int32_t* terminated,
                          int32_t* truncated) {
  using Task = EnvTask<KC>;
  if (cfg->kind != Task::KIND) return fail(SAC_E_INVALID, who + ": kind must be " + Task::NAME);
  if (cfg->max_steps < 1 || step < 0) return fail(SAC_E_INVALID, who + ": max_steps >= 1 and step >= 0");
  EnvOut o;
  Task::dynamics(state, action, *cfg, obs_out, o);
  *reward = o.reward;
  if (terminated) *terminated = o.terminated ? 1 : 0;
  *truncated = step + 1 >= cfg->max_steps ? 1 : 0;
  return SAC_OK;
}
template <int KC>
static int task_reset_host(uint64_t seed, uint64_t t, int32_t row, double* state_out) {
  if (!state_out || row < 0) return fail(SAC_E_INVALID, "need row >= 0 and state_out != NULL");
  EnvTask<KC>::reset_draw(seed, t, (uint32_t)row, state_out);
  return SAC_OK;
}

extern "C" {

const char* sac_last_error(void) { return g_err.c_str(); }
const char* sac_version(void) { return SAC_VERSION; }

size_t sac_engine_workspace_bytes(const sac_engine_config* cfg) {
  if (validate(cfg) != SAC_OK) return 0;
  return plan(cfg, nullptr, nullptr).bytes;  // also of a refused override: create reports that
}

const char* sac_phase_kernel_name(int32_t phase) {
  switch (phase) {
    case 0: return "sac_target_critic";
    case 1: return "sac_critic_update";
    case 2: return "sac_actor";
    case 3: return "sac_actor_update";
    default: return "";
  }
}

int sac_engine_sync_params(sac_engine* e, void* stream) {
  if (!e) return fail(SAC_E_INVALID, "null engine");
  hipStream_t s = (hipStream_t)stream;
  const bool bf = e->cfg.precision == SAC_PREC_BF16;
  for (int ni = 0; ni < 5; ++ni) {
    const NetDev& nd = e->h.net[ni];
    for (int l = 0; l < nd.L; ++l) {
      const LayerDev& ly = nd.l[l];
      const int blocks = std::min(1024, (ly.Np * ly.Kp + 255) / 256);
      if (bf)
        pack_weights<bf16><<<blocks, 256, 0, s>>>(nd.P + ly.w_off, ly.K, ly.N, ly.Kp, ly.Np, (bf16*)ly.Wc, (bf16*)ly.WTc);
      else
        pack_weights<float><<<blocks, 256, 0, s>>>(nd.P + ly.w_off, ly.K, ly.N, ly.Kp, ly.Np, (float*)ly.Wc,
                                                   (float*)ly.WTc);
    }
  }
  HIPCHK(hipGetLastError());
  return SAC_OK;
}

int sac_engine_create(const sac_engine_config* cfg, const sac_engine_buffers* buf, void* stream, sac_engine** out) {
  if (!out || !buf) return fail(SAC_E_INVALID, "null argument");
  *out = nullptr;
  int rc = validate(cfg);
  if (rc) return rc;
  const PlanSize sized = plan(cfg, nullptr, nullptr);
  const size_t need = sized.bytes;
  if (!buf->workspace || buf->workspace_bytes < need)
    return fail(SAC_E_INVALID, "workspace too small: need " + std::to_string(need) + " bytes");
  if (((uintptr_t)buf->workspace) & 255) return fail(SAC_E_INVALID, "workspace must be 256-byte aligned");
  if (!buf->pi || !buf->q1 || !buf->q2 || !buf->q1t || !buf->q2t || !buf->pi_m || !buf->pi_v || !buf->q1_m ||
      !buf->q1_v || !buf->q2_m || !buf->q2_v || !buf->alpha_state || !buf->opt_steps || !buf->rng_step || !buf->stats)
    return fail(SAC_E_INVALID, "null device buffer");
  if (sized.refused) return fail_refused(sized.refused);
  sac_engine* e = new sac_engine();
  e->cfg = *cfg;
  e->buf = *buf;
  {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
      e->ncu = n;
  }
  plan(cfg, e, (char*)buf->workspace);
  rc = check_plan(e);
  if (rc) {
    delete e;
    return rc;
  }
  if (cfg->precision == SAC_PREC_BF16)
    set_lds_attrs<bf16>(e->lds_bytes);
  else
    set_lds_attrs<float>(e->lds_bytes);
  hipStream_t s = (hipStream_t)stream;
  hipError_t err = hipMemsetAsync(buf->workspace, 0, buf->workspace_bytes, s);
  if (err == hipSuccess) err = hipMemcpyAsync(e->d, &e->h, sizeof(EngineDev), hipMemcpyHostToDevice, s);
  if (err == hipSuccess) err = hipMemcpyAsync(e->tilesB, e->hostB.data(), e->hostB.size() * sizeof(TileDesc), hipMemcpyHostToDevice, s);
  if (err == hipSuccess) err = hipMemcpyAsync(e->tilesD, e->hostD.data(), e->hostD.size() * sizeof(TileDesc), hipMemcpyHostToDevice, s);
  const bool wide = e->path == PATH_WIDE;
  if (err == hipSuccess && wide) err = hipMemcpyAsync(e->wdd, &e->wdh, sizeof(WideDev), hipMemcpyHostToDevice, s);
  if (err == hipSuccess && wide)
    err = hipMemcpyAsync(e->wjobs, e->hostW.data(), e->hostW.size() * sizeof(WJob), hipMemcpyHostToDevice, s);
  if (err == hipSuccess) err = hipStreamSynchronize(s);
  if (err != hipSuccess) {
    delete e;
    return fail(SAC_E_HIP, std::string("engine upload: ") + hipGetErrorString(err));
  }
  rc = sac_engine_sync_params(e, stream);
  if (rc) {
    delete e;
    return rc;
  }
  *out = e;
  return SAC_OK;
}

int sac_engine_set_alpha_update(sac_engine* e, int32_t enabled, void* stream) {
  if (!e) return fail(SAC_E_INVALID, "null engine");
  e->h.alpha_update = enabled ? 1 : 0;
  HIPCHK(hipMemcpyAsync((char*)e->d + offsetof(EngineDev, alpha_update), &e->h.alpha_update, sizeof(int),
                        hipMemcpyHostToDevice, (hipStream_t)stream));
  return SAC_OK;
}

int sac_engine_set_done_mode(sac_engine* e, int32_t mode) {
  if (mode < SAC_DONE_ANY_END || mode > SAC_DONE_END_CODE)
    return fail(SAC_E_INVALID, "set_done_mode: mode (" + std::to_string(mode) + ") outside 0..2");
  if (!e) return fail(SAC_E_INVALID, "set_done_mode: null engine");
  e->done_mode = mode;
  return SAC_OK;
}

int sac_engine_set_action_source(sac_engine* e, int32_t source) {
  if (source < SAC_ACTIONS_POLICY || source > SAC_ACTIONS_UNIFORM)
    return fail(SAC_E_INVALID, "set_action_source: source (" + std::to_string(source) + ") outside 0..1");
  if (!e) return fail(SAC_E_INVALID, "set_action_source: null engine");
  e->action_source = source;
  return SAC_OK;
}

int sac_engine_check(sac_engine* e, void* stream) {
  if (!e) return fail(SAC_E_INVALID, "null engine");
  uint32_t w[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(w, e->h.sync, sizeof(w), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  if (w[1]) return fail(SAC_E_HIP, "a workgroup hand-off timed out: results of the affected steps are invalid");
  return SAC_OK;
}

int sac_engine_debug_staged_step(sac_engine* e, uint64_t* step_out, void* stream) {
  if (!e || !step_out) return fail(SAC_E_INVALID, "bad debug_staged_step arguments");
  HIPCHK(hipMemcpyAsync(step_out, e->h.sync + SYNC_STAGED, sizeof(uint64_t), hipMemcpyDeviceToHost,
                        (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return SAC_OK;
}

void sac_engine_destroy(sac_engine* e) {
  if (!e) return;
  if (e->gexec) (void)hipGraphExecDestroy(e->gexec);
  if (e->graph) (void)hipGraphDestroy(e->graph);
  if (e->lgexec) (void)hipGraphExecDestroy(e->lgexec);
  if (e->lgraph) (void)hipGraphDestroy(e->lgraph);
  if (e->cap) (void)hipStreamDestroy(e->cap);
  delete e;
}

int sac_engine_train(sac_engine* e, const sac_replay* rb, int32_t n_steps, const int32_t* indices, const float* eps,
                     void* stream) {
  if (!e) return fail(SAC_E_INVALID, "null engine");
  int rc = check_replay(e, rb);
  if (rc) return rc;
  launch_steps(e, rb, n_steps, indices, eps, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return SAC_OK;
}

int sac_engine_train_graph(sac_engine* e, const sac_replay* rb, int32_t n_steps, int32_t chunk, void* stream) {
  if (!e) return fail(SAC_E_INVALID, "null engine");
  int rc = check_replay(e, rb);
  if (rc) return rc;
  if (chunk < 1) return fail(SAC_E_INVALID, "chunk >= 1");
  hipStream_t s = (hipStream_t)stream;
  const bool same = e->gexec && e->gchunk == chunk && !memcmp(&e->gkey, rb, sizeof(sac_replay));
  if (!same && (n_steps >= chunk || n_steps == 0)) {  // n_steps == 0: capture only
    if (e->gexec) (void)hipGraphExecDestroy(e->gexec);
    if (e->graph) (void)hipGraphDestroy(e->graph);
    e->gexec = nullptr;
    e->graph = nullptr;
    if (!e->cap) HIPCHK(hipStreamCreateWithFlags(&e->cap, hipStreamNonBlocking));
    HIPCHK(hipStreamBeginCapture(e->cap, hipStreamCaptureModeThreadLocal));
    launch_steps(e, rb, chunk, nullptr, nullptr, e->cap);
    HIPCHK(hipStreamEndCapture(e->cap, &e->graph));
    HIPCHK(hipGraphInstantiate(&e->gexec, e->graph, nullptr, nullptr, 0));
    // device-side setup of the executable graph now, on the caller's stream,
    // not inside its first replay (the timed region of a short run)
    HIPCHK(hipGraphUpload(e->gexec, s));
    e->gchunk = chunk;
    e->gkey = *rb;
  }
  int done = 0;
  if (e->gexec)
    for (; done + chunk <= n_steps; done += chunk) HIPCHK(hipGraphLaunch(e->gexec, s));
  if (done < n_steps) launch_steps(e, rb, n_steps - done, nullptr, nullptr, s);
  HIPCHK(hipGetLastError());
  return SAC_OK;
}

// The forward-only kernels (policy_act, rollout_step, q_values) run one network
// on the row-tile LDS layout: plan() sizes ld / ldo over all five networks, so
// this holds for every engine create accepts; it is checked where it is relied on.
static bool rowtile_fits(const sac_engine* e, int net) {
  const EngineDev& h = e->h;
  const NetDev& q = h.net[net];
  for (int l = 0; l < q.L; ++l) {
    if (q.l[l].Kp + 4 > h.ld) return false;
    if (l == q.L - 1 ? q.l[l].Np + 4 > h.ldo : q.l[l].Np + 4 > h.ld) return false;
  }
  const size_t ends[4] = {(size_t)h.o_X + SAC_ROWS * h.ld, (size_t)h.o_Y + SAC_ROWS * h.ld,
                          (size_t)h.o_out + SAC_ROWS * h.ldo, (size_t)h.o_outp + SAC_ROWS * h.ldo};
  return *std::max_element(ends, ends + 4) * 4 <= e->lds_bytes && e->lds_bytes <= 160 * 1024;
}

// what a launch of the policy's forward-only kernels needs of the engine
static int check_policy_forward(const sac_engine* e, const char* who) {
  if (!e->d)
    return fail(SAC_E_INVALID, std::string(who) + ": the engine has no device state (host-only test engine)");
  if (!rowtile_fits(e, NET_PI))
    return fail(SAC_E_INVALID, std::string(who) + ": the row-tile LDS layout does not hold the policy's layer widths");
  return SAC_OK;
}

int sac_policy_act(sac_engine* e, const float* obs, int32_t n, const float* eps, float* action, float* log_pi,
                   void* stream) {
  if (!e || !obs || !action || n < 1) return fail(SAC_E_INVALID, "bad policy_act arguments");
  int rc = check_policy_forward(e, "policy_act");
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = (n + SAC_ROWS - 1) / SAC_ROWS;
  if (e->cfg.precision == SAC_PREC_BF16)
    sac_policy_act_kernel<bf16><<<blocks, SAC_THREADS, e->lds_bytes, s>>>(e->d, obs, n, eps, action, log_pi);
  else
    sac_policy_act_kernel<float><<<blocks, SAC_THREADS, e->lds_bytes, s>>>(e->d, obs, n, eps, action, log_pi);
  HIPCHK(hipGetLastError());
  return SAC_OK;
}

// what a launch of the critic-evaluation kernel needs of the engine
static int check_q_forward(const sac_engine* e) {
  if (!e->d) return fail(SAC_E_INVALID, "q_values: the engine has no device state (host-only test engine)");
  if (!rowtile_fits(e, NET_Q1))
    return fail(SAC_E_INVALID, "q_values: the row-tile LDS layout does not hold the critics' layer widths");
  return SAC_OK;
}

// every argument validated by the caller; one launch, no host-side state
static int launch_q_values(sac_engine* e, const QRows& rows, int32_t n, int32_t target, float* q, void* stream) {
  const int rc = check_q_forward(e);
  if (rc) return rc;
  const dim3 grid((unsigned)((n + SAC_ROWS - 1) / SAC_ROWS), 2);
  hipStream_t s = (hipStream_t)stream;
  if (e->cfg.precision == SAC_PREC_BF16)
    sac_q_values_kernel<bf16><<<grid, SAC_THREADS, e->lds_bytes, s>>>(e->d, rows, n, target ? 1 : 0, q);
  else
    sac_q_values_kernel<float><<<grid, SAC_THREADS, e->lds_bytes, s>>>(e->d, rows, n, target ? 1 : 0, q);
  HIPCHK(hipGetLastError());
  return SAC_OK;
}

int sac_q_values(sac_engine* e, const float* obs, int64_t obs_stride, const float* act, int64_t act_stride, int32_t n,
                 int32_t target, float* q, void* stream) {
  if (!obs || !act) return fail(SAC_E_INVALID, "q_values: null input (obs or act)");
  if (!q) return fail(SAC_E_INVALID, "q_values: null output");
  if (n < 1) return fail(SAC_E_INVALID, "q_values: n >= 1");
  if (!e) return fail(SAC_E_INVALID, "null engine");
  if (obs_stride < e->cfg.obs_dim || act_stride < e->cfg.act_dim)
    return fail(SAC_E_INVALID, "q_values: stride below the field width (obs_stride " + std::to_string(obs_stride) +
                                   " < " + std::to_string(e->cfg.obs_dim) + " or act_stride " +
                                   std::to_string(act_stride) + " < " + std::to_string(e->cfg.act_dim) + ")");
  return launch_q_values(e, QRows{obs, obs_stride, act, act_stride, 0, 0, nullptr, 0}, n, target, q, stream);
}

// The descriptor of n ring rows of a replay buffer (first left 0) once rb's pointers, n >= 1 and
// capacity >= 1 are known good: the checks the two replay entry points share.
static int q_replay_rows(sac_engine* e, const sac_replay* rb, int32_t n, int32_t use_next_obs, QRows* rows) {
  const int64_t cap = rb->capacity;
  if (n > cap)
    return fail(SAC_E_INVALID, "q_values_replay: n (" + std::to_string(n) + ") exceeds the replay capacity (" +
                                   std::to_string(cap) + ")");
  if (!e) return fail(SAC_E_INVALID, "null engine");
  if (rb->obs_dim != e->cfg.obs_dim || rb->act_dim != e->cfg.act_dim)
    return fail(SAC_E_INVALID, "replay dims do not match the engine");
  const RowStrides rs = row_strides(rb->row_stride, rb->obs_dim, rb->act_dim);
  if (rs.obs < rb->obs_dim || rs.act < rb->act_dim)
    return fail(SAC_E_INVALID, "q_values_replay: record stride below the field width");
  *rows = QRows{use_next_obs ? rb->next_obs : rb->obs, rs.obs, rb->act, rs.act, 0, cap, nullptr, 0};
  return SAC_OK;
}

int sac_q_values_replay(sac_engine* e, const sac_replay* rb, int64_t first_slot, int32_t n, int32_t use_next_obs,
                        int32_t target, float* q, void* stream) {
  if (!rb || !rb->obs || !rb->act || !rb->next_obs) return fail(SAC_E_INVALID, "q_values_replay: null replay buffer");
  if (!q) return fail(SAC_E_INVALID, "q_values_replay: null output");
  if (n < 1) return fail(SAC_E_INVALID, "q_values_replay: n >= 1");
  const int64_t cap = rb->capacity;
  if (cap < 1 || first_slot < 0 || first_slot >= cap)
    return fail(SAC_E_INVALID, "q_values_replay: first_slot (" + std::to_string(first_slot) +
                                   ") outside [0, capacity " + std::to_string(cap) + ")");
  QRows rows;
  const int rc = q_replay_rows(e, rb, n, use_next_obs, &rows);
  if (rc) return rc;
  rows.first = first_slot;
  return launch_q_values(e, rows, n, target, q, stream);
}

// One slot of a device loop cursor and its parity, as the cursor entry points take them.
static int check_cursor(const int64_t* cursor, int32_t parity, const char* who) {
  if (!cursor) return fail(SAC_E_INVALID, std::string(who) + ": null cursor");
  if (parity != 0 && parity != 1)
    return fail(SAC_E_INVALID, std::string(who) + ": parity (" + std::to_string(parity) + ") must be 0 or 1");
  return SAC_OK;
}

int sac_q_values_replay_dev(sac_engine* e, const sac_replay* rb, const int64_t* cursor, int32_t parity, int32_t n,
                            int32_t use_next_obs, int32_t target, float* q_ring, int32_t q_ring_steps, void* stream) {
  if (!rb || !rb->obs || !rb->act || !rb->next_obs)
    return fail(SAC_E_INVALID, "q_values_replay_dev: null replay buffer");
  if (!q_ring) return fail(SAC_E_INVALID, "q_values_replay_dev: null output ring");
  int rc = check_cursor(cursor, parity, "q_values_replay_dev");
  if (rc) return rc;
  if (n < 1) return fail(SAC_E_INVALID, "q_values_replay_dev: n >= 1");
  if (q_ring_steps < 1) return fail(SAC_E_INVALID, "q_values_replay_dev: q_ring_steps >= 1");
  if (rb->capacity < 1) return fail(SAC_E_INVALID, "q_values_replay_dev: capacity >= 1");
  QRows rows;
  rc = q_replay_rows(e, rb, n, use_next_obs, &rows);
  if (rc) return rc;
  rows.cursor = cursor + 4 * parity;
  rows.ring_steps = q_ring_steps;
  return launch_q_values(e, rows, n, target, q_ring, stream);
}

int sac_debug_engine_host(const sac_engine_config* cfg, sac_engine** out) {
  if (!out) return fail(SAC_E_INVALID, "null out");
  int rc = validate(cfg);
  if (rc) return rc;
  sac_engine* e = new sac_engine();
  e->cfg = *cfg;
  memset(&e->buf, 0, sizeof(e->buf));
  memset(&e->h, 0, sizeof(e->h));
  *out = e;
  return SAC_OK;
}

int sac_envs_reset(const sac_envs* envs, uint64_t seed, void* stream) {
  int rc = check_envs(envs, false);
  if (rc) return rc;
  const int n = envs->cfg.num_envs;
  sac_envs_reset_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(*envs, seed);
  HIPCHK(hipGetLastError());
  return SAC_OK;
}

int sac_envs_step(const sac_envs* envs, const float* actions, uint64_t t, float* obs, float* final_obs, float* reward,
                  uint8_t* terminated, uint8_t* truncated, void* stream) {
  int rc = check_envs(envs, false);
  if (rc) return rc;
  if (!actions || !obs || !final_obs || !reward || !terminated || !truncated)
    return fail(SAC_E_INVALID, "bad envs_step arguments: null actions or outputs");
  const int n = envs->cfg.num_envs;
  sac_envs_step_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(*envs, actions, t, obs, final_obs, reward,
                                                                        terminated, truncated);
  HIPCHK(hipGetLastError());
  return SAC_OK;
}

// What a fused rollout step needs, in two parts (sac_rollout_step checks its host (size, pos) between
// them): the environments with their episode ring, a whole replay buffer that holds one vector step ...
static int check_rollout_buffers(const sac_envs* envs, const sac_replay* rb) {
  int rc = check_envs(envs, true);
  if (rc) return rc;
  if (!rb || !rb->obs || !rb->act || !rb->rew || !rb->next_obs || !rb->done || !rb->state)
    return fail(SAC_E_INVALID, "null replay buffer");
  const int64_t n = envs->cfg.num_envs, cap = rb->capacity;
  if (cap < 1 || n > cap)
    return fail(SAC_E_INVALID, "num_envs (" + std::to_string(n) + ") exceeds the replay capacity (" +
                                   std::to_string(cap) + ")");
  return SAC_OK;
}
// ... and replay, environments and engine of one shape, on an engine that can run the policy's forward.
static int check_rollout_dims(const sac_engine* e, const sac_envs* envs, const sac_replay* rb, const char* who) {
  const int A = env_act_dim(envs->cfg.kind);
  if (rb->obs_dim != envs->cfg.obs_dim || rb->act_dim != A)
    return fail(SAC_E_INVALID, "replay dims do not match the environments (act_dim " + std::to_string(A) + ")");
  if (!e) return fail(SAC_E_INVALID, "null engine");
  if (e->cfg.obs_dim != envs->cfg.obs_dim || e->cfg.act_dim != A)
    return fail(SAC_E_INVALID, "engine dims do not match the environments (act_dim " + std::to_string(A) + ")");
  return check_policy_forward(e, who);
}

// rollout_step_body's `store`: 0 stores nothing, else 1 + the engine's sac_done_mode picks the done word
static int rollout_store(const sac_engine* e, int32_t store) { return store ? 1 + e->done_mode : 0; }
// a sampled step of an engine whose source is SAC_ACTIONS_UNIFORM takes the uniform kernels; the policy mean never does
static bool rollout_uniform(const sac_engine* e, int deterministic) {
  return !deterministic && e->action_source == SAC_ACTIONS_UNIFORM;
}
static int uniform_blocks(int64_t n) { return (int)((n + SAC_UNIFORM_THREADS - 1) / SAC_UNIFORM_THREADS); }

int sac_rollout_step(sac_engine* e, const sac_envs* envs, const sac_replay* rb, int64_t size_host, int64_t pos_host,
                     uint64_t t, int32_t deterministic, int32_t store, void* stream) {
  int rc = check_rollout_buffers(envs, rb);
  if (rc) return rc;
  const int64_t n = envs->cfg.num_envs, cap = rb->capacity;
  if (size_host < 0 || size_host > cap || pos_host < 0 || pos_host >= cap)
    return fail(SAC_E_INVALID, "replay (size, pos) out of range");
  rc = check_rollout_dims(e, envs, rb, "rollout_step");
  if (rc) return rc;
  const int64_t new_size = std::min(cap, size_host + n);
  const int64_t new_pos = (pos_host + n) % cap;
  const int blocks = (int)((n + SAC_ROWS - 1) / SAC_ROWS);
  hipStream_t s = (hipStream_t)stream;
  const int kind = envs->cfg.kind;
  if (rollout_uniform(e, deterministic)) {
    rollout_uniform_kernel(kind)<<<uniform_blocks(n), SAC_UNIFORM_THREADS, 0, s>>>(
        e->cfg.seed, e->cfg.action_scale, *envs, *rb, pos_host, new_size, new_pos, t, rollout_store(e, store));
    HIPCHK(hipGetLastError());
    return SAC_OK;
  }
  auto kernel = e->cfg.precision == SAC_PREC_BF16 ? rollout_kernel<bf16>(kind) : rollout_kernel<float>(kind);
  kernel<<<blocks, SAC_THREADS, e->lds_bytes, s>>>(e->d, *envs, *rb, pos_host, new_size, new_pos, t, deterministic ? 1 : 0,
                                                   rollout_store(e, store));
  HIPCHK(hipGetLastError());
  return SAC_OK;
}

// every argument validated by the caller; one launch, no host-side state written (the action source is read)
static int launch_rollout_dev(sac_engine* e, const sac_envs* envs, const sac_replay* rb, int64_t* cursor, int parity,
                              int deterministic, int store, hipStream_t s) {
  const int blocks = (envs->cfg.num_envs + SAC_ROWS - 1) / SAC_ROWS;
  const int64_t* cur = cursor + 4 * parity;
  int64_t* nxt = cursor + 4 * (parity ^ 1);
  const int kind = envs->cfg.kind;
  if (rollout_uniform(e, deterministic)) {
    rollout_uniform_dev_kernel(kind)<<<uniform_blocks(envs->cfg.num_envs), SAC_UNIFORM_THREADS, 0, s>>>(
        e->cfg.seed, e->cfg.action_scale, *envs, *rb, cur, nxt, store);
    HIPCHK(hipGetLastError());
    return SAC_OK;
  }
  auto kernel = e->cfg.precision == SAC_PREC_BF16 ? rollout_dev_kernel<bf16>(kind) : rollout_dev_kernel<float>(kind);
  kernel<<<blocks, SAC_THREADS, e->lds_bytes, s>>>(e->d, *envs, *rb, cur, nxt, deterministic, store);
  HIPCHK(hipGetLastError());
  return SAC_OK;
}

int sac_rollout_step_dev(sac_engine* e, const sac_envs* envs, const sac_replay* rb, int64_t* cursor, int32_t parity,
                         int32_t deterministic, int32_t store, void* stream) {
  int rc = check_rollout_buffers(envs, rb);
  if (rc) return rc;
  rc = check_cursor(cursor, parity, "rollout_step_dev");
  if (rc) return rc;
  rc = check_rollout_dims(e, envs, rb, "rollout_step_dev");
  if (rc) return rc;
  return launch_rollout_dev(e, envs, rb, cursor, parity, deterministic ? 1 : 0, rollout_store(e, store),
                            (hipStream_t)stream);
}

int sac_engine_loop_graph(sac_engine* e, const sac_envs* envs, const sac_replay* rb, int64_t* cursor, int32_t k_steps,
                          const int32_t* grad_steps_host, float* q_ring, int32_t q_ring_steps, int32_t n_replays,
                          void* stream) {
  int rc = check_rollout_buffers(envs, rb);
  if (rc) return rc;
  if (!cursor) return fail(SAC_E_INVALID, "loop_graph: null cursor");
  if (k_steps < 2 || (k_steps & 1))
    return fail(SAC_E_INVALID, "loop_graph: k_steps (" + std::to_string(k_steps) +
                                   ") must be even and >= 2 (the cursor slot of vector step j is j & 1)");
  if (!grad_steps_host) return fail(SAC_E_INVALID, "loop_graph: null gradient-step counts");
  for (int j = 0; j < k_steps; ++j)
    if (grad_steps_host[j] < 0)
      return fail(SAC_E_INVALID, "loop_graph: negative gradient-step count at vector step " + std::to_string(j));
  if (n_replays < 0) return fail(SAC_E_INVALID, "loop_graph: n_replays >= 0");
  if (q_ring && q_ring_steps < 1) return fail(SAC_E_INVALID, "loop_graph: q_ring needs q_ring_steps >= 1");
  rc = check_rollout_dims(e, envs, rb, "loop_graph");
  if (rc) return rc;
  rc = check_replay(e, rb);
  if (rc) return rc;
  const int n = envs->cfg.num_envs;
  QRows rows{};
  if (q_ring) {
    rc = q_replay_rows(e, rb, n, 1, &rows);
    if (rc) return rc;
    rc = check_q_forward(e);
    if (rc) return rc;
    rows.ring_steps = q_ring_steps;
  }
  hipStream_t s = (hipStream_t)stream;
  const sac_engine::LoopKey& k = e->lkey;
  const bool same = e->lgexec && !memcmp(&k.envs, envs, sizeof(sac_envs)) && !memcmp(&k.rb, rb, sizeof(sac_replay)) &&
                    k.cursor == cursor && k.done_mode == e->done_mode && k.action_source == e->action_source &&
                    k.q_ring == q_ring && k.q_ring_steps == (q_ring ? q_ring_steps : 0) &&
                    (int)k.grad.size() == k_steps && std::equal(k.grad.begin(), k.grad.end(), grad_steps_host);
  if (!same) {
    if (e->lgexec) (void)hipGraphExecDestroy(e->lgexec);
    if (e->lgraph) (void)hipGraphDestroy(e->lgraph);
    e->lgexec = nullptr;
    e->lgraph = nullptr;
    if (!e->cap) HIPCHK(hipStreamCreateWithFlags(&e->cap, hipStreamNonBlocking));
    // one stream, no forks: node j + 1 follows node j, so the slot vector step j writes is the one j + 1 reads
    HIPCHK(hipStreamBeginCapture(e->cap, hipStreamCaptureModeThreadLocal));
    for (int j = 0; j < k_steps && !rc; ++j) {
      rc = launch_rollout_dev(e, envs, rb, cursor, j & 1, 0, rollout_store(e, 1), e->cap);
      if (!rc && grad_steps_host[j]) launch_steps(e, rb, grad_steps_host[j], nullptr, nullptr, e->cap);
      if (!rc && q_ring) {
        rows.cursor = cursor + 4 * (j & 1);  // the slot this vector step read: its pos is the step's first row
        rc = launch_q_values(e, rows, n, 0, q_ring, e->cap);
      }
    }
    const hipError_t end = hipStreamEndCapture(e->cap, &e->lgraph);
    if (rc || end != hipSuccess) {
      if (e->lgraph) (void)hipGraphDestroy(e->lgraph);
      e->lgraph = nullptr;
      return rc ? rc : fail(SAC_E_HIP, std::string("loop_graph capture: ") + hipGetErrorString(end));
    }
    HIPCHK(hipGraphInstantiate(&e->lgexec, e->lgraph, nullptr, nullptr, 0));
    HIPCHK(hipGraphUpload(e->lgexec, s));  // as train_graph: not inside the first replay
    e->lkey.envs = *envs;
    e->lkey.rb = *rb;
    e->lkey.cursor = cursor;
    e->lkey.done_mode = e->done_mode;
    e->lkey.action_source = e->action_source;
    e->lkey.q_ring = q_ring;
    e->lkey.q_ring_steps = q_ring ? q_ring_steps : 0;
    e->lkey.grad.assign(grad_steps_host, grad_steps_host + k_steps);
  }
  for (int r = 0; r < n_replays; ++r) HIPCHK(hipGraphLaunch(e->lgexec, s));
  return SAC_OK;
}

int sac_uniform_actions_host(uint64_t seed, uint64_t t, int32_t n, int32_t act_dim, float scale, float* out_host) {
  if (!out_host || n < 1 || act_dim < 1 || act_dim > 32 || !(scale > 0.f) || !std::isfinite(scale))
    return fail(SAC_E_INVALID, "uniform_actions: need out != NULL, n >= 1, act_dim in 1..32 and a finite scale > 0");
  for (int i = 0; i < n; ++i) uniform_actions_row(seed, t, (uint32_t)i, scale, act_dim, out_host + (size_t)i * act_dim);
  return SAC_OK;
}

int sac_debug_rollout_eps_host(uint64_t seed, uint64_t t, int32_t n, int32_t act_dim, float* out) {
  if (!out || n < 1 || act_dim < 1) return fail(SAC_E_INVALID, "need n >= 1, act_dim >= 1, out != NULL");
  for (int i = 0; i < n; ++i)
    for (int p = 0; 2 * p < act_dim; ++p) {
      float n0, n1;
      philox_normal2(seed, t, (uint32_t)i, ENV_WHICH_NOISE, (uint32_t)p, n0, n1);
      out[(size_t)i * act_dim + 2 * p] = n0;
      if (2 * p + 1 < act_dim) out[(size_t)i * act_dim + 2 * p + 1] = n1;
    }
  return SAC_OK;
}

// The rollout step's action noise as its row owners draw it, one thread per (env row, action pair)
__global__ void rollout_eps_kernel(uint64_t seed, uint64_t t, int n, int A, float* __restrict__ out) {
  const int NP = (A + 1) / 2;
  const int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (k >= (int64_t)n * NP) return;
  const int i = (int)(k / NP), p = (int)(k % NP);
  float n0, n1;
  philox_normal2(seed, t, (uint32_t)i, ENV_WHICH_NOISE, (uint32_t)p, n0, n1);
  out[(size_t)i * A + 2 * p] = n0;
  if (2 * p + 1 < A) out[(size_t)i * A + 2 * p + 1] = n1;
}

int sac_debug_rollout_eps_device(uint64_t seed, uint64_t t, int32_t n, int32_t act_dim, float* out, void* stream) {
  if (!out || n < 1 || act_dim < 1) return fail(SAC_E_INVALID, "need n >= 1, act_dim >= 1, out != NULL");
  const int64_t work = (int64_t)n * ((act_dim + 1) / 2);
  rollout_eps_kernel<<<(unsigned)((work + 255) / 256), 256, 0, (hipStream_t)stream>>>(seed, t, n, act_dim, out);
  HIPCHK(hipGetLastError());
  return SAC_OK;
}

int sac_debug_env_obs_host(uint64_t seed, uint64_t t, int32_t which, int32_t n, int32_t obs_dim, float* out) {
  if (!out || n < 1 || obs_dim < 1 || obs_dim > 4 * 65536 || which < 0 || which > 0xFFFF)
    return fail(SAC_E_INVALID, "need n >= 1, 1 <= obs_dim <= 262144, 0 <= which < 65536, out != NULL");
  for (int i = 0; i < n; ++i)
    for (int b = 0; 4 * b < obs_dim; ++b) {
      float u[4];
      philox_uniform4(seed, t, (uint32_t)i, (uint32_t)which, (uint32_t)b, u);
      for (int k = 0; k < 4 && 4 * b + k < obs_dim; ++k) out[(size_t)i * obs_dim + 4 * b + k] = env_uniform_obs(u[k]);
    }
  return SAC_OK;
}

int sac_debug_env_step_host(const sac_env_config* cfg, double state[2], int32_t step, float action, float obs_out[3],
                            double* reward, int32_t* truncated) {
  if (!cfg || !state || !obs_out || !reward || !truncated)
    return fail(SAC_E_INVALID, "need cfg, state, obs_out, reward and truncated != NULL");
  return task_step_host<ENV_CLASS_PENDULUM>("env_step_host", cfg, state, step, &action, obs_out, reward, nullptr,
                                            truncated);
}

int sac_debug_env_reset_host(uint64_t seed, uint64_t t, int32_t row, double state_out[2]) {
  return task_reset_host<ENV_CLASS_PENDULUM>(seed, t, row, state_out);
}

int sac_debug_reacher_step_host(const sac_env_config* cfg, double state[6], int32_t step, const float action[2],
                                float obs_out[10], double* reward, int32_t* truncated) {
  if (!cfg || !state || !action || !obs_out || !reward || !truncated)
    return fail(SAC_E_INVALID, "need cfg, state, action, obs_out, reward and truncated != NULL");
  return task_step_host<ENV_CLASS_REACHER>("reacher_step_host", cfg, state, step, action, obs_out, reward, nullptr,
                                           truncated);
}

int sac_debug_reacher_reset_host(uint64_t seed, uint64_t t, int32_t row, double state_out[6]) {
  return task_reset_host<ENV_CLASS_REACHER>(seed, t, row, state_out);
}

int sac_debug_cartpole_step_host(const sac_env_config* cfg, double state[4], int32_t step, const float action[1],
                                 float obs_out[4], double* reward, int32_t* terminated, int32_t* truncated) {
  if (!cfg || !state || !action || !obs_out || !reward || !terminated || !truncated)
    return fail(SAC_E_INVALID, "need cfg, state, action, obs_out, reward, terminated and truncated != NULL");
  return task_step_host<ENV_CLASS_CARTPOLE>("cartpole_step_host", cfg, state, step, action, obs_out, reward,
                                            terminated, truncated);
}

int sac_debug_cartpole_reset_host(uint64_t seed, uint64_t t, int32_t row, double state_out[4]) {
  return task_reset_host<ENV_CLASS_CARTPOLE>(seed, t, row, state_out);
}

int sac_replay_push(const sac_replay* rb, const float* rows, int64_t n, int64_t size_host, int64_t pos_host,
                    void* stream) {
  if (!rb || !rows || n < 0 || rb->capacity < 1) return fail(SAC_E_INVALID, "bad replay_push arguments");
  if (n == 0) return SAC_OK;
  const int64_t cap = rb->capacity;
  const int64_t skip = n > cap ? n - cap : 0;
  const int64_t new_size = std::min(cap, size_host + n);
  const int64_t new_pos = (pos_host + n) % cap;
  const int64_t total = (n - skip) * (2 * rb->obs_dim + rb->act_dim + 2);
  const int blocks = (int)std::min<int64_t>(4096, (total + 255) / 256);
  replay_push_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(*rb, rows, n, skip, pos_host, new_size, new_pos);
  HIPCHK(hipGetLastError());
  return SAC_OK;
}

static bool replay_fields(const sac_replay* rb) {
  return rb && rb->obs && rb->act && rb->rew && rb->next_obs && rb->done;
}

// sac_replay_emit_nstep (codes = false: gpow_host[0..n-1]) and sac_replay_emit_nstep_codes (true: gpow_host[0..n])
static int emit_nstep(const sac_replay* stage, const sac_replay* rb, int32_t n, int32_t num_envs, int64_t newest,
                      const double* gpow_host, int64_t size_host, int64_t pos_host, bool codes, hipStream_t stream) {
  if (!replay_fields(stage)) return fail(SAC_E_INVALID, "emit_nstep: null staging table or field");
  if (!replay_fields(rb) || !rb->state) return fail(SAC_E_INVALID, "emit_nstep: null replay buffer, field or state");
  if (!gpow_host) return fail(SAC_E_INVALID, "emit_nstep: null discount powers");
  if (n < 1 || n > SAC_NSTEP_MAX)
    return fail(SAC_E_INVALID, "emit_nstep: n (" + std::to_string(n) + ") outside 1.." + std::to_string(SAC_NSTEP_MAX));
  if (num_envs < 1) return fail(SAC_E_INVALID, "emit_nstep: num_envs >= 1");
  const int64_t scap = (int64_t)n * num_envs, cap = rb->capacity;
  if (stage->capacity != scap)
    return fail(SAC_E_INVALID, "emit_nstep: the staging table holds " + std::to_string(stage->capacity) +
                                   " rows, not n * num_envs = " + std::to_string(scap));
  if (stage->obs_dim != rb->obs_dim || stage->act_dim != rb->act_dim || rb->obs_dim < 1 || rb->act_dim < 1)
    return fail(SAC_E_INVALID, "emit_nstep: staging dims do not match the replay buffer's");
  for (const sac_replay* t : {stage, rb})
    if (t->row_stride < 0 || (t->row_stride && t->row_stride < std::max(t->obs_dim, t->act_dim)))
      return fail(SAC_E_INVALID, "emit_nstep: record stride below the field width");
  if (cap < 1 || num_envs > cap)
    return fail(SAC_E_INVALID, "emit_nstep: num_envs (" + std::to_string(num_envs) + ") exceeds the replay capacity (" +
                                   std::to_string(cap) + ")");
  if (newest < 0 || newest >= scap)
    return fail(SAC_E_INVALID, "emit_nstep: newest (" + std::to_string(newest) + ") outside the staging table");
  if (size_host < 0 || size_host > cap || pos_host < 0 || pos_host >= cap)
    return fail(SAC_E_INVALID, "emit_nstep: replay (size, pos) out of range");
  if (stage == rb || stage->obs == rb->obs || stage->rew == rb->rew)
    return fail(SAC_E_INVALID, "emit_nstep: the staging table and the replay buffer are the same table");
  const int64_t new_size = std::min(cap, size_host + (int64_t)num_envs);
  const int64_t new_pos = (pos_host + num_envs) % cap;
  const int blocks = (num_envs + 3) / 4;  // one wave per environment row
  if (codes) {
    NStepCodePowers gp{};
    for (int j = 0; j <= n; ++j) gp.g[j] = gpow_host[j];
    sac_replay_emit_nstep_codes_kernel<SAC_NSTEP_MAX + 1>
        <<<blocks, 256, 0, stream>>>(*stage, *rb, n, num_envs, newest, gp, pos_host, new_size, new_pos);
  } else {
    NStepPowers gp{};
    for (int j = 0; j < n; ++j) gp.g[j] = gpow_host[j];
    sac_replay_emit_nstep_kernel<<<blocks, 256, 0, stream>>>(*stage, *rb, n, num_envs, newest, gp, pos_host,
                                                                new_size, new_pos);
  }
  HIPCHK(hipGetLastError());
  return SAC_OK;
}

int sac_replay_emit_nstep(const sac_replay* stage, const sac_replay* rb, int32_t n, int32_t num_envs, int64_t newest,
                          const double* gpow_host, int64_t size_host, int64_t pos_host, void* stream) {
  return emit_nstep(stage, rb, n, num_envs, newest, gpow_host, size_host, pos_host, false, (hipStream_t)stream);
}

int sac_replay_emit_nstep_codes(const sac_replay* stage, const sac_replay* rb, int32_t n, int32_t num_envs,
                                int64_t newest, const double* gpow_host, int64_t size_host, int64_t pos_host,
                                void* stream) {
  return emit_nstep(stage, rb, n, num_envs, newest, gpow_host, size_host, pos_host, true, (hipStream_t)stream);
}

// rows per wave of the records gather: 16 (4x the waves in flight of 64 rows per wave:
// 65,536 rows 1.51 -> 2.42 TB/s, 1,048,576 rows 3.00 -> 3.17 TB/s)
static constexpr int GATHER_RPW = 16;

int sac_replay_gather(const sac_replay* rb, const int32_t* logical_idx, int32_t batch, float* s, float* a, float* r,
                      float* s2, float* d, void* stream) {
  if (!rb || !logical_idx || batch < 1 || !s || !a || !r || !s2 || !d) return fail(SAC_E_INVALID, "bad gather arguments");
  const int blocks = (batch + 255) / 256;  // one wave per 64 rows
  const int rpw = GATHER_RPW;
  if (standard_records(rb))
    replay_gather_records_kernel<false><<<(batch + 4 * rpw - 1) / (4 * rpw), 256, 0, (hipStream_t)stream>>>(
        *rb, logical_idx, batch, FeistelKeys{}, nullptr, s, a, r, s2, d, rpw);
  else
    replay_gather_kernel<false><<<blocks, 256, 0, (hipStream_t)stream>>>(*rb, logical_idx, batch, FeistelKeys{}, nullptr, s,
                                                                         a, r, s2, d);
  HIPCHK(hipGetLastError());
  return SAC_OK;
}

int sac_replay_sample_gather(const sac_replay* rb, int32_t batch, uint64_t seed, uint64_t step, int32_t* idx_out,
                             float* s, float* a, float* r, float* s2, float* d, void* stream) {
  if (!rb || batch < 1 || !s || !a || !r || !s2 || !d) return fail(SAC_E_INVALID, "bad sample_gather arguments");
  const int blocks = (batch + 255) / 256;
  const int rpw = GATHER_RPW;
  if (standard_records(rb))
    replay_gather_records_kernel<true><<<(batch + 4 * rpw - 1) / (4 * rpw), 256, 0, (hipStream_t)stream>>>(
        *rb, nullptr, batch, feistel_keys(seed, step), idx_out, s, a, r, s2, d, rpw);
  else
    replay_gather_kernel<true><<<blocks, 256, 0, (hipStream_t)stream>>>(*rb, nullptr, batch, feistel_keys(seed, step), idx_out, s,
                                                                        a, r, s2, d);
  HIPCHK(hipGetLastError());
  return SAC_OK;
}

int sac_engine_read_status(sac_engine* e, uint32_t* host_dst, void* stream) {
  if (!e || !host_dst) return fail(SAC_E_INVALID, "bad read_status arguments");
  HIPCHK(hipMemcpyAsync(host_dst, e->h.sync, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
  return SAC_OK;
}

int sac_engine_clear_status(sac_engine* e, void* stream) {
  if (!e) return fail(SAC_E_INVALID, "null engine");
  HIPCHK(hipMemsetAsync(e->h.sync + SYNC_TIMEOUT, 0, sizeof(uint32_t), (hipStream_t)stream));
  return SAC_OK;
}

int sac_engine_debug_set_spin_limit(sac_engine* e, int32_t polls, void* stream) {
  if (!e || polls < 0) return fail(SAC_E_INVALID, "bad spin limit");
  e->h.spin_limit = polls;
  HIPCHK(hipMemcpyAsync(e->d, &e->h, sizeof(EngineDev), hipMemcpyHostToDevice, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return SAC_OK;
}

int sac_replay_sample_indices(const sac_replay* rb, int32_t batch, uint64_t seed, uint64_t step, int32_t* out,
                              void* stream) {
  if (!rb || !out || batch < 1) return fail(SAC_E_INVALID, "bad sample arguments");
  const int blocks = std::min(4096, (batch + 255) / 256);
  replay_sample_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(rb->state, batch, feistel_keys(seed, step), out);
  HIPCHK(hipGetLastError());
  return SAC_OK;
}

int sac_engine_debug_stamps(sac_engine* e, long long* dev_buf, void* stream) {
  if (!e) return fail(SAC_E_INVALID, "null engine");
  e->h.stamps = dev_buf;
  HIPCHK(hipMemcpyAsync(e->d, &e->h, sizeof(EngineDev), hipMemcpyHostToDevice, (hipStream_t)stream));
#ifdef SAC_STAMPS
  HIPCHK(hipMemcpyToSymbolAsync(HIP_SYMBOL(sac_dbg_stamps), &dev_buf, sizeof(dev_buf), 0, hipMemcpyHostToDevice,
                                (hipStream_t)stream));
#endif
  if (e->gexec) {  // graphs captured the old kernel arguments
    (void)hipGraphExecDestroy(e->gexec);
    (void)hipGraphDestroy(e->graph);
    e->gexec = nullptr;
    e->graph = nullptr;
  }
  if (e->lgexec) {
    (void)hipGraphExecDestroy(e->lgexec);
    (void)hipGraphDestroy(e->lgraph);
    e->lgexec = nullptr;
    e->lgraph = nullptr;
  }
  return SAC_OK;
}

int sac_debug_sample_indices_host(int64_t size, int32_t batch, uint64_t seed, uint64_t step, int32_t* out) {
  if (!out || batch < 0 || size < batch) return fail(SAC_E_INVALID, "need 0 <= batch <= size and out != NULL");
  const Feistel f = feistel_make(seed, step, size);
  for (int32_t b = 0; b < batch; ++b) out[b] = (int32_t)feistel_sample(f, b, size);
  return SAC_OK;
}

int sac_debug_eps_host(uint64_t seed, uint64_t step, int32_t batch, int32_t act_dim, float* out) {
  if (!out || batch < 1 || act_dim < 1) return fail(SAC_E_INVALID, "need batch >= 1, act_dim >= 1, out != NULL");
  for (int which = 0; which < 2; ++which)
    for (int b = 0; b < batch; ++b)
      for (int p = 0; p < (act_dim + 1) / 2; ++p) eps_pair(seed, step, b, which, p, batch, act_dim, out);
  return SAC_OK;
}

// sac_math.h compiled for the host, one element i < n at a time (include/sac_engine_testing.h)
int sac_debug_head_host(int32_t n, const float* in, float lo, float hi, float scale, float gamma, float alpha,
                        int32_t B, float* out) {
  if (!in || !out || n < 1 || B < 1) return fail(SAC_E_INVALID, "need n >= 1, B >= 1, in != NULL, out != NULL");
  for (int32_t i = 0; i < n; ++i) {
    auto I = [&](int k) { return in[(size_t)k * n + i]; };
    auto O = [&](int k) -> float& { return out[(size_t)k * n + i]; };
    const float mu = I(SAC_HEAD_IN_MU), e = I(SAC_HEAD_IN_E);
    const float q1 = I(SAC_HEAD_IN_Q1), q2 = I(SAC_HEAD_IN_Q2), lp = I(SAC_HEAD_IN_LP);
    const HeadAct a = head_act(mu, I(SAC_HEAD_IN_LSR), e, lo, hi, scale);
    O(SAC_HEAD_LS) = a.ls, O(SAC_HEAD_ACT_Z) = a.z, O(SAC_HEAD_ACT_ACT) = a.act;
    O(SAC_HEAD_ACT_MEAN) = head_act_mean(mu, scale);
    O(SAC_HEAD_ACT_LP) = head_act_lp(e, a.ls), O(SAC_HEAD_ACT_CORR) = head_corr(a.z);
    const float y = td_target(I(SAC_HEAD_IN_R), I(SAC_HEAD_IN_D), gamma, q1, q2, alpha, lp);
    const CriticSeed cs = critic_seed(q1, y, B);
    O(SAC_HEAD_Y) = y, O(SAC_HEAD_SEED_D) = cs.d, O(SAC_HEAD_SEED) = cs.seed;
    const MinQ w = minq_weights(q1, q2, -1.0f / (float)B);
    O(SAC_HEAD_MINQ) = w.m, O(SAC_HEAD_W1) = w.w1, O(SAC_HEAD_W2) = w.w2;
    O(SAC_HEAD_PI_TERM) = pi_loss_term(alpha, lp, w.m);
  }
  return SAC_OK;
}

int sac_debug_eps_device(uint64_t seed, uint64_t step, int32_t batch, int32_t act_dim, float* out, void* stream) {
  if (!out || batch < 1 || act_dim < 1) return fail(SAC_E_INVALID, "need batch >= 1, act_dim >= 1, out != NULL");
  const int64_t n = 2LL * batch * ((act_dim + 1) / 2);
  const int blocks = (int)std::min<int64_t>(4096, (n + 255) / 256);
  eps_draw_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(seed, step, batch, act_dim, out);
  HIPCHK(hipGetLastError());
  return SAC_OK;
}

// The plan of a config as JSON, with no HIP call (include/sac_engine_testing.h).
int sac_debug_plan_host(const sac_engine_config* cfg, int32_t ncu, char* out, size_t cap) {
  if (!out) return fail(SAC_E_INVALID, "null argument");
  int rc = validate(cfg);
  if (rc) return rc;
  if (ncu < 1) return fail(SAC_E_INVALID, "ncu >= 1");
  sac_engine e;
  e.cfg = *cfg;
  e.ncu = ncu;
  // the fifteen parameter buffers are the struct's first fifteen pointers, in order
  void* fake[15];
  for (int i = 0; i < 15; ++i) fake[i] = (void*)(uintptr_t)(SAC_PLAN_FAKE_BUFFER0 + i * SAC_PLAN_FAKE_BUFFER_STEP);
  static_assert(offsetof(sac_engine_buffers, workspace) == sizeof(fake), "fifteen pointers before the workspace");
  memcpy(&e.buf, fake, sizeof(fake));
  e.buf.workspace = (void*)(uintptr_t)SAC_PLAN_FAKE_WORKSPACE;
  const PlanSize sized = plan(cfg, nullptr, nullptr);
  if (sized.refused) return fail_refused(sized.refused);
  e.buf.workspace_bytes = sized.bytes;
  plan(cfg, &e, (char*)e.buf.workspace);
  rc = check_plan(&e);
  if (rc) return rc;
  auto fnv = [](const void* p, size_t n) {  // FNV-1a 64
    uint64_t hsh = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i) hsh = (hsh ^ ((const unsigned char*)p)[i]) * 0x100000001b3ull;
    char b[20];
    snprintf(b, sizeof(b), "\"%016llx\"", (unsigned long long)hsh);
    return std::string(b);
  };
  auto kv = [](const char* k, unsigned long long v) { return "\"" + std::string(k) + "\": " + std::to_string(v); };
  const bool wide = e.path == PATH_WIDE;
  const char* paths[] = {"split", "roles", "pairs", "rows", "wide"};  // by sac_path
  const char* path = paths[e.path];
  std::string j = "{\"path\": \"" + std::string(path) + "\", " + kv("workspace_bytes", e.buf.workspace_bytes) + ", " +
                  kv("lds_bytes", e.lds_bytes) + ", " + kv("upd_lds", e.upd_lds) + ", " + kv("upd_lds_b", e.launch[L_B].lds) +
                  ", " + kv("upd_threads_b", e.launch[L_B].threads) + ", " + kv("nB", e.nB) + ", " + kv("nD", e.nD) + ", " +
                  kv("nrt", e.h.nrt) + ", " + kv("xs", e.h.xs) + ", " + kv("role_xcd", e.h.role_xcd) + ", " +
                  kv("stage", e.h.stage) + ", " + kv("upd_slots", e.h.upd_slots) + ", \"launch\": {";
  const char* names[4] = {"A", "B", "C", "D"};
  bool first = true;
  for (int k = L_A; k <= L_D; ++k) {
    if (wide && (k == L_A || k == L_C)) continue;  // the stage list below
    const PhaseLaunch& d = e.launch[k];
    j += std::string(first ? "" : ", ") + "\"" + names[k] + "\": {" + kv("grid", d.grid) + ", " +
         kv("threads", d.threads) + ", " + kv("lds", d.lds) + "}";
    first = false;
  }
  if (wide) {
    j += ", \"stages\": [";
    for (size_t i = 0; i < e.wst.size(); ++i) {
      const sac_engine::WStage& st = e.wst[i];
      j += std::string(i ? ", {" : "{") + kv("kind", st.kind) + ", " + kv("j0", st.j0) + ", " + kv("j1", st.j1) + ", " +
           kv("grid", st.grid) + ", " + kv("phase", st.phase) + ", " + kv("last", st.last) + ", " + kv("lds", st.lds) + "}";
    }
    j += "]";
  }
  EngineDev hd;
  memcpy(&hd, &e.h, sizeof(hd));
  j += "}, \"hash\": {\"engine_dev\": " + fnv(&hd, sizeof(hd)) +
       ", \"tiles_b\": " + fnv(e.hostB.data(), e.hostB.size() * sizeof(TileDesc)) +
       ", \"tiles_d\": " + fnv(e.hostD.data(), e.hostD.size() * sizeof(TileDesc)) +
       ", \"wide_dev\": " + fnv(&e.wdh, wide ? sizeof(WideDev) : 0) +
       ", \"wjobs\": " + fnv(e.hostW.data(), wide ? e.hostW.size() * sizeof(WJob) : 0) + "}}";
  if (j.size() + 1 > cap) return fail(SAC_E_INVALID, "plan dump needs " + std::to_string(j.size() + 1) + " bytes");
  memcpy(out, j.c_str(), j.size() + 1);
  return SAC_OK;
}

// the hidden-split kernels are role kernels too
int sac_engine_uses_roles(const sac_engine* e) { return e && (e->path == PATH_ROLES || e->path == PATH_SPLIT); }

int sac_engine_uses_split(const sac_engine* e) { return e && e->path == PATH_SPLIT; }

int sac_engine_uses_pairs(const sac_engine* e) { return e && e->path == PATH_PAIRS; }

int sac_engine_uses_wide(const sac_engine* e) { return e && e->path == PATH_WIDE ? (int)e->wst.size() : 0; }

int sac_engine_phase_launches(const sac_engine* e, int32_t* out) {
  if (!e || !out) return fail(SAC_E_INVALID, "null argument");
  for (int k = 0; k < 4; ++k) out[k] = 1;
  if (e->path == PATH_WIDE) {
    for (int k = 0; k < 4; ++k) out[k] = 0;
    for (const sac_engine::WStage& st : e->wst)
      if (st.kind != 0 && st.phase >= 0 && st.phase < 4) ++out[st.phase];
  }
  return SAC_OK;
}

int sac_engine_debug_launch(sac_engine* e, const sac_replay* rb, int32_t kind, void* stream) {
  if (!e || !rb || kind < L_A || kind > L_D) return fail(SAC_E_INVALID, "bad debug_launch arguments");
  if (e->path == PATH_WIDE) {  // every launch of that phase
    for (const sac_engine::WStage& st : e->wst)
      if (st.phase == kind) launch_wide(e, st, rb, nullptr, nullptr, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return SAC_OK;
  }
  BY_PRECISION(e, launch_kind, e, kind, rb, nullptr, nullptr, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return SAC_OK;
}

int sac_engine_debug_stamped(void) {
#ifdef SAC_STAMPS
  return 1;
#else
  return 0;
#endif
}

int sac_engine_time_phases(sac_engine* e, const sac_replay* rb, int32_t n_steps, float* ms_host, void* stream) {
  if (!e || !ms_host || n_steps < 1) return fail(SAC_E_INVALID, "bad time_phases arguments");
  int rc = check_replay(e, rb);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  // events after every launch of the step sequence; a launch's time = its event
  // minus the previous one
  std::vector<int> kinds;
  std::vector<hipEvent_t> ev;
  hipEvent_t start;
  HIPCHK(hipEventCreate(&start));
  // hold the stream while the whole sequence is enqueued (~0.2 ms of host time
  // per step), so the intervals are device time, not host-submission time
  const long long hold = std::min(20000000LL, 20000LL * n_steps + 200000LL);
  sac_spin_kernel<<<1, 64, 0, s>>>(hold);
  HIPCHK(hipEventRecord(start, s));
  launch_steps(e, rb, n_steps, nullptr, nullptr, s, &kinds, &ev);
  HIPCHK(hipStreamSynchronize(s));
  double sum[4] = {0, 0, 0, 0};
  int cnt[4] = {0, 0, 0, 0};
  for (size_t i = 0; i < ev.size(); ++i) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, i ? ev[i - 1] : start, ev[i]));
    sum[kinds[i]] += ms;
    ++cnt[kinds[i]];
  }
  // per phase and step (the stage path has several launches per phase)
  auto avg = [&](int k) { return cnt[k] ? (float)(sum[k] / (e->path == PATH_WIDE ? n_steps : cnt[k])) : 0.f; };
  for (int p = 0; p < 4; ++p) ms_host[p] = avg(p);
  // the same event pattern around empty launches: the per-launch gap
  {
    const int n = 64;
    std::vector<hipEvent_t> ez(n + 1);
    for (auto& x : ez) HIPCHK(hipEventCreate(&x));
    sac_spin_kernel<<<1, 64, 0, s>>>(200000LL);  // 2 ms: every empty launch queued behind it
    HIPCHK(hipEventRecord(ez[0], s));
    for (int i = 1; i <= n; ++i) {
      sac_noop_kernel<<<1, 64, 0, s>>>();
      HIPCHK(hipEventRecord(ez[i], s));
    }
    HIPCHK(hipStreamSynchronize(s));
    double tot = 0.0;
    for (int i = 1; i <= n; ++i) {
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, ez[i - 1], ez[i]));
      tot += ms;
    }
    ms_host[4] = (float)(tot / n);
    for (auto& x : ez) (void)hipEventDestroy(x);
  }
  (void)hipEventDestroy(start);
  for (auto& x : ev) (void)hipEventDestroy(x);
  return SAC_OK;
}

}  // extern "C"
