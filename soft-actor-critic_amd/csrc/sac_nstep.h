// sac_nstep.h — n-step returns for the rollout path (include/sac_engine.h
// sac_replay_emit_nstep, sac_replay_emit_nstep_codes).
// One stateless kernel turns the last n vector steps' one-step rows, held in a
// staging table of n * num_envs rows, into num_envs n-step rows of the training
// replay ring.  A window an episode end closes spans k <= n steps and an open
// one exactly n; the rows train with the constant discount gamma^n and no
// kernel of the gradient step changes.  The staged done word is either the flag
// terminated | truncated, stored as it is (a closed window never bootstraps), or
// the end code terminated + 2 * truncated, from which the stored done is the
// share of gamma^n the row must not bootstrap with: 1 after a termination, 1 -
// gamma^k / gamma^n after a truncation alone.
#pragma once

// The discount powers by value in the kernel arguments: the launch keeps no
// host state.  Flags read gpow[0..n-1]; end codes read gpow[n] too.
template <int NP>
struct NStepPowersN {
  double g[NP];
};
typedef NStepPowersN<SAC_NSTEP_MAX> NStepPowers;
typedef NStepPowersN<SAC_NSTEP_MAX + 1> NStepCodePowers;

// What one environment's window gives: its oldest row, row k - 1 (the one that
// closed it, or the newest), that row's done word, R in float64, and gpow[k] /
// gpow[n] for the end codes.
struct NStepWindow {
  int64_t first, last;
  float dlast;
  double acc, gk, gn;
};

// The scan of environment i's window, the same for every lane of its wave
// (wave-uniform addresses: no divergence).  A staged done word other than 0
// closes the window, flag or end code alike.  The loops over SAC_NSTEP_MAX
// unroll, so nothing is indexed at run time.  gk and gn are read only where
// the powers hold gpow[n] (end codes).
template <int NP>
__device__ __forceinline__ NStepWindow nstep_window(const sac_replay& st, const RowStrides& ss, int n, int num_envs,
                                                    int64_t newest, int i, const NStepPowersN<NP>& gp) {
  constexpr bool CODES = NP > SAC_NSTEP_MAX;
  const int64_t scap = (int64_t)n * num_envs;
  // window step j (0 = oldest) is age n - 1 - j: slot (newest - age * num_envs + i) mod scap
  int64_t slot[SAC_NSTEP_MAX];
  float r[SAC_NSTEP_MAX], d[SAC_NSTEP_MAX];
  NStepWindow w;
  w.gn = 0.0;  // gpow[n]: set by window step n - 1
#pragma unroll
  for (int j = 0; j < SAC_NSTEP_MAX; ++j) {
    slot[j] = 0;
    r[j] = d[j] = 0.f;
    if (j < n) {
      slot[j] = (newest + i - (int64_t)(n - 1 - j) * num_envs + scap) % scap;
      r[j] = st.rew[slot[j] * ss.one];
      d[j] = st.done[slot[j] * ss.one];
      if constexpr (CODES) w.gn = gp.g[j + 1];
    }
  }
  // R = sum_{j<k} gpow[j] r_j in float64, starting from the first product (n = 1 keeps -0.0), rounded once
  w.acc = gp.g[0] * (double)r[0];
  w.first = w.last = slot[0];
  w.dlast = d[0];
  w.gk = gp.g[1];  // n = 1 without gpow[n]: never read
  bool open = d[0] == 0.f;
#pragma unroll
  for (int j = 1; j < SAC_NSTEP_MAX; ++j) {
    if (j < n && open) {
      w.acc = w.acc + gp.g[j] * (double)r[j];
      w.last = slot[j];
      w.dlast = d[j];
      if constexpr (CODES) w.gk = gp.g[j + 1];
      open = d[j] == 0.f;
    }
  }
  return w;
}

// One 64-lane wave per environment row, four waves per workgroup.  Every lane
// of a wave scans the window (nstep_window) and, with end codes, divides
// gpow[k] by gpow[n] -- on every lane, so nothing diverges before the copies;
// the lanes then copy obs and act of the oldest row and next_obs of row k-1
// column by column, lane 0 writes rew and done, thread 0 of block 0 the state
// words.  No LDS, no barrier, no atomic; no workgroup reads a word another one
// writes (stage is only read, rb only written).
template <int NP>
__device__ __forceinline__ void emit_nstep_rows(const sac_replay& st, const sac_replay& rb, int n, int num_envs,
                                                int64_t newest, const NStepPowersN<NP>& gp, int64_t pos,
                                                int64_t new_size, int64_t new_pos) {
  constexpr bool CODES = NP > SAC_NSTEP_MAX;
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);  // environment row: the same for the whole wave
  if (i < num_envs) {
    const int O = rb.obs_dim, A = rb.act_dim;
    const RowStrides ss = row_strides(st.row_stride, O, A);
    const RowStrides ds = row_strides(rb.row_stride, O, A);
    const NStepWindow w = nstep_window(st, ss, n, num_envs, newest, i, gp);
    float done = w.dlast;
    if constexpr (CODES) {
      // one float64 division, one float64 subtraction, one rounding: +0.0 at k = n, negative below
      const float share = (float)(1.0 - w.gk / w.gn);
      done = w.dlast == 0.f ? 0.f : w.dlast == 2.f ? share : 1.f;
    }
    const int64_t dst = (pos + i) % rb.capacity;
    const float* __restrict__ so = st.obs + w.first * ss.obs;
    const float* __restrict__ sn = st.next_obs + w.last * ss.obs;
    const float* __restrict__ sa = st.act + w.first * ss.act;
    for (int c = lane; c < O; c += 64) {
      rb.obs[dst * ds.obs + c] = so[c];
      rb.next_obs[dst * ds.obs + c] = sn[c];
    }
    for (int c = lane; c < A; c += 64) rb.act[dst * ds.act + c] = sa[c];
    if (lane == 0) {
      rb.rew[dst * ds.one] = (float)w.acc;
      rb.done[dst * ds.one] = done;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // as replay_push_kernel
    rb.state[0] = new_size;
    rb.state[1] = new_pos;
    rb.state[2] += 1;  // push generation: a batch phase C staged before this launch is stale
  }
}

// sac_replay_emit_nstep: the staged done words are flags
__global__ void __launch_bounds__(256) sac_replay_emit_nstep_kernel(sac_replay st, sac_replay rb, int n, int num_envs,
                                                                    int64_t newest, NStepPowers gp, int64_t pos,
                                                                    int64_t new_size, int64_t new_pos) {
  emit_nstep_rows(st, rb, n, num_envs, newest, gp, pos, new_size, new_pos);
}

// sac_replay_emit_nstep_codes: the staged done words are end codes.  A template over the powers' count, like
// their struct; the entry point instantiates it with SAC_NSTEP_MAX + 1.
template <int NP>
__global__ void __launch_bounds__(256) sac_replay_emit_nstep_codes_kernel(sac_replay st, sac_replay rb, int n,
                                                                          int num_envs, int64_t newest,
                                                                          NStepPowersN<NP> gp, int64_t pos,
                                                                          int64_t new_size, int64_t new_pos) {
  static_assert(NP == SAC_NSTEP_MAX + 1, "end codes read gpow[0..n]");
  emit_nstep_rows(st, rb, n, num_envs, newest, gp, pos, new_size, new_pos);
}
