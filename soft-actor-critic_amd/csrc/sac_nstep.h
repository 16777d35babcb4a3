// sac_nstep.h — n-step returns for the rollout path (include/sac_engine.h
// sac_replay_emit_nstep).  One stateless kernel turns the last
// n vector steps' one-step rows, held in a staging table of n * num_envs rows,
// into num_envs n-step rows of the training replay ring.  The stored done is
// terminated | truncated, so a window an episode end closes never bootstraps
// and an open one spans exactly n steps: the rows train with the constant
// discount gamma^n and no kernel of the gradient step changes.
#pragma once

// gpow[0..n-1] by value in the kernel arguments: the launch keeps no host state
struct NStepPowers {
  double g[SAC_NSTEP_MAX];
};

// One 64-lane wave per environment row, four waves per workgroup.  Every lane
// of a wave reads the window's n reward and done words (wave-uniform
// addresses: no divergence) and computes k and R; the lanes then copy obs and
// act of the oldest row and next_obs of row k-1 column by column, lane 0 writes
// rew and done, thread 0 of block 0 the state words.  No LDS, no barrier, no
// atomic; no workgroup reads a word another one writes (stage is only read, rb
// only written).
__global__ void __launch_bounds__(256) sac_replay_emit_nstep_kernel(sac_replay st, sac_replay rb, int n, int num_envs,
                                                                    int64_t newest, NStepPowers gp, int64_t pos,
                                                                    int64_t new_size, int64_t new_pos) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);  // environment row: the same for the whole wave
  if (i < num_envs) {
    const int O = rb.obs_dim, A = rb.act_dim;
    const RowStrides ss = row_strides(st.row_stride, O, A);
    const RowStrides ds = row_strides(rb.row_stride, O, A);
    const int64_t scap = (int64_t)n * num_envs;
    // window step j (0 = oldest) is age n - 1 - j: slot (newest - age * num_envs + i) mod scap
    int64_t slot[SAC_NSTEP_MAX];
    float r[SAC_NSTEP_MAX], d[SAC_NSTEP_MAX];
#pragma unroll
    for (int j = 0; j < SAC_NSTEP_MAX; ++j) {
      slot[j] = 0;
      r[j] = d[j] = 0.f;
      if (j < n) {
        slot[j] = (newest + i - (int64_t)(n - 1 - j) * num_envs + scap) % scap;
        r[j] = st.rew[slot[j] * ss.one];
        d[j] = st.done[slot[j] * ss.one];
      }
    }
    // R = sum_{j<k} gpow[j] r_j in float64, starting from the first product (n = 1 keeps -0.0), rounded once
    double acc = gp.g[0] * (double)r[0];
    int64_t last = slot[0];
    float dlast = d[0];
    bool open = d[0] == 0.f;
#pragma unroll
    for (int j = 1; j < SAC_NSTEP_MAX; ++j) {
      if (j < n && open) {
        acc = acc + gp.g[j] * (double)r[j];
        last = slot[j];
        dlast = d[j];
        open = d[j] == 0.f;
      }
    }
    const int64_t dst = (pos + i) % rb.capacity;
    const float* __restrict__ so = st.obs + slot[0] * ss.obs;
    const float* __restrict__ sn = st.next_obs + last * ss.obs;
    const float* __restrict__ sa = st.act + slot[0] * ss.act;
    for (int c = lane; c < O; c += 64) {
      rb.obs[dst * ds.obs + c] = so[c];
      rb.next_obs[dst * ds.obs + c] = sn[c];
    }
    for (int c = lane; c < A; c += 64) rb.act[dst * ds.act + c] = sa[c];
    if (lane == 0) {
      rb.rew[dst * ds.one] = (float)acc;
      rb.done[dst * ds.one] = dlast;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // as replay_push_kernel
    rb.state[0] = new_size;
    rb.state[1] = new_pos;
    rb.state[2] += 1;  // push generation: a batch phase C staged before this launch is stale
  }
}
