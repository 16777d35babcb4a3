// sac_math.h — scalar arithmetic of the algorithm as host/device functions: the acting form of the squashed-Gaussian
// head (reference sac/models.py:79-91), the TD target and the critics' seed (agent.py:195-236), the min-Q weights and
// the policy-loss term (agent.py:244-252), and the constants and softplus the training head uses.  Called where the
// call leaves the kernel instruction for instruction what the hand-written text gave: sac_policy_act_kernel, the
// rollout body (sac_envs.h) and the stage path's WR_YSEED / WR_MINQ prologues (sac_wide.h).  The row-tile, split and
// pair kernels keep the same arithmetic written out: there a call changes the schedule and costs about half a percent
// of the step rate.  No loads, stores, shuffles or descriptor; with -ffp-contract=off a force-inlined call
// yields the bits of the text it replaced, and the operand order of every expression is part of the fp32 parity
// contract.  Host-callable so the C ABI can export the same inline code (sac_debug_head_host).
#pragma once
#include "sac_device.h"

#define SAC_HD __host__ __device__ __forceinline__

#define LOG2F 0.69314718055994530942f
#define HALF_LOG_2PI 0.91893853320467274178f

// torch.min of two values: a NaN in either propagates
SAC_HD float fmin_nan(float a, float b) { return (a != a) ? a : (a < b ? a : b); }

// torch softplus(beta=1, threshold=20) and its derivative
SAC_HD float softplus20(float x) { return x > 20.f ? x : log1pf(expf(x)); }
SAC_HD float softplus20_grad(float x) {
  if (x > 20.f) return 1.f;
  const float z = expf(x);
  return z / (z + 1.f);
}

// ----------------------------------------------------------------------------- acting head
// log sigma clamped to [lo, hi] (models.py:81); one action dim's tanh correction (models.py:86)
SAC_HD float head_clamp(float lsr, float lo, float hi) { return lsr < lo ? lo : (lsr > hi ? hi : lsr); }
SAC_HD float head_corr(float z) { return 2.f * ((LOG2F - z) - softplus20(-2.f * z)); }

// Acting form: z = mu + e sd and the sampled action (head_act_mean: the deterministic one); with head_act_lp and
// head_corr, the log pi terms of a sampled dim
struct HeadAct { float ls, z, act; };
SAC_HD HeadAct head_act(float mu, float lsr, float e, float lo, float hi, float scale) {
  HeadAct a;
  a.ls = head_clamp(lsr, lo, hi);
  const float sd = expf(a.ls);
  a.z = mu + e * sd;
  a.act = tanhf(a.z) * scale;
  return a;
}
SAC_HD float head_act_mean(float mu, float scale) { return tanhf(mu) * scale; }
// (z - mu)^2 / (2 sd^2) = e^2 / 2 and log sd = ls, taken from e and ls themselves: z - mu
// loses e * sd to rounding once sd is far below |mu| (at the lower clamp, sd = e^-20, all of it)
SAC_HD float head_act_lp(float e, float ls) { return -0.5f * e * e - ls - HALF_LOG_2PI; }

// ----------------------------------------------------------------------------- target, seeds, min-Q
// y = r + gamma (1 - d) (min Q_target - alpha log pi') (agent.py:205-211)
SAC_HD float td_target(float r, float d, float gamma, float q1t, float q2t, float alpha32, float lp) {
  return r + (gamma * (1.f - d)) * (fmin_nan(q1t, q2t) - alpha32 * lp);
}

// mse_loss of one critic row: d = q - y feeds the loss partial, seed = dL/dq; the caller zeroes invalid rows
struct CriticSeed { float d, seed; };
SAC_HD CriticSeed critic_seed(float q, float y, int B) {
  CriticSeed s;
  s.d = q - y;
  s.seed = (2.0f / (float)B) * s.d;
  return s;
}

// min(Q1, Q2) and its backward for the caller's gm = v ? -1/B : 0: the smaller critic takes gm, a tie gives each half
struct MinQ { float m, w1, w2; };
SAC_HD MinQ minq_weights(float q1, float q2, float gm) {
  MinQ w;
  w.m = fmin_nan(q1, q2);
  w.w1 = (q1 == q2) ? gm * 0.5f : (q1 > q2 ? 0.f : gm);
  w.w2 = (q1 == q2) ? gm * 0.5f : (q1 < q2 ? 0.f : gm);
  return w;
}
// one row's term of L_pi = mean(alpha log pi - min Q) (agent.py:251-252)
SAC_HD float pi_loss_term(float alpha32, float lp, float m) { return alpha32 * lp - m; }
