// The row arithmetic of the action heads, once: the Philox4x32-10 draw and its counter layout, the masked categorical head (its
// normalisation and entropy), the Normal log-probability and entropy, and the value loss.  No kernels, no layout, no reductions:
// categorical.hip, gaussian.hip, ppo_loss.hip, ppg.hip and dqn.hip bring the rows and place the results.  Every caller evaluates
// exactly these expressions, in this operand order and grouping, which is what lets one host restatement (tests/loss_ref.py) pin
// them all: the counter word by word, a dead head's exact zeros, the value loss's branch points.
#pragma once
#include "srl_common.h"

namespace {

// ---- Philox4x32-10 (Salmon et al. 2011, "Parallel random numbers: as easy as 1, 2, 3") ------------------------------------------
__device__ __forceinline__ uint4 philox4x32_10(uint4 ctr, uint2 key) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, ctr.x), lo0 = M0 * ctr.x;
    const uint32_t hi1 = __umulhi(M1, ctr.z), lo1 = M1 * ctr.z;
    ctr = make_uint4(hi1 ^ ctr.y ^ key.x, lo1, hi0 ^ ctr.w ^ key.y, lo0);
    key.x += W0;
    key.y += W1;
  }
  return ctr;
}

// The four words of one draw.  counter = {row low, row high, stream, offset low}, key = {seed low, seed high}: `row` is the row's
// number in the caller's whole batch (pieces of a batch sample what the whole would), `stream` tells a row's draws apart (the head
// of a categorical action, the dimension of a Normal one, 0 for epsilon-greedy), and only the offset's low word enters.
__device__ __forceinline__ uint4 philox_draw(uint64_t row, uint32_t stream, uint64_t offset, uint64_t seed) {
  return philox4x32_10(make_uint4((uint32_t)row, (uint32_t)(row >> 32), stream, (uint32_t)offset),
                       make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
}

// uniform in [0, 1) from the top 24 bits of a word: exact in float32
__device__ __forceinline__ float u24(uint32_t x) { return (float)(x >> 8) * (1.0f / 16777216.0f); }

// ---- categorical heads: a row of logits is n_heads segments of dims[k] actions --------------------------------------------------
struct Heads {
  int n_heads;
  int dims[SRL_MAX_HEADS];
};

inline int make_heads(int n_heads, const int32_t* dims, Heads& h, int& atot) {
  if (n_heads < 1 || n_heads > SRL_MAX_HEADS || !dims) return -1;
  h.n_heads = n_heads;
  atot = 0;
  for (int k = 0; k < n_heads; ++k) {
    if (dims[k] < 1) return -1;
    h.dims[k] = dims[k];
    atot += dims[k];
  }
  return 0;
}

constexpr float kMaskedLogit = -1e10f;  // actor_critic_policy.py:136

__device__ __forceinline__ float masked_logit(const float* row, const uint8_t* av, int j) {
  return (av && av[j] == 0) ? kMaskedLogit : row[j];
}

// The normalisation of the head at row[s .. s + d): mx = max z, se = sum exp(z - mx), lse = logsumexp z, over the masked logits z.
// A head with no available action has every z = -1e10, where float32 is spaced 1024 apart: lse = fl(-1e10 + log d) = -1e10 and
// every normalised logit z - lse is exactly 0 (tests/loss_ref.py derives the head's zero log-probability and entropy from this).
struct HeadNorm { float mx, se, lse; };
// ... from a maximum the caller has (the sampler finds it together with its first index)
__device__ __forceinline__ HeadNorm head_norm(const float* row, const uint8_t* av, int s, int d, float mx) {
  float se = 0.f;
  for (int j = 0; j < d; ++j) se += expf(masked_logit(row, av, s + j) - mx);
  return {mx, se, mx + logf(se)};
}
__device__ __forceinline__ HeadNorm head_norm(const float* row, const uint8_t* av, int s, int d) {
  float mx = -INFINITY;
  for (int j = 0; j < d; ++j) mx = fmaxf(mx, masked_logit(row, av, s + j));
  return head_norm(row, av, s, d, mx);
}

// Categorical.entropy of the head: -sum p log p
__device__ __forceinline__ float head_entropy(const float* row, const uint8_t* av, int s, int d, float lse) {
  float hk = 0.f;
  for (int j = 0; j < d; ++j) {
    const float nl = masked_logit(row, av, s + j) - lse;  // normalised logit = log p
    hk -= expf(nl) * nl;
  }
  return hk;
}

// ---- Normal heads (torch/distributions/normal.py), one action dimension: d = x - mu, sd = sigma ---------------------------------
constexpr float kHalfLog2Pi = 0.91893853320467274178f;  // log sqrt(2 pi)

__device__ __forceinline__ float normal_log_prob(float d, float sd) {
  return -(d * d) / (2.f * sd * sd) - logf(sd) - kHalfLog2Pi;
}
__device__ __forceinline__ float normal_entropy(float sd) { return 0.5f + kHalfLog2Pi + logf(sd); }

// ---- value loss: nn.MSELoss / nn.HuberLoss(delta) / nn.SmoothL1Loss(beta = delta), reduction='none' (kind 0 | 1 | 2), l(v, target)
// and dl/dv.  The critic's loss of PPO (modules/utils.py:228-265) and the TD loss of Q-learning (modules/utils.py:242-265).
__device__ __forceinline__ void vloss(int kind, float delta, float v, float target, float& l, float& dl) {
  const float d = v - target;
  if (kind == 0) {
    l = d * d;
    dl = 2.0f * d;
    return;
  }
  const float a = fabsf(d);
  const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
  if (kind == 1) {
    if (a <= delta) { l = 0.5f * d * d; dl = d; }
    else { l = delta * (a - 0.5f * delta); dl = delta * sgn; }
  } else {
    if (a < delta) { l = 0.5f * d * d / delta; dl = d / delta; }
    else { l = a - 0.5f * delta; dl = sgn; }
  }
}

}  // namespace
