// Categorical action heads (discrete and multi-discrete actions): torch.distributions.Categorical per head on
// masked_fill(avail == 0, -1e10) as the reference uses it (legacy/algorithm/ppo/actor_critic_policies/actor_critic_policy.py:135-136,
// 311-324): log-probability and entropy summed over the heads, their gradient, the rollout's Philox inverse-CDF sampler, and the
// normalised logits a PPG cache entry keeps.  HBM-bound streaming work: one thread per row, coalesced float32 streams; the head
// arithmetic itself is action_dist.h's.
#include "action_dist.h"

namespace {

__global__ __launch_bounds__(256) void categorical_fwd_kernel(const float* logits, int ld, const int32_t* action,
                                                              const uint8_t* avail, long n, Heads h, int atot,
                                                              float* logp, float* entropy) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* row = logits + i * ld;
  const uint8_t* av = avail ? avail + i * atot : nullptr;
  float lp = 0.f, ent = 0.f;
  int s = 0;
  for (int k = 0; k < h.n_heads; ++k) {
    const int d = h.dims[k];
    const HeadNorm nm = head_norm(row, av, s, d);
    const float hk = head_entropy(row, av, s, d, nm.lse);
    lp += masked_logit(row, av, s + action[i * h.n_heads + k]) - nm.lse;
    ent += hk;
    s += d;
  }
  logp[i] = lp;
  entropy[i] = ent;
}

__global__ __launch_bounds__(256) void categorical_bwd_kernel(const float* logits, int ld, const int32_t* action,
                                                              const uint8_t* avail, long n, Heads h, int atot,
                                                              const float* d_logp, const float* d_entropy,
                                                              float* d_logits, int ldd) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* row = logits + i * ld;
  const uint8_t* av = avail ? avail + i * atot : nullptr;
  float* drow = d_logits + i * ldd;
  const float glp = d_logp[i], gent = d_entropy[i];
  int s = 0;
  for (int k = 0; k < h.n_heads; ++k) {
    const int d = h.dims[k];
    const HeadNorm nm = head_norm(row, av, s, d);
    const float hk = head_entropy(row, av, s, d, nm.lse);
    const int act = action[i * h.n_heads + k];
    for (int j = 0; j < d; ++j) {
      const float nl = masked_logit(row, av, s + j) - nm.lse;
      const float pj = expf(nl);
      // d logp / d z_j = 1[j==a] - p_j ;  d H / d z_j = -p_j (log p_j + H)
      float g = glp * ((j == act ? 1.f : 0.f) - pj) - gent * pj * (nl + hk);
      if (av && av[s + j] == 0) g = 0.f;  // overwritten logits receive no gradient (:135-136)
      drow[s + j] = g;
    }
    s += d;
  }
}

__global__ __launch_bounds__(256) void categorical_sample_kernel(const float* logits, int ld, const uint8_t* avail,
                                                                 const uint8_t* is_eval, long n, Heads h, int atot,
                                                                 uint64_t seed, uint64_t offset, int64_t* action_out,
                                                                 float* logp, long row0) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t ctr_row = (uint64_t)(row0 + i);  // the row's number in the caller's whole batch: pieces of it sample alike
  const float* row = logits + i * ld;
  const uint8_t* av = avail ? avail + i * atot : nullptr;
  const bool greedy = is_eval && is_eval[i];
  float lp = 0.f;
  int s = 0;
  for (int k = 0; k < h.n_heads; ++k) {
    const int d = h.dims[k];
    // its own max pass: the evaluation pick is the first maximal index
    float mx = -INFINITY;
    int amax = 0;
    for (int j = 0; j < d; ++j) {
      const float z = masked_logit(row, av, s + j);
      if (z > mx) { mx = z; amax = j; }  // first maximum, like argmax on probs
    }
    const HeadNorm nm = head_norm(row, av, s, d, mx);
    int pick = amax;
    if (!greedy) {
      const float u = u24(philox_draw(ctr_row, (uint32_t)k, offset, seed).x) * nm.se;  // uniform in [0, se)
      float cdf = 0.f;
      pick = -1;
      int last_ok = amax;
      for (int j = 0; j < d; ++j) {
        const float e = expf(masked_logit(row, av, s + j) - mx);
        if (e > 0.f) last_ok = j;
        cdf += e;
        if (pick < 0 && u < cdf) pick = j;
      }
      if (pick < 0) pick = last_ok;  // rounding at the top of the CDF
    }
    action_out[i * h.n_heads + k] = pick;
    lp += masked_logit(row, av, s + pick) - nm.lse;
    s += d;
  }
  logp[i] = lp;
}

// out[i, head segment] = masked logits - logsumexp: what torch.distributions.Categorical(logits=...) keeps as `.logits`
__global__ __launch_bounds__(256) void categorical_log_softmax_kernel(const float* logits, int ld, const uint8_t* avail, long n, Heads h,
                                                                      int atot, float* out, int ldo) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* row = logits + i * ld;
  const uint8_t* av = avail ? avail + i * atot : nullptr;
  float* o = out + i * ldo;
  int s = 0;
  for (int k = 0; k < h.n_heads; ++k) {
    const int d = h.dims[k];
    const HeadNorm nm = head_norm(row, av, s, d);
    for (int j = 0; j < d; ++j) o[s + j] = masked_logit(row, av, s + j) - nm.lse;
    s += d;
  }
}

}  // namespace

extern "C" int srl_categorical_fwd(void* stream, const float* logits, int ld_logits, const int32_t* action,
                                   const uint8_t* avail, long n, int n_heads, const int32_t* host_head_dims,
                                   float* logp, float* entropy) {
  Heads h;
  int atot;
  SRL_CHECK_ARG(make_heads(n_heads, host_head_dims, h, atot) == 0, "bad head dims");
  SRL_CHECK_ARG(logits && action && logp && entropy && ld_logits >= atot, "null tensor / ld");
  if (n == 0) return 0;
  hipLaunchKernelGGL(categorical_fwd_kernel, dim3((unsigned)srl_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream,
                     logits, ld_logits, action, avail, n, h, atot, logp, entropy);
  SRL_LAUNCH_CHECK();
  return 0;
}

extern "C" int srl_categorical_bwd(void* stream, const float* logits, int ld_logits, const int32_t* action,
                                   const uint8_t* avail, long n, int n_heads, const int32_t* host_head_dims,
                                   const float* d_logp, const float* d_entropy, float* d_logits, int ld_dlogits) {
  Heads h;
  int atot;
  SRL_CHECK_ARG(make_heads(n_heads, host_head_dims, h, atot) == 0, "bad head dims");
  SRL_CHECK_ARG(logits && action && d_logp && d_entropy && d_logits && ld_logits >= atot && ld_dlogits >= atot,
                "null tensor / ld");
  if (n == 0) return 0;
  hipLaunchKernelGGL(categorical_bwd_kernel, dim3((unsigned)srl_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream,
                     logits, ld_logits, action, avail, n, h, atot, d_logp, d_entropy, d_logits, ld_dlogits);
  SRL_LAUNCH_CHECK();
  return 0;
}

extern "C" int srl_categorical_sample(void* stream, const float* logits, int ld_logits, const uint8_t* avail,
                                      const uint8_t* is_eval, long n, int n_heads, const int32_t* host_head_dims,
                                      uint64_t seed, uint64_t offset, int64_t* action_out, float* logp, int64_t row0) {
  Heads h;
  int atot;
  SRL_CHECK_ARG(make_heads(n_heads, host_head_dims, h, atot) == 0, "bad head dims");
  SRL_CHECK_ARG(logits && action_out && logp && ld_logits >= atot, "null tensor / ld");
  if (n == 0) return 0;
  hipLaunchKernelGGL(categorical_sample_kernel, dim3((unsigned)srl_ceil_div(n, 256)), dim3(256), 0,
                     (hipStream_t)stream, logits, ld_logits, avail, is_eval, n, h, atot, seed, offset, action_out,
                     logp, (long)row0);
  SRL_LAUNCH_CHECK();
  return 0;
}

extern "C" int srl_categorical_log_softmax(void* stream, const float* logits, int ld_logits, const uint8_t* avail, long n, int n_heads,
                                           const int32_t* host_head_dims, float* out, int ld_out) {
  Heads h;
  int atot;
  SRL_CHECK_ARG(make_heads(n_heads, host_head_dims, h, atot) == 0, "bad head dims");
  SRL_CHECK_ARG(logits && out && ld_logits >= atot && ld_out >= atot && n >= 0, "null tensor / ld");
  if (n == 0) return 0;
  hipLaunchKernelGGL(categorical_log_softmax_kernel, dim3((unsigned)srl_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, logits,
                     ld_logits, avail, n, h, atot, out, ld_out);
  SRL_LAUNCH_CHECK();
  return 0;
}
