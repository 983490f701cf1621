// Phasic Policy Gradient, auxiliary phase (phasic_policy_gradient.py:140-153, 262-280): the joint loss  L = aux_value_loss + beta_clone * policy_distance + value_head_weight * value_head_loss  with its
// gradient with respect to the network's outputs, in one pass over the rows, for categorical heads (the distributions a cache entry
// keeps are categorical.hip's srl_categorical_log_softmax rows) and for Normal heads.
//   policy_distance  = sum over heads of  sum_rows KL(old_h || new_h) (1 - done) / sum_rows (1 - done)      (:140-144)
//   *_value_loss     = 1/2 sum (v - target)^2 (1 - done) / sum_rows (1 - done)                               (:146-147)
// HBM-bound row work (a few dozen floats per row): one thread per row, no matrix cores.
#include "action_dist.h"

namespace {

// What both kinds of head share: the two value terms, the row weights and the three sums
struct AuxCommon {
  const float* aux;       // [n, vd]
  const float* pred;      // [n, vd]
  const float* target;    // [n, vd]
  const uint8_t* done;    // [n] (the cache entry's info_mask, :264)
  const double* count;    // sum over rows of (1 - done)
  long n;
  int vd;
  float beta_clone, value_head_weight;
  float* d_aux;           // [n, vd]
  float* d_pred;          // [n, vd]
  double* terms;          // [3]: auxiliary value loss, value head loss, policy distance (each already divided by count)
};

// The value terms of row i (weight w = und / count, und = 1 - done): d_aux, d_pred and the row's share of acc[0], acc[1]
__device__ __forceinline__ void aux_value_terms(const AuxCommon& c, long i, float und, float w, double (&acc)[3]) {
  for (int ch = 0; ch < c.vd; ++ch) {
    const long e = i * c.vd + ch;
    const float da = c.aux[e] - c.target[e], dp = c.pred[e] - c.target[e];
    c.d_aux[e] = da * w;
    c.d_pred[e] = c.value_head_weight * dp * w;
    acc[0] += 0.5 * (double)(da * da * und);
    acc[1] += 0.5 * (double)(dp * dp * und);
  }
}

// The workgroup's three sums, divided by the count, into terms (`red`: 4 * 3 doubles of LDS)
__device__ __forceinline__ void aux_reduce(const AuxCommon& c, double cnt, double (&acc)[3], double* red) {
  block_sum<3, 256>(acc, red);
  if (threadIdx.x == 0 && cnt > 0.0) {
#pragma unroll
    for (int i = 0; i < 3; ++i) atomicAdd(&c.terms[i], acc[i] / cnt);
  }
}

struct AuxArgs {
  AuxCommon c;
  const float* logq_old;  // [n, atot] normalised log-probabilities of the distributions kept by the cache entry
  const float* logits;    // [n, atot] raw logits of the current policy
  const uint8_t* avail;   // [n, atot] or null
  int ld_old, ld, atot;
  float* d_logits;        // [n, atot] (pitch ldd)
  int ldd;
  Heads h;
};

__global__ __launch_bounds__(256) void ppg_aux_loss_kernel(AuxArgs a) {
  __shared__ double red[4 * 3];
  double acc[3] = {0.0, 0.0, 0.0};
  const double cnt = *a.c.count;
  const float inv = cnt > 0.0 ? (float)(1.0 / cnt) : 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.c.n; i += (long)gridDim.x * 256) {
    const float und = 1.f - (float)a.c.done[i];
    const float w = und * inv;
    const float* row = a.logits + i * a.ld;
    const float* old = a.logq_old + i * a.ld_old;
    const uint8_t* av = a.avail ? a.avail + i * a.atot : nullptr;
    float* drow = a.d_logits + i * a.ldd;
    int s = 0;
    float kl = 0.f;
    for (int k = 0; k < a.h.n_heads; ++k) {
      const int d = a.h.dims[k];
      const float lse = head_norm(row, av, s, d).lse;
      for (int j = 0; j < d; ++j) {
        const float lq = masked_logit(row, av, s + j) - lse, lp = old[s + j];
        const float p = expf(lp), q = expf(lq);
        // torch.distributions.kl._kl_categorical_categorical: p (log p - log q), +inf where q == 0, 0 where p == 0
        float t = p * (lp - lq);
        if (q == 0.f) t = INFINITY;
        if (p == 0.f) t = 0.f;
        kl += t;
        // d KL / d z_j = q_j - p_j (sum p = 1); logits overwritten with the mask constant receive no gradient (:135-136)
        drow[s + j] = (av && av[s + j] == 0) ? 0.f : a.c.beta_clone * w * (q - p);
      }
      s += d;
    }
    acc[2] += (double)(kl * und);
    aux_value_terms(a.c, i, und, w, acc);
  }
  aux_reduce(a.c, cnt, acc, red);
}

struct GaussAuxArgs {
  AuxCommon c;
  const float* mean_old;     // [n, A] (pitch ld_old): the means kept by the cache entry
  const float* log_std_old;  // [A] (pitch 0) or [n, A] rows (pitch ld_ls_old): log sigma kept by the cache entry
  const float* mean;         // [n, A] (pitch ld): the current policy's means
  const float* log_std;      // [A] (pitch 0) or [n, A] rows (pitch ld_ls): the current policy's log sigma
  int ld_old, ld_ls_old, ld, ld_ls, A;
  float* d_mean;             // [n, A] (pitch ldd)
  int ldd;
  float* d_log_std;          // [n, A] or null (`fixed`: log sigma takes no gradient)
};

// Normal heads: KL(N(m0, s0) || N(m1, s1)) per action dimension as torch.distributions.kl._kl_normal_normal,
//   0.5 (r + t - 1 - log r),  r = (s0 / s1)^2,  t = ((m0 - m1) / s1)^2,
// every dimension of a row weighted by the row's (1 - done), summed over rows and dimensions, divided by the undone rows.
__global__ __launch_bounds__(256) void ppg_aux_loss_gaussian_kernel(GaussAuxArgs a) {
  __shared__ double red[4 * 3];
  double acc[3] = {0.0, 0.0, 0.0};
  const double cnt = *a.c.count;
  const float inv = cnt > 0.0 ? (float)(1.0 / cnt) : 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.c.n; i += (long)gridDim.x * 256) {
    const float und = 1.f - (float)a.c.done[i];
    const float w = und * inv;
    const float gw = a.c.beta_clone * w;
    const float* m0 = a.mean_old + i * a.ld_old;
    const float* l0 = a.log_std_old + i * a.ld_ls_old;
    const float* m1 = a.mean + i * a.ld;
    const float* l1 = a.log_std + i * a.ld_ls;
    float* dm = a.d_mean + i * a.ldd;
    float* dl = a.d_log_std ? a.d_log_std + i * a.A : nullptr;
    float kl = 0.f;
    for (int j = 0; j < a.A; ++j) {
      const float dls = l0[j] - l1[j];
      const float r = expf(2.f * dls);
      const float is1 = expf(-l1[j]);
      const float z = (m0[j] - m1[j]) * is1;
      const float t = z * z;
      kl += 0.5f * (r + t - 1.f) - dls;
      dm[j] = -gw * z * is1;                // d KL / d m1 = -(m0 - m1) exp(-2 ls1)
      if (dl) dl[j] = gw * (1.f - r - t);   // d KL / d ls1
    }
    acc[2] += (double)(kl * und);
    aux_value_terms(a.c, i, und, w, acc);
  }
  aux_reduce(a.c, cnt, acc, red);
}

}  // namespace

extern "C" int srl_ppg_aux_loss_fwd_bwd(void* stream, const float* logq_old, int ld_old, const float* logits, int ld_logits,
                                        const uint8_t* avail, long n, int n_heads, const int32_t* host_head_dims, const float* aux_value,
                                        const float* pred_value, const float* target, int value_dim, const uint8_t* done,
                                        const double* undone_count, float beta_clone, float value_head_weight, float* d_logits,
                                        int ld_dlogits, float* d_aux, float* d_pred, double* terms) {
  AuxArgs a{};
  SRL_CHECK_ARG(make_heads(n_heads, host_head_dims, a.h, a.atot) == 0, "bad head dims");
  SRL_CHECK_ARG(logq_old && logits && aux_value && pred_value && target && done && undone_count && d_logits && d_aux && d_pred && terms,
                "null tensor");
  SRL_CHECK_ARG(ld_old >= a.atot && ld_logits >= a.atot && ld_dlogits >= a.atot && value_dim >= 1 && n >= 0, "ld / value_dim");
  hipStream_t st = (hipStream_t)stream;
  SRL_HIP_TRY(hipMemsetAsync(terms, 0, 3 * sizeof(double), st));
  if (n == 0) return 0;
  a.c = AuxCommon{aux_value, pred_value, target, done, undone_count, n, value_dim, beta_clone, value_head_weight, d_aux, d_pred, terms};
  a.logq_old = logq_old; a.logits = logits; a.avail = avail; a.ld_old = ld_old; a.ld = ld_logits; a.d_logits = d_logits;
  a.ldd = ld_dlogits;
  const unsigned grid = (unsigned)(srl_ceil_div(n, 256) < 2048 ? srl_ceil_div(n, 256) : 2048);
  hipLaunchKernelGGL(ppg_aux_loss_kernel, dim3(grid), dim3(256), 0, st, a);
  SRL_LAUNCH_CHECK();
  return 0;
}

extern "C" int srl_ppg_aux_loss_gaussian_fwd_bwd(void* stream, const float* mean_old, int ld_mean_old, const float* log_std_old,
                                                 int ld_log_std_old, const float* mean, int ld_mean, const float* log_std,
                                                 int ld_log_std, long n, int A, const float* aux_value, const float* pred_value,
                                                 const float* target, int value_dim, const uint8_t* done, const double* undone_count,
                                                 float beta_clone, float value_head_weight, float* d_mean, int ld_dmean,
                                                 float* d_log_std, float* d_aux, float* d_pred, double* terms) {
  SRL_CHECK_ARG(terms, "null tensor");
  SRL_CHECK_ARG(n >= 0 && A >= 1 && value_dim >= 1 && ld_mean_old >= A && ld_mean >= A && ld_dmean >= A &&
                    (ld_log_std_old == 0 || ld_log_std_old >= A) && (ld_log_std == 0 || ld_log_std >= A),
                "ld / value_dim");
  hipStream_t st = (hipStream_t)stream;
  SRL_HIP_TRY(hipMemsetAsync(terms, 0, 3 * sizeof(double), st));
  if (n == 0) return 0;
  SRL_CHECK_ARG(mean_old && log_std_old && mean && log_std && aux_value && pred_value && target && done && undone_count && d_mean &&
                    d_aux && d_pred,
                "null tensor");
  GaussAuxArgs a{};
  a.c = AuxCommon{aux_value, pred_value, target, done, undone_count, n, value_dim, beta_clone, value_head_weight, d_aux, d_pred, terms};
  a.mean_old = mean_old; a.log_std_old = log_std_old; a.mean = mean; a.log_std = log_std; a.ld_old = ld_mean_old;
  a.ld_ls_old = ld_log_std_old; a.ld = ld_mean; a.ld_ls = ld_log_std; a.A = A; a.d_mean = d_mean; a.ldd = ld_dmean;
  a.d_log_std = d_log_std;
  // at most 512 workgroups (the categorical kernel's limit is 2048): every workgroup ends with three float64 atomics into the one
  // 24-byte `terms`, and those -- not the rows' bytes -- set the time of a large call (524 288 rows x 6: 90 us per call with 2048
  // workgroups, 60 with 1024, 40 with 512, 38 with 256, 53 with 128; measured)
  const unsigned grid = (unsigned)(srl_ceil_div(n, 256) < 512 ? srl_ceil_div(n, 256) : 512);
  hipLaunchKernelGGL(ppg_aux_loss_gaussian_kernel, dim3(grid), dim3(256), 0, st, a);
  SRL_LAUNCH_CHECK();
  return 0;
}
