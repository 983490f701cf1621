// Deep Q-learning: the TD step between the forward and the backward pass (dueling combine, double-Q gather, scalar transforms,
// n-step return, value loss and its gradient, priorities), the epsilon-greedy rollout head, and the target network's Polyak update.
// All of it is small streaming work: one thread per row where rows are independent (the dueling combine and the gathers, the
// sampler), one thread per batch column walking time for the n-step return; float64 registers where the reference computes in
// float64, float32 roundings where it rounds.  (Both passes of the TD step in the column walk took 390 us at 64 x 44 rows of 18
// actions -- one wavefront reading 38 floats per row, 44 rows in sequence; the row pass now runs 2816 threads wide.)
// The value loss and the sampler's Philox draw are action_dist.h's.
#include "action_dist.h"

namespace {

__device__ __forceinline__ double sign_of(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0); }

// modules/utils.py:324-328: float64 arithmetic, float32 result
__device__ __forceinline__ float scalar_transform(float x32, double eps) {
  const double x = (double)x32;
  return (float)(sign_of(x) * (sqrt(fabs(x) + 1.0) - 1.0) + eps * x);
}

// modules/utils.py:331-335
__device__ __forceinline__ float inverse_scalar_transform(float x32, double eps) {
  const double x = (double)x32;
  const double a = sqrt(1.0 + 4.0 * eps * (fabs(x) + 1.0 + eps)) - 1.0;
  const double h = a / (2.0 * eps);
  return (float)(sign_of(x) * (h * h - 1.0));
}

// mean_a adv[a] in float32 (atari_dqn_policy.py:101): Q[a] = (v + adv[a]) - mean
__device__ __forceinline__ float adv_mean(const float* adv, int A) {
  float s = 0.f;
  for (int a = 0; a < A; ++a) s += adv[a];
  return s / (float)A;
}

// first maximal index of Q[a] = (v + adv[a]) - mean, as torch.argmax documents
__device__ __forceinline__ int q_argmax(const float* adv, float v, float mean, int A, float& qmax) {
  int best = 0;
  float mx = (v + adv[0]) - mean;
  for (int a = 1; a < A; ++a) {
    const float q = (v + adv[a]) - mean;
    if (q > mx) { mx = q; best = a; }
  }
  qmax = mx;
  return best;
}

constexpr int kTdThreads = 64;  // one wavefront per workgroup: B columns spread over ceil(B / 64) compute units

struct TdArgs {
  const float *adv, *v, *tadv, *tv;
  long ld_adv, ld_tadv, ld_dadv;
  const int32_t* action;
  const float* reward;
  const uint8_t *done, *truncated;
  const float* weight;
  int T, B, A;
  srl_dqn_hparams hp;
  float *d_adv, *d_v;
  double* terms;
  float* priorities;
};

// Per row, both nets' dueling combine: the bootstrap value tq'[row] is left in d_v[row] and, for the S loss rows, q[row] in
// d_adv[row][0], until the column kernel overwrites them with the gradient; and the sum of the loss mask 1 - done over the loss
// rows, which every mean of the step divides by (deep_q_learning.py:159).  Rows are independent here: one thread each.
__global__ __launch_bounds__(256) void dqn_rows_kernel(TdArgs p) {
  const long row = (long)blockIdx.x * 256 + threadIdx.x;
  const int A = p.A;
  const srl_dqn_hparams hp = p.hp;
  double c = 0.0;
  if (row < (long)p.T * p.B) {
    const float* ar = p.adv + row * p.ld_adv;
    const float* tr = p.tadv + row * p.ld_tadv;
    const float v = p.v[row], tv = p.tv[row];
    const float mean = adv_mean(ar, A), tmean = adv_mean(tr, A);
    float qmax, tqmax;
    const int greedy = q_argmax(ar, v, mean, A, qmax);
    q_argmax(tr, tv, tmean, A, tqmax);
    float tq = hp.double_q ? (tv + tr[greedy]) - tmean : tqmax;
    if (hp.apply_scalar_transform) tq = inverse_scalar_transform(tq, hp.scalar_transform_eps);
    p.d_v[row] = tq;
    if (row < (long)(p.T - hp.n) * p.B) {
      const int act = min(max(p.action[row], 0), A - 1);  // never read past the row
      p.d_adv[row * p.ld_dadv] = (v + ar[act]) - mean;
      c = p.done[row] ? 0.0 : 1.0;
    }
  }
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0 && c != 0.0) atomicAdd(&p.terms[SRL_DQ_MASK], c);
}

__global__ __launch_bounds__(kTdThreads) void dqn_td_kernel(TdArgs p) {
  const int b = blockIdx.x * kTdThreads + threadIdx.x;
  const int T = p.T, B = p.B, A = p.A, n = p.hp.n, S = T - n;
  const srl_dqn_hparams hp = p.hp;
  double acc[SRL_DQ_COUNT];
#pragma unroll
  for (int i = 0; i < SRL_DQ_COUNT; ++i) acc[i] = 0.0;
  float td_max_all = 0.f;

  if (b < B) {
    // n-step return (modules/n_step_return.py:36-50, float64) from what dqn_rows_kernel left, loss, gradient, statistics.  This
    // thread owns the column: nobody else reads the rows it overwrites
    const float inv_n = (float)(1.0 / p.terms[SRL_DQ_MASK]);
    const float w = p.weight ? p.weight[b] : 1.0f;
    const float inv_A = 1.0f / (float)A;
    float td_sum = 0.f, td_max = 0.f, cnt = 0.f;
    for (int t = 0; t < S; ++t) {
      const long row = (long)t * B + b;
      double ret = 0.0, disc = 1.0;
      for (int i = 0; i < n; ++i) {
        const long r = (long)(t + i) * B + b, nx = r + B;
        const double nv = (double)p.d_v[nx];
        const double nd = (double)p.done[nx], nt = (double)p.truncated[nx];
        ret += (double)p.reward[r] * disc;
        ret += disc * hp.gamma * nt * nv;  // the next step is truncated: bootstrap in advance
        disc *= hp.gamma * (1.0 - nd) * (1.0 - nt);
      }
      float y = (float)(ret + disc * (double)p.d_v[(long)(t + n) * B + b]);
      if (hp.apply_scalar_transform) y = scalar_transform(y, hp.scalar_transform_eps);
      float* drow = p.d_adv + row * p.ld_dadv;
      const float q = drow[0];
      const float m = p.done[row] ? 0.f : 1.f;
      float l, dl;
      vloss(hp.value_loss, hp.huber_delta, q, y, l, dl);
      const float g = w * dl * m * inv_n;
      const int act = p.action[row];
      for (int a = 0; a < A; ++a) drow[a] = g * ((a == act ? 1.f : 0.f) - inv_A);
      p.d_v[row] = g;
      const float td = fabsf(q - y);
      td_sum += td * m;
      td_max = fmaxf(td_max, td * m);
      cnt += m;
      if (m != 0.f) {
        acc[SRL_DQ_VLOSS] += (double)(w * l);
        acc[SRL_DQ_Q] += (double)q;
        acc[SRL_DQ_Y] += (double)y;
        // denormalised for logging, with the transform's DEFAULT eps (deep_q_learning.py:190-192)
        acc[SRL_DQ_QINV] += (double)(hp.apply_scalar_transform ? inverse_scalar_transform(q, 1e-3) : q);
        acc[SRL_DQ_YINV] += (double)(hp.apply_scalar_transform ? inverse_scalar_transform(y, 1e-3) : y);
        acc[SRL_DQ_TD] += (double)td;
        td_max_all = fmaxf(td_max_all, td);
      }
    }
    for (int t = S; t < T; ++t) {
      const long row = (long)t * B + b;
      float* drow = p.d_adv + row * p.ld_dadv;
      for (int a = 0; a < A; ++a) drow[a] = 0.f;
      p.d_v[row] = 0.f;
    }
    // deep_q_learning.py:175-179 in float32; a column whose loss rows are all done gives 0/0 = NaN like the reference
    p.priorities[b] = (float)hp.priority_interpolation_eta * td_max +
                      (float)(1.0 - hp.priority_interpolation_eta) * (td_sum / cnt);
  }
#pragma unroll
  for (int i = 0; i < SRL_DQ_COUNT; ++i) acc[i] = wave_sum(acc[i]);
  td_max_all = wave_allmax(td_max_all);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < SRL_DQ_COUNT; ++i)
      if (i != SRL_DQ_MASK && i != SRL_DQ_TDMAX) atomicAdd(&p.terms[i], acc[i]);
    // non-negative doubles order like their bit patterns
    atomicMax((unsigned long long*)&p.terms[SRL_DQ_TDMAX], (unsigned long long)__double_as_longlong((double)td_max_all));
  }
}

__global__ __launch_bounds__(256) void epsilon_greedy_kernel(const float* adv, long ld_adv, const float* v, const float* tadv,
                                                             long ld_tadv, const float* tv, const float* epsilon,
                                                             const uint8_t* is_eval, long n, int A, int double_q, uint64_t seed,
                                                             uint64_t offset, long row0, int64_t* action, float* value,
                                                             float* target_value) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* ar = adv + i * ld_adv;
  const float* tr = tadv + i * ld_tadv;
  const float vi = v[i], tvi = tv[i];
  const float mean = adv_mean(ar, A), tmean = adv_mean(tr, A);
  float qmax, tqmax;
  const int greedy = q_argmax(ar, vi, mean, A, qmax);
  q_argmax(tr, tvi, tmean, A, tqmax);
  int pick = greedy;
  if (!(is_eval && is_eval[i])) {
    const uint4 rnd = philox_draw((uint64_t)(row0 + i), 0u, offset, seed);  // the row's number in the caller's whole batch
    const float u = u24(rnd.x);
    // floor((x1 >> 8) 2^-24 A) in integers: never A
    if (!(u > epsilon[i])) pick = (int)(((uint64_t)(rnd.y >> 8) * (uint64_t)A) >> 24);
  }
  action[i] = pick;
  value[i] = (vi + ar[pick]) - mean;
  target_value[i] = double_q ? (tvi + tr[greedy]) - tmean : tqmax;
}

// target = target (1 - tau) + param tau, each product and the sum rounded once like the torch ops of modules/utils.py:309
__global__ __launch_bounds__(256) void polyak_kernel(float* target, const float* param, long n, float keep, float tau, int copy) {
  const long n4 = ((((uintptr_t)target | (uintptr_t)param) & 15) == 0) ? n / 4 : 0;
  const long stride = (long)gridDim.x * 256, tid = (long)blockIdx.x * 256 + threadIdx.x;
  float4* t4 = (float4*)target;
  const float4* p4 = (const float4*)param;
  for (long i = tid; i < n4; i += stride) {
    const float4 s = p4[i];
    float4 d = t4[i];
    d.x = copy ? s.x : __fadd_rn(__fmul_rn(d.x, keep), __fmul_rn(s.x, tau));
    d.y = copy ? s.y : __fadd_rn(__fmul_rn(d.y, keep), __fmul_rn(s.y, tau));
    d.z = copy ? s.z : __fadd_rn(__fmul_rn(d.z, keep), __fmul_rn(s.z, tau));
    d.w = copy ? s.w : __fadd_rn(__fmul_rn(d.w, keep), __fmul_rn(s.w, tau));
    t4[i] = d;
  }
  for (long i = n4 * 4 + tid; i < n; i += stride)
    target[i] = copy ? param[i] : __fadd_rn(__fmul_rn(target[i], keep), __fmul_rn(param[i], tau));
}

}  // namespace

extern "C" int srl_dqn_td_fwd_bwd(void* stream, const float* adv, int64_t ld_adv, const float* v, const float* target_adv,
                                  int64_t ld_target_adv, const float* target_v, const int32_t* action, const float* reward,
                                  const uint8_t* done, const uint8_t* truncated, const float* weight, int T, int B, int A,
                                  const srl_dqn_hparams* hp, float* d_adv, int64_t ld_dadv, float* d_v, double* terms,
                                  float* priorities) {
  SRL_CHECK_ARG(hp && hp->n >= 1 && T > hp->n && B >= 1 && A >= 1, "need bootstrap_steps >= 1, T > bootstrap_steps, B, A >= 1");
  SRL_CHECK_ARG(adv && v && target_adv && target_v && action && reward && done && truncated, "null input");
  SRL_CHECK_ARG(d_adv && d_v && terms && priorities, "null output");
  SRL_CHECK_ARG(ld_adv >= A && ld_target_adv >= A && ld_dadv >= A, "row pitch below A");
  SRL_CHECK_ARG(hp->value_loss >= 0 && hp->value_loss <= 2, "value_loss must be 0|1|2");
  hipStream_t st = (hipStream_t)stream;
  SRL_HIP_TRY(hipMemsetAsync(terms, 0, SRL_DQ_COUNT * sizeof(double), st));
  TdArgs p{adv, v, target_adv, target_v, (long)ld_adv, (long)ld_target_adv, (long)ld_dadv, action, reward, done, truncated,
           weight, T, B, A, *hp, d_adv, d_v, terms, priorities};
  hipLaunchKernelGGL(dqn_rows_kernel, dim3((unsigned)srl_ceil_div((long)T * B, 256)), dim3(256), 0, st, p);
  SRL_LAUNCH_CHECK();
  hipLaunchKernelGGL(dqn_td_kernel, dim3((unsigned)srl_ceil_div(B, kTdThreads)), dim3(kTdThreads), 0, st, p);
  SRL_LAUNCH_CHECK();
  return 0;
}

extern "C" int srl_epsilon_greedy_sample(void* stream, const float* adv, int64_t ld_adv, const float* v,
                                         const float* target_adv, int64_t ld_target_adv, const float* target_v,
                                         const float* epsilon, const uint8_t* is_eval, long n, int A, int double_q,
                                         uint64_t seed, uint64_t offset, int64_t row0, int64_t* action, float* value,
                                         float* target_value) {
  SRL_CHECK_ARG(n >= 0 && A >= 1 && ld_adv >= A && ld_target_adv >= A, "n >= 0, A >= 1 and row pitches >= A required");
  SRL_CHECK_ARG(adv && v && target_adv && target_v && epsilon, "null input");
  SRL_CHECK_ARG(action && value && target_value, "null output");
  if (n == 0) return 0;
  hipLaunchKernelGGL(epsilon_greedy_kernel, dim3((unsigned)srl_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, adv,
                     (long)ld_adv, v, target_adv, (long)ld_target_adv, target_v, epsilon, is_eval, n, A, double_q, seed, offset,
                     (long)row0, action, value, target_value);
  SRL_LAUNCH_CHECK();
  return 0;
}

extern "C" int srl_polyak_update(void* stream, float* target, const float* param, int64_t n, double tau) {
  SRL_CHECK_ARG(n >= 0 && tau >= 0.0 && tau <= 1.0, "n >= 0 and 0 <= tau <= 1 required");
  SRL_CHECK_ARG(n == 0 || (target && param), "null buffer");
  if (n == 0) return 0;
  const long cap = 2048;
  const long blocks = srl_ceil_div(srl_ceil_div(n, 4), 256);
  hipLaunchKernelGGL(polyak_kernel, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(256), 0, (hipStream_t)stream, target,
                     param, (long)n, (float)(1.0 - tau), (float)tau, tau == 1.0 ? 1 : 0);
  SRL_LAUNCH_CHECK();
  return 0;
}
