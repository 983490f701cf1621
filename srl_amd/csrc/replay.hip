// Prioritised experience replay resident in HBM (srl_amd/runtime/replay.py): the two segment trees of the reference's
// PrioritizedReplayBuffer (base/buffer.py:280-465, base/segment_tree.py) as float64[2 * capacity] device arrays, the stratified
// draw with its importance weights, the priority update, and the time-major gather of the drawn sequences from the store.
// Every float64 expression is evaluated once, in the order written, with no FMA contraction: the numpy float64 statement of
// runtime/replay.py then gives the same bits (pow apart, which is the device library's).
#include "srl_common.h"
#include "action_dist.h"

#pragma STDC FP_CONTRACT OFF

namespace {

constexpr int kSetThreads = 1024;

// Loads and stores that go to the device's coherent level: the set kernel's phases hand values between the threads of its one
// workgroup through global memory (atomics resolve there), and a plain load may be served by a line the CU read before.
__device__ __forceinline__ double ld_node(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_node(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ bool accepted(float p, int slot, int n_slots) {
  return isfinite(p) && p > 0.f && slot >= 0 && slot < n_slots;
}

// One workgroup, four phases separated by barriers; thread k owns the pairs k, k + 1024, ...
//   1. last[slot] = the largest pair number among the accepted pairs of the slot (the reference's loop lets the last one stand);
//      refused pairs are counted, the accepted ones raise max_priority
//   2. the winning pair of each slot writes both leaves
//   3. level by level towards the root, every winner recomputes its ancestor from the two children, left first
//      (segment_tree.py:79-82); winners under the same ancestor write the same value
//   4. last[] goes back to -1
__global__ __launch_bounds__(kSetThreads) void per_set_kernel(double* __restrict__ sum_tree, double* __restrict__ min_tree,
                                                              int capacity, int n_slots, const int32_t* __restrict__ slots,
                                                              const float* priorities, long n, double alpha,
                                                              int32_t* __restrict__ last, float* max_priority,
                                                              int32_t* __restrict__ refused) {  // (priorities may BE max_priority)
#pragma clang fp contract(off)
  const long tid = threadIdx.x;
  int n_refused = 0;
  float top = 0.f;
  for (long i = tid; i < n; i += kSetThreads) {
    const int s = slots[i];
    const float p = priorities[i];
    if (accepted(p, s, n_slots)) {
      atomicMax(&last[s], (int32_t)i);
      top = fmaxf(top, p);
    } else {
      ++n_refused;
    }
  }
  if (n_refused) atomicAdd(refused, n_refused);
  // positive float32 values order as their bit patterns do
  if (top > 0.f) atomicMax(reinterpret_cast<int32_t*>(max_priority), __float_as_int(top));
  __syncthreads();

  auto wins = [&](long i) {
    const int s = slots[i];
    return accepted(priorities[i], s, n_slots) && __hip_atomic_load(&last[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int32_t)i;
  };
  for (long i = tid; i < n; i += kSetThreads) {
    if (!wins(i)) continue;
    const double x = (double)priorities[i];
    // pow(x, 1) is x and pow(x, 0) is 1 whatever the library's last bit
    const double leaf = alpha == 1.0 ? x : (alpha == 0.0 ? 1.0 : pow(x, alpha));
    st_node(&sum_tree[capacity + slots[i]], leaf);
    st_node(&min_tree[capacity + slots[i]], leaf);
  }
  __syncthreads();

  for (int shift = 1; (capacity >> shift) >= 1; ++shift) {
    for (long i = tid; i < n; i += kSetThreads) {
      if (!wins(i)) continue;
      const int node = (capacity + slots[i]) >> shift;
      st_node(&sum_tree[node], ld_node(&sum_tree[2 * node]) + ld_node(&sum_tree[2 * node + 1]));
      const double a = ld_node(&min_tree[2 * node]), b = ld_node(&min_tree[2 * node + 1]);
      st_node(&min_tree[node], b < a ? b : a);  // Python's min(a, b)
    }
    __syncthreads();
  }

  for (long i = tid; i < n; i += kSetThreads) {
    const int s = slots[i];
    if (s >= 0 && s < n_slots) last[s] = -1;
  }
}

// One thread per draw: the stratified mass, find_prefixsum_idx (segment_tree.py:117-124), the clamp, the importance weight
// (buffer.py:430-437).
__global__ __launch_bounds__(256) void per_sample_kernel(const double* __restrict__ sum_tree, const double* __restrict__ min_tree,
                                                         int capacity, int n_filled, int B, double beta, uint64_t seed,
                                                         uint64_t offset, int32_t* __restrict__ idx, float* __restrict__ weight) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B) return;
  const double total = sum_tree[1];
  const uint4 x = philox_draw((uint64_t)i, 0u, offset, seed);
  const double u = (double)(x.x >> 8) * (1.0 / 16777216.0);
  const double range = total / (double)B;
  const double pos = u + (double)i;
  double mass = pos * range;
  int node = 1;
  while (node < capacity) {
    const double left = sum_tree[2 * node];
    if (left > mass) {
      node = 2 * node;
    } else {
      mass = mass - left;
      node = 2 * node + 1;
    }
  }
  int k = node - capacity;
  if (k > n_filled - 1) k = n_filled - 1;
  idx[i] = k;
  const double filled = (double)n_filled;
  const double p_sample = sum_tree[capacity + k] / total;
  const double p_min = min_tree[1] / total;
  const double w = pow(p_sample * filled, -beta);
  const double w_max = pow(p_min * filled, -beta);
  weight[i] = (float)(w / w_max);
}

// dst[t, b, :] = store[idx[b], t, :]; a slot outside the store leaves its rows alone.  One workgroup per destination row, 16-byte
// pieces.
__global__ __launch_bounds__(256) void replay_gather16_kernel(const uint4* __restrict__ store, long row_vec, int Tb, int max_size,
                                                              const int32_t* __restrict__ idx, int B, uint4* __restrict__ dst) {
  const long rows = (long)Tb * B;
  for (long r = blockIdx.x; r < rows; r += gridDim.x) {
    const long t = r / B, b = r - t * B;
    const long s = idx[b];
    if (s < 0 || s >= max_size) continue;
    const uint4* in = store + (s * Tb + t) * row_vec;
    uint4* out = dst + r * row_vec;
    for (long j = threadIdx.x; j < row_vec; j += 256) out[j] = in[j];
  }
}

// narrow rows (rewards, flags widened to words, actions): one thread per 4-byte word
__global__ __launch_bounds__(256) void replay_gather4_kernel(const uint32_t* __restrict__ store, int row_words, int Tb, int max_size,
                                                             const int32_t* __restrict__ idx, int B, long total,
                                                             uint32_t* __restrict__ dst) {
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long r = e / row_words;
    const int j = (int)(e - r * row_words);
    const long t = r / B, b = r - t * B;
    const long s = idx[b];
    if (s >= 0 && s < max_size) dst[e] = store[(s * Tb + t) * row_words + j];
  }
}

// numpy's float32 pairwise sum (numpy/core/src/umath/loops_utils.h.src, pairwise_sum): what ndarray.mean() of a contiguous float32
// vector adds up, so that a statistic computed here equals the one the host path computes from the same numbers.
template <int DEPTH>
__device__ __noinline__ float pairwise_sum(const float* a, long n) {
#pragma clang fp contract(off)
  if (n < 8) {
    float res = 0.f;
    for (long i = 0; i < n; ++i) res += a[i];
    return res;
  }
  if (n <= 128 || DEPTH == 0) {
    float r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    long i;
    for (i = 8; i < n - (n % 8); i += 8) {
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    }
    float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
  }
  long n2 = n / 2;
  n2 -= n2 % 8;
  constexpr int NEXT = DEPTH > 0 ? DEPTH - 1 : 0;
  return pairwise_sum<NEXT>(a, n2) + pairwise_sum<NEXT>(a + n2, n - n2);
}

constexpr int kMeanDepth = 14;  // vectors of up to 128 * 2^14 elements split as numpy splits them

struct MeanArgs {
  const float* x[3];
  long n[3];
};

__global__ __launch_bounds__(64) void pairwise_means_kernel(MeanArgs a, double* __restrict__ out) {
  const int k = threadIdx.x;
  if (k >= 3) return;
  out[k] = (a.x[k] && a.n[k] > 0) ? (double)(pairwise_sum<kMeanDepth>(a.x[k], a.n[k]) / (float)a.n[k]) : 0.0;
}

}  // namespace

extern "C" int srl_per_set(void* stream, double* sum_tree, double* min_tree, int64_t capacity, int64_t n_slots, const int32_t* slots,
                           const float* priorities, int64_t n, double alpha, int32_t* last, float* max_priority,
                           int32_t* refused) {
  SRL_CHECK_ARG(sum_tree && min_tree && slots && priorities && last && max_priority && refused, "null tensor");
  SRL_CHECK_ARG(capacity >= 1 && capacity <= (1L << 29) && (capacity & (capacity - 1)) == 0, "capacity must be a power of two <= 2^29");
  SRL_CHECK_ARG(n_slots >= 1 && n_slots <= capacity && n >= 0 && n <= 0x7fffffffL && alpha >= 0.0, "n_slots / n / alpha out of range");
  if (n == 0) return 0;
  hipLaunchKernelGGL(per_set_kernel, dim3(1), dim3(kSetThreads), 0, (hipStream_t)stream, sum_tree, min_tree, (int)capacity,
                     (int)n_slots, slots, priorities, (long)n, alpha, last, max_priority, refused);
  SRL_LAUNCH_CHECK();
  return 0;
}

extern "C" int srl_per_sample(void* stream, const double* sum_tree, const double* min_tree, int64_t capacity, int64_t n_filled,
                              int64_t B, double beta, uint64_t seed, uint64_t offset, int32_t* idx, float* weight) {
  SRL_CHECK_ARG(sum_tree && min_tree && idx && weight, "null tensor");
  SRL_CHECK_ARG(capacity >= 1 && capacity <= (1L << 29) && (capacity & (capacity - 1)) == 0, "capacity must be a power of two <= 2^29");
  SRL_CHECK_ARG(n_filled >= 1 && n_filled <= capacity && B >= 1 && B <= (1L << 29), "n_filled / B out of range");
  hipLaunchKernelGGL(per_sample_kernel, dim3((unsigned)srl_ceil_div(B, 256)), dim3(256), 0, (hipStream_t)stream, sum_tree, min_tree,
                     (int)capacity, (int)n_filled, (int)B, beta, seed, offset, idx, weight);
  SRL_LAUNCH_CHECK();
  return 0;
}

extern "C" int srl_replay_gather(void* stream, const void* store, int64_t max_size, const int32_t* idx, int64_t B, int64_t Tb,
                                 int64_t row_bytes, void* dst) {
  SRL_CHECK_ARG(store && idx && dst && max_size >= 1 && max_size <= 0x7fffffffL, "null tensor / max_size out of range");
  SRL_CHECK_ARG(row_bytes > 0 && row_bytes % 4 == 0 && B >= 0 && B <= 0x7fffffffL && Tb >= 1 && Tb <= 0x7fffffffL,
                "row_bytes must be a positive multiple of 4");
  if (B == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const long rows = B * Tb;
  const bool vec = row_bytes % 16 == 0 && ((uintptr_t)store & 15) == 0 && ((uintptr_t)dst & 15) == 0 && row_bytes >= 1024;
  if (vec) {
    const long blocks = rows < (1L << 20) ? rows : (1L << 20);
    hipLaunchKernelGGL(replay_gather16_kernel, dim3((unsigned)blocks), dim3(256), 0, st, static_cast<const uint4*>(store),
                       (long)(row_bytes / 16), (int)Tb, (int)max_size, idx, (int)B, static_cast<uint4*>(dst));
  } else {
    SRL_CHECK_ARG(row_bytes / 4 <= 0x7fffffffL, "row too wide for the word gather");
    const long total = rows * (row_bytes / 4);
    long blocks = srl_ceil_div(total, 256);
    if (blocks > (1L << 20)) blocks = 1L << 20;
    hipLaunchKernelGGL(replay_gather4_kernel, dim3((unsigned)blocks), dim3(256), 0, st, static_cast<const uint32_t*>(store),
                       (int)(row_bytes / 4), (int)Tb, (int)max_size, idx, (int)B, total, static_cast<uint32_t*>(dst));
  }
  SRL_LAUNCH_CHECK();
  return 0;
}

extern "C" int srl_pairwise_means(void* stream, const float* a, int64_t na, const float* b, int64_t nb, const float* c, int64_t nc,
                                  double* out) {
  SRL_CHECK_ARG(out && na >= 0 && nb >= 0 && nc >= 0, "null tensor / negative length");
  const long top = 128L << kMeanDepth;
  SRL_CHECK_ARG(na <= top && nb <= top && nc <= top, "vector too long");
  MeanArgs m{{a, b, c}, {(long)na, (long)nb, (long)nc}};
  hipLaunchKernelGGL(pairwise_means_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, m, out);
  SRL_LAUNCH_CHECK();
  return 0;
}
