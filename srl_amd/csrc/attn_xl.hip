// Relative multi-head attention of Transformer-XL in one launch per direction (srl_attn_xl_fwd / srl_attn_xl_bwd;
// include/srl_hip.h): what AttentionXL.forward does between its projections (legacy/algorithm/modules/gtrxl.py:140-169, 193-231).
// Per batch row b and head h, C current steps over F = M + C keys (M of them memory), scale = dh^-0.5:
//   s[i][j] = scale ((q[i] + u) . k[j] + (q[i] + v) . r[j + C - 1 - i])   for j <= i + M, else -inf
//   out[i]  = sum_j softmax_j(s)[i][j] val[j]
// All five kinds of product (q k^T, q r^T, p val and their transposes in the backward) run on the float32 matrix cores
// (v_mfma_f32_32x32x2_f32: exact float32 multiply-adds); the [C, F] score matrix lives in accumulator registers and one LDS
// block and never reaches HBM.
//
// Work split.  The unit is (batch row, head, 32-row tile of the C queries) and ONE WAVEFRONT owns it from the first load to the
// last store: a workgroup is 64 lanes, so its barriers are free, 4-8 of them share a CU's matrix cores, and C = 1 (a rollout step)
// or C = 7 is the same code with rows predicated.  A wavefront holds the whole 32 x F score strip as ceil(F / 32) accumulator
// blocks (<= 6 x 16 registers), so the softmax is one pass in registers: the row maximum and sum are 5-step butterflies inside
// each 32-lane half (an accumulator register's row lives in one half).
//
// MFMA layout: lane l -- column (or A row) l & 31, k half hb = l >> 5; accumulator register e: row (e & 3) + 8 (e >> 2) + 4 hb.
// Where the reduction runs over the head width (scores, d p) the k index is PERMUTED: lane half hb takes d = hb dh/2 + s, so a
// lane's fragment is dh/2 consecutive floats of one row of q / k / val / r / d out, read as float4 straight from global memory
// (the same permutation on both operands leaves the product unchanged).  Where it runs over keys or queries (p val, dq, dk, dval,
// dr) the B operand is read with lane = channel: 128 consecutive bytes of a row per half.
//
// The relative shift costs address arithmetic only.  T[i][m] = (q[i] + v) . r[m] is an ordinary product; its accumulator block is
// written to LDS at [i][m - (C - 1 - i)] -- the skew -- and the block of s that the content product is about to accumulate into is
// SEEDED from LDS at [i][j]: the position term never exists as a separate pass.  Entries the skewed write does not reach
// (j > i + M) hold whatever LDS held; they are replaced (selected, not multiplied) by the mask.  The same LDS block then takes the
// probabilities, which p val reads back as A fragments (row pitch = 1 mod 32: lane = row reads are conflict-free).
// A row tile only forms the column blocks it can see (j < min(C, i0 + 32) + M) and the r blocks its skew can reach.
//
// Backward.  Grid (slabs, heads): workgroup w of a head walks batch rows w, w + slabs, ...; per batch row the row tiles from the
// LAST to the first.  Per tile and column block: s as in the forward, p = exp(s - lse) (no reductions: lse is the forward's) and
// w = p (d out val^T) go to two LDS blocks -- w over the very seeds the lane has just read, so no strip is held in registers and
// the kernel does not depend on F; D = row sums of w, then g = scale (w - p D) in place.  From the two blocks
//   dq   = g k  +  gs r          gs[i][m] = g[i][m - (C - 1 - i)]: the INVERSE skew, read from LDS as A fragments
//   dk   = g^T (q + u)           dval = p^T d out          dr = gs^T (q + v)   (A fragments read with lane = key / position)
//   du   = column sums of g k    dv   = column sums of gs r   (they are the sums over i of the two halves of dq)
// dk / dval of a batch row receive a term from each row tile: the last tile (which sees every key) stores, the first adds to what
// the same lanes stored -- same thread, same address, program order.  dr, du, dv sum over the batch: dr in the workgroup's slab of
// the workspace (L2-resident read-modify-write by the same lanes, first visit stores), du / dv in registers until the end; a
// second launch folds the slabs in slab order.  No float atomics: the result does not depend on scheduling.
//
// Constraints held.
//   LDS       forward 32 x (32 ceil(F/32) + 1) floats: 24.7 KB at F = 192, 8.3 KB at F = 64; backward twice that (49.4 KB).
//   registers a wavefront alone in its workgroup may take 512; the build prints what each kernel took
//             (-Rpass-analysis=kernel-resource-usage) and must show no scratch: forward 113 - 254 by dh and strip length,
//             backward 292 / 307 / 394 at dh 16 / 32 / 64.  The backward's product loops over blocks are NOT unrolled and its
//             inner loops only by 4: fully unrolled, the hoisted operand loads spilled (1.3 - 8.7 KB of scratch per lane).
//   stores    ordinary vector stores only; no atomics, no cooperative launch, no flags in memory.
// Rows beyond C, keys beyond F and channels beyond dh compute on zeros and are never stored; out-of-range operand loads are
// redirected to element 0 of their tensor and discarded.
#include "srl_common.h"

#include "../../include/srl_hip.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
using f4 = __attribute__((ext_vector_type(4))) float;

constexpr int kMaxC = 64, kMaxF = 192, kMaxHeads = 8;
constexpr int kBwdGroups = 1024;   // backward workgroups over all heads: slabs per head = min(N, kBwdGroups / nh)

struct XlArgs {
  const float *q, *k, *val, *r, *u, *v;
  long ldq, ldkv, ldr, N;
  int nh, C, M, F;
  float scale;
  float* out;
  long ldo;
  float* lse;   // forward: written; backward: read
  // backward
  const float* dout;
  long lddo;
  float* dq;
  long lddq;
  float *dk, *dval;
  long lddkv;
  float* dr;
  long lddr;
  float *du, *dv;
  float* ws;    // [slabs][nh][F][dh] dr | [slabs][nh][dh] du | [slabs][nh][dh] dv
  int slabs;
};

// the row (within the tile) of accumulator register e in lane half hb
__device__ __forceinline__ constexpr int row_of(int e, int hb) { return (e & 3) + 8 * (e >> 2) + 4 * hb; }
// butterflies inside a 32-lane half
__device__ __forceinline__ float half_max(float v) {
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// p[off] where ok, else 0: the load itself is unconditional and lands on element 0 when it is not wanted
__device__ __forceinline__ float at_or0(const float* p, long off, bool ok) {
  const float x = p[ok ? off : 0];
  return ok ? x : 0.f;
}
// dh/2 consecutive floats (16-byte aligned) as a fragment, zeros when the row does not exist
template <int HD>
__device__ __forceinline__ void load_half(const float* p, long off, bool ok, float (&f)[HD]) {
  const float* s = p + (ok ? off : 0);
#pragma unroll
  for (int t = 0; t < HD / 4; ++t) {
    const f4 x = *reinterpret_cast<const f4*>(s + 4 * t);
#pragma unroll
    for (int c = 0; c < 4; ++c) f[4 * t + c] = ok ? x[c] : 0.f;
  }
}
__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int e = 0; e < 16; ++e) z[e] = 0.f;
  return z;
}

// The position term of the row tile at i0: T = (q + v) r^T one block of r at a time (from mt0, the first the tile's skew
// reaches), each accumulator block written through the skew into sb.  qf: the tile's q fragments.
template <int DH>
__device__ __forceinline__ void position_term(const XlArgs& a, int h, int i0, int mt0, const float (&qf)[DH / 2], float* sb,
                                              int pitch) {
  constexpr int HD = DH / 2;
  const int lane = threadIdx.x, l32 = lane & 31, hb = lane >> 5, nmt = (a.F + 31) / 32;
  float wf[HD];
  load_half<HD>(a.v, h * DH + hb * HD, true, wf);
#pragma unroll
  for (int s = 0; s < HD; ++s) wf[s] += qf[s];
#pragma unroll 1
  for (int mt = mt0; mt < nmt; ++mt) {
    const int m = 32 * mt + l32;
    float rf[HD];
    load_half<HD>(a.r, (long)m * a.ldr + h * DH + hb * HD, m < a.F, rf);
    f32x16 t = zero16();
#pragma unroll
    for (int s = 0; s < HD; ++s) t = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[s], rf[s], t, 0, 0, 0);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int il = row_of(e, hb), j = m - (a.C - 1 - (i0 + il));   // j <= m < F
      if (i0 + il < a.C && m < a.F && j >= 0) sb[il * pitch + j] = t[e];
    }
  }
}
// Column block ct of the unscaled, unmasked scores: the content product accumulated on top of the position term read from sb.
// qu: the tile's q + u fragments.
template <int DH>
__device__ __forceinline__ f32x16 score_block(const XlArgs& a, long b, int h, int ct, const float (&qu)[DH / 2], const float* sb,
                                              int pitch) {
  constexpr int HD = DH / 2;
  const int lane = threadIdx.x, l32 = lane & 31, hb = lane >> 5, j = 32 * ct + l32;
  float kf[HD];
  load_half<HD>(a.k, ((long)j * a.N + b) * a.ldkv + h * DH + hb * HD, j < a.F, kf);
  f32x16 c;
#pragma unroll
  for (int e = 0; e < 16; ++e) c[e] = sb[row_of(e, hb) * pitch + j];
#pragma unroll
  for (int s = 0; s < HD; ++s) c = __builtin_amdgcn_mfma_f32_32x32x2f32(qu[s], kf[s], c, 0, 0, 0);
  return c;
}
// the tile's q fragments, and q + u in their place once the position term is written
template <int DH>
__device__ __forceinline__ void add_u(const XlArgs& a, int h, float (&qf)[DH / 2]) {
  constexpr int HD = DH / 2;
  float uf[HD];
  load_half<HD>(a.u, h * DH + ((int)threadIdx.x >> 5) * HD, true, uf);
#pragma unroll
  for (int s = 0; s < HD; ++s) qf[s] += uf[s];
}

// grid (N, nh, row tiles)
template <int DH, int NCT>
__global__ __launch_bounds__(64) void attn_xl_fwd_kernel(XlArgs a) {
  constexpr int NDT = (DH + 31) / 32;
  extern __shared__ __attribute__((aligned(16))) float sm[];   // [32][pitch]: the skewed position term, then the probabilities
  const int lane = threadIdx.x, l32 = lane & 31, hb = lane >> 5;
  const long b = blockIdx.x;
  const int h = blockIdx.y, i0 = 32 * blockIdx.z;
  const int pitch = 32 * ((a.F + 31) / 32) + 1;
  const int rows_end = a.C < i0 + 32 ? a.C : i0 + 32;
  const int nct = (rows_end + a.M + 31) / 32, mt0 = (a.C - rows_end) / 32;
  f32x16 acc[NCT];
  {
    float qf[DH / 2];
    load_half<DH / 2>(a.q, ((long)(i0 + l32) * a.N + b) * a.ldq + h * DH + hb * (DH / 2), i0 + l32 < a.C, qf);
    position_term<DH>(a, h, i0, mt0, qf, sm, pitch);
    __syncthreads();
    add_u<DH>(a, h, qf);
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
      if (ct < nct) acc[ct] = score_block<DH>(a, b, h, ct, qf, sm, pitch);
  }
  float mx[16], sum[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) mx[e] = -INFINITY, sum[e] = 0.f;
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    if (ct < nct) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = i0 + row_of(e, hb), j = 32 * ct + l32;
        acc[ct][e] = (i < a.C && j <= i + a.M) ? acc[ct][e] * a.scale : -INFINITY;
        mx[e] = fmaxf(mx[e], acc[ct][e]);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    mx[e] = half_max(mx[e]);
    if (i0 + row_of(e, hb) >= a.C) mx[e] = 0.f;   // a row that does not exist: p = exp(-inf - 0) = 0, not exp(-inf + inf)
  }
  __syncthreads();   // (every seed is read: the block now takes the probabilities)
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    if (ct < nct) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float p = expf(acc[ct][e] - mx[e]);
        sum[e] += p;
        sm[row_of(e, hb) * pitch + 32 * ct + l32] = p;
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) sum[e] = half_sum(sum[e]);
  __syncthreads();
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) {
    const int d = 32 * dt + l32;
    const bool dok = d < DH;
    f32x16 o = zero16();
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      if (ct < nct) {
#pragma unroll
        for (int s = 0; s < 16; ++s) {
          const int j = 32 * ct + 16 * hb + s;
          const float vb = at_or0(a.val, ((long)j * a.N + b) * a.ldkv + h * DH + d, dok && j < a.F);
          o = __builtin_amdgcn_mfma_f32_32x32x2f32(sm[l32 * pitch + j], vb, o, 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int i = i0 + row_of(e, hb);
      if (i < a.C && dok) a.out[((long)i * a.N + b) * a.ldo + h * DH + d] = o[e] / sum[e];
    }
  }
  if (l32 == 0) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int i = i0 + row_of(e, hb);
      if (i < a.C) a.lse[(b * a.nh + h) * a.C + i] = mx[e] + logf(sum[e]);
    }
  }
}

// grid (slabs, nh)
template <int DH>
__global__ __launch_bounds__(64) void attn_xl_bwd_kernel(XlArgs a) {
  constexpr int HD = DH / 2, NDT = (DH + 31) / 32;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int lane = threadIdx.x, l32 = lane & 31, hb = lane >> 5;
  const int slab = blockIdx.x, h = blockIdx.y;
  const int nctF = (a.F + 31) / 32, pitch = 32 * nctF + 1, nit = (a.C + 31) / 32;
  float* gb = sm;                // [32][pitch]: the skewed position term, then g = d s
  float* pb = sm + 32 * pitch;   // [32][pitch]: p
  float* dr_slab = a.ws + (long)(slab * a.nh + h) * a.F * DH;
  float ub[NDT], vb[NDT], du_acc[NDT], dv_acc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) {
    ub[dt] = at_or0(a.u, h * DH + 32 * dt + l32, 32 * dt + l32 < DH);
    vb[dt] = at_or0(a.v, h * DH + 32 * dt + l32, 32 * dt + l32 < DH);
    du_acc[dt] = dv_acc[dt] = 0.f;
  }
  bool first = true;   // the slab has not been written yet
  for (long b = slab; b < a.N; b += a.slabs) {
    for (int it = nit - 1; it >= 0; --it) {   // the last tile sees every key and every position: it stores, the others add
      const int i0 = 32 * it;
      const int rows_end = a.C < i0 + 32 ? a.C : i0 + 32;
      const int nct = (rows_end + a.M + 31) / 32, mt0 = (a.C - rows_end) / 32, wcols = 32 * nct;
      float D[16];
      {   // per column block: p = exp(s - lse) into pb, w = p (d out val^T) over the block's own seeds in gb
        float qf[HD], dof[HD], lr[16];
        load_half<HD>(a.q, ((long)(i0 + l32) * a.N + b) * a.ldq + h * DH + hb * HD, i0 + l32 < a.C, qf);
        load_half<HD>(a.dout, ((long)(i0 + l32) * a.N + b) * a.lddo + h * DH + hb * HD, i0 + l32 < a.C, dof);
        position_term<DH>(a, h, i0, mt0, qf, gb, pitch);
        __syncthreads();
        add_u<DH>(a, h, qf);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int i = i0 + row_of(e, hb);
          lr[e] = at_or0(a.lse, (b * a.nh + h) * a.C + i, i < a.C);
          D[e] = 0.f;
        }
#pragma unroll 1
        for (int ct = 0; ct < nct; ++ct) {
          const f32x16 c = score_block<DH>(a, b, h, ct, qf, gb, pitch);
          const int j = 32 * ct + l32;
          float vf[HD];
          load_half<HD>(a.val, ((long)j * a.N + b) * a.ldkv + h * DH + hb * HD, j < a.F, vf);
          f32x16 t = zero16();
#pragma unroll
          for (int s = 0; s < HD; ++s) t = __builtin_amdgcn_mfma_f32_32x32x2f32(dof[s], vf[s], t, 0, 0, 0);
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int i = i0 + row_of(e, hb), o = row_of(e, hb) * pitch + j;
            const float p = (i < a.C && j <= i + a.M) ? expf(c[e] * a.scale - lr[e]) : 0.f;
            const float w = p * t[e];
            pb[o] = p;
            gb[o] = w;   // (over the seed this lane has just read)
            D[e] += w;
          }
        }
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) D[e] = half_sum(D[e]);
#pragma unroll 1
      for (int ct = 0; ct < nct; ++ct) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int o = row_of(e, hb) * pitch + 32 * ct + l32;
          gb[o] = a.scale * (gb[o] - pb[o] * D[e]);   // g = d s; 0 under the mask and in rows beyond C
        }
      }
      __syncthreads();
      // dq = g k + gs r; du, dv = the column sums of the two terms
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        const int d = 32 * dt + l32;
        const bool dok = d < DH;
        f32x16 ak = zero16(), ar = zero16();
#pragma unroll 1
        for (int ct = 0; ct < nct; ++ct) {
          {
#pragma unroll 4
            for (int s = 0; s < 16; ++s) {
              const int j = 32 * ct + 16 * hb + s;
              const float kb = at_or0(a.k, ((long)j * a.N + b) * a.ldkv + h * DH + d, dok && j < a.F);
              ak = __builtin_amdgcn_mfma_f32_32x32x2f32(gb[l32 * pitch + j], kb, ak, 0, 0, 0);
            }
          }
        }
#pragma unroll 1
        for (int mt = mt0; mt < nctF; ++mt) {
          {
#pragma unroll 4
            for (int s = 0; s < 16; ++s) {
              const int m = 32 * mt + 16 * hb + s, j = m - (a.C - 1 - (i0 + l32));
              const float ga = at_or0(gb, l32 * pitch + j, j >= 0 && j < wcols && m < a.F);
              const float rb = at_or0(a.r, (long)m * a.ldr + h * DH + d, dok && m < a.F);
              ar = __builtin_amdgcn_mfma_f32_32x32x2f32(ga, rb, ar, 0, 0, 0);
            }
          }
        }
        float sk = 0.f, sr = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int i = i0 + row_of(e, hb);
          if (i < a.C && dok) a.dq[((long)i * a.N + b) * a.lddq + h * DH + d] = ak[e] + ar[e];
          sk += ak[e];   // (rows beyond C are zeros)
          sr += ar[e];
        }
        du_acc[dt] += sk;
        dv_acc[dt] += sr;
      }
      // dk = g^T (q + u), dval = p^T d out, per block of keys
#pragma unroll 1
      for (int ct = 0; ct < nct; ++ct) {
        {
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt) {
            const int d = 32 * dt + l32;
            const bool dok = d < DH;
            f32x16 kk = zero16(), vv = zero16();
#pragma unroll 4
            for (int s = 0; s < 16; ++s) {
              const int il = 16 * hb + s, i = i0 + il;
              const bool ok = dok && i < a.C;
              const float qb = at_or0(a.q, ((long)i * a.N + b) * a.ldq + h * DH + d, ok);
              const float db = at_or0(a.dout, ((long)i * a.N + b) * a.lddo + h * DH + d, ok);
              kk = __builtin_amdgcn_mfma_f32_32x32x2f32(gb[il * pitch + 32 * ct + l32], ok ? qb + ub[dt] : 0.f, kk, 0, 0, 0);
              vv = __builtin_amdgcn_mfma_f32_32x32x2f32(pb[il * pitch + 32 * ct + l32], db, vv, 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
              const int j = 32 * ct + row_of(e, hb);
              if (j < a.F && dok) {
                const long o = ((long)j * a.N + b) * a.lddkv + h * DH + d;
                if (it != nit - 1) {
                  kk[e] += a.dk[o];
                  vv[e] += a.dval[o];
                }
                a.dk[o] = kk[e];
                a.dval[o] = vv[e];
              }
            }
          }
        }
      }
      // dr = gs^T (q + v), per block of positions, into the slab
#pragma unroll 1
      for (int mt = mt0; mt < nctF; ++mt) {
        {
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt) {
            const int d = 32 * dt + l32;
            const bool dok = d < DH;
            f32x16 rr = zero16();
#pragma unroll 4
            for (int s = 0; s < 16; ++s) {
              const int il = 16 * hb + s, i = i0 + il, m = 32 * mt + l32, j = m - (a.C - 1 - i);
              const float ga = at_or0(gb, il * pitch + j, i < a.C && j >= 0 && j < wcols && m < a.F);
              const bool ok = dok && i < a.C;
              const float qb = at_or0(a.q, ((long)i * a.N + b) * a.ldq + h * DH + d, ok);
              rr = __builtin_amdgcn_mfma_f32_32x32x2f32(ga, ok ? qb + vb[dt] : 0.f, rr, 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
              const int m = 32 * mt + row_of(e, hb);
              if (m < a.F && dok) {
                if (!first) rr[e] += dr_slab[m * DH + d];
                dr_slab[m * DH + d] = rr[e];
              }
            }
          }
        }
      }
      first = false;
      __syncthreads();   // gb and pb are read: the next tile may overwrite them
    }
  }
  float* du_slab = a.ws + (long)a.slabs * a.nh * a.F * DH + (long)(slab * a.nh + h) * DH;
  float* dv_slab = du_slab + (long)a.slabs * a.nh * DH;
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) {
    const int d = 32 * dt + l32;
    const float su = du_acc[dt] + __shfl_xor(du_acc[dt], 32, 64), sv = dv_acc[dt] + __shfl_xor(dv_acc[dt], 32, 64);
    if (hb == 0 && d < DH) {
      du_slab[d] = su;
      dv_slab[d] = sv;
    }
  }
}

// dr, du, dv = the slabs summed in slab order; one thread per element
__global__ __launch_bounds__(256) void attn_xl_fold_kernel(XlArgs a, int dh) {
  const long n_dr = (long)a.nh * a.F * dh, n_b = (long)a.nh * dh;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_dr + 2 * n_b) return;
  const float* src;
  float* dst;
  long stride;
  if (idx < n_dr) {
    const int d = (int)(idx % dh), m = (int)(idx / dh % a.F), h = (int)(idx / ((long)dh * a.F));
    src = a.ws + ((long)h * a.F + m) * dh + d;
    stride = n_dr;
    dst = a.dr + (long)m * a.lddr + h * dh + d;
  } else {
    const long o = idx - n_dr;
    src = a.ws + (long)a.slabs * n_dr + (o >= n_b ? (long)a.slabs * n_b : 0) + o % n_b;
    stride = n_b;
    dst = (o >= n_b ? a.dv : a.du) + o % n_b;
  }
  float s = 0.f;
  for (int w = 0; w < a.slabs; ++w) s += src[w * stride];
  *dst = s;
}

bool supported(int nh, int dh, int C, int M) {
  return (dh == 16 || dh == 32 || dh == 64) && nh >= 1 && nh <= kMaxHeads && C >= 1 && C <= kMaxC && M >= 0 && M <= kMaxF - C;
}
int slabs_for(int nh, int64_t N) { return (int)(N < kBwdGroups / nh ? N : kBwdGroups / nh); }
inline bool aligned16(const void* p) { return p && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool rows_ok(const void* p, int64_t ld, int width) { return aligned16(p) && ld % 4 == 0 && ld >= width; }

template <int DH, int NCT>
void launch(const XlArgs& a, bool bwd, hipStream_t st) {
  const int pitch = 32 * ((a.F + 31) / 32) + 1;
  const int lds = (int)sizeof(float) * 32 * pitch * (bwd ? 2 : 1);   // <= 49 408 B
  if (bwd) hipLaunchKernelGGL((attn_xl_bwd_kernel<DH>), dim3(a.slabs, a.nh), dim3(64), lds, st, a);
  else hipLaunchKernelGGL((attn_xl_fwd_kernel<DH, NCT>), dim3((unsigned)a.N, a.nh, (a.C + 31) / 32), dim3(64), lds, st, a);
}
template <int DH>
void launch_f(const XlArgs& a, bool bwd, hipStream_t st) {
  const int nct = (a.F + 31) / 32;   // the accumulator strip a wavefront holds: 2, 4 or 6 blocks
  if (nct <= 2) launch<DH, 2>(a, bwd, st);
  else if (nct <= 4) launch<DH, 4>(a, bwd, st);
  else launch<DH, 6>(a, bwd, st);
}
void launch_any(int dh, const XlArgs& a, bool bwd, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (dh == 16) launch_f<16>(a, bwd, st);
  else if (dh == 32) launch_f<32>(a, bwd, st);
  else launch_f<64>(a, bwd, st);
}

}  // namespace

extern "C" int srl_attn_xl_supported(int nh, int dh, int C, int M) { return supported(nh, dh, C, M) ? 1 : 0; }

extern "C" int64_t srl_attn_xl_bwd_workspace(int nh, int dh, int C, int M, int64_t N) {
  if (!supported(nh, dh, C, M) || N < 1) return -1;
  return (int64_t)slabs_for(nh, N) * nh * (C + M + 2) * dh * (int64_t)sizeof(float);
}

extern "C" int srl_attn_xl_fwd(void* stream, const float* q, int64_t ldq, const float* k, const float* val, int64_t ldkv,
                               const float* r, int64_t ldr, const float* u, const float* v, int64_t N, int nh, int dh, int C, int M,
                               float* out, int64_t ldo, float* lse) {
  SRL_CHECK_ARG(supported(nh, dh, C, M), "unsupported (dh in 16 | 32 | 64, 1 <= nh <= 8, 1 <= C <= 64, M >= 0, M + C <= 192)");
  SRL_CHECK_ARG(N >= 0 && N <= 0x7fffffff, "N");
  const int W = nh * dh;
  SRL_CHECK_ARG(rows_ok(q, ldq, W) && rows_ok(k, ldkv, W) && rows_ok(val, ldkv, W) && rows_ok(r, ldr, W) && rows_ok(out, ldo, W),
                "q, k, val, r, out: 16-byte aligned, leading dimension a multiple of 4 and >= nh dh");
  SRL_CHECK_ARG(aligned16(u) && aligned16(v) && lse, "u, v (16-byte aligned), lse");
  if (N == 0) return 0;
  XlArgs a{};
  a.q = q; a.k = k; a.val = val; a.r = r; a.u = u; a.v = v; a.ldq = ldq; a.ldkv = ldkv; a.ldr = ldr; a.N = N;
  a.nh = nh; a.C = C; a.M = M; a.F = C + M; a.scale = (float)(1.0 / sqrt((double)dh));
  a.out = out; a.ldo = ldo; a.lse = lse;
  launch_any(dh, a, false, stream);
  SRL_LAUNCH_CHECK();
  return 0;
}

extern "C" int srl_attn_xl_bwd(void* stream, const float* d_out, int64_t lddo, const float* q, int64_t ldq, const float* k,
                               const float* val, int64_t ldkv, const float* r, int64_t ldr, const float* u, const float* v,
                               const float* lse, int64_t N, int nh, int dh, int C, int M, float* dq, int64_t lddq, float* dk,
                               float* dval, int64_t lddkv, float* dr, int64_t lddr, float* du, float* dv, void* workspace,
                               int64_t workspace_bytes) {
  SRL_CHECK_ARG(supported(nh, dh, C, M), "unsupported (see srl_attn_xl_fwd)");
  SRL_CHECK_ARG(N >= 1 && N <= 0x7fffffff, "N");
  const int W = nh * dh;
  SRL_CHECK_ARG(rows_ok(d_out, lddo, W) && rows_ok(q, ldq, W) && rows_ok(k, ldkv, W) && rows_ok(val, ldkv, W) && rows_ok(r, ldr, W),
                "d_out, q, k, val, r: 16-byte aligned, leading dimension a multiple of 4 and >= nh dh");
  SRL_CHECK_ARG(rows_ok(dq, lddq, W) && rows_ok(dk, lddkv, W) && rows_ok(dval, lddkv, W) && rows_ok(dr, lddr, W),
                "dq, dk, dval, dr: 16-byte aligned, leading dimension a multiple of 4 and >= nh dh");
  SRL_CHECK_ARG(aligned16(u) && aligned16(v) && lse && du && dv, "u, v (16-byte aligned), lse, du, dv");
  SRL_CHECK_ARG(aligned16(workspace) && workspace_bytes >= srl_attn_xl_bwd_workspace(nh, dh, C, M, N),
                "workspace: 16-byte aligned, srl_attn_xl_bwd_workspace bytes");
  XlArgs a{};
  a.q = q; a.k = k; a.val = val; a.r = r; a.u = u; a.v = v; a.ldq = ldq; a.ldkv = ldkv; a.ldr = ldr; a.N = N;
  a.nh = nh; a.C = C; a.M = M; a.F = C + M; a.scale = (float)(1.0 / sqrt((double)dh));
  a.lse = const_cast<float*>(lse); a.dout = d_out; a.lddo = lddo; a.dq = dq; a.lddq = lddq; a.dk = dk; a.dval = dval; a.lddkv = lddkv;
  a.dr = dr; a.lddr = lddr; a.du = du; a.dv = dv; a.ws = static_cast<float*>(workspace); a.slabs = slabs_for(nh, N);
  launch_any(dh, a, true, stream);
  SRL_LAUNCH_CHECK();
  const long n = (long)nh * (a.F + 2) * dh;
  hipLaunchKernelGGL(attn_xl_fold_kernel, dim3((unsigned)srl_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, a, dh);
  SRL_LAUNCH_CHECK();
  return 0;
}
