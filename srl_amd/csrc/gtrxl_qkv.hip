// The front of a GTrXL layer in one launch per direction (srl_gtrxl_qkv_fwd / srl_gtrxl_qkv_bwd; include/srl_hip.h): what
// GatedTransformerXLLayer.forward / AttentionXL.forward do before the attention itself (legacy/algorithm/modules/gtrxl.py:313-314,
// 196-198) together with the reset product of AutoResetRNN.forward (autoreset_rnn.py:59):
//   full = cat([keep o mem, x])   x1 = LayerNorm(full)   kv = x1 w_kv^T + b_kv (all F = M + C steps)   q = x w_q^T + b_q (raw x)
// float32 throughout, D in {64, 128, 256}.  The masked copy of the memory and the concatenation never exist: the F N rows are
// time-major, row g < M N is keep[g mod N] * mem row g, row g >= M N is x row g - M N, and the source is chosen PER ROW, so a tile
// may straddle the seam.
//
// Work split.  A workgroup is 8 wavefronts and owns a tile of RT = 8192 / D rows (32 / 64 / 128 at D = 256 / 128 / 64) at the full
// width D in LDS.  It walks a tile in two thread layouts:
//   row layout   L = D / 4 consecutive lanes own one row, 16 bytes each; thread t keeps column group 4 (t mod L) for the whole
//                launch (512 is a multiple of L) and takes the rows t / L + j 512 / L, j < 4.  Staging, the LayerNorm statistics
//                (butterflies over the L lanes), the LayerNorm backward and every row-wide store run here: whole 16-byte
//                accesses, and whatever is summed over rows (dgamma, dbeta, db_kv, db_q) stays in the thread's registers
//                from the first tile to the last.
//   MFMA layout  WC = D / 32 wavefronts across the output columns by WR = 8 / WC across blocks of 32 rows; lane l: A row / B
//                column l & 31, k half hb = l >> 5; accumulator register e: row (e & 3) + 8 (e >> 2) + 4 hb, column l & 31 (as
//                attn_xl.hip and gtrxl_gate.hip).  Every product runs on v_mfma_f32_32x32x2_f32 with the weights read as they
//                lie: in the forward a wavefront's lane reads ROW n of w_kv (key), row D + n (value) and row n of w_q for the
//                SAME output column n, so the key and value products share their A fragments (x1 in LDS) and the q product
//                takes the raw rows staged beside them; in the backward the lane reads COLUMN n (a dword per MFMA, 128
//                consecutive bytes per lane half).  The reduction index is permuted inside a chunk as in gtrxl_gate.hip (lane
//                half hb takes k = k0 + NF hb + s in MFMA s, on both operands).
// Sums are two-level: the backward's dx1 = dkv w_kv has K = 2D = 512 at D = 256, a chain of 256 MFMAs; every product accumulates
// 64 k at a time in a short chain that is added into a second accumulator (what brought gtrxl_gate.hip under its bound).
// dq w_q is a product of its own and is added to LN'(dx1) at the end, each rounded at its own size.
//
// Uneven tiles.  A tile of memory rows runs two products forward (key, value) and one backward (dx1; only dgamma, dbeta and db_kv
// take its rows: no gradient reaches the memory, so LN' is not formed); a tile that holds current rows runs three forward and two
// backward plus LN'.  The current rows are the LAST ceil(C N / RT) (+ 1) tiles.  Workgroups are persistent, at most 256, and take
// tiles w, w + groups, ...: consecutive tiles go to different workgroups, so the heavy tiles, being contiguous, are dealt out
// round-robin and no two workgroups differ by more than one of them (nor by more than one tile in all).  Whether a tile holds
// current rows is uniform across the workgroup and picks one of two instantiations of the sweep.
//
// Forward, per tile: (1) row layout: the row from its source, mean and rstd by two butterflies (centred second pass), raw row
// and normalised row to LDS, x1 and stats stored when asked for; (2) the sweep over K = D; (3) bias added, kv stored for every
// row, q for rows >= M N.
// Backward, per tile: (1) dkv (and dq of current rows) to LDS, their column sums in registers on the way; xhat of the thread's
// four rows recomputed from the source and `stats` into registers (never from x1: a zero in gamma costs nothing); (2) dx1 = dkv w_kv
// and dq w_q on the cores; (3) both written back over their operands in LDS; (4) row layout again: dgamma += dx1 xhat, dbeta +=
// dx1 for every row, and for current rows LN' from two butterflies, + dq w_q, stored 16 bytes a lane.  At the end the workgroup
// folds its threads' column sums through LDS in thread order into one slab [dgamma | dbeta | db_kv | db_q] of 5D floats in the
// workspace; a second launch folds the slabs in slab order.  No float atomics: two runs give the same bits.
//
// Constraints held.
//   LDS       forward 2 RT (D + 4) floats: 66 560 / 67 584 / 69 632 B at D = 256 / 128 / 64; backward RT (3D + 8) floats: 99 328 /
//             100 352 / 102 400 B.  One workgroup per CU in both directions.
//   registers (-Rpass-analysis=kernel-resource-usage; no scratch): see DESIGN 4.5.
//   stores    ordinary vector stores only; no atomics, no cooperative launch, no flags in memory.
// Addressing as gtrxl_gate.hip: (a pointer uniform across the wavefront)[an unsigned 32-bit lane offset] in the MFMA layout.
// Rows beyond F N compute on zeros and are never stored; columns beyond the payload of a row are never touched.
#include "layer_norm.h"
#include "srl_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
using f4 = __attribute__((ext_vector_type(4))) float;

constexpr int kGroups = 256;    // persistent workgroups at most (one per CU)
constexpr int kThreads = 512;   // 8 wavefronts
constexpr int kPasses = 4;      // rows per thread and tile in the row layout: RT / (kThreads / (D / 4))
constexpr int kRed = 2048;      // floats per column-sum block in the closing fold: (kThreads / L) rows of 4 L columns

struct QkvArgs {
  const float *mem, *x, *keep, *gamma, *beta, *w_kv, *b_kv, *w_q, *b_q, *dkv, *dq, *stats_in;
  long ldm, ldx, ldkv, ldq, ldx1, lddkv, lddq, lddx;
  long N, MN, rows;   // batch rows; memory rows M N; all rows F N
  float *kv, *q, *x1, *stats, *dx, *dgamma, *dbeta, *db_kv, *db_q, *ws;
  int groups;
};

__device__ __forceinline__ f4 ld4(const float* p) { return *reinterpret_cast<const f4*>(p); }
__device__ __forceinline__ void st4(float* p, f4 v) { *reinterpret_cast<f4*>(p) = v; }
__device__ __forceinline__ f4 zero4() { return f4{0.f, 0.f, 0.f, 0.f}; }
__device__ __forceinline__ constexpr int row_of(int e) { return (e & 3) + 8 * (e >> 2); }
__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int e = 0; e < 16; ++e) z[e] = 0.f;
  return z;
}
// the sum over the L consecutive lanes that own a row (L = 16 / 32 / 64); every lane of the wavefront takes part
template <int L>
__device__ __forceinline__ float row_sum(float v) {
#pragma unroll
  for (int o = L / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// columns c .. c + 3 of row g of cat([keep o mem, x]); zeros beyond the last row
__device__ __forceinline__ f4 full_row(const QkvArgs& a, long g, int c) {
  if (g >= a.rows) return zero4();
  if (g >= a.MN) return ld4(a.x + (g - a.MN) * a.ldx + c);
  f4 v = ld4(a.mem + g * a.ldm + c);
  if (a.keep) v *= a.keep[g % a.N];
  return v;
}
// A chunk's fragment of NF floats for this lane half: an LDS row (A) or a weight row (B: the lane's output column)
template <int NF>
__device__ __forceinline__ void row_frag(const float* p, unsigned off, float (&f)[NF]) {
#pragma unroll
  for (int t = 0; t < NF / 4; ++t) {
    const f4 v = ld4(p + off + 4 * t);
#pragma unroll
    for (int c = 0; c < 4; ++c) f[4 * t + c] = v[c];
  }
}
// ... and where the lane's output column is a COLUMN of the weight (w: the chunk's first row; off = 8 hb D + n): rows 8 hb + s
template <int D>
__device__ __forceinline__ void col_frag(const float* w, unsigned off, float (&f)[8]) {
#pragma unroll
  for (int s = 0; s < 8; ++s) f[s] = w[off + s * D];
}
template <int NF>
__device__ __forceinline__ void mfmas(f32x16& acc, const float (&af)[NF], const float (&bf)[NF]) {
#pragma unroll
  for (int s = 0; s < NF; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[s], bf[s], acc, 0, 0, 0);
}

// The forward's sweep over K = D for one 32 x 32 block of key, value and (CUR: the tile holds current rows) q: one weight
// fragment in use, one in flight (the fences keep the scheduler from requesting all of a chunk's at once).
template <int D, bool CUR>
__device__ __forceinline__ void fwd_sweep(const QkvArgs& a, const float* ns, const float* xs, unsigned ao, unsigned wo, f32x16& hk,
                                          f32x16& hv, f32x16& hq) {
  constexpr int DD = D * D;
  f32x16 ak = zero16(), av = zero16(), aq = zero16();
  float b0[16], b1[16];
  row_frag<16>(a.w_kv, wo, b0);
#pragma unroll 1
  for (int k0 = 0; k0 < D; k0 += 32) {
    const int kn = k0 + 32 < D ? k0 + 32 : k0;   // (the last chunk's key fragment is loaded twice rather than branched around)
    float an[16], ax[16];
    row_frag<16>(ns + k0, ao, an);
    if (CUR) row_frag<16>(xs + k0, ao, ax);
    row_frag<16>(a.w_kv + DD + k0, wo, b1);
    mfmas<16>(ak, an, b0);
    __builtin_amdgcn_sched_barrier(0);
    if (CUR) {
      row_frag<16>(a.w_q + k0, wo, b0);
      mfmas<16>(av, an, b1);
      __builtin_amdgcn_sched_barrier(0);
      row_frag<16>(a.w_kv + kn, wo, b1);
      mfmas<16>(aq, ax, b0);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s = 0; s < 16; ++s) b0[s] = b1[s];
    } else {
      row_frag<16>(a.w_kv + kn, wo, b0);
      mfmas<16>(av, an, b1);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (k0 & 32) {   // two-level sums: the short chains close every 64 k
      hk += ak, hv += av, ak = av = zero16();
      if (CUR) hq += aq, aq = zero16();
    }
  }
}

// grid (groups)
template <int D>
__global__ __launch_bounds__(kThreads) void gtrxl_qkv_fwd_kernel(QkvArgs a) {
  constexpr int WC = D / 32, WR = 8 / WC, RT = 32 * WR, P = D + 4, L = D / 4, RPP = kThreads / L;
  static_assert(RT == kPasses * RPP, "four rows per thread and tile");
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* ns = sm;             // [RT][P]: x1, the normalised rows
  float* xs = sm + RT * P;    // [RT][P]: the raw rows (read by the q product)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, hb = lane >> 5;
  const int n = 32 * (wave % WC) + l32, rl0 = 32 * (wave / WC);   // this lane's output column; the wavefront's rows
  const unsigned wo = n * D + 16 * hb;              // row n of a weight, this half's 16 floats of a chunk
  const unsigned ao = (rl0 + l32) * P + 16 * hb;    // the lane's LDS row as an A operand
  const unsigned lrow = rl0 + 4 * hb;               // the first of this lane's accumulator rows
  const unsigned okv = lrow * (unsigned)a.ldkv + n, oq = lrow * (unsigned)a.ldq + n;
  const int cg = 4 * (tid % L), rs = tid / L;       // row layout: this thread's columns and its first row
  const f4 gam = ld4(a.gamma + cg), bet = ld4(a.beta + cg);
  const float bk = a.b_kv[n], bv = a.b_kv[D + n], bq = a.b_q[n];
  const long tiles = (a.rows + RT - 1) / RT;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long r0 = tile * RT;
    const bool cur = r0 + RT > a.MN;   // the tile holds current rows (uniform)
#pragma unroll
    for (int j = 0; j < kPasses; ++j) {
      const int row = rs + j * RPP;
      const long g = r0 + row;
      const f4 v = full_row(a, g, cg);
      const float mean = row_sum<L>((v[0] + v[1]) + (v[2] + v[3])) / (float)D;
      const f4 d = v - mean;
      const float rstd = ln_rstd(row_sum<L>((d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3])), D);
      f4 y;
#pragma unroll
      for (int c = 0; c < 4; ++c) y[c] = ln_affine(ln_xhat(v[c], mean, rstd), gam[c], bet[c]);
      st4(ns + row * P + cg, y);
      if (cur) st4(xs + row * P + cg, v);
      if (g < a.rows) {
        if (a.x1) st4(a.x1 + g * a.ldx1 + cg, y);
        if (a.stats && cg == 0) a.stats[2 * g] = mean, a.stats[2 * g + 1] = rstd;
      }
    }
    __syncthreads();
    f32x16 hk = zero16(), hv = zero16(), hq = zero16();
    if (cur) fwd_sweep<D, true>(a, ns, xs, ao, wo, hk, hv, hq);
    else fwd_sweep<D, false>(a, ns, xs, ao, wo, hk, hv, hq);
    const int nrows = (int)(a.rows - r0 < RT ? a.rows - r0 : RT) - (int)lrow;   // valid rows from this lane's first
    const long qfirst = a.MN - r0 - (long)lrow;                                 // ... and the first of them that is a current row
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = row_of(e);   // (uniform: from the lane's first row)
      if (row < nrows) {
        float* kvr = a.kv + (r0 + row) * a.ldkv;
        kvr[okv] = hk[e] + bk;
        kvr[okv + D] = hv[e] + bv;
        if (cur && row >= qfirst) a.q[(r0 + row - a.MN) * a.ldq + (long)oq] = hq[e] + bq;
      }
    }
    __syncthreads();   // x1 and the raw rows are read: the next tile may overwrite them
  }
}

// grid (groups)
template <int D>
__global__ __launch_bounds__(kThreads) void gtrxl_qkv_bwd_kernel(QkvArgs a) {
  constexpr int WC = D / 32, WR = 8 / WC, RT = 32 * WR, P2 = 2 * D + 4, P = D + 4, L = D / 4, RPP = kThreads / L;
  constexpr int L2 = D / 2, RPP2 = kThreads / L2;   // dkv in the row layout: 2D columns, L2 lanes a row
  static_assert(RT == kPasses * RPP && RPP * D == kRed && RPP2 * 2 * D == kRed && 4 * kRed <= RT * P2, "row layout / closing fold");
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* gs = sm;              // [RT][P2]: dk | dval, then dx1 in its first D columns
  float* qs = sm + RT * P2;    // [RT][P]: dq of the current rows (zeros elsewhere), then dq w_q
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, hb = lane >> 5;
  const int n = 32 * (wave % WC) + l32, rl0 = 32 * (wave / WC);
  const unsigned wo = 8 * hb * D + n;                                        // column n of a weight, from this half's first row of a chunk
  const unsigned ag = (rl0 + l32) * P2 + 8 * hb, aq = (rl0 + l32) * P + 8 * hb;   // the lane's LDS rows as A operands
  const unsigned cgs = (rl0 + 4 * hb) * P2 + n, cqs = (rl0 + 4 * hb) * P + n;     // its accumulator rows' column n in LDS
  const int cg = 4 * (tid % L), rs = tid / L, cg2 = 4 * (tid % L2), rs2 = tid / L2;
  const f4 gam = ld4(a.gamma + cg);
  const long tiles = (a.rows + RT - 1) / RT;
  float pg[4] = {0.f, 0.f, 0.f, 0.f}, pb[4] = {0.f, 0.f, 0.f, 0.f};   // this thread's columns of dgamma, dbeta
  f4 pkv = zero4(), pq = zero4();                                     // ... of db_kv, db_q
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long r0 = tile * RT;
    const bool cur = r0 + RT > a.MN;   // the tile holds current rows (uniform)
#pragma unroll
    for (int j = 0; j < RT / RPP2; ++j) {
      const int row = rs2 + j * RPP2;
      const long g = r0 + row;
      const f4 v = g < a.rows ? ld4(a.dkv + g * a.lddkv + cg2) : zero4();
      st4(gs + row * P2 + cg2, v);
      pkv += v;
    }
    f4 xh[kPasses];
    float rstd[kPasses];
#pragma unroll
    for (int j = 0; j < kPasses; ++j) {
      const int row = rs + j * RPP;
      const long g = r0 + row;
      const bool ok = g < a.rows;
      const f4 v = full_row(a, g, cg);
      const float mean = ok ? a.stats_in[2 * g] : 0.f;
      rstd[j] = ok ? a.stats_in[2 * g + 1] : 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) xh[j][c] = ln_xhat(v[c], mean, rstd[j]);
      if (cur) {
        const f4 dqv = ok && g >= a.MN ? ld4(a.dq + (g - a.MN) * a.lddq + cg) : zero4();
        st4(qs + row * P + cg, dqv);
        pq += dqv;
      }
    }
    __syncthreads();
    f32x16 t = zero16(), u = zero16();
    {   // dx1 = dkv w_kv over K = 2D, the next chunk's weight fragment requested before this chunk's MFMAs
      f32x16 tl = zero16();
      float bf[8], bn[8], af[8];
      col_frag<D>(a.w_kv, wo, bf);
#pragma unroll 1
      for (int j0 = 0; j0 < 2 * D; j0 += 16) {
        const int jn = j0 + 16 < 2 * D ? j0 + 16 : j0;
        col_frag<D>(a.w_kv + jn * D, wo, bn);
        row_frag<8>(gs + j0, ag, af);
        mfmas<8>(tl, af, bf);
#pragma unroll
        for (int s = 0; s < 8; ++s) bf[s] = bn[s];
        if ((j0 & 48) == 48) t += tl, tl = zero16();   // two-level sums: the short chain closes every 64 k
      }
    }
    if (cur) {   // dq w_q over K = D
      f32x16 ul = zero16();
      float bf[8], bn[8], af[8];
      col_frag<D>(a.w_q, wo, bf);
#pragma unroll 1
      for (int j0 = 0; j0 < D; j0 += 16) {
        const int jn = j0 + 16 < D ? j0 + 16 : j0;
        col_frag<D>(a.w_q + jn * D, wo, bn);
        row_frag<8>(qs + j0, aq, af);
        mfmas<8>(ul, af, bf);
#pragma unroll
        for (int s = 0; s < 8; ++s) bf[s] = bn[s];
        if ((j0 & 48) == 48) u += ul, ul = zero16();
      }
    }
    __syncthreads();   // every wavefront has read dkv and dq: the products go over them
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      gs[row_of(e) * P2 + cgs] = t[e];
      if (cur) qs[row_of(e) * P + cqs] = u[e];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kPasses; ++j) {
      const int row = rs + j * RPP;
      const long g = r0 + row;
      const f4 d1 = ld4(gs + row * P2 + cg);   // (zeros in rows beyond the last: dkv was staged as zeros there)
      f4 gv;
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) gv[c] = ln_bwd_accumulate(d1[c], gam[c], xh[j][c], s1, s2, pg[c], pb[c]);
      if (cur) {   // (uniform: the butterflies run in every lane, the store only where the row is a current one)
        const float m1 = row_sum<L>(s1) / (float)D, m2 = row_sum<L>(s2) / (float)D;
        const f4 dqw = ld4(qs + row * P + cg);
        f4 o;
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c] = ln_dx(gv[c], xh[j][c], m1, m2, rstd[j]) + dqw[c];
        if (g >= a.MN && g < a.rows) st4(a.dx + (g - a.MN) * a.lddx + cg, o);
      }
    }
    __syncthreads();   // dx1 and dq w_q are read: the next tile may overwrite them
  }
  // The workgroup's slab: threads that share a column group are summed in thread order.
  st4(sm + rs * D + cg, f4{pg[0], pg[1], pg[2], pg[3]});
  st4(sm + kRed + rs * D + cg, f4{pb[0], pb[1], pb[2], pb[3]});
  st4(sm + 2 * kRed + rs2 * 2 * D + cg2, pkv);
  st4(sm + 3 * kRed + rs * D + cg, pq);
  __syncthreads();
  float* slab = a.ws + (long)blockIdx.x * 5 * D;
  for (int c = tid; c < 5 * D; c += kThreads) {
    const bool kvcol = c >= 2 * D && c < 4 * D;
    const int blk = c < D ? 0 : c < 2 * D ? 1 : c < 4 * D ? 2 : 3;
    const int col = c < 2 * D ? c % D : c < 4 * D ? c - 2 * D : c - 4 * D;
    const int width = kvcol ? 2 * D : D, cnt = kvcol ? RPP2 : RPP;
    float s = 0.f;
    for (int r = 0; r < cnt; ++r) s += sm[blk * kRed + r * width + col];
    slab[c] = s;
  }
}

// dgamma | dbeta | db_kv | db_q = the slabs summed in slab order; one thread per column
__global__ __launch_bounds__(256) void gtrxl_qkv_fold_kernel(QkvArgs a, int D) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= 5 * D) return;
  float s = 0.f;
  for (int w = 0; w < a.groups; ++w) s += a.ws[(long)w * 5 * D + c];
  if (c < D) a.dgamma[c] = s;
  else if (c < 2 * D) a.dbeta[c - D] = s;
  else if (c < 4 * D) a.db_kv[c - 2 * D] = s;
  else a.db_q[c - 4 * D] = s;
}

bool supported(int D) { return D == 64 || D == 128 || D == 256; }
int groups_of(int D, int64_t rows) {
  const int64_t tiles = srl_ceil_div(rows, (int64_t)(8192 / D));
  return (int)(tiles < kGroups ? tiles : kGroups);
}
inline bool aligned16(const void* p) { return p && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
constexpr int64_t kMaxLd = 1 << 22;   // a tile is at most 128 rows and is addressed with 32-bit offsets
inline bool rows_ok(const void* p, int64_t ld, int width) { return aligned16(p) && ld % 4 == 0 && ld >= width && ld <= kMaxLd; }
// all rows F N within 2^31 - 1: with a leading dimension of at most 2^22 every element offset stays far inside 64 bits
inline bool shape_ok(int M, int C, int64_t N, int D) {
  return supported(D) && M >= 0 && C >= 1 && N >= 1 && N <= INT32_MAX && ((int64_t)M + C) * N <= INT32_MAX;
}

template <int D>
void launch(const QkvArgs& a, bool bwd, hipStream_t st) {
  constexpr int RT = 8192 / D;
  if (bwd) {
    constexpr int lds = (int)sizeof(float) * RT * (3 * D + 8);   // <= 102 400 B
    auto kern = gtrxl_qkv_bwd_kernel<D>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipLaunchKernelGGL(kern, dim3(a.groups), dim3(kThreads), lds, st, a);
  } else {
    constexpr int lds = (int)sizeof(float) * 2 * RT * (D + 4);   // <= 69 632 B
    auto kern = gtrxl_qkv_fwd_kernel<D>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipLaunchKernelGGL(kern, dim3(a.groups), dim3(kThreads), lds, st, a);
  }
}
void launch_any(int D, const QkvArgs& a, bool bwd, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (D == 64) launch<64>(a, bwd, st);
  else if (D == 128) launch<128>(a, bwd, st);
  else launch<256>(a, bwd, st);
}

}  // namespace

extern "C" int srl_gtrxl_qkv_supported(int D) { return supported(D) ? 1 : 0; }

extern "C" int64_t srl_gtrxl_qkv_bwd_workspace(int D, int64_t rows) {
  if (!supported(D) || rows < 1) return -1;
  return (int64_t)groups_of(D, rows) * 5 * D * (int64_t)sizeof(float);
}

extern "C" int srl_gtrxl_qkv_fwd(void* stream, const float* mem, int64_t ldm, const float* x, int64_t ldx, const float* keep,
                                 const float* gamma, const float* beta, const float* w_kv, const float* b_kv, const float* w_q,
                                 const float* b_q, int M, int C, int64_t N, int D, float* kv, int64_t ldkv, float* q, int64_t ldq,
                                 float* x1, int64_t ldx1, float* stats) {
  SRL_CHECK_ARG(shape_ok(M, C, N, D), "unsupported (D in 64 | 128 | 256, M >= 0, C >= 1, N >= 1, (M + C) N < 2^31)");
  SRL_CHECK_ARG(M == 0 || rows_ok(mem, ldm, D), "mem: 16-byte aligned, leading dimension a multiple of 4 and >= D");
  SRL_CHECK_ARG(rows_ok(x, ldx, D) && rows_ok(q, ldq, D), "x, q: 16-byte aligned, leading dimension a multiple of 4 and >= D");
  SRL_CHECK_ARG(rows_ok(kv, ldkv, 2 * D), "kv: 16-byte aligned, leading dimension a multiple of 4 and >= 2D");
  SRL_CHECK_ARG(!x1 || rows_ok(x1, ldx1, D), "x1: 16-byte aligned, leading dimension a multiple of 4 and >= D");
  SRL_CHECK_ARG(aligned16(gamma) && aligned16(beta) && aligned16(w_kv) && aligned16(b_kv) && aligned16(w_q) && aligned16(b_q),
                "gamma, beta, w_kv, b_kv, w_q, b_q (16-byte aligned)");
  SRL_CHECK_ARG(!stats || aligned16(stats), "stats (16-byte aligned)");
  QkvArgs a{};
  a.mem = mem; a.ldm = ldm; a.x = x; a.ldx = ldx; a.keep = keep; a.gamma = gamma; a.beta = beta; a.w_kv = w_kv; a.b_kv = b_kv;
  a.w_q = w_q; a.b_q = b_q; a.N = N; a.MN = (int64_t)M * N; a.rows = ((int64_t)M + C) * N;
  a.kv = kv; a.ldkv = ldkv; a.q = q; a.ldq = ldq; a.x1 = x1; a.ldx1 = ldx1; a.stats = stats;
  a.groups = groups_of(D, a.rows);
  launch_any(D, a, false, stream);
  SRL_LAUNCH_CHECK();
  return 0;
}

extern "C" int srl_gtrxl_qkv_bwd(void* stream, const float* dkv, int64_t lddkv, const float* dq, int64_t lddq, const float* mem,
                                 int64_t ldm, const float* x, int64_t ldx, const float* keep, const float* stats, const float* gamma,
                                 const float* w_kv, const float* w_q, int M, int C, int64_t N, int D, float* dx, int64_t lddx,
                                 float* dgamma, float* dbeta, float* db_kv, float* db_q, void* workspace, int64_t workspace_bytes) {
  SRL_CHECK_ARG(shape_ok(M, C, N, D), "unsupported (D in 64 | 128 | 256, M >= 0, C >= 1, N >= 1, (M + C) N < 2^31)");
  SRL_CHECK_ARG(M == 0 || rows_ok(mem, ldm, D), "mem: 16-byte aligned, leading dimension a multiple of 4 and >= D");
  SRL_CHECK_ARG(rows_ok(x, ldx, D) && rows_ok(dq, lddq, D) && rows_ok(dx, lddx, D),
                "x, dq, dx: 16-byte aligned, leading dimension a multiple of 4 and >= D");
  SRL_CHECK_ARG(rows_ok(dkv, lddkv, 2 * D), "dkv: 16-byte aligned, leading dimension a multiple of 4 and >= 2D");
  SRL_CHECK_ARG(aligned16(stats) && aligned16(gamma) && aligned16(w_kv) && aligned16(w_q), "stats, gamma, w_kv, w_q (16-byte aligned)");
  SRL_CHECK_ARG(dgamma && dbeta && db_kv && db_q, "dgamma, dbeta, db_kv, db_q");
  const int64_t rows = ((int64_t)M + C) * N;
  SRL_CHECK_ARG(aligned16(workspace) && workspace_bytes >= srl_gtrxl_qkv_bwd_workspace(D, rows),
                "workspace: 16-byte aligned, srl_gtrxl_qkv_bwd_workspace bytes");
  QkvArgs a{};
  a.dkv = dkv; a.lddkv = lddkv; a.dq = dq; a.lddq = lddq; a.mem = mem; a.ldm = ldm; a.x = x; a.ldx = ldx; a.keep = keep;
  a.stats_in = stats; a.gamma = gamma; a.w_kv = w_kv; a.w_q = w_q; a.N = N; a.MN = (int64_t)M * N; a.rows = rows;
  a.dx = dx; a.lddx = lddx; a.dgamma = dgamma; a.dbeta = dbeta; a.db_kv = db_kv; a.db_q = db_q;
  a.ws = static_cast<float*>(workspace); a.groups = groups_of(D, rows);
  launch_any(D, a, true, stream);
  SRL_LAUNCH_CHECK();
  hipLaunchKernelGGL(gtrxl_qkv_fold_kernel, dim3((5 * D + 255) / 256), dim3(256), 0, (hipStream_t)stream, a, D);
  SRL_LAUNCH_CHECK();
  return 0;
}
