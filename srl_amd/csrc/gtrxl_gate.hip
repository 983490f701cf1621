// GTrXL's GRU-style gating unit in one launch per direction (srl_gtrxl_gate_fwd / srl_gtrxl_gate_bwd; include/srl_hip.h): what
// GRUGatingUnit.forward does (legacy/algorithm/modules/gtrxl.py:44-84; gate1 and gate2 of every layer, :317 and :320), per row of
// [rows, D] with w_y = Wr | Wz | Wg and w_x = Ur | Uz | Ug stacked along the output dimension ([3D, D] each, as torch Linear
// weights lie):
//   r = s(y Wr^T + x Ur^T)   z = s(y Wz^T + x Uz^T - bg)   h = tanh(y Wg^T + (r o x) Ug^T)   g = (1 - z) o x + z o h
// This is not the GRU cell of rnn_step.hip / rnn_seq.hip: there r multiplies a FINISHED product, here r o x is the operand of the
// sixth product, which therefore cannot start before r is complete across the whole row.  That dependence is resolved inside a
// workgroup: it owns a tile of rows at the FULL width D.  All six products (and the backward's three) run on the float32 matrix
// cores (v_mfma_f32_32x32x2_f32: exact float32 multiply-adds), D in {64, 128, 256}.
//
// Work split.  A workgroup is 8 wavefronts laid out WR x WC over its tile: WC = D / 32 of them across the columns, each owning
// the SAME 32 columns n of all three gates, and WR = 8 / WC across row blocks of 32.  Tile height: 32 WR = 8192 / D rows (32 / 64 /
// 128 at D = 256 / 128 / 64).  Workgroups are persistent: at most 256, workgroup w takes tiles w, w + groups, ...  (The forward
// kernel is written for RB row blocks per wavefront; RB = 2 -- every weight fragment feeding two MFMAs, half the L2 traffic -- fits
// LDS but leaves no registers for the second-level accumulators below, and without them the forward misses its error bound at
// D = 256: only RB = 1 is instantiated.)
// MFMA layout (as attn_xl.hip): lane l -- A row / B column l & 31, k half hb = l >> 5; accumulator register e: row
// (e & 3) + 8 (e >> 2) + 4 hb, column l & 31.  The reduction index is PERMUTED inside a chunk: lane half hb takes k = k0 + NF hb + s in
// MFMA s, on both operands.  Forward (NF = 16, chunks of 32): the A fragment is four 16-byte LDS reads of one row of the tile and
// the B fragment -- the weight's row is the output column -- four 16-byte reads of one row of the weight as it lies in global
// memory / L2: the two lane halves consume one whole 128-byte line per row and chunk, so a line is fetched once.  The five
// products of a chunk run one after another, each with the next product's weight fragment in flight (two fragment buffers;
// scheduler fences keep the compiler from requesting all five at once).  Backward (NF = 8, chunks of 16): the output column is the
// weight's COLUMN: lane = column reads a dword per MFMA, 128 consecutive bytes per lane half; the next chunk's fragments are
// requested before the current chunk's MFMAs.
// Sums are two-level where the bound needs it: a single chain of 256 MFMAs (K = 2D at D = 256) rounds ~ sqrt(256) times at the
// size of the running sum, so r_pre, z_pre, h_pre and t accumulate 64 k at a time in short chains that are added into a second
// accumulator.  dx's direct term dg (1 - z) + t r is added to its product at the END: seeded into the accumulator, every MFMA
// rounded at ITS size (measured: error / bound 1.6 seeded, 0.6 added last).
// Addressing: (a pointer uniform across the wavefront)[an unsigned 32-bit lane offset] everywhere, one offset register per tensor;
// with a 64-bit address per element touched the kernels spilled (144 - 1 100 B of scratch per lane).
//
// Forward, per tile: (1) x and y to LDS, rows beyond `rows` as zeros; (2) one sweep over K = D accumulates r_pre, z_pre and the
// y Wg^T half of h_pre; (3) barrier, r = s(r_pre), r o x written over y in LDS (y is finished), r stored; barrier; (4) (r o x) Ug^T
// onto h_pre; (5) z, h, g in registers (x from LDS), stored.
// Backward, per tile: (1) a_g = dg z (1 - h^2) and a_z = dg (h - x) z (1 - z) from registers to LDS (and over z, h in `gates`);
// (2) t = a_g Ug on the cores; (3) a_r = t x r (1 - r) to LDS (and over r), rx = r o x stored, dg (1 - z) + t r kept for the end;
// (4) dy = A w_y (K = 3D) and A[:, :2D] w_x[:2D] share their A fragments; (5) stored.  Every (row, column) of gates / A is read and
// written by one lane only, so the overwrite in place needs no ordering beyond program order.
// d_bg = - column sums of a_z: in a register per lane over the workgroup's tiles, then one slab [D] per workgroup in the workspace,
// folded in slab order by a second launch.  No float atomics: two runs give the same bits.
//
// Constraints held.
//   LDS       forward 2 RT (D + 4) floats: 66 560 / 67 584 / 69 632 B at D = 256 / 128 / 64; backward RT (3D + 4) floats + 1 KB:
//             99 840 / 100 352 / 101 376 B.  Of a CU's 160 KB that is one backward workgroup; two forward ones would fit LDS, but
//             at 217 - 223 registers a lane a SIMD holds two wavefronts: one workgroup (8 wavefronts) per CU in both directions.
//   registers (-Rpass-analysis=kernel-resource-usage; no scratch) forward 217 / 217 / 223, backward 256 / 231 / 233 at D = 256 / 128 / 64.
//   stores    ordinary vector stores only; no atomics, no cooperative launch, no flags in memory.
// The row arithmetic beside the MFMAs stays on unpacked float32 ops (as rnn_step.hip's backward: per kernel).
// Rows beyond `rows` compute on zeros and are never stored (guarded loads go through the tile's first row, which exists); columns
// beyond D of a row are never touched.
#include "rnn_cell.h"
#include "srl_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
using f4 = __attribute__((ext_vector_type(4))) float;
using rnn_cell::LibmGates;

#ifdef __HIP_DEVICE_COMPILE__
#define SRL_UNPACKED_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define SRL_UNPACKED_F32
#endif

constexpr int kGroups = 256;    // persistent workgroups at most (one per CU)
constexpr int kThreads = 512;   // 8 wavefronts

struct GateArgs {
  const float *x, *y, *w_y, *w_x, *bg, *dg;
  long ldx, ldy, lddg, rows;
  float *g, *gates, *dx, *dy, *rx, *d_bg, *ws;
  long ldg, ldgates, lddx, lddy, ldrx;
  int groups;
};

__device__ __forceinline__ f4 ld4(const float* p) { return *reinterpret_cast<const f4*>(p); }
__device__ __forceinline__ void st4(float* p, f4 v) { *reinterpret_cast<f4*>(p) = v; }
// Addressing: every global access below is (a pointer that is uniform across the wavefront)[an unsigned 32-bit lane offset], so
// that a lane keeps ONE offset register per tensor instead of a 64-bit address per element it touches.
// The rows of accumulator register e: row_of(e) + 4 hb within a 32-row block; the 4 hb part belongs to the lane offset.
__device__ __forceinline__ constexpr int row_of(int e) { return (e & 3) + 8 * (e >> 2); }
__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int e = 0; e < 16; ++e) z[e] = 0.f;
  return z;
}
// p[off] where ok, else 0: the load itself is unconditional and lands on element 0 when it is not wanted
__device__ __forceinline__ float at_or0(const float* p, unsigned off, bool ok) {
  const float v = p[ok ? off : 0u];
  return ok ? v : 0.f;
}
// A chunk's fragment of NF floats for this lane half, A (an LDS row) or B (a weight row: the lane's output column); off carries the
// lane's row and its half's + NF hb.  In the forward (NF = 16) both halves together consume one whole 128-byte line per chunk.
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
template <int RB, int NF>
__device__ __forceinline__ void mfmas(f32x16 (&acc)[RB], const float (&af)[RB][NF], const float (&bf)[NF]) {
#pragma unroll
  for (int s = 0; s < NF; ++s)
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[rb][s], bf[s], acc[rb], 0, 0, 0);
}

// grid (groups); RB row blocks of 32 per wavefront
template <int D, int RB>
__global__ __launch_bounds__(kThreads) SRL_UNPACKED_F32 void gtrxl_gate_fwd_kernel(GateArgs a) {
  constexpr int WC = D / 32, WR = 8 / WC, RT = 32 * WR * RB, P = D + 4, DD = D * D;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* xs = sm;             // [RT][P]: x
  float* ys = sm + RT * P;    // [RT][P]: y, then r o x
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, hb = lane >> 5;
  const int n = 32 * (wave % WC) + l32, rl0 = 32 * RB * (wave / WC);   // this lane's column of every gate; the wavefront's rows
  const unsigned wo = n * D + 16 * hb;                 // row n of Wr / Ur (Wz, Wg, Uz, Ug at + DD, + 2 DD), this half's 16 floats
  const unsigned ao = (rl0 + l32) * P + 16 * hb;       // the lane's LDS row as an A operand
  const unsigned co = (rl0 + 4 * hb) * P + n;          // ... and its accumulator rows' column n in LDS
  const unsigned og = (rl0 + 4 * hb) * (unsigned)a.ldg + n, ogt = (rl0 + 4 * hb) * (unsigned)a.ldgates + n;
  const float bgn = a.bg[n];
  const long tiles = (a.rows + RT - 1) / RT;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long r0 = tile * RT;
    const int nrows = (int)(a.rows - r0 < RT ? a.rows - r0 : RT) - rl0 - 4 * hb;   // valid rows from this lane's first
    for (int i = tid; i < RT * (D / 4); i += kThreads) {
      const int row = i / (D / 4), c = 4 * (i % (D / 4));
      const long gr = r0 + row;
      f4 vx = f4{0.f, 0.f, 0.f, 0.f}, vy = vx;
      if (gr < a.rows) {
        vx = ld4(a.x + gr * a.ldx + c);
        vy = ld4(a.y + gr * a.ldy + c);
      }
      st4(xs + row * P + c, vx);
      st4(ys + row * P + c, vy);
    }
    __syncthreads();
    // Two-level sums: a chain of 256 MFMAs (K = 2D at D = 256) rounds ~ sqrt(256) times; every 64 k the short chains ar / az / ah are
    // added into hr / hz / hh and start again from zero.
    f32x16 ar[RB], az[RB], ah[RB], hr[RB], hz[RB], hh[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) ar[rb] = az[rb] = ah[rb] = hr[rb] = hz[rb] = hh[rb] = zero16();
    {   // r_pre, z_pre and the y half of h_pre: Wr, Wz, Wg on y, then Ur, Uz on x, one weight fragment ahead
      float b0[16], b1[16];
      row_frag<16>(a.w_y, wo, b0);
#pragma unroll 1
      for (int k0 = 0; k0 < D; k0 += 32) {
        const int kn = k0 + 32 < D ? k0 + 32 : k0;   // (the last chunk's Wr is loaded twice rather than branching around the loads)
        float ay[RB][16], ax[RB][16];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
          row_frag<16>(ys + 32 * rb * P + k0, ao, ay[rb]);
          row_frag<16>(xs + 32 * rb * P + k0, ao, ax[rb]);
        }
        // (the fences keep the scheduler from requesting all five fragments at once: one in flight, one in use)
        row_frag<16>(a.w_y + DD + k0, wo, b1);
        mfmas<RB, 16>(ar, ay, b0);
        __builtin_amdgcn_sched_barrier(0);
        row_frag<16>(a.w_y + 2 * DD + k0, wo, b0);
        mfmas<RB, 16>(az, ay, b1);
        __builtin_amdgcn_sched_barrier(0);
        row_frag<16>(a.w_x + k0, wo, b1);
        mfmas<RB, 16>(ah, ay, b0);
        __builtin_amdgcn_sched_barrier(0);
        row_frag<16>(a.w_x + DD + k0, wo, b0);
        mfmas<RB, 16>(ar, ax, b1);
        __builtin_amdgcn_sched_barrier(0);
        row_frag<16>(a.w_y + kn, wo, b1);
        mfmas<RB, 16>(az, ax, b0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 16; ++s) b0[s] = b1[s];
        if (k0 & 32) {
#pragma unroll
          for (int rb = 0; rb < RB; ++rb) {
            hr[rb] += ar[rb], hz[rb] += az[rb], hh[rb] += ah[rb];
            ar[rb] = az[rb] = ah[rb] = zero16();
          }
        }
      }
    }
    __syncthreads();   // (every wavefront has read y: the block now takes r o x)
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = 32 * rb + row_of(e);   // (uniform: from the lane's first row)
        const float r = LibmGates::sigm(hr[rb][e]);
        ys[row * P + co] = r * xs[row * P + co];
        if (a.gates && row < nrows) (a.gates + (r0 + row) * a.ldgates)[ogt] = r;
      }
    }
    __syncthreads();
    {   // (r o x) Ug^T onto h_pre
      float uf[16], un[16];
      row_frag<16>(a.w_x + 2 * DD, wo, uf);
#pragma unroll 1
      for (int k0 = 0; k0 < D; k0 += 32) {
        const int kn = k0 + 32 < D ? k0 + 32 : k0;
        row_frag<16>(a.w_x + 2 * DD + kn, wo, un);
        float af[RB][16];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) row_frag<16>(ys + 32 * rb * P + k0, ao, af[rb]);
        mfmas<RB, 16>(ah, af, uf);
#pragma unroll
        for (int s = 0; s < 16; ++s) uf[s] = un[s];
        if (k0 & 32) {
#pragma unroll
          for (int rb = 0; rb < RB; ++rb) hh[rb] += ah[rb], ah[rb] = zero16();
        }
      }
    }
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = 32 * rb + row_of(e);
        const float z = LibmGates::sigm(hz[rb][e] - bgn), h = LibmGates::tanh(hh[rb][e]), xv = xs[row * P + co];
        if (row < nrows) {
          (a.g + (r0 + row) * a.ldg)[og] = (1.0f - z) * xv + z * h;
          if (a.gates) {
            float* gt = a.gates + (r0 + row) * a.ldgates;
            gt[ogt + D] = z;
            gt[ogt + 2 * D] = h;
          }
        }
      }
    }
    __syncthreads();   // x and r o x are read: the next tile may overwrite them
  }
}

// grid (groups)
template <int D>
__global__ __launch_bounds__(kThreads) SRL_UNPACKED_F32 void gtrxl_gate_bwd_kernel(GateArgs a) {
  constexpr int WC = D / 32, WR = 8 / WC, RT = 32 * WR, P = 3 * D + 4;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* As = sm;              // [RT][P]: a_r | a_z | a_g
  float* red = sm + RT * P;    // [8][32]: the wavefronts' column sums of a_z
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, hb = lane >> 5;
  const int n = 32 * (wave % WC) + l32, rl0 = 32 * (wave / WC);
  const unsigned wo = 8 * hb * D + n;                  // column n of a weight, from this lane half's first row of a chunk
  const unsigned ao = (rl0 + l32) * P + 8 * hb;        // the lane's LDS row as an A operand
  const unsigned co = (rl0 + 4 * hb) * P + n;          // its accumulator rows' column n in LDS
  const unsigned lrow = rl0 + 4 * hb;
  const unsigned odg = lrow * (unsigned)a.lddg + n, ox = lrow * (unsigned)a.ldx + n, ogt = lrow * (unsigned)a.ldgates + n;
  const unsigned odx = lrow * (unsigned)a.lddx + n, ody = lrow * (unsigned)a.lddy + n, orx = lrow * (unsigned)a.ldrx + n;
  const long tiles = (a.rows + RT - 1) / RT;
  float dbg = 0.f;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long r0 = tile * RT;
    const int nrows = (int)(a.rows - r0 < RT ? a.rows - r0 : RT) - (int)lrow;   // valid rows from this lane's first
    float xv[16], rv[16];
    f32x16 dxs, dxa = zero16();   // dxs = dg (1 - z) + t r: added to the product at the END (summed onto it, every MFMA would round at its size)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = row_of(e);   // (uniform: from the lane's first row)
      const bool ok = row < nrows;
      // (loads go through the tile's first row, which exists: an unwanted one lands on its element 0)
      float* gt = a.gates + (r0 + row) * a.ldgates;
      const float* gt0 = a.gates + r0 * a.ldgates;
      const unsigned og = ogt + row * (unsigned)a.ldgates;
      const float dgv = at_or0(a.dg + r0 * a.lddg, odg + row * (unsigned)a.lddg, ok);
      xv[e] = at_or0(a.x + r0 * a.ldx, ox + row * (unsigned)a.ldx, ok);
      rv[e] = at_or0(gt0, og, ok);
      const float z = at_or0(gt0 + D, og, ok), h = at_or0(gt0 + 2 * D, og, ok);
      const float ag = dgv * z * (1.0f - h * h), azv = dgv * (h - xv[e]) * (z * (1.0f - z));
      As[row * P + 2 * D + co] = ag;
      As[row * P + D + co] = azv;
      dbg += azv;   // (rows beyond `rows` are zeros)
      dxs[e] = dgv * (1.0f - z);
      if (ok) {
        gt[ogt + D] = azv;
        gt[ogt + 2 * D] = ag;
      }
    }
    __syncthreads();
    f32x16 t[1] = {zero16()}, tl[1] = {zero16()};   // (two-level sums as in the forward: tl is the short chain)
    {   // t = a_g Ug
      float bf[8], bn[8], af[1][8];
      col_frag<D>(a.w_x + 2 * D * D, wo, bf);
#pragma unroll 1
      for (int j0 = 0; j0 < D; j0 += 16) {
        const int jn = j0 + 16 < D ? j0 + 16 : j0;
        col_frag<D>(a.w_x + (2 * D + jn) * D, wo, bn);
        row_frag<8>(As + 2 * D + j0, ao, af[0]);
        mfmas<1, 8>(tl, af, bf);
#pragma unroll
        for (int s = 0; s < 8; ++s) bf[s] = bn[s];
        if ((j0 & 48) == 48) t[0] += tl[0], tl[0] = zero16();
      }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = row_of(e);
      const float arv = t[0][e] * xv[e] * (rv[e] * (1.0f - rv[e]));
      As[row * P + co] = arv;
      dxs[e] += t[0][e] * rv[e];
      if (row < nrows) {
        (a.gates + (r0 + row) * a.ldgates)[ogt] = arv;
        if (a.rx) (a.rx + (r0 + row) * a.ldrx)[orx] = rv[e] * xv[e];
      }
    }
    __syncthreads();
    f32x16 dya = zero16();   // (dy and dx stay single chains: their terms are small beside what a_z, a_r inherit from the gates)
    {   // dy = A w_y over K = 3D; dx += A[:, :2D] w_x[:2D] on the same A fragments
      float yf[8], yn[8], xf[8], xn[8];
      col_frag<D>(a.w_y, wo, yf);
      col_frag<D>(a.w_x, wo, xf);
#pragma unroll 1
      for (int j0 = 0; j0 < 2 * D; j0 += 16) {
        const int jn = j0 + 16;   // (2D is a row of w_y; of w_x too: Ug's first, loaded and not used)
        col_frag<D>(a.w_y + jn * D, wo, yn);
        col_frag<D>(a.w_x + jn * D, wo, xn);
        float af[8];
        row_frag<8>(As + j0, ao, af);
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          dya = __builtin_amdgcn_mfma_f32_32x32x2f32(af[s], yf[s], dya, 0, 0, 0);
          dxa = __builtin_amdgcn_mfma_f32_32x32x2f32(af[s], xf[s], dxa, 0, 0, 0);
        }
#pragma unroll
        for (int s = 0; s < 8; ++s) yf[s] = yn[s], xf[s] = xn[s];
      }
#pragma unroll 1
      for (int j0 = 2 * D; j0 < 3 * D; j0 += 16) {
        const int jn = j0 + 16 < 3 * D ? j0 + 16 : j0;
        col_frag<D>(a.w_y + jn * D, wo, yn);
        float af[8];
        row_frag<8>(As + j0, ao, af);
#pragma unroll
        for (int s = 0; s < 8; ++s) dya = __builtin_amdgcn_mfma_f32_32x32x2f32(af[s], yf[s], dya, 0, 0, 0);
#pragma unroll
        for (int s = 0; s < 8; ++s) yf[s] = yn[s];
      }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = row_of(e);
      if (row < nrows) {
        (a.dx + (r0 + row) * a.lddx)[odx] = dxs[e] + dxa[e];
        (a.dy + (r0 + row) * a.lddy)[ody] = dya[e];
      }
    }
    __syncthreads();   // A is read: the next tile may overwrite it
  }
  dbg += __shfl_xor(dbg, 32, 64);
  if (hb == 0) red[wave * 32 + l32] = dbg;
  __syncthreads();
  if (wave < WC && hb == 0) {   // (the first row of wavefronts: column n = 32 wave + l32)
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < WR; ++w) s += red[(w * WC + wave) * 32 + l32];
    a.ws[(long)blockIdx.x * D + n] = s;
  }
}

// d_bg = - the slabs summed in slab order; one thread per column
__global__ __launch_bounds__(256) void gtrxl_gate_fold_kernel(GateArgs a, int D) {
  const int n = threadIdx.x;
  if (n >= D) return;
  float s = 0.f;
  for (int w = 0; w < a.groups; ++w) s += a.ws[(long)w * D + n];
  a.d_bg[n] = -s;
}

bool supported(int D) { return D == 64 || D == 128 || D == 256; }
int64_t tiles_of(int D, int64_t rows, int rb) { return srl_ceil_div(rows, (int64_t)rb * (8192 / D)); }
int groups_of(int64_t tiles) { return (int)(tiles < kGroups ? tiles : kGroups); }
inline bool aligned16(const void* p) { return p && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
constexpr int64_t kMaxLd = 1 << 22;   // a tile is at most 256 rows and is addressed with 32-bit offsets
inline bool rows_ok(const void* p, int64_t ld, int width) { return aligned16(p) && ld % 4 == 0 && ld >= width && ld <= kMaxLd; }

template <int D, int RB>
void launch_fwd(const GateArgs& a, int groups, hipStream_t st) {
  constexpr int lds = (int)sizeof(float) * 2 * (32 * (8 / (D / 32)) * RB) * (D + 4);   // <= 69 632 B
  auto kern = gtrxl_gate_fwd_kernel<D, RB>;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  hipLaunchKernelGGL(kern, dim3(groups), dim3(kThreads), lds, st, a);
}
template <int D>
void launch(const GateArgs& a, bool bwd, hipStream_t st) {
  if (bwd) {
    constexpr int lds = (int)sizeof(float) * ((8192 / D) * (3 * D + 4) + 8 * 32);   // <= 101 376 B
    auto kern = gtrxl_gate_bwd_kernel<D>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipLaunchKernelGGL(kern, dim3(a.groups), dim3(kThreads), lds, st, a);
  } else {
    launch_fwd<D, 1>(a, groups_of(tiles_of(D, a.rows, 1)), st);
  }
}
void launch_any(int D, const GateArgs& a, bool bwd, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (D == 64) launch<64>(a, bwd, st);
  else if (D == 128) launch<128>(a, bwd, st);
  else launch<256>(a, bwd, st);
}

}  // namespace

extern "C" int srl_gtrxl_gate_supported(int D) { return supported(D) ? 1 : 0; }

extern "C" int64_t srl_gtrxl_gate_bwd_workspace(int D, int64_t rows) {
  if (!supported(D) || rows < 1) return -1;
  return (int64_t)groups_of(tiles_of(D, rows, 1)) * D * (int64_t)sizeof(float);
}

extern "C" int srl_gtrxl_gate_fwd(void* stream, const float* x, int64_t ldx, const float* y, int64_t ldy, const float* w_y,
                                  const float* w_x, const float* bg, int64_t rows, int D, float* g, int64_t ldg, float* gates,
                                  int64_t ldgates) {
  SRL_CHECK_ARG(supported(D), "unsupported (D in 64 | 128 | 256)");
  SRL_CHECK_ARG(rows >= 0, "rows");
  SRL_CHECK_ARG(rows_ok(x, ldx, D) && rows_ok(y, ldy, D) && rows_ok(g, ldg, D),
                "x, y, g: 16-byte aligned, leading dimension a multiple of 4 and >= D");
  SRL_CHECK_ARG(!gates || rows_ok(gates, ldgates, 3 * D), "gates: 16-byte aligned, leading dimension a multiple of 4 and >= 3D");
  SRL_CHECK_ARG(aligned16(w_y) && aligned16(w_x) && aligned16(bg), "w_y, w_x, bg (16-byte aligned)");
  if (rows == 0) return 0;
  GateArgs a{};
  a.x = x; a.ldx = ldx; a.y = y; a.ldy = ldy; a.w_y = w_y; a.w_x = w_x; a.bg = bg; a.rows = rows;
  a.g = g; a.ldg = ldg; a.gates = gates; a.ldgates = ldgates;
  launch_any(D, a, false, stream);
  SRL_LAUNCH_CHECK();
  return 0;
}

extern "C" int srl_gtrxl_gate_bwd(void* stream, const float* dg, int64_t lddg, const float* x, int64_t ldx, const float* y,
                                  int64_t ldy, const float* w_y, const float* w_x, float* gates, int64_t ldgates, int64_t rows, int D,
                                  float* dx, int64_t lddx, float* dy, int64_t lddy, float* rx, int64_t ldrx, float* d_bg,
                                  void* workspace, int64_t workspace_bytes) {
  SRL_CHECK_ARG(supported(D), "unsupported (D in 64 | 128 | 256)");
  SRL_CHECK_ARG(rows >= 1, "rows");
  SRL_CHECK_ARG(rows_ok(dg, lddg, D) && rows_ok(x, ldx, D) && rows_ok(y, ldy, D) && rows_ok(dx, lddx, D) && rows_ok(dy, lddy, D),
                "dg, x, y, dx, dy: 16-byte aligned, leading dimension a multiple of 4 and >= D");
  SRL_CHECK_ARG(rows_ok(gates, ldgates, 3 * D), "gates: 16-byte aligned, leading dimension a multiple of 4 and >= 3D");
  SRL_CHECK_ARG(!rx || rows_ok(rx, ldrx, D), "rx: 16-byte aligned, leading dimension a multiple of 4 and >= D");
  SRL_CHECK_ARG(aligned16(w_y) && aligned16(w_x) && d_bg, "w_y, w_x (16-byte aligned), d_bg");
  SRL_CHECK_ARG(aligned16(workspace) && workspace_bytes >= srl_gtrxl_gate_bwd_workspace(D, rows),
                "workspace: 16-byte aligned, srl_gtrxl_gate_bwd_workspace bytes");
  GateArgs a{};
  a.dg = dg; a.lddg = lddg; a.x = x; a.ldx = ldx; a.y = y; a.ldy = ldy; a.w_y = w_y; a.w_x = w_x; a.rows = rows;
  a.gates = gates; a.ldgates = ldgates; a.dx = dx; a.lddx = lddx; a.dy = dy; a.lddy = lddy; a.rx = rx; a.ldrx = ldrx;
  a.d_bg = d_bg; a.ws = static_cast<float*>(workspace); a.groups = groups_of(tiles_of(D, rows, 1));
  launch_any(D, a, true, stream);
  SRL_LAUNCH_CHECK();
  hipLaunchKernelGGL(gtrxl_gate_fold_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a, D);
  SRL_LAUNCH_CHECK();
  return 0;
}
