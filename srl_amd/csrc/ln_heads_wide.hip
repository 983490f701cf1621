// The closing LayerNorm and the heads behind it in one launch per direction for 9 to 32 head outputs (srl_ln_heads_wide_fwd /
// srl_ln_heads_wide_bwd): the contract of csrc/ln_heads.hip (actor_critic_policy.py:117-140; include/srl_hip.h), argument for
// argument, by another design.  ln_heads.hip keeps every head weight row in a lane's registers and finishes each dot product by a
// wave reduction: at 32 outputs and D = 512 that is 512 registers of weights and gradient sums and 32 reductions per row.  Here the
// head products run on the float32 matrix cores (v_mfma_f32_32x32x2_f32, exact float32 multiply-adds), the 9..32 output columns
// padded to 32 with zeros in registers (no padded parameter copies in HBM).
//
// Work split.  A workgroup of 4 wavefronts takes a tile of TR rows (32; at D = 1024 16 forward, 8 backward); the grid is min(tiles, CUs) and a
// workgroup walks tiles, the head weights loaded once.  Two layouts meet in LDS:
//   ROW layout     wavefront w owns rows [w TR / 4, (w + 1) TR / 4) of the tile; lane l holds channels 256 j + 4 l + (0..3): float4
//                  global accesses of whole kilobytes, the row statistics are wave butterflies -- the LayerNorm arithmetic
//                  (layer_norm.h) lives here, in both directions.
//   MFMA layout    lane l: column l & 31, k or row half l >> 5; accumulator register e: row (e & 3) + 8 (e >> 2) + 4 (l >> 5).
// The tile passes through LDS 256 CHANNELS AT A TIME ([TR][260] floats, 33 KB): a whole 32 x 512 tile with any padding is over
// 64 KB, and so is 16 x 1024; the rows wait in the registers of the wavefront that owns them (lane l's float4 number j is pass j).
// The pitch of 260 makes both the float4 accesses of the row layout and the MFMA layout's accesses conflict-free (float4 reads by
// lane = row: 8 lanes cover 32 banks; scalar reads / writes by lane = channel: consecutive).
//
// Forward.  The row owners load x (finishing slabs / bias / activation on the way, x_out written), form mean, rstd and
// f = LayerNorm(x) in registers.  Per pass they write f's 256 channels to LDS; wavefront w multiplies channels [64 w, 64 w + 64)
// of the pass: A = f (lane: row l & 31, read as float4 = 4 MFMA steps), B = W (lane: output l & 31, k = 256 j + 64 w + 32 (l >> 5)
// + s: 32 consecutive floats of a row of W per pass, D / 8 registers, resident across tiles).  K = D is thus split over the 4
// wavefronts (chains of D / 4); the four accumulators meet in LDS ([4][32][33]), the bias is added and only the heads' real
// columns are stored.
//
// Backward.  dy of both heads is a zero-padded [32][33] block in LDS, read once per tile as the A fragments of both products.
// Per pass the row owners write f to LDS; wavefront w owns channels [64 w, 64 w + 64) of the pass (two blocks of 32):
//   dW[out][ch] += dy^T f    A = dy^T (lane: out), B = f read from LDS with lane = channel; K = the tile's rows.  The
//                            accumulators (D / 8 registers) are held across every tile the workgroup walks and leave by ONE
//                            atomic per parameter and workgroup -- the MFMA has already summed the rows, nothing meets in LDS.
//   df[row][ch]   = dy W     A = dy (lane: row), B = W[out][ch] (D / 8 registers, resident up to D = 512; at D = 1024 these
//                            fragments, gamma and beta are read per pass from L2 and the dy fragments per block from LDS --
//                            with them resident the compiler spilled 53 registers to scratch), K = 32.
//                            df is written IN PLACE over the f the wavefront has just read (its own columns: no barrier between).
// The row owners take df back as float4 and run LayerNorm's backward as ln_heads.hip does: g = df gamma, the row sums, dgamma /
// dbeta in-lane across rows and tiles; after the last pass dx = rstd (g - m1 - xhat m2) times in_act's derivative, max |dx|
// tracked, whole rows stored as float4.  Two barriers per pass.  dgamma / dbeta of the 4 wavefronts meet in the tile's LDS at the
// end, one atomic per parameter and workgroup.  Head bias gradients are column sums of dy formed by the first 8 workgroups over a
// slice of the rows each (8 atomics per address, not one per workgroup or wavefront: ln_heads.hip measured the serial chain).
//
// Constraints held.
//   LDS       forward (TR 260 + 4 x 32 x 33) x 4 B = 50 176 B (TR = 32) / 33 536 B (TR = 16); backward (TR 260 + 32 x 33) x 4 B =
//             37 504 B, at D = 1024 the 4 D parameter sums of the end, 16 384 B: under 64 KB at every D -- this launch shares CUs
//             with other pipelines' persistent kernels.
//             D = 1024 takes the SHORTER TILE, not a two-pass one (16 rows forward, 8 backward; the MFMA's other rows are zeros
//             and are not read): the rows a wavefront keeps in registers across the passes set it, not LDS -- with 16 rows the
//             backward kernel spilled.  The MFMAs then run a quarter full; nothing in the project has a 1024-wide closing LayerNorm.
//   registers per lane of the 512 one wavefront per SIMD has (the build prints what the compiler took,
//             -Rpass-analysis=kernel-resource-usage, and must show no scratch), D = 256 / 512 / 1024:
//             forward   f 32 / 64 / 64, W 32 / 64 / 128, gamma beta x_bias 12 / 24 / 48, acc 16      compiled: 162 / 242 / 314
//             backward  x + g 64 / 128 / 64, W 32 / 64 / 16, dW 32 / 64 / 128, dy fragments 32 / 32 / 20,
//                       gamma beta 8 / 16 / 8, dgamma dbeta 8 / 16 / 32, f + df 32                    compiled: 306 / 474 / 448
//             all with no scratch.
//   stores    ordinary vector stores and float atomics only; no cooperative launch, no flags in memory.
// Rows beyond n in the last tile are predicated: nothing is read or written for them (their lanes compute on zeros).
#include "layer_norm.h"
#include "srl_common.h"

#include "../../include/srl_hip.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
using f4 = __attribute__((ext_vector_type(4))) float;

constexpr int kMinOut = SRL_LN_HEADS_MAX_OUT + 1;   // what ln_heads.hip does not take
constexpr int kMaxOut = SRL_LN_HEADS_WIDE_MAX_OUT;  // = the MFMA's 32 columns
constexpr int kP = 260;        // floats between the rows of the 256-channel block in LDS
constexpr int kDy = 33;        // ... of the dy block and of the forward's partial accumulators
constexpr int kDbGroups = 8;   // workgroups that form the heads' bias gradients
static_assert(kMaxOut == 32, "the output columns are one MFMA block");

// rows of a tile: what a wavefront keeps in registers of its rows across the passes (forward f; backward x and g) sets it
constexpr int tile_rows(int D, bool bwd) { return D > 512 ? (bwd ? 8 : 16) : 32; }
// backward LDS: the pass block and the dy block; at the end 4 D parameter sums over both
constexpr int bwd_lds_floats(int D) { return tile_rows(D, true) * kP + 32 * kDy > 4 * D ? tile_rows(D, true) * kP + 32 * kDy : 4 * D; }

struct LwArgs {
  const float* x;
  long ldx, n;
  const float *gamma, *beta;
  const float* W[2];      // head weights [A, D] row-major
  const float* b[2];
  int A[2];
  float* y[2];
  long ldy[2];
  float *mean, *rstd;
  // backward
  const float* dy[2];
  long lddy[2];
  int in_act;
  float* dx;
  long lddx;
  float *dgamma, *dbeta;
  float* dW[2];
  float* db[2];
  float* dx_absmax;
  // forward: x = act(sum of x_slabs slabs (x_slab_stride floats apart) + x_bias), as srl_ln_heads_fwd
  int x_slabs;
  long x_slab_stride;
  const float* x_bias;
  int x_act;
  float* x_out;
  long ldxo;
};

__device__ __forceinline__ float allsum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// the row (within the tile) of accumulator register e in lane half hb
__device__ __forceinline__ constexpr int row_of(int e, int hb) { return (e & 3) + 8 * (e >> 2) + 4 * hb; }

// row layout: lane l holds channels 256 j + 4 l + (0..3), j < NV / 4
template <int NV>
__device__ __forceinline__ void load_row(const float* p, int lane, float (&v)[NV]) {
#pragma unroll
  for (int j = 0; j < NV / 4; ++j) {
    const f4 q = *reinterpret_cast<const f4*>(p + 256 * j + 4 * lane);
    v[4 * j] = q[0]; v[4 * j + 1] = q[1]; v[4 * j + 2] = q[2]; v[4 * j + 3] = q[3];
  }
}
template <int NV>
__device__ __forceinline__ void store_row(float* p, int lane, const float (&v)[NV]) {
#pragma unroll
  for (int j = 0; j < NV / 4; ++j) {
    const f4 q = {v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]};
    *reinterpret_cast<f4*>(p + 256 * j + 4 * lane) = q;
  }
}
// row `o` of the heads' stacked weights (or of their gradients); o < A[0] + A[1]
__device__ __forceinline__ const float* w_row(const LwArgs& a, int o, int D) {
  return o < a.A[0] ? a.W[0] + (long)o * D : a.W[1] + (long)(o - a.A[0]) * D;
}
__device__ __forceinline__ float* dw_row(const LwArgs& a, int o, int D) {
  return o < a.A[0] ? a.dW[0] + (long)o * D : a.dW[1] + (long)(o - a.A[0]) * D;
}
__device__ __forceinline__ float dy_at(const LwArgs& a, long row, int o) {
  return o < a.A[0] ? a.dy[0][row * a.lddy[0] + o] : a.dy[1][row * a.lddy[1] + o - a.A[0]];
}

template <int D>
__global__ __launch_bounds__(256, 1) void ln_heads_wide_fwd_kernel(LwArgs a) {
  constexpr int NV = D / 64, NP = D / 256, TR = tile_rows(D, false), RW = TR / 4;
  extern __shared__ __attribute__((aligned(16))) float sm[];   // [TR][kP]: a pass of f; then [4][32][kDy]: the partial products
  float* red = sm + TR * kP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, hb = lane >> 5;
  const int A0 = a.A[0], AT = a.A[0] + a.A[1];
  // B fragments: w[j][s] = W[l32][256 j + 64 wave + 32 hb + s]; zeros in the padded columns
  float w[NP][32];
#pragma unroll
  for (int j = 0; j < NP; ++j)
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      f4 v = {0.f, 0.f, 0.f, 0.f};
      if (l32 < AT) v = *reinterpret_cast<const f4*>(w_row(a, l32, D) + 256 * j + 64 * wave + 32 * hb + 4 * q);
      w[j][4 * q] = v[0]; w[j][4 * q + 1] = v[1]; w[j][4 * q + 2] = v[2]; w[j][4 * q + 3] = v[3];
    }
  float g[NV], be[NV], xb[NV];
  load_row<NV>(a.gamma, lane, g);
  load_row<NV>(a.beta, lane, be);
#pragma unroll
  for (int k = 0; k < NV; ++k) xb[k] = 0.f;
  if (a.x_bias) load_row<NV>(a.x_bias, lane, xb);
  const int oo = tid & 31;   // the epilogue's output column
  float bias = 0.f;
  if (oo < AT) {
    const float* bp = oo < A0 ? a.b[0] : a.b[1];
    if (bp) bias = bp[oo < A0 ? oo : oo - A0];
  }
  const long ntiles = (a.n + TR - 1) / TR;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long row0 = tile * TR;
    const int nv = (int)(a.n - row0 < TR ? a.n - row0 : TR);
    float f[RW][NV];
#pragma unroll
    for (int i = 0; i < RW; ++i) {
      const int r = wave * RW + i;
      if (r < nv) {   // (uniform in the wavefront)
        const long row = row0 + r;
        float x[NV];
        load_row<NV>(a.x + row * a.ldx, lane, x);
        if (a.x_slabs > 1 || a.x_bias || a.x_act) {
          for (int sl = 1; sl < a.x_slabs; ++sl) {
            float t[NV];
            load_row<NV>(a.x + sl * a.x_slab_stride + row * a.ldx, lane, t);
#pragma unroll
            for (int k = 0; k < NV; ++k) x[k] += t[k];
          }
#pragma unroll
          for (int k = 0; k < NV; ++k) {
            x[k] += xb[k];
            x[k] = a.x_act == 1 ? fmaxf(x[k], 0.f) : (a.x_act == 2 ? tanhf(x[k]) : x[k]);
          }
          if (a.x_out) store_row<NV>(a.x_out + row * a.ldxo, lane, x);
        }
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < NV; ++k) s += x[k];
        const float mean = allsum(s) / (float)D;
        float q = 0.f;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
          x[k] -= mean;
          q = fmaf(x[k], x[k], q);
        }
        const float rstd = ln_rstd(allsum(q), D);
#pragma unroll
        for (int k = 0; k < NV; ++k) f[i][k] = ln_affine(x[k] * rstd, g[k], be[k]);   // x holds x - mean
        if (lane == 0) {
          a.mean[row] = mean;
          a.rstd[row] = rstd;
        }
      } else {
#pragma unroll
        for (int k = 0; k < NV; ++k) f[i][k] = 0.f;
      }
    }
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
#pragma unroll
      for (int i = 0; i < RW; ++i) {
        const f4 q = {f[i][4 * j], f[i][4 * j + 1], f[i][4 * j + 2], f[i][4 * j + 3]};
        *reinterpret_cast<f4*>(sm + (wave * RW + i) * kP + 4 * lane) = q;
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        f4 av = {0.f, 0.f, 0.f, 0.f};
        if (l32 < TR) av = *reinterpret_cast<const f4*>(sm + l32 * kP + 64 * wave + 32 * hb + 4 * q);
#pragma unroll
        for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[c], w[j][4 * q + c], acc, 0, 0, 0);
      }
      __syncthreads();   // the pass is read: the next one (or the next tile's first) may overwrite it
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) red[(wave * 32 + row_of(e, hb)) * kDy + l32] = acc[e];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = (tid >> 5) + 8 * i;
      const float v = ((red[r * kDy + oo] + red[(32 + r) * kDy + oo]) + (red[(64 + r) * kDy + oo] + red[(96 + r) * kDy + oo])) + bias;
      if (r < nv && oo < AT) {
        if (oo < A0) a.y[0][(row0 + r) * a.ldy[0] + oo] = v;
        else a.y[1][(row0 + r) * a.ldy[1] + oo - A0] = v;
      }
    }
    // (the next tile's partial products are written two barriers from here)
  }
}

template <int D>
__global__ __launch_bounds__(256, 1) void ln_heads_wide_bwd_kernel(LwArgs a) {
  constexpr int NV = D / 64, NP = D / 256, TR = tile_rows(D, true), RW = TR / 4;
  constexpr bool kWResident = D <= 512;   // beyond it the lane budget is the dW accumulators': W, gamma, beta come per pass from
                                           // L2 and the dy fragments per block from LDS
  extern __shared__ __attribute__((aligned(16))) float sm[];   // [TR][kP]: a pass of f, then of df; [32][kDy]: dy of the tile
  float* dys = sm + TR * kP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, hb = lane >> 5;
  const int AT = a.A[0] + a.A[1];
  float g[kWResident ? NV : 4], be[kWResident ? NV : 4], accg[NV], accb[NV];
  if constexpr (kWResident) {
    load_row<NV>(a.gamma, lane, g);
    load_row<NV>(a.beta, lane, be);
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) accg[k] = accb[k] = 0.f;
  // B fragments of df = dy W: W[2 s + hb][256 j + 64 wave + 32 b + l32], zeros from row AT on
  auto w_frag = [&](int j, int b, float (&wf)[16]) {
#pragma unroll
    for (int s = 0; s < 16; ++s) wf[s] = 2 * s + hb < AT ? w_row(a, 2 * s + hb, D)[256 * j + 64 * wave + 32 * b + l32] : 0.f;
  };
  float wres[kWResident ? NP : 1][2][16];
  if constexpr (kWResident) {
#pragma unroll
    for (int j = 0; j < NP; ++j)
#pragma unroll
      for (int b = 0; b < 2; ++b) w_frag(j, b, wres[j][b]);
  }
  f32x16 accw[NP][2];   // dW[row_of(e, hb)][256 j + 64 wave + 32 b + l32]
#pragma unroll
  for (int j = 0; j < NP; ++j)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) accw[j][b][e] = 0.f;
  float amax = 0.f;
  const long ntiles = (a.n + TR - 1) / TR;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long row0 = tile * TR;
    const int nv = (int)(a.n - row0 < TR ? a.n - row0 : TR);
    // (every read of the last tile's dy block lies before that tile's first pass barrier)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = (tid >> 5) + 8 * i, o = tid & 31;
      dys[r * kDy + o] = (r < nv && o < AT) ? dy_at(a, row0 + r, o) : 0.f;
    }
    float x[RW][NV], mean[RW], rstd[RW];
#pragma unroll
    for (int i = 0; i < RW; ++i) {
      const int r = wave * RW + i;
      if (r < nv) {
        load_row<NV>(a.x + (row0 + r) * a.ldx, lane, x[i]);
        mean[i] = a.mean[row0 + r];
        rstd[i] = a.rstd[row0 + r];
      } else {
#pragma unroll
        for (int k = 0; k < NV; ++k) x[i][k] = 0.f;
        mean[i] = rstd[i] = 0.f;
      }
    }
    __syncthreads();
    float at[TR / 2], ad[16];   // A fragments: dy^T (lane: out l32, k = row 2 s + hb) and dy (lane: row l32, k = out 2 s + hb)
    auto dy_frags = [&]() {
#pragma unroll
      for (int s = 0; s < TR / 2; ++s) at[s] = dys[(2 * s + hb) * kDy + l32];
#pragma unroll
      for (int s = 0; s < 16; ++s) ad[s] = dys[l32 * kDy + 2 * s + hb];
    };
    if constexpr (kWResident) dy_frags();
    float gg[RW][NV], m1[RW], m2[RW];
#pragma unroll
    for (int i = 0; i < RW; ++i) m1[i] = m2[i] = 0.f;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const int pj = kWResident ? 4 * j : 0;   // this pass's gamma / beta: g[pj + c], be[pj + c]
      if constexpr (!kWResident) {
        const f4 gv = *reinterpret_cast<const f4*>(a.gamma + 256 * j + 4 * lane), bv = *reinterpret_cast<const f4*>(a.beta + 256 * j + 4 * lane);
#pragma unroll
        for (int c = 0; c < 4; ++c) g[c] = gv[c], be[c] = bv[c];
      }
#pragma unroll
      for (int i = 0; i < RW; ++i) {
        f4 q;
#pragma unroll
        for (int c = 0; c < 4; ++c) q[c] = ln_affine(ln_xhat(x[i][4 * j + c], mean[i], rstd[i]), g[pj + c], be[pj + c]);
        *reinterpret_cast<f4*>(sm + (wave * RW + i) * kP + 4 * lane) = q;
      }
      __syncthreads();
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int cl = 64 * wave + 32 * b + l32;   // this lane's channel of the pass
        if constexpr (!kWResident) dy_frags();
#pragma unroll
        for (int s = 0; s < TR / 2; ++s) accw[j][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(at[s], sm[(2 * s + hb) * kP + cl], accw[j][b], 0, 0, 0);
        float wl[16];
        if constexpr (!kWResident) w_frag(j, b, wl);
        f32x16 df;
#pragma unroll
        for (int e = 0; e < 16; ++e) df[e] = 0.f;
#pragma unroll
        for (int s = 0; s < 16; ++s) df = __builtin_amdgcn_mfma_f32_32x32x2f32(ad[s], kWResident ? wres[kWResident ? j : 0][b][s] : wl[s], df, 0, 0, 0);
        // in place: these columns are this wavefront's, and it has read them
#pragma unroll
        for (int e = 0; e < 16; ++e)
          if (row_of(e, hb) < TR) sm[row_of(e, hb) * kP + cl] = df[e];
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < RW; ++i) {
        const f4 dfv = *reinterpret_cast<const f4*>(sm + (wave * RW + i) * kP + 4 * lane);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int k = 4 * j + c;
          gg[i][k] = ln_bwd_accumulate(dfv[c], g[pj + c], ln_xhat(x[i][k], mean[i], rstd[i]), m1[i], m2[i], accg[k], accb[k]);
        }
      }
      // (a wavefront rewrites only the rows it has just read; the other wavefronts' reads of them follow the next barrier)
    }
#pragma unroll
    for (int i = 0; i < RW; ++i) {
      const int r = wave * RW + i;
      const float M1 = allsum(m1[i]) / (float)D, M2 = allsum(m2[i]) / (float)D;
      float dx[NV];
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const float xv = x[i][k];
        const float der = a.in_act == 1 ? (xv > 0.f ? 1.f : 0.f) : (a.in_act == 2 ? 1.f - xv * xv : 1.f);
        dx[k] = ln_dx(gg[i][k], ln_xhat(xv, mean[i], rstd[i]), M1, M2, rstd[i]) * der;
        amax = fmaxf(amax, fabsf(dx[k]));
      }
      if (r < nv) store_row<NV>(a.dx + (row0 + r) * a.lddx, lane, dx);
    }
  }
  if (a.dx_absmax) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off, 64));
    if (lane == 0 && amax > 0.f) atomicMax(reinterpret_cast<int*>(a.dx_absmax), __float_as_int(amax));
  }
  // head weight gradients: every (output, channel) of the workgroup is in exactly one lane's accumulator
#pragma unroll
  for (int j = 0; j < NP; ++j)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (row_of(e, hb) < AT) atomicAdd(dw_row(a, row_of(e, hb), D) + 256 * j + 64 * wave + 32 * b + l32, accw[j][b][e]);
  // dgamma, dbeta: the four wavefronts' sums meet in LDS (4 D floats over the tile and the dy block: bwd_lds_floats), one atomic
  // per parameter
#pragma unroll
  for (int pl = 0; pl < 2; ++pl) {
    __syncthreads();
    if (pl == 0) store_row<NV>(sm + wave * D, lane, accg);
    else store_row<NV>(sm + wave * D, lane, accb);
    __syncthreads();
    for (int c = tid; c < D; c += 256) atomicAdd((pl == 0 ? a.dgamma : a.dbeta) + c, (sm[c] + sm[D + c]) + (sm[2 * D + c] + sm[3 * D + c]));
  }
  // head bias gradients = column sums of dy: the first kDbGroups workgroups sum a slice of the rows each
  const int G = gridDim.x < kDbGroups ? (int)gridDim.x : kDbGroups;
  if ((int)blockIdx.x < G && (a.db[0] || a.db[1])) {
    const int o = tid & 31;
    const long r0 = a.n * blockIdx.x / G, r1 = a.n * (blockIdx.x + 1) / G;
    float s = 0.f;
    if (o < AT)
      for (long row = r0 + (tid >> 5); row < r1; row += 8) s += dy_at(a, row, o);
    __syncthreads();   // the parameter sums above are read
    dys[(tid >> 5) * kDy + o] = s;
    __syncthreads();
    if (tid < AT) {
      float v = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) v += dys[i * kDy + tid];
      float* dst = tid < a.A[0] ? a.db[0] : a.db[1];
      if (dst) atomicAdd(dst + (tid < a.A[0] ? tid : tid - a.A[0]), v);
    }
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int total_outputs(int D, int nh, const int32_t* A) {
  if (!(D == 256 || D == 512 || D == 1024) || nh < 1 || nh > 2 || !A) return -1;
  int at = 0;
  for (int h = 0; h < nh; ++h) {
    if (A[h] < 1) return -1;
    at += A[h];
  }
  return at >= kMinOut && at <= kMaxOut ? at : -1;
}

int check_common(const float* x, int64_t ldx, int D, const float* gamma, const float* beta, const float* const* W, const int32_t* A,
                 int nh) {
  if (!x || !gamma || !beta || !W || total_outputs(D, nh, A) < 0) return -1;
  if (ldx % 4 != 0 || ldx < D || !aligned16(x) || !aligned16(gamma) || !aligned16(beta)) return -1;
  for (int h = 0; h < nh; ++h)
    if (!W[h] || !aligned16(W[h])) return -1;
  return 1;
}

int num_cus() {
  static int n = 0;
  if (!n) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) n = v;
    else return 256;
  }
  return n;
}

template <int D>
void launch(const LwArgs& a, bool bwd, hipStream_t st) {
  const int TR = tile_rows(D, bwd);
  const long tiles = srl_ceil_div(a.n, (long)TR), cus = num_cus();
  const unsigned grid = (unsigned)(tiles < cus ? tiles : cus);
  const int lds = (int)sizeof(float) * (bwd ? bwd_lds_floats(D) : TR * kP + 4 * 32 * kDy);   // (under the 64 KB every kernel may ask for)
  if (bwd) hipLaunchKernelGGL(ln_heads_wide_bwd_kernel<D>, dim3(grid), dim3(256), lds, st, a);
  else hipLaunchKernelGGL(ln_heads_wide_fwd_kernel<D>, dim3(grid), dim3(256), lds, st, a);
}

void launch_any(int D, const LwArgs& a, bool bwd, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (D == 256) launch<256>(a, bwd, st);
  else if (D == 512) launch<512>(a, bwd, st);
  else launch<1024>(a, bwd, st);
}

}  // namespace

extern "C" int srl_ln_heads_wide_supported(int D, int n_heads, const int32_t* head_dims) {
  return total_outputs(D, n_heads, head_dims) > 0;
}

extern "C" int srl_ln_heads_wide_fwd(void* stream, const float* x, int64_t ldx, int64_t n, int D, const float* gamma, const float* beta,
                                     int n_heads, const float* const* W, const float* const* b, const int32_t* head_dims,
                                     float* const* y, const int64_t* ldy, float* mean, float* rstd, int x_slabs, int64_t x_slab_stride,
                                     const float* x_bias, int x_act, float* x_out, int64_t ldxo) {
  SRL_CHECK_ARG(check_common(x, ldx, D, gamma, beta, W, head_dims, n_heads) > 0,
                "unsupported (D in 256 | 512 | 1024, 1-2 heads, 9..SRL_LN_HEADS_WIDE_MAX_OUT outputs, 16-byte aligned rows)");
  SRL_CHECK_ARG(y && ldy && mean && rstd && n >= 0, "null output");
  SRL_CHECK_ARG(x_slabs >= 1 && (x_slabs == 1 || x_slab_stride % 4 == 0) && x_act >= 0 && x_act <= 2 && (!x_bias || aligned16(x_bias)),
                "x_slabs >= 1, aligned slabs / bias, x_act 0..2");
  SRL_CHECK_ARG(!x_out || ((x_slabs > 1 || x_bias || x_act) && ldxo % 4 == 0 && ldxo >= D && aligned16(x_out)),
                "x_out: only with a finishing step (slabs / bias / activation), 16-byte aligned rows");
  if (n == 0) return 0;
  LwArgs a{};
  a.x = x; a.ldx = ldx; a.n = n; a.gamma = gamma; a.beta = beta; a.mean = mean; a.rstd = rstd;
  a.x_slabs = x_slabs; a.x_slab_stride = x_slab_stride; a.x_bias = x_bias; a.x_act = x_act; a.x_out = x_out; a.ldxo = ldxo;
  for (int h = 0; h < n_heads; ++h) {
    SRL_CHECK_ARG(y[h] && ldy[h] >= head_dims[h], "null head output / short rows");
    a.W[h] = W[h]; a.b[h] = b ? b[h] : nullptr; a.A[h] = head_dims[h]; a.y[h] = y[h]; a.ldy[h] = ldy[h];
  }
  launch_any(D, a, false, stream);
  SRL_LAUNCH_CHECK();
  return 0;
}

extern "C" int srl_ln_heads_wide_bwd(void* stream, const float* x, int64_t ldx, int64_t n, int D, const float* gamma, const float* beta,
                                     const float* mean, const float* rstd, int n_heads, const float* const* W,
                                     const int32_t* head_dims, const float* const* dy, const int64_t* lddy, int in_act, float* dx,
                                     int64_t lddx, float* dgamma, float* dbeta, float* const* dW, float* const* db,
                                     float* dx_absmax) {
  SRL_CHECK_ARG(check_common(x, ldx, D, gamma, beta, W, head_dims, n_heads) > 0, "unsupported (see srl_ln_heads_wide_fwd)");
  SRL_CHECK_ARG(mean && rstd && dy && lddy && dx && dgamma && dbeta && dW && n >= 0, "null tensor");
  SRL_CHECK_ARG(lddx % 4 == 0 && lddx >= D && aligned16(dx) && in_act >= 0 && in_act <= 2, "dx rows / activation");
  if (n == 0) return 0;
  LwArgs a{};
  a.x = x; a.ldx = ldx; a.n = n; a.gamma = gamma; a.beta = beta; a.mean = const_cast<float*>(mean); a.rstd = const_cast<float*>(rstd);
  a.in_act = in_act; a.dx = dx; a.lddx = lddx; a.dgamma = dgamma; a.dbeta = dbeta; a.dx_absmax = dx_absmax;
  for (int h = 0; h < n_heads; ++h) {
    SRL_CHECK_ARG(dy[h] && lddy[h] >= head_dims[h] && dW[h], "null head gradient");
    a.W[h] = W[h]; a.A[h] = head_dims[h]; a.dy[h] = dy[h]; a.lddy[h] = lddy[h]; a.dW[h] = dW[h]; a.db[h] = db ? db[h] : nullptr;
  }
  launch_any(D, a, true, stream);
  SRL_LAUNCH_CHECK();
  return 0;
}
