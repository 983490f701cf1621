// The recurrent time loop of a chunk inside ONE launch at H = 128, the width every recurrent preset defaults to (football,
// overcooked, the generic actor-critic): what csrc/rnn_seq.hip does at H in {32, 64}, on the same buffers and with the same saved
// values (include/srl_hip.h), by another design.  rnn_seq keeps W_hh in LDS and the state in registers; at H = 128 W_hh is
// 192 KB (GRU) / 256 KB (LSTM) of float32 and no longer fits a CU's 160 KB of LDS -- but it fits the register files of one
// four-wavefront workgroup.  So here the WEIGHTS are stationary in registers and the STATE goes through LDS.
//
// Work split.  A workgroup (4 wavefronts, one per SIMD) takes a tile of 32 rows through all C steps; the grid is min(tiles, CUs)
// and a workgroup walks the tiles, its weights loaded once.  Rows are independent (autoreset_rnn.py:42-66): no workgroup reads
// what another writes, there is no cooperative launch, no flag in memory, and every store is an ordinary vector store.
//
// Forward.  Wavefront w owns hidden units [32 w, 32 w + 32) in EVERY gate, so the cell of a unit is local to a lane.  Per step
// D[row][unit] = h . W_hh^T on v_mfma_f32_32x32x2_f32 (exact float32 multiply-adds): the state is the A operand (lane l: row
// l & 31, read from LDS), the wavefront's slice of W_hh the B operand (lane l: unit 32 w + (l & 31)); MFMA step s of 64 takes
// k = 64 (l >> 5) + s from both, so a lane's B fragments of a gate are 64 consecutive floats of one row of W_hh: 64 registers
// per gate, 192 (GRU) / 256 (LSTM) per lane, resident across steps and tiles, b_hh one register per gate.  The accumulator of
// lane l holds its unit for the 16 rows (e & 3) + 8 (e >> 2) + 4 (l >> 5); the G gate blocks put r, z, n (i, f, g, o) of a
// (row, unit) in the same lane and register index.  The state of the tile is a [k][row] block in LDS, double buffered: a step
// reads one buffer (all wavefronts, every k), writes h_new (1 - reset_next) for its own units into the other, and ends in the
// step's one barrier.  A step's gi / pre are asked for at its top and used after its MFMAs (they depend on no earlier step, so
// this hides them as a load one step ahead would, without a second set of registers); the LSTM's c stays in the registers of
// the wavefront that owns its units (so does the GRU's h_in for z * h_in).
//
// Summation.  Every product is summed in four chains of K / 4 (the forward a gate at a time, four accumulators; the backward one
// chain after the other), added afterwards: the summation of the per-step kernel (csrc/rnn_step.hip).  One chain of 128
// roundings measured 2.5 to 3 times that kernel's error against float64 (up to 5 times in d gi), four chains 0.7 to 1.5 times.
//
// Backward.  The same split and loop from C - 1 down to 0; the product is d h_in = d gates . W_hh (K = 3 H / 4 H).  Wavefront w
// owns OUTPUT units [32 w, 32 w + 32) and holds W_hh[:, 32 w .. 32 w + 32) as B fragments (MFMA step s of K / 2 takes k = (K / 2)
// (l >> 5) + s): 192 / 256 registers.  It computes the cell backward for its units (d h_in and d c_in of the step after arrive
// in its own accumulator layout: the carries never leave registers), writes its d-gate columns in place to HBM and as a
// [k][row] block to LDS; after a barrier every wavefront multiplies all K columns of that block; a second barrier frees the
// block for the next step.  The next step's operands are loaded while the MFMAs run.
//
// Budget (per lane, of the 512 registers one wavefront per SIMD has, accumulation registers counted; the build prints what the
// compiler took, -Rpass-analysis=kernel-resource-usage, and must show no scratch):
//   forward   GRU  192 W + 3 b + 64 acc (a gate's four chains) + 48 gi + 48 gh + 16 h_in            compiled: 401, no scratch
//             LSTM 256 W + 4 b + 64 acc + 64 pre (the sums are added into them) + 16 c            compiled: 497, no scratch
//   backward  192 / 256 W + 16 acc + 16 sum + 16 (+ 16) carries + 96 / 112 operands of the next step  compiled: 410 / 488, no scratch
// LDS (rows of a [k][row] block are 33 floats apart: the transposed writes, lane = k, hit 32 banks):
//   forward   2 x 128 x 33 x 4 B = 33 792 B
//   backward  GRU 384 x 33 x 4 B = 50 688 B, LSTM 512 x 33 x 4 B = 67 584 B
// Rows beyond N in the last tile are predicated: nothing is read or written for them (their lanes compute on zeros).
// The gates are libm's (rnn_cell::LibmGates), as on the per-step path this kernel is held against.
#include "rnn_cell.h"
#include "srl_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
using f4 = __attribute__((ext_vector_type(4))) float;
using Gates = rnn_cell::LibmGates;

constexpr int H = 128;   // the one width (srl_rnn_wseq_supported)
constexpr int LDR = 33;  // floats between the rows of a [k][row] block in LDS

struct WseqArgs {
  float* pre;            // LSTM: [C][N][4H] = W_ih x + b_ih -> activated gates (forward) -> d pre (backward); GRU: gi [C][N][3H] likewise
  float* gh;             // GRU: [C][N][3H]: W_hh h + b_hh (forward), d gh (backward)
  const float* w_hh;     // [G H][H]
  const float* b_hh;     // [G H] or NULL
  float* hin;            // [C][N][H]: hin[0] is the caller's (masked); steps 1.. written by the forward
  float* cin;            // LSTM: [C][N][H] likewise
  float* y;              // [C][N][H]
  float* cnew;           // LSTM: [C][N][H]
  const uint8_t* reset;  // [C][N] or NULL: reset[c] masks the state ENTERING step c
  const float* dy;       // backward: [C][N][ld_dy] or NULL
  long ld_dy;
  long N;
  int C;
};

// the row (within the tile) of accumulator register e in lane half hb: rc_of(e) + 4 hb
__device__ __forceinline__ constexpr int rc_of(int e) { return (e & 3) + 8 * (e >> 2); }
__device__ __forceinline__ int row_of(int e, int hb) { return rc_of(e) + 4 * hb; }
// ... is one of the tile's nv rows (the lane's side of the comparison is the same for every e)
__device__ __forceinline__ bool row_ok(int e, int hb, int nv) { return 4 * hb < nv - rc_of(e); }

// 16 values of one column of a row-major block, rows `ld` floats apart: `p` is the tile's first row (the same in every lane, so
// that a row's address is scalar arithmetic), `v` = 4 hb ld + column the lane's one 32-bit offset.  Rows from nv on are neither
// read (0 instead) nor written.
__device__ __forceinline__ void col_load(const float* p, long ld, unsigned v, int hb, int nv, float (&x)[16]) {
#pragma unroll
  for (int e = 0; e < 16; ++e) x[e] = row_ok(e, hb, nv) ? (p + rc_of(e) * ld)[v] : 0.f;
}
__device__ __forceinline__ void col_store(float* p, long ld, unsigned v, int hb, int nv, const float (&x)[16]) {
#pragma unroll
  for (int e = 0; e < 16; ++e)
    if (row_ok(e, hb, nv)) (p + rc_of(e) * ld)[v] = x[e];
}
// bit e: row_of(e) is reset; `r`: the flags of the tile's first row in the step asked about, or NULL
__device__ __forceinline__ unsigned reset_bits(const uint8_t* r, int hb, int nv) {
  unsigned m = 0;
  if (r) {
#pragma unroll
    for (int e = 0; e < 16; ++e)
      if (row_ok(e, hb, nv) && (r + rc_of(e))[4u * hb]) m |= 1u << e;
  }
  return m;
}

// KIND 1: LSTM (gates i | f | g | o), 0: GRU (r | z | n)
template <int KIND>
__global__ __launch_bounds__(256, 1) void rnn_wseq_fwd_kernel(WseqArgs a) {
  constexpr int G = KIND ? 4 : 3;
  extern __shared__ __attribute__((aligned(16))) float sm[];   // [2][H][LDR]: the tile's state, [k][row]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, hb = lane >> 5;
  const int unit = 32 * wave + l32;
  const unsigned vg = 4u * hb * G * H + unit, vh = 4u * hb * H + unit;   // the lane's offset in a block of G H / H columns
  const long N = a.N;
  // B fragments: w[g][s] = W_hh[g H + unit][64 hb + s]
  float w[G][64], bv[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const float* wr = a.w_hh + (long)(g * H + unit) * H + 64 * hb;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const f4 v = *reinterpret_cast<const f4*>(wr + 4 * q);
      w[g][4 * q] = v[0]; w[g][4 * q + 1] = v[1]; w[g][4 * q + 2] = v[2]; w[g][4 * q + 3] = v[3];
    }
    bv[g] = a.b_hh ? a.b_hh[g * H + unit] : 0.f;
  }
  const long ntiles = (N + 31) / 32;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long row0 = tile * 32;
    const int nv = (int)(N - row0 < 32 ? N - row0 : 32);   // rows of this tile
    // the state entering step 0 -> buffer 0 (the last step's barrier has retired every read of the tile before)
    {
      int t = tid;
      asm volatile("" : "+v"(t));   // (derived anew per tile: sixteen rows and addresses are not worth keeping across the steps)
      const float* src = a.hin + row0 * H;
#pragma unroll
      for (int i = 0; i < 16; ++i)   // element t + 256 i of the tile: row (t >> 7) + 2 i, k = t & 127
        sm[(t & 127) * LDR + (t >> 7) + 2 * i] = (t >> 7) < nv - 2 * i ? (src + 256 * i)[(unsigned)t] : 0.f;
    }
    __syncthreads();
    float st[16];   // GRU: h_in of this lane's (row, unit)s; LSTM: c_in
    if constexpr (KIND) {
      col_load(a.cin + row0 * H, H, vh, hb, nv, st);
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e) st[e] = sm[unit * LDR + row_of(e, hb)];
    }
    for (int c = 0; c < a.C; ++c) {
      const long base = (long)c * N + row0;   // the tile's first row of step c
      const bool nxt = c + 1 < a.C;
      const float* hs = sm + (c & 1) * H * LDR;
      float* hd = sm + ((c + 1) & 1) * H * LDR;
      const unsigned rs = nxt && a.reset ? reset_bits(a.reset + base + N, hb, nv) : 0u;
      // gi / pre of this step: asked for here, used after the products (nothing of the step before is needed to ask)
      float p[G][16];
#pragma unroll
      for (int g = 0; g < G; ++g) col_load(a.pre + base * G * H + g * H, G * H, vg, hb, nv, p[g]);
      // W_hh h + b_hh, a gate at a time: k in four chains of 32 (MFMA steps 16 j .. 16 j + 15) summed as a tree, the summation
      // of the per-step kernel (csrc/rnn_step.hip) -- one chain of 128 roundings was 2.5 to 3 times its error against float64
      float gh[G][16];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        f32x16 acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(hs[(64 * hb + 16 * j + i) * LDR + l32], w[g][16 * j + i], acc[j], 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          float v = ((acc[0][e] + acc[1][e]) + (acc[2][e] + acc[3][e])) + bv[g];
          asm volatile("" : "+v"(v));   // (summed HERE: sunk to the cell, the accumulators of all gates would be live at once)
          if constexpr (KIND) p[g][e] += v;   // the LSTM's summed pre-activation
          else gh[g][e] = v;
        }
      }
      // the cell, a row at a time: what a row produces leaves for HBM (and the other LDS buffer) before the next row is computed
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const bool ok = row_ok(e, hb, nv), z = (rs >> e) & 1;
        float* gp = a.pre + (base + rc_of(e)) * G * H;   // row e of the tile in step c, the same in every lane
        const long o1 = (base + rc_of(e)) * H, o1n = o1 + N * H;
        float hn;
        if constexpr (KIND) {
          const auto o = rnn_cell::lstm_fwd<Gates>(p[0][e], p[1][e], p[2][e], p[3][e], st[e]);
          st[e] = z ? 0.f : o.c;
          hn = z ? 0.f : o.h;
          if (ok) {
            gp[vg] = o.i; (gp + H)[vg] = o.f; (gp + 2 * H)[vg] = o.g; (gp + 3 * H)[vg] = o.o;
            (a.cnew + o1)[vh] = o.c;
            (a.y + o1)[vh] = o.h;
            if (nxt) (a.cin + o1n)[vh] = st[e];
          }
        } else {
          const auto o = rnn_cell::gru_fwd<Gates>(p[0][e], p[1][e], p[2][e], gh[0][e], gh[1][e], gh[2][e], st[e]);
          hn = st[e] = z ? 0.f : o.h;
          if (ok) {
            float* hp = a.gh + (base + rc_of(e)) * 3 * H;
            gp[vg] = o.r; (gp + H)[vg] = o.z; (gp + 2 * H)[vg] = o.n;
            hp[vg] = gh[0][e]; (hp + H)[vg] = gh[1][e]; (hp + 2 * H)[vg] = gh[2][e];
            (a.y + o1)[vh] = o.h;
          }
        }
        if (nxt) {
          if (ok) (a.hin + o1n)[vh] = hn;
          hd[unit * LDR + row_of(e, hb)] = hn;
        }
      }
      __syncthreads();   // the step's one barrier: the other buffer is written, this one is read
    }
  }
}

// what the cell backward of a step reads, for this lane's unit and 16 rows
template <int KIND>
struct BwdIn {
  float dy[16], g[KIND ? 4 : 3][16];
  float x0[16];   // LSTM: c' as the forward stored it; GRU: the n part of gh
  float x1[16];   // LSTM: c_in; GRU: h_in
};
template <int KIND>
__device__ __forceinline__ void bwd_load(const WseqArgs& a, int c, long row0, int unit, int hb, int nv, BwdIn<KIND>& v) {
  constexpr int G = KIND ? 4 : 3;
  const unsigned vg = 4u * hb * G * H + unit, vh = 4u * hb * H + unit;
  const long base = (long)c * a.N + row0;
  if (a.dy) {
    col_load(a.dy + base * a.ld_dy, a.ld_dy, 4u * hb * (unsigned)a.ld_dy + unit, hb, nv, v.dy);
  } else {
#pragma unroll
    for (int e = 0; e < 16; ++e) v.dy[e] = 0.f;
  }
#pragma unroll
  for (int g = 0; g < G; ++g) col_load(a.pre + base * G * H + g * H, G * H, vg, hb, nv, v.g[g]);
  if constexpr (KIND) {
    col_load(a.cnew + base * H, H, vh, hb, nv, v.x0);
    col_load(a.cin + base * H, H, vh, hb, nv, v.x1);
  } else {
    col_load(a.gh + base * 3 * H + 2 * H, 3 * H, vg, hb, nv, v.x0);
    col_load(a.hin + base * H, H, vh, hb, nv, v.x1);
  }
}

template <int KIND>
__global__ __launch_bounds__(256, 1) void rnn_wseq_bwd_kernel(WseqArgs a) {
  constexpr int G = KIND ? 4 : 3, K = G * H;
  extern __shared__ __attribute__((aligned(16))) float sm[];   // [K][LDR]: the tile's d gates of one step, [k][row]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, hb = lane >> 5;
  const int unit = 32 * wave + l32;
  const unsigned vg = 4u * hb * G * H + unit;
  const long N = a.N;
  // B fragments: w[s] = W_hh[(K / 2) hb + s][unit]
  float w[K / 2];
#pragma unroll
  for (int s = 0; s < K / 2; ++s) w[s] = a.w_hh[(long)((K / 2) * hb + s) * H + unit];
  const long ntiles = (N + 31) / 32;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long row0 = tile * 32;
    const int nv = (int)(N - row0 < 32 ? N - row0 : 32);
    float ch[16], cc[16];   // d loss / d (h_in, c_in) of the step after the one at hand
#pragma unroll
    for (int e = 0; e < 16; ++e) ch[e] = cc[e] = 0.f;
    BwdIn<KIND> in;
    bwd_load<KIND>(a, a.C - 1, row0, unit, hb, nv, in);
    for (int c = a.C - 1; c >= 0; --c) {
      const long base = (long)c * N + row0;
      // bit e set: the carry into row_of(e) is cut (the chunk's end, or a reset between this step and the next)
      const unsigned cut = c + 1 == a.C ? 0xffffu : a.reset ? reset_bits(a.reset + base + N, hb, nv) : 0u;
      float d[G][16];   // d pre (LSTM) / d gi (GRU), in place of the gates
      float direct[16];
      if constexpr (KIND) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const bool keep = !((cut >> e) & 1);
          const float dh = in.dy[e] + (keep ? ch[e] : 0.f), dc = keep ? cc[e] : 0.f;
          const auto b = rnn_cell::lstm_bwd<Gates>(dh, dc, in.g[0][e], in.g[1][e], in.g[2][e], in.g[3][e], in.x1[e], in.x0[e]);
          d[0][e] = b.d_i; d[1][e] = b.d_f; d[2][e] = b.d_g; d[3][e] = b.d_o;
          cc[e] = b.dc_in;
          direct[e] = 0.f;
        }
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int e = 0; e < 16; ++e) sm[(g * H + unit) * LDR + row_of(e, hb)] = d[g][e];
      } else {
        float q[3][16];   // d gh: what multiplies W_hh
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float dh = in.dy[e] + ((cut >> e) & 1 ? 0.f : ch[e]);
          const auto b = rnn_cell::gru_bwd(dh, in.g[0][e], in.g[1][e], in.g[2][e], in.x0[e], in.x1[e]);
          d[0][e] = b.d_r; d[1][e] = b.d_z; d[2][e] = b.d_n;
          q[0][e] = b.d_r; q[1][e] = b.d_z; q[2][e] = b.d_gh_n;
          direct[e] = b.direct;   // the part of d h_in that does not go through W_hh
        }
#pragma unroll
        for (int g = 0; g < 3; ++g) {
          col_store(a.gh + base * 3 * H + g * H, 3 * H, vg, hb, nv, q[g]);
#pragma unroll
          for (int e = 0; e < 16; ++e) sm[(g * H + unit) * LDR + row_of(e, hb)] = q[g][e];
        }
      }
#pragma unroll
      for (int g = 0; g < G; ++g) col_store(a.pre + base * G * H + g * H, G * H, vg, hb, nv, d[g]);
      __syncthreads();   // the step's d gates are in LDS
      if (c > 0) bwd_load<KIND>(a, c - 1, row0, unit, hb, nv, in);   // on its way while the matrix cores run
      // d h_in(c)[row][unit] = (GRU: direct +) sum over the gate columns k of d gates[row][k] W_hh[k][unit]
      // (k in four chains of K / 8 MFMA steps, as in the forward; one after the other, so that one accumulator and the running sum
      // are all that is live beside the weights and the next step's operands)
      float sum[16];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
        for (int i = 0; i < K / 8; ++i)
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sm[((K / 2) * hb + (K / 8) * j + i) * LDR + l32], w[(K / 8) * j + i], acc, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          sum[e] = j ? sum[e] + acc[e] : acc[e];
          asm volatile("" : "+v"(sum[e]));   // (added HERE, not after the last chain)
        }
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) ch[e] = direct[e] + sum[e];
      __syncthreads();   // ... and read: the next step may overwrite them
    }
  }
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

template <int KIND>
void launch_wseq(void* stream, const WseqArgs& a, bool bwd) {
  constexpr int G = KIND ? 4 : 3;
  const long tiles = srl_ceil_div(a.N, 32L), cus = num_cus();
  const unsigned grid = (unsigned)(tiles < cus ? tiles : cus);
  const int lds = (int)sizeof(float) * LDR * (bwd ? G * H : 2 * H);
  auto kern = bwd ? rnn_wseq_bwd_kernel<KIND> : rnn_wseq_fwd_kernel<KIND>;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, (hipStream_t)stream, a);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int srl_rnn_wseq_supported(int kind, int H_) { return (kind == 0 || kind == 1) && H_ == H; }

extern "C" int srl_lstm_wseq_fwd(void* stream, float* pre, const float* w_hh, const float* b_hh, float* hin, float* cin,
                                 const uint8_t* reset, int64_t N, int H_, int C, float* y, float* cnew) {
  SRL_CHECK_ARG(srl_rnn_wseq_supported(1, H_) && N >= 0 && C >= 1, "H must be 128");
  SRL_CHECK_ARG(pre && w_hh && hin && cin && y && cnew, "null tensor");
  SRL_CHECK_ARG(aligned16(w_hh), "w_hh must be 16-byte aligned");
  if (N == 0) return 0;
  WseqArgs a{};
  a.pre = pre; a.w_hh = w_hh; a.b_hh = b_hh; a.hin = hin; a.cin = cin; a.reset = reset; a.N = N; a.C = C; a.y = y; a.cnew = cnew;
  launch_wseq<1>(stream, a, false);
  SRL_LAUNCH_CHECK();
  return 0;
}

extern "C" int srl_lstm_wseq_bwd(void* stream, const float* dy, int64_t ld_dy, float* gates, const float* w_hh, const float* cin,
                                 const float* cnew, const uint8_t* reset, int64_t N, int H_, int C) {
  SRL_CHECK_ARG(srl_rnn_wseq_supported(1, H_) && N >= 0 && C >= 1, "H must be 128");
  SRL_CHECK_ARG(gates && w_hh && cin && cnew && (!dy || (ld_dy >= H_ && ld_dy < (1 << 24))), "null tensor");
  if (N == 0) return 0;
  WseqArgs a{};
  a.pre = gates; a.w_hh = w_hh; a.cin = const_cast<float*>(cin); a.cnew = const_cast<float*>(cnew); a.reset = reset; a.dy = dy;
  a.ld_dy = ld_dy; a.N = N; a.C = C;
  launch_wseq<1>(stream, a, true);
  SRL_LAUNCH_CHECK();
  return 0;
}

extern "C" int srl_gru_wseq_fwd(void* stream, float* gi, float* gh, const float* w_hh, const float* b_hh, float* hin,
                                const uint8_t* reset, int64_t N, int H_, int C, float* y) {
  SRL_CHECK_ARG(srl_rnn_wseq_supported(0, H_) && N >= 0 && C >= 1, "H must be 128");
  SRL_CHECK_ARG(gi && gh && w_hh && hin && y, "null tensor");
  SRL_CHECK_ARG(aligned16(w_hh), "w_hh must be 16-byte aligned");
  if (N == 0) return 0;
  WseqArgs a{};
  a.pre = gi; a.gh = gh; a.w_hh = w_hh; a.b_hh = b_hh; a.hin = hin; a.reset = reset; a.N = N; a.C = C; a.y = y;
  launch_wseq<0>(stream, a, false);
  SRL_LAUNCH_CHECK();
  return 0;
}

extern "C" int srl_gru_wseq_bwd(void* stream, const float* dy, int64_t ld_dy, float* gates, float* gh, const float* w_hh,
                                const float* hin, const uint8_t* reset, int64_t N, int H_, int C) {
  SRL_CHECK_ARG(srl_rnn_wseq_supported(0, H_) && N >= 0 && C >= 1, "H must be 128");
  SRL_CHECK_ARG(gates && gh && w_hh && hin && (!dy || (ld_dy >= H_ && ld_dy < (1 << 24))), "null tensor");
  if (N == 0) return 0;
  WseqArgs a{};
  a.pre = gates; a.gh = gh; a.w_hh = w_hh; a.hin = const_cast<float*>(hin); a.reset = reset; a.dy = dy; a.ld_dy = ld_dy; a.N = N;
  a.C = C;
  launch_wseq<0>(stream, a, true);
  SRL_LAUNCH_CHECK();
  return 0;
}
