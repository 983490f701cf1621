// One time step of the auto-reset GRU / LSTM at the wide widths (H a multiple of 16, at least 128) in ONE launch: what srl_gemm
// (W_hh h + b_hh) followed by srl_gru_cell_fwd / srl_lstm_cell_fwd (csrc/gru.hip) do in two.  csrc/rnn_seq.hip runs a whole
// chunk in one launch, but only where W_hh fits a workgroup's LDS (H in {32, 64}); at H = 512 (the recurrent atari-dqn agent)
// every step of the host's time loop was a GEMM plus a cell launch.
//
// A workgroup (4 wavefronts) owns 16 hidden units across all gates, for a tile of 16 or 32 columns (rows of the [N, .] buffers).
// Its slice of W_hh h is formed on the float32 matrix cores (v_mfma_f32_16x16x4_f32: an exact fmaf chain) with W_hh as the A
// operand (lane l: unit l & 15) and h as the B operand (lane l: column l & 15), so the accumulator of lane l holds units
// 4 (l >> 4) + {0..3} of column l & 15 -- all gates of a unit in the same lane and register, the cell is lane-local, and the
// four values are contiguous in every [N, H] buffer.  The reduction over k is split between the wavefronts in blocks of 16
// (block c goes to wavefront c % 4; within a block lane group q = l >> 4 takes k = 16 c + 4 q + j in MFMA j, for both operands,
// so each lane loads 16 bytes of a row at a time); the four partial sums meet in LDS in a fixed order, the first wavefront(s)
// add b_hh, apply the cell csrc/gru.hip applies (csrc/rnn_cell.h, libm gates) and write y, the masked next state and the saved
// gates -- gi / pre and gh come out as the two-launch path leaves them, so the per-step backward runs unchanged.
//
// No workgroup reads what another writes in the same launch (hin_t / cin_t are read-only here and must not alias hin_next /
// cin_next; gi, gh, pre are read and written only at the workgroup's own units and columns); there is no grid-wide barrier,
// no cooperative launch and no flag in memory; every store is an ordinary vector store.
//
// The backward step (srl_gru_step_bwd / srl_lstm_step_bwd, rnn_step_bwd_kernel) is the same split turned round, fused ACROSS the
// step boundary: the launch for step t first forms D = d gates(t+1) . W_hh -- the product the two-launch path runs as srl_gemm
// after the cell of step t+1 -- for its 16 units and 16 or 32 rows, then runs the cell backward of step t (csrc/rnn_cell.h) on
// them.  (The cell of step t followed by ITS product would not do: the product needs d gates of all G H columns of a row, which
// other workgroups are writing in place.)  d gates(t+1) [N, G H] is the B operand (lane l: row l & 15, 16 bytes of k) and
// W_hh, read as it lies, the A operand: row k of [G H, H] holds the workgroup's 16 units contiguously, so lane l takes
// W_hh[16 b + 4 q + j][u0 + (l & 15)] for MFMA j as a scalar dword and the 16 lanes of a group q read 64 contiguous bytes.  The
// accumulator layout is the forward's -- lane l: units 4 (l >> 4) + {0..3} of row l & 15 -- so the cell is lane-local and every
// [N, H] access 16 bytes.  K = G H is dealt in blocks of 16, block b to wavefront b % 4; a wavefront keeps four blocks in flight
// (their loads issued a group ahead, under the previous group's MFMAs), each summed in an accumulator of its own: a K of 1536
// behind one launch boundary is latency, and 16 short chains round less than 4 long ones.  The chains are added in a fixed
// order, the four partial sums meet in LDS (4 KB per 16 rows) in a fixed order, and wavefront t applies the cell to row tile t,
// on operands it asked for before the product.  GRU: dh = dy + (direct(t+1) + D) (1 - reset(t+1)); gi <- d gi, gh <- d gh,
// direct(t) = dh z.  LSTM: dh = dy + D (1 - reset), dc = dc_in(t+1) (1 - reset); pre <- d pre, dc_in(t) written.  A chunk's last
// step has no successor (null next-step pointers): no product, the cell only.  d h_in of step 0 is never formed.
// No workgroup reads what another writes here either: d gates(t+1) and the carry of step t+1 were finished by the previous launch
// and are read-only (they must not alias the buffers of step t); gates, gh and the carry of step t are read and written at the
// workgroup's own units and rows only.  No grid barrier, no cooperative launch, no flag in memory, ordinary vector stores.
// As compiled (VGPRs + AGPRs a lane, scratch, LDS): GRU 16 rows 224 + 16, 0 B, 4096 B; GRU 32 rows 256 + 42, 0 B, 8192 B;
// LSTM 16 rows 166 + 16, 0 B, 4096 B; LSTM 32 rows 198 + 32, 0 B, 8192 B (-Rpass-analysis=kernel-resource-usage prints them).
#include "rnn_cell.h"
#include "srl_common.h"

namespace {

using f4 = __attribute__((ext_vector_type(4))) float;

using rnn_cell::LibmGates;
__device__ __forceinline__ f4 ld4(const float* p) { return *reinterpret_cast<const f4*>(p); }
__device__ __forceinline__ void st4(float* p, f4 v) { *reinterpret_cast<f4*>(p) = v; }

struct StepArgs {
  float* g0;             // GRU: gi_t [N, 3H]; LSTM: pre_t [N, 4H]
  float* gh;             // GRU: gh_t [N, 3H]
  const float* w_hh;     // [G H, H]
  const float* b_hh;     // [G H] or null
  const float* hin;      // [N, H]
  const float* cin;      // LSTM: [N, H]
  const uint8_t* reset_next;
  long N;
  int H;
  float* y;
  float* cnew;
  float* hin_next;
  float* cin_next;
};

// G gates (3 GRU, 4 LSTM), CT column tiles of 16 per workgroup.  grid = (H / 16, ceil(N / (16 CT))).
template <int G, int CT>
__global__ __launch_bounds__(256) void rnn_step_kernel(StepArgs a) {
  __shared__ f4 red[4][G][CT][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, q = lane >> 4;
  const int H = a.H, u0 = blockIdx.x * 16;
  const long N = a.N, tiles = (N + 16 * CT - 1) / (16 * CT);
  for (long tile = blockIdx.y; tile < tiles; tile += gridDim.y) {   // (one pass unless N exceeds 65 535 tiles)
  const long n0 = tile * (16 * CT);
  const float* wrow[G];
#pragma unroll
  for (int g = 0; g < G; ++g) wrow[g] = a.w_hh + ((long)g * H + u0 + lr) * H + 4 * q;
  const float* hrow[CT];
#pragma unroll
  for (int t = 0; t < CT; ++t) {
    long n = n0 + 16 * t + lr;
    if (n >= N) n = N - 1;   // a ragged tile reads the last row again; its results are not written
    hrow[t] = a.hin + n * H + 4 * q;
  }
  f4 acc[G][CT];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int t = 0; t < CT; ++t) acc[g][t] = f4{0.f, 0.f, 0.f, 0.f};
  const int blocks = H / 16;
  f4 wf[G], hf[CT];
  int c = wave;
  if (c < blocks) {
#pragma unroll
    for (int g = 0; g < G; ++g) wf[g] = ld4(wrow[g] + 16 * c);
#pragma unroll
    for (int t = 0; t < CT; ++t) hf[t] = ld4(hrow[t] + 16 * c);
  }
  for (; c < blocks; c += 4) {
    f4 wn[G], hn[CT];
    const int cn = c + 4 < blocks ? c + 4 : c;   // (the last block is loaded twice rather than branching around the loads)
#pragma unroll
    for (int g = 0; g < G; ++g) wn[g] = ld4(wrow[g] + 16 * cn);
#pragma unroll
    for (int t = 0; t < CT; ++t) hn[t] = ld4(hrow[t] + 16 * cn);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int t = 0; t < CT; ++t) acc[g][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[g][j], hf[t][j], acc[g][t], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < G; ++g) wf[g] = wn[g];
#pragma unroll
    for (int t = 0; t < CT; ++t) hf[t] = hn[t];
  }
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int t = 0; t < CT; ++t) red[wave][g][t][lane] = acc[g][t];
  __syncthreads();
  const int t = wave;
  const long n = n0 + 16 * t + lr;
  if (wave < CT && n < N) {
  const int u = u0 + 4 * q;   // this lane's four units
  f4 s[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    s[g] = (red[0][g][t][lane] + red[1][g][t][lane]) + (red[2][g][t][lane] + red[3][g][t][lane]);
    if (a.b_hh) s[g] += ld4(a.b_hh + g * H + u);
  }
  const bool rs = a.reset_next && a.reset_next[n];
  const f4 zero = f4{0.f, 0.f, 0.f, 0.f};
  if constexpr (G == 3) {
    float* gi = a.g0 + n * 3 * H + u;
    float* gh = a.gh + n * 3 * H + u;
    const f4 ir = ld4(gi), iz = ld4(gi + H), in = ld4(gi + 2 * H), hp = ld4(a.hin + n * H + u);
    f4 r, z, nn, h;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const auto o = rnn_cell::gru_fwd<LibmGates>(ir[e], iz[e], in[e], s[0][e], s[1][e], s[2][e], hp[e]);
      r[e] = o.r, z[e] = o.z, nn[e] = o.n, h[e] = o.h;
    }
    st4(gi, r), st4(gi + H, z), st4(gi + 2 * H, nn);       // saved for the backward pass
    st4(gh, s[0]), st4(gh + H, s[1]), st4(gh + 2 * H, s[2]);
    st4(a.y + n * H + u, h);
    if (a.hin_next) st4(a.hin_next + n * H + u, rs ? zero : h);
  } else {
    float* p = a.g0 + n * 4 * H + u;
    const f4 cp = ld4(a.cin + n * H + u);
    const f4 pi = ld4(p), pf = ld4(p + H), pg = ld4(p + 2 * H), po = ld4(p + 3 * H);
    f4 gi, gf, gg, go, c2, h;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const auto o = rnn_cell::lstm_fwd<LibmGates>(pi[e] + s[0][e], pf[e] + s[1][e], pg[e] + s[2][e], po[e] + s[3][e], cp[e]);
      gi[e] = o.i, gf[e] = o.f, gg[e] = o.g, go[e] = o.o, c2[e] = o.c, h[e] = o.h;
    }
    st4(p, gi), st4(p + H, gf), st4(p + 2 * H, gg), st4(p + 3 * H, go);
    st4(a.y + n * H + u, h);
    st4(a.cnew + n * H + u, c2);
    if (a.hin_next) {
      st4(a.hin_next + n * H + u, rs ? zero : h);
      st4(a.cin_next + n * H + u, rs ? zero : c2);
    }
  }
  }
  __syncthreads();   // the partial sums are read: the next tile may overwrite them
  }
}

struct StepBwdArgs {
  const float* dy;          // [N, ld_dy] or null (zeros)
  long ld_dy;
  const float* dg_next;     // GRU: d gh(t+1) [N, 3H]; LSTM: d pre(t+1) [N, 4H]; null at a chunk's last step
  const float* carry_next;  // GRU: direct(t+1); LSTM: dc_in(t+1)   [N, H]
  const uint8_t* reset_next;
  const float* w_hh;        // [G H, H]
  float* g0;                // GRU: gates_t -> d gi; LSTM: gates_t -> d pre
  float* gh;                // GRU: gh_t -> d gh
  const float* s0;          // GRU: hin_t; LSTM: cin_t
  const float* s1;          // LSTM: cnew_t
  long N;
  int H;
  float* carry;             // GRU: direct_t; LSTM: dc_in_t
};

constexpr int BU = 4;   // k-blocks a wavefront has in flight, each with an accumulator of its own

// The fragments of BU k-blocks (b, b + 4, ...) of one wavefront: W_hh[16 b + 4 q + j][u0 + lr] as scalar dwords (the 16 lanes of a
// group q read 64 contiguous bytes of row k), d gates[row][16 b + 4 q ..+ 4] as 16 bytes.  A block from `blocks` on contributes
// zeros and loads nothing.
template <int CT>
struct BwdFrag {
  float w[BU][4];
  f4 d[BU][CT];
  __device__ __forceinline__ void load(const float* wcol, const float* const (&drow)[CT], int b, int blocks, int H) {
#pragma unroll
    for (int u = 0; u < BU; ++u) {
      const int bb = b + 4 * u;   // (wavefront-uniform)
      if (bb < blocks) {
#pragma unroll
        for (int j = 0; j < 4; ++j) w[u][j] = wcol[(long)(16 * bb + j) * H];
#pragma unroll
        for (int t = 0; t < CT; ++t) d[u][t] = ld4(drow[t] + 16 * bb);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) w[u][j] = 0.f;
#pragma unroll
        for (int t = 0; t < CT; ++t) d[u][t] = f4{0.f, 0.f, 0.f, 0.f};
      }
    }
  }
};

// The cell arithmetic beside the MFMAs stays on unpacked float32 ops (what the Makefile asks of rnn_wseq.hip for the whole file;
// here per kernel, so that the forward above compiles to what it always has).
#ifdef __HIP_DEVICE_COMPILE__
#define SRL_UNPACKED_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define SRL_UNPACKED_F32
#endif

// The backward step.  G gates, CT row tiles of 16 per workgroup, grid as rnn_step_kernel's.
template <int G, int CT>
__global__ __launch_bounds__(256) SRL_UNPACKED_F32 void rnn_step_bwd_kernel(StepBwdArgs a) {
  __shared__ f4 red[4][CT][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, q = lane >> 4;
  const int H = a.H, u0 = blockIdx.x * 16, K = G * H, blocks = K / 16;
  const long N = a.N, tiles = (N + 16 * CT - 1) / (16 * CT);
  const f4 zero = f4{0.f, 0.f, 0.f, 0.f};
  for (long tile = blockIdx.y; tile < tiles; tile += gridDim.y) {
  const long n0 = tile * (16 * CT);
  // The cell's operands (this lane's row of tile `wave`, its four units) are asked for first: they arrive under the product.
  const int t = wave, u = u0 + 4 * q;
  const long n = n0 + 16 * t + lr, i = n * H + u;
  const bool mine = wave < CT && n < N;
  const bool cut = !a.dg_next || (mine && a.reset_next && a.reset_next[n]);   // nothing arrives from a step that began reset
  float* const g = a.g0 + n * G * H + u;
  float* const p = G == 3 ? a.gh + n * G * H + u : nullptr;
  f4 op[6], dh = zero, cn = zero;   // cn: GRU direct(t+1), LSTM dc_in(t+1)
  if (mine) {
    if (a.dy) dh = ld4(a.dy + n * a.ld_dy + u);
    if (!cut) cn = ld4(a.carry_next + i);
#pragma unroll
    for (int e = 0; e < G; ++e) op[e] = ld4(g + e * H);   // r z n | i f g o
    if constexpr (G == 3) op[3] = ld4(p + 2 * H), op[4] = ld4(a.s0 + i);   // gh_n, h_in
    else op[4] = ld4(a.s0 + i), op[5] = ld4(a.s1 + i);                     // c_in, c'
  }
  if (a.dg_next) {   // (grid-uniform) D = d gates(t+1) . W_hh for this workgroup's 16 units and 16 CT rows
    const float* wcol = a.w_hh + (long)(4 * q) * H + u0 + lr;
    const float* drow[CT];
#pragma unroll
    for (int tt = 0; tt < CT; ++tt) {
      long nr = n0 + 16 * tt + lr;
      if (nr >= N) nr = N - 1;   // a ragged tile reads the last row again; its results are not written
      drow[tt] = a.dg_next + nr * K + 4 * q;
    }
    f4 acc[BU][CT];
#pragma unroll
    for (int b = 0; b < BU; ++b)
#pragma unroll
      for (int tt = 0; tt < CT; ++tt) acc[b][tt] = zero;
    BwdFrag<CT> cur, nxt;
    cur.load(wcol, drow, wave, blocks, H);
    for (int b = wave; b < blocks; b += 4 * BU) {
      nxt.load(wcol, drow, b + 4 * BU, blocks, H);   // in flight under this group's MFMAs
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int x = 0; x < BU; ++x)
#pragma unroll
          for (int tt = 0; tt < CT; ++tt)
            acc[x][tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.w[x][j], cur.d[x][tt][j], acc[x][tt], 0, 0, 0);
      cur = nxt;
    }
#pragma unroll
    for (int tt = 0; tt < CT; ++tt) red[wave][tt][lane] = (acc[0][tt] + acc[1][tt]) + (acc[2][tt] + acc[3][tt]);
    __syncthreads();
  }
  if (mine) {
    if (!cut) {
      const f4 D = (red[0][t][lane] + red[1][t][lane]) + (red[2][t][lane] + red[3][t][lane]);
      if constexpr (G == 3) dh += cn + D;   // d h_in(t+1) = direct(t+1) + d gh(t+1) . W_hh
      else dh += D;
    }
    if constexpr (G == 3) {
      f4 dr, dz, dn, dhn, direct;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const auto o = rnn_cell::gru_bwd(dh[e], op[0][e], op[1][e], op[2][e], op[3][e], op[4][e]);
        dr[e] = o.d_r, dz[e] = o.d_z, dn[e] = o.d_n, dhn[e] = o.d_gh_n, direct[e] = o.direct;
      }
      st4(g, dr), st4(g + H, dz), st4(g + 2 * H, dn);    // d gi
      st4(p, dr), st4(p + H, dz), st4(p + 2 * H, dhn);   // d gh
      st4(a.carry + i, direct);
    } else {
      f4 di, df, dg, d_o, dc;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const auto o = rnn_cell::lstm_bwd<LibmGates>(dh[e], cn[e], op[0][e], op[1][e], op[2][e], op[3][e], op[4][e], op[5][e]);
        di[e] = o.d_i, df[e] = o.d_f, dg[e] = o.d_g, d_o[e] = o.d_o, dc[e] = o.dc_in;
      }
      st4(g, di), st4(g + H, df), st4(g + 2 * H, dg), st4(g + 3 * H, d_o);
      st4(a.carry + i, dc);
    }
  }
  __syncthreads();   // the partial sums are read: the next tile may overwrite them
  }
}

// 32 columns per workgroup once that still gives every compute unit a workgroup; 16 below (N ~ 100 at H = 512: 256 workgroups)
inline bool two_tiles(long N, int H) { return srl_ceil_div(N, 32L) * (H / 16) >= 256; }

template <int G>
int launch(void* stream, const StepArgs& a) {
  const bool two = two_tiles(a.N, a.H);
  const long tiles = srl_ceil_div(a.N, two ? 32L : 16L);
  dim3 grid((unsigned)(a.H / 16), (unsigned)(tiles < 65535 ? tiles : 65535));
  if (two) hipLaunchKernelGGL((rnn_step_kernel<G, 2>), grid, dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((rnn_step_kernel<G, 1>), grid, dim3(256), 0, (hipStream_t)stream, a);
  return 0;
}

template <int G>
int launch_bwd(void* stream, const StepBwdArgs& a) {
  const bool two = two_tiles(a.N, a.H);   // the forward's rule
  const long tiles = srl_ceil_div(a.N, two ? 32L : 16L);
  dim3 grid((unsigned)(a.H / 16), (unsigned)(tiles < 65535 ? tiles : 65535));
  if (two) hipLaunchKernelGGL((rnn_step_bwd_kernel<G, 2>), grid, dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((rnn_step_bwd_kernel<G, 1>), grid, dim3(256), 0, (hipStream_t)stream, a);
  return 0;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int srl_rnn_step_supported(int kind, int H) { return (kind == 0 || kind == 1) && H >= 128 && H % 16 == 0; }

extern "C" int srl_gru_step_fwd(void* stream, float* gi_t, float* gh_t, const float* w_hh, const float* b_hh, const float* hin_t,
                                const uint8_t* reset_next, int64_t N, int H, float* y_t, float* hin_next) {
  SRL_CHECK_ARG(srl_rnn_step_supported(0, H) && N >= 0, "H must be a multiple of 16, at least 128");
  if (N == 0) return 0;
  SRL_CHECK_ARG(gi_t && gh_t && w_hh && hin_t && y_t, "null tensor");
  SRL_CHECK_ARG(hin_next != hin_t && y_t != hin_t, "hin_t is read by every workgroup: it must not be an output");
  SRL_CHECK_ARG(aligned16(gi_t) && aligned16(gh_t) && aligned16(w_hh) && aligned16(b_hh) && aligned16(hin_t) && aligned16(y_t) &&
                    aligned16(hin_next), "tensors must be 16-byte aligned");
  StepArgs a{gi_t, gh_t, w_hh, b_hh, hin_t, nullptr, reset_next, (long)N, H, y_t, nullptr, hin_next, nullptr};
  launch<3>(stream, a);
  SRL_LAUNCH_CHECK();
  return 0;
}

extern "C" int srl_lstm_step_fwd(void* stream, float* pre_t, const float* w_hh, const float* b_hh, const float* hin_t,
                                 const float* cin_t, const uint8_t* reset_next, int64_t N, int H, float* y_t, float* cnew_t,
                                 float* hin_next, float* cin_next) {
  SRL_CHECK_ARG(srl_rnn_step_supported(1, H) && N >= 0, "H must be a multiple of 16, at least 128");
  if (N == 0) return 0;
  SRL_CHECK_ARG(pre_t && w_hh && hin_t && cin_t && y_t && cnew_t && (!hin_next == !cin_next), "null tensor");
  SRL_CHECK_ARG(hin_next != hin_t && y_t != hin_t, "hin_t is read by every workgroup: it must not be an output");
  SRL_CHECK_ARG(aligned16(pre_t) && aligned16(w_hh) && aligned16(b_hh) && aligned16(hin_t) && aligned16(cin_t) && aligned16(y_t) &&
                    aligned16(cnew_t) && aligned16(hin_next) && aligned16(cin_next), "tensors must be 16-byte aligned");
  StepArgs a{pre_t, nullptr, w_hh, b_hh, hin_t, cin_t, reset_next, (long)N, H, y_t, cnew_t, hin_next, cin_next};
  launch<4>(stream, a);
  SRL_LAUNCH_CHECK();
  return 0;
}

extern "C" int srl_gru_step_bwd(void* stream, const float* dy_t, int64_t ld_dy, const float* dgh_next, const float* direct_next,
                                const uint8_t* reset_next, const float* w_hh, float* gates_t, float* gh_t, const float* hin_t,
                                int64_t N, int H, float* direct_t) {
  SRL_CHECK_ARG(srl_rnn_step_supported(0, H) && N >= 0, "H must be a multiple of 16, at least 128");
  if (N == 0) return 0;
  SRL_CHECK_ARG(gates_t && gh_t && hin_t && direct_t && w_hh, "null tensor");
  SRL_CHECK_ARG(!dgh_next == !direct_next && (dgh_next || !reset_next), "the next step's d gh and direct: both or neither");
  SRL_CHECK_ARG(!dy_t || (ld_dy >= H && ld_dy % 4 == 0), "ld_dy must be at least H and a multiple of 4");
  SRL_CHECK_ARG(dgh_next != gh_t && dgh_next != gates_t && direct_next != direct_t,
                "the next step's d gh and direct are read by every workgroup: they must not be outputs");
  SRL_CHECK_ARG(aligned16(dy_t) && aligned16(dgh_next) && aligned16(direct_next) && aligned16(w_hh) && aligned16(gates_t) &&
                    aligned16(gh_t) && aligned16(hin_t) && aligned16(direct_t), "tensors must be 16-byte aligned");
  StepBwdArgs a{dy_t, (long)ld_dy, dgh_next, direct_next, reset_next, w_hh, gates_t, gh_t, hin_t, nullptr, (long)N, H, direct_t};
  launch_bwd<3>(stream, a);
  SRL_LAUNCH_CHECK();
  return 0;
}

extern "C" int srl_lstm_step_bwd(void* stream, const float* dy_t, int64_t ld_dy, const float* dpre_next, const float* dc_next,
                                 const uint8_t* reset_next, const float* w_hh, float* gates_t, const float* cin_t,
                                 const float* cnew_t, int64_t N, int H, float* dc_in_t) {
  SRL_CHECK_ARG(srl_rnn_step_supported(1, H) && N >= 0, "H must be a multiple of 16, at least 128");
  if (N == 0) return 0;
  SRL_CHECK_ARG(gates_t && cin_t && cnew_t && dc_in_t && w_hh, "null tensor");
  SRL_CHECK_ARG(!dpre_next == !dc_next && (dpre_next || !reset_next), "the next step's d pre and dc_in: both or neither");
  SRL_CHECK_ARG(!dy_t || (ld_dy >= H && ld_dy % 4 == 0), "ld_dy must be at least H and a multiple of 4");
  SRL_CHECK_ARG(dpre_next != gates_t && dc_next != dc_in_t,
                "the next step's d pre and dc_in are read by every workgroup: they must not be outputs");
  SRL_CHECK_ARG(aligned16(dy_t) && aligned16(dpre_next) && aligned16(dc_next) && aligned16(w_hh) && aligned16(gates_t) &&
                    aligned16(cin_t) && aligned16(cnew_t) && aligned16(dc_in_t), "tensors must be 16-byte aligned");
  StepBwdArgs a{dy_t, (long)ld_dy, dpre_next, dc_next, reset_next, w_hh, gates_t, nullptr, cin_t, cnew_t, (long)N, H, dc_in_t};
  launch_bwd<4>(stream, a);
  SRL_LAUNCH_CHECK();
  return 0;
}
