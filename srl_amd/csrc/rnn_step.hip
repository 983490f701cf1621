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

template <int G>
int launch(void* stream, const StepArgs& a) {
  // 32 columns per workgroup once that still gives every compute unit a workgroup; 16 below (N ~ 100 at H = 512: 256 workgroups)
  const long wide = srl_ceil_div(a.N, 32L) * (a.H / 16);
  const bool two = wide >= 256;
  const long tiles = srl_ceil_div(a.N, two ? 32L : 16L);
  dim3 grid((unsigned)(a.H / 16), (unsigned)(tiles < 65535 ? tiles : 65535));
  if (two) hipLaunchKernelGGL((rnn_step_kernel<G, 2>), grid, dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((rnn_step_kernel<G, 1>), grid, dim3(256), 0, (hipStream_t)stream, a);
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
