// LinF16: the Linear policy of mlp_sig.h's shape kernels on the 16-bit matrix pipe (round 6): every Linear layer of the chain as
// THREE products of f16 pieces (h1 h0' + h0 h1' + h0 h0', v_mfma_f32_32x32x16_f16) instead of sixteen float32 MFMAs per
// 32 x 32 x 32 block -- 96 matrix cycles where the float32 instructions take 512 (of the backward launch's 434 us, 212
// were its float32 MFMAs).  The walk of the chain -- a wavefront owns 32 rows and keeps them in registers through the chain, the
// accumulator layout is the next layer's operand layout -- the LayerNorm layers, the flush and the launches are mlp_sig.h's; this
// file holds what a Linear layer does differently from LinF32:
//   * the weights sit in LDS as two f16 pieces under ONE power-of-two scale per layer (max |w| -> [2^13, 2^14)): per 32 x 32 block
//     and piece 32 rows (out channel) of 64 bytes = the block's 32 k-values as four 16-byte chunks (chunk 2 s + g holds what lane
//     half g supplies to k-step s: channels 16 s + 4 g + {0..3, 8..11}), chunk index XOR ((row >> 2) & 3).  The forward product reads
//     a fragment with one conflict-free ds_read_b128; the data gradient reads the SAME copy transposed (ds_read_b64_tr_b16: four
//     rows x 64 bytes per 32 lanes at a 64-byte pitch is every bank once), so one copy serves both directions as before;
//   * a layer's input rows are split in registers, under a power-of-two scale PER ROW (its largest |value| -> [2^13, 2^14): the
//     contraction runs over channels, so a row's scale leaves with the epilogue): two mixed-precision instructions per element;
//   * bias is added in the epilogue (the accumulator is in scaled units): y = acc / (scale_w scale_row) + b, one fused multiply-add.
// Error of a product against float32: the dropped h1 h1' term and the pieces' rounding, <= 2^-21 of |w| |x| per term (the same
// arithmetic as the Atari encoder's h2 kernels); parity tests as for LinF32.  SRL_MLP_F16=0: the float32 policy (A/B).
// Reference: modules/utils.py:154-161 (mlp), actor_critic_policy.py:92-107 (heads).
#pragma once

namespace {

typedef _Float16 hx_f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 hx_f16x2 __attribute__((ext_vector_type(2)));
typedef short hx_s16x4 __attribute__((ext_vector_type(4)));

constexpr int kHB = 4096;   // bytes of a 32 x 32 weight block: piece 0 | piece 1, 32 rows of 64 bytes each

template <class S>
struct HP {   // LDS plan in bytes
  static constexpr int wb(int i) {
    int f = 0;
    for (int k = 0; k < i; ++k) f += S::kind(k) == 1 ? S::nbo(k) * S::nbi(k) * kHB + S::nbo(k) * 32 * 4 : 2 * S::nbi(k) * 32 * 4;
    return f;
  }
  static constexpr int tb(int i) { return wb(i) + S::nbo(i) * S::nbi(i) * kHB; }   // Linear: bias table; LayerNorm: wb = gamma | beta
  static constexpr int par_bytes = wb(S::n);
  static constexpr int inv = par_bytes;              // [n] floats: 1 / the layer's weight scale
  static constexpr int mx = par_bytes + 4 * S::n;    // [n] ints: max |w| of the layer (staging)
  static constexpr int total = (par_bytes + 8 * S::n + 15) / 16 * 16;
};

constexpr int hx_steps(int dim, int blk) { return (mm_ne(dim, blk) + 7) / 8; }   // k-steps of 16 channels of a 32-channel block

// byte offset of element (row r, k-value kl) of a block's piece plane
__device__ __forceinline__ int hx_welem(int r, int kl) {
  const int s = kl >> 4, kk = kl & 15, run = kk >> 3, g = (kk >> 2) & 1, jj = kk & 3;
  return r * 64 + (((2 * s + g) ^ ((r >> 2) & 3)) << 4) + ((4 * run + jj) << 1);
}

// m >= 0 -> the power of two that takes it into [2^13, 2^14), and its inverse; 0 -> 1
__device__ __forceinline__ void hx_pow2(float m, float& sc, float& inv) {
  int ex;
  (void)frexpf(m, &ex);
  ex = m > 0.f ? ex : 14;
  sc = ldexpf(1.f, 14 - ex);
  inv = ldexpf(1.f, ex - 14);
}

template <int DIM>
__device__ __forceinline__ float hx_lane_max(const float (&v)[kMB][16]) {
  float m = 0.f;
#pragma unroll
  for (int ib = 0; ib < kMB; ++ib)
#pragma unroll
    for (int e = 0; e < 16; ++e)
      if (e < mm_ne(DIM, ib)) m = fmaxf(m, fabsf(v[ib][e]));
  return m;
}

// registers 8 s .. 8 s + 7 of a block (this lane's 8 k-values of step s) as two f16 pieces of v * sc; registers at or beyond NE: zeros
template <int NE>
__device__ __forceinline__ void hx_split8(const float (&v)[16], int s, float sc, hx_f16x8& p0, hx_f16x8& p1) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int e = 8 * s + j;
    if (e < NE) {
      const _Float16 a0 = (_Float16)__builtin_fmaf(v[e], sc, 0.f);
      p0[j] = a0;
      p1[j] = (_Float16)__builtin_fmaf(v[e], sc, -(float)a0);
    } else {
      p0[j] = (_Float16)0.f;
      p1[j] = (_Float16)0.f;
    }
  }
}

__device__ __forceinline__ hx_f16x8 hx_frag(const uint8_t* p) {
  const uint4 q = *reinterpret_cast<const uint4*>(p);
  return __builtin_bit_cast(hx_f16x8, q);
}

// ---- backward: all three products of a Linear layer on f16 pieces ------------------------------------------------------------------
//   * dz (the gradient at the layer's output) is split ONCE per layer and tile under a power-of-two scale of the TILE (the largest
//     |dz| of the wavefront's 32 rows: the weight gradient sums over rows, so a row's own scale would not leave the sum), into
//     packed registers -- the B operand of the data gradient -- and into the wavefront's dz tile in LDS;
//   * data gradient: A = the layer's weights read transposed from the one copy in LDS (two ds_read_b64_tr_b16 per fragment);
//   * weight gradient: the dz and x tiles are rows of 320 bytes (64 channels x piece 0 | piece 1, + 64: four consecutive rows fall
//     into different 64-byte bank windows) with the 8-byte slot index XOR ((row >> 2) & 7) (the 32 rows of a write instruction hit
//     32 different bank pairs); both operands of dW[o][k] = sum_rows dz[row][o] x[row][k] come out through transposing reads.  A
//     tile's product is formed in a FRESH accumulator and folded into the wavefront's persistent block with the tile's scales (one
//     fused multiply-add per accumulator register and tile);
//   * bias gradient: column sums of dz from the weight gradient's own A fragments (v_dot2_f32_f16 against ones), by the wavefronts
//     whose block has in-block 0, kept in a register per layer.
constexpr int kHRow = 320;                 // bytes per row of a piece tile
constexpr int kHTile = 32 * kHRow;         // one operand's tile
constexpr int kHArea = 2 * kHTile;         // a wavefront's tile area: dz | x  (LayerNorm layers use it as two float32 half tiles)
static_assert(kHArea >= 2 * 32 * kTh * 4, "LayerNorm's half tiles fit");

__device__ __forceinline__ hx_s16x4 hx_tr(const uint8_t* p) {
  typedef __attribute__((address_space(3))) hx_s16x4 lds_s16x4;
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p);
}
__device__ __forceinline__ hx_f16x8 hx_tr2(const uint8_t* p0, const uint8_t* p1) {
  union { hx_s16x4 s[2]; hx_f16x8 v; } f;
  f.s[0] = hx_tr(p0);
  f.s[1] = hx_tr(p1);
  return f.v;
}

// largest value of v (>= 0) over the wavefront, in every lane's copy (DPP row shifts and broadcasts, then lane 63)
__device__ __forceinline__ float hx_wave_max(float v) {
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xf, 0xf, true)));   // row_shr:1
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x112, 0xf, 0xf, true)));   // row_shr:2
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x114, 0xf, 0xf, true)));   // row_shr:4
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x118, 0xf, 0xf, true)));   // row_shr:8
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x142, 0xa, 0xf, false)));  // row_bcast:15
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x143, 0xc, 0xf, false)));  // row_bcast:31
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// this lane's registers 8 s .. 8 s + 7 of a block, as pieces, into row r of a piece tile: two runs of four channels per piece
__device__ __forceinline__ void hx_tile_write(uint8_t* T, int r, int hb, int blk, int s, const hx_f16x8& p0, const hx_f16x8& p1) {
  const uint4 q0 = __builtin_bit_cast(uint4, p0), q1 = __builtin_bit_cast(uint4, p1);
  const int x = (r >> 2) & 7;
  uint8_t* row = T + r * kHRow;
  const int sa = 8 * blk + 4 * s + hb, sb = sa + 2;     // 8-byte slots of the two runs inside a piece's 128 bytes
  *reinterpret_cast<uint2*>(row + ((sa ^ x) << 3)) = make_uint2(q0.x, q0.y);
  *reinterpret_cast<uint2*>(row + ((sb ^ x) << 3)) = make_uint2(q0.z, q0.w);
  *reinterpret_cast<uint2*>(row + (((16 + sa) ^ x) << 3)) = make_uint2(q1.x, q1.y);
  *reinterpret_cast<uint2*>(row + (((16 + sb) ^ x) << 3)) = make_uint2(q1.z, q1.w);
}

__device__ __forceinline__ void hx_tile_read(const uint8_t* T, int r, int hb, int blk, int s, hx_f16x8& p0, hx_f16x8& p1) {
  const int x = (r >> 2) & 7;
  const uint8_t* row = T + r * kHRow;
  const int sa = 8 * blk + 4 * s + hb, sb = sa + 2;
  const uint2 a0 = *reinterpret_cast<const uint2*>(row + ((sa ^ x) << 3)), a1 = *reinterpret_cast<const uint2*>(row + ((sb ^ x) << 3));
  const uint2 b0 = *reinterpret_cast<const uint2*>(row + (((16 + sa) ^ x) << 3)), b1 = *reinterpret_cast<const uint2*>(row + (((16 + sb) ^ x) << 3));
  p0 = __builtin_bit_cast(hx_f16x8, make_uint4(a0.x, a0.y, a1.x, a1.y));
  p1 = __builtin_bit_cast(hx_f16x8, make_uint4(b0.x, b0.y, b1.x, b1.y));
}

struct LinF16 {
  static constexpr int kFwdLdsCap = 76 * 1024;           // two workgroups per CU
  static constexpr int kAreaBytes = kHArea;
  static constexpr int kAuxBytes = kBwdWaves * 8;        // tile scales [waves][2]: 1 / dz's scale, 1 / (dz's scale x's scale)
  template <class S>
  static constexpr int par_bytes() { return HP<S>::total; }
  template <class S, int I>
  static __device__ __forceinline__ const float* ln_table(const uint8_t* smb) { return reinterpret_cast<const float*>(smb + HP<S>::wb(I)); }

  template <class S>
  static __device__ __forceinline__ void stage(const XArgs& a, uint8_t* smb, int tid, int nthr) {
    for (int e = tid; e < HP<S>::total / 4; e += nthr) reinterpret_cast<uint32_t*>(smb)[e] = 0u;   // padding of every block and table
    __syncthreads();
    mm_static_for<S::n>([&](auto IC) __attribute__((always_inline)) {
      constexpr int i = decltype(IC)::value;
      if constexpr (S::kind(i) == 1) {
        float m = 0.f;
        for (int idx = tid; idx < S::out(i) * S::in(i); idx += nthr) m = fmaxf(m, fabsf(a.w[i][idx]));
        atomicMax(reinterpret_cast<int*>(smb + HP<S>::mx) + i, __float_as_int(m));
      }
    });
    __syncthreads();
    mm_static_for<S::n>([&](auto IC) __attribute__((always_inline)) {
      constexpr int i = decltype(IC)::value;
      constexpr int in = S::in(i), out = S::out(i);
      const float* w = a.w[i];
      const float* b = a.b[i];
      if constexpr (S::kind(i) == 1) {
        constexpr int nbi = S::nbi(i);
        float sc, isc;
        hx_pow2(__int_as_float(reinterpret_cast<const int*>(smb + HP<S>::mx)[i]), sc, isc);
        for (int idx = tid; idx < out * in; idx += nthr) {
          const int o = idx / in, k = idx - o * in;
          const float v = w[idx] * sc;
          const _Float16 h0 = (_Float16)v;
          const _Float16 h1 = (_Float16)(v - (float)h0);
          uint8_t* blk = smb + HP<S>::wb(i) + ((o >> 5) * nbi + (k >> 5)) * kHB + hx_welem(o & 31, k & 31);
          *reinterpret_cast<_Float16*>(blk) = h0;
          *reinterpret_cast<_Float16*>(blk + 2048) = h1;
        }
        if (b)
          for (int c = tid; c < out; c += nthr) reinterpret_cast<float*>(smb + HP<S>::tb(i))[c] = b[c];
        if (tid == 0) reinterpret_cast<float*>(smb + HP<S>::inv)[i] = 1.f / sc;
      } else {
        constexpr int nb = S::nbi(i);
        float* t = reinterpret_cast<float*>(smb + HP<S>::wb(i));
        for (int c = tid; c < in; c += nthr) {
          t[c] = w[c];
          t[nb * 32 + c] = b[c];
        }
      }
    });
  }

  template <class S, int I>
  static __device__ __forceinline__ void lin_fwd(const uint8_t* smb, float (&cur)[kMB][16], int lane, int hb) {
    constexpr int in = S::in(I), out = S::out(I), nbi = S::nbi(I), nbo = S::nbo(I), act = S::act(I);
    // this lane's row: max |v| over its channels of the layer's input (both half-lanes), as the power-of-two scale and its inverse
    float m = hx_lane_max<in>(cur);
    m = fmaxf(m, __shfl_xor(m, 32));
    float sc, inv;
    hx_pow2(m, sc, inv);
    inv *= reinterpret_cast<const float*>(smb + HP<S>::inv)[I];
    hx_f16x8 b0[kMB][2], b1[kMB][2];
    mm_static_for<nbi>([&](auto IB) __attribute__((always_inline)) {
      constexpr int ib = decltype(IB)::value;
      mm_static_for<hx_steps(in, ib)>([&](auto SS) __attribute__((always_inline)) {
        constexpr int s = decltype(SS)::value;
        hx_split8<mm_ne(in, ib)>(cur[ib], s, sc, b0[ib][s], b1[ib][s]);
      });
    });
    const int r = lane & 31;
    const int frow = r * 64, fx = (r >> 2) & 3;
    f32x16 acc[kMB];
    mm_static_for<nbo>([&](auto OB) __attribute__((always_inline)) {
      constexpr int ob = decltype(OB)::value;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[ob][e] = 0.f;
      mm_static_for<nbi>([&](auto IB) __attribute__((always_inline)) {
        constexpr int ib = decltype(IB)::value;
        const uint8_t* blk = smb + HP<S>::wb(I) + (ob * nbi + ib) * kHB + frow;
        mm_static_for<hx_steps(in, ib)>([&](auto SS) __attribute__((always_inline)) {
          constexpr int s = decltype(SS)::value;
          const int ch = ((2 * s + hb) ^ fx) << 4;
          const hx_f16x8 a0 = hx_frag(blk + ch), a1 = hx_frag(blk + 2048 + ch);
          acc[ob] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0[ib][s], acc[ob], 0, 0, 0);
          acc[ob] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1[ib][s], acc[ob], 0, 0, 0);
          acc[ob] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0[ib][s], acc[ob], 0, 0, 0);
        });
      });
      __builtin_amdgcn_sched_barrier(0);
    });
    const float* bt = reinterpret_cast<const float*>(smb + HP<S>::tb(I));
#pragma unroll
    for (int ob = 0; ob < kMB; ++ob)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (4 * j < mm_ne(out, ob)) {
          const float4 b4 = *reinterpret_cast<const float4*>(bt + 32 * ob + 8 * j + 4 * hb);
          const float bv[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float y = fmaf(acc[ob][4 * j + q], inv, bv[q]);
            cur[ob][4 * j + q] = act == 1 ? fmaxf(y, 0.f) : (act == 2 ? tanhf(y) : y);
          }
        }
  }

  template <class S>
  struct Bwd {
    float bsum[S::nlin > 0 ? S::nlin : 1];   // for blocks with in-block 0: its rows' share of the bias gradient (lane = out channel, row half)
    float* tsc;                              // the tile scales in LDS
    int lv, tq, tp, th, tkg;                 // lane roles of the transposing reads, per tile (bwd_tile)
  };
  template <class S>
  static __device__ __forceinline__ void bwd_init(Bwd<S>& st, uint8_t* aux, int) {
#pragma unroll
    for (int k = 0; k < (S::nlin > 0 ? S::nlin : 1); ++k) st.bsum[k] = 0.f;
    st.tsc = reinterpret_cast<float*>(aux);
  }
  // lane roles of the transposing reads: 16-lane group g = 2 kg + h, lane i of the group = 4 q + p.  From an OPAQUE copy of the
  // lane index, made per tile: the few dozen fragment addresses below are loop-invariant, and the compiler otherwise keeps every
  // one of them in a register across the tile loop (47 spilled registers; the same trap as h2gemmp.h's epilogue)
  template <class S>
  static __device__ __forceinline__ int bwd_tile(Bwd<S>& st, int lane) {
    int lv = lane;
    asm volatile("" : "+v"(lv));
    st.lv = lv;
    st.tq = (lv >> 2) & 3; st.tp = lv & 3; st.th = (lv >> 4) & 1; st.tkg = lv >> 5;
    return lv;
  }

  template <class S, int i, bool DX>
  static __device__ __forceinline__ void lin_bwd(Bwd<S>& st, const XArgs& a, const uint8_t* smb, f32x16& Wb, float*, uint8_t* tiles,
                                                 uint8_t* myT, float (&d)[kMB][16], float (&xin)[kMB][16], int lane, int wave) {
    constexpr int in = S::in(i), out = S::out(i), nbi = S::nbi(i), nbo = S::nbo(i), lin = S::lin(i), pact = S::pact(i);
    const int lv = st.lv, tq = st.tq, tp = st.tp, th = st.th, tkg = st.tkg;
    float* const tsc = st.tsc;
    // ---- scales of the tile, dz and x as pieces: dz into registers (the data gradient's B operand) and both into the tiles
    float sdz, idz, sx, ix;
    hx_pow2(hx_wave_max(hx_lane_max<out>(d)), sdz, idz);
    hx_pow2(hx_wave_max(hx_lane_max<in>(xin)), sx, ix);
    mm_static_for<nbo>([&](auto OB) __attribute__((always_inline)) {
      constexpr int ob = decltype(OB)::value;
      mm_static_for<hx_steps(out, ob)>([&](auto SS) __attribute__((always_inline)) {
        constexpr int s = decltype(SS)::value;
        hx_f16x8 p0, p1;
        hx_split8<mm_ne(out, ob)>(d[ob], s, sdz, p0, p1);
        hx_tile_write(myT, lv & 31, lv >> 5, ob, s, p0, p1);
      });
    });
    mm_static_for<nbi>([&](auto IB) __attribute__((always_inline)) {
      constexpr int ib = decltype(IB)::value;
      mm_static_for<hx_steps(in, ib)>([&](auto SS) __attribute__((always_inline)) {
        constexpr int s = decltype(SS)::value;
        hx_f16x8 x0, x1;
        hx_split8<mm_ne(in, ib)>(xin[ib], s, sx, x0, x1);
        hx_tile_write(myT + kHTile, lv & 31, lv >> 5, ib, s, x0, x1);
      });
    });
    if (lane == 0) {
      tsc[2 * wave] = idz;
      tsc[2 * wave + 1] = idz * ix;
    }
    // ---- data gradient (before the barrier: it needs registers and the weights only)
    if constexpr (i > 0 || DX) {
      f32x16 acc[kMB];
      const float dinv = idz * reinterpret_cast<const float*>(smb + HP<S>::inv)[i];
      mm_static_for<nbi>([&](auto IB) __attribute__((always_inline)) {
        constexpr int ib = decltype(IB)::value;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[ib][e] = 0.f;
        mm_static_for<nbo>([&](auto OB) __attribute__((always_inline)) {
          constexpr int ob = decltype(OB)::value;
          const uint8_t* blk = smb + HP<S>::wb(i) + (ob * nbi + ib) * kHB;
          mm_static_for<hx_steps(out, ob)>([&](auto SS) __attribute__((always_inline)) {
            constexpr int s = decltype(SS)::value;
            // rows (out channels) 16 s + 4 kg + q and + 8; this lane's run: k-values 16 h + 4 p .. + 3 of the block
            const int o0 = 16 * s + 4 * tkg + tq, o1 = o0 + 8;
            const int c0 = (((2 * th + (tp & 1)) ^ ((o0 >> 2) & 3)) << 4) + ((tp >> 1) << 3);
            const int c1 = (((2 * th + (tp & 1)) ^ ((o1 >> 2) & 3)) << 4) + ((tp >> 1) << 3);
            const hx_f16x8 a0 = hx_tr2(blk + o0 * 64 + c0, blk + o1 * 64 + c1);
            const hx_f16x8 a1 = hx_tr2(blk + 2048 + o0 * 64 + c0, blk + 2048 + o1 * 64 + c1);
            // B: this lane's own 8 k-values of dz, back from its row of the tile (32 registers less than keeping them)
            hx_f16x8 pd0, pd1;
            hx_tile_read(myT, lv & 31, lv >> 5, ob, s, pd0, pd1);
            acc[ib] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, pd0, acc[ib], 0, 0, 0);
            acc[ib] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, pd1, acc[ib], 0, 0, 0);
            acc[ib] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, pd0, acc[ib], 0, 0, 0);
          });
        });
        __builtin_amdgcn_sched_barrier(0);
      });
#pragma unroll
      for (int ib = 0; ib < kMB; ++ib)
#pragma unroll
        for (int e = 0; e < 16; ++e)
          if (e < mm_ne(in, ib)) d[ib][e] = acc[ib][e] * dinv * act_der(xin[ib][e], pact);
    }
    __syncthreads();
    // behind a branch the compiler cannot fold, the block stays a region of its own: merged into the layer's code, its
    // addresses stay live across it and the C1 towers' kernels spill (~570 bytes of scratch per lane)
    int on = 1;
    asm volatile("" : "+s"(on));
    if (on) {
      // this wavefront's block of the layer, over its share of the four tiles: 4 blocks -> every tile; 2 -> two tiles; 1 -> its own
      constexpr int nblk = nbo * nbi, per = nblk >= kBwdWaves ? kBwdWaves : nblk;
      const int b = wave % nblk, ob = b / nbi, ib = b - ob * nbi, t0 = (wave / nblk) * per;
      const bool bias = a.gb[i] != nullptr && ib == 0;
      const hx_f16x2 ones2 = {(_Float16)1.f, (_Float16)1.f};
      // fragment addresses inside a tile: rows 16 ts + 8 kg + q (+ 4), 8-byte slot 8 blk + 4 h + p of piece 0 (+ 16: piece 1)
#pragma unroll
      for (int t = 0; t < per; ++t) {
        const uint8_t* TA = tiles + (t0 + t) * kHArea;
        const uint8_t* TB = TA + kHTile;
        f32x16 D;
#pragma unroll
        for (int e = 0; e < 16; ++e) D[e] = 0.f;
        float bs = 0.f;
#pragma unroll
        for (int ts = 0; ts < 2; ++ts) {
          const int r0 = 16 * ts + 8 * tkg, x0 = (r0 >> 2) & 7, x1 = ((r0 + 4) >> 2) & 7;
          const int ra = (r0 + tq) * kHRow, rb = (r0 + 4 + tq) * kHRow;
          const int sa = 8 * ob + 4 * th + tp, sb = 8 * ib + 4 * th + tp;
          const hx_f16x8 a0 = hx_tr2(TA + ra + ((sa ^ x0) << 3), TA + rb + ((sa ^ x1) << 3));
          const hx_f16x8 a1 = hx_tr2(TA + ra + (((16 + sa) ^ x0) << 3), TA + rb + (((16 + sa) ^ x1) << 3));
          const hx_f16x8 b0 = hx_tr2(TB + ra + ((sb ^ x0) << 3), TB + rb + ((sb ^ x1) << 3));
          const hx_f16x8 b1 = hx_tr2(TB + ra + (((16 + sb) ^ x0) << 3), TB + rb + (((16 + sb) ^ x1) << 3));
          D = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0, D, 0, 0, 0);
          D = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, D, 0, 0, 0);
          D = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, D, 0, 0, 0);
          if (bias) {
            const uint4 q0 = __builtin_bit_cast(uint4, a0), q1 = __builtin_bit_cast(uint4, a1);
            const uint32_t w[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
            for (int k = 0; k < 8; ++k) bs = __builtin_amdgcn_fdot2(__builtin_bit_cast(hx_f16x2, w[k]), ones2, bs, false);
          }
        }
        const float it = tsc[2 * (t0 + t) + 1];
#pragma unroll
        for (int e = 0; e < 16; ++e) Wb[e] = fmaf(D[e], it, Wb[e]);
        if (bias) st.bsum[lin] = fmaf(bs, tsc[2 * (t0 + t)], st.bsum[lin]);
      }
    }
    __syncthreads();   // the tile areas are rewritten by the next layer below
  }

  // bias gradients: lane (out channel, row half) of the wavefronts that formed a block with in-block 0
  template <class S>
  static __device__ __forceinline__ void bias_flush(Bwd<S>& st, float* pgs, int lane, int wave) {
    mm_static_for<S::n>([&](auto IC) __attribute__((always_inline)) {
      constexpr int i = decltype(IC)::value;
      if constexpr (S::kind(i) == 1) {
        constexpr int nbi = S::nbi(i), nblk = S::nbo(i) * nbi, lin = S::lin(i);
        const int b = wave % nblk, ob = b / nbi, ib = b - ob * nbi;
        const float v = st.bsum[lin] + __shfl_xor(st.bsum[lin], 32);
        if (ib == 0 && lane < 32) pgs[S::pg(i) * 64 + 32 * ob + lane] = v;
      }
    });
  }
};

inline int hx_mode() {   // SRL_MLP_F16: 0 the float32 policy; 1 (default) f16 pieces; bit 1 set: f16 pieces forward only
  static const int v = [] { const char* e = getenv("SRL_MLP_F16"); return e ? atoi(e) : 1; }();
  return v;
}

}  // namespace
