// The LSTM / GRU cell, once: the gate activations, the state update and the derivative taken by hand, as scalar functions of
// values in registers.  No kernels, no loads or stores, no layout: gru.hip (one launch per step), rnn_step.hip (W_hh h and the
// cell in one launch) and rnn_seq.hip (a chunk's time loop in one launch) bring the operands and place the results; adding the
// carry to dh, the reset masks and the saving of the gates are theirs.  Those paths are interchangeable -- each can run another's
// backward on what its forward saved -- because they all evaluate exactly these expressions, in this operand order and grouping.
// Two statements remain outside, each for the sake of the bits it has always produced (both forwards end in a sum of two products,
// one of which the compiler fuses into an FMA; which one is its choice, and the result differs by a rounding):
//   gru.hip's two forward kernels spell the state update out (gates from LibmGates).  They read the incoming state from memory
//     after the gates; as an argument here it is read before them, and the compiler then fuses the other product.
//   instr_lstm.hip keeps its own LSTM: see the note at lstm_fwd.
#pragma once
#include <hip/hip_runtime.h>

namespace rnn_cell {

// Gate math as a compile-time policy.
struct LibmGates {
  static __device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }
  static __device__ __forceinline__ float tanh(float x) { return tanhf(x); }
};
// The gates on the hardware's exp2 / reciprocal (v_exp_f32, v_rcp_f32: 1 ulp each) instead of libm's expf / tanhf and an IEEE
// division: a step's 5 transcendentals per unit were ~4 800 vector instructions per 32 rows, as long as the step's 256 MFMAs, and
// with one wavefront per SIMD the two add up.  |error| <= ~2e-7 absolute on values in [-1, 1] (tanh near 0 through 1 - 2 / (1 +
// e^2x): absolute, not relative).
struct FastGates {
  static __device__ __forceinline__ float sigm(float x) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896341f * x)); }
  static __device__ __forceinline__ float tanh(float x) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(2.88539008177792681f * x)); }
};

// GRU (torch.nn.GRU, gates r | z | n): gi = W_ih x + b_ih, gh = W_hh h_in + b_hh; b_hn sits inside r * (.).
struct GruFwd { float r, z, n, h; };
template <class M>
__device__ __forceinline__ GruFwd gru_fwd(float gi_r, float gi_z, float gi_n, float gh_r, float gh_z, float gh_n, float h_in) {
  GruFwd o;
  o.r = M::sigm(gi_r + gh_r);
  o.z = M::sigm(gi_z + gh_z);
  o.n = M::tanh(gi_n + o.r * gh_n);
  o.h = (1.0f - o.z) * o.n + o.z * h_in;
  return o;
}

// d gi (r, z, n); d gh is (d_r, d_z, d_gh_n); direct = dh * z, the part of d h_in that does not go through W_hh
struct GruBwd { float d_r, d_z, d_n, d_gh_n, direct; };
__device__ __forceinline__ GruBwd gru_bwd(float dh, float r, float z, float n, float gh_n, float h_in) {
  const float dn = dh * (1.0f - z);
  const float dz = dh * (h_in - n);
  GruBwd o;
  o.d_n = dn * (1.0f - n * n);
  o.d_r = o.d_n * gh_n * r * (1.0f - r);
  o.d_z = dz * z * (1.0f - z);
  o.d_gh_n = o.d_n * r;
  o.direct = dh * z;
  return o;
}

// LSTM (torch.nn.LSTM, gates i | f | g | o) on the summed pre-activations W_ih x + b_ih + W_hh h_in + b_hh:
// c' = s(f) c_in + s(i) tanh(g), h = s(o) tanh(c').
// instr_lstm.hip (the instruction encoder's LSTM over tokens) is not a caller: it writes c' and d c as explicit fmaf's and
// recomputes c' in its backward, and no single spelling here compiles to what each of the four files gave with its cell written out -- with
// fmaf(f, c_in, i * g) gru.hip and rnn_step.hip lose their packed FMAs, with the plain form below instr_lstm.hip gains packed ones.
struct LstmFwd { float i, f, g, o, c, h; };
template <class M>
__device__ __forceinline__ LstmFwd lstm_fwd(float pre_i, float pre_f, float pre_g, float pre_o, float c_in) {
  LstmFwd o;
  o.i = M::sigm(pre_i), o.f = M::sigm(pre_f), o.g = M::tanh(pre_g), o.o = M::sigm(pre_o);
  o.c = o.f * c_in + o.i * o.g;
  o.h = o.o * M::tanh(o.c);
  return o;
}

// dc: d loss / d c' arriving from the step after (0 at the chunk's end or across a reset); c is c' as the forward stored it
struct LstmBwd { float d_i, d_f, d_g, d_o, dc_in; };
template <class M>
__device__ __forceinline__ LstmBwd lstm_bwd(float dh, float dc, float i, float f, float g, float o, float c_in, float c) {
  const float tc = M::tanh(c);
  dc += dh * o * (1.0f - tc * tc);
  LstmBwd b;
  b.d_i = dc * g * i * (1.0f - i);
  b.d_f = dc * c_in * f * (1.0f - f);
  b.d_g = dc * i * (1.0f - g * g);
  b.d_o = dh * tc * o * (1.0f - o);
  b.dc_in = dc * f;
  return b;
}

}  // namespace rnn_cell
