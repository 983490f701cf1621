// Language encoder of the DMLab agent in one launch per direction (include/srl_hip.h: srl_instr_lstm_*).
//
// Reference: DMLabActorCritic.forward (legacy/algorithm/ppo/game_policies/dmlab_policy.py:144-158): per row, len = max(1, number of
// non-zero tokens); the FIRST len tokens (zeros inside the prefix included) are embedded (nn.Embedding(V, Ed, padding_idx=0)) and
// run through nn.LSTM(Ed, H) from a zero state; the feature is h at step len - 1.
//
// A workgroup of 4 wavefronts walks tiles of 32 rows (a persistent grid).  W_ih | W_hh are staged ONCE per workgroup in LDS as
// Ws[k][p] (k: the Ed embedding columns, padded to an even count, then the H state columns; p: a permutation of the 4H gate
// channels, below; leading dimension 4H + 1, so that both Ws[k][p..p+31] and Ws[k..k+31][p] are conflict-free).  A step forms
// z[p][row] = Ws^T . X^T on v_mfma_f32_32x32x2_f32 (exact float32 multiply-adds) with X = (emb[tok_t] | h_{t-1}) [32][K] in LDS.
// Channel order: wavefront w owns the hidden units [w H/4, (w+1) H/4); a 32-channel block holds 8 of them, gate-major
// (p = 32 (w NB + b) + 8 gate + u  <->  channel gate H + w H/4 + 8 b + u).  In the accumulator, lane (row r, half hb) then holds
// register e = 4 gate + m  <->  unit 8 b + 4 hb + m: all four gates of a unit for one row sit in ONE lane, the cell update is
// lane-local and c never leaves registers.  The time loop runs to the TILE's longest sequence; a row whose sequence has ended
// keeps its h (it lives in X), so the tile's output is X's state columns.  At t = 0 the state is zero and its columns are skipped.
//
// Backward (no tape between the calls): the forward walk is repeated and keeps h_t, c_t of its tile in the caller's workspace
// (2 L H 32 floats per workgroup: at L = 16 that is 256 KiB, more than the LDS holds beside the weights).  The reverse walk
// recomputes the gates of step t from (x_t, h_{t-1}), forms d z lane-locally and stores it as dz[row][p] in LDS;
//   d W[p][k] += dz^T X    MFMA over the 32 rows; every wavefront keeps ITS channels' [32 NB][K] sums in accumulators over all steps
//                          and all tiles and adds them to global memory once, at the end (float atomics);
//   d X[k][row] = Ws dz^T  MFMA over the 4H channels (wavefront kb: columns [32 kb, 32 kb + 32)): the state columns are d h_{t-1},
//                          the embedding columns are added to g_emb[tok_t] (float atomics; never for token 0);
//   d b                    lane-local sums, reduced over the rows with shuffles at the end.
#include "srl_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = 256;
constexpr int kRows = 32;        // rows of a tile = columns of an MFMA block
constexpr int kMaxGrid = 256;    // workgroups the backward's workspace is sized for
constexpr int kLdsBytes = 160 * 1024;

struct IlPlan {
  int EdP, K, nkb, ldw, ldx;   // Ed rounded up to even; EdP + H; ceil(K / 32); 4H + 1; 32 nkb + 1
  int o_ws, o_b, o_x, o_dz, o_dx, o_len, total;   // LDS offsets (floats)
};

struct IlArgs {
  srl_instr_lstm d;
  IlPlan pl;
  int64_t rows;
  float* out;
  int64_t ldo;
  const float* dout;
  int64_t lddo;
  float* ws;
};

bool valid_shape(const srl_instr_lstm* d) {
  return d && d->V >= 1 && d->V <= 65536 && d->Ed >= 1 && d->Ed <= 32 && (d->H == 32 || d->H == 64) && d->L >= 1 && d->L <= 64;
}

void make_plan(const srl_instr_lstm& d, bool bwd, IlPlan* p) {
  p->EdP = (d.Ed + 1) & ~1;
  p->K = p->EdP + d.H;
  p->nkb = (p->K + 31) / 32;
  p->ldw = 4 * d.H + 1;
  p->ldx = 32 * p->nkb + 1;
  int o = 0;
  p->o_ws = o; o += p->K * p->ldw;
  p->o_b = o; o += 4 * d.H;
  p->o_x = o; o += kRows * p->ldx;
  p->o_dz = o; o += bwd ? kRows * p->ldw : 0;
  p->o_dx = o; o += bwd ? kRows * p->ldx : 0;
  p->o_len = o; o += kRows;
  p->total = o;
}

int64_t ws_floats_per_group(const srl_instr_lstm& d) { return 2LL * d.L * d.H * kRows; }

// the token at (row, t) as the reference's .long() reads it; anything outside [1, V) is padding (0)
__device__ __forceinline__ int tok_at(const srl_instr_lstm& d, int64_t row, int t) {
  if (d.tok_i32) {
    const int v = static_cast<const int32_t*>(d.tok)[row * d.ld_tok + t];
    return (v > 0 && v < d.V) ? v : 0;
  }
  const float f = static_cast<const float*>(d.tok)[row * d.ld_tok + t];
  return (f >= 1.0f && f < (float)d.V) ? (int)f : 0;
}

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

// acc[b][..] += Ws[2kk + hb][pbase + 32 b + r] * X[r][2kk + hb] over the column pairs [kp0, kp1)
template <int NB>
__device__ __forceinline__ void gate_mm(f32x16 (&acc)[NB], const float* Ws, int ldw, const float* xs, int ldx, int kp0, int kp1,
                                        int pbase, int r, int hb) {
  for (int kk = kp0; kk < kp1; ++kk) {
    const int k = 2 * kk + hb;
    const float x = xs[r * ldx + k];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ws[k * ldw + pbase + 32 * b + r], x, acc[b], 0, 0, 0);
  }
}

template <int NB, bool BWD>
__global__ void __launch_bounds__(kThreads) instr_lstm_kernel(const IlArgs A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int H = 32 * NB, U = 8 * NB, NT = kThreads;
  const srl_instr_lstm& d = A.d;
  const IlPlan& pl = A.pl;
  const int tid = threadIdx.x, lane = tid & 63, wq = tid >> 6, r = lane & 31, hb = lane >> 5;
  const int Ed = d.Ed, EdP = pl.EdP, K = pl.K, ldw = pl.ldw, ldx = pl.ldx, L = d.L;
  const int pbase = wq * 32 * NB;
  float* Ws = lds + pl.o_ws;
  float* bs = lds + pl.o_b;
  float* xs = lds + pl.o_x;
  float* dzs = lds + pl.o_dz;
  float* dxs = lds + pl.o_dx;
  int* lens = reinterpret_cast<int*>(lds + pl.o_len);
  // unit of (block b, register m) for this lane, and its channel of gate g
  auto unit = [&](int b, int m) { return wq * U + 8 * b + 4 * hb + m; };

  // ---- stage the weights (global reads run along a weight row) and the summed bias, in position order
  for (int i = tid; i < 4 * H * K; i += NT) {
    const int ch = i / K, k = i % K, gate = ch / H, u = ch % H;
    const int p = 32 * NB * (u / U) + 32 * ((u % U) / 8) + 8 * gate + (u % 8);
    Ws[k * ldw + p] = k < Ed ? d.w_ih[ch * Ed + k] : (k < EdP ? 0.0f : d.w_hh[ch * H + (k - EdP)]);
  }
  for (int ch = tid; ch < 4 * H; ch += NT) bs[ch] = d.b_ih[ch] + d.b_hh[ch];

  f32x16 wacc[NB][3];   // backward: d (W_ih | W_hh) of this wavefront's channels
  float gb[NB][16];     // backward: d b of this lane's units, one row's share
  if (BWD) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
#pragma unroll
      for (int kb = 0; kb < 3; ++kb)
#pragma unroll
        for (int e = 0; e < 16; ++e) wacc[b][kb][e] = 0.0f;
#pragma unroll
      for (int e = 0; e < 16; ++e) gb[b][e] = 0.0f;
    }
  }
  float* hws = BWD ? A.ws + (int64_t)blockIdx.x * (2LL * L * H * kRows) : nullptr;
  float* cws = BWD ? hws + (int64_t)L * H * kRows : nullptr;
  __syncthreads();

  const int64_t ntiles = (A.rows + kRows - 1) / kRows;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * kRows;
    const int nv = (int)((A.rows - row0) < kRows ? (A.rows - row0) : kRows);   // rows past the end are never read or written

    // ---- lengths; a zero state
    if (tid < kRows) {
      int len = 0;
      if (tid < nv) {
        for (int t = 0; t < L; ++t) len += tok_at(d, row0 + tid, t) != 0;
        len = len < 1 ? 1 : len;
      }
      lens[tid] = len;
    }
    for (int i = tid; i < kRows * H; i += NT) xs[(i / H) * ldx + EdP + i % H] = 0.0f;
    __syncthreads();
    int maxlen = 0;
    for (int i = 0; i < kRows; ++i) maxlen = lens[i] > maxlen ? lens[i] : maxlen;
    const int mylen = lens[r];

    // ---- the forward walk
    float c[NB][4];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int m = 0; m < 4; ++m) c[b][m] = 0.0f;
    for (int t = 0; t < maxlen; ++t) {
      for (int i = tid; i < kRows * EdP; i += NT) {
        const int rr = i / EdP, e = i % EdP;
        const int tk = t < lens[rr] ? tok_at(d, row0 + rr, t) : 0;
        xs[rr * ldx + e] = e < Ed ? d.emb[(int64_t)tk * Ed + e] : 0.0f;
      }
      __syncthreads();
      f32x16 acc[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[b][e] = bs[(e >> 2) * H + unit(b, e & 3)];
      gate_mm<NB>(acc, Ws, ldw, xs, ldx, 0, EdP / 2, pbase, r, hb);
      if (t > 0) gate_mm<NB>(acc, Ws, ldw, xs, ldx, EdP / 2, K / 2, pbase, r, hb);
      __syncthreads();   // every wavefront has read h_{t-1}
      if (t < mylen) {
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            const float gi = sigm(acc[b][m]), gf = sigm(acc[b][4 + m]), gg = tanhf(acc[b][8 + m]), go = sigm(acc[b][12 + m]);
            c[b][m] = fmaf(gf, c[b][m], gi * gg);
            const float h = go * tanhf(c[b][m]);
            xs[r * ldx + EdP + unit(b, m)] = h;
            if (BWD) {
              hws[((int64_t)t * H + unit(b, m)) * kRows + r] = h;
              cws[((int64_t)t * H + unit(b, m)) * kRows + r] = c[b][m];
            }
          }
      }
    }
    __syncthreads();

    if (!BWD) {
      for (int i = tid; i < nv * H; i += NT) A.out[(row0 + i / H) * A.ldo + i % H] = xs[(i / H) * ldx + EdP + i % H];
      __syncthreads();   // the next tile clears the state
      continue;
    }

    // ---- the reverse walk (hws / cws: this workgroup's own writes, visible to it behind the barrier)
    float dhc[NB][4], dcc[NB][4];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int m = 0; m < 4; ++m) dhc[b][m] = dcc[b][m] = 0.0f;
    for (int t = maxlen - 1; t >= 0; --t) {
      // X of step t; rows that are not in this step get a finite X (their d z is 0)
      for (int i = tid; i < kRows * EdP; i += NT) {
        const int rr = i / EdP, e = i % EdP;
        const int tk = t < lens[rr] ? tok_at(d, row0 + rr, t) : 0;
        xs[rr * ldx + e] = e < Ed ? d.emb[(int64_t)tk * Ed + e] : 0.0f;
      }
      for (int i = tid; i < kRows * H; i += NT) {
        const int k = i / kRows, rr = i % kRows;
        xs[rr * ldx + EdP + k] = (t > 0 && t < lens[rr]) ? hws[((int64_t)(t - 1) * H + k) * kRows + rr] : 0.0f;
      }
      __syncthreads();
      f32x16 acc[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[b][e] = bs[(e >> 2) * H + unit(b, e & 3)];
      gate_mm<NB>(acc, Ws, ldw, xs, ldx, 0, EdP / 2, pbase, r, hb);
      if (t > 0) gate_mm<NB>(acc, Ws, ldw, xs, ldx, EdP / 2, K / 2, pbase, r, hb);
      const bool active = t < mylen;
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          float di = 0.0f, df = 0.0f, dg = 0.0f, dgo = 0.0f;
          if (active) {
            const int u = unit(b, m);
            const float gi = sigm(acc[b][m]), gf = sigm(acc[b][4 + m]), gg = tanhf(acc[b][8 + m]), go = sigm(acc[b][12 + m]);
            const float cp = t > 0 ? cws[((int64_t)(t - 1) * H + u) * kRows + r] : 0.0f;
            const float tc = tanhf(fmaf(gf, cp, gi * gg));
            const float dh = dhc[b][m] + (t == mylen - 1 ? A.dout[(row0 + r) * A.lddo + u] : 0.0f);
            const float dc = fmaf(dh * go, 1.0f - tc * tc, dcc[b][m]);
            dgo = dh * tc * go * (1.0f - go);
            di = dc * gg * gi * (1.0f - gi);
            df = dc * cp * gf * (1.0f - gf);
            dg = dc * gi * (1.0f - gg * gg);
            dcc[b][m] = dc * gf;
          }
          float* z = dzs + r * ldw + pbase + 32 * b + 4 * hb + m;
          z[0] = di; z[8] = df; z[16] = dg; z[24] = dgo;
          gb[b][m] += di; gb[b][4 + m] += df; gb[b][8 + m] += dg; gb[b][12 + m] += dgo;
        }
      __syncthreads();
      // d W += dz^T X over the tile's rows
      for (int kk = 0; kk < kRows / 2; ++kk) {
        const int rr = 2 * kk + hb;
        float xv[3];
#pragma unroll
        for (int kb = 0; kb < 3; ++kb) xv[kb] = kb < pl.nkb ? xs[rr * ldx + 32 * kb + r] : 0.0f;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const float a = dzs[rr * ldw + pbase + 32 * b + r];
#pragma unroll
          for (int kb = 0; kb < 3; ++kb)
            if (kb < pl.nkb) wacc[b][kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xv[kb], wacc[b][kb], 0, 0, 0);
        }
      }
      // d X = Ws dz^T: wavefront kb forms columns [32 kb, 32 kb + 32) (a column past K repeats column K - 1 and is dropped)
      if (wq < pl.nkb) {
        f32x16 xacc;
#pragma unroll
        for (int e = 0; e < 16; ++e) xacc[e] = 0.0f;
        const int kr = (32 * wq + r) < K ? (32 * wq + r) : K - 1;
        for (int kk = 0; kk < 2 * H; ++kk)
          xacc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ws[kr * ldw + 2 * kk + hb], dzs[r * ldw + 2 * kk + hb], xacc, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 16; ++e) dxs[r * ldx + 32 * wq + 8 * (e >> 2) + 4 * hb + (e & 3)] = xacc[e];
      }
      __syncthreads();
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int m = 0; m < 4; ++m) dhc[b][m] = active ? dxs[r * ldx + EdP + unit(b, m)] : 0.0f;
      for (int i = tid; i < kRows * Ed; i += NT) {
        const int rr = i / Ed, e = i % Ed;
        if (t < lens[rr]) {
          const int tk = tok_at(d, row0 + rr, t);
          if (tk != 0) atomicAdd(d.g_emb + (int64_t)tk * Ed + e, dxs[rr * ldx + e]);
        }
      }
    }
    __syncthreads();   // the next tile overwrites lens and X
  }

  if (BWD) {   // the workgroup's sums, once
#pragma unroll
    for (int b = 0; b < NB; ++b) {
#pragma unroll
      for (int kb = 0; kb < 3; ++kb) {
        if (kb >= pl.nkb) continue;
        const int k = 32 * kb + r;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int i = 8 * (e >> 2) + 4 * hb + (e & 3);           // row of the block: 8 gate + u
          const int ch = (i >> 3) * H + wq * U + 8 * b + (i & 7);
          const float v = wacc[b][kb][e];
          if (v == 0.0f) continue;
          if (k < Ed) atomicAdd(d.g_w_ih + ch * Ed + k, v);
          else if (k >= EdP && k < K) atomicAdd(d.g_w_hh + ch * H + (k - EdP), v);
        }
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        float v = gb[b][e];
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);   // over the rows; the halves stay apart
        if (r == 0 && v != 0.0f) {
          const int ch = (e >> 2) * H + unit(b, e & 3);
          atomicAdd(d.g_b_ih + ch, v);
          atomicAdd(d.g_b_hh + ch, v);
        }
      }
    }
  }
}

int check_desc(const srl_instr_lstm* d, bool bwd, const char** why) {
  if (!valid_shape(d)) { *why = "unsupported shape (srl_instr_lstm_supported)"; return 0; }
  if (!d->emb || !d->w_ih || !d->w_hh || !d->b_ih || !d->b_hh) { *why = "null parameter"; return 0; }
  if (bwd && (!d->g_emb || !d->g_w_ih || !d->g_w_hh || !d->g_b_ih || !d->g_b_hh)) { *why = "null gradient"; return 0; }
  if (!d->tok || d->ld_tok < d->L) { *why = "null tokens / short token rows"; return 0; }
  return 1;
}

// workgroups a launch runs `rows` rows on (the staged weights take more than half the LDS: one workgroup per CU), at most
// `max_groups`: what launch<> uses and what srl_instr_lstm_groups reports
int64_t make_grid(int64_t rows, int64_t max_groups) {
  int cus = 256;
  int dev = 0;
  if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  const int64_t ntiles = srl_ceil_div(rows, (int64_t)kRows);
  const int64_t grid = ntiles < cus ? ntiles : cus;
  return grid < max_groups ? grid : max_groups;
}

// workgroups a caller's workspace holds the states of (srl_instr_lstm_bwd refuses 0)
int64_t ws_groups(const srl_instr_lstm& d, int64_t workspace_bytes) {
  return workspace_bytes / (ws_floats_per_group(d) * (int64_t)sizeof(float));
}

template <bool BWD>
int launch(void* stream, const srl_instr_lstm* d, int64_t rows, float* out, int64_t ldo, const float* dout, int64_t lddo, float* ws,
           int64_t max_groups) {
  if (rows == 0) return 0;
  IlArgs a;
  memset(&a, 0, sizeof(a));
  a.d = *d;
  make_plan(*d, BWD, &a.pl);
  a.rows = rows; a.out = out; a.ldo = ldo; a.dout = dout; a.lddo = lddo; a.ws = ws;
  const size_t lds = (size_t)a.pl.total * sizeof(float);
  const int64_t grid = make_grid(rows, max_groups);
  void (*kern)(const IlArgs) = d->H == 64 ? instr_lstm_kernel<2, BWD> : instr_lstm_kernel<1, BWD>;
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kThreads), lds, (hipStream_t)stream, a);
  SRL_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int srl_instr_lstm_supported(const srl_instr_lstm* d) {
  if (!valid_shape(d)) return 0;
  IlPlan pl;
  make_plan(*d, true, &pl);
  return pl.nkb <= 3 && (size_t)pl.total * sizeof(float) <= (size_t)kLdsBytes ? 1 : 0;
}

extern "C" int64_t srl_instr_lstm_bwd_workspace(const srl_instr_lstm* d, int64_t rows) {
  if (!valid_shape(d) || rows <= 0) return 0;
  const int64_t ntiles = srl_ceil_div(rows, (int64_t)kRows);
  return (ntiles < kMaxGrid ? ntiles : kMaxGrid) * ws_floats_per_group(*d) * (int64_t)sizeof(float);
}

extern "C" int srl_instr_lstm_fwd(void* stream, const srl_instr_lstm* d, int64_t rows, float* out, int64_t ldo) {
  const char* why = "";
  SRL_CHECK_ARG(check_desc(d, false, &why), why);
  SRL_CHECK_ARG(srl_instr_lstm_supported(d), "unsupported shape (srl_instr_lstm_supported)");
  SRL_CHECK_ARG(out && rows >= 0 && ldo >= d->H, "null out / short out rows");
  return launch<false>(stream, d, rows, out, ldo, nullptr, 0, nullptr, kMaxGrid);
}

extern "C" int srl_instr_lstm_bwd(void* stream, const srl_instr_lstm* d, int64_t rows, const float* d_out, int64_t lddo,
                                  void* workspace, int64_t workspace_bytes) {
  const char* why = "";
  SRL_CHECK_ARG(check_desc(d, true, &why), why);
  SRL_CHECK_ARG(srl_instr_lstm_supported(d), "unsupported shape (srl_instr_lstm_supported)");
  SRL_CHECK_ARG(d_out && rows >= 0 && lddo >= d->H, "null d_out / short d_out rows");
  if (rows == 0) return 0;
  SRL_CHECK_ARG(workspace && ws_groups(*d, workspace_bytes) >= 1, "workspace smaller than one workgroup's states (srl_instr_lstm_bwd_workspace)");
  return launch<true>(stream, d, rows, nullptr, 0, d_out, lddo, static_cast<float*>(workspace), ws_groups(*d, workspace_bytes));
}

extern "C" int64_t srl_instr_lstm_groups(const srl_instr_lstm* d, int64_t rows, int64_t workspace_bytes) {
  if (!srl_instr_lstm_supported(d) || rows <= 0) return 0;
  if (workspace_bytes < 0) return make_grid(rows, kMaxGrid);
  const int64_t fit = ws_groups(*d, workspace_bytes);
  return fit >= 1 ? make_grid(rows, fit) : 0;
}
