// Pieces of the `Convolution` encoder (legacy/algorithm/modules/cnn.py:93-135) beyond unpadded 2-D convolutions: the
// whole-observation LayerNorm (policies/utils.py:53) as an explicit pass producing a channels-last float32 image, and -- on
// channels-last volumes [n, D, H, W, C] -- border padding (nn.ConvNd(padding=p, padding_mode=...)) and its adjoint, MaxPool
// (`use_maxpool`, :100-106) and its backward, the patch matrix of the explicit convolution and its adjoint.  One kernel per
// operation for every rank (modules/cnn.py:60-71 picks nn.Conv1d / Conv2d / Conv3d and the matching MaxPool by the
// observation's rank): an image is the volume with D = 1, a sequence the one with D = H = 1.  All HBM-bound element-wise
// passes; the 2-D contractions stay on the implicit-GEMM kernels, which see an already padded / pooled activation, and the
// patch matrix feeds the dense GEMM (Conv1d / Conv3d, and Conv2d geometries the implicit kernels do not take).  No reference
// experiment sets padding or use_maxpool (only modules_test.py:385-401 exercises them), so this path is built for parity,
// not for speed.
// The pooling forward starts its running maximum from the window's first element, as the backward does: a window that is
// NaN throughout gives NaN (until ABI 22 the volume kernel started from -inf and gave -inf there; the 2-D one gave NaN).
#include "srl_common.h"

namespace {

inline unsigned grid_for(long n, long cap = 65535L * 16) {
  const long b = srl_ceil_div(n, 256);
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

// y[n,h,w,c] = (x[n,c,h,w] - mean_n) * rstd_n * gamma[c,h,w] + beta[c,h,w]
template <bool U8>
__global__ __launch_bounds__(256) void obs_ln_nhwc_kernel(const void* obs, const float* mean, const float* rstd,
                                                          const float* gamma, const float* beta, long n, int C, int H, int W,
                                                          float* y) {
  const long D = (long)C * H * W, total = n * D;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long s = e / D;
    const int r = (int)(e - s * D);  // (h, w, c) order of the output
    const int c = r % C, hw = r / C;
    const int p = c * H * W + hw;    // (c, h, w) order of the observation and of the LayerNorm tables
    const float x = U8 ? (float)static_cast<const uint8_t*>(obs)[s * D + p] : static_cast<const float*>(obs)[s * D + p];
    y[e] = (x - mean[s]) * rstd[s] * gamma[p] + beta[p];
  }
}

// dgamma[p] += sum_n dy[n, p'] * xhat[n, p];  dbeta[p] += sum_n dy[n, p']   (p' = the channels-last index of p)
template <bool U8>
__global__ __launch_bounds__(256) void obs_ln_nhwc_bwd_kernel(const float* dy, const void* obs, const float* mean,
                                                              const float* rstd, long n, int C, int H, int W, float* dgamma,
                                                              float* dbeta) {
  const int D = C * H * W;
  const int r = blockIdx.x * 256 + threadIdx.x;  // channels-last index: neighbouring threads read neighbouring dy
  if (r >= D) return;
  const int c = r % C, hw = r / C;
  const int p = c * H * W + hw;
  float ag = 0.f, ab = 0.f;
  for (long s = 0; s < n; ++s) {
    const float x = U8 ? (float)static_cast<const uint8_t*>(obs)[s * D + p] : static_cast<const float*>(obs)[s * D + p];
    const float g = dy[s * D + r];
    ag += g * ((x - mean[s]) * rstd[s]);
    ab += g;
  }
  dgamma[p] += ag;
  dbeta[p] += ab;
}

// ---- channels-last volumes [n, D, H, W, C] ----------------------------------------------------------------------------
struct Vol {
  int D, H, W, C;
};
__host__ __device__ inline long voxels(Vol v) { return (long)v.D * v.H * v.W; }

// Element e of a tensor [n][D][H][W][C] as sample, voxel and channel.  One sample has fewer than 2^31 elements
// (host-checked: vol_ok), so everything below the sample index is unsigned 32-bit arithmetic: one 64-bit division per
// element (unsigned: a signed 32-bit division costs a third more instructions).
struct Pos {
  long s;
  int d, h, w, c;
};
__device__ __forceinline__ Pos split(long e, Vol v) {
  const unsigned per = v.D * v.H * v.W * v.C, C = v.C, W = v.W, H = v.H;
  Pos p;
  p.s = e / per;
  unsigned r = (unsigned)(e - p.s * per);
  p.c = r % C; r /= C;
  p.w = r % W; r /= W;
  p.h = r % H;
  p.d = r / H;
  return p;
}
// offset of (d, h, w, c) inside its sample
__device__ __forceinline__ int at(Vol v, int d, int h, int w, int c) { return ((d * v.H + h) * v.W + w) * v.C + c; }

// border of (pd, ph, pw) voxels on both sides of each axis, filled per nn.ConvNd's padding_mode: 0 zeros, 1 reflect
// (without the edge), 2 replicate, 3 circular.  Source index of padded coordinate o (already shifted by -pad) along an
// axis of extent D, or -1 for a zero.
__device__ __forceinline__ int pad_src(int o, int D, int mode) {
  if (o >= 0 && o < D) return o;
  if (mode == 1) return o < 0 ? -o : 2 * (D - 1) - o;
  if (mode == 2) return o < 0 ? 0 : D - 1;
  if (mode == 3) return o < 0 ? o + D : o - D;
  return -1;
}
// ZEROS: mode 0 known at compile time (nn.ConvNd's default, and the explicit 2-D fallback's hot case): no per-voxel
// branching on the mode in pad_src / pad_preimage(s)
template <bool ZEROS>
__global__ __launch_bounds__(256) void pad_kernel(const float* x, long n, Vol v, int pd, int ph, int pw, int mode_, float* y) {
  const int mode = ZEROS ? 0 : mode_;
  const Vol vp = {v.D + 2 * pd, v.H + 2 * ph, v.W + 2 * pw, v.C};
  const long per = voxels(v) * v.C, total = n * voxels(vp) * v.C;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const Pos p = split(e, vp);
    const int w = pad_src(p.w - pw, v.W, mode), h = pad_src(p.h - ph, v.H, mode), d = pad_src(p.d - pd, v.D, mode);
    y[e] = (d >= 0 && h >= 0 && w >= 0) ? x[p.s * per + at(v, d, h, w, p.c)] : 0.f;
  }
}
// The padded coordinates (0 .. D + 2p - 1) that read interior index i along one axis: the copy itself first, then the
// border voxels filled from it, at most 1 + 2p of them (replicate at an edge).  pad_preimages: how many;
// pad_preimage: the j-th.
__device__ __forceinline__ int pad_preimages(int i, int D, int p, int mode) {
  if (p == 0 || mode == 0) return 1;
  if (mode == 1) return 1 + (i >= 1 && i <= p) + (i <= D - 2 && i >= D - 1 - p);
  if (mode == 2) return 1 + (i == 0 ? p : 0) + (i == D - 1 ? p : 0);
  return 1 + (i >= D - p) + (i < p);
}
__device__ __forceinline__ int pad_preimage(int j, int i, int D, int p, int mode) {
  if (j == 0) return i + p;
  if (mode == 1) return (j == 1 && i >= 1 && i <= p) ? p - i : p + 2 * (D - 1) - i;
  if (mode == 2) return (i == 0 && j <= p) ? j - 1 : p + D + j - 1 - (i == 0 ? p : 0);
  return (j == 1 && i >= D - p) ? i + p - D : i + p + D;
}
// adjoint of pad_kernel: x[i] = sum of the padded voxels that were filled from i (mode 0: the crop)
template <bool ZEROS>
__global__ __launch_bounds__(256) void crop_kernel(const float* yp, long n, Vol v, int pd, int ph, int pw, int mode_, float* x) {
  const int mode = ZEROS ? 0 : mode_;
  const Vol vp = {v.D + 2 * pd, v.H + 2 * ph, v.W + 2 * pw, v.C};
  const long per = voxels(vp) * v.C, total = n * voxels(v) * v.C;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const Pos p = split(e, v);
    const float* src = yp + p.s * per;
    const int nd = pad_preimages(p.d, v.D, pd, mode), nh = pad_preimages(p.h, v.H, ph, mode), nw = pad_preimages(p.w, v.W, pw, mode);
    float acc = 0.f;
    for (int a = 0; a < nd; ++a) {
      const int od = pad_preimage(a, p.d, v.D, pd, mode);
      for (int b = 0; b < nh; ++b) {
        const int oh = pad_preimage(b, p.h, v.H, ph, mode);
        for (int g = 0; g < nw; ++g) acc += src[at(vp, od, oh, pad_preimage(g, p.w, v.W, pw, mode), p.c)];
      }
    }
    x[e] = acc;
  }
}

// max over windows of (wd, wh, ww) voxels (each 1 or 2), stride = window, floor: a trailing odd plane / row / column is
// dropped.  MaxPool2d(2) is the window (1, 2, 2); IMAGE: that window known at compile time (its four loads issue together).
template <bool IMAGE>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const float* x, long n, Vol v, int wd_, int wh_, int ww_, float* y) {
  const int wd = IMAGE ? 1 : wd_, wh = IMAGE ? 2 : wh_, ww = IMAGE ? 2 : ww_;
  const Vol vo = {v.D / wd, v.H / wh, v.W / ww, v.C};
  const long per = voxels(v) * v.C, total = n * voxels(vo) * v.C;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const Pos p = split(e, vo);
    const float* src = x + p.s * per;
    float m = 0.f;
    int idx = 0;
    for (int i = 0; i < wd; ++i)
      for (int j = 0; j < wh; ++j)
        for (int k = 0; k < ww; ++k, ++idx) {
          const float val = src[at(v, p.d * wd + i, p.h * wh + j, p.w * ww + k, p.c)];
          m = idx ? fmaxf(m, val) : val;
        }
    y[e] = m;
  }
}
// dx = route(dy) to the FIRST maximum of each window in (d, h, w) scan order (torch's rule: a later element wins only if
// strictly greater), times act'(x) of the activation that produced x (dact 1 relu, 2 tanh, 0 none); voxels no window
// covers get 0
template <bool IMAGE>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* dy, const float* x, long n, Vol v, int wd_, int wh_, int ww_,
                                                          int dact, float* dx) {
  const int wd = IMAGE ? 1 : wd_, wh = IMAGE ? 2 : wh_, ww = IMAGE ? 2 : ww_;
  const Vol vo = {v.D / wd, v.H / wh, v.W / ww, v.C};
  const long per = voxels(v) * v.C, total = n * per;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const Pos p = split(e, v);
    const int z = p.d / wd, a = p.h / wh, b = p.w / ww;
    float g = 0.f;
    if (z < vo.D && a < vo.H && b < vo.W) {
      const float* src = x + p.s * per;
      float m = -INFINITY;
      int arg = -1, idx = 0;
      for (int i = 0; i < wd; ++i)
        for (int j = 0; j < wh; ++j)
          for (int k = 0; k < ww; ++k, ++idx) {
            const float val = src[at(v, z * wd + i, a * wh + j, b * ww + k, p.c)];
            if (arg < 0 || val > m) { m = val; arg = idx; }
          }
      const int mine = ((p.d - z * wd) * wh + (p.h - a * wh)) * ww + (p.w - b * ww);
      if (arg == mine) g = dy[p.s * (voxels(vo) * v.C) + at(vo, z, a, b, p.c)];
    }
    dx[e] = g * act_grad_from_output(x[e], dact);
  }
}

// P[(s, od, oh, ow)][(kd, kh, kw, c)] = x[s, od S + kd, oh S + kh, ow S + kw, c]   (V = 4: float4 along c, V = 1: any C)
template <int V>
__global__ __launch_bounds__(256) void im2col_kernel(const float* x, long n, Vol v, int KD, int KH, int KW, int S, Vol vo, float* P) {
  const int CV = v.C / V;
  const Vol rows = {vo.D, vo.H, vo.W, vo.C / V};  // P ([n] x vo, vo.C = KD KH KW C floats per row) in units of V floats
  const long per = voxels(v) * v.C, total = n * voxels(rows) * rows.C;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const Pos p = split(e, rows);
    unsigned k = p.c;
    const int cv = k % (unsigned)CV; k /= (unsigned)CV;
    const int kw = k % (unsigned)KW; k /= (unsigned)KW;
    const int kh = k % (unsigned)KH;
    const int kd = k / (unsigned)KH;
    const float* src = x + p.s * per + at(v, p.d * S + kd, p.h * S + kh, p.w * S + kw, cv * V);
    if (V == 4) *reinterpret_cast<float4*>(P + e * 4) = *reinterpret_cast<const float4*>(src);
    else P[e] = src[0];
  }
}
// Gather form of the adjoint: dX[s, d, h, w, c] = sum over the taps that reach the voxel ((d - kd) % S == 0, ..., in range;
// kd, kh, kw ascending) of dP[(s, od, oh, ow)][(kd, kh, kw, c)]   (* act'(y))
template <int V>
__global__ __launch_bounds__(256) void col2im_kernel(const float* dP, long n, Vol v, int KD, int KH, int KW, int S, Vol vo,
                                                     const float* y, int dact, float* dX) {
  const Vol vv = {v.D, v.H, v.W, v.C / V};  // dX in units of V floats
  const long per = voxels(vo) * vo.C, total = n * voxels(vv) * vv.C;  // dP: [n] x vo, vo.C = KD KH KW C floats per row
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const Pos p = split(e, vv);
    const float* rows_s = dP + p.s * per;
    float acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.f;
    // along an axis the taps k = d % S, d % S + S, ... reach the outputs o = (d - k) / S = d / S, d / S - 1, ... >= 0
    for (int kd = p.d % S, od = p.d / S; kd < KD && od >= 0; kd += S, --od) {
      if (od >= vo.D) continue;
      for (int kh = p.h % S, oh = p.h / S; kh < KH && oh >= 0; kh += S, --oh) {
        if (oh >= vo.H) continue;
        for (int kw = p.w % S, ow = p.w / S; kw < KW && ow >= 0; kw += S, --ow) {
          if (ow >= vo.W) continue;
          const float* src = rows_s + at(vo, od, oh, ow,((kd * KH + kh) * KW + kw) * v.C + p.c * V);
          if (V == 4) {
            const float4 q = *reinterpret_cast<const float4*>(src);
            acc[0] += q.x; acc[1 % V] += q.y; acc[2 % V] += q.z; acc[3 % V] += q.w;
          } else {
            acc[0] += src[0];
          }
        }
      }
    }
    if (y && dact) {
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] *= act_grad_from_output(y[e * V + j], dact);
    }
    if (V == 4) *reinterpret_cast<float4*>(dX + e * 4) = make_float4(acc[0], acc[1 % V], acc[2 % V], acc[3 % V]);
    else dX[e] = acc[0];
  }
}

}  // namespace

extern "C" int srl_obs_ln_nhwc(void* stream, const void* obs, int is_u8, const float* mean, const float* rstd,
                               const float* gamma, const float* beta, int64_t n, int C, int H, int W, float* y) {
  SRL_CHECK_ARG(obs && mean && rstd && gamma && beta && y && C >= 1 && H >= 1 && W >= 1, "null tensor / bad shape");
  if (n == 0) return 0;
  const long total = n * C * H * W;
  if (is_u8) hipLaunchKernelGGL(obs_ln_nhwc_kernel<true>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, obs, mean, rstd, gamma, beta, (long)n, C, H, W, y);
  else hipLaunchKernelGGL(obs_ln_nhwc_kernel<false>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, obs, mean, rstd, gamma, beta, (long)n, C, H, W, y);
  SRL_LAUNCH_CHECK();
  return 0;
}

extern "C" int srl_obs_ln_nhwc_bwd(void* stream, const float* dy, const void* obs, int is_u8, const float* mean,
                                   const float* rstd, int64_t n, int C, int H, int W, float* dgamma, float* dbeta) {
  SRL_CHECK_ARG(dy && obs && mean && rstd && dgamma && dbeta, "null tensor");
  if (n == 0) return 0;
  const int D = C * H * W;
  if (is_u8) hipLaunchKernelGGL(obs_ln_nhwc_bwd_kernel<true>, dim3((unsigned)srl_ceil_div(D, 256)), dim3(256), 0, (hipStream_t)stream, dy, obs, mean, rstd, (long)n, C, H, W, dgamma, dbeta);
  else hipLaunchKernelGGL(obs_ln_nhwc_bwd_kernel<false>, dim3((unsigned)srl_ceil_div(D, 256)), dim3(256), 0, (hipStream_t)stream, dy, obs, mean, rstd, (long)n, C, H, W, dgamma, dbeta);
  SRL_LAUNCH_CHECK();
  return 0;
}

// Workgroups of the pad / crop / pool passes (grid-stride beyond): one resident round of the chip.  A wavefront's prologue --
// the reciprocals of `split`'s divisors -- is as long as one element's work, so a thread takes several elements of a large
// tensor (n = 512, 20 x 20 x 32: pad 32.6 -> 26.4 us).  The two patch-matrix passes, bound by their loads, keep the grid they had.
constexpr long kVolGridCap = 2048, kPatchGridCap = 16384;

// a sample of fewer than 2^31 elements: what `split` and `at` assume
static bool vol_ok(Vol v) { return v.D >= 1 && v.H >= 1 && v.W >= 1 && v.C >= 1 && voxels(v) * v.C <= 0x7fffffffL; }

constexpr int kMaxPad = 8;  // per side: the encoders' limit (netspec._pad_mode)
// nn.ConvNd's own preconditions: reflect needs pad < extent, circular pad <= extent (torch raises otherwise)
static bool pad_ok(Vol v, int pd, int ph, int pw, int mode) {
  if (pd < 0 || ph < 0 || pw < 0 || mode < 0 || mode > 3 || pd > kMaxPad || ph > kMaxPad || pw > kMaxPad) return false;
  if (mode == 1 && !(pd < v.D && ph < v.H && pw < v.W)) return false;
  if (mode == 3 && !(pd <= v.D && ph <= v.H && pw <= v.W)) return false;
  return vol_ok(Vol{v.D + 2 * pd, v.H + 2 * ph, v.W + 2 * pw, v.C});
}

extern "C" int srl_pad_ndhwc(void* stream, const float* x, int64_t n, int D, int H, int W, int C, int pd, int ph, int pw, int mode,
                             float* y) {
  const Vol v = {D, H, W, C};
  SRL_CHECK_ARG(x && y && vol_ok(v) && pad_ok(v, pd, ph, pw, mode), "null tensor / bad shape / padding too wide");
  if (n == 0) return 0;
  const long total = n * (D + 2 * pd) * (H + 2 * ph) * (W + 2 * pw) * C;
  hipLaunchKernelGGL(mode == 0 ? pad_kernel<true> : pad_kernel<false>, dim3(grid_for(total, kVolGridCap)), dim3(256), 0, (hipStream_t)stream, x, (long)n, v, pd, ph, pw, mode, y);
  SRL_LAUNCH_CHECK();
  return 0;
}

extern "C" int srl_crop_ndhwc(void* stream, const float* yp, int64_t n, int D, int H, int W, int C, int pd, int ph, int pw, int mode,
                              float* x) {
  const Vol v = {D, H, W, C};
  SRL_CHECK_ARG(x && yp && vol_ok(v) && pad_ok(v, pd, ph, pw, mode), "null tensor / bad shape / padding too wide");
  if (n == 0) return 0;
  hipLaunchKernelGGL(mode == 0 ? crop_kernel<true> : crop_kernel<false>, dim3(grid_for(n * voxels(v) * C, kVolGridCap)), dim3(256), 0, (hipStream_t)stream, yp, (long)n, v, pd, ph, pw, mode, x);
  SRL_LAUNCH_CHECK();
  return 0;
}

static bool image_win(int wd, int wh, int ww) { return wd == 1 && wh == 2 && ww == 2; }
static bool win_ok(Vol v, int wd, int wh, int ww) {
  return (wd == 1 || wd == 2) && (wh == 1 || wh == 2) && (ww == 1 || ww == 2) && v.D >= wd && v.H >= wh && v.W >= ww;
}

extern "C" int srl_maxpool_ndhwc_fwd(void* stream, const float* x, int64_t n, int D, int H, int W, int C, int wd, int wh, int ww,
                                     float* y) {
  const Vol v = {D, H, W, C};
  SRL_CHECK_ARG(x && y && vol_ok(v) && win_ok(v, wd, wh, ww), "null tensor / volume smaller than the window");
  if (n == 0) return 0;
  const long total = n * (D / wd) * (H / wh) * (W / ww) * C;
  hipLaunchKernelGGL(image_win(wd, wh, ww) ? maxpool_fwd_kernel<true> : maxpool_fwd_kernel<false>, dim3(grid_for(total, kVolGridCap)), dim3(256), 0, (hipStream_t)stream, x, (long)n, v, wd, wh, ww, y);
  SRL_LAUNCH_CHECK();
  return 0;
}

extern "C" int srl_maxpool_ndhwc_bwd(void* stream, const float* dy, const float* x, int64_t n, int D, int H, int W, int C, int wd,
                                     int wh, int ww, int dact, float* dx) {
  const Vol v = {D, H, W, C};
  SRL_CHECK_ARG(dy && x && dx && vol_ok(v) && win_ok(v, wd, wh, ww) && dact >= 0 && dact <= 2, "null tensor / bad argument");
  if (n == 0) return 0;
  hipLaunchKernelGGL(image_win(wd, wh, ww) ? maxpool_bwd_kernel<true> : maxpool_bwd_kernel<false>, dim3(grid_for(n * voxels(v) * C, kVolGridCap)), dim3(256), 0, (hipStream_t)stream, dy, x, (long)n, v, wd, wh,
                     ww, dact, dx);
  SRL_LAUNCH_CHECK();
  return 0;
}

// the output volume of a convolution's patches (C: floats per patch row) in *vo; false for a geometry that has none, or whose
// patch matrix of one sample reaches 2^31 elements
static bool patch_ok(Vol v, int KD, int KH, int KW, int stride, Vol* vo) {
  if (!(vol_ok(v) && KD >= 1 && KH >= 1 && KW >= 1 && KD <= v.D && KH <= v.H && KW <= v.W && stride >= 1)) return false;
  const long kp = (long)KD * KH * KW * v.C;
  if (kp > 0x7fffffffL) return false;
  *vo = Vol{(v.D - KD) / stride + 1, (v.H - KH) / stride + 1, (v.W - KW) / stride + 1, (int)kp};
  return vol_ok(*vo);
}

// float4 along c whenever C is a multiple of 4: every row of x, P and dX then starts a multiple of 4 floats into its tensor
extern "C" int srl_im2col_ndhwc(void* stream, const float* x, int64_t n, int D, int H, int W, int C, int KD, int KH, int KW, int stride,
                                float* P) {
  const Vol v = {D, H, W, C};
  Vol vo;
  SRL_CHECK_ARG(x && P && patch_ok(v, KD, KH, KW, stride, &vo), "null tensor / invalid geometry");
  if (n == 0) return 0;
  const int V = C % 4 == 0 ? 4 : 1;
  const auto kernel = V == 4 ? im2col_kernel<4> : im2col_kernel<1>;
  hipLaunchKernelGGL(kernel, dim3(grid_for(n * voxels(vo) * (vo.C / V), kPatchGridCap)), dim3(256), 0, (hipStream_t)stream, x, (long)n, v,
                     KD, KH, KW, stride, vo, P);
  SRL_LAUNCH_CHECK();
  return 0;
}

extern "C" int srl_col2im_ndhwc(void* stream, const float* dP, int64_t n, int D, int H, int W, int C, int KD, int KH, int KW, int stride,
                                const float* y, int dact, float* dX) {
  const Vol v = {D, H, W, C};
  Vol vo;
  SRL_CHECK_ARG(dP && dX && patch_ok(v, KD, KH, KW, stride, &vo) && dact >= 0 && dact <= 2, "null tensor / invalid geometry");
  if (n == 0) return 0;
  const int V = C % 4 == 0 ? 4 : 1;
  const auto kernel = V == 4 ? col2im_kernel<4> : col2im_kernel<1>;
  hipLaunchKernelGGL(kernel, dim3(grid_for(n * voxels(v) * (C / V), kPatchGridCap)), dim3(256), 0, (hipStream_t)stream, dP, (long)n, v, KD,
                     KH, KW, stride, vo, y, dact, dX);
  SRL_LAUNCH_CHECK();
  return 0;
}
