// Agent-specific attention encoder of SMACNet in one launch per direction (include/srl_hip.h: srl_entity_attn_*).
//
// Reference: SMACAgentwiseObsEncoder / SMACAgentwiseEncoder (legacy/algorithm/ppo/game_policies/smac_rnn.py:29-84) with
// CatSelfEmbedding, MultiHeadSelfAttention and masked_avg_pooling (legacy/algorithm/modules/attention.py:7-92,116-122).
//
// A workgroup of 1024 threads walks tiles of R rows (a persistent grid); everything of a tile lives in LDS, float32:
//   a      [R][S + sum n_k f_k]   the LayerNorm'ed inputs (affine applied); backward: later the gradients w.r.t. them
//   xhat   [R][S + sum n_k f_k]   backward only: the normalised inputs before the affine
//   emb    [R][E][D+1]            relu(W_k cat(a_self, a_e) + b_k)
//   xn     [R][E][D+1]            pre_norm(emb)
//   q k v  [R][E][D+1]            backward: q is reused for d xn, k for d z (the embeddings' pre-activation gradient)
//   dq dk  [R][E][D+1]            backward only
//   misc   [R][...]               mask, pooling weights, pre_norm statistics, softmax statistics, self embedding, ...
// The pooled output only needs  w[h][j] = sum_i c_i p[h][i][j]  (c_i = mask_i / (sum mask + 1e-5)):  pooled^h = sum_j w[h][j] v_j^h,
// so the probabilities are never stored: a thread per (head, query) finds the row maximum and the normaliser, a thread per (head,
// key) then sums its column.  Backward: d out_i = c_i d pooled, hence d p[h][i][j] = c_i t[h][j] with t[h][j] = d pooled^h . v_j^h,
// d s[h][i][j] = c_i p (t[h][j] - tbar[h][i]), d v_j^h = w[h][j] d pooled^h (formed where it is used, not stored).
// NO TAPE: the backward kernel walks forward again from the observation leaves; nothing is kept between the two calls.
//
// Parameters are staged in LDS once per workgroup (matrices transposed, leading dimension D + 1: conflict-free both for the
// product and for its transpose) and the parameter gradients are summed there over the workgroup's tiles and added to global
// memory once, with float atomics -- when they fit beside one row's intermediates in 160 KiB; otherwise the parameters are read
// from global memory and / or every tile adds its sums with atomics.
#include "srl_common.h"

namespace {

constexpr int kThreads = 1024;  // 16 wavefronts: the phases are chains of dependent LDS reads, four per SIMD hide each other
constexpr int kHeads = 4;
constexpr int kLdsFloats = 160 * 1024 / 4;
constexpr int NS = SRL_EATTN_SLOTS;

struct EaPlan {
  int R;                 // rows per tile
  int stage_p, stage_g;  // parameters / gradient sums in LDS
  int n[NS];             // elements per slot (0: absent)
  int rows_[NS];         // matrices: number of input columns (else 0)
  int poff[NS];          // offset of the staged slot (matrices: [in][D + 1])
  int goff[NS];          // offset of the slot's gradient sums (global layout)
  int in_row, koff[3], ent0[3];
  int o_par, o_grad, o_a, o_xhat, o_emb, o_xn, o_q, o_k, o_v, o_dq, o_dk, o_misc;
  int misc_row;
  int total;
};

struct EaArgs {
  srl_entity_attn d;
  EaPlan pl;
  int64_t rows;
  float* out;
  int64_t ldo;
  const float* dout;
  int64_t lddo;
};

bool valid_shape(const srl_entity_attn* d) {
  if (!d || (d->D != 16 && d->D != 32 && d->D != 64) || d->S < 1 || d->S > 128 || d->nkeys < 1 || d->nkeys > SRL_EATTN_MAX_KEYS) return false;
  int e = 0;
  for (int k = 0; k < d->nkeys; ++k) {
    if (d->cnt[k] < 1 || d->f[k] < 1 || d->f[k] > 64) return false;
    e += d->cnt[k];
  }
  return e == d->E && e <= 64;
}

bool make_plan(const srl_entity_attn& d, bool bwd, EaPlan* p) {
  const int D = d.D, S = d.S, E = d.E, DP = D + 1;
  memset(p, 0, sizeof(*p));
  auto vec = [&](int s, int n) { p->n[s] = n; };
  auto mat = [&](int s, int in) { p->n[s] = D * in; p->rows_[s] = in; };
  vec(SRL_EATTN_LN_SELF_W, S); vec(SRL_EATTN_LN_SELF_B, S);
  mat(SRL_EATTN_SELF_W, S); vec(SRL_EATTN_SELF_B, D);
  int off = S, e0 = 0;
  for (int k = 0; k < 3; ++k) { p->ent0[k] = 1 << 20; }
  for (int k = 0; k < d.nkeys; ++k) {
    vec(SRL_EATTN_LN_KEY_W + k, d.f[k]); vec(SRL_EATTN_LN_KEY_B + k, d.f[k]);
    mat(SRL_EATTN_KEY_W + k, S + d.f[k]); vec(SRL_EATTN_KEY_B + k, D);
    p->koff[k] = off; p->ent0[k] = e0;
    off += d.cnt[k] * d.f[k]; e0 += d.cnt[k];
  }
  p->in_row = off;
  vec(SRL_EATTN_PRE_W, D); vec(SRL_EATTN_PRE_B, D);
  for (int s = SRL_EATTN_Q_W; s <= SRL_EATTN_V_W; s += 2) { mat(s, D); vec(s + 1, D); }
  int np = 0, ng = 0;
  for (int s = 0; s < NS; ++s) {
    p->poff[s] = np; p->goff[s] = ng;
    np += p->rows_[s] ? p->rows_[s] * DP : p->n[s];
    ng += p->n[s];
  }
  p->misc_row = 24 * E + 3 * D + S;
  const int per_row = p->in_row * (bwd ? 2 : 1) + (bwd ? 7 : 5) * E * DP + p->misc_row;
  if (per_row > kLdsFloats) return false;
  int fixed = 0;
  if (np + (bwd ? ng : 0) + per_row <= kLdsFloats) { p->stage_p = 1; p->stage_g = bwd; fixed = np + (bwd ? ng : 0); }
  else if (np + per_row <= kLdsFloats) { p->stage_p = 1; fixed = np; }
  int want = 4096 / (E * D);   // enough (row, entity, feature) items for 1024 threads
  want = want < 1 ? 1 : (want > 16 ? 16 : want);
  int fit = (kLdsFloats - fixed) / per_row;
  p->R = want < fit ? want : fit;
  const int R = p->R;
  int o = 0;
  p->o_par = o; o += p->stage_p ? np : 0;
  p->o_grad = o; o += p->stage_g ? ng : 0;
  p->o_a = o; o += R * p->in_row;
  p->o_xhat = o; o += bwd ? R * p->in_row : 0;
  p->o_emb = o; o += R * E * DP;
  p->o_xn = o; o += R * E * DP;
  p->o_q = o; o += R * E * DP;
  p->o_k = o; o += R * E * DP;
  p->o_v = o; o += R * E * DP;
  p->o_dq = o; o += bwd ? R * E * DP : 0;
  p->o_dk = o; o += bwd ? R * E * DP : 0;
  p->o_misc = o; o += R * p->misc_row;
  p->total = o;
  return o <= kLdsFloats;
}

// element (d, j) of a [D, in] matrix: staged (transposed, leading dimension D + 1) or in global memory (row-major)
struct Mat {
  const float* p;
  int sd, sj;
  __device__ __forceinline__ float operator()(int d, int j) const { return p[d * sd + j * sj]; }
};

template <int DH, bool BWD>
__global__ void __launch_bounds__(kThreads) entity_attn_kernel(const EaArgs A) {
  extern __shared__ float lds[];
  const srl_entity_attn& d = A.d;
  const EaPlan& pl = A.pl;
  const int D = d.D, S = d.S, E = d.E, DP = D + 1, R = pl.R, NT = kThreads, tid = threadIdx.x;
  const int in_row = pl.in_row, MR = pl.misc_row, E1 = E + 1;
  const float scale = 1.0f / sqrtf((float)DH);

  // ---- stage the parameters, clear the gradient sums
  if (pl.stage_p) {
    for (int s = 0; s < NS; ++s) {
      const int n = pl.n[s], in = pl.rows_[s];
      const float* src = d.p[s];
      float* dst = lds + pl.o_par + pl.poff[s];
      if (in) {
        for (int i = tid; i < n; i += NT) dst[(i % in) * DP + i / in] = src[i];
      } else {
        for (int i = tid; i < n; i += NT) dst[i] = src[i];
      }
    }
  }
  if (BWD && pl.stage_g) {
    const int ng = pl.goff[NS - 1] + pl.n[NS - 1];
    for (int i = tid; i < ng; i += NT) lds[pl.o_grad + i] = 0.0f;
  }
  __syncthreads();
  auto vecp = [&](int s) -> const float* { return pl.stage_p ? lds + pl.o_par + pl.poff[s] : d.p[s]; };
  auto matp = [&](int s) -> Mat {
    if (pl.stage_p) return Mat{lds + pl.o_par + pl.poff[s], 1, DP};
    return Mat{d.p[s], pl.rows_[s], 1};
  };
  // g[s][i] += v: the workgroup's sum in LDS (every element has one owner per phase) or straight to global memory
  auto gadd = [&](int s, int i, float v) {
    if (pl.stage_g) lds[pl.o_grad + pl.goff[s] + i] += v;
    else atomicAdd(d.g[s] + i, v);
  };
  auto key_of = [&](int e) -> int { return (e >= pl.ent0[1] ? 1 : 0) + (e >= pl.ent0[2] ? 1 : 0); };

  float* a_ = lds + pl.o_a;
  float* xh_ = lds + pl.o_xhat;
  float* emb_ = lds + pl.o_emb;
  float* xn_ = lds + pl.o_xn;
  float* q_ = lds + pl.o_q;
  float* k_ = lds + pl.o_k;
  float* v_ = lds + pl.o_v;
  float* dq_ = lds + pl.o_dq;
  float* dk_ = lds + pl.o_dk;
  float* misc = lds + pl.o_misc;
  // per-row misc: m[E] c[E] mean[E] rstd[E] | smax sinv wsum t tbar [4E each] | selfemb[D] dzs[D] dpool[D] | (S spare)
  auto m_ = [&](int r) { return misc + r * MR; };
  auto c_ = [&](int r) { return misc + r * MR + E; };
  auto mean_ = [&](int r) { return misc + r * MR + 2 * E; };
  auto rstd_ = [&](int r) { return misc + r * MR + 3 * E; };
  auto smax_ = [&](int r) { return misc + r * MR + 4 * E; };
  auto sinv_ = [&](int r) { return misc + r * MR + 8 * E; };
  auto wsum_ = [&](int r) { return misc + r * MR + 12 * E; };
  auto t_ = [&](int r) { return misc + r * MR + 16 * E; };
  auto tbar_ = [&](int r) { return misc + r * MR + 20 * E; };
  auto semb_ = [&](int r) { return misc + r * MR + 24 * E; };
  auto dzs_ = [&](int r) { return misc + r * MR + 24 * E + D; };
  auto dpool_ = [&](int r) { return misc + r * MR + 24 * E + 2 * D; };

  const int64_t ntiles = (A.rows + R - 1) / R;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * R;
    const int nv = (int)((A.rows - row0) < R ? (A.rows - row0) : R);   // rows of this tile (rows past the end are never touched)

    // ---- phase 0: leaves -> LDS
    for (int i = tid; i < nv * S; i += NT) {
      const int r = i / S, j = i % S;
      a_[r * in_row + j] = d.x_self[(row0 + r) * d.ld_self + j];
    }
    for (int k = 0; k < d.nkeys; ++k) {
      const int nk = d.cnt[k] * d.f[k];
      for (int i = tid; i < nv * nk; i += NT) {
        const int r = i / nk, j = i % nk;
        a_[r * in_row + pl.koff[k] + j] = d.x_key[k][(row0 + r) * d.ld_key[k] + j];
      }
    }
    for (int i = tid; i < nv * E; i += NT) {
      const int r = i / E, e = i % E;
      m_(r)[e] = d.mask[(row0 + r) * d.ld_mask + e] ? 1.0f : 0.0f;
    }
    if (BWD) {
      for (int i = tid; i < nv * D; i += NT) {
        const int r = i / D, c = i % D;
        dpool_(r)[c] = A.dout[(row0 + r) * A.lddo + D + c];
      }
    }
    __syncthreads();

    // ---- phase 0b: LayerNorm of the self vector and of every entity (one thread per vector); pooling weights
    for (int u = tid; u < nv * E1; u += NT) {
      const int r = u / E1, ee = u % E1;
      int off, len, sw, sb;
      if (ee == 0) {
        off = 0; len = S; sw = SRL_EATTN_LN_SELF_W; sb = SRL_EATTN_LN_SELF_B;
      } else {
        const int e = ee - 1, k = key_of(e);
        off = pl.koff[k] + (e - pl.ent0[k]) * d.f[k]; len = d.f[k]; sw = SRL_EATTN_LN_KEY_W + k; sb = SRL_EATTN_LN_KEY_B + k;
      }
      float* x = a_ + r * in_row + off;
      const float *w = vecp(sw), *b = vecp(sb);
      float mu = 0.0f;
      for (int j = 0; j < len; ++j) mu += x[j];
      mu /= (float)len;
      float var = 0.0f;
      for (int j = 0; j < len; ++j) { const float t = x[j] - mu; var = fmaf(t, t, var); }
      const float rs = 1.0f / sqrtf(var / (float)len + 1e-5f);
      for (int j = 0; j < len; ++j) {
        const float h = (x[j] - mu) * rs;
        if (BWD) xh_[r * in_row + off + j] = h;
        x[j] = fmaf(h, w[j], b[j]);
      }
    }
    for (int i = tid; i < nv * E; i += NT) {
      const int r = i / E, e = i % E;
      float ms = 0.0f;
      for (int j = 0; j < E; ++j) ms += m_(r)[j];
      c_(r)[e] = m_(r)[e] / (ms + 1e-5f);
    }
    __syncthreads();

    // ---- phase 1: embeddings
    for (int i = tid; i < nv * E1 * D; i += NT) {
      const int dd = i % D, u = i / D, r = u / E1, ee = u % E1;
      const float* as = a_ + r * in_row;
      if (ee == 0) {
        const Mat W = matp(SRL_EATTN_SELF_W);
        float z = vecp(SRL_EATTN_SELF_B)[dd];
        for (int j = 0; j < S; ++j) z = fmaf(W(dd, j), as[j], z);
        z = fmaxf(z, 0.0f);
        semb_(r)[dd] = z;
        if (BWD) dzs_(r)[dd] = z > 0.0f ? A.dout[(row0 + r) * A.lddo + dd] : 0.0f;
        else A.out[(row0 + r) * A.ldo + dd] = z;
      } else {
        const int e = ee - 1, k = key_of(e), f = d.f[k];
        const Mat W = matp(SRL_EATTN_KEY_W + k);
        const float* ae = as + pl.koff[k] + (e - pl.ent0[k]) * f;
        float z = vecp(SRL_EATTN_KEY_B + k)[dd];
        for (int j = 0; j < S; ++j) z = fmaf(W(dd, j), as[j], z);
        for (int j = 0; j < f; ++j) z = fmaf(W(dd, S + j), ae[j], z);
        emb_[(r * E + e) * DP + dd] = fmaxf(z, 0.0f);
      }
    }
    __syncthreads();

    // ---- phase 2: pre_norm (one thread per entity)
    for (int u = tid; u < nv * E; u += NT) {
      const int r = u / E, e = u % E;
      const float* x = emb_ + u * DP;
      const float *w = vecp(SRL_EATTN_PRE_W), *b = vecp(SRL_EATTN_PRE_B);
      float mu = 0.0f;
      for (int c = 0; c < D; ++c) mu += x[c];
      mu /= (float)D;
      float var = 0.0f;
      for (int c = 0; c < D; ++c) { const float t = x[c] - mu; var = fmaf(t, t, var); }
      const float rs = 1.0f / sqrtf(var / (float)D + 1e-5f);
      mean_(r)[e] = mu;
      rstd_(r)[e] = rs;
      for (int c = 0; c < D; ++c) xn_[u * DP + c] = fmaf((x[c] - mu) * rs, w[c], b[c]);
    }
    __syncthreads();

    // ---- phase 3: q, k, v
    {
      const Mat Wq = matp(SRL_EATTN_Q_W), Wk = matp(SRL_EATTN_K_W), Wv = matp(SRL_EATTN_V_W);
      const float *bq = vecp(SRL_EATTN_Q_B), *bk = vecp(SRL_EATTN_K_B), *bv = vecp(SRL_EATTN_V_B);
      for (int i = tid; i < nv * E * D; i += NT) {
        const int dd = i % D, u = i / D;
        const float* x = xn_ + u * DP;
        float q = bq[dd], k = bk[dd], v = bv[dd];
        for (int c = 0; c < D; ++c) {
          const float xc = x[c];
          q = fmaf(Wq(dd, c), xc, q);
          k = fmaf(Wk(dd, c), xc, k);
          v = fmaf(Wv(dd, c), xc, v);
        }
        q_[u * DP + dd] = q; k_[u * DP + dd] = k; v_[u * DP + dd] = v;
      }
    }
    __syncthreads();

    // ---- phase 4: per (head, query): maximum and normaliser of the scores over the unmasked keys
    for (int i = tid; i < nv * kHeads * E; i += NT) {
      const int qi = i % E, h = (i / E) % kHeads, r = i / (E * kHeads);
      float qv[DH];
#pragma unroll
      for (int t = 0; t < DH; ++t) qv[t] = q_[(r * E + qi) * DP + h * DH + t];
      const float* m = m_(r);
      float mx = -INFINITY;
      for (int j = 0; j < E; ++j) {
        if (m[j] == 0.0f) continue;
        const float* kj = k_ + (r * E + j) * DP + h * DH;
        float s = 0.0f;
#pragma unroll
        for (int t = 0; t < DH; ++t) s = fmaf(qv[t], kj[t], s);
        mx = fmaxf(mx, s * scale);
      }
      float sum = 0.0f;
      for (int j = 0; j < E; ++j) {
        if (m[j] == 0.0f) continue;
        const float* kj = k_ + (r * E + j) * DP + h * DH;
        float s = 0.0f;
#pragma unroll
        for (int t = 0; t < DH; ++t) s = fmaf(qv[t], kj[t], s);
        sum += expf(s * scale - mx);
      }
      smax_(r)[h * E + qi] = mx;
      sinv_(r)[h * E + qi] = sum > 0.0f ? 1.0f / sum : 0.0f;
    }
    __syncthreads();

    // ---- phase 5: per (head, key): w = sum_i c_i p[i][key]; backward: t = d pooled^h . v_key^h
    for (int i = tid; i < nv * kHeads * E; i += NT) {
      const int kj = i % E, h = (i / E) % kHeads, r = i / (E * kHeads);
      float w = 0.0f, tt = 0.0f;
      if (m_(r)[kj] != 0.0f) {
        float kv[DH];
#pragma unroll
        for (int t = 0; t < DH; ++t) kv[t] = k_[(r * E + kj) * DP + h * DH + t];
        const float* c = c_(r);
        for (int qi = 0; qi < E; ++qi) {
          if (c[qi] == 0.0f) continue;
          const float* qq = q_ + (r * E + qi) * DP + h * DH;
          float s = 0.0f;
#pragma unroll
          for (int t = 0; t < DH; ++t) s = fmaf(qq[t], kv[t], s);
          w = fmaf(c[qi], expf(s * scale - smax_(r)[h * E + qi]) * sinv_(r)[h * E + qi], w);
        }
        if (BWD) {
#pragma unroll
          for (int t = 0; t < DH; ++t) tt = fmaf(dpool_(r)[h * DH + t], v_[(r * E + kj) * DP + h * DH + t], tt);
        }
      }
      wsum_(r)[h * E + kj] = w;
      if (BWD) t_(r)[h * E + kj] = tt;
    }
    __syncthreads();

    if (!BWD) {
      // ---- phase 6: pooled = sum_j w[h][j] v_j
      for (int i = tid; i < nv * D; i += NT) {
        const int r = i / D, dd = i % D, h = dd / DH;
        float acc = 0.0f;
        for (int j = 0; j < E; ++j) acc = fmaf(wsum_(r)[h * E + j], v_[(r * E + j) * DP + dd], acc);
        A.out[(row0 + r) * A.ldo + D + dd] = acc;
      }
      __syncthreads();   // the next tile overwrites the row buffers
      continue;
    }

    // ---- phase 7: per (head, query): tbar = sum_j p t_j, d q = scale sum_j c p (t_j - tbar) k_j
    for (int i = tid; i < nv * kHeads * E; i += NT) {
      const int qi = i % E, h = (i / E) % kHeads, r = i / (E * kHeads);
      float dq[DH];
#pragma unroll
      for (int t = 0; t < DH; ++t) dq[t] = 0.0f;
      float tb = 0.0f;
      const float ci = c_(r)[qi];
      if (ci != 0.0f) {
        float qv[DH];
#pragma unroll
        for (int t = 0; t < DH; ++t) qv[t] = q_[(r * E + qi) * DP + h * DH + t];
        const float* m = m_(r);
        const float mx = smax_(r)[h * E + qi], inv = sinv_(r)[h * E + qi];
        for (int j = 0; j < E; ++j) {
          if (m[j] == 0.0f) continue;
          const float* kj = k_ + (r * E + j) * DP + h * DH;
          float s = 0.0f;
#pragma unroll
          for (int t = 0; t < DH; ++t) s = fmaf(qv[t], kj[t], s);
          tb = fmaf(expf(s * scale - mx) * inv, t_(r)[h * E + j], tb);
        }
        for (int j = 0; j < E; ++j) {
          if (m[j] == 0.0f) continue;
          const float* kj = k_ + (r * E + j) * DP + h * DH;
          float s = 0.0f;
#pragma unroll
          for (int t = 0; t < DH; ++t) s = fmaf(qv[t], kj[t], s);
          const float ds = ci * expf(s * scale - mx) * inv * (t_(r)[h * E + j] - tb) * scale;
#pragma unroll
          for (int t = 0; t < DH; ++t) dq[t] = fmaf(ds, kj[t], dq[t]);
        }
      }
      tbar_(r)[h * E + qi] = tb;
#pragma unroll
      for (int t = 0; t < DH; ++t) dq_[(r * E + qi) * DP + h * DH + t] = dq[t];
    }
    __syncthreads();

    // ---- phase 8: per (head, key): d k = scale sum_i c_i p (t_key - tbar_i) q_i
    for (int i = tid; i < nv * kHeads * E; i += NT) {
      const int kj = i % E, h = (i / E) % kHeads, r = i / (E * kHeads);
      float dk[DH];
#pragma unroll
      for (int t = 0; t < DH; ++t) dk[t] = 0.0f;
      if (m_(r)[kj] != 0.0f) {
        float kv[DH];
#pragma unroll
        for (int t = 0; t < DH; ++t) kv[t] = k_[(r * E + kj) * DP + h * DH + t];
        const float* c = c_(r);
        const float tj = t_(r)[h * E + kj];
        for (int qi = 0; qi < E; ++qi) {
          if (c[qi] == 0.0f) continue;
          const float* qq = q_ + (r * E + qi) * DP + h * DH;
          float s = 0.0f;
#pragma unroll
          for (int t = 0; t < DH; ++t) s = fmaf(qq[t], kv[t], s);
          const float ds = c[qi] * expf(s * scale - smax_(r)[h * E + qi]) * sinv_(r)[h * E + qi] * (tj - tbar_(r)[h * E + qi]) * scale;
#pragma unroll
          for (int t = 0; t < DH; ++t) dk[t] = fmaf(ds, qq[t], dk[t]);
        }
      }
#pragma unroll
      for (int t = 0; t < DH; ++t) dk_[(r * E + kj) * DP + h * DH + t] = dk[t];
    }
    __syncthreads();

    // ---- phase 9: gradients of q / k / v_linear (d v_e[d] = w[h(d)][e] d pooled[d])
    for (int i = tid; i < D * D; i += NT) {
      const int dd = i / D, c = i % D, h = dd / DH;
      float gq = 0.0f, gk = 0.0f, gv = 0.0f;
      for (int r = 0; r < nv; ++r) {
        const float dp = dpool_(r)[dd];
        for (int e = 0; e < E; ++e) {
          const int u = r * E + e;
          const float x = xn_[u * DP + c];
          gq = fmaf(dq_[u * DP + dd], x, gq);
          gk = fmaf(dk_[u * DP + dd], x, gk);
          gv = fmaf(wsum_(r)[h * E + e] * dp, x, gv);
        }
      }
      gadd(SRL_EATTN_Q_W, i, gq); gadd(SRL_EATTN_K_W, i, gk); gadd(SRL_EATTN_V_W, i, gv);
    }
    for (int dd = tid; dd < D; dd += NT) {
      const int h = dd / DH;
      float gq = 0.0f, gk = 0.0f, gv = 0.0f;
      for (int r = 0; r < nv; ++r) {
        const float dp = dpool_(r)[dd];
        for (int e = 0; e < E; ++e) {
          const int u = r * E + e;
          gq += dq_[u * DP + dd]; gk += dk_[u * DP + dd];
          gv = fmaf(wsum_(r)[h * E + e], dp, gv);
        }
      }
      gadd(SRL_EATTN_Q_B, dd, gq); gadd(SRL_EATTN_K_B, dd, gk); gadd(SRL_EATTN_V_B, dd, gv);
    }
    // ---- phase 10: d xn = Wq^T dq + Wk^T dk + Wv^T dv  -> the q buffer (q, k, v have had their last reader)
    __syncthreads();
    {
      const Mat Wq = matp(SRL_EATTN_Q_W), Wk = matp(SRL_EATTN_K_W), Wv = matp(SRL_EATTN_V_W);
      for (int i = tid; i < nv * E * D; i += NT) {
        const int c = i % D, u = i / D, r = u / E, e = u % E;
        float acc = 0.0f;
        for (int dd = 0; dd < D; ++dd) {
          acc = fmaf(Wq(dd, c), dq_[u * DP + dd], acc);
          acc = fmaf(Wk(dd, c), dk_[u * DP + dd], acc);
          acc = fmaf(Wv(dd, c), wsum_(r)[(dd / DH) * E + e] * dpool_(r)[dd], acc);
        }
        q_[u * DP + c] = acc;
      }
    }
    __syncthreads();

    // ---- phase 11: pre_norm backward: its affine gradients; d z = relu'(emb) * d emb -> the k buffer
    for (int c = tid; c < D; c += NT) {
      float gw = 0.0f, gb = 0.0f;
      for (int r = 0; r < nv; ++r)
        for (int e = 0; e < E; ++e) {
          const int u = r * E + e;
          const float g = q_[u * DP + c];
          gw = fmaf(g, (emb_[u * DP + c] - mean_(r)[e]) * rstd_(r)[e], gw);
          gb += g;
        }
      gadd(SRL_EATTN_PRE_W, c, gw); gadd(SRL_EATTN_PRE_B, c, gb);
    }
    for (int u = tid; u < nv * E; u += NT) {
      const int r = u / E, e = u % E;
      const float* w = vecp(SRL_EATTN_PRE_W);
      const float mu = mean_(r)[e], rs = rstd_(r)[e];
      float s1 = 0.0f, s2 = 0.0f;
      for (int c = 0; c < D; ++c) {
        const float g = q_[u * DP + c] * w[c];
        s1 += g;
        s2 = fmaf(g, (emb_[u * DP + c] - mu) * rs, s2);
      }
      s1 /= (float)D; s2 /= (float)D;
      for (int c = 0; c < D; ++c) {
        const float x = emb_[u * DP + c];
        const float g = q_[u * DP + c] * w[c];
        k_[u * DP + c] = x > 0.0f ? rs * (g - s1 - (x - mu) * rs * s2) : 0.0f;
      }
    }
    __syncthreads();

    // ---- phase 12: gradients of the embedding layers
    for (int i = tid; i < D * S; i += NT) {
      const int dd = i / S, j = i % S;
      float g = 0.0f;
      for (int r = 0; r < nv; ++r) g = fmaf(dzs_(r)[dd], a_[r * in_row + j], g);
      gadd(SRL_EATTN_SELF_W, i, g);
    }
    for (int dd = tid; dd < D; dd += NT) {
      float g = 0.0f;
      for (int r = 0; r < nv; ++r) g += dzs_(r)[dd];
      gadd(SRL_EATTN_SELF_B, dd, g);
    }
    for (int k = 0; k < d.nkeys; ++k) {
      const int f = d.f[k], in = S + f, cnt = d.cnt[k], e0 = pl.ent0[k], ko = pl.koff[k];
      for (int i = tid; i < D * in; i += NT) {
        const int dd = i / in, j = i % in;
        float g = 0.0f;
        for (int r = 0; r < nv; ++r) {
          const float* ar = a_ + r * in_row;
          for (int le = 0; le < cnt; ++le) {
            const float x = j < S ? ar[j] : ar[ko + le * f + (j - S)];
            g = fmaf(k_[(r * E + e0 + le) * DP + dd], x, g);
          }
        }
        gadd(SRL_EATTN_KEY_W + k, i, g);
      }
      for (int dd = tid; dd < D; dd += NT) {
        float g = 0.0f;
        for (int r = 0; r < nv; ++r)
          for (int le = 0; le < cnt; ++le) g += k_[(r * E + e0 + le) * DP + dd];
        gadd(SRL_EATTN_KEY_B + k, dd, g);
      }
    }
    __syncthreads();

    // ---- phase 13: gradients w.r.t. the LayerNorm'ed inputs, written over them
    for (int k = 0; k < d.nkeys; ++k) {
      const int f = d.f[k], cnt = d.cnt[k], e0 = pl.ent0[k], ko = pl.koff[k];
      const Mat W = matp(SRL_EATTN_KEY_W + k);
      for (int i = tid; i < nv * cnt * f; i += NT) {
        const int j = i % f, le = (i / f) % cnt, r = i / (f * cnt);
        const float* dz = k_ + (r * E + e0 + le) * DP;
        float acc = 0.0f;
        for (int dd = 0; dd < D; ++dd) acc = fmaf(W(dd, S + j), dz[dd], acc);
        a_[r * in_row + ko + le * f + j] = acc;
      }
    }
    for (int i = tid; i < nv * S; i += NT) {
      const int r = i / S, j = i % S;
      const Mat Ws = matp(SRL_EATTN_SELF_W);
      float acc = 0.0f;
      for (int dd = 0; dd < D; ++dd) acc = fmaf(Ws(dd, j), dzs_(r)[dd], acc);
      for (int k = 0; k < d.nkeys; ++k) {
        const Mat W = matp(SRL_EATTN_KEY_W + k);
        for (int le = 0; le < d.cnt[k]; ++le) {
          const float* dz = k_ + (r * E + pl.ent0[k] + le) * DP;
          for (int dd = 0; dd < D; ++dd) acc = fmaf(W(dd, j), dz[dd], acc);
        }
      }
      a_[r * in_row + j] = acc;
    }
    __syncthreads();

    // ---- phase 14: gradients of the input LayerNorms' affines
    for (int j = tid; j < S; j += NT) {
      float gw = 0.0f, gb = 0.0f;
      for (int r = 0; r < nv; ++r) {
        const float g = a_[r * in_row + j];
        gw = fmaf(g, xh_[r * in_row + j], gw);
        gb += g;
      }
      gadd(SRL_EATTN_LN_SELF_W, j, gw); gadd(SRL_EATTN_LN_SELF_B, j, gb);
    }
    for (int k = 0; k < d.nkeys; ++k) {
      const int f = d.f[k], cnt = d.cnt[k], ko = pl.koff[k];
      for (int j = tid; j < f; j += NT) {
        float gw = 0.0f, gb = 0.0f;
        for (int r = 0; r < nv; ++r)
          for (int le = 0; le < cnt; ++le) {
            const int o = r * in_row + ko + le * f + j;
            gw = fmaf(a_[o], xh_[o], gw);
            gb += a_[o];
          }
        gadd(SRL_EATTN_LN_KEY_W + k, j, gw); gadd(SRL_EATTN_LN_KEY_B + k, j, gb);
      }
    }
    __syncthreads();   // the next tile overwrites the row buffers
  }

  if (BWD && pl.stage_g) {   // the workgroup's sums, once
    for (int s = 0; s < NS; ++s) {
      const int n = pl.n[s];
      for (int i = tid; i < n; i += NT) {
        const float v = lds[pl.o_grad + pl.goff[s] + i];
        if (v != 0.0f) atomicAdd(d.g[s] + i, v);
      }
    }
  }
}

// The grid a plan runs `rows` rows on: what launch<> uses and what srl_entity_attn_plan reports.
struct EaGrid {
  size_t lds;       // dynamic LDS bytes of a workgroup
  int64_t ntiles;   // tiles of R rows
  unsigned groups;  // workgroups launched: min(ntiles, CUs x workgroups a CU holds)
};

EaGrid make_grid(const EaPlan& pl, int64_t rows) {
  EaGrid g;
  int cus = 256;
  int dev = 0;
  if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  g.lds = (size_t)pl.total * sizeof(float);
  g.ntiles = srl_ceil_div(rows, (int64_t)pl.R);
  int per_cu = (int)((size_t)(160 * 1024) / (g.lds ? g.lds : 1));
  per_cu = per_cu < 1 ? 1 : (per_cu > 2 ? 2 : per_cu);   // (a CU holds at most two workgroups of 1024 threads)
  const int64_t cap = (int64_t)cus * per_cu;
  g.groups = (unsigned)(g.ntiles < cap ? g.ntiles : cap);
  return g;
}

template <bool BWD>
int launch(void* stream, const srl_entity_attn* d, const EaPlan& pl, int64_t rows, float* out, int64_t ldo, const float* dout,
           int64_t lddo) {
  EaArgs a;
  memset(&a, 0, sizeof(a));
  a.d = *d;
  a.pl = pl;
  a.rows = rows; a.out = out; a.ldo = ldo; a.dout = dout; a.lddo = lddo;
  if (rows == 0) return 0;
  const EaGrid g = make_grid(a.pl, rows);
  const size_t lds = g.lds;
  void (*kern)(const EaArgs) = nullptr;
  switch (d->D / kHeads) {
    case 4: kern = entity_attn_kernel<4, BWD>; break;
    case 8: kern = entity_attn_kernel<8, BWD>; break;
    default: kern = entity_attn_kernel<16, BWD>; break;
  }
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kern, dim3(g.groups), dim3(kThreads), lds, (hipStream_t)stream, a);
  SRL_LAUNCH_CHECK();
  return 0;
}

// the shape part of check_desc (no pointer is looked at)
int check_shape(const srl_entity_attn* d, bool bwd, EaPlan* plan, const char** why) {
  if (!valid_shape(d)) { *why = "unsupported shape (srl_entity_attn_supported)"; return 0; }
  if (!make_plan(*d, bwd, plan)) { *why = "one row does not fit the LDS"; return 0; }
  return 1;
}

int check_desc(const srl_entity_attn* d, bool bwd, EaPlan* plan, const char** why) {
  if (!check_shape(d, bwd, plan, why)) return 0;
  const EaPlan& pl = *plan;
  for (int s = 0; s < NS; ++s) {
    if (pl.n[s] && (!d->p[s] || (bwd && !d->g[s]))) { *why = "null parameter / gradient"; return 0; }
  }
  if (!d->x_self || !d->mask || d->ld_self < d->S || d->ld_mask < d->E) { *why = "null leaf / short leaf rows"; return 0; }
  for (int k = 0; k < d->nkeys; ++k)
    if (!d->x_key[k] || d->ld_key[k] < (int64_t)d->cnt[k] * d->f[k]) { *why = "null leaf / short leaf rows"; return 0; }
  return 1;
}

}  // namespace

extern "C" int srl_entity_attn_supported(const srl_entity_attn* d) {
  if (!valid_shape(d)) return 0;
  EaPlan pl;
  return make_plan(*d, false, &pl) && make_plan(*d, true, &pl) ? 1 : 0;
}

extern "C" int srl_entity_attn_plan(const srl_entity_attn* d, int bwd, int64_t rows, int32_t* out) {
  const char* why = "";
  EaPlan pl;
  SRL_CHECK_ARG(check_shape(d, bwd != 0, &pl, &why), why);
  SRL_CHECK_ARG(out && rows >= 0, "null out / negative rows");
  const EaGrid g = make_grid(pl, rows);
  out[0] = pl.R; out[1] = pl.stage_p; out[2] = pl.stage_g; out[3] = (int32_t)g.lds;
  out[4] = (int32_t)g.groups; out[5] = (int32_t)g.ntiles;
  return 0;
}

extern "C" int srl_entity_attn_fwd(void* stream, const srl_entity_attn* d, int64_t rows, float* out, int64_t ldo) {
  const char* why = "";
  EaPlan pl;
  SRL_CHECK_ARG(check_desc(d, false, &pl, &why), why);
  SRL_CHECK_ARG(out && rows >= 0 && ldo >= 2 * d->D, "null out / short out rows");
  return launch<false>(stream, d, pl, rows, out, ldo, nullptr, 0);
}

extern "C" int srl_entity_attn_bwd(void* stream, const srl_entity_attn* d, int64_t rows, const float* d_out, int64_t lddo) {
  const char* why = "";
  EaPlan pl;
  SRL_CHECK_ARG(check_desc(d, true, &pl, &why), why);
  SRL_CHECK_ARG(d_out && rows >= 0 && lddo >= 2 * d->D, "null d_out / short d_out rows");
  return launch<true>(stream, d, pl, rows, nullptr, 0, d_out, lddo);
}
