// K8l: the heads that read more than one logit per example.
//
// er_softmax_ce   tf.losses.sparse_softmax_cross_entropy(labels, logits, weights), reduction SUM_BY_NONZERO_WEIGHTS
//                 (reference builders/loss_builder.py:40-46), with everything else a multi-class head needs from the same
//                 pass over the logits: softmax, argmax, the row maxima, d loss / d logits and the label's rank (accuracy
//                 and recall at k).  Up to 8 heads per launch (the towers of a multi-task model).
// er_jrc          reference loss/jrc_loss.py (arXiv 2208.06164) with same_label_loss and the fixed weight strategy:
//                 alpha * cross entropy + (1 - alpha) * the per-session generative loss, and its gradient.  The
//                 reference's [B, B] masks reduce to per-session sums (below); nothing of size B x B is stored.
//
// fp32, precise expf / logf, no MFMA, no atomics; every sum has one fixed order, so two runs and a graph replay give the
// same bits.  The logits are read where the layer left them (a row pitch).
//
// ---- er_softmax_ce geometry.  G lanes share a row: G = 1 for C <= 8 (the row lives in 8 registers), else the power of
// two >= ceil(C / 8), at most 64; lane l of the group owns the columns l, l + G, ...  A workgroup of 256 threads holds
// RW = 256 / G rows at a time; the head's `grid` = min(ceil(B / RW), 1024) workgroups walk the row blocks g, g + grid, ..
// A lane folds its columns in ascending order from the first; the G lanes meet in the xor butterfly 1, 2, .., G / 2
// (maxima with the smaller column winning a tie: tf.argmax's first index).  The loss: the row's leader lane adds w * ce
// to its own sum in the order it walks its rows, from 0.f; the 256 sums meet in block_sum_256's tree; workgroup g stores
// loss_scale * that / nz as partials[g].  nz: every workgroup counts the non-zero weights of all B rows itself (integer
// counts: no order to fix), so no workgroup waits for another.
//
// ---- er_jrc.  With S(i) = {k : key_k == key_i}, n = |S(i)|, P = sum_S y_k, W = sum_S w_k and lse_c the log-sum-exp of
// z[k, c] over S(i), the reference's masked [B, B] form evaluates to (a masked entry adds exp(-1e9) = 0)
//   ge = (1 / B) sum_i (w_i / n) * sum_{k in S(i)} t_k,   t_k = -(y_k (z[k, 1] - lse_1) + (1 - y_k) (z[k, 0] - lse_0))
//      = (1 / B) sum_k (W / n) t_k                        (each session's inner sum is shared by its n members)
//   d ge / d z[i, 1] = (1 / B) (W / n) (P softmax_S(z[:, 1])_i - y_i),  d ge / d z[i, 0] likewise with 1 - y and n - P.
// Thread i owns example i and walks k = 0, 1, .., B - 1 in ascending order, 256 examples at a time staged through LDS
// (every lane reads the same LDS word: a broadcast); the log-sum-exps are running (max, sum) pairs rescaled when the
// maximum moves, so they subtract the session's maximum.  ceil(B / 256) workgroups; partials as above.
#include <math.h>

#include "er_common.h"

namespace er {

constexpr int kSmcMaxC = 4096;
constexpr int kSmcSmallC = 8;
constexpr int kSmcMaxGrid = 1024;
constexpr int kSmcHeads = 8;
constexpr int kJrcMaxB = 8192;

__host__ __device__ inline int smc_group(int C) {
  if (C <= kSmcSmallC) return 1;
  const int need = (C + 7) / 8;
  int g = 2;
  while (g < need && g < kWave) g <<= 1;
  return g;
}

struct SmcHead {
  const float* z; const float* y; const float* w;
  float* probs; int64_t* ymax; float* logits_y; float* probs_y; float* dz; int32_t* rank; float* partials;
  int64_t B, ldz, ldp, lddz;
  int C, grid, first;  // this head's workgroups are [first, first + grid) of the launch
  float scale;
};
struct SmcArgs {
  SmcHead h[kSmcHeads];
  int n;
};

// the number of non-zero entries of w[0..B) (B without weights), at least 1, as a float; valid in every thread
__device__ __forceinline__ float block_nonzero(const float* __restrict__ w, int64_t B, int* s4) {
  if (w == nullptr) return static_cast<float>(B);
  int cnt = 0;
  for (int64_t i = threadIdx.x; i < B; i += kBlock) cnt += w[i] != 0.f ? 1 : 0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, kWave);
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = cnt;
  __syncthreads();
  const int tot = s4[0] + s4[1] + s4[2] + s4[3];
  __syncthreads();
  return tot > 0 ? static_cast<float>(tot) : 1.f;
}

// what a row's leader lane stores once the row is reduced; returns the row's w * ce
__device__ __forceinline__ float smc_finish_row(const SmcHead& h, int64_t r, float m, int am, float lse, float zl, int rank,
                                                bool ok, float wi) {
  if (h.ymax) h.ymax[r] = am;
  if (h.logits_y) h.logits_y[r] = m;
  if (h.probs_y) h.probs_y[r] = expf(m - lse);
  if (h.rank) h.rank[r] = ok ? rank : h.C;
  return ok ? wi * (lse - zl) : 0.f;
}

// C <= 8: one lane per row, the row in registers
__device__ __forceinline__ float smc_rows_small(const SmcHead& h, int bid, float nz) {
  float acc = 0.f;
  const int C = h.C;
  for (int64_t r = static_cast<int64_t>(bid) * kBlock + threadIdx.x; r < h.B; r += static_cast<int64_t>(h.grid) * kBlock) {
    const float* zr = h.z + r * h.ldz;
    float v[kSmcSmallC];
#pragma unroll
    for (int c = 0; c < kSmcSmallC; ++c) v[c] = c < C ? zr[c] : -INFINITY;
    float m = v[0];
    int am = 0;
#pragma unroll
    for (int c = 1; c < kSmcSmallC; ++c)
      if (v[c] > m) { m = v[c]; am = c; }
    const float yl = h.y ? h.y[r] : -1.f;  // (no labels: a forward-only launch)
    const bool ok = yl >= 0.f && yl < static_cast<float>(C);  // (false for a NaN label too)
    const int lab = ok ? static_cast<int>(yl) : 0;
    float zl = v[0];
#pragma unroll
    for (int c = 1; c < kSmcSmallC; ++c)
      if (c == lab) zl = v[c];
    float s = 0.f;
    int rank = 0;
#pragma unroll
    for (int c = 0; c < kSmcSmallC; ++c)
      if (c < C) {
        s = s + expf(v[c] - m);
        rank += (v[c] > zl || (c < lab && v[c] == zl)) ? 1 : 0;
      }
    const float lse = m + logf(s);
    const float wi = h.w ? h.w[r] : 1.f;
    const float coef = ok ? h.scale * wi / nz : 0.f;
#pragma unroll
    for (int c = 0; c < kSmcSmallC; ++c)
      if (c < C) {
        const float p = expf(v[c] - lse);
        if (h.probs) h.probs[r * h.ldp + c] = p;
        if (h.dz) h.dz[r * h.lddz + c] = coef * (p - (ok && c == lab ? 1.f : 0.f));
      }
    acc = acc + smc_finish_row(h, r, m, am, lse, zl, rank, ok, wi);
  }
  return acc;
}

// C > 8: G lanes per row; every lane of a wave runs the same number of row blocks (a lane past the last row works on
// row B - 1 and stores nothing), so the cross-lane exchanges always find their partners
__device__ __forceinline__ float smc_rows_wide(const SmcHead& h, int bid, float nz) {
  float acc = 0.f;
  const int C = h.C, G = smc_group(C), RW = kBlock / G;
  const int gl = static_cast<int>(threadIdx.x) % G, rl = static_cast<int>(threadIdx.x) / G;
  for (int64_t base = static_cast<int64_t>(bid) * RW; base < h.B; base += static_cast<int64_t>(h.grid) * RW) {
    const bool live = base + rl < h.B;
    const int64_t r = live ? base + rl : h.B - 1;
    const float* zr = h.z + r * h.ldz;
    float m = -INFINITY;
    int am = C;
    for (int c = gl; c < C; c += G) {
      const float v = zr[c];
      if (v > m || am == C) { m = v; am = c; }
    }
    for (int off = 1; off < G; off <<= 1) {
      const float om = __shfl_xor(m, off, kWave);
      const int oa = __shfl_xor(am, off, kWave);
      if (om > m || (om == m && oa < am)) { m = om; am = oa; }
    }
    const float yl = h.y ? h.y[r] : -1.f;  // (no labels: a forward-only launch)
    const bool ok = yl >= 0.f && yl < static_cast<float>(C);
    const int lab = ok ? static_cast<int>(yl) : 0;
    const float zl = zr[lab];
    float s = 0.f;
    int rank = 0;
    for (int c = gl; c < C; c += G) {
      const float v = zr[c];
      s = s + expf(v - m);
      rank += (v > zl || (c < lab && v == zl)) ? 1 : 0;
    }
    s = group_sum_rt(s, G);
    for (int off = 1; off < G; off <<= 1) rank += __shfl_xor(rank, off, kWave);
    const float lse = m + logf(s);
    const float wi = h.w ? h.w[r] : 1.f;
    const float coef = ok ? h.scale * wi / nz : 0.f;
    if (live && (h.probs || h.dz)) {
      for (int c = gl; c < C; c += G) {
        const float p = expf(zr[c] - lse);
        if (h.probs) h.probs[r * h.ldp + c] = p;
        if (h.dz) h.dz[r * h.lddz + c] = coef * (p - (ok && c == lab ? 1.f : 0.f));
      }
    }
    if (live && gl == 0) acc = acc + smc_finish_row(h, r, m, am, lse, zl, rank, ok, wi);
  }
  return acc;
}

__global__ __launch_bounds__(kBlock) void softmax_ce_kernel(SmcArgs a) {
  __shared__ float red[4];
  __shared__ int ired[4];
  int t = 0;
  while (t + 1 < a.n && static_cast<int>(blockIdx.x) >= a.h[t + 1].first) ++t;
  const SmcHead& h = a.h[t];
  const int bid = static_cast<int>(blockIdx.x) - h.first;
  const float nz = block_nonzero(h.w, h.B, ired);
  const float acc = h.C <= kSmcSmallC ? smc_rows_small(h, bid, nz) : smc_rows_wide(h, bid, nz);
  const float tot = block_sum_256(acc, red);
  if (threadIdx.x == 0 && h.partials) h.partials[bid] = h.scale * tot / nz;
}

// ------------------------------------------------------------------------------------------------------------ JRC
__device__ __forceinline__ void jrc_lse_step(float v, float* m, float* s) {
  if (v > *m) {
    *s = *s * expf(*m - v) + 1.f;  // (the first member: 0 * exp(-inf) + 1)
    *m = v;
  } else {
    *s = *s + expf(v - *m);
  }
}

__global__ __launch_bounds__(kBlock) void jrc_kernel(const float* __restrict__ z, int ldz, const float* __restrict__ y,
                                                    const int64_t* __restrict__ keys, const float* __restrict__ w, int B,
                                                    float alpha, float ce_scale, float scale, float* __restrict__ partials,
                                                    float* __restrict__ dz, int lddz, float* __restrict__ probs) {
  __shared__ int64_t s_key[kBlock];
  __shared__ float s_z0[kBlock], s_z1[kBlock], s_y[kBlock], s_w[kBlock];
  __shared__ float red[4];
  const int i = static_cast<int>(blockIdx.x) * kBlock + threadIdx.x;
  const bool live = i < B;
  const int ii = live ? i : B - 1;
  const int64_t key = keys[ii];
  float n = 0.f, P = 0.f, W = 0.f, m1 = -INFINITY, s1 = 0.f, m0 = -INFINITY, s0 = 0.f;
  int nzc = 0;
  for (int k0 = 0; k0 < B; k0 += kBlock) {
    const int k = k0 + threadIdx.x;
    if (k < B) {
      s_key[threadIdx.x] = keys[k];
      s_z0[threadIdx.x] = z[static_cast<int64_t>(k) * ldz];
      s_z1[threadIdx.x] = z[static_cast<int64_t>(k) * ldz + 1];
      s_y[threadIdx.x] = y[k] != 0.f ? 1.f : 0.f;
      s_w[threadIdx.x] = w ? w[k] : 1.f;
    }
    __syncthreads();
    const int cnt = min(kBlock, B - k0);
    for (int j = 0; j < cnt; ++j) {
      const float wk = s_w[j];
      nzc += wk != 0.f ? 1 : 0;
      if (s_key[j] == key) {
        n += 1.f;
        P += s_y[j];
        W = W + wk;
        jrc_lse_step(s_z1[j], &m1, &s1);
        jrc_lse_step(s_z0[j], &m0, &s0);
      }
    }
    __syncthreads();
  }
  const float nz = w ? (nzc > 0 ? static_cast<float>(nzc) : 1.f) : static_cast<float>(B);
  float term = 0.f;
  if (live) {
    const float z0 = z[static_cast<int64_t>(i) * ldz], z1 = z[static_cast<int64_t>(i) * ldz + 1];
    const float yi = y[i] != 0.f ? 1.f : 0.f, wi = w ? w[i] : 1.f;
    // the cross entropy at C = 2
    const float m = fmaxf(z0, z1);
    const float lse = m + logf(expf(z0 - m) + expf(z1 - m));
    const float p0 = expf(z0 - lse), p1 = expf(z1 - lse);
    const float ce = lse - (yi != 0.f ? z1 : z0);
    // the session's part
    const float lse1 = m1 + logf(s1), lse0 = m0 + logf(s0);
    const float f = (W / n) / static_cast<float>(B);
    const float ge = f * -(yi * (z1 - lse1) + (1.f - yi) * (z0 - lse0));
    const float cc = alpha * ce_scale * wi / nz, cg = (1.f - alpha) * f;
    term = alpha * ce_scale * (wi * ce) / nz + (1.f - alpha) * ge;
    if (dz) {
      dz[static_cast<int64_t>(i) * lddz] = scale * (cc * (p0 - (1.f - yi)) + cg * ((n - P) * expf(z0 - lse0) - (1.f - yi)));
      dz[static_cast<int64_t>(i) * lddz + 1] = scale * (cc * (p1 - yi) + cg * (P * expf(z1 - lse1) - yi));
    }
    if (probs) probs[i] = p1;
  }
  const float tot = block_sum_256(term, red);
  if (threadIdx.x == 0 && partials) partials[blockIdx.x] = scale * tot;
}

}  // namespace er

extern "C" {

int32_t er_softmax_ce_grid(int64_t B, int32_t C) {
  if (B < 1 || C < 2 || C > er::kSmcMaxC) return 0;
  const int64_t g = er::ceil_div(B, static_cast<int64_t>(er::kBlock / er::smc_group(C)));
  return static_cast<int32_t>(g < er::kSmcMaxGrid ? g : er::kSmcMaxGrid);
}

namespace er {
// head t of a launch, checked; `first`: the workgroups in front of it.  0, or ER_REQUIRE's error code
static int smc_set_head(SmcArgs* a, int t, int* first, const float* logits, int64_t ld_logits, const float* labels,
                        const float* weights, int64_t B, int32_t C, float loss_scale, float* probs, int64_t ld_probs,
                        int64_t* y, float* logits_y, float* probs_y, float* dlogits, int64_t ld_dlogits, int32_t* label_rank,
                        float* loss_partials) {
  const int grid = er_softmax_ce_grid(B, C);
  ER_REQUIRE(grid > 0, "er_softmax_ce: head %d: B = %lld, C = %d outside the envelope (B >= 1, 2 <= C <= %d)", t,
             static_cast<long long>(B), C, kSmcMaxC);
  ER_REQUIRE(logits, "er_softmax_ce: head %d: logits are required", t);
  ER_REQUIRE(labels || !(dlogits || label_rank || loss_partials),
             "er_softmax_ce: head %d: dlogits, label_rank and loss_partials need labels", t);
  ER_REQUIRE(ld_logits >= C && (probs == nullptr || ld_probs >= C) && (dlogits == nullptr || ld_dlogits >= C),
             "er_softmax_ce: head %d: a pitch below C = %d", t, C);
  SmcHead& h = a->h[t];
  h.z = logits; h.y = labels; h.w = weights;
  h.probs = probs; h.ymax = y; h.logits_y = logits_y; h.probs_y = probs_y; h.dz = dlogits;
  h.rank = label_rank; h.partials = loss_partials;
  h.B = B; h.ldz = ld_logits; h.ldp = ld_probs; h.lddz = ld_dlogits;
  h.C = C; h.grid = grid; h.first = *first; h.scale = loss_scale;
  *first += grid;
  return 0;
}
static int smc_launch(const SmcArgs& a, int total, er_stream_t stream) {
  hipLaunchKernelGGL(softmax_ce_kernel, dim3(static_cast<unsigned>(total)), dim3(kBlock), 0, as_stream(stream), a);
  ER_LAUNCH_CHECK();
  return 0;
}
}  // namespace er

int er_softmax_ce(const float* logits, int64_t ld_logits, const float* labels, const float* weights, int64_t B, int32_t C,
                  float loss_scale, float* probs, int64_t ld_probs, int64_t* y, float* logits_y, float* probs_y,
                  float* dlogits, int64_t ld_dlogits, int32_t* label_rank, float* loss_partials, er_stream_t stream) {
  er::SmcArgs a;
  memset(&a, 0, sizeof(a));
  a.n = 1;
  int total = 0;
  const int rc = er::smc_set_head(&a, 0, &total, logits, ld_logits, labels, weights, B, C, loss_scale, probs, ld_probs, y,
                                  logits_y, probs_y, dlogits, ld_dlogits, label_rank, loss_partials);
  return rc ? rc : er::smc_launch(a, total, stream);
}

int er_softmax_ce_multi(int32_t n, const float* const* logits_host, const int64_t* ld_logits_host,
                        const float* const* labels_host, const float* const* weights_host, const int64_t* B_host,
                        const int32_t* C_host, const float* loss_scale_host, float* const* probs_host,
                        float* const* dlogits_host, float* const* loss_partials_host, er_stream_t stream) {
  ER_REQUIRE(n >= 1 && n <= er::kSmcHeads, "er_softmax_ce_multi: 1 to %d heads per launch (n = %d)", er::kSmcHeads, n);
  ER_REQUIRE(logits_host && ld_logits_host && labels_host && weights_host && B_host && C_host && loss_scale_host &&
                 probs_host && dlogits_host && loss_partials_host, "er_softmax_ce_multi: every host array is required");
  er::SmcArgs a;
  memset(&a, 0, sizeof(a));
  a.n = n;
  int total = 0;
  for (int t = 0; t < n; ++t) {
    const int rc = er::smc_set_head(&a, t, &total, logits_host[t], ld_logits_host[t], labels_host[t], weights_host[t],
                                    B_host[t], C_host[t], loss_scale_host[t], probs_host[t], C_host[t], nullptr, nullptr,
                                    nullptr, dlogits_host[t], C_host[t], nullptr, loss_partials_host[t]);
    if (rc) return rc;
  }
  return er::smc_launch(a, total, stream);
}

int32_t er_jrc_grid(int64_t B) {
  if (B < 1 || B > er::kJrcMaxB) return 0;
  return static_cast<int32_t>(er::ceil_div(B, static_cast<int64_t>(er::kBlock)));
}

int er_jrc(const float* logits, int64_t ld_logits, const float* labels, const int64_t* session_keys, const float* weights,
           int64_t B, float alpha, float ce_scale, float loss_scale, float* loss_partials, float* dlogits,
           int64_t ld_dlogits, float* probs, er_stream_t stream) {
  const int grid = er_jrc_grid(B);
  ER_REQUIRE(grid > 0, "er_jrc: B = %lld outside the envelope (1 <= B <= %d)", static_cast<long long>(B), er::kJrcMaxB);
  ER_REQUIRE(logits && labels && session_keys, "er_jrc: logits, labels and session keys are required");
  ER_REQUIRE(ld_logits >= 2 && ld_logits <= (1 << 20) && (dlogits == nullptr || (ld_dlogits >= 2 && ld_dlogits <= (1 << 20))),
             "er_jrc: a pitch outside [2, 2^20]");
  hipLaunchKernelGGL(er::jrc_kernel, dim3(static_cast<unsigned>(grid)), dim3(er::kBlock), 0, er::as_stream(stream), logits,
                     static_cast<int>(ld_logits), labels, session_keys, weights, static_cast<int>(B), alpha, ce_scale,
                     loss_scale, loss_partials, dlogits, static_cast<int>(ld_dlogits), probs);
  ER_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
