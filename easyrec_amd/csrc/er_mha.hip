// K8f: the BERT-style encoder's two launches that are not contractions (reference
// layers/multihead_cross_attention.py): the masked multi-head attention core between the projections and the output
// dense (:179-243), and the residual add + LayerNorm that closes every sub-layer (:346, :365, :768;
// compat/layers.py layer_norm, epsilon 1e-12).
//
// Attention.  One workgroup (512 threads) owns whole (example, head) units and walks them grid-stride: it stages the
// unit's Q_h [F, ds], K_h and V_h [T, ds] (the backward also dctx_h [F, ds]) in LDS at the odd row pitch odd(ds), so
// that a walk over rows at one column is conflict-free for ds_read_b32; the global side of the staging is 16-byte loads
// wherever ds, the row pitch and the base address are multiples of 16 bytes.  Every product is the same scalar loop
// (mha_mm): a thread owns four rows x one column of the result, lanes run along the operand whose pitch is 1 or odd,
// the other operand is a broadcast, and the sum over k runs 0, 1, .. from 0.f.  Row softmax: one wave per row, lanes
// over the keys, the fixed butterfly of wave_max / wave_sum.  The backward recomputes P from Q and K (nothing but the
// inputs is kept; the [B, H, F, T] matrix never reaches HBM) and, owning the unit, writes every row of dQ_h, dK_h and
// dV_h itself: no atomics, every sum in a fixed order.
//
// The mask's adder (1 - mask[b, j]) * -10000 is applied RELATIVE to the example's largest adder: softmax is invariant
// under a shift of the whole row, and s - 10000 in fp32 would round s to multiples of 2^-10 when every key is masked.
// With an open key nothing changes (masked keys get exp(-10000 + ..) = 0 either way); with none the row is the softmax
// of the unmasked scores, the value the reference's formula has in exact arithmetic.
//
// Grouped units (mha_group_*): for short sequences the 512 threads are G = 8, 4 or 2 groups, each owning a unit in its own
// LDS region with its own thread index and count.  The forward of both forms is ONE body (mha_fwd_units, a template on
// the grouped flag); the backward kernels are the same statements written out twice (see there for why); the results
// are the one-unit kernels' bits.  Segment mean (segment_mean_*):
// CMBF's masked mean pooling over consecutive token segments (reference layers/cmbf.py:292-326, :364), lanes along the
// width, one division per element.
//
// Add & LayerNorm.  One wave per row.  W % 4 == 0, W <= 1024 and 16-byte aligned operands: the row x + res lives in
// registers (up to 4 float4 per lane) between the passes; otherwise the row is re-read (it sits in L1 / L2).  The mean
// is taken about the row's first element and the variance as the mean of squared differences from that mean: a
// constant row gives exactly mean = the constant, variance = 0, y = beta.  The backward re-reads x and res:
// 16 W + 8 bytes per row in (dy, x, res, gamma amortised; mean, rstd), 4 W out (dz), against 12 W + 8 for a kept x + res,
// which would cost the forward 4 W more.  It never divides by gamma.  dgamma | dbeta leave as per-workgroup partial sums
// [er_add_ln_grid, 2 W] over the workgroup's contiguous stretch of rows, for er_theta_grad_reduce.
#include <math.h>

#include <initializer_list>

#include "er_field_block.h"

namespace er {

constexpr int kMhaLdsBudget = 80 * 1024;  // bytes per workgroup: two workgroups per CU (160 KiB)
constexpr int kMhaMaxGrid = 1024;         // persistent workgroups
constexpr int kMhaMaxDs = 128;
constexpr int kMhaThreads = 512;  // 8 waves: with two workgroups per CU, 4 waves per SIMD hide the LDS latency of mha_mm

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

struct MhaGeom {
  int F, T, H, ds;
  int ld;   // LDS pitch of a Q / K / V / dctx row (odd)
  int ldp;  // LDS pitch of a score row (odd)
  float scale;  // 1 / sqrt(ds)
};

inline MhaGeom mha_geom(int F, int T, int H, int ds) {
  MhaGeom g;
  g.F = F;
  g.T = T;
  g.H = H;
  g.ds = ds;
  g.ld = odd(ds);
  g.ldp = odd(T);
  g.scale = static_cast<float>(1.0 / sqrt(static_cast<double>(ds)));
  return g;
}

// floats: Q, K, V rows, the scores, the keys' adders; the backward adds dctx rows and dS
inline int64_t mha_fwd_floats(int F, int T, int ds) {
  return static_cast<int64_t>(F + 2 * T) * odd(ds) + static_cast<int64_t>(F) * odd(T) + T;
}
inline int64_t mha_bwd_floats(int F, int T, int ds) {
  return static_cast<int64_t>(2 * F + 2 * T) * odd(ds) + 2 * static_cast<int64_t>(F) * odd(T) + T;
}

inline bool mha_shape_ok(int F, int T, int H, int ds) {
  if (F < 1 || T < 1 || H < 1 || ds < 1 || ds > kMhaMaxDs || F > 4096 || T > 4096) return false;
  return 4 * mha_bwd_floats(F, T, ds) <= kMhaLdsBudget;
}

struct MhaArgs {
  const float* q;
  const float* k;
  const float* v;
  const float* dctx;
  const int32_t* mask;
  float* ctx;
  float* dq;
  float* dk;
  float* dv;
  int64_t ldq, ldk, ldv, lddq, lddk, lddv;  // row pitches in floats
  int64_t units;                            // B * H
  int vec;                                  // bit 0 / 1 / 2 / 3: q / k / v / dctx take 16-byte loads
  MhaGeom g;
};

// rows x ds floats at `pitch` -> LDS rows at ld
__device__ inline void mha_stage(int tid, int nthr, const float* __restrict__ src, int64_t pitch, int rows, int ds,
                                 bool vec, int ld, float* dst) {
  if (vec) {
    const int q4 = ds >> 2, n = rows * q4;
    for (int t = tid; t < n; t += nthr) {
      const int r = t / q4, c = (t - r * q4) << 2;
      const float4 x = *reinterpret_cast<const float4*>(src + r * pitch + c);
      float* d = dst + r * ld + c;
      d[0] = x.x;
      d[1] = x.y;
      d[2] = x.z;
      d[3] = x.w;
    }
  } else {
    const int n = rows * ds;
    for (int t = tid; t < n; t += nthr) {
      const int r = t / ds, c = t - r * ds;
      dst[r * ld + c] = src[r * pitch + c];
    }
  }
}

// C[m, n] = sum_k A[m * sam + k * sak] * Bm[n * sbn + k * sbk] for m < M, n < N, from LDS: a thread owns rows
// m0 .. m0 + 3 of one column n; lanes run along n (sbn is 1 or odd: conflict-free), A is a broadcast.
template <class Out>
__device__ __forceinline__ void mha_mm(int tid, int nthr, int M, int N, int K, const float* A, int sam, int sak,
                                       const float* Bm, int sbn, int sbk, Out out) {
  const int items = ((M + 3) >> 2) * N;
  for (int t = tid; t < items; t += nthr) {
    const int mb = t / N, n = t - mb * N, m0 = mb << 2;
    const float* a0 = A + m0 * sam;
    const float* a1 = A + min(m0 + 1, M - 1) * sam;  // (rows past M repeat the last one and are not written)
    const float* a2 = A + min(m0 + 2, M - 1) * sam;
    const float* a3 = A + min(m0 + 3, M - 1) * sam;
    const float* b = Bm + n * sbn;
    float c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
      const float bv = b[k * sbk];
      const int ka = k * sak;
      c0 += a0[ka] * bv;
      c1 += a1[ka] * bv;
      c2 += a2[ka] * bv;
      c3 += a3[ka] * bv;
    }
    out(m0, n, c0);
    if (m0 + 1 < M) out(m0 + 1, n, c1);
    if (m0 + 2 < M) out(m0 + 2, n, c2);
    if (m0 + 3 < M) out(m0 + 3, n, c3);
  }
}

// the keys' adders of example b, relative to the largest: 0 for an open key (or every key when none is open)
__device__ inline void mha_stage_adder(int tid, const int32_t* mask, int64_t b, int T, float* madd) {
  if (tid < kWave) {  // one wave: T is small
    const int lane = tid;
    float top = -INFINITY;
    if (mask != nullptr)
      for (int j = lane; j < T; j += kWave) top = fmaxf(top, (1.0f - static_cast<float>(mask[b * T + j])) * -10000.0f);
    top = wave_max(top);
    for (int j = lane; j < T; j += kWave)
      madd[j] = mask != nullptr ? (1.0f - static_cast<float>(mask[b * T + j])) * -10000.0f - top : 0.f;
  }
}

// S = Q K^T * scale
__device__ inline void mha_scores(int tid, int nthr, const MhaGeom& g, const float* Qs, const float* Ks, float* S) {
  const float scale = g.scale;
  const int ldp = g.ldp;
  mha_mm(tid, nthr, g.F, g.T, g.ds, Qs, g.ld, 1, Ks, g.ld, 1, [=](int i, int j, float s) { S[i * ldp + j] = s * scale; });
}

// P = softmax over the keys of S + adder, in S's place: one wave per row
__device__ inline void mha_softmax(int tid, int nthr, const MhaGeom& g, const float* madd, float* S) {
  const int ldp = g.ldp;
  const int lane = tid & (kWave - 1), wave = tid / kWave, waves = nthr / kWave;
  for (int i = wave; i < g.F; i += waves) {
    float* p = S + i * ldp;
    float m = -INFINITY;
    for (int j = lane; j < g.T; j += kWave) {
      const float s = p[j] + madd[j];
      p[j] = s;
      m = fmaxf(m, s);
    }
    m = wave_max(m);
    float sum = 0.f;
    for (int j = lane; j < g.T; j += kWave) {
      const float e = expf(p[j] - m);
      p[j] = e;
      sum += e;
    }
    sum = wave_sum(sum);
    for (int j = lane; j < g.T; j += kWave) p[j] = p[j] / sum;
  }
}

// dS = P o (dP - rowsum(dP o P)), times scale (both dQ and dK carry it), in dP's place: one wave per row
__device__ inline void mha_ds(int tid, int nthr, const MhaGeom& g, const float* P, float* D) {
  const int ldp = g.ldp;
  const int lane = tid & (kWave - 1), wave = tid / kWave, waves = nthr / kWave;
  for (int i = wave; i < g.F; i += waves) {
    const float* p = P + i * ldp;
    float* d = D + i * ldp;
    float dot = 0.f;
    for (int j = lane; j < g.T; j += kWave) dot += d[j] * p[j];
    dot = wave_sum(dot);
    for (int j = lane; j < g.T; j += kWave) d[j] = p[j] * (d[j] - dot) * g.scale;
  }
}

// ------------------------------------------------------------------------------- the unit loops, one-unit and grouped
// Grouped: the 512 threads split into G groups of 512 / G (a group is whole waves); group `grp` owns the unit
// pass * G + grp in its own LDS region (unit_floats apart) and its loops stride by the group size.  Every barrier is the
// workgroup's: a group whose unit is past the end skips the work between them, never a barrier.  An output element is
// the same single-thread chain over k and a softmax row the same wave butterfly in either form, so the results are the
// same bits.
//
// The forward is ONE body for both forms: one-unit is the grouped loop with the compile-time constants nthr = 512,
// grp = 0, on = true.  (MhaArgs BY VALUE: through a reference the compiler copies the kernel argument and allocates
// the one-unit kernel's registers differently - 1 % slower at CMBF's shapes; by value the ISA is the hand-written
// kernels' but for a handful of scalar instructions.)
template <bool kGroup>
__device__ __forceinline__ void mha_fwd_units(const MhaArgs a, int G, int unit_floats) {
  extern __shared__ float lds[];
  const MhaGeom g = a.g;
  const int F = g.F, T = g.T, ds = g.ds, ld = g.ld;
  const int nthr = kGroup ? kMhaThreads / G : kMhaThreads, grp = kGroup ? threadIdx.x / nthr : 0;
  const int tid = threadIdx.x - grp * nthr;
  float* Qs = lds + grp * unit_floats;
  float* Ks = Qs + F * ld;
  float* Vs = Ks + T * ld;
  float* S = Vs + T * ld;
  float* madd = S + F * g.ldp;
  const int64_t dctx = static_cast<int64_t>(g.H) * ds;
  const int64_t per = kGroup ? G : 1;  // units a workgroup takes per pass
  for (int64_t u0 = blockIdx.x * per; u0 < a.units; u0 += gridDim.x * per) {
    const int64_t u = u0 + grp;
    const bool on = !kGroup || u < a.units;
    const int64_t b = on ? u / g.H : 0;
    const int h = on ? static_cast<int>(u - b * g.H) : 0;
    if (on) {
      mha_stage(tid, nthr, a.q + b * F * a.ldq + h * ds, a.ldq, F, ds, a.vec & 1, ld, Qs);
      mha_stage(tid, nthr, a.k + b * T * a.ldk + h * ds, a.ldk, T, ds, a.vec & 2, ld, Ks);
      mha_stage(tid, nthr, a.v + b * T * a.ldv + h * ds, a.ldv, T, ds, a.vec & 4, ld, Vs);
      mha_stage_adder(tid, a.mask, b, T, madd);
    }
    __syncthreads();
    if (on) mha_scores(tid, nthr, g, Qs, Ks, S);
    __syncthreads();
    if (on) mha_softmax(tid, nthr, g, madd, S);
    __syncthreads();
    if (on) {
      // ctx_h = P V_h
      float* out = a.ctx + b * F * dctx + h * ds;
      mha_mm(tid, nthr, F, ds, T, S, g.ldp, 1, Vs, 1, ld, [=](int i, int c, float s) { out[i * dctx + c] = s; });
    }
    __syncthreads();  // (the next pass restages)
  }
}

__global__ __launch_bounds__(kMhaThreads) void mha_fwd_kernel(MhaArgs a) { mha_fwd_units<false>(a, 1, 0); }
__global__ __launch_bounds__(kMhaThreads) void mha_group_fwd_kernel(MhaArgs a, int G, int unit_floats) {
  mha_fwd_units<true>(a, G, unit_floats);
}

// The backward is written out per form.  Through a shared body as above the one-unit kernel keeps its register and
// instruction counts, but the compiler allocates its registers otherwise and it runs 0.2 - 0.9 % slower at every shape
// (CMBF's and Uniter's, alternating windows in one process); by reference, by value and with the loop restated it stays
// so.  A change to the order of calls and barriers is made in BOTH kernels below.
__global__ __launch_bounds__(kMhaThreads) void mha_bwd_kernel(MhaArgs a) {
  extern __shared__ float lds[];
  const MhaGeom g = a.g;
  const int F = g.F, T = g.T, ds = g.ds, ld = g.ld, ldp = g.ldp;
  float* Qs = lds;
  float* Ks = Qs + F * ld;
  float* Vs = Ks + T * ld;
  float* Cs = Vs + T * ld;   // dctx_h [F, ld]
  float* P = Cs + F * ld;    // [F, ldp]
  float* D = P + F * ldp;    // dP, then dS * scale [F, ldp]
  float* madd = D + F * ldp;
  const int64_t dctx = static_cast<int64_t>(g.H) * ds;
  for (int64_t u = blockIdx.x; u < a.units; u += gridDim.x) {
    const int64_t b = u / g.H;
    const int h = static_cast<int>(u - b * g.H);
    mha_stage(threadIdx.x, kMhaThreads, a.q + b * F * a.ldq + h * ds, a.ldq, F, ds, a.vec & 1, ld, Qs);
    mha_stage(threadIdx.x, kMhaThreads, a.k + b * T * a.ldk + h * ds, a.ldk, T, ds, a.vec & 2, ld, Ks);
    mha_stage(threadIdx.x, kMhaThreads, a.v + b * T * a.ldv + h * ds, a.ldv, T, ds, a.vec & 4, ld, Vs);
    mha_stage(threadIdx.x, kMhaThreads, a.dctx + b * F * dctx + h * ds, dctx, F, ds, a.vec & 8, ld, Cs);
    mha_stage_adder(threadIdx.x, a.mask, b, T, madd);
    __syncthreads();
    mha_scores(threadIdx.x, kMhaThreads, g, Qs, Ks, P);
    __syncthreads();
    mha_softmax(threadIdx.x, kMhaThreads, g, madd, P);
    __syncthreads();
    // dP[i, j] = dctx_h[i] . V_h[j];  dV_h[j] = sum_i P[i, j] dctx_h[i]
    mha_mm(threadIdx.x, kMhaThreads, F, T, ds, Cs, ld, 1, Vs, ld, 1, [=](int i, int j, float s) { D[i * ldp + j] = s; });
    float* dv = a.dv + b * T * a.lddv + h * ds;
    const int64_t lddv = a.lddv;
    mha_mm(threadIdx.x, kMhaThreads, T, ds, F, P, 1, ldp, Cs, 1, ld, [=](int j, int c, float s) { dv[j * lddv + c] = s; });
    __syncthreads();
    mha_ds(threadIdx.x, kMhaThreads, g, P, D);
    __syncthreads();
    // dQ_h[i] = sum_j dS[i, j] K_h[j];  dK_h[j] = sum_i dS[i, j] Q_h[i]
    float* dq = a.dq + b * F * a.lddq + h * ds;
    float* dk = a.dk + b * T * a.lddk + h * ds;
    const int64_t lddq = a.lddq, lddk = a.lddk;
    mha_mm(threadIdx.x, kMhaThreads, F, ds, T, D, ldp, 1, Ks, 1, ld, [=](int i, int c, float s) { dq[i * lddq + c] = s; });
    mha_mm(threadIdx.x, kMhaThreads, T, ds, F, D, 1, ldp, Qs, 1, ld, [=](int j, int c, float s) { dk[j * lddk + c] = s; });
    __syncthreads();  // (the next unit restages)
  }
}

__global__ __launch_bounds__(kMhaThreads, 4) void mha_group_bwd_kernel(MhaArgs a, int G, int unit_floats) {
  extern __shared__ float lds[];
  const MhaGeom g = a.g;
  const int F = g.F, T = g.T, ds = g.ds, ld = g.ld, ldp = g.ldp;
  const int nthr = kMhaThreads / G, grp = threadIdx.x / nthr, tid = threadIdx.x - grp * nthr;
  float* Qs = lds + grp * unit_floats;
  float* Ks = Qs + F * ld;
  float* Vs = Ks + T * ld;
  float* Cs = Vs + T * ld;
  float* P = Cs + F * ld;
  float* D = P + F * ldp;
  float* madd = D + F * ldp;
  const int64_t dctx = static_cast<int64_t>(g.H) * ds;
  for (int64_t u0 = static_cast<int64_t>(blockIdx.x) * G; u0 < a.units; u0 += static_cast<int64_t>(gridDim.x) * G) {
    const int64_t u = u0 + grp;
    const bool on = u < a.units;
    const int64_t b = on ? u / g.H : 0;
    const int h = on ? static_cast<int>(u - b * g.H) : 0;
    if (on) {
      mha_stage(tid, nthr, a.q + b * F * a.ldq + h * ds, a.ldq, F, ds, a.vec & 1, ld, Qs);
      mha_stage(tid, nthr, a.k + b * T * a.ldk + h * ds, a.ldk, T, ds, a.vec & 2, ld, Ks);
      mha_stage(tid, nthr, a.v + b * T * a.ldv + h * ds, a.ldv, T, ds, a.vec & 4, ld, Vs);
      mha_stage(tid, nthr, a.dctx + b * F * dctx + h * ds, dctx, F, ds, a.vec & 8, ld, Cs);
      mha_stage_adder(tid, a.mask, b, T, madd);
    }
    __syncthreads();
    if (on) mha_scores(tid, nthr, g, Qs, Ks, P);
    __syncthreads();
    if (on) mha_softmax(tid, nthr, g, madd, P);
    __syncthreads();
    if (on) {
      mha_mm(tid, nthr, F, T, ds, Cs, ld, 1, Vs, ld, 1, [=](int i, int j, float s) { D[i * ldp + j] = s; });
      float* dv = a.dv + b * T * a.lddv + h * ds;
      const int64_t lddv = a.lddv;
      mha_mm(tid, nthr, T, ds, F, P, 1, ldp, Cs, 1, ld, [=](int j, int c, float s) { dv[j * lddv + c] = s; });
    }
    __syncthreads();
    if (on) mha_ds(tid, nthr, g, P, D);
    __syncthreads();
    if (on) {
      float* dq = a.dq + b * F * a.lddq + h * ds;
      float* dk = a.dk + b * T * a.lddk + h * ds;
      const int64_t lddq = a.lddq, lddk = a.lddk;
      mha_mm(tid, nthr, F, ds, T, D, ldp, 1, Ks, 1, ld, [=](int i, int c, float s) { dq[i * lddq + c] = s; });
      mha_mm(tid, nthr, T, ds, F, D, 1, ldp, Qs, 1, ld, [=](int j, int c, float s) { dk[j * lddk + c] = s; });
    }
    __syncthreads();  // (the next pass restages)
  }
}

// units per workgroup: the largest of 8, 4, 2 whose backward regions fit the budget; 1: only one; 0: outside
inline int mha_group_units(int F, int T, int ds) {
  if (!mha_shape_ok(F, T, 1, ds)) return 0;
  const int64_t unit = 4 * mha_bwd_floats(F, T, ds);
  for (int G : {8, 4, 2})
    if (G * unit <= kMhaLdsBudget) return G;
  return 1;
}

// ---------------------------------------------------------------------------------------- segment mean
constexpr int kSegMaxSeg = 64;
constexpr int kSegMaxW = 4096;
constexpr int kSegMaxS = 4096;

// rows [t0, t0 + len) of segment s of example b: the begins clamped into [0, S] and ascending, len into the width
__device__ __forceinline__ void seg_range(const int32_t* __restrict__ seg_begin, const int32_t* __restrict__ lens,
                                          int64_t b, int s, int n_seg, int S, int* t0, int* width, int* len) {
  const int b0 = min(max(seg_begin[s], 0), S);
  const int b1 = min(max(seg_begin[s + 1], b0), S);
  *t0 = b0;
  *width = b1 - b0;
  *len = lens != nullptr ? min(max(lens[b * n_seg + s], 0), b1 - b0) : b1 - b0;
}

// a thread owns VEC columns of one (example, segment): the sum over t ascending, then one division
template <int VEC>
__global__ __launch_bounds__(kBlock) void segment_mean_fwd_kernel(const float* __restrict__ x,
                                                                 const int32_t* __restrict__ seg_begin,
                                                                 const int32_t* __restrict__ lens, int64_t B, int S, int W,
                                                                 int n_seg, float* __restrict__ out) {
  const int wv = W / VEC;
  const int64_t total = B * n_seg * wv;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; t < total;
       t += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int c = static_cast<int>(t % wv) * VEC;
    const int64_t bs = t / wv;
    const int s = static_cast<int>(bs % n_seg);
    const int64_t b = bs / n_seg;
    int t0, width, len;
    seg_range(seg_begin, lens, b, s, n_seg, S, &t0, &width, &len);
    const float* src = x + (b * S + t0) * W + c;
    const float n = static_cast<float>(len);
    if (VEC == 4) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int r = 0; r < len; ++r) {
        const float4 v = ld4(src + static_cast<int64_t>(r) * W);
        acc.x += v.x;
        acc.y += v.y;
        acc.z += v.z;
        acc.w += v.w;
      }
      *reinterpret_cast<float4*>(out + bs * W + c) = make_float4(acc.x / n, acc.y / n, acc.z / n, acc.w / n);
    } else {
      float acc = 0.f;
      for (int r = 0; r < len; ++r) acc += src[static_cast<int64_t>(r) * W];
      out[bs * W + c] = acc / n;
    }
  }
}

// the same ownership: dout / len to the segment's first len rows, 0 to the rest: every element of dx is written
template <int VEC>
__global__ __launch_bounds__(kBlock) void segment_mean_bwd_kernel(const float* __restrict__ dout,
                                                                 const int32_t* __restrict__ seg_begin,
                                                                 const int32_t* __restrict__ lens, int64_t B, int S, int W,
                                                                 int n_seg, float* __restrict__ dx) {
  const int wv = W / VEC;
  const int64_t total = B * n_seg * wv;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; t < total;
       t += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int c = static_cast<int>(t % wv) * VEC;
    const int64_t bs = t / wv;
    const int s = static_cast<int>(bs % n_seg);
    const int64_t b = bs / n_seg;
    int t0, width, len;
    seg_range(seg_begin, lens, b, s, n_seg, S, &t0, &width, &len);
    float* dst = dx + (b * S + t0) * W + c;
    const float n = static_cast<float>(len);
    if (VEC == 4) {
      const float4 d = ld4(dout + bs * W + c);
      const float4 gq = len > 0 ? make_float4(d.x / n, d.y / n, d.z / n, d.w / n) : make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int r = 0; r < len; ++r) *reinterpret_cast<float4*>(dst + static_cast<int64_t>(r) * W) = gq;
      for (int r = len; r < width; ++r) *reinterpret_cast<float4*>(dst + static_cast<int64_t>(r) * W) = zero;
    } else {
      const float gq = len > 0 ? dout[bs * W + c] / n : 0.f;
      for (int r = 0; r < len; ++r) dst[static_cast<int64_t>(r) * W] = gq;
      for (int r = len; r < width; ++r) dst[static_cast<int64_t>(r) * W] = 0.f;
    }
  }
}

struct MhaPackSrc {
  const float* w[3];
  const float* b[3];
};

// [W_0 | .. | W_{n-1}] ([din, d] each, row-major) -> w [din, n d];  [b_0 | ..] -> bias [n d]
__global__ __launch_bounds__(kBlock) void mha_pack_kernel(MhaPackSrc src, int n, int din, int d, float* __restrict__ w,
                                                         float* __restrict__ bias) {
  const int nd = n * d;
  const int64_t total = static_cast<int64_t>(din + 1) * nd;  // (the last row: the biases)
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; t < total;
       t += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int c = static_cast<int>(t % nd);
    const int64_t r = t / nd;
    const int k = c / d;
    if (r < din)
      w[t] = src.w[k][r * d + (c - k * d)];
    else
      bias[c] = src.b[k][c - k * d];
  }
}

// opt in to more than 64 KB of dynamic LDS: the attribute belongs to the current device's copy of the kernel, so it is
// set (to the whole envelope) at every launch that needs it, with no cache that a second device or a second launching
// thread could find stale (a host call with no stream work: safe inside a capture)
static int mha_set_lds(const void* fn, int bytes) {
  if (bytes > kFieldLdsBudget)
    ER_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kMhaLdsBudget));
  return 0;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ------------------------------------------------------------------------------------------------ add & LayerNorm
constexpr int kLnMaxW = 4096;
constexpr int kLnMaxGrid = 1024;  // rows of `partials`
constexpr int kLnRegW = 1024;     // widest row the register form keeps (4 float4 per lane)

template <int NV>
__global__ __launch_bounds__(kBlock) void add_ln_fwd_vec_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                               int64_t rows, int64_t res_rows, int W,
                                                               const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float eps,
                                                               float* __restrict__ y, float* __restrict__ mean,
                                                               float* __restrict__ rstd) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t step = static_cast<int64_t>(gridDim.x) * (kBlock / kWave);
  const float inv_w = 1.0f / static_cast<float>(W);
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * (kBlock / kWave) + wave; r < rows; r += step) {
    const float* xr = x + r * W;
    const float* rr = res != nullptr ? res + (r % res_rows) * W : nullptr;
    float4 z[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int c = (k * kWave + lane) << 2;
      z[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < W) {
        z[k] = ld4(xr + c);
        if (rr != nullptr) {
          const float4 q = ld4(rr + c);
          z[k].x += q.x;
          z[k].y += q.y;
          z[k].z += q.z;
          z[k].w += q.w;
        }
      }
    }
    const float shift = __shfl(z[0].x, 0, kWave);  // the row's first element
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k)
      if (((k * kWave + lane) << 2) < W) {
        s += z[k].x - shift;
        s += z[k].y - shift;
        s += z[k].z - shift;
        s += z[k].w - shift;
      }
    const float mu = shift + wave_sum(s) * inv_w;
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k)
      if (((k * kWave + lane) << 2) < W) {
        z[k].x -= mu;
        z[k].y -= mu;
        z[k].z -= mu;
        z[k].w -= mu;
        v += z[k].x * z[k].x;
        v += z[k].y * z[k].y;
        v += z[k].z * z[k].z;
        v += z[k].w * z[k].w;
      }
    const float rs = 1.0f / sqrtf(wave_sum(v) * inv_w + eps);
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int c = (k * kWave + lane) << 2;
      if (c < W) {
        const float4 ga = ld4(gamma + c), be = ld4(beta + c);
        float4 o;
        o.x = z[k].x * rs * ga.x + be.x;
        o.y = z[k].y * rs * ga.y + be.y;
        o.z = z[k].z * rs * ga.z + be.z;
        o.w = z[k].w * rs * ga.w + be.w;
        *reinterpret_cast<float4*>(y + r * W + c) = o;
      }
    }
    if (lane == 0) {
      mean[r] = mu;
      rstd[r] = rs;
    }
  }
}

// any width and alignment: the row is read three times
__global__ __launch_bounds__(kBlock) void add_ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                           int64_t rows, int64_t res_rows, int W,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float eps, float* __restrict__ y, float* __restrict__ mean,
                                                           float* __restrict__ rstd) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t step = static_cast<int64_t>(gridDim.x) * (kBlock / kWave);
  const float inv_w = 1.0f / static_cast<float>(W);
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * (kBlock / kWave) + wave; r < rows; r += step) {
    const float* xr = x + r * W;
    const float* rr = res != nullptr ? res + (r % res_rows) * W : nullptr;
    const float shift = xr[0] + (rr != nullptr ? rr[0] : 0.f);
    float s = 0.f;
    for (int c = lane; c < W; c += kWave) s += (xr[c] + (rr != nullptr ? rr[c] : 0.f)) - shift;
    const float mu = shift + wave_sum(s) * inv_w;
    float v = 0.f;
    for (int c = lane; c < W; c += kWave) {
      const float d = (xr[c] + (rr != nullptr ? rr[c] : 0.f)) - mu;
      v += d * d;
    }
    const float rs = 1.0f / sqrtf(wave_sum(v) * inv_w + eps);
    for (int c = lane; c < W; c += kWave) {
      const float d = (xr[c] + (rr != nullptr ? rr[c] : 0.f)) - mu;
      y[r * W + c] = d * rs * gamma[c] + beta[c];
    }
    if (lane == 0) {
      mean[r] = mu;
      rstd[r] = rs;
    }
  }
}

// rows [r0, r1) of workgroup blockIdx.x: a contiguous stretch of ceil(rows / grid)
__device__ __forceinline__ void ln_row_range(int64_t rows, int64_t* r0, int64_t* r1) {
  const int64_t per = (rows + gridDim.x - 1) / gridDim.x;
  *r0 = min(rows, static_cast<int64_t>(blockIdx.x) * per);
  *r1 = min(rows, *r0 + per);
}

template <int NV>
__global__ __launch_bounds__(kBlock) void add_ln_bwd_vec_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                               const float* __restrict__ res, int64_t rows,
                                                               int64_t res_rows, int W, const float* __restrict__ gamma,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, float* __restrict__ dz,
                                                               float* __restrict__ partials) {
  __shared__ float acc[kBlock / kWave][2 * kLnRegW];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const float inv_w = 1.0f / static_cast<float>(W);
  int64_t r0, r1;
  ln_row_range(rows, &r0, &r1);
  float4 ga[NV], dg[NV], db[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c = (k * kWave + lane) << 2;
    ga[k] = c < W ? ld4(gamma + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    dg[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    db[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  for (int64_t r = r0 + wave; r < r1; r += kBlock / kWave) {
    const float* rr = res != nullptr ? res + (r % res_rows) * W : nullptr;
    const float mu = mean[r], rs = rstd[r];
    float4 xh[NV], g[NV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int c = (k * kWave + lane) << 2;
      xh[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      g[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < W) {
        float4 z = ld4(x + r * W + c);
        if (rr != nullptr) {
          const float4 q = ld4(rr + c);
          z.x += q.x;
          z.y += q.y;
          z.z += q.z;
          z.w += q.w;
        }
        const float4 d = ld4(dy + r * W + c);
        xh[k].x = (z.x - mu) * rs;
        xh[k].y = (z.y - mu) * rs;
        xh[k].z = (z.z - mu) * rs;
        xh[k].w = (z.w - mu) * rs;
        g[k].x = d.x * ga[k].x;
        g[k].y = d.y * ga[k].y;
        g[k].z = d.z * ga[k].z;
        g[k].w = d.w * ga[k].w;
        s1 += g[k].x;
        s1 += g[k].y;
        s1 += g[k].z;
        s1 += g[k].w;
        s2 += g[k].x * xh[k].x;
        s2 += g[k].y * xh[k].y;
        s2 += g[k].z * xh[k].z;
        s2 += g[k].w * xh[k].w;
        dg[k].x += d.x * xh[k].x;
        dg[k].y += d.y * xh[k].y;
        dg[k].z += d.z * xh[k].z;
        dg[k].w += d.w * xh[k].w;
        db[k].x += d.x;
        db[k].y += d.y;
        db[k].z += d.z;
        db[k].w += d.w;
      }
    }
    const float m1 = wave_sum(s1) * inv_w, m2 = wave_sum(s2) * inv_w;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int c = (k * kWave + lane) << 2;
      if (c < W) {
        float4 o;
        o.x = rs * (g[k].x - m1 - xh[k].x * m2);
        o.y = rs * (g[k].y - m1 - xh[k].y * m2);
        o.z = rs * (g[k].z - m1 - xh[k].z * m2);
        o.w = rs * (g[k].w - m1 - xh[k].w * m2);
        *reinterpret_cast<float4*>(dz + r * W + c) = o;
      }
    }
  }
  // the four waves' column sums, combined in the order 0, 1, 2, 3
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c = (k * kWave + lane) << 2;
    if (c < W) {
      float* pg = &acc[wave][c];
      float* pb = &acc[wave][W + c];
      pg[0] = dg[k].x;
      pg[1] = dg[k].y;
      pg[2] = dg[k].z;
      pg[3] = dg[k].w;
      pb[0] = db[k].x;
      pb[1] = db[k].y;
      pb[2] = db[k].z;
      pb[3] = db[k].w;
    }
  }
  __syncthreads();
  float* out = partials + static_cast<int64_t>(blockIdx.x) * 2 * W;
  for (int c = threadIdx.x; c < 2 * W; c += kBlock) out[c] = ((acc[0][c] + acc[1][c]) + acc[2][c]) + acc[3][c];
}

__global__ __launch_bounds__(kBlock) void add_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                           const float* __restrict__ res, int64_t rows, int64_t res_rows,
                                                           int W, const float* __restrict__ gamma,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           float* __restrict__ dz, float* __restrict__ partials) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const float inv_w = 1.0f / static_cast<float>(W);
  int64_t r0, r1;
  ln_row_range(rows, &r0, &r1);
  for (int64_t r = r0 + wave; r < r1; r += kBlock / kWave) {
    const float* xr = x + r * W;
    const float* rr = res != nullptr ? res + (r % res_rows) * W : nullptr;
    const float* dr = dy + r * W;
    const float mu = mean[r], rs = rstd[r];
    float s1 = 0.f, s2 = 0.f;
    for (int c = lane; c < W; c += kWave) {
      const float xh = ((xr[c] + (rr != nullptr ? rr[c] : 0.f)) - mu) * rs;
      const float g = dr[c] * gamma[c];
      s1 += g;
      s2 += g * xh;
    }
    const float m1 = wave_sum(s1) * inv_w, m2 = wave_sum(s2) * inv_w;
    for (int c = lane; c < W; c += kWave) {
      const float xh = ((xr[c] + (rr != nullptr ? rr[c] : 0.f)) - mu) * rs;
      const float g = dr[c] * gamma[c];
      dz[r * W + c] = rs * (g - m1 - xh * m2);
    }
  }
  // a thread per column over the workgroup's rows, in order
  float* out = partials + static_cast<int64_t>(blockIdx.x) * 2 * W;
  for (int c = threadIdx.x; c < W; c += kBlock) {
    float dg = 0.f, db = 0.f;
    for (int64_t r = r0; r < r1; ++r) {
      const float z = x[r * W + c] + (res != nullptr ? res[(r % res_rows) * W + c] : 0.f);
      const float d = dy[r * W + c];
      dg += d * ((z - mean[r]) * rstd[r]);
      db += d;
    }
    out[c] = dg;
    out[W + c] = db;
  }
}

inline bool ln_vec_ok(int W, std::initializer_list<const void*> ptrs) {
  if (W % 4 != 0 || W > kLnRegW) return false;
  for (const void* p : ptrs)
    if (p != nullptr && !aligned16(p)) return false;
  return true;
}

}  // namespace er

extern "C" {

int64_t er_mha_lds_bytes(int32_t F, int32_t T, int32_t ds, int bwd) {
  if (F < 1 || T < 1 || ds < 1) return 0;
  return 4 * (bwd ? er::mha_bwd_floats(F, T, ds) : er::mha_fwd_floats(F, T, ds));
}

// the four attention entries: `what` names the caller in the error texts; the forward passes ctx and no dctx / dq / dk /
// dv, the backward the reverse; group: G = mha_group_units(F, T, ds) units per workgroup, refused below 2
static int mha_launch(const char* what, bool bwd, bool group, const float* q, int64_t ldq, const float* k, int64_t ldk,
                      const float* v, int64_t ldv, const int32_t* to_mask, const float* dctx, int64_t B, int32_t F,
                      int32_t T, int32_t H, int32_t ds, float* ctx, float* dq, int64_t lddq, float* dk, int64_t lddk,
                      float* dv, int64_t lddv, er_stream_t stream) {
  ER_REQUIRE(q && k && v && (bwd ? dctx && dq && dk && dv : ctx != nullptr) && B > 0, "%s: bad arguments", what);
  ER_REQUIRE(er::mha_shape_ok(F, T, H, ds), "%s: F = %d, T = %d, H = %d, ds = %d outside the envelope", what, F, T, H, ds);
  const int G = group ? er::mha_group_units(F, T, ds) : 1;
  ER_REQUIRE(!group || G >= 2, "%s: F = %d, T = %d, ds = %d leaves room for one unit per workgroup", what, F, T, ds);
  const int64_t d = static_cast<int64_t>(H) * ds;
  ER_REQUIRE(ldq >= d && ldk >= d && ldv >= d && (!bwd || (lddq >= d && lddk >= d && lddv >= d)),
             "%s: a row pitch is below H * ds = %lld", what, static_cast<long long>(d));
  er::MhaArgs a = {};
  a.q = q;
  a.k = k;
  a.v = v;
  a.dctx = dctx;
  a.mask = to_mask;
  a.ctx = ctx;
  a.dq = dq;
  a.dk = dk;
  a.dv = dv;
  a.ldq = ldq;
  a.ldk = ldk;
  a.ldv = ldv;
  a.lddq = lddq;
  a.lddk = lddk;
  a.lddv = lddv;
  a.units = B * H;
  a.g = er::mha_geom(F, T, H, ds);
  if (ds % 4 == 0) {
    if (ldq % 4 == 0 && er::aligned16(q)) a.vec |= 1;
    if (ldk % 4 == 0 && er::aligned16(k)) a.vec |= 2;
    if (ldv % 4 == 0 && er::aligned16(v)) a.vec |= 4;
    if (bwd && er::aligned16(dctx)) a.vec |= 8;  // (its pitch H * ds is a multiple of 4 with ds)
  }
  const int unit_floats = static_cast<int>(bwd ? er::mha_bwd_floats(F, T, ds) : er::mha_fwd_floats(F, T, ds));
  const int bytes = 4 * unit_floats * G;
  const int64_t passes = er::ceil_div(a.units, static_cast<int64_t>(G));
  const dim3 grid(static_cast<unsigned>(passes < er::kMhaMaxGrid ? passes : er::kMhaMaxGrid)), block(er::kMhaThreads);
  const hipStream_t s = er::as_stream(stream);
  if (group) {
    const auto fn = bwd ? er::mha_group_bwd_kernel : er::mha_group_fwd_kernel;
    if (er::mha_set_lds(reinterpret_cast<const void*>(fn), bytes)) return 1;
    hipLaunchKernelGGL(fn, grid, block, bytes, s, a, G, unit_floats);
  } else {
    const auto fn = bwd ? er::mha_bwd_kernel : er::mha_fwd_kernel;
    if (er::mha_set_lds(reinterpret_cast<const void*>(fn), bytes)) return 1;
    hipLaunchKernelGGL(fn, grid, block, bytes, s, a);
  }
  ER_LAUNCH_CHECK();
  return 0;
}

int er_mha_fwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
               const int32_t* to_mask, int64_t B, int32_t F, int32_t T, int32_t H, int32_t ds, float* ctx,
               er_stream_t stream) {
  return mha_launch("er_mha_fwd", false, false, q, ldq, k, ldk, v, ldv, to_mask, nullptr, B, F, T, H, ds, ctx, nullptr, 0,
                    nullptr, 0, nullptr, 0, stream);
}

int er_mha_bwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
               const int32_t* to_mask, const float* dctx, int64_t B, int32_t F, int32_t T, int32_t H, int32_t ds,
               float* dq, int64_t lddq, float* dk, int64_t lddk, float* dv, int64_t lddv, er_stream_t stream) {
  return mha_launch("er_mha_bwd", true, false, q, ldq, k, ldk, v, ldv, to_mask, dctx, B, F, T, H, ds, nullptr, dq, lddq, dk,
                    lddk, dv, lddv, stream);
}

int32_t er_mha_group_units(int32_t F, int32_t T, int32_t ds) { return er::mha_group_units(F, T, ds); }

int er_mha_group_fwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                     const int32_t* to_mask, int64_t B, int32_t F, int32_t T, int32_t H, int32_t ds, float* ctx,
                     er_stream_t stream) {
  return mha_launch("er_mha_group_fwd", false, true, q, ldq, k, ldk, v, ldv, to_mask, nullptr, B, F, T, H, ds, ctx, nullptr,
                    0, nullptr, 0, nullptr, 0, stream);
}

int er_mha_group_bwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                     const int32_t* to_mask, const float* dctx, int64_t B, int32_t F, int32_t T, int32_t H, int32_t ds,
                     float* dq, int64_t lddq, float* dk, int64_t lddk, float* dv, int64_t lddv, er_stream_t stream) {
  return mha_launch("er_mha_group_bwd", true, true, q, ldq, k, ldk, v, ldv, to_mask, dctx, B, F, T, H, ds, nullptr, dq, lddq,
                    dk, lddk, dv, lddv, stream);
}

static int segment_mean_check(const char* what, const void* a, const void* seg_begin, const void* b, int64_t B, int32_t S,
                              int32_t W, int32_t n_seg) {
  ER_REQUIRE(a && seg_begin && b && B > 0, "%s: bad arguments", what);
  ER_REQUIRE(S >= 1 && S <= er::kSegMaxS && W >= 1 && W <= er::kSegMaxW, "%s: S = %d, W = %d outside 1 .. %d", what, S, W,
             er::kSegMaxW);
  ER_REQUIRE(n_seg >= 1 && n_seg <= er::kSegMaxSeg && n_seg <= S, "%s: n_seg = %d outside 1 .. min(%d, S)", what, n_seg,
             er::kSegMaxSeg);
  return 0;
}

int er_segment_mean_fwd(const float* x, const int32_t* seg_begin, const int32_t* lens, int64_t B, int32_t S, int32_t W,
                        int32_t n_seg, float* out, er_stream_t stream) {
  if (segment_mean_check("er_segment_mean_fwd", x, seg_begin, out, B, S, W, n_seg)) return 1;
  const bool vec = W % 4 == 0 && er::aligned16(x) && er::aligned16(out);
  const int64_t total = B * n_seg * (vec ? W / 4 : W);
  const int64_t blocks = er::ceil_div(total, static_cast<int64_t>(er::kBlock));
  const dim3 grid(static_cast<unsigned>(blocks < 8192 ? blocks : 8192)), block(er::kBlock);
  if (vec)
    hipLaunchKernelGGL(er::segment_mean_fwd_kernel<4>, grid, block, 0, er::as_stream(stream), x, seg_begin, lens, B, S, W,
                       n_seg, out);
  else
    hipLaunchKernelGGL(er::segment_mean_fwd_kernel<1>, grid, block, 0, er::as_stream(stream), x, seg_begin, lens, B, S, W,
                       n_seg, out);
  ER_LAUNCH_CHECK();
  return 0;
}

int er_segment_mean_bwd(const float* dout, const int32_t* seg_begin, const int32_t* lens, int64_t B, int32_t S, int32_t W,
                        int32_t n_seg, float* dx, er_stream_t stream) {
  if (segment_mean_check("er_segment_mean_bwd", dout, seg_begin, dx, B, S, W, n_seg)) return 1;
  const bool vec = W % 4 == 0 && er::aligned16(dout) && er::aligned16(dx);
  const int64_t total = B * n_seg * (vec ? W / 4 : W);
  const int64_t blocks = er::ceil_div(total, static_cast<int64_t>(er::kBlock));
  const dim3 grid(static_cast<unsigned>(blocks < 8192 ? blocks : 8192)), block(er::kBlock);
  if (vec)
    hipLaunchKernelGGL(er::segment_mean_bwd_kernel<4>, grid, block, 0, er::as_stream(stream), dout, seg_begin, lens, B, S, W,
                       n_seg, dx);
  else
    hipLaunchKernelGGL(er::segment_mean_bwd_kernel<1>, grid, block, 0, er::as_stream(stream), dout, seg_begin, lens, B, S, W,
                       n_seg, dx);
  ER_LAUNCH_CHECK();
  return 0;
}

int er_mha_pack(const float* w0, const float* w1, const float* w2, const float* b0, const float* b1, const float* b2,
                int32_t n, int32_t din, int32_t d, float* w, float* bias, er_stream_t stream) {
  ER_REQUIRE((n == 2 || n == 3) && din > 0 && d > 0 && w && bias, "er_mha_pack: bad arguments");
  ER_REQUIRE(w0 && w1 && b0 && b1 && (n == 2 || (w2 && b2)), "er_mha_pack: a source is null");
  er::MhaPackSrc src;
  src.w[0] = w0;
  src.w[1] = w1;
  src.w[2] = w2;
  src.b[0] = b0;
  src.b[1] = b1;
  src.b[2] = b2;
  const int64_t total = static_cast<int64_t>(din + 1) * n * d;
  const int64_t blocks = er::ceil_div(total, static_cast<int64_t>(er::kBlock));
  const int grid = static_cast<int>(blocks < 1024 ? blocks : 1024);
  hipLaunchKernelGGL(er::mha_pack_kernel, dim3(grid), dim3(er::kBlock), 0, er::as_stream(stream), src, n, din, d, w, bias);
  ER_LAUNCH_CHECK();
  return 0;
}

int32_t er_add_ln_grid(int64_t rows, int32_t W) {
  if (rows < 1 || W < 1 || W > er::kLnMaxW) return 0;
  const int64_t n = er::ceil_div(rows, static_cast<int64_t>(er::kBlock / er::kWave));
  return static_cast<int32_t>(n < er::kLnMaxGrid ? n : er::kLnMaxGrid);
}

int er_add_ln_fwd(const float* x, const float* res, int64_t rows, int64_t res_rows, int32_t W, const float* gamma,
                  const float* beta, float eps, float* y, float* mean, float* rstd, er_stream_t stream) {
  ER_REQUIRE(x && gamma && beta && y && mean && rstd && rows > 0, "er_add_ln_fwd: bad arguments");
  ER_REQUIRE(W >= 1 && W <= er::kLnMaxW, "er_add_ln_fwd: W = %d outside 1 .. %d", W, er::kLnMaxW);
  ER_REQUIRE(res == nullptr || res_rows >= 1, "er_add_ln_fwd: res_rows = %lld", static_cast<long long>(res_rows));
  const int64_t n = er::ceil_div(rows, static_cast<int64_t>(er::kBlock / er::kWave));
  const dim3 grid(static_cast<unsigned>(n < 8192 ? n : 8192)), block(er::kBlock);
  const hipStream_t s = er::as_stream(stream);
  if (res == nullptr) res_rows = 1;
#define ER_LN_FWD(KERNEL) hipLaunchKernelGGL(KERNEL, grid, block, 0, s, x, res, rows, res_rows, W, gamma, beta, eps, y, mean, rstd)
  if (!er::ln_vec_ok(W, {x, res, gamma, beta, y}))
    ER_LN_FWD(er::add_ln_fwd_kernel);
  else if (W <= 256)
    ER_LN_FWD(er::add_ln_fwd_vec_kernel<1>);
  else if (W <= 512)
    ER_LN_FWD(er::add_ln_fwd_vec_kernel<2>);
  else
    ER_LN_FWD(er::add_ln_fwd_vec_kernel<4>);
#undef ER_LN_FWD
  ER_LAUNCH_CHECK();
  return 0;
}

int er_add_ln_bwd(const float* dy, const float* x, const float* res, int64_t rows, int64_t res_rows, int32_t W,
                  const float* gamma, const float* mean, const float* rstd, float* dz, float* partials,
                  er_stream_t stream) {
  ER_REQUIRE(dy && x && gamma && mean && rstd && dz && partials && rows > 0, "er_add_ln_bwd: bad arguments");
  ER_REQUIRE(W >= 1 && W <= er::kLnMaxW, "er_add_ln_bwd: W = %d outside 1 .. %d", W, er::kLnMaxW);
  ER_REQUIRE(res == nullptr || res_rows >= 1, "er_add_ln_bwd: res_rows = %lld", static_cast<long long>(res_rows));
  const dim3 grid(er_add_ln_grid(rows, W)), block(er::kBlock);
  const hipStream_t s = er::as_stream(stream);
  if (res == nullptr) res_rows = 1;
#define ER_LN_BWD(KERNEL) hipLaunchKernelGGL(KERNEL, grid, block, 0, s, dy, x, res, rows, res_rows, W, gamma, mean, rstd, dz, partials)
  if (!er::ln_vec_ok(W, {dy, x, res, gamma, dz}))
    ER_LN_BWD(er::add_ln_bwd_kernel);
  else if (W <= 256)
    ER_LN_BWD(er::add_ln_bwd_vec_kernel<1>);
  else if (W <= 512)
    ER_LN_BWD(er::add_ln_bwd_vec_kernel<2>);
  else
    ER_LN_BWD(er::add_ln_bwd_vec_kernel<4>);
#undef ER_LN_BWD
  ER_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
