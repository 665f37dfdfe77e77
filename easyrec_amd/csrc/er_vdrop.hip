// K8k: variational dropout on a feature group's concatenated output (reference layers/variational_dropout_layer.py,
// "Dropout Feature Ranking for Deep Learning Models", arXiv 1712.08645).  With p = sigmoid(logit_p) [P], uniform noise
// u [B, P] and EPS = 2.220446e-16 as an fp32 constant:
//   training    a = log(p + EPS) - log(1 - p + EPS) + log(u + EPS) - log(1 - u + EPS), summed left to right
//               m = 1 - sigmoid(a / 0.1);  out[b, c] = x[b, c] * m[b, seg(c)]
//   evaluation  (u == NULL) m[b, j] = 1 - p[j]
//   penalty     lambda_over_rows * sum_j (1 - p[j])
// seg is the column -> parameter map (the feature that owns column c); NULL is the identity (P == W: one probability per
// embedding column).  One launch forward instead of about a dozen elementwise ones; one launch backward, which
// recomputes m, plus the shared fixed-order reduce for dlogit_p.
//
// fp32, streaming: no MFMA, no atomics, no mask saved.  x stays where the engine left it (a row pitch of its own).
//
// Geometry, both directions: er_vdrop_grid = min(ceil(B / 8), 1024) workgroups of 256 threads; workgroup g owns the rows
// [g * per, min(B, (g + 1) * per)), per = ceil(B / grid).  The unit of work within a row is a PIECE:
//   identity   V adjacent columns = V parameters (V = 4 on the 16-byte path, 1 on the 4-byte path); np = W / V pieces
//   seg        one parameter j and its columns [c0, c1) (found by binary search in seg); np = P pieces; the columns are
//              walked in ascending order, V at a time
// TC = min(np, 256), RL = 256 / TC; thread t is piece lane t % TC and row lane t / TC (t >= TC * RL idle); it walks the
// pieces tc, tc + TC, .. and, per piece, the rows r0 + rl, r0 + rl + RL, ...
//
// dlogit_p.  Per (row, parameter) the thread forms acc = sum over the parameter's columns of dout * x in ascending
// column order from 0.f (identity: the one product), then adds dm/dlogit * acc to its row sum in the order it walks the
// rows, from 0.f.  With RL > 1 the row lanes' sums meet in LDS and are combined in the order 0, 1, .., RL - 1.  Workgroup
// g's sums are row g of partials [grid + 1, P]; row `grid` is the penalty's own gradient, written by workgroup 0.
// er_theta_grad_reduce (row_groups = 8) then sums the grid + 1 rows.  Every order is fixed.
//
// Finite for every finite input: sigmoid(t) = 1 / (1 + expf(-t)) is 0 where expf overflows to +inf (t below about -88.7)
// and 1 where it underflows; |a / 0.1| reaches 720 (u = 0 against logit_p = +-100).  logf / expf are the precise ones.
#include <math.h>

#include "er_common.h"

namespace er {

constexpr int kVdropMaxW = 4096;
constexpr int kVdropRowsPerWg = 8;
constexpr int kVdropMaxGrid = 1024;
constexpr float kVdropEps = 2.220446049250313e-16f;  // np.finfo(float).eps as an fp32 constant
constexpr float kVdropTemp = 0.1f;

__device__ __forceinline__ float vd_sigmoid(float t) { return 1.0f / (1.0f + expf(-t)); }

// what depends on the parameter alone
struct VdParam {
  float p;     // sigmoid(logit_p)
  float lp;    // log(p + EPS) - log(1 - p + EPS)
  float dadl;  // da / dlogit_p = p (1 - p) (1 / (p + EPS) + 1 / (1 - p + EPS))
};
__device__ __forceinline__ VdParam vd_param(float logit) {
  VdParam q;
  q.p = vd_sigmoid(logit);
  const float a = q.p + kVdropEps, b = (1.0f - q.p) + kVdropEps;
  q.lp = logf(a) - logf(b);
  q.dadl = q.p * (1.0f - q.p) * (1.0f / a + 1.0f / b);
  return q;
}
// m and dm / dlogit_p of one (row, parameter); training: u is the row's draw
__device__ __forceinline__ void vd_mask(const VdParam& q, bool train, float u, float* m, float* dmdl) {
  if (!train) {
    *m = 1.0f - q.p;
    *dmdl = -(q.p * (1.0f - q.p));
    return;
  }
  const float a = (q.lp + logf(u + kVdropEps)) - logf((1.0f - u) + kVdropEps);
  const float s = vd_sigmoid(a / kVdropTemp);
  *m = 1.0f - s;
  *dmdl = -10.0f * s * (1.0f - s) * q.dadl;
}

// this thread's place in the shared geometry; false: the thread is idle
struct VdPlace {
  int np, TC, RL, tc, rl;
  int64_t r0, r1;
};
__device__ __forceinline__ bool vd_place(int64_t B, int np, VdPlace* p) {
  p->np = np;
  p->TC = np < kBlock ? np : kBlock;
  p->RL = kBlock / p->TC;
  p->tc = static_cast<int>(threadIdx.x) % p->TC;
  p->rl = static_cast<int>(threadIdx.x) / p->TC;
  const int64_t per = (B + gridDim.x - 1) / gridDim.x;
  p->r0 = min(B, static_cast<int64_t>(blockIdx.x) * per);
  p->r1 = min(B, p->r0 + per);
  return p->rl < p->RL;
}

// first column c in [0, W] with seg[c] >= j (seg non-decreasing); never leaves [0, W] whatever seg holds
__device__ __forceinline__ int vd_lower_bound(const int32_t* __restrict__ seg, int W, int j) {
  int lo = 0, hi = W;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (seg[mid] < j)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// ---------------------------------------------------------------------------------------------------- forward
// the penalty, by workgroup 0: thread t sums 1 - p over j = t, t + 256, .. from 0.f, then block_sum_256's fixed tree
__device__ __forceinline__ void vd_penalty(const float* __restrict__ logit_p, int P, float lam, float* __restrict__ penalty) {
  __shared__ float red[4];
  float s = 0.f;
  for (int j = threadIdx.x; j < P; j += kBlock) s += 1.0f - vd_sigmoid(logit_p[j]);
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) penalty[0] = lam * s;
}

template <int V>
__global__ __launch_bounds__(kBlock) void vdrop_fwd_kernel(const float* __restrict__ x, int64_t ldx,
                                                          const float* __restrict__ logit_p, const float* __restrict__ u,
                                                          int64_t ldu, int64_t B, int W, float lam, float* __restrict__ out,
                                                          int64_t ldout, float* __restrict__ penalty) {
  VdPlace pl;
  if (vd_place(B, W / V, &pl)) {
    for (int pc = pl.tc; pc < pl.np; pc += pl.TC) {
      const int col = pc * V;
      VdParam q[V];
#pragma unroll
      for (int v = 0; v < V; ++v) q[v] = vd_param(logit_p[col + v]);
      for (int64_t r = pl.r0 + pl.rl; r < pl.r1; r += pl.RL) {
        alignas(16) float xv[V], uv[V], ov[V];
        if constexpr (V == 4) {
          *reinterpret_cast<float4*>(xv) = *reinterpret_cast<const float4*>(x + r * ldx + col);
          if (u != nullptr) *reinterpret_cast<float4*>(uv) = *reinterpret_cast<const float4*>(u + r * ldu + col);
        } else {
          xv[0] = x[r * ldx + col];
          if (u != nullptr) uv[0] = u[r * ldu + col];
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
          float m, dmdl;
          vd_mask(q[v], u != nullptr, u != nullptr ? uv[v] : 0.f, &m, &dmdl);
          ov[v] = xv[v] * m;
        }
        if constexpr (V == 4)
          *reinterpret_cast<float4*>(out + r * ldout + col) = *reinterpret_cast<const float4*>(ov);
        else
          out[r * ldout + col] = ov[0];
      }
    }
  }
  if (blockIdx.x == 0) vd_penalty(logit_p, W, lam, penalty);  // (uniform over the workgroup; identity: P == W)
}

template <int V>
__global__ __launch_bounds__(kBlock) void vdrop_seg_fwd_kernel(const float* __restrict__ x, int64_t ldx,
                                                              const float* __restrict__ logit_p,
                                                              const float* __restrict__ u, int64_t ldu,
                                                              const int32_t* __restrict__ seg, int64_t B, int W, int P,
                                                              float lam, float* __restrict__ out, int64_t ldout,
                                                              float* __restrict__ penalty) {
  VdPlace pl;
  if (vd_place(B, P, &pl)) {
    for (int j = pl.tc; j < pl.np; j += pl.TC) {
      const int c0 = vd_lower_bound(seg, W, j), c1 = vd_lower_bound(seg, W, j + 1);
      const VdParam q = vd_param(logit_p[j]);
      for (int64_t r = pl.r0 + pl.rl; r < pl.r1; r += pl.RL) {
        float m, dmdl;
        vd_mask(q, u != nullptr, u != nullptr ? u[r * ldu + j] : 0.f, &m, &dmdl);
        const float* __restrict__ xr = x + r * ldx;
        float* __restrict__ orow = out + r * ldout;
        for (int c = c0; c + V <= c1; c += V) {
          if constexpr (V == 4) {
            const float4 xv = *reinterpret_cast<const float4*>(xr + c);
            *reinterpret_cast<float4*>(orow + c) = make_float4(xv.x * m, xv.y * m, xv.z * m, xv.w * m);
          } else {
            orow[c] = xr[c] * m;
          }
        }
      }
    }
  }
  if (blockIdx.x == 0) vd_penalty(logit_p, P, lam, penalty);
}

// ---------------------------------------------------------------------------------------------------- backward
// after the main loop: the row lanes' sums combined through LDS (RL > 1), and the penalty's own gradient as row `grid`
__device__ __forceinline__ void vd_finish_partials(const VdPlace& pl, const float* acc, int P, const float* logit_p,
                                                   float lam, const float* gpen, float* __restrict__ partials) {
  if (pl.RL > 1) {  // (uniform over the workgroup; np < 256: the main loop ran once)
    __syncthreads();
    float* __restrict__ prow = partials + static_cast<int64_t>(blockIdx.x) * P;
    for (int j = threadIdx.x; j < P; j += kBlock) {
      float s = acc[j];
      for (int rl = 1; rl < pl.RL; ++rl) s += acc[rl * P + j];
      prow[j] = s;
    }
  }
  if (blockIdx.x == 0) {
    float* __restrict__ last = partials + static_cast<int64_t>(gridDim.x) * P;
    const float g = gpen != nullptr ? gpen[0] : 0.f;
    for (int j = threadIdx.x; j < P; j += kBlock) {
      const float p = vd_sigmoid(logit_p[j]);
      last[j] = gpen != nullptr ? -(lam * (p * (1.0f - p))) * g : 0.f;
    }
  }
}

template <int V>
__global__ __launch_bounds__(kBlock) void vdrop_bwd_kernel(const float* __restrict__ dout, int64_t lddout,
                                                          const float* __restrict__ x, int64_t ldx,
                                                          const float* __restrict__ logit_p, const float* __restrict__ u,
                                                          int64_t ldu, int64_t B, int W, float lam,
                                                          const float* __restrict__ gpen, float* __restrict__ dx,
                                                          int64_t lddx, float* __restrict__ partials) {
  __shared__ float acc[kBlock * V];  // [RL][W] when RL > 1 (W = TC * V <= 255 * V)
  VdPlace pl;
  const bool active = vd_place(B, W / V, &pl);
  if (active) {
    for (int pc = pl.tc; pc < pl.np; pc += pl.TC) {
      const int col = pc * V;
      VdParam q[V];
      float sum[V];
#pragma unroll
      for (int v = 0; v < V; ++v) {
        q[v] = vd_param(logit_p[col + v]);
        sum[v] = 0.f;
      }
      for (int64_t r = pl.r0 + pl.rl; r < pl.r1; r += pl.RL) {
        alignas(16) float dv[V], xv[V], uv[V], gx[V];
        if constexpr (V == 4) {
          *reinterpret_cast<float4*>(dv) = *reinterpret_cast<const float4*>(dout + r * lddout + col);
          *reinterpret_cast<float4*>(xv) = *reinterpret_cast<const float4*>(x + r * ldx + col);
          if (u != nullptr) *reinterpret_cast<float4*>(uv) = *reinterpret_cast<const float4*>(u + r * ldu + col);
        } else {
          dv[0] = dout[r * lddout + col];
          xv[0] = x[r * ldx + col];
          if (u != nullptr) uv[0] = u[r * ldu + col];
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
          float m, dmdl;
          vd_mask(q[v], u != nullptr, u != nullptr ? uv[v] : 0.f, &m, &dmdl);
          gx[v] = dv[v] * m;
          sum[v] = sum[v] + dmdl * (dv[v] * xv[v]);
        }
        if (dx != nullptr) {
          if constexpr (V == 4)
            *reinterpret_cast<float4*>(dx + r * lddx + col) = *reinterpret_cast<const float4*>(gx);
          else
            dx[r * lddx + col] = gx[0];
        }
      }
      float* __restrict__ dst = pl.RL == 1 ? partials + static_cast<int64_t>(blockIdx.x) * W + col : acc + pl.rl * W + col;
#pragma unroll
      for (int v = 0; v < V; ++v) dst[v] = sum[v];
    }
  }
  vd_finish_partials(pl, acc, W, logit_p, lam, gpen, partials);
}

template <int V>
__global__ __launch_bounds__(kBlock) void vdrop_seg_bwd_kernel(const float* __restrict__ dout, int64_t lddout,
                                                              const float* __restrict__ x, int64_t ldx,
                                                              const float* __restrict__ logit_p,
                                                              const float* __restrict__ u, int64_t ldu,
                                                              const int32_t* __restrict__ seg, int64_t B, int W, int P,
                                                              float lam, const float* __restrict__ gpen,
                                                              float* __restrict__ dx, int64_t lddx,
                                                              float* __restrict__ partials) {
  __shared__ float acc[kBlock];  // [RL][P] when RL > 1 (P = TC <= 255)
  VdPlace pl;
  const bool active = vd_place(B, P, &pl);
  if (active) {
    for (int j = pl.tc; j < pl.np; j += pl.TC) {
      const int c0 = vd_lower_bound(seg, W, j), c1 = vd_lower_bound(seg, W, j + 1);
      const VdParam q = vd_param(logit_p[j]);
      float sum = 0.f;
      for (int64_t r = pl.r0 + pl.rl; r < pl.r1; r += pl.RL) {
        float m, dmdl;
        vd_mask(q, u != nullptr, u != nullptr ? u[r * ldu + j] : 0.f, &m, &dmdl);
        const float* __restrict__ dr = dout + r * lddout;
        const float* __restrict__ xr = x + r * ldx;
        float* __restrict__ gr = dx != nullptr ? dx + r * lddx : nullptr;
        float dot = 0.f;
        for (int c = c0; c + V <= c1; c += V) {
          if constexpr (V == 4) {
            const float4 dv = *reinterpret_cast<const float4*>(dr + c);
            const float4 xv = *reinterpret_cast<const float4*>(xr + c);
            if (gr != nullptr) *reinterpret_cast<float4*>(gr + c) = make_float4(dv.x * m, dv.y * m, dv.z * m, dv.w * m);
            dot = dot + dv.x * xv.x;
            dot = dot + dv.y * xv.y;
            dot = dot + dv.z * xv.z;
            dot = dot + dv.w * xv.w;
          } else {
            const float dv = dr[c];
            if (gr != nullptr) gr[c] = dv * m;
            dot = dot + dv * xr[c];
          }
        }
        sum = sum + dmdl * dot;
      }
      if (pl.RL == 1)
        partials[static_cast<int64_t>(blockIdx.x) * P + j] = sum;
      else
        acc[pl.rl * P + j] = sum;
    }
  }
  vd_finish_partials(pl, acc, P, logit_p, lam, gpen, partials);
}

inline bool vd_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline bool vd_shape_ok(int64_t B, int32_t W) { return B >= 1 && W >= 1 && W <= kVdropMaxW; }

// seg_host: non-decreasing, from 0, in steps of at most 1, up to P - 1 (every parameter owns >= 1 column); *quads: every
// segment starts at a multiple of 4 columns
inline bool vd_seg_ok(const int32_t* seg_host, int32_t W, int32_t P, bool* quads) {
  *quads = true;
  if (seg_host[0] != 0 || seg_host[W - 1] != P - 1) return false;
  for (int32_t c = 1; c < W; ++c) {
    const int32_t d = seg_host[c] - seg_host[c - 1];
    if (d != 0 && d != 1) return false;
    if (d == 1 && c % 4 != 0) *quads = false;
  }
  return true;
}

}  // namespace er

extern "C" {

int32_t er_vdrop_grid(int64_t B, int32_t W) {
  if (!er::vd_shape_ok(B, W)) return 0;
  const int64_t g = er::ceil_div(B, static_cast<int64_t>(er::kVdropRowsPerWg));
  return static_cast<int32_t>(g < er::kVdropMaxGrid ? g : er::kVdropMaxGrid);
}

int er_vdrop_fwd(const float* x, int64_t ldx, const float* logit_p, const float* u, int64_t ldu, const int32_t* seg_host,
                 const int32_t* seg, int64_t B, int32_t W, int32_t P, float lambda_over_rows, float* out, int64_t ldout,
                 float* penalty, er_stream_t stream) {
  ER_REQUIRE(er::vd_shape_ok(B, W) && P >= 1 && P <= W, "er_vdrop_fwd: B = %lld, W = %d, P = %d outside the envelope",
             static_cast<long long>(B), W, P);
  ER_REQUIRE(x && logit_p && out && penalty && (seg_host != nullptr) == (seg != nullptr), "er_vdrop_fwd: bad arguments");
  ER_REQUIRE(seg != nullptr || P == W, "er_vdrop_fwd: P = %d != W = %d without a column map", P, W);
  ER_REQUIRE(ldx >= W && ldout >= W && (u == nullptr || ldu >= P), "er_vdrop_fwd: a pitch below the row's width");
  bool quads = true;
  ER_REQUIRE(seg == nullptr || er::vd_seg_ok(seg_host, W, P, &quads),
             "er_vdrop_fwd: the column map is not non-decreasing over 0 .. P - 1");
  bool vec = W % 4 == 0 && ldx % 4 == 0 && ldout % 4 == 0 && er::vd_aligned16(x) && er::vd_aligned16(out) && quads;
  if (seg == nullptr) vec = vec && er::vd_aligned16(logit_p) && (u == nullptr || (ldu % 4 == 0 && er::vd_aligned16(u)));
  const dim3 grid(er_vdrop_grid(B, W)), block(er::kBlock);
  const hipStream_t s = er::as_stream(stream);
  if (seg == nullptr) {
    if (vec)
      hipLaunchKernelGGL(er::vdrop_fwd_kernel<4>, grid, block, 0, s, x, ldx, logit_p, u, ldu, B, W, lambda_over_rows, out,
                         ldout, penalty);
    else
      hipLaunchKernelGGL(er::vdrop_fwd_kernel<1>, grid, block, 0, s, x, ldx, logit_p, u, ldu, B, W, lambda_over_rows, out,
                         ldout, penalty);
  } else {
    if (vec)
      hipLaunchKernelGGL(er::vdrop_seg_fwd_kernel<4>, grid, block, 0, s, x, ldx, logit_p, u, ldu, seg, B, W, P,
                         lambda_over_rows, out, ldout, penalty);
    else
      hipLaunchKernelGGL(er::vdrop_seg_fwd_kernel<1>, grid, block, 0, s, x, ldx, logit_p, u, ldu, seg, B, W, P,
                         lambda_over_rows, out, ldout, penalty);
  }
  ER_LAUNCH_CHECK();
  return 0;
}

int er_vdrop_bwd(const float* dout, int64_t lddout, const float* x, int64_t ldx, const float* logit_p, const float* u,
                 int64_t ldu, const int32_t* seg_host, const int32_t* seg, int64_t B, int32_t W, int32_t P,
                 float lambda_over_rows, const float* dpenalty, float* dx, int64_t lddx, float* partials,
                 er_stream_t stream) {
  ER_REQUIRE(er::vd_shape_ok(B, W) && P >= 1 && P <= W, "er_vdrop_bwd: B = %lld, W = %d, P = %d outside the envelope",
             static_cast<long long>(B), W, P);
  ER_REQUIRE(dout && x && logit_p && partials && (seg_host != nullptr) == (seg != nullptr), "er_vdrop_bwd: bad arguments");
  ER_REQUIRE(seg != nullptr || P == W, "er_vdrop_bwd: P = %d != W = %d without a column map", P, W);
  ER_REQUIRE(lddout >= W && ldx >= W && (u == nullptr || ldu >= P) && (dx == nullptr || lddx >= W),
             "er_vdrop_bwd: a pitch below the row's width");
  bool quads = true;
  ER_REQUIRE(seg == nullptr || er::vd_seg_ok(seg_host, W, P, &quads),
             "er_vdrop_bwd: the column map is not non-decreasing over 0 .. P - 1");
  bool vec = W % 4 == 0 && lddout % 4 == 0 && ldx % 4 == 0 && er::vd_aligned16(dout) && er::vd_aligned16(x) && quads &&
             (dx == nullptr || (lddx % 4 == 0 && er::vd_aligned16(dx)));
  if (seg == nullptr) vec = vec && er::vd_aligned16(logit_p) && (u == nullptr || (ldu % 4 == 0 && er::vd_aligned16(u)));
  const dim3 grid(er_vdrop_grid(B, W)), block(er::kBlock);
  const hipStream_t s = er::as_stream(stream);
  if (seg == nullptr) {
    if (vec)
      hipLaunchKernelGGL(er::vdrop_bwd_kernel<4>, grid, block, 0, s, dout, lddout, x, ldx, logit_p, u, ldu, B, W,
                         lambda_over_rows, dpenalty, dx, lddx, partials);
    else
      hipLaunchKernelGGL(er::vdrop_bwd_kernel<1>, grid, block, 0, s, dout, lddout, x, ldx, logit_p, u, ldu, B, W,
                         lambda_over_rows, dpenalty, dx, lddx, partials);
  } else {
    if (vec)
      hipLaunchKernelGGL(er::vdrop_seg_bwd_kernel<4>, grid, block, 0, s, dout, lddout, x, ldx, logit_p, u, ldu, seg, B, W,
                         P, lambda_over_rows, dpenalty, dx, lddx, partials);
    else
      hipLaunchKernelGGL(er::vdrop_seg_bwd_kernel<1>, grid, block, 0, s, dout, lddout, x, ldx, logit_p, u, ldu, seg, B, W,
                         P, lambda_over_rows, dpenalty, dx, lddx, partials);
  }
  ER_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
