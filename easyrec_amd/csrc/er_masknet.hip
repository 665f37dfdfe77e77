// K8i: MaskNet's two launches that are neither a Dense layer nor an existing kernel (reference
// layers/keras/mask_net.py): the instance-guided mask multiply net * weights (:100) of up to 8 blocks over one input, and
// the LayerNormalization + ReLU that ends every block (:106-107; keras' epsilon 1e-3), written straight into the
// blocks' concatenation.
//
// The operands stay where the Dense layers left them: every launch takes HOST arrays of device pointers and pitches, one
// entry per block, copied by value into the kernel's argument record (under 1 KB), so nothing is built on the device and a
// first call inside a stream capture works.  fp32, streaming: no LDS tiles, no MFMA, no atomics; every sum in a fixed
// order, so two runs and a graph replay give the same bits.
//
// Mask multiply.  A thread owns one 16-byte (or, on the scalar path, 4-byte) piece of a row for ALL blocks: x is read
// once.  The backward's dx is one fmaf chain per element over the blocks ascending, the first term a plain product.
//
// LayerNorm + ReLU.  The arithmetic of er_mha.hip's add_ln_* kernels with res = NULL: one wave per (row, block), the
// block being blockIdx.y; O % 4 == 0, O <= 1024 and 16-byte aligned operands keep the row in registers between the
// passes, anything else re-reads it.  The backward takes the ReLU pattern from the saved output (y > 0) and leaves
// dgamma_i | dbeta_i as per-workgroup partial sums at columns [2 i O, 2 (i + 1) O) of partials [grid, 2 n O] for
// er_theta_grad_reduce.
#include <math.h>

#include "er_common.h"

namespace er {

constexpr int kMaskMaxN = 8;
constexpr int kMaskMaxW = 4096;
constexpr int kMaskMaxGrid = 8192;
constexpr int kLnReluMaxO = 4096;
constexpr int kLnReluMaxGrid = 1024;   // rows of `partials`
constexpr int kLnReluRegO = 1024;      // widest row the register form keeps (4 float4 per lane)
constexpr int kThetaMaxP = 65536;      // er_theta_grad_reduce takes P < 65536

struct MaskMulArgs {
  const float* v[kMaskMaxN];
  const float* d[kMaskMaxN];  // dout (backward)
  float* o[kMaskMaxN];        // out (forward), dv (backward)
  int64_t ldv[kMaskMaxN], ldd[kMaskMaxN], ldo[kMaskMaxN];
};

struct LnReluArgs {
  const float* h[kMaskMaxN];
  const float* gamma[kMaskMaxN];
  const float* beta[kMaskMaxN];
  float* dh[kMaskMaxN];
  int64_t ldh[kMaskMaxN], lddh[kMaskMaxN];
};

template <int V>
struct Piece;
template <>
struct Piece<1> {
  typedef float T;
  static __device__ __forceinline__ float mul(float a, float b) { return a * b; }
  static __device__ __forceinline__ float fma(float a, float b, float c) { return fmaf(a, b, c); }
};
template <>
struct Piece<4> {
  typedef float4 T;
  static __device__ __forceinline__ float4 mul(float4 a, float4 b) {
    return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
  }
  static __device__ __forceinline__ float4 fma(float4 a, float4 b, float4 c) {
    return make_float4(fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w));
  }
};

template <int V>
__global__ __launch_bounds__(kBlock) void mask_mul_fwd_kernel(const float* __restrict__ x, int64_t ldx, MaskMulArgs a, int n,
                                                             int64_t B, int W) {
  typedef typename Piece<V>::T T;
  const int wc = W / V;
  const int64_t total = B * wc, step = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < total; e += step) {
    const int64_t b = e / wc;
    const int c = static_cast<int>(e - b * wc) * V;
    const T xv = *reinterpret_cast<const T*>(x + b * ldx + c);
    for (int i = 0; i < n; ++i) {
      const T vv = *reinterpret_cast<const T*>(a.v[i] + b * a.ldv[i] + c);
      *reinterpret_cast<T*>(a.o[i] + b * a.ldo[i] + c) = Piece<V>::mul(xv, vv);
    }
  }
}

template <int V>
__global__ __launch_bounds__(kBlock) void mask_mul_bwd_kernel(const float* __restrict__ x, int64_t ldx, MaskMulArgs a, int n,
                                                             int64_t B, int W, float* __restrict__ dx, int64_t lddx) {
  typedef typename Piece<V>::T T;
  const int wc = W / V;
  const int64_t total = B * wc, step = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < total; e += step) {
    const int64_t b = e / wc;
    const int c = static_cast<int>(e - b * wc) * V;
    const T xv = *reinterpret_cast<const T*>(x + b * ldx + c);
    T acc = {};
    for (int i = 0; i < n; ++i) {
      const T dv = *reinterpret_cast<const T*>(a.d[i] + b * a.ldd[i] + c);
      *reinterpret_cast<T*>(a.o[i] + b * a.ldo[i] + c) = Piece<V>::mul(dv, xv);
      if (dx != nullptr) {
        const T vv = *reinterpret_cast<const T*>(a.v[i] + b * a.ldv[i] + c);
        acc = i == 0 ? Piece<V>::mul(dv, vv) : Piece<V>::fma(dv, vv, acc);
      }
    }
    if (dx != nullptr) *reinterpret_cast<T*>(dx + b * lddx + c) = acc;
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// ------------------------------------------------------------------------------------------------ LayerNorm + ReLU
template <int NV>
__global__ __launch_bounds__(kBlock) void ln_relu_fwd_vec_kernel(LnReluArgs a, int64_t B, int O, float eps,
                                                                float* __restrict__ y, int64_t ldy,
                                                                float* __restrict__ mean, float* __restrict__ rstd) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, blk = blockIdx.y;
  const float* __restrict__ h = a.h[blk];
  const float* __restrict__ gamma = a.gamma[blk];
  const float* __restrict__ beta = a.beta[blk];
  const int64_t ldh = a.ldh[blk];
  const int64_t step = static_cast<int64_t>(gridDim.x) * (kBlock / kWave);
  const float inv_w = 1.0f / static_cast<float>(O);
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * (kBlock / kWave) + wave; r < B; r += step) {
    const float* hr = h + r * ldh;
    float4 z[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int c = (k * kWave + lane) << 2;
      z[k] = c < O ? ld4(hr + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float shift = __shfl(z[0].x, 0, kWave);  // the row's first element
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k)
      if (((k * kWave + lane) << 2) < O) {
        s += z[k].x - shift;
        s += z[k].y - shift;
        s += z[k].z - shift;
        s += z[k].w - shift;
      }
    const float mu = shift + wave_sum(s) * inv_w;
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k)
      if (((k * kWave + lane) << 2) < O) {
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
    float* yr = y + r * ldy + static_cast<int64_t>(blk) * O;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int c = (k * kWave + lane) << 2;
      if (c < O) {
        const float4 ga = ld4(gamma + c), be = ld4(beta + c);
        float4 o;
        o.x = fmaxf(0.f, z[k].x * rs * ga.x + be.x);
        o.y = fmaxf(0.f, z[k].y * rs * ga.y + be.y);
        o.z = fmaxf(0.f, z[k].z * rs * ga.z + be.z);
        o.w = fmaxf(0.f, z[k].w * rs * ga.w + be.w);
        *reinterpret_cast<float4*>(yr + c) = o;
      }
    }
    if (lane == 0) {
      mean[blk * B + r] = mu;
      rstd[blk * B + r] = rs;
    }
  }
}

// any width and alignment: the row is read three times
__global__ __launch_bounds__(kBlock) void ln_relu_fwd_kernel(LnReluArgs a, int64_t B, int O, float eps, float* __restrict__ y,
                                                            int64_t ldy, float* __restrict__ mean,
                                                            float* __restrict__ rstd) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, blk = blockIdx.y;
  const float* __restrict__ h = a.h[blk];
  const float* __restrict__ gamma = a.gamma[blk];
  const float* __restrict__ beta = a.beta[blk];
  const int64_t ldh = a.ldh[blk];
  const int64_t step = static_cast<int64_t>(gridDim.x) * (kBlock / kWave);
  const float inv_w = 1.0f / static_cast<float>(O);
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * (kBlock / kWave) + wave; r < B; r += step) {
    const float* hr = h + r * ldh;
    const float shift = hr[0];
    float s = 0.f;
    for (int c = lane; c < O; c += kWave) s += hr[c] - shift;
    const float mu = shift + wave_sum(s) * inv_w;
    float v = 0.f;
    for (int c = lane; c < O; c += kWave) {
      const float d = hr[c] - mu;
      v += d * d;
    }
    const float rs = 1.0f / sqrtf(wave_sum(v) * inv_w + eps);
    float* yr = y + r * ldy + static_cast<int64_t>(blk) * O;
    for (int c = lane; c < O; c += kWave) yr[c] = fmaxf(0.f, (hr[c] - mu) * rs * gamma[c] + beta[c]);
    if (lane == 0) {
      mean[blk * B + r] = mu;
      rstd[blk * B + r] = rs;
    }
  }
}

// rows [r0, r1) of workgroup blockIdx.x: a contiguous stretch of ceil(B / grid)
__device__ __forceinline__ void ln_relu_row_range(int64_t B, int64_t* r0, int64_t* r1) {
  const int64_t per = (B + gridDim.x - 1) / gridDim.x;
  *r0 = min(B, static_cast<int64_t>(blockIdx.x) * per);
  *r1 = min(B, *r0 + per);
}

template <int NV>
__global__ __launch_bounds__(kBlock) void ln_relu_bwd_vec_kernel(const float* __restrict__ dy, int64_t lddy,
                                                                const float* __restrict__ y, int64_t ldy, LnReluArgs a,
                                                                int64_t B, int O, int n, const float* __restrict__ mean,
                                                                const float* __restrict__ rstd,
                                                                float* __restrict__ partials) {
  __shared__ float acc[kBlock / kWave][2 * kLnReluRegO];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, blk = blockIdx.y;
  const float* __restrict__ h = a.h[blk];
  const float* __restrict__ gamma = a.gamma[blk];
  float* __restrict__ dh = a.dh[blk];
  const int64_t ldh = a.ldh[blk], lddh = a.lddh[blk], col0 = static_cast<int64_t>(blk) * O;
  const float inv_w = 1.0f / static_cast<float>(O);
  int64_t r0, r1;
  ln_relu_row_range(B, &r0, &r1);
  float4 ga[NV], dg[NV], db[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c = (k * kWave + lane) << 2;
    ga[k] = c < O ? ld4(gamma + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    dg[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    db[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  for (int64_t r = r0 + wave; r < r1; r += kBlock / kWave) {
    const float mu = mean[blk * B + r], rs = rstd[blk * B + r];
    float4 xh[NV], g[NV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int c = (k * kWave + lane) << 2;
      xh[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      g[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < O) {
        const float4 z = ld4(h + r * ldh + c);
        const float4 yo = ld4(y + r * ldy + col0 + c);
        float4 d = ld4(dy + r * lddy + col0 + c);
        d.x = yo.x > 0.f ? d.x : 0.f;
        d.y = yo.y > 0.f ? d.y : 0.f;
        d.z = yo.z > 0.f ? d.z : 0.f;
        d.w = yo.w > 0.f ? d.w : 0.f;
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
      if (c < O) {
        float4 o;
        o.x = rs * (g[k].x - m1 - xh[k].x * m2);
        o.y = rs * (g[k].y - m1 - xh[k].y * m2);
        o.z = rs * (g[k].z - m1 - xh[k].z * m2);
        o.w = rs * (g[k].w - m1 - xh[k].w * m2);
        *reinterpret_cast<float4*>(dh + r * lddh + c) = o;
      }
    }
  }
  // the four waves' column sums, combined in the order 0, 1, 2, 3
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c = (k * kWave + lane) << 2;
    if (c < O) {
      float* pg = &acc[wave][c];
      float* pb = &acc[wave][O + c];
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
  float* out = partials + (static_cast<int64_t>(blockIdx.x) * n + blk) * 2 * O;
  for (int c = threadIdx.x; c < 2 * O; c += kBlock) out[c] = ((acc[0][c] + acc[1][c]) + acc[2][c]) + acc[3][c];
}

__global__ __launch_bounds__(kBlock) void ln_relu_bwd_kernel(const float* __restrict__ dy, int64_t lddy,
                                                            const float* __restrict__ y, int64_t ldy, LnReluArgs a, int64_t B,
                                                            int O, int n, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd, float* __restrict__ partials) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, blk = blockIdx.y;
  const float* __restrict__ h = a.h[blk];
  const float* __restrict__ gamma = a.gamma[blk];
  float* __restrict__ dh = a.dh[blk];
  const int64_t ldh = a.ldh[blk], lddh = a.lddh[blk], col0 = static_cast<int64_t>(blk) * O;
  const float inv_w = 1.0f / static_cast<float>(O);
  int64_t r0, r1;
  ln_relu_row_range(B, &r0, &r1);
  for (int64_t r = r0 + wave; r < r1; r += kBlock / kWave) {
    const float* hr = h + r * ldh;
    const float* yr = y + r * ldy + col0;
    const float* dr = dy + r * lddy + col0;
    const float mu = mean[blk * B + r], rs = rstd[blk * B + r];
    float s1 = 0.f, s2 = 0.f;
    for (int c = lane; c < O; c += kWave) {
      const float xh = (hr[c] - mu) * rs;
      const float g = (yr[c] > 0.f ? dr[c] : 0.f) * gamma[c];
      s1 += g;
      s2 += g * xh;
    }
    const float m1 = wave_sum(s1) * inv_w, m2 = wave_sum(s2) * inv_w;
    for (int c = lane; c < O; c += kWave) {
      const float xh = (hr[c] - mu) * rs;
      const float g = (yr[c] > 0.f ? dr[c] : 0.f) * gamma[c];
      dh[r * lddh + c] = rs * (g - m1 - xh * m2);
    }
  }
  // a thread per column over the workgroup's rows, in order
  float* out = partials + (static_cast<int64_t>(blockIdx.x) * n + blk) * 2 * O;
  for (int c = threadIdx.x; c < O; c += kBlock) {
    float dg = 0.f, db = 0.f;
    for (int64_t r = r0; r < r1; ++r) {
      const float d = y[r * ldy + col0 + c] > 0.f ? dy[r * lddy + col0 + c] : 0.f;
      dg += d * ((h[r * ldh + c] - mean[blk * B + r]) * rstd[blk * B + r]);
      db += d;
    }
    out[c] = dg;
    out[O + c] = db;
  }
}

inline bool mask_shape_ok(int64_t B, int32_t W, int32_t n) {
  return B >= 1 && W >= 1 && W <= kMaskMaxW && n >= 1 && n <= kMaskMaxN;
}

inline bool ln_relu_shape_ok(int64_t B, int32_t O, int32_t n) {
  return B >= 1 && O >= 1 && O <= kLnReluMaxO && n >= 1 && n <= kMaskMaxN && 2 * static_cast<int64_t>(n) * O < kThetaMaxP;
}

inline unsigned mask_grid(int64_t pieces) {
  const int64_t blocks = ceil_div(pieces, static_cast<int64_t>(kBlock));
  return static_cast<unsigned>(blocks < kMaskMaxGrid ? blocks : kMaskMaxGrid);
}

}  // namespace er

extern "C" {

int er_mask_mul_fwd(const float* x, int64_t ldx, const float* const* v_host, const int64_t* ldv_host, int32_t n, int64_t B,
                    int32_t W, float* const* out_host, const int64_t* ldout_host, er_stream_t stream) {
  ER_REQUIRE(er::mask_shape_ok(B, W, n), "er_mask_mul_fwd: B = %lld, W = %d, n = %d outside the envelope",
             static_cast<long long>(B), W, n);
  ER_REQUIRE(x && v_host && ldv_host && out_host && ldout_host, "er_mask_mul_fwd: bad arguments");
  er::MaskMulArgs a = {};
  bool vec = W % 4 == 0 && ldx % 4 == 0 && er::aligned16(x);
  ER_REQUIRE(ldx >= W, "er_mask_mul_fwd: ldx = %lld < W", static_cast<long long>(ldx));
  for (int i = 0; i < n; ++i) {
    ER_REQUIRE(v_host[i] && out_host[i] && ldv_host[i] >= W && ldout_host[i] >= W, "er_mask_mul_fwd: bad operand %d", i);
    a.v[i] = v_host[i];
    a.o[i] = out_host[i];
    a.ldv[i] = ldv_host[i];
    a.ldo[i] = ldout_host[i];
    vec = vec && er::aligned16(a.v[i]) && er::aligned16(a.o[i]) && a.ldv[i] % 4 == 0 && a.ldo[i] % 4 == 0;
  }
  const dim3 grid(er::mask_grid(B * (vec ? W / 4 : W))), block(er::kBlock);
  if (vec)
    hipLaunchKernelGGL(er::mask_mul_fwd_kernel<4>, grid, block, 0, er::as_stream(stream), x, ldx, a, n, B, W);
  else
    hipLaunchKernelGGL(er::mask_mul_fwd_kernel<1>, grid, block, 0, er::as_stream(stream), x, ldx, a, n, B, W);
  ER_LAUNCH_CHECK();
  return 0;
}

int er_mask_mul_bwd(const float* x, int64_t ldx, const float* const* v_host, const int64_t* ldv_host,
                    const float* const* dout_host, const int64_t* lddout_host, int32_t n, int64_t B, int32_t W,
                    float* const* dv_host, const int64_t* lddv_host, float* dx, int64_t lddx, er_stream_t stream) {
  ER_REQUIRE(er::mask_shape_ok(B, W, n), "er_mask_mul_bwd: B = %lld, W = %d, n = %d outside the envelope",
             static_cast<long long>(B), W, n);
  ER_REQUIRE(x && v_host && ldv_host && dout_host && lddout_host && dv_host && lddv_host, "er_mask_mul_bwd: bad arguments");
  ER_REQUIRE(ldx >= W && (dx == nullptr || lddx >= W), "er_mask_mul_bwd: a pitch below W");
  er::MaskMulArgs a = {};
  bool vec = W % 4 == 0 && ldx % 4 == 0 && er::aligned16(x) && (dx == nullptr || (lddx % 4 == 0 && er::aligned16(dx)));
  for (int i = 0; i < n; ++i) {
    ER_REQUIRE(v_host[i] && dout_host[i] && dv_host[i] && ldv_host[i] >= W && lddout_host[i] >= W && lddv_host[i] >= W,
               "er_mask_mul_bwd: bad operand %d", i);
    a.v[i] = v_host[i];
    a.d[i] = dout_host[i];
    a.o[i] = dv_host[i];
    a.ldv[i] = ldv_host[i];
    a.ldd[i] = lddout_host[i];
    a.ldo[i] = lddv_host[i];
    vec = vec && er::aligned16(a.v[i]) && er::aligned16(a.d[i]) && er::aligned16(a.o[i]) && a.ldv[i] % 4 == 0 &&
          a.ldd[i] % 4 == 0 && a.ldo[i] % 4 == 0;
  }
  const dim3 grid(er::mask_grid(B * (vec ? W / 4 : W))), block(er::kBlock);
  if (vec)
    hipLaunchKernelGGL(er::mask_mul_bwd_kernel<4>, grid, block, 0, er::as_stream(stream), x, ldx, a, n, B, W, dx, lddx);
  else
    hipLaunchKernelGGL(er::mask_mul_bwd_kernel<1>, grid, block, 0, er::as_stream(stream), x, ldx, a, n, B, W, dx, lddx);
  ER_LAUNCH_CHECK();
  return 0;
}

int32_t er_ln_relu_grid(int64_t B, int32_t O, int32_t n) {
  if (!er::ln_relu_shape_ok(B, O, n)) return 0;
  const int64_t g = er::ceil_div(B, static_cast<int64_t>(er::kBlock / er::kWave));
  return static_cast<int32_t>(g < er::kLnReluMaxGrid ? g : er::kLnReluMaxGrid);
}

int er_ln_relu_fwd(const float* const* h_host, const int64_t* ldh_host, const float* const* gamma_host,
                   const float* const* beta_host, int32_t n, int64_t B, int32_t O, float eps, float* y, int64_t ldy,
                   float* mean, float* rstd, er_stream_t stream) {
  ER_REQUIRE(er::ln_relu_shape_ok(B, O, n), "er_ln_relu_fwd: B = %lld, O = %d, n = %d outside the envelope",
             static_cast<long long>(B), O, n);
  ER_REQUIRE(h_host && ldh_host && gamma_host && beta_host && y && mean && rstd, "er_ln_relu_fwd: bad arguments");
  ER_REQUIRE(ldy >= static_cast<int64_t>(n) * O, "er_ln_relu_fwd: ldy = %lld < n * O", static_cast<long long>(ldy));
  er::LnReluArgs a = {};
  bool vec = O % 4 == 0 && O <= er::kLnReluRegO && ldy % 4 == 0 && er::aligned16(y);
  for (int i = 0; i < n; ++i) {
    ER_REQUIRE(h_host[i] && gamma_host[i] && beta_host[i] && ldh_host[i] >= O, "er_ln_relu_fwd: bad operand %d", i);
    a.h[i] = h_host[i];
    a.ldh[i] = ldh_host[i];
    a.gamma[i] = gamma_host[i];
    a.beta[i] = beta_host[i];
    vec = vec && er::aligned16(a.h[i]) && a.ldh[i] % 4 == 0 && er::aligned16(a.gamma[i]) && er::aligned16(a.beta[i]);
  }
  const int64_t g = er::ceil_div(B, static_cast<int64_t>(er::kBlock / er::kWave));
  const dim3 grid(static_cast<unsigned>(g < 8192 ? g : 8192), n), block(er::kBlock);
  const hipStream_t s = er::as_stream(stream);
#define ER_LNR_FWD(KERNEL) hipLaunchKernelGGL(KERNEL, grid, block, 0, s, a, B, O, eps, y, ldy, mean, rstd)
  if (!vec)
    ER_LNR_FWD(er::ln_relu_fwd_kernel);
  else if (O <= 256)
    ER_LNR_FWD(er::ln_relu_fwd_vec_kernel<1>);
  else if (O <= 512)
    ER_LNR_FWD(er::ln_relu_fwd_vec_kernel<2>);
  else
    ER_LNR_FWD(er::ln_relu_fwd_vec_kernel<4>);
#undef ER_LNR_FWD
  ER_LAUNCH_CHECK();
  return 0;
}

int er_ln_relu_bwd(const float* dy, int64_t lddy, const float* y, int64_t ldy, const float* const* h_host,
                   const int64_t* ldh_host, const float* const* gamma_host, const float* mean, const float* rstd, int32_t n,
                   int64_t B, int32_t O, float* const* dh_host, const int64_t* lddh_host, float* partials,
                   er_stream_t stream) {
  ER_REQUIRE(er::ln_relu_shape_ok(B, O, n), "er_ln_relu_bwd: B = %lld, O = %d, n = %d outside the envelope",
             static_cast<long long>(B), O, n);
  ER_REQUIRE(dy && y && h_host && ldh_host && gamma_host && mean && rstd && dh_host && lddh_host && partials,
             "er_ln_relu_bwd: bad arguments");
  ER_REQUIRE(ldy >= static_cast<int64_t>(n) * O && lddy >= static_cast<int64_t>(n) * O, "er_ln_relu_bwd: a pitch below n * O");
  er::LnReluArgs a = {};
  bool vec = O % 4 == 0 && O <= er::kLnReluRegO && ldy % 4 == 0 && lddy % 4 == 0 && er::aligned16(y) && er::aligned16(dy);
  for (int i = 0; i < n; ++i) {
    ER_REQUIRE(h_host[i] && gamma_host[i] && dh_host[i] && ldh_host[i] >= O && lddh_host[i] >= O,
               "er_ln_relu_bwd: bad operand %d", i);
    a.h[i] = h_host[i];
    a.ldh[i] = ldh_host[i];
    a.gamma[i] = gamma_host[i];
    a.dh[i] = dh_host[i];
    a.lddh[i] = lddh_host[i];
    vec = vec && er::aligned16(a.h[i]) && a.ldh[i] % 4 == 0 && er::aligned16(a.gamma[i]) && er::aligned16(a.dh[i]) &&
          a.lddh[i] % 4 == 0;
  }
  const dim3 grid(er_ln_relu_grid(B, O, n), n), block(er::kBlock);
  const hipStream_t s = er::as_stream(stream);
#define ER_LNR_BWD(KERNEL) hipLaunchKernelGGL(KERNEL, grid, block, 0, s, dy, lddy, y, ldy, a, B, O, n, mean, rstd, partials)
  if (!vec)
    ER_LNR_BWD(er::ln_relu_bwd_kernel);
  else if (O <= 256)
    ER_LNR_BWD(er::ln_relu_bwd_vec_kernel<1>);
  else if (O <= 512)
    ER_LNR_BWD(er::ln_relu_bwd_vec_kernel<2>);
  else
    ER_LNR_BWD(er::ln_relu_bwd_vec_kernel<4>);
#undef ER_LNR_BWD
  ER_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
