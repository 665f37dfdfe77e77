// K8j: PPNet's gate multiply (reference layers/keras/ppnet.py:51-58, :185-187): out = x * 2 * sigmoid(z + bias), where x
// is an MLP layer's output, z the gate's `weight` Dense before its bias and bias that layer's bias variable.  One launch
// forward instead of BiasAdd, Sigmoid and two Mul; one launch backward (plus the shared fixed-order reduce for the bias
// gradient) instead of their gradients and the bias gradient's column sum.
//
// fp32, streaming: no MFMA, no atomics, nothing saved beyond the inputs (the backward recomputes the gate).  The operands
// stay where the Dense layers left them (row pitches of their own, column slices of wider tensors included).
//
// Both directions share one geometry.  The grid is er_gate_scale_grid = min(ceil(B / 8), 1024) workgroups of 256 threads;
// workgroup g owns the rows [g * per, min(B, (g + 1) * per)), per = ceil(B / grid).  A row is wc = W / V pieces of V floats
// (V = 4 on the 16-byte path, 1 on the 4-byte path).  With TC = min(wc, 256) and RL = 256 / TC, thread t is piece lane
// t % TC and row lane t / TC (threads t >= TC * RL idle); it walks the pieces tc, tc + TC, .. and, per piece, the rows
// r0 + rl, r0 + rl + RL, ..: consecutive threads read consecutive pieces of one row.
//
// Column sums of dz (the bias gradient's partials).  A thread sums its rows in the order it walks them, from 0.f.  With
// RL == 1 that is the workgroup's sum and goes straight to partials[g, .].  With RL > 1 (wc < 256: one piece per thread)
// the row lanes' sums meet in LDS and are combined in the order 0, 1, .., RL - 1.  er_theta_grad_reduce (row_groups = 8)
// then sums the workgroups.  Every order is fixed: two runs and a graph replay give the same bits.
//
// g = 2 / (1 + exp(-(z + bias))): exp overflows to +inf for z + bias below about -88.7, where the quotient is 0; it
// underflows to 0 above +88.7 (exactly 2 from about +17 on), so every finite input gives a finite gate in [0, 2].
#include <math.h>

#include "er_common.h"

namespace er {

constexpr int kGateMaxW = 4096;
constexpr int kGateRowsPerWg = 8;
constexpr int kGateMaxGrid = 1024;  // rows of `partials`

__device__ __forceinline__ float gate_of(float a) { return 2.0f / (1.0f + expf(-a)); }

template <int V>
struct GatePiece;
template <>
struct GatePiece<1> {
  typedef float T;
  static __device__ __forceinline__ float zero() { return 0.f; }
  static __device__ __forceinline__ float gate(float z, float b) { return gate_of(z + b); }
  static __device__ __forceinline__ float mul(float a, float b) { return a * b; }
  // dout * x * g * (1 - g / 2), left to right
  static __device__ __forceinline__ float dz(float d, float x, float g) { return d * x * g * (1.0f - 0.5f * g); }
  static __device__ __forceinline__ float add(float a, float b) { return a + b; }
  static __device__ __forceinline__ void put(float* p, float v) { p[0] = v; }
};
template <>
struct GatePiece<4> {
  typedef float4 T;
  static __device__ __forceinline__ float4 zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
  static __device__ __forceinline__ float4 gate(float4 z, float4 b) {
    return make_float4(gate_of(z.x + b.x), gate_of(z.y + b.y), gate_of(z.z + b.z), gate_of(z.w + b.w));
  }
  static __device__ __forceinline__ float4 mul(float4 a, float4 b) {
    return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
  }
  static __device__ __forceinline__ float4 dz(float4 d, float4 x, float4 g) {
    return make_float4(GatePiece<1>::dz(d.x, x.x, g.x), GatePiece<1>::dz(d.y, x.y, g.y), GatePiece<1>::dz(d.z, x.z, g.z),
                       GatePiece<1>::dz(d.w, x.w, g.w));
  }
  static __device__ __forceinline__ float4 add(float4 a, float4 b) {
    return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
  }
  static __device__ __forceinline__ void put(float* p, float4 v) {
    p[0] = v.x;
    p[1] = v.y;
    p[2] = v.z;
    p[3] = v.w;
  }
};

// this thread's place in the shared geometry; false: the thread is idle
struct GatePlace {
  int wc, TC, RL, tc, rl;
  int64_t r0, r1;
};
template <int V>
__device__ __forceinline__ bool gate_place(int64_t B, int W, GatePlace* p) {
  p->wc = W / V;
  p->TC = p->wc < kBlock ? p->wc : kBlock;
  p->RL = kBlock / p->TC;
  p->tc = static_cast<int>(threadIdx.x) % p->TC;
  p->rl = static_cast<int>(threadIdx.x) / p->TC;
  const int64_t per = (B + gridDim.x - 1) / gridDim.x;
  p->r0 = min(B, static_cast<int64_t>(blockIdx.x) * per);
  p->r1 = min(B, p->r0 + per);
  return p->rl < p->RL;
}

template <int V>
__global__ __launch_bounds__(kBlock) void gate_scale_fwd_kernel(const float* __restrict__ x, int64_t ldx,
                                                               const float* __restrict__ z, int64_t ldz,
                                                               const float* __restrict__ bias, int64_t B, int W,
                                                               float* __restrict__ out, int64_t ldout) {
  typedef typename GatePiece<V>::T T;
  GatePlace p;
  if (!gate_place<V>(B, W, &p)) return;
  for (int c = p.tc; c < p.wc; c += p.TC) {
    const int col = c * V;
    const T bv = bias != nullptr ? *reinterpret_cast<const T*>(bias + col) : GatePiece<V>::zero();
    for (int64_t r = p.r0 + p.rl; r < p.r1; r += p.RL) {
      const T xv = *reinterpret_cast<const T*>(x + r * ldx + col);
      const T zv = *reinterpret_cast<const T*>(z + r * ldz + col);
      *reinterpret_cast<T*>(out + r * ldout + col) = GatePiece<V>::mul(xv, GatePiece<V>::gate(zv, bv));
    }
  }
}

template <int V>
__global__ __launch_bounds__(kBlock) void gate_scale_bwd_kernel(const float* __restrict__ dout, int64_t lddout,
                                                               const float* __restrict__ x, int64_t ldx,
                                                               const float* __restrict__ z, int64_t ldz,
                                                               const float* __restrict__ bias, int64_t B, int W,
                                                               float* __restrict__ dx, int64_t lddx, float* __restrict__ dz,
                                                               int64_t lddz, float* __restrict__ partials) {
  typedef typename GatePiece<V>::T T;
  __shared__ float acc[kBlock * V];  // [RL][TC * V] when RL > 1
  GatePlace p;
  const bool active = gate_place<V>(B, W, &p);
  float* __restrict__ prow = partials != nullptr ? partials + static_cast<int64_t>(blockIdx.x) * W : nullptr;
  if (active) {
    for (int c = p.tc; c < p.wc; c += p.TC) {
      const int col = c * V;
      const T bv = bias != nullptr ? *reinterpret_cast<const T*>(bias + col) : GatePiece<V>::zero();
      T sum = GatePiece<V>::zero();
      for (int64_t r = p.r0 + p.rl; r < p.r1; r += p.RL) {
        const T dv = *reinterpret_cast<const T*>(dout + r * lddout + col);
        const T xv = *reinterpret_cast<const T*>(x + r * ldx + col);
        const T zv = *reinterpret_cast<const T*>(z + r * ldz + col);
        const T g = GatePiece<V>::gate(zv, bv);
        const T dzv = GatePiece<V>::dz(dv, xv, g);
        if (dx != nullptr) *reinterpret_cast<T*>(dx + r * lddx + col) = GatePiece<V>::mul(dv, g);
        *reinterpret_cast<T*>(dz + r * lddz + col) = dzv;
        sum = GatePiece<V>::add(sum, dzv);
      }
      if (prow != nullptr) {
        if (p.RL == 1)
          GatePiece<V>::put(prow + col, sum);
        else
          GatePiece<V>::put(acc + (p.rl * p.TC + p.tc) * V, sum);  // (wc < kBlock: this loop runs once)
      }
    }
  }
  if (prow == nullptr || p.RL == 1) return;  // (uniform over the workgroup)
  __syncthreads();
  for (int col = threadIdx.x; col < W; col += kBlock) {
    float s = acc[col];
    for (int rl = 1; rl < p.RL; ++rl) s += acc[rl * W + col];
    prow[col] = s;
  }
}

inline bool gate_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline bool gate_shape_ok(int64_t B, int32_t W) { return B >= 1 && W >= 1 && W <= kGateMaxW; }

}  // namespace er

extern "C" {

int32_t er_gate_scale_grid(int64_t B, int32_t W) {
  if (!er::gate_shape_ok(B, W)) return 0;
  const int64_t g = er::ceil_div(B, static_cast<int64_t>(er::kGateRowsPerWg));
  return static_cast<int32_t>(g < er::kGateMaxGrid ? g : er::kGateMaxGrid);
}

int er_gate_scale_fwd(const float* x, int64_t ldx, const float* z, int64_t ldz, const float* bias, int64_t B, int32_t W,
                      float* out, int64_t ldout, er_stream_t stream) {
  ER_REQUIRE(er::gate_shape_ok(B, W), "er_gate_scale_fwd: B = %lld, W = %d outside the envelope", static_cast<long long>(B),
             W);
  ER_REQUIRE(x && z && out, "er_gate_scale_fwd: bad arguments");
  ER_REQUIRE(ldx >= W && ldz >= W && ldout >= W, "er_gate_scale_fwd: a pitch below W");
  const bool vec = W % 4 == 0 && ldx % 4 == 0 && ldz % 4 == 0 && ldout % 4 == 0 && er::gate_aligned16(x) &&
                   er::gate_aligned16(z) && er::gate_aligned16(out) && er::gate_aligned16(bias);
  const dim3 grid(er_gate_scale_grid(B, W)), block(er::kBlock);
  if (vec)
    hipLaunchKernelGGL(er::gate_scale_fwd_kernel<4>, grid, block, 0, er::as_stream(stream), x, ldx, z, ldz, bias, B, W, out,
                       ldout);
  else
    hipLaunchKernelGGL(er::gate_scale_fwd_kernel<1>, grid, block, 0, er::as_stream(stream), x, ldx, z, ldz, bias, B, W, out,
                       ldout);
  ER_LAUNCH_CHECK();
  return 0;
}

int er_gate_scale_bwd(const float* dout, int64_t lddout, const float* x, int64_t ldx, const float* z, int64_t ldz,
                      const float* bias, int64_t B, int32_t W, float* dx, int64_t lddx, float* dz, int64_t lddz,
                      float* partials, er_stream_t stream) {
  ER_REQUIRE(er::gate_shape_ok(B, W), "er_gate_scale_bwd: B = %lld, W = %d outside the envelope", static_cast<long long>(B),
             W);
  ER_REQUIRE(dout && x && z && dz && (partials || !bias), "er_gate_scale_bwd: bad arguments");
  ER_REQUIRE(lddout >= W && ldx >= W && ldz >= W && lddz >= W && (dx == nullptr || lddx >= W),
             "er_gate_scale_bwd: a pitch below W");
  const bool vec = W % 4 == 0 && lddout % 4 == 0 && ldx % 4 == 0 && ldz % 4 == 0 && lddz % 4 == 0 &&
                   er::gate_aligned16(dout) && er::gate_aligned16(x) && er::gate_aligned16(z) && er::gate_aligned16(dz) &&
                   er::gate_aligned16(bias) && (dx == nullptr || (lddx % 4 == 0 && er::gate_aligned16(dx)));
  const dim3 grid(er_gate_scale_grid(B, W)), block(er::kBlock);
  if (vec)
    hipLaunchKernelGGL(er::gate_scale_bwd_kernel<4>, grid, block, 0, er::as_stream(stream), dout, lddout, x, ldx, z, ldz,
                       bias, B, W, dx, lddx, dz, lddz, partials);
  else
    hipLaunchKernelGGL(er::gate_scale_bwd_kernel<1>, grid, block, 0, er::as_stream(stream), dout, lddout, x, ldx, z, ldz,
                       bias, B, W, dx, lddx, dz, lddz, partials);
  ER_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
