// K8c: AutoInt's multi-head self-attention core (reference layers/multihead_attention.py:50-161 with use_res,
// model/autoint.py:54-75).
//
// The four projections Q | K | V | R = X [Wq | Wk | Wv | Wr] are one fp32 MFMA contraction (er_gemm_f32) into a
// [B * F, 4d] buffer G; these launches do what lies between that contraction and the next: per example and head
// S = Q_h K_h^T * sqrt(ds) (the reference divides by ds ** -0.5), P = softmax(S) over all F fields (no mask),
// O_h = P V_h, and Y = relu(O + R).  The backward recomputes S and P from G (nothing but Y is stored) and writes
// dQ | dK | dV | dR into one [B * F, 4d] buffer, so that the weight gradients are contractions too: no atomics, and
// every sum runs in a fixed order (two runs and a graph replay give the same bits).
//
// Layout: one workgroup (256 threads) stages `epb` examples in LDS - Q | K | V rows at an odd pitch (a column walk
// over rows is conflict-free for ds_read_b32 / ds_write_b32), then each phase is one flat loop over (example, ...)
// items separated by workgroup barriers.  epb = min(8, 64 KiB / the backward's LDS per example); the envelope is
// where one example fits: 4 * (F * odd(3d) + F * odd(d) + 2 * H * F^2) <= 65536 bytes (er_autoint_lds_bytes).
#include "er_field_block.h"

namespace er {

struct AiGeom {
  int F, H, ds, d;
  int ldq;      // LDS pitch of a Q | K | V row (odd)
  int lda;      // LDS pitch of a dA row (odd)
  float scale;  // sqrt(ds)
};

inline AiGeom ai_geom(int F, int H, int ds) {
  AiGeom g;
  g.F = F;
  g.H = H;
  g.ds = ds;
  g.d = H * ds;
  g.ldq = odd(3 * g.d);
  g.lda = odd(g.d);
  g.scale = sqrtf(static_cast<float>(ds));
  return g;
}

__host__ __device__ inline int ai_fwd_floats(const AiGeom& g) { return g.F * g.ldq + g.H * g.F * g.F; }
__host__ __device__ inline int ai_bwd_floats(const AiGeom& g) { return g.F * g.ldq + g.F * g.lda + 2 * g.H * g.F * g.F; }

// Q | K | V of the workgroup's examples -> LDS (example e at lds + e * per, row i at + i * ldq)
__device__ inline void ai_stage_qkv(const float* __restrict__ Gb, int ne, const AiGeom& g, int per, float* lds) {
  const int d3 = 3 * g.d, d4 = 4 * g.d;
  const int n = ne * g.F * d3;
  for (int t = threadIdx.x; t < n; t += kFieldThreads) {
    const int c = t % d3, r = t / d3;  // r = e * F + i
    const int e = r / g.F, i = r - e * g.F;
    lds[e * per + i * g.ldq + c] = Gb[static_cast<int64_t>(r) * d4 + c];
  }
}

// S[e, h, i, j] = sqrt(ds) * Q_h[i] . K_h[j] -> sbuf (at lds + e * per + soff), then each row's softmax in place
__device__ inline void ai_softmax_scores(int ne, const AiGeom& g, int per, int soff, float* lds) {
  const int F = g.F, H = g.H, ds = g.ds, FF = F * F;
  const int n = ne * H * FF;
  for (int t = threadIdx.x; t < n; t += kFieldThreads) {
    const int j = t % F;
    int q = t / F;
    const int i = q % F;
    q /= F;
    const int h = q % H, e = q / H;
    const float* X = lds + e * per;
    const float* qi = X + i * g.ldq + h * ds;
    const float* kj = X + j * g.ldq + g.d + h * ds;
    float s = 0.f;
    for (int c = 0; c < ds; ++c) s += qi[c] * kj[c];
    lds[e * per + soff + (h * F + i) * F + j] = s * g.scale;
  }
  __syncthreads();
  const int rows = ne * H * F;
  for (int t = threadIdx.x; t < rows; t += kFieldThreads) {
    const int e = t / (H * F), hi = t - e * (H * F);
    float* p = lds + e * per + soff + hi * F;
    float m = p[0];
    for (int j = 1; j < F; ++j) m = fmaxf(m, p[j]);
    float sum = 0.f;
    for (int j = 0; j < F; ++j) {
      const float x = expf(p[j] - m);
      p[j] = x;
      sum += x;
    }
    for (int j = 0; j < F; ++j) p[j] = p[j] / sum;
  }
  __syncthreads();
}

__global__ __launch_bounds__(kFieldThreads) void autoint_attn_fwd_kernel(const float* __restrict__ G, int64_t B, AiGeom g,
                                                                       int epb, float* __restrict__ Y) {
  extern __shared__ float lds[];
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * epb;
  const int ne = static_cast<int>(min(static_cast<int64_t>(epb), B - b0));
  const int F = g.F, d = g.d, d4 = 4 * d;
  const int per = ai_fwd_floats(g), soff = F * g.ldq;
  const float* Gb = G + b0 * F * d4;
  ai_stage_qkv(Gb, ne, g, per, lds);
  __syncthreads();
  ai_softmax_scores(ne, g, per, soff, lds);
  // O = P V_h, Y = relu(O + R)
  const int n = ne * F * d;
  for (int t = threadIdx.x; t < n; t += kFieldThreads) {
    const int c = t % d, r = t / d;
    const int e = r / F, i = r - e * F, h = c / g.ds;
    const float* X = lds + e * per;
    const float* p = X + soff + (h * F + i) * F;
    const float* v = X + 2 * d + c;
    float o = 0.f;
    for (int j = 0; j < F; ++j) o += p[j] * v[j * g.ldq];
    o += Gb[static_cast<int64_t>(r) * d4 + 3 * d + c];
    Y[(b0 * F + r) * d + c] = o > 0.f ? o : 0.f;
  }
}

__global__ __launch_bounds__(kFieldThreads) void autoint_attn_bwd_kernel(const float* __restrict__ G,
                                                                       const float* __restrict__ Y,
                                                                       const float* __restrict__ dY, int64_t B,
                                                                       AiGeom g, int epb, float* __restrict__ dG) {
  extern __shared__ float lds[];
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * epb;
  const int ne = static_cast<int>(min(static_cast<int64_t>(epb), B - b0));
  const int F = g.F, H = g.H, ds = g.ds, d = g.d, d4 = 4 * d, FF = F * F;
  const int per = ai_bwd_floats(g);
  const int aoff = F * g.ldq;           // dA [F, lda]
  const int poff = aoff + F * g.lda;    // P [H, F, F]
  const int soff = poff + H * FF;       // dP, then dS [H, F, F]
  const float* Gb = G + b0 * F * d4;
  float* dGb = dG + b0 * F * d4;
  ai_stage_qkv(Gb, ne, g, per, lds);
  // dA = dY * [Y > 0] -> LDS, and it is dR
  const int nrd = ne * F * d;
  for (int t = threadIdx.x; t < nrd; t += kFieldThreads) {
    const int c = t % d, r = t / d;
    const int e = r / F, i = r - e * F;
    const int64_t o = (b0 * F + r) * d + c;
    const float a = Y[o] > 0.f ? dY[o] : 0.f;
    lds[e * per + aoff + i * g.lda + c] = a;
    dGb[static_cast<int64_t>(r) * d4 + 3 * d + c] = a;
  }
  __syncthreads();
  ai_softmax_scores(ne, g, per, poff, lds);
  // dP[h, i, j] = dA_h[i] . V_h[j]
  const int nsc = ne * H * FF;
  for (int t = threadIdx.x; t < nsc; t += kFieldThreads) {
    const int j = t % F;
    int q = t / F;
    const int i = q % F;
    q /= F;
    const int h = q % H, e = q / H;
    const float* X = lds + e * per;
    const float* ai = X + aoff + i * g.lda + h * ds;
    const float* vj = X + j * g.ldq + 2 * d + h * ds;
    float s = 0.f;
    for (int c = 0; c < ds; ++c) s += ai[c] * vj[c];
    lds[e * per + soff + (h * F + i) * F + j] = s;
  }
  // dV_h[j] = sum_i P[h, i, j] dA_h[i]
  for (int t = threadIdx.x; t < nrd; t += kFieldThreads) {
    const int c = t % d, r = t / d;
    const int e = r / F, j = r - e * F, h = c / ds;
    const float* X = lds + e * per;
    const float* p = X + poff + h * FF + j;
    const float* a = X + aoff + c;
    float s = 0.f;
    for (int i = 0; i < F; ++i) s += p[i * F] * a[i * g.lda];
    dGb[static_cast<int64_t>(r) * d4 + 2 * d + c] = s;
  }
  __syncthreads();
  // dS = P * (dP - rowsum(dP * P))
  const int rows = ne * H * F;
  for (int t = threadIdx.x; t < rows; t += kFieldThreads) {
    const int e = t / (H * F), hi = t - e * (H * F);
    const float* p = lds + e * per + poff + hi * F;
    float* s = lds + e * per + soff + hi * F;
    float dot = 0.f;
    for (int j = 0; j < F; ++j) dot += s[j] * p[j];
    for (int j = 0; j < F; ++j) s[j] = p[j] * (s[j] - dot);
  }
  __syncthreads();
  // dQ_h[i] = sqrt(ds) sum_j dS[h, i, j] K_h[j];  dK_h[j] = sqrt(ds) sum_i dS[h, i, j] Q_h[i]
  for (int t = threadIdx.x; t < nrd; t += kFieldThreads) {
    const int c = t % d, r = t / d;
    const int e = r / F, i = r - e * F, h = c / ds;
    const float* X = lds + e * per;
    const float* s = X + soff + (h * F + i) * F;
    const float* k = X + d + c;
    float acc = 0.f;
    for (int j = 0; j < F; ++j) acc += s[j] * k[j * g.ldq];
    dGb[static_cast<int64_t>(r) * d4 + c] = acc * g.scale;
  }
  for (int t = threadIdx.x; t < nrd; t += kFieldThreads) {
    const int c = t % d, r = t / d;
    const int e = r / F, j = r - e * F, h = c / ds;
    const float* X = lds + e * per;
    const float* s = X + soff + h * FF + j;
    const float* q = X + c;
    float acc = 0.f;
    for (int i = 0; i < F; ++i) acc += s[i * F] * q[i * g.ldq];
    dGb[static_cast<int64_t>(r) * d4 + d + c] = acc * g.scale;
  }
}

struct AiPackSrc {
  const float* w[4];
};

// [Wq | Wk | Wv | Wr] ([din, d] each, row-major) -> w [din, 4d]
__global__ __launch_bounds__(kBlock) void autoint_pack_kernel(AiPackSrc src, int din, int d, float* __restrict__ w) {
  const int64_t n = static_cast<int64_t>(din) * 4 * d;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; t < n;
       t += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int c = static_cast<int>(t % (4 * d));
    const int64_t r = t / (4 * d);
    const int k = c / d;
    w[t] = src.w[k][r * d + (c - k * d)];
  }
}

bool ai_shape_ok(int F, int H, int ds) {
  if (F < 1 || H < 1 || ds < 1 || H * ds > 4096) return false;
  return 4 * ai_bwd_floats(ai_geom(F, H, ds)) <= kFieldLdsBudget;
}

}  // namespace er

extern "C" {

int64_t er_autoint_lds_bytes(int32_t F, int32_t H, int32_t ds) {
  if (F < 1 || H < 1 || ds < 1) return 0;
  return 4 * static_cast<int64_t>(er::ai_bwd_floats(er::ai_geom(F, H, ds)));
}

int32_t er_autoint_epb(int32_t F, int32_t H, int32_t ds, int bwd) {
  if (!er::ai_shape_ok(F, H, ds)) return 0;
  const er::AiGeom g = er::ai_geom(F, H, ds);
  return er::epb(0, bwd ? er::ai_bwd_floats(g) : er::ai_fwd_floats(g));
}

int er_autoint_attn_fwd(const float* qkvr, int64_t B, int32_t F, int32_t H, int32_t ds, float* y, er_stream_t stream) {
  ER_REQUIRE(qkvr && y && B > 0, "er_autoint_attn_fwd: bad arguments");
  ER_REQUIRE(er::ai_shape_ok(F, H, ds), "er_autoint_attn_fwd: F = %d, H = %d, ds = %d outside the envelope", F, H, ds);
  const er::AiGeom g = er::ai_geom(F, H, ds);
  const int epb = er::epb(0, er::ai_fwd_floats(g));
  const int64_t grid = (B + epb - 1) / epb;
  ER_REQUIRE(grid <= 0x7fffffff, "er_autoint_attn_fwd: B = %lld too large", static_cast<long long>(B));
  hipLaunchKernelGGL(er::autoint_attn_fwd_kernel, dim3(static_cast<unsigned>(grid)), dim3(er::kFieldThreads),
                     4 * epb * er::ai_fwd_floats(g), er::as_stream(stream), qkvr, B, g, epb, y);
  ER_LAUNCH_CHECK();
  return 0;
}

int er_autoint_attn_bwd(const float* qkvr, const float* y, const float* dy, int64_t B, int32_t F, int32_t H, int32_t ds,
                        float* dqkvr, er_stream_t stream) {
  ER_REQUIRE(qkvr && y && dy && dqkvr && B > 0, "er_autoint_attn_bwd: bad arguments");
  ER_REQUIRE(er::ai_shape_ok(F, H, ds), "er_autoint_attn_bwd: F = %d, H = %d, ds = %d outside the envelope", F, H, ds);
  const er::AiGeom g = er::ai_geom(F, H, ds);
  const int epb = er::epb(0, er::ai_bwd_floats(g));
  const int64_t grid = (B + epb - 1) / epb;
  ER_REQUIRE(grid <= 0x7fffffff, "er_autoint_attn_bwd: B = %lld too large", static_cast<long long>(B));
  hipLaunchKernelGGL(er::autoint_attn_bwd_kernel, dim3(static_cast<unsigned>(grid)), dim3(er::kFieldThreads),
                     4 * epb * er::ai_bwd_floats(g), er::as_stream(stream), qkvr, y, dy, B, g, epb, dqkvr);
  ER_LAUNCH_CHECK();
  return 0;
}

int er_autoint_pack(const float* wq, const float* wk, const float* wv, const float* wr, int32_t din, int32_t d,
                    float* w, er_stream_t stream) {
  ER_REQUIRE(wq && wk && wv && wr && w && din > 0 && d > 0, "er_autoint_pack: bad arguments");
  er::AiPackSrc src;
  src.w[0] = wq;
  src.w[1] = wk;
  src.w[2] = wv;
  src.w[3] = wr;
  const int64_t n = static_cast<int64_t>(din) * 4 * d;
  const int64_t blocks = er::ceil_div(n, static_cast<int64_t>(er::kBlock));
  const int grid = static_cast<int>(blocks < 1024 ? blocks : 1024);
  hipLaunchKernelGGL(er::autoint_pack_kernel, dim3(grid), dim3(er::kBlock), 0, er::as_stream(stream), src, din, d, w);
  ER_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
