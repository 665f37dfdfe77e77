// K8g: MIND's capsule layer with dynamic routing (reference layers/capsule_layer.py:60-176) and its label-aware
// attention (reference model/mind.py:168-200).
//
// Capsule routing.  One workgroup (4 waves) works on ONE example at a time over a persistent grid (at most 1536
// workgroups backward, 6144 forward).  The example's X [S, D], its projection H = X Smat [S, E], the routing weights W
// [S, K] and the capsules c [K, E] live in LDS, every row at an odd pitch; Smat (D * E floats, 4 KB at the taobao shape)
// is read through the vector L1.  [B, S, E] never reaches HBM.  Examples per workgroup: one.  At the taobao shape (S 64,
// D 16, E 64, K 5) an example takes 24 KiB, so six workgroups share a CU's 160 KiB and the CU stays busy through the
// routing loop's barriers by switching between them; at the envelope's corner (S = D = E = 128) one example takes 142 KiB
// and nothing else would fit beside it anyway.  Staging several examples per workgroup would buy nothing the co-resident
// workgroups do not already give.
//
// The backward recomputes H and the pre-squash c from the saved last-iteration W (every earlier iteration sits behind
// stop_gradient) and keeps its share of dSmat in its own row of `partials`: every entry is read, added and written by
// the same thread for every example, and er_theta_grad_reduce sums the rows in a fixed order.  No atomics, so two runs
// and a graph replay give the same bits.  fp32 throughout.
#include "er_field_block.h"

namespace er {

constexpr int kCapsMaxS = 128;
constexpr int kCapsMaxD = 128;
constexpr int kCapsMaxE = 128;
constexpr int kCapsMaxK = 8;
constexpr int kCapsMaxIters = 8;
constexpr int kCapsMaxLds = 160 * 1024;
// persistent workgroups of the backward = rows of `partials`: 6 per CU on MI355X, what the taobao shape's LDS lets a CU
// hold; the forward keeps no per-workgroup state and takes up to four times as many, so the hardware balances them
constexpr int kCapsMaxGrid = 1536;

struct CapsGeom {
  int S, D, E, K, Dp, Ep;
};

__host__ __device__ inline CapsGeom caps_geom(int S, int D, int E, int K) {
  CapsGeom g;
  g.S = S;
  g.D = D;
  g.E = E;
  g.K = K;
  g.Dp = odd(D);
  g.Ep = odd(E);
  return g;
}

// LDS floats: X, H (the backward turns it into dH), W, c, dc (backward only) and the rows' inverse norms (forward only)
__host__ __device__ inline int caps_lds_floats(const CapsGeom& g) {
  return g.S * g.Dp + g.S * g.Ep + g.S * g.K + 2 * g.K * g.Ep + g.S;
}

inline bool caps_shape_ok(int S, int D, int E, int K) {
  return S >= 1 && S <= kCapsMaxS && D >= 1 && D <= kCapsMaxD && E >= 1 && E <= kCapsMaxE && K >= 1 && K <= kCapsMaxK &&
         D * E < 65536;
}

// max(1, min(K, int(log(float(len))))) by integer thresholds: no integer lies near a power of e, so they are exact
__host__ __device__ inline int caps_count(int len, int K, int const_caps) {
  if (const_caps) return K;
  const int n = len < 8 ? 1 : len < 21 ? 2 : len < 55 ? 3 : len < 149 ? 4 : len < 404 ? 5 : len < 1097 ? 6 : len < 2981 ? 7 : 8;
  return n < K ? n : K;
}

// X rows s < len (zero for s >= L: the reference's pad) and H = X Smat for the same rows
__device__ inline void caps_project(const CapsGeom& g, const float* __restrict__ hist_b, int L, int len,
                                    const float* __restrict__ Smat, float* X, float* H) {
  const int D = g.D, E = g.E;
  for (int idx = threadIdx.x; idx < len * D; idx += kFieldThreads) {
    const int s = idx / D, d = idx - s * D;
    X[s * g.Dp + d] = s < L ? hist_b[static_cast<int64_t>(s) * D + d] : 0.f;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < len * E; idx += kFieldThreads) {
    const int s = idx / E, e = idx - s * E;
    const float* x = X + s * g.Dp;
    float acc = 0.f;
    for (int d = 0; d < D; ++d) acc = fmaf(x[d], Smat[d * E + e], acc);
    H[s * g.Ep + e] = acc;
  }
  __syncthreads();
}

// c[h, :] = sum_{s < len} W[s, h] H[s, :] for h < ncaps, 0 for the other rows
__device__ inline void caps_gather(const CapsGeom& g, const float* W, const float* H, int len, int ncaps, float* C) {
  for (int idx = threadIdx.x; idx < g.K * g.E; idx += kFieldThreads) {
    const int h = idx / g.E, e = idx - h * g.E;
    float acc = 0.f;
    if (h < ncaps)
      for (int s = 0; s < len; ++s) acc = fmaf(W[s * g.K + h], H[s * g.Ep + e], acc);
    C[h * g.Ep + e] = acc;
  }
}

// sum of squares of row r of M (pitch), by the calling wave; valid in every lane
__device__ inline float caps_row_sumsq(const float* M, int pitch, int r, int n) {
  const int lane = threadIdx.x & (kWave - 1);
  float v = 0.f;
  for (int e = lane; e < n; e += kWave) {
    const float x = M[r * pitch + e];
    v = fmaf(x, x, v);
  }
  return wave_sum(v);
}

__global__ void __launch_bounds__(kFieldThreads) capsule_fwd_kernel(
    const float* __restrict__ hist, const int32_t* __restrict__ seq_len, const float* __restrict__ Smat,
    const float* __restrict__ logits0, int64_t logits_stride, int64_t B, int L, CapsGeom g, int num_iters, float scale,
    float squash_pow, float scale_ratio, int const_caps, float* __restrict__ high, int32_t* __restrict__ num_caps,
    float* __restrict__ Wout) {
  extern __shared__ float lds[];
  const int S = g.S, E = g.E, K = g.K;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  float* X = lds;
  float* H = X + S * g.Dp;
  float* W = H + S * g.Ep;
  float* C = W + S * K;
  float* hinv = C + 2 * K * g.Ep;
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    const int len = min(max(seq_len[b], 0), S);
    const int ncaps = caps_count(len, K, const_caps);
    caps_project(g, hist + b * static_cast<int64_t>(L) * g.D, L, len, Smat, X, H);
    if (scale > 0.f && num_iters > 1) {
      for (int s = wave; s < len; s += kFieldWaves) {
        const float n = caps_row_sumsq(H, g.Ep, s, E);
        if (lane == 0) hinv[s] = rsqrtf(fmaxf(n, 1e-12f));
      }
    }
    const float* l0 = logits0 + b * logits_stride;
    for (int idx = threadIdx.x; idx < len * K; idx += kFieldThreads) W[idx] = l0[idx];
    __syncthreads();
    for (int it = 0; it < num_iters; ++it) {
      // W = softmax over h < ncaps (a masked logit adds exactly 0) * the sequence mask (rows s >= len are never read)
      for (int s = threadIdx.x; s < len; s += kFieldThreads) {
        float* w = W + s * K;
        float m = w[0];
        for (int h = 1; h < ncaps; ++h) m = fmaxf(m, w[h]);
        float z = 0.f;
        for (int h = 0; h < ncaps; ++h) {
          const float e = expf(w[h] - m);
          w[h] = e;
          z += e;
        }
        for (int h = 0; h < K; ++h) w[h] = h < ncaps ? w[h] / z : 0.f;
      }
      __syncthreads();
      caps_gather(g, W, H, len, ncaps, C);
      __syncthreads();
      if (it + 1 == num_iters) break;
      for (int h = wave; h < ncaps; h += kFieldWaves) {  // tf.nn.l2_normalize
        const float r = rsqrtf(fmaxf(caps_row_sumsq(C, g.Ep, h, E), 1e-12f));
        for (int e = lane; e < E; e += kWave) C[h * g.Ep + e] *= r;
      }
      __syncthreads();
      for (int idx = threadIdx.x; idx < len * K; idx += kFieldThreads) {
        const int s = idx / K, h = idx - s * K;
        const float* hs = H + s * g.Ep;
        const float* ch = C + h * g.Ep;
        float acc = 0.f;
        if (scale > 0.f) {
          const float r = hinv[s];
          for (int e = 0; e < E; ++e) acc = fmaf(hs[e] * r, ch[e], acc);
          acc *= scale;
        } else {
          for (int e = 0; e < E; ++e) acc = fmaf(hs[e], ch[e], acc);
        }
        W[idx] = acc;
      }
      __syncthreads();
    }
    // squash; rows h >= ncaps are zero
    float* out = high + b * static_cast<int64_t>(K) * E;
    for (int h = wave; h < K; h += kFieldWaves) {
      float f = 0.f;
      if (h < ncaps) {
        const float n = fmaxf(caps_row_sumsq(C, g.Ep, h, E), 1e-8f);
        f = powf(n / (1.f + n), squash_pow) * scale_ratio / sqrtf(n);
      }
      for (int e = lane; e < E; e += kWave) out[h * E + e] = h < ncaps ? f * C[h * g.Ep + e] : 0.f;
    }
    float* wo = Wout + b * static_cast<int64_t>(S) * K;
    for (int idx = threadIdx.x; idx < S * K; idx += kFieldThreads) wo[idx] = idx < len * K ? W[idx] : 0.f;
    if (threadIdx.x == 0) num_caps[b] = ncaps;
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kFieldThreads) capsule_bwd_kernel(
    const float* __restrict__ hist, const int32_t* __restrict__ seq_len, const float* __restrict__ Smat,
    const float* __restrict__ Wsaved, const float* __restrict__ dhigh, int64_t B, int L, CapsGeom g, float squash_pow,
    float scale_ratio, int const_caps, float* __restrict__ dhist, int acc, float* __restrict__ partials) {
  extern __shared__ float lds[];
  const int S = g.S, D = g.D, E = g.E, K = g.K;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  float* X = lds;
  float* H = X + S * g.Dp;
  float* W = H + S * g.Ep;
  float* C = W + S * K;
  float* dC = C + K * g.Ep;
  float* part = partials + static_cast<int64_t>(blockIdx.x) * D * E;
  for (int i = threadIdx.x; i < D * E; i += kFieldThreads) part[i] = 0.f;
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    const int len = min(max(seq_len[b], 0), S);
    const int ncaps = caps_count(len, K, const_caps);
    const int rows = min(len, L);  // the rows that exist in hist and count: the others' X is zero
    const float* ws = Wsaved + b * static_cast<int64_t>(S) * K;
    for (int idx = threadIdx.x; idx < len * K; idx += kFieldThreads) W[idx] = ws[idx];
    caps_project(g, hist + b * static_cast<int64_t>(L) * D, L, len, Smat, X, H);
    caps_gather(g, W, H, len, ncaps, C);
    __syncthreads();
    // out = f(n) c, n = max(|c|^2, 1e-8), f = ratio n^(p - 1/2) (1 + n)^-p:
    // dc = f dout + [|c|^2 > 1e-8] 2 <dout, c> f ((p - 1/2) / n - p / (1 + n)) c; rows h >= ncaps get nothing
    const float* dout = dhigh + b * static_cast<int64_t>(K) * E;
    for (int h = wave; h < K; h += kFieldWaves) {
      float f = 0.f, q = 0.f;
      if (h < ncaps) {
        const float n0 = caps_row_sumsq(C, g.Ep, h, E);
        const float n = fmaxf(n0, 1e-8f);
        f = powf(n / (1.f + n), squash_pow) * scale_ratio / sqrtf(n);
        float dot = 0.f;
        for (int e = lane; e < E; e += kWave) dot = fmaf(dout[h * E + e], C[h * g.Ep + e], dot);
        dot = wave_sum(dot);
        if (n0 > 1e-8f) q = 2.f * dot * f * ((squash_pow - 0.5f) / n - squash_pow / (1.f + n));
      }
      for (int e = lane; e < E; e += kWave)
        dC[h * g.Ep + e] = h < ncaps ? fmaf(q, C[h * g.Ep + e], f * dout[h * E + e]) : 0.f;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < rows * E; idx += kFieldThreads) {  // dH = W dc  -> the H buffer
      const int s = idx / E, e = idx - s * E;
      float a = 0.f;
      for (int h = 0; h < ncaps; ++h) a = fmaf(W[s * K + h], dC[h * g.Ep + e], a);
      H[s * g.Ep + e] = a;
    }
    __syncthreads();
    float* dx = dhist + b * static_cast<int64_t>(L) * D;
    for (int idx = threadIdx.x; idx < L * D; idx += kFieldThreads) {  // dhist = dH Smat^T
      const int s = idx / D, d = idx - s * D;
      if (s < rows) {
        const float* dh = H + s * g.Ep;
        const float* w = Smat + d * E;
        float a = 0.f;
        for (int e = 0; e < E; ++e) a = fmaf(dh[e], w[e], a);
        dx[idx] = acc ? dx[idx] + a : a;
      } else if (!acc) {
        dx[idx] = 0.f;
      }
    }
    for (int idx = threadIdx.x; idx < D * E; idx += kFieldThreads) {  // dSmat += X^T dH
      const int d = idx / E, e = idx - d * E;
      float a = 0.f;
      for (int s = 0; s < rows; ++s) a = fmaf(X[s * g.Dp + d], H[s * g.Ep + e], a);
      part[idx] += a;
    }
    __syncthreads();
  }
}

// opt in to more than 64 KB of dynamic LDS once per kernel and size (no stream work: safe inside a capture).  The two
// flags below are per process, not per device, and unsynchronised: this rests on the library's scope, ONE device per
// process (the single-GPU engine; MatchModel refuses the embedding-parallel one) driven by one host thread.  A second
// device or a second launching thread would need the flags keyed by device and a lock.
static int caps_set_lds(const void* fn, int bytes, int* done) {
  if (bytes > kFieldLdsBudget && bytes > *done) {
    ER_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    *done = bytes;
  }
  return 0;
}
static int g_caps_fwd_lds = 0, g_caps_bwd_lds = 0;

// ---- the label-aware attention: one wave per example, the K <= 8 rows of E <= 128 floats in registers (two per lane)
constexpr int kAttMaxE = 128;
constexpr int kAttEpl = kAttMaxE / kWave;  // elements per lane

__global__ void __launch_bounds__(kFieldThreads) mind_attention_fwd_kernel(
    const float* __restrict__ interests, const float* __restrict__ pos_item, const int32_t* __restrict__ num_caps,
    int64_t B, int K, int E, float simi_pow, float* __restrict__ user_emb, float* __restrict__ user_interests,
    float* __restrict__ weights) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (int64_t b = static_cast<int64_t>(blockIdx.x) * kFieldWaves + wave; b < B;
       b += static_cast<int64_t>(gridDim.x) * kFieldWaves) {
    const int nc = min(max(num_caps[b], 0), K);
    float p[kAttEpl], v[kCapsMaxK][kAttEpl], sim[kCapsMaxK];
#pragma unroll
    for (int j = 0; j < kAttEpl; ++j) {
      const int e = lane + j * kWave;
      p[j] = e < E ? pos_item[b * E + e] : 0.f;
    }
    float m = -1e32f;
#pragma unroll
    for (int h = 0; h < kCapsMaxK; ++h) {
      float dot = 0.f;
#pragma unroll
      for (int j = 0; j < kAttEpl; ++j) {
        const int e = lane + j * kWave;
        v[h][j] = (h < K && e < E) ? interests[(b * K + h) * E + e] : 0.f;
        dot = fmaf(v[h][j], p[j], dot);
      }
      sim[h] = h < nc ? wave_sum(dot) * simi_pow : -1e32f;  // tf.minimum(simi, (mask * 2 - 1) * 1e32)
      m = fmaxf(m, sim[h]);
    }
    float z = 0.f;
#pragma unroll
    for (int h = 0; h < kCapsMaxK; ++h) {
      sim[h] = h < nc ? expf(sim[h] - m) : 0.f;
      z += sim[h];
    }
    int best = 0;
    float wbest = -1.f;
#pragma unroll
    for (int h = 0; h < kCapsMaxK; ++h) {
      sim[h] = (h < K && nc > 0) ? sim[h] / z : 0.f;
      if (h < K && sim[h] > wbest) {  // tf.argmax: the lowest index wins a tie
        wbest = sim[h];
        best = h;
      }
    }
    if (nc == 0) {  // every logit is -1e32: a uniform softmax over the K rows, all of them masked afterwards
#pragma unroll
      for (int h = 0; h < kCapsMaxK; ++h) sim[h] = h < K ? 1.f / static_cast<float>(K) : 0.f;
      best = 0;
    }
    if (simi_pow >= 100.f) {
#pragma unroll
      for (int h = 0; h < kCapsMaxK; ++h) sim[h] = h == best ? 1.f : 0.f;
    }
    float u[kAttEpl];
#pragma unroll
    for (int j = 0; j < kAttEpl; ++j) u[j] = 0.f;
#pragma unroll
    for (int h = 0; h < kCapsMaxK; ++h) {
      if (h >= K) continue;
#pragma unroll
      for (int j = 0; j < kAttEpl; ++j) {
        const int e = lane + j * kWave;
        const float x = h < nc ? v[h][j] : 0.f;
        u[j] = fmaf(sim[h], x, u[j]);
        if (e < E) user_interests[(b * K + h) * E + e] = x;
      }
      if (lane == 0) weights[b * K + h] = sim[h];
    }
#pragma unroll
    for (int j = 0; j < kAttEpl; ++j) {
      const int e = lane + j * kWave;
      if (e < E) user_emb[b * E + e] = u[j];
    }
  }
}

// d_emb [B, E], d_ui [B, K, E] or null (nothing read the masked interests); w: the forward's weights
__global__ void __launch_bounds__(kFieldThreads) mind_attention_bwd_kernel(
    const float* __restrict__ interests, const float* __restrict__ pos_item, const int32_t* __restrict__ num_caps,
    const float* __restrict__ weights, const float* __restrict__ d_emb, const float* __restrict__ d_ui, int64_t B, int K,
    int E, float simi_pow, float* __restrict__ d_interests, float* __restrict__ d_pos) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (int64_t b = static_cast<int64_t>(blockIdx.x) * kFieldWaves + wave; b < B;
       b += static_cast<int64_t>(gridDim.x) * kFieldWaves) {
    const int nc = min(max(num_caps[b], 0), K);
    const bool soft = simi_pow < 100.f;  // through the one-hot of the argmax no gradient passes
    float p[kAttEpl], de[kAttEpl], dp[kAttEpl], v[kCapsMaxK][kAttEpl], w[kCapsMaxK], dw[kCapsMaxK];
#pragma unroll
    for (int j = 0; j < kAttEpl; ++j) {
      const int e = lane + j * kWave;
      p[j] = e < E ? pos_item[b * E + e] : 0.f;
      de[j] = e < E ? d_emb[b * E + e] : 0.f;
      dp[j] = 0.f;
    }
    float wdw = 0.f;
#pragma unroll
    for (int h = 0; h < kCapsMaxK; ++h) {
      float dot = 0.f;
#pragma unroll
      for (int j = 0; j < kAttEpl; ++j) {
        const int e = lane + j * kWave;
        v[h][j] = (h < K && e < E) ? interests[(b * K + h) * E + e] : 0.f;
        dot = fmaf(de[j], h < nc ? v[h][j] : 0.f, dot);
      }
      w[h] = h < K ? weights[b * K + h] : 0.f;
      dw[h] = wave_sum(dot);  // d(user_emb)/d(weight h) = the masked row
      wdw = fmaf(w[h], dw[h], wdw);
    }
#pragma unroll
    for (int h = 0; h < kCapsMaxK; ++h) {
      if (h >= K) continue;
      // softmax backward, then simi = <interests_h, pos> * simi_pow for the rows h < nc
      const float ds = (soft && h < nc) ? w[h] * (dw[h] - wdw) * simi_pow : 0.f;
#pragma unroll
      for (int j = 0; j < kAttEpl; ++j) {
        const int e = lane + j * kWave;
        float g = 0.f;
        if (h < nc) {
          g = w[h] * de[j];
          if (d_ui != nullptr && e < E) g += d_ui[(b * K + h) * E + e];
        }
        g = fmaf(ds, p[j], g);
        dp[j] = fmaf(ds, v[h][j], dp[j]);
        if (e < E) d_interests[(b * K + h) * E + e] = g;
      }
    }
#pragma unroll
    for (int j = 0; j < kAttEpl; ++j) {
      const int e = lane + j * kWave;
      if (e < E) d_pos[b * E + e] = dp[j];
    }
  }
}

inline int att_grid(int64_t B) {
  const int64_t n = ceil_div(B, kFieldWaves);
  return static_cast<int>(n < 4 * kFieldMaxGrid ? n : 4 * kFieldMaxGrid);
}

}  // namespace er

extern "C" {

int64_t er_capsule_lds_bytes(int32_t S, int32_t D, int32_t E, int32_t K) {
  if (!er::caps_shape_ok(S, D, E, K)) return 0;
  const int64_t bytes = 4 * static_cast<int64_t>(er::caps_lds_floats(er::caps_geom(S, D, E, K)));
  return bytes <= er::kCapsMaxLds ? bytes : 0;
}

int32_t er_capsule_grid(int64_t B) { return static_cast<int32_t>(B < er::kCapsMaxGrid ? (B < 1 ? 1 : B) : er::kCapsMaxGrid); }

int er_capsule_fwd(const float* hist, const int32_t* seq_len, const float* Smat, const float* logits0,
                   int64_t logits_stride, int64_t B, int32_t L, int32_t S, int32_t D, int32_t E, int32_t K,
                   int32_t num_iters, float routing_logits_scale, float squash_pow, float scale_ratio, int const_caps_num,
                   float* high_capsules, int32_t* num_caps, float* W, er_stream_t stream) {
  ER_REQUIRE(hist && seq_len && Smat && logits0 && high_capsules && num_caps && W && B > 0 && L > 0,
             "er_capsule_fwd: bad arguments");
  const int64_t bytes = er_capsule_lds_bytes(S, D, E, K);
  ER_REQUIRE(bytes > 0, "er_capsule_fwd: S = %d, D = %d, E = %d, K = %d outside the envelope", S, D, E, K);
  ER_REQUIRE(num_iters >= 1 && num_iters <= er::kCapsMaxIters, "er_capsule_fwd: num_iters = %d outside 1 .. %d", num_iters,
             er::kCapsMaxIters);
  ER_REQUIRE(logits_stride == 0 || logits_stride == static_cast<int64_t>(S) * K,
             "er_capsule_fwd: logits stride %lld, neither 0 nor S * K", static_cast<long long>(logits_stride));
  if (er::caps_set_lds(reinterpret_cast<const void*>(er::capsule_fwd_kernel), static_cast<int>(bytes), &er::g_caps_fwd_lds))
    return 1;
  const int64_t fwd_grid = B < 4 * er::kCapsMaxGrid ? B : 4 * er::kCapsMaxGrid;
  hipLaunchKernelGGL(er::capsule_fwd_kernel, dim3(static_cast<unsigned>(fwd_grid)), dim3(er::kFieldThreads), bytes,
                     er::as_stream(stream), hist, seq_len, Smat, logits0, logits_stride, B, L, er::caps_geom(S, D, E, K),
                     num_iters, routing_logits_scale, squash_pow, scale_ratio, const_caps_num, high_capsules, num_caps, W);
  ER_LAUNCH_CHECK();
  return 0;
}

int er_capsule_bwd(const float* hist, const int32_t* seq_len, const float* Smat, const float* W, const float* d_high,
                   int64_t B, int32_t L, int32_t S, int32_t D, int32_t E, int32_t K, float squash_pow, float scale_ratio,
                   int const_caps_num, float* dhist, int acc, float* partials, er_stream_t stream) {
  ER_REQUIRE(hist && seq_len && Smat && W && d_high && dhist && partials && B > 0 && L > 0,
             "er_capsule_bwd: bad arguments");
  const int64_t bytes = er_capsule_lds_bytes(S, D, E, K);
  ER_REQUIRE(bytes > 0, "er_capsule_bwd: S = %d, D = %d, E = %d, K = %d outside the envelope", S, D, E, K);
  if (er::caps_set_lds(reinterpret_cast<const void*>(er::capsule_bwd_kernel), static_cast<int>(bytes), &er::g_caps_bwd_lds))
    return 1;
  hipLaunchKernelGGL(er::capsule_bwd_kernel, dim3(er_capsule_grid(B)), dim3(er::kFieldThreads), bytes,
                     er::as_stream(stream), hist, seq_len, Smat, W, d_high, B, L, er::caps_geom(S, D, E, K), squash_pow,
                     scale_ratio, const_caps_num, dhist, acc, partials);
  ER_LAUNCH_CHECK();
  return 0;
}

int er_mind_attention_fwd(const float* interests, const float* pos_item, const int32_t* num_caps, int64_t B, int32_t K,
                          int32_t E, float simi_pow, float* user_emb, float* user_interests, float* weights,
                          er_stream_t stream) {
  ER_REQUIRE(interests && pos_item && num_caps && user_emb && user_interests && weights && B > 0,
             "er_mind_attention_fwd: bad arguments");
  ER_REQUIRE(K >= 1 && K <= er::kCapsMaxK && E >= 1 && E <= er::kAttMaxE,
             "er_mind_attention_fwd: K = %d, E = %d outside 1 <= K <= %d, 1 <= E <= %d", K, E, er::kCapsMaxK, er::kAttMaxE);
  hipLaunchKernelGGL(er::mind_attention_fwd_kernel, dim3(er::att_grid(B)), dim3(er::kFieldThreads), 0,
                     er::as_stream(stream), interests, pos_item, num_caps, B, K, E, simi_pow, user_emb, user_interests,
                     weights);
  ER_LAUNCH_CHECK();
  return 0;
}

int er_mind_attention_bwd(const float* interests, const float* pos_item, const int32_t* num_caps, const float* weights,
                          const float* d_user_emb, const float* d_user_interests, int64_t B, int32_t K, int32_t E,
                          float simi_pow, float* d_interests, float* d_pos_item, er_stream_t stream) {
  ER_REQUIRE(interests && pos_item && num_caps && weights && d_user_emb && d_interests && d_pos_item && B > 0,
             "er_mind_attention_bwd: bad arguments");
  ER_REQUIRE(K >= 1 && K <= er::kCapsMaxK && E >= 1 && E <= er::kAttMaxE,
             "er_mind_attention_bwd: K = %d, E = %d outside 1 <= K <= %d, 1 <= E <= %d", K, E, er::kCapsMaxK, er::kAttMaxE);
  hipLaunchKernelGGL(er::mind_attention_bwd_kernel, dim3(er::att_grid(B)), dim3(er::kFieldThreads), 0,
                     er::as_stream(stream), interests, pos_item, num_caps, weights, d_user_emb, d_user_interests, B, K, E,
                     simi_pow, d_interests, d_pos_item);
  ER_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
