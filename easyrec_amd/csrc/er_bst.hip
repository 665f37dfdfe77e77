// K8b: the BST transformer block (reference model/multi_tower_bst.py:78-151, layers/layer_norm.py:28-37).
//
// One workgroup (4 waves) works on one example at a time over a persistent grid: the example's [T, E] sequence, one
// head's Q / K / V and its [T, T] score tile live in LDS, the ~11 KB of block weights (E = 32) are read through the
// vector L1.  The backward recomputes the forward of its example (nothing per example is saved: P alone would be
// 4 * B * H * T^2 bytes) and keeps its share of the parameter gradient in its own row of `partials` - every entry is
// read, added and written by the same thread for every example, and er_theta_grad_reduce sums the rows in a fixed order:
// no atomics, so two runs and a graph replay give the same bits.
//
// Both envelope limits (T, E <= 64) make a row of the sequence or of a score tile one lane per element of a wave:
// LayerNorm and softmax rows are wave reductions.  fp32 throughout.
#include "er_field_block.h"

namespace er {

constexpr int kBstMaxT = 64;
constexpr int kBstMaxE = 64;
constexpr float kBstMasked = -4294967296.f;  // -2^32 + 1 in fp32 (multi_tower_bst.py:91)
constexpr float kLnEps = 1e-6f;              // layers/layer_norm.py:16

// offsets into the packed parameter vector (easyrec_hip.h K8b)
struct BstGeom {
  int T, E, p, nh, QW, P;
  int wq, bq, wk, bk, wv, bv, wo, bo, wf, bf, g1, b1, g2, b2;
};

__host__ __device__ inline BstGeom bst_geom(int T, int E, int H) {
  BstGeom g;
  g.T = T;
  g.E = E;
  g.p = (E + H - 1) / H;  // ceil(E / H) (multi_tower_bst.py:102)
  g.nh = (E + g.p - 1) / g.p;
  const int last = E - (g.nh - 1) * g.p;
  g.QW = (g.nh - 1) * g.p * g.p + last * last;
  g.wq = 0;
  g.bq = g.wq + g.QW;
  g.wk = g.bq + E;
  g.bk = g.wk + g.QW;
  g.wv = g.bk + E;
  g.bv = g.wv + g.QW;
  g.wo = g.bv + E;
  g.bo = g.wo + E * E;
  g.wf = g.bo + E;
  g.bf = g.wf + E * E;
  g.g1 = g.bf + E;
  g.b1 = g.g1 + E;
  g.g2 = g.b1 + E;
  g.b2 = g.g2 + E;
  g.P = g.b2 + E;
  return g;
}

__host__ __device__ inline int bst_head_w(const BstGeom& g, int h) { return min(g.p, g.E - h * g.p); }

// LDS floats: the forward keeps X, O, Y + one head's Q, K, V and score tile; the backward X, two [T, E] buffers and
// the row statistics, plus a region U that holds (O + Q, K, V + S) while recomputing the attention, (O + Z2) around the
// LayerNorms and (Q, K, V, D + P, dP) in the attention backward
__host__ __device__ inline int bst_fwd_lds(const BstGeom& g) {
  return 3 * g.T * g.E + 3 * g.T * g.p + g.T * g.T;
}
__host__ __device__ inline int bst_u_floats(const BstGeom& g) {
  const int a = g.T * g.E + 3 * g.T * g.p + g.T * g.T, b = 2 * g.T * g.E, c = 4 * g.T * g.p + 2 * g.T * g.T;
  return max(a, max(b, c));
}
__host__ __device__ inline int bst_bwd_lds(const BstGeom& g) { return 3 * g.T * g.E + 4 * g.T + bst_u_floats(g); }

// dst[t, j] = bias[j] + sum_i src[t, s + i] * W[i, j] for one head (W: [w, w]); src rows have E floats
__device__ inline void bst_head_dense(const float* src, int E, int T, int s, int w, const float* W, const float* bias,
                                      float* dst) {
  for (int idx = threadIdx.x; idx < T * w; idx += kFieldThreads) {
    const int t = idx / w, j = idx - t * w;
    const float* x = src + t * E + s;
    float acc = 0.f;
    for (int i = 0; i < w; ++i) acc = fmaf(x[i], W[i * w + j], acc);
    dst[idx] = acc + bias[j];
  }
}

// the attention of one example for every head into O [T, E]; qkv / S are scratch (3 T p, T T floats)
__device__ void bst_attention(const BstGeom& g, const float* theta, const float* X, int nvalid, float* O, float* q,
                              float* k, float* v, float* S) {
  const int T = g.T, E = g.E;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (int h = 0; h < g.nh; ++h) {
    const int s = h * g.p, w = bst_head_w(g, h), wo = h * g.p * g.p;
    bst_head_dense(X, E, T, s, w, theta + g.wq + wo, theta + g.bq + s, q);
    bst_head_dense(X, E, T, s, w, theta + g.wk + wo, theta + g.bk + s, k);
    bst_head_dense(X, E, T, s, w, theta + g.wv + wo, theta + g.bv + s, v);
    __syncthreads();
    for (int idx = threadIdx.x; idx < T * T; idx += kFieldThreads) {
      const int t = idx / T, u = idx - t * T;
      float acc = 0.f;
      for (int c = 0; c < w; ++c) acc = fmaf(q[t * w + c], k[u * w + c], acc);
      S[idx] = acc;  // (no 1/sqrt(d): the reference's "# Scale" scales nothing, :95)
    }
    __syncthreads();
    // masked softmax over the keys (:84-96): column T-1 is never masked, so exp of a masked score is exactly 0
    for (int t = wave; t < T; t += kFieldWaves) {
      const bool ok = lane < T && (lane < nvalid || lane == T - 1);
      const float sc = ok ? S[t * T + lane] : kBstMasked;
      const float m = wave_max(sc);
      const float e = ok ? expf(sc - m) : 0.f;
      const float z = wave_sum(e);
      if (lane < T) S[t * T + lane] = e / z;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < T * w; idx += kFieldThreads) {
      const int t = idx / w, c = idx - t * w;
      float acc = 0.f;
      for (int u = 0; u < nvalid; ++u) acc = fmaf(S[t * T + u], v[u * w + c], acc);
      acc = fmaf(S[t * T + T - 1], v[(T - 1) * w + c], acc);
      O[t * E + s + c] = acc;
    }
    __syncthreads();
  }
}

// dst[t, j] = add[t, j] + (b[j] + sum_i src[t, i] * W[i, j])   (W: [E, E])
__device__ inline void bst_dense_add(const float* src, const float* W, const float* b, const float* add, int T, int E,
                                     float* dst) {
  for (int idx = threadIdx.x; idx < T * E; idx += kFieldThreads) {
    const int t = idx / E, j = idx - t * E;
    const float* x = src + t * E;
    float acc = 0.f;
    for (int i = 0; i < E; ++i) acc = fmaf(x[i], W[i * E + j], acc);
    dst[idx] = add[idx] + (acc + b[j]);
  }
}

// per-row LayerNorm statistics of Z (wave per row); with y != nullptr also y = (z - mean) * rstd * gamma + beta
__device__ inline void bst_layer_norm(const float* Z, int T, int E, const float* gamma, const float* beta, float* mu,
                                      float* rs, float* y) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const float inv = 1.f / static_cast<float>(E);
  for (int t = wave; t < T; t += kFieldWaves) {
    const float z = lane < E ? Z[t * E + lane] : 0.f;
    const float m = wave_sum(z) * inv;
    const float d = lane < E ? z - m : 0.f;
    const float var = wave_sum(d * d) * inv;
    const float r = 1.f / sqrtf(var + kLnEps);
    if (lane == 0) {
      mu[t] = m;
      rs[t] = r;
    }
    if (y != nullptr && lane < E) y[t * E + lane] = d * r * gamma[lane] + beta[lane];
  }
}

__global__ void __launch_bounds__(kFieldThreads) bst_fwd_kernel(const float* __restrict__ key,
                                                              const float* __restrict__ hist,
                                                              const int32_t* __restrict__ seq_len,
                                                              const float* __restrict__ theta, int64_t B, int L,
                                                              BstGeom g, float* __restrict__ out) {
  extern __shared__ float lds[];
  const int T = g.T, E = g.E;
  float* X = lds;
  float* O = X + T * E;
  float* Y = O + T * E;
  float* q = Y + T * E;
  float* k = q + T * g.p;
  float* v = k + T * g.p;
  float* S = v + T * g.p;
  __shared__ float stat[2 * kBstMaxT];
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    for (int idx = threadIdx.x; idx < T * E; idx += kFieldThreads) {
      const int t = idx / E, c = idx - t * E;
      X[idx] = t == T - 1 ? key[b * E + c] : (t < L ? hist[(b * L + t) * E + c] : 0.f);
    }
    const int nvalid = min(max(seq_len[b], 0), T - 1);
    __syncthreads();
    bst_attention(g, theta, X, nvalid, O, q, k, v, S);
    bst_dense_add(O, theta + g.wo, theta + g.bo, X, T, E, Y);  // X + multi_head_attention (:139-140)
    __syncthreads();
    bst_layer_norm(Y, T, E, theta + g.g1, theta + g.b1, stat, stat + kBstMaxT, Y);  // in place, row by row
    __syncthreads();
    bst_dense_add(Y, theta + g.wf, theta + g.bf, Y, T, E, O);  // Y1 + feed_forward_net (:141-143)
    __syncthreads();
    bst_layer_norm(O, T, E, theta + g.g2, theta + g.b2, stat, stat + kBstMaxT, out + b * static_cast<int64_t>(T) * E);
    __syncthreads();
  }
}

// part[i, j] += sum_t A[t, a0 + i] * D[t, j] for i < m, j < n (A rows of lda floats, D rows of n floats)
__device__ inline void bst_wgrad(const float* A, int lda, int a0, const float* D, int T, int m, int n, float* part) {
  for (int idx = threadIdx.x; idx < m * n; idx += kFieldThreads) {
    const int i = idx / n, j = idx - i * n;
    float acc = 0.f;
    for (int t = 0; t < T; ++t) acc = fmaf(A[t * lda + a0 + i], D[t * n + j], acc);
    part[idx] += acc;
  }
}
// part[j] += sum_t D[t, j]
__device__ inline void bst_bgrad(const float* D, int T, int n, float* part) {
  for (int j = threadIdx.x; j < n; j += kFieldThreads) {
    float acc = 0.f;
    for (int t = 0; t < T; ++t) acc += D[t * n + j];
    part[j] += acc;
  }
}

// LayerNorm backward in place: dZ overwrites Z (Z: the LN input; dy: the output gradient); gamma / beta gradients
// go to part_g / part_b
__device__ inline void bst_layer_norm_bwd(float* Z, const float* dy, int T, int E, const float* gamma, const float* mu,
                                          const float* rs, float* part_g, float* part_b) {
  for (int j = threadIdx.x; j < E; j += kFieldThreads) {
    float sg = 0.f, sb = 0.f;
    for (int t = 0; t < T; ++t) {
      const float d = dy[t * E + j];
      sg = fmaf(d, (Z[t * E + j] - mu[t]) * rs[t], sg);
      sb += d;
    }
    part_g[j] += sg;
    part_b[j] += sb;
  }
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const float inv = 1.f / static_cast<float>(E);
  for (int t = wave; t < T; t += kFieldWaves) {
    const float xh = lane < E ? (Z[t * E + lane] - mu[t]) * rs[t] : 0.f;
    const float dxh = lane < E ? dy[t * E + lane] * gamma[lane] : 0.f;
    const float m1 = wave_sum(dxh) * inv;
    const float m2 = wave_sum(dxh * xh) * inv;
    if (lane < E) Z[t * E + lane] = rs[t] * (dxh - m1 - xh * m2);
  }
}

__global__ void __launch_bounds__(kFieldThreads) bst_bwd_kernel(const float* __restrict__ key,
                                                              const float* __restrict__ hist,
                                                              const int32_t* __restrict__ seq_len,
                                                              const float* __restrict__ theta,
                                                              const float* __restrict__ dout, int64_t B, int L,
                                                              BstGeom g, float* __restrict__ dkey,
                                                              float* __restrict__ dhist, int acc_h,
                                                              float* __restrict__ partials) {
  extern __shared__ float lds[];
  const int T = g.T, E = g.E, p = g.p;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  float* X = lds;
  float* B2 = X + T * E;
  float* B3 = B2 + T * E;
  float* mu1 = B3 + T * E;
  float* rs1 = mu1 + T;
  float* mu2 = rs1 + T;
  float* rs2 = mu2 + T;
  float* U = rs2 + T;
  float* O = U;               // attention output (recompute), read again by the Wo gradient
  float* Z2 = U + T * E;      // LN2 input -> dZ2
  float* q = U + T * E;       // (recompute) Q, K, V of one head + its score tile, behind O
  float* k = q + T * p;
  float* v = k + T * p;
  float* S = v + T * p;
  float* bq = U;              // (attention backward) Q -> dQ, K, V -> dV, D = dK, P -> dS, dP
  float* bk = bq + T * p;
  float* bv = bk + T * p;
  float* bd = bv + T * p;
  float* P = bd + T * p;
  float* dP = P + T * T;
  float* part = partials + static_cast<int64_t>(blockIdx.x) * g.P;
  for (int i = threadIdx.x; i < g.P; i += kFieldThreads) part[i] = 0.f;
  __syncthreads();
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    // -- recompute the forward (the same code and order as bst_fwd_kernel: the same bits)
    for (int idx = threadIdx.x; idx < T * E; idx += kFieldThreads) {
      const int t = idx / E, c = idx - t * E;
      X[idx] = t == T - 1 ? key[b * E + c] : (t < L ? hist[(b * L + t) * E + c] : 0.f);
    }
    const int nvalid = min(max(seq_len[b], 0), T - 1);
    __syncthreads();
    bst_attention(g, theta, X, nvalid, O, q, k, v, S);
    bst_dense_add(O, theta + g.wo, theta + g.bo, X, T, E, B3);  // Z1
    __syncthreads();
    bst_layer_norm(B3, T, E, theta + g.g1, theta + g.b1, mu1, rs1, B2);  // Y1
    __syncthreads();
    bst_dense_add(B2, theta + g.wf, theta + g.bf, B2, T, E, Z2);
    __syncthreads();
    bst_layer_norm(Z2, T, E, theta + g.g2, theta + g.b2, mu2, rs2, nullptr);
    __syncthreads();
    // -- LN2, the feed-forward dense, LN1
    const float* dy = dout + b * static_cast<int64_t>(T) * E;
    bst_layer_norm_bwd(Z2, dy, T, E, theta + g.g2, mu2, rs2, part + g.g2, part + g.b2);  // Z2 <- dZ2
    __syncthreads();
    bst_wgrad(B2, E, 0, Z2, T, E, E, part + g.wf);
    bst_bgrad(Z2, T, E, part + g.bf);
    __syncthreads();
    for (int idx = threadIdx.x; idx < T * E; idx += kFieldThreads) {  // dY1 = dZ2 + dZ2 Wf^T  -> B2
      const int t = idx / E, i = idx - t * E;
      const float* d = Z2 + t * E;
      const float* w = theta + g.wf + i * E;
      float acc = 0.f;
      for (int j = 0; j < E; ++j) acc = fmaf(d[j], w[j], acc);
      B2[idx] = d[i] + acc;
    }
    __syncthreads();
    bst_layer_norm_bwd(B3, B2, T, E, theta + g.g1, mu1, rs1, part + g.g1, part + g.b1);  // B3 <- dZ1 (= dX so far)
    __syncthreads();
    // -- the output projection
    bst_wgrad(O, E, 0, B3, T, E, E, part + g.wo);
    bst_bgrad(B3, T, E, part + g.bo);
    for (int idx = threadIdx.x; idx < T * E; idx += kFieldThreads) {  // dO = dZ1 Wo^T  -> B2
      const int t = idx / E, i = idx - t * E;
      const float* d = B3 + t * E;
      const float* w = theta + g.wo + i * E;
      float acc = 0.f;
      for (int j = 0; j < E; ++j) acc = fmaf(d[j], w[j], acc);
      B2[idx] = acc;
    }
    __syncthreads();
    // -- attention, head by head
    for (int h = 0; h < g.nh; ++h) {
      const int s = h * p, w = bst_head_w(g, h), wo = h * p * p;
      const float* Wq = theta + g.wq + wo;
      const float* Wk = theta + g.wk + wo;
      const float* Wv = theta + g.wv + wo;
      bst_head_dense(X, E, T, s, w, Wq, theta + g.bq + s, bq);
      bst_head_dense(X, E, T, s, w, Wk, theta + g.bk + s, bk);
      bst_head_dense(X, E, T, s, w, Wv, theta + g.bv + s, bv);
      __syncthreads();
      for (int idx = threadIdx.x; idx < T * T; idx += kFieldThreads) {
        const int t = idx / T, u = idx - t * T;
        float acc = 0.f, dacc = 0.f;
        for (int c = 0; c < w; ++c) {
          acc = fmaf(bq[t * w + c], bk[u * w + c], acc);
          dacc = fmaf(B2[t * E + s + c], bv[u * w + c], dacc);  // dP = dO_h V_h^T
        }
        P[idx] = acc;
        dP[idx] = dacc;
      }
      __syncthreads();
      for (int t = wave; t < T; t += kFieldWaves) {  // softmax as in the forward, then dS = P * (dP - sum_u dP P)
        const bool ok = lane < T && (lane < nvalid || lane == T - 1);
        const float sc = ok ? P[t * T + lane] : kBstMasked;
        const float m = wave_max(sc);
        const float e = ok ? expf(sc - m) : 0.f;
        const float z = wave_sum(e);
        const float pr = e / z;
        const float dp = ok ? dP[t * T + lane] : 0.f;
        const float r = wave_sum(dp * pr);
        if (lane < T) {
          P[t * T + lane] = pr;
          dP[t * T + lane] = pr * (dp - r);
        }
      }
      __syncthreads();
      for (int idx = threadIdx.x; idx < T * w; idx += kFieldThreads) {
        const int u = idx / w, c = idx - u * w;
        float dv = 0.f, dk = 0.f;
        for (int t = 0; t < T; ++t) {
          dv = fmaf(P[t * T + u], B2[t * E + s + c], dv);  // dV = P^T dO_h
          dk = fmaf(dP[t * T + u], bq[t * w + c], dk);     // dK = dS^T Q
        }
        bv[idx] = dv;
        bd[idx] = dk;
      }
      __syncthreads();
      for (int idx = threadIdx.x; idx < T * w; idx += kFieldThreads) {  // dQ = dS K  -> the Q buffer
        const int t = idx / w, c = idx - t * w;
        float acc = 0.f;
        for (int u = 0; u < T; ++u) acc = fmaf(dP[t * T + u], bk[u * w + c], acc);
        bq[idx] = acc;
      }
      __syncthreads();
      bst_wgrad(X, E, s, bq, T, w, w, part + g.wq + wo);
      bst_wgrad(X, E, s, bd, T, w, w, part + g.wk + wo);
      bst_wgrad(X, E, s, bv, T, w, w, part + g.wv + wo);
      bst_bgrad(bq, T, w, part + g.bq + s);
      bst_bgrad(bd, T, w, part + g.bk + s);
      bst_bgrad(bv, T, w, part + g.bv + s);
      for (int idx = threadIdx.x; idx < T * w; idx += kFieldThreads) {  // dX_h += dQ Wq^T + dK Wk^T + dV Wv^T
        const int t = idx / w, i = idx - t * w;
        float acc = 0.f;
        for (int j = 0; j < w; ++j) {
          acc = fmaf(bq[t * w + j], Wq[i * w + j], acc);
          acc = fmaf(bd[t * w + j], Wk[i * w + j], acc);
          acc = fmaf(bv[t * w + j], Wv[i * w + j], acc);
        }
        B3[t * E + s + i] += acc;
      }
      __syncthreads();
    }
    // -- dX: the history rows the reference's slice / pad kept, and the key row; the rest is dropped
    const int keep = min(T - 1, L);
    for (int idx = threadIdx.x; idx < L * E; idx += kFieldThreads) {
      const int t = idx / E;
      float* dst = dhist + b * static_cast<int64_t>(L) * E + idx;
      if (t < keep) {
        *dst = acc_h ? *dst + B3[idx] : B3[idx];
      } else if (!acc_h) {
        *dst = 0.f;
      }
    }
    for (int c = threadIdx.x; c < E; c += kFieldThreads) dkey[b * E + c] = B3[(T - 1) * E + c];
    __syncthreads();
  }
}

bool bst_shape_ok(int T, int E, int H) { return T >= 2 && T <= kBstMaxT && E >= 1 && E <= kBstMaxE && H >= 1; }

// opt in to more than 64 KB of dynamic LDS once per kernel and size (no stream work: safe inside a capture)
int bst_set_lds(const void* fn, int bytes, int* done) {
  if (bytes > kFieldLdsBudget && bytes > *done) {
    ER_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    *done = bytes;
  }
  return 0;
}
static int g_fwd_lds = 0, g_bwd_lds = 0;

}  // namespace er

extern "C" {

int64_t er_bst_param_count(int32_t E, int32_t H) {
  if (E < 1 || H < 1) return 0;
  return er::bst_geom(2, E, H).P;
}

int64_t er_bst_lds_bytes(int32_t T, int32_t E, int32_t H) {
  if (T < 1 || E < 1 || H < 1) return 0;
  const er::BstGeom g = er::bst_geom(T, E, H);
  return 4 * static_cast<int64_t>(max(er::bst_bwd_lds(g), er::bst_fwd_lds(g)));
}

int32_t er_bst_grid(int64_t B) { return er::persistent_grid(B, 1); }

int er_bst_fwd(const float* key, const float* hist, const int32_t* seq_len, const float* theta, int64_t B, int32_t L,
               int32_t T, int32_t E, int32_t H, float* out, er_stream_t stream) {
  ER_REQUIRE(key && hist && seq_len && theta && out && B > 0 && L > 0, "er_bst_fwd: bad arguments");
  ER_REQUIRE(er::bst_shape_ok(T, E, H), "er_bst_fwd: T = %d, E = %d, H = %d outside 2 <= T <= %d, 1 <= E <= %d", T, E,
             H, er::kBstMaxT, er::kBstMaxE);
  const er::BstGeom g = er::bst_geom(T, E, H);
  const int bytes = 4 * er::bst_fwd_lds(g);
  if (er::bst_set_lds(reinterpret_cast<const void*>(er::bst_fwd_kernel), bytes, &er::g_fwd_lds)) return 1;
  hipLaunchKernelGGL(er::bst_fwd_kernel, dim3(er_bst_grid(B)), dim3(er::kFieldThreads), bytes, er::as_stream(stream), key,
                     hist, seq_len, theta, B, L, g, out);
  ER_LAUNCH_CHECK();
  return 0;
}

int er_bst_bwd(const float* key, const float* hist, const int32_t* seq_len, const float* theta, const float* dout,
               int64_t B, int32_t L, int32_t T, int32_t E, int32_t H, float* dkey, float* dhist, int acc_h,
               float* partials, er_stream_t stream) {
  ER_REQUIRE(key && hist && seq_len && theta && dout && dkey && dhist && partials && B > 0 && L > 0,
             "er_bst_bwd: bad arguments");
  ER_REQUIRE(er::bst_shape_ok(T, E, H), "er_bst_bwd: T = %d, E = %d, H = %d outside 2 <= T <= %d, 1 <= E <= %d", T, E,
             H, er::kBstMaxT, er::kBstMaxE);
  const er::BstGeom g = er::bst_geom(T, E, H);
  const int bytes = 4 * er::bst_bwd_lds(g);
  if (er::bst_set_lds(reinterpret_cast<const void*>(er::bst_bwd_kernel), bytes, &er::g_bwd_lds)) return 1;
  hipLaunchKernelGGL(er::bst_bwd_kernel, dim3(er_bst_grid(B)), dim3(er::kFieldThreads), bytes, er::as_stream(stream), key,
                     hist, seq_len, theta, dout, B, L, g, dkey, dhist, acc_h, partials);
  ER_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
