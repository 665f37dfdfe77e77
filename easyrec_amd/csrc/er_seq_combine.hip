// Combining one sequence column over time (easyrec_hip.h K8h): TextCNN (Conv1D per filter size, activation, max over the
// window positions, concatenation) and attention pooling (a bias-free Dense(1), masked softmax, weighted sum), each one
// launch per direction.  Both read the column where the embedding engine left it: `x` points at the column's first
// float, consecutive positions lie `ld` floats apart and an example owns L_buf positions.  fp32; every sum is one
// thread's fmaf chain in a fixed order or a fixed butterfly, no atomics, so two runs and a graph replay give the same
// bits.  The contractions (k * D <= 512 by F <= 64 per example) are far below an MFMA tile's worth of work per launch
// round: FMA chains out of LDS.
#include "er_field_block.h"

namespace er {

constexpr int kTcMaxSizes = 4;
constexpr int kTcMaxP = 64, kTcMaxD = 64, kTcMaxF = 64, kTcMaxK = 8;

struct TcGeom {
  int P, D, n, SF, Pc;    // pad length, width, filter sizes, sum of the filters, packed parameter count
  int k[kTcMaxSizes], F[kTcMaxSizes];
  int koff[kTcMaxSizes], boff[kTcMaxSizes];  // kernel_i and bias_i in the packed theta
  int lk[kTcMaxSizes], lb[kTcMaxSizes];      // the same in the staged copy
  int fp[kTcMaxSizes];                       // the staged kernel's row pitch: odd(F_i) in LDS, F_i in memory
  int yoff[kTcMaxSizes], zoff[kTcMaxSizes];  // first output column; first float of z_i inside an example
  int xp, per, th_lds;                       // x row pitch; floats per example; staged theta floats (0: read in place)
};

inline bool tc_shape_ok(int P, int D, int n, const int32_t* k, const int32_t* F) {
  if (P < 1 || P > kTcMaxP || D < 1 || D > kTcMaxD || n < 1 || n > kTcMaxSizes || !k || !F) return false;
  int SF = 0;
  for (int i = 0; i < n; ++i) {
    if (k[i] < 1 || k[i] > kTcMaxK || k[i] > P || F[i] < 1) return false;
    SF += F[i];
  }
  return SF <= kTcMaxF;
}

// (the caller has checked the shape)
inline TcGeom tc_geom(int P, int D, int n, const int32_t* k, const int32_t* F) {
  TcGeom g;
  memset(&g, 0, sizeof(g));
  g.P = P;
  g.D = D;
  g.n = n;
  g.xp = odd(D);
  int o = 0, lo = 0, y = 0, z = 0;
  for (int i = 0; i < n; ++i) {
    g.k[i] = k[i];
    g.F[i] = F[i];
    g.koff[i] = o;
    g.boff[i] = o + k[i] * D * F[i];
    o = g.boff[i] + F[i];
    g.lk[i] = lo;
    g.lb[i] = lo + k[i] * D * odd(F[i]);
    lo = g.lb[i] + F[i];
    g.fp[i] = odd(F[i]);
    g.yoff[i] = y;
    y += F[i];
    g.zoff[i] = z;
    z += (P - k[i] + 1) * F[i];
  }
  g.SF = y;
  g.Pc = o;
  g.per = (P * g.xp + z + 3) & ~3;
  g.th_lds = (lo + 3) & ~3;
  if (g.th_lds + g.per > kFieldLdsBudget / 4) {
    // theta does not fit beside one example: the kernels read it where it lies
    g.th_lds = 0;
    for (int i = 0; i < n; ++i) {
      g.lk[i] = g.koff[i];
      g.lb[i] = g.boff[i];
      g.fp[i] = F[i];
    }
  }
  return g;
}

inline int tc_epb(const TcGeom& g) { return epb(g.th_lds, g.per); }

// examples per workgroup round of a launch over B examples: as few as fill the persistent grid (the phases are chains of
// LDS latencies, so more workgroups with less each finish sooner), at most what fits
inline int tc_epb_run(const TcGeom& g, int64_t B) {
  const int64_t want = ceil_div(B, kFieldMaxGrid);
  const int fit = tc_epb(g);
  return static_cast<int>(want < 1 ? 1 : (want < fit ? want : fit));
}

// theta into LDS, the kernels' rows at their odd pitch (kLds), or nothing
template <bool kLds>
__device__ __forceinline__ const float* tc_stage_theta(float* lds, const float* __restrict__ theta, const TcGeom& g) {
  if (!kLds) return theta;
  for (int i = 0; i < g.n; ++i) {
    const int Fi = g.F[i], nk = g.k[i] * g.D * Fi;
    for (int t = threadIdx.x; t < nk + Fi; t += kFieldThreads) {
      const float v = theta[g.koff[i] + t];
      if (t < nk) {
        const int q = t / Fi;
        lds[g.lk[i] + q * g.fp[i] + (t - q * Fi)] = v;
      } else {
        lds[g.lb[i] + (t - nk)] = v;
      }
    }
  }
  return lds;
}

// x of `ne` examples (padded with zeros from min(P, L_buf) on) and z_i = act(bias_i + window . kernel_i) into `ex`;
// ends with a barrier
__device__ __forceinline__ void tc_forward(const float* __restrict__ xb, int64_t ld, int L_buf, int ne, const TcGeom& g,
                                           const float* th, float* ex, int act) {
  const int P = g.P, D = g.D, xp = g.xp, per = g.per;
  const int Lx = P < L_buf ? P : L_buf;
  for (int t = threadIdx.x; t < ne * P * D; t += kFieldThreads) {
    const int e = t / (P * D), r = t - e * P * D, p = r / D, d = r - p * D;
    ex[e * per + p * xp + d] = p < Lx ? xb[(static_cast<int64_t>(e) * L_buf + p) * ld + d] : 0.f;
  }
  __syncthreads();
  const int zo = P * xp;
  for (int i = 0; i < g.n; ++i) {
    const int k = g.k[i], Fi = g.F[i], np = P - k + 1, fp = g.fp[i];
    for (int t = threadIdx.x; t < ne * np * Fi; t += kFieldThreads) {
      const int e = t / (np * Fi), r = t - e * np * Fi, p = r / Fi, f = r - p * Fi;
      const float* X = ex + e * per + p * xp;
      const float* K = th + g.lk[i] + f;
      float acc = th[g.lb[i] + f];
      // (unrolled so that the LDS loads of eight steps are in flight together; the chain's order is unchanged)
      for (int j = 0; j < k; ++j) {
#pragma unroll 8
        for (int d = 0; d < D; ++d) acc = fmaf(X[j * xp + d], K[(j * D + d) * fp], acc);
      }
      ex[e * per + zo + g.zoff[i] + r] = act && acc < 0.f ? 0.f : acc;
    }
  }
  __syncthreads();
}

template <bool kLds>
__global__ __launch_bounds__(kFieldThreads) void text_cnn_fwd_kernel(const float* __restrict__ x, int64_t ld, int L_buf,
                                                                   const float* __restrict__ theta, int64_t B, TcGeom g,
                                                                   int epb, int act, float* __restrict__ y,
                                                                   int64_t ldy, uint64_t* __restrict__ sel) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const float* th = tc_stage_theta<kLds>(lds, theta, g);
  float* ex = lds + g.th_lds;
  const int zo = g.P * g.xp, SF = g.SF;
  const int64_t nchunks = (B + epb - 1) / epb;
  for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int64_t b0 = chunk * epb;
    const int ne = static_cast<int>(min(static_cast<int64_t>(epb), B - b0));
    __syncthreads();
    tc_forward(x + b0 * L_buf * ld, ld, L_buf, ne, g, th, ex, act);
    for (int t = threadIdx.x; t < ne * SF; t += kFieldThreads) {
      const int e = t / SF, c = t - e * SF;
      int i = 0;
      while (i + 1 < g.n && c >= g.yoff[i + 1]) ++i;
      const int Fi = g.F[i], np = g.P - g.k[i] + 1;
      const float* z = ex + e * g.per + zo + g.zoff[i] + (c - g.yoff[i]);
      float m = z[0];
      for (int p = 1; p < np; ++p) m = fmaxf(m, z[p * Fi]);
      y[(b0 + e) * ldy + c] = m;
      if (sel != nullptr) {  // the positions the backward will share the gradient among
        uint64_t bits = 0;
        for (int p = 0; p < np; ++p) bits |= static_cast<uint64_t>(z[p * Fi] == m) << p;
        sel[(b0 + e) * SF + c] = bits;
      }
    }
  }
}

template <bool kLds>
__global__ __launch_bounds__(kFieldThreads) void text_cnn_bwd_kernel(const float* __restrict__ x, int64_t ld, int L_buf,
                                                                   const float* __restrict__ theta,
                                                                   const float* __restrict__ dy, int64_t lddy, int64_t B,
                                                                   TcGeom g, int epb, int act, float* __restrict__ dx,
                                                                   int64_t lddx, float* __restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const float* th = tc_stage_theta<kLds>(lds, theta, g);
  float* ex = lds + g.th_lds;
  const int P = g.P, D = g.D, xp = g.xp, per = g.per, zo = P * xp, SF = g.SF;
  const int Lx = P < L_buf ? P : L_buf;
  float* part = partials + static_cast<int64_t>(blockIdx.x) * g.Pc;
  const int64_t nchunks = (B + epb - 1) / epb;
  for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int64_t b0 = chunk * epb;
    const int ne = static_cast<int>(min(static_cast<int64_t>(epb), B - b0));
    const bool first = chunk == blockIdx.x;
    __syncthreads();
    tc_forward(x + b0 * L_buf * ld, ld, L_buf, ne, g, th, ex, act);
    // z_i[:, f] -> the gradient at the pre-activation: dy split evenly among the positions that equal the maximum
    // (TensorFlow's reduce_max), through the ReLU (nothing where the output is 0)
    for (int t = threadIdx.x; t < ne * SF; t += kFieldThreads) {
      const int e = t / SF, c = t - e * SF;
      int i = 0;
      while (i + 1 < g.n && c >= g.yoff[i + 1]) ++i;
      const int Fi = g.F[i], np = P - g.k[i] + 1;
      float* z = ex + e * per + zo + g.zoff[i] + (c - g.yoff[i]);
      float m = z[0];
      for (int p = 1; p < np; ++p) m = fmaxf(m, z[p * Fi]);
      int ties = 0;
      for (int p = 0; p < np; ++p) ties += z[p * Fi] == m;
      const float share = (act && !(m > 0.f)) ? 0.f : dy[(b0 + e) * lddy + c] / static_cast<float>(ties);
      for (int p = 0; p < np; ++p) z[p * Fi] = z[p * Fi] == m ? share : 0.f;
    }
    __syncthreads();
    // dx[t, d] = sum_i sum_j sum_f g_i[t - j, f] kernel_i[j, d, f]; zeros from P on
    float* dxb = dx + b0 * L_buf * lddx;
    for (int t = threadIdx.x; t < ne * L_buf * D; t += kFieldThreads) {
      const int e = t / (L_buf * D), r = t - e * L_buf * D, q = r / D, d = r - q * D;
      float acc = 0.f;
      if (q < Lx) {
        for (int i = 0; i < g.n; ++i) {
          const int k = g.k[i], Fi = g.F[i], np = P - k + 1, fp = g.fp[i];
          const float* G = ex + e * per + zo + g.zoff[i];
          for (int j = 0; j < k; ++j) {
            const int p = q - j;
            if (p < 0 || p >= np) continue;
            const float* gr = G + p * Fi;
            const float* kr = th + g.lk[i] + (j * D + d) * fp;
#pragma unroll 4
            for (int f = 0; f < Fi; ++f) acc = fmaf(gr[f], kr[f], acc);
          }
        }
      }
      dxb[(static_cast<int64_t>(e) * L_buf + q) * lddx + d] = acc;
    }
    // dkernel_i[j, d, f] = sum_e sum_p x[p + j, d] g_i[p, f]; dbias_i[f] = sum_e sum_p g_i[p, f]
    for (int t = threadIdx.x; t < g.Pc; t += kFieldThreads) {
      int i = 0;
      while (i + 1 < g.n && t >= g.koff[i + 1]) ++i;
      const int Fi = g.F[i], np = P - g.k[i] + 1, r = t - g.koff[i], nk = g.k[i] * D * Fi;
      float acc = 0.f;
      if (r < nk) {
        const int q = r / Fi, f = r - q * Fi, j = q / D, d = q - j * D;
        for (int e = 0; e < ne; ++e) {
          const float* X = ex + e * per + j * xp + d;
          const float* G = ex + e * per + zo + g.zoff[i] + f;
#pragma unroll 8
          for (int p = 0; p < np; ++p) acc = fmaf(X[p * xp], G[p * Fi], acc);
        }
      } else {
        const int f = r - nk;
        for (int e = 0; e < ne; ++e) {
          const float* G = ex + e * per + zo + g.zoff[i] + f;
          for (int p = 0; p < np; ++p) acc += G[p * Fi];
        }
      }
      part[t] = first ? acc : part[t] + acc;
    }
  }
}

// ---- attention pooling: one wave per example, four examples per workgroup round ----

constexpr int kApMaxL = 1024, kApMaxD = 128;
constexpr float kApMasked = -4294967295.f;  // -2^32 + 1 (fp32: -2^32)

__device__ __forceinline__ int ap_lane_pitch(int D) {
  int Dp = 1;
  while (Dp < D && Dp < kWave) Dp <<= 1;
  return Dp;
}

// the softmax over pw[0 .. L) of one wave (every lane has written its t = lane, lane + 64, ..); `mx` = the lane's maximum
__device__ __forceinline__ void ap_softmax(float* pw, int L, int lane, float mx) {
  mx = wave_max(mx);
  float s = 0.f;
  for (int t = lane; t < L; t += kWave) {
    const float e = expf(pw[t] - mx);
    pw[t] = e;
    s += e;
  }
  s = wave_sum(s);
  for (int t = lane; t < L; t += kWave) pw[t] = pw[t] / s;
}

__global__ __launch_bounds__(kFieldThreads) void seq_attn_pool_fwd_kernel(const float* __restrict__ x, int64_t ld,
                                                                        const int32_t* __restrict__ len,
                                                                        const float* __restrict__ w, int64_t B, int L,
                                                                        int D, float* __restrict__ y, int64_t ldy) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int L4 = (L + 3) & ~3;
  float* pw = lds + wave * L4;
  const int Dp = ap_lane_pitch(D), G = kWave / Dp, gi = lane / Dp, d0 = lane - gi * Dp;
  const int64_t nround = (B + kFieldWaves - 1) / kFieldWaves;
  for (int64_t r = blockIdx.x; r < nround; r += gridDim.x) {
    const int64_t b = r * kFieldWaves + wave;
    const bool live = b < B;  // (wave-uniform)
    const float* xb = x + (live ? b : 0) * L * ld;
    if (live) {
      const int n = len[b];
      float mx = kApMasked;
      for (int t = lane; t < L; t += kWave) {
        const float* xr = xb + static_cast<int64_t>(t) * ld;
        float acc = 0.f;
        for (int d = 0; d < D; ++d) acc = fmaf(xr[d], w[d], acc);
        acc = t < n ? acc : kApMasked;
        pw[t] = acc;
        mx = fmaxf(mx, acc);
      }
      ap_softmax(pw, L, lane, mx);
    }
    __syncthreads();
    if (live) {
      float a0 = 0.f, a1 = 0.f;
      for (int t = gi; t < L; t += G) {
        const float* xr = xb + static_cast<int64_t>(t) * ld;
        const float p = pw[t];
        if (d0 < D) a0 = fmaf(p, xr[d0], a0);
        if (d0 + kWave < D) a1 = fmaf(p, xr[d0 + kWave], a1);
      }
      for (int off = Dp; off < kWave; off <<= 1) a0 += __shfl_xor(a0, off, kWave);
      if (gi == 0 && d0 < D) y[b * ldy + d0] = a0;
      if (d0 + kWave < D) y[b * ldy + d0 + kWave] = a1;  // (D > 64: one group)
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kFieldThreads) void seq_attn_pool_bwd_kernel(const float* __restrict__ x, int64_t ld,
                                                                        const int32_t* __restrict__ len,
                                                                        const float* __restrict__ w,
                                                                        const float* __restrict__ dy, int64_t B, int L,
                                                                        int D, float* __restrict__ dx,
                                                                        int64_t lddx, float* __restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int L4 = (L + 3) & ~3;
  float* pw = lds + wave * 2 * L4;  // p
  float* sw = pw + L4;              // <dy, x_t>, then dlogit_t
  float* red = lds + kFieldWaves * 2 * L4;
  const int Dp = ap_lane_pitch(D), G = kWave / Dp, gi = lane / Dp, d0 = lane - gi * Dp;
  const bool has0 = d0 < D, has1 = d0 + kWave < D;
  const float w0 = has0 ? w[d0] : 0.f, w1 = has1 ? w[d0 + kWave] : 0.f;
  float dw0 = 0.f, dw1 = 0.f;
  const int64_t nround = (B + kFieldWaves - 1) / kFieldWaves;
  for (int64_t r = blockIdx.x; r < nround; r += gridDim.x) {
    const int64_t b = r * kFieldWaves + wave;
    const bool live = b < B;
    const float* xb = x + (live ? b : 0) * L * ld;
    const float* dyb = dy + (live ? b : 0) * D;
    if (live) {
      const int n = len[b];
      float mx = kApMasked;
      for (int t = lane; t < L; t += kWave) {
        const float* xr = xb + static_cast<int64_t>(t) * ld;
        float acc = 0.f, s = 0.f;
        for (int d = 0; d < D; ++d) {
          acc = fmaf(xr[d], w[d], acc);
          s = fmaf(xr[d], dyb[d], s);
        }
        acc = t < n ? acc : kApMasked;
        pw[t] = acc;
        sw[t] = s;
        mx = fmaxf(mx, acc);
      }
      ap_softmax(pw, L, lane, mx);
      float sb = 0.f;
      for (int t = lane; t < L; t += kWave) sb = fmaf(pw[t], sw[t], sb);
      sb = wave_sum(sb);
      // (a masked position's logit is the constant, so nothing flows to <x_t, w> there)
      for (int t = lane; t < L; t += kWave) sw[t] = t < n ? pw[t] * (sw[t] - sb) : 0.f;
    }
    __syncthreads();
    if (live) {
      float* dxb = dx + b * L * lddx;
      const float g0 = has0 ? dyb[d0] : 0.f, g1 = has1 ? dyb[d0 + kWave] : 0.f;
      for (int t = gi; t < L; t += G) {
        const float* xr = xb + static_cast<int64_t>(t) * ld;
        float* dr = dxb + static_cast<int64_t>(t) * lddx;
        const float p = pw[t], dl = sw[t];
        if (has0) {
          dr[d0] = fmaf(dl, w0, p * g0);
          dw0 = fmaf(dl, xr[d0], dw0);
        }
        if (has1) {
          dr[d0 + kWave] = fmaf(dl, w1, p * g1);
          dw1 = fmaf(dl, xr[d0 + kWave], dw1);
        }
      }
    }
    __syncthreads();
  }
  // dw: the lane groups of a wave by butterfly, the four waves in order
  for (int off = Dp; off < kWave; off <<= 1) dw0 += __shfl_xor(dw0, off, kWave);
  if (gi == 0 && has0) red[wave * kApMaxD + d0] = dw0;
  if (has1) red[wave * kApMaxD + d0 + kWave] = dw1;
  __syncthreads();
  for (int d = threadIdx.x; d < D; d += kFieldThreads)
    partials[static_cast<int64_t>(blockIdx.x) * D + d] =
        ((red[d] + red[kApMaxD + d]) + red[2 * kApMaxD + d]) + red[3 * kApMaxD + d];
}

inline bool ap_shape_ok(int L, int D) { return L >= 1 && L <= kApMaxL && D >= 1 && D <= kApMaxD; }

}  // namespace er

extern "C" {

int64_t er_text_cnn_param_count(int32_t D, int32_t n_sizes, const int32_t* sizes, const int32_t* filters) {
  if (D < 1 || n_sizes < 1 || n_sizes > er::kTcMaxSizes || !sizes || !filters) return 0;
  int64_t n = 0;
  for (int i = 0; i < n_sizes; ++i) n += static_cast<int64_t>(sizes[i]) * D * filters[i] + filters[i];
  return n;
}

int64_t er_text_cnn_lds_bytes(int32_t P, int32_t D, int32_t n_sizes, const int32_t* sizes, const int32_t* filters) {
  if (!er::tc_shape_ok(P, D, n_sizes, sizes, filters)) return 0;
  const er::TcGeom g = er::tc_geom(P, D, n_sizes, sizes, filters);
  return 4 * (static_cast<int64_t>(g.th_lds) + static_cast<int64_t>(er::tc_epb(g)) * g.per);
}

int32_t er_text_cnn_epb(int32_t P, int32_t D, int32_t n_sizes, const int32_t* sizes, const int32_t* filters) {
  if (!er::tc_shape_ok(P, D, n_sizes, sizes, filters)) return 0;
  return er::tc_epb(er::tc_geom(P, D, n_sizes, sizes, filters));
}

int32_t er_text_cnn_grid(int64_t B, int32_t P, int32_t D, int32_t n_sizes, const int32_t* sizes,
                         const int32_t* filters) {
  const int epb = er_text_cnn_epb(P, D, n_sizes, sizes, filters);
  if (epb <= 0 || B <= 0) return 0;
  return er::persistent_grid(B, er::tc_epb_run(er::tc_geom(P, D, n_sizes, sizes, filters), B));
}

int er_text_cnn_fwd(const float* x, int64_t ld, int32_t L_buf, const float* theta, int64_t B, int32_t P, int32_t D,
                    int32_t n_sizes, const int32_t* sizes, const int32_t* filters, int act, float* y, int64_t ldy,
                    uint64_t* sel, er_stream_t stream) {
  ER_REQUIRE(x && theta && y && B > 0 && L_buf >= 1, "er_text_cnn_fwd: bad arguments");
  ER_REQUIRE(er::tc_shape_ok(P, D, n_sizes, sizes, filters), "er_text_cnn_fwd: P = %d, D = %d, %d sizes outside the envelope",
             P, D, n_sizes);
  ER_REQUIRE(act == 0 || act == 1, "er_text_cnn_fwd: act = %d, not 0 (linear) or 1 (relu)", act);
  const er::TcGeom g = er::tc_geom(P, D, n_sizes, sizes, filters);
  ER_REQUIRE(ld >= D && ldy >= g.SF, "er_text_cnn_fwd: pitches %lld, %lld below the widths %d, %d",
             static_cast<long long>(ld), static_cast<long long>(ldy), D, g.SF);
  const int epb = er::tc_epb_run(g, B);
  const size_t lds = 4 * (static_cast<size_t>(g.th_lds) + static_cast<size_t>(epb) * g.per);
  const dim3 grid(er::persistent_grid(B, epb)), block(er::kFieldThreads);
  if (g.th_lds > 0)
    hipLaunchKernelGGL(er::text_cnn_fwd_kernel<true>, grid, block, lds, er::as_stream(stream), x, ld, L_buf, theta, B, g,
                       epb, act, y, ldy, sel);
  else
    hipLaunchKernelGGL(er::text_cnn_fwd_kernel<false>, grid, block, lds, er::as_stream(stream), x, ld, L_buf, theta, B, g,
                       epb, act, y, ldy, sel);
  ER_LAUNCH_CHECK();
  return 0;
}

int er_text_cnn_bwd(const float* x, int64_t ld, int32_t L_buf, const float* theta, const float* dy, int64_t lddy,
                    int64_t B, int32_t P, int32_t D, int32_t n_sizes, const int32_t* sizes, const int32_t* filters,
                    int act, float* dx, int64_t lddx, float* partials, er_stream_t stream) {
  ER_REQUIRE(x && theta && dy && dx && partials && B > 0 && L_buf >= 1, "er_text_cnn_bwd: bad arguments");
  ER_REQUIRE(er::tc_shape_ok(P, D, n_sizes, sizes, filters), "er_text_cnn_bwd: P = %d, D = %d, %d sizes outside the envelope",
             P, D, n_sizes);
  ER_REQUIRE(act == 0 || act == 1, "er_text_cnn_bwd: act = %d, not 0 (linear) or 1 (relu)", act);
  const er::TcGeom g = er::tc_geom(P, D, n_sizes, sizes, filters);
  ER_REQUIRE(ld >= D && lddx >= D && lddy >= g.SF, "er_text_cnn_bwd: pitches %lld, %lld, %lld below the widths %d, %d",
             static_cast<long long>(ld), static_cast<long long>(lddx), static_cast<long long>(lddy), D, g.SF);
  const int epb = er::tc_epb_run(g, B);
  const size_t lds = 4 * (static_cast<size_t>(g.th_lds) + static_cast<size_t>(epb) * g.per);
  const dim3 grid(er::persistent_grid(B, epb)), block(er::kFieldThreads);
  if (g.th_lds > 0)
    hipLaunchKernelGGL(er::text_cnn_bwd_kernel<true>, grid, block, lds, er::as_stream(stream), x, ld, L_buf, theta, dy,
                       lddy, B, g, epb, act, dx, lddx, partials);
  else
    hipLaunchKernelGGL(er::text_cnn_bwd_kernel<false>, grid, block, lds, er::as_stream(stream), x, ld, L_buf, theta, dy,
                       lddy, B, g, epb, act, dx, lddx, partials);
  ER_LAUNCH_CHECK();
  return 0;
}

int64_t er_seq_attn_pool_lds_bytes(int32_t L_buf, int32_t D, int bwd) {
  if (!er::ap_shape_ok(L_buf, D)) return 0;
  const int64_t L4 = (L_buf + 3) & ~3;
  return 4 * (bwd ? er::kFieldWaves * (2 * L4 + er::kApMaxD) : er::kFieldWaves * L4);
}

int32_t er_seq_attn_pool_epb(int32_t L_buf, int32_t D) { return er::ap_shape_ok(L_buf, D) ? er::kFieldWaves : 0; }

int32_t er_seq_attn_pool_grid(int64_t B, int32_t L_buf, int32_t D) {
  return er::ap_shape_ok(L_buf, D) && B > 0 ? er::persistent_grid(B, er::kFieldWaves) : 0;
}

int er_seq_attn_pool_fwd(const float* x, int64_t ld, const int32_t* len, const float* w, int64_t B, int32_t L_buf,
                         int32_t D, float* y, int64_t ldy, er_stream_t stream) {
  ER_REQUIRE(x && len && w && y && B > 0, "er_seq_attn_pool_fwd: bad arguments");
  ER_REQUIRE(er::ap_shape_ok(L_buf, D), "er_seq_attn_pool_fwd: L_buf = %d, D = %d outside the envelope", L_buf, D);
  ER_REQUIRE(ld >= D && ldy >= D, "er_seq_attn_pool_fwd: a pitch below the width %d", D);
  hipLaunchKernelGGL(er::seq_attn_pool_fwd_kernel, dim3(er_seq_attn_pool_grid(B, L_buf, D)), dim3(er::kFieldThreads),
                     static_cast<size_t>(er_seq_attn_pool_lds_bytes(L_buf, D, 0)), er::as_stream(stream), x, ld, len, w,
                     B, L_buf, D, y, ldy);
  ER_LAUNCH_CHECK();
  return 0;
}

int er_seq_attn_pool_bwd(const float* x, int64_t ld, const int32_t* len, const float* w, const float* dy, int64_t B,
                         int32_t L_buf, int32_t D, float* dx, int64_t lddx, float* partials, er_stream_t stream) {
  ER_REQUIRE(x && len && w && dy && dx && partials && B > 0, "er_seq_attn_pool_bwd: bad arguments");
  ER_REQUIRE(er::ap_shape_ok(L_buf, D), "er_seq_attn_pool_bwd: L_buf = %d, D = %d outside the envelope", L_buf, D);
  ER_REQUIRE(ld >= D && lddx >= D, "er_seq_attn_pool_bwd: a pitch below the width %d", D);
  hipLaunchKernelGGL(er::seq_attn_pool_bwd_kernel, dim3(er_seq_attn_pool_grid(B, L_buf, D)), dim3(er::kFieldThreads),
                     static_cast<size_t>(er_seq_attn_pool_lds_bytes(L_buf, D, 1)), er::as_stream(stream), x, ld, len, w,
                     dy, B, L_buf, D, dx, lddx, partials);
  ER_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
