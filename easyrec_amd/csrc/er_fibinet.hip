// K8d: FiBiNet's two field blocks (reference layers/keras/fibinet.py): the bilinear interaction of BiLinear.call
// (:175-203, `all` / `each`, with and without use_plus) and SENet.call (:63-93), each ONE forward and ONE backward launch
// with nothing but the block's input and output crossing HBM.
//
// Layout of both pairs: a persistent grid of at most 512 workgroups (256 threads; 2 per CU on MI355X) stages the packed
// parameters `theta` in LDS once, then walks chunks of `epb` examples: a chunk's rows are staged in LDS and every phase is
// one flat loop over (example, ...) items between workgroup barriers.  epb = min(8, what is left of 64 KiB beside theta
// / the LDS of one example); the envelope is where one example fits (er_bilinear_lds_bytes, er_senet_lds_bytes).
//
// Parameter gradients: every entry of theta belongs to one fixed thread of every workgroup; it sums the chunk's examples
// in order and adds that to ITS slot of the workgroup's row of `partials` [grid, param_count] (written on the
// workgroup's first chunk, read, added and written by the same thread after).  er_theta_grad_reduce then sums the rows in a
// fixed order into the variables' gradient buffers: no atomics, so two runs and a graph replay give the same bits.
// fp32 throughout.
#include "er_field_block.h"

namespace er {

constexpr int kFbMaxF = 64;
constexpr int kFbMaxD = 64;
constexpr float kSeLnEps = 1e-3f;    // keras LayerNormalization default

// ------------------------------------------------------------------------------------------------ bilinear
// theta: layer l at l * (D * D + D): kernel [D, D] ([in, out] row-major), bias [D].  In LDS the kernel rows sit at the
// odd pitch ldw (a walk down a column, the backward's W^T, is conflict-free), layer l at l * (D * ldw + D).
struct BlGeom {
  int F, D, nw, plus;
  int ldw, np;     // LDS pitch of a kernel row; F (F - 1) / 2 pairs
  int P, lw;       // floats of theta; of theta in LDS
  int fixed, per;  // LDS floats beside the examples (theta + the pair table); per example (the backward's)
};

__host__ __device__ inline BlGeom bl_geom(int F, int D, int each, int plus) {
  BlGeom g;
  g.F = F;
  g.D = D;
  g.nw = each ? F - 1 : 1;
  g.plus = plus;
  g.ldw = odd(D);
  g.np = F * (F - 1) / 2;
  g.P = g.nw * (D * D + D);
  g.lw = g.nw * (D * g.ldw + D);
  g.fixed = g.lw + g.np;
  g.per = F * D + 2 * (F - 1) * D;  // x, u, du (the forward uses the first two)
  return g;
}

__host__ __device__ inline int bl_pair_base(int i, int F) { return i * (2 * F - i - 1) / 2; }  // index of pair (i, i + 1)

inline bool bl_shape_ok(int F, int D) {
  if (F < 2 || F > kFbMaxF || D < 1 || D > kFbMaxD) return false;
  const BlGeom g = bl_geom(F, D, 1, 1);  // (`each` holds the most parameters)
  return 4 * (g.fixed + g.per) <= kFieldLdsBudget;
}

// theta -> LDS at the padded pitch, and the pair table (i << 8 | j) in itertools.combinations order
__device__ inline void bl_stage_theta(const float* __restrict__ theta, const BlGeom& g, float* th, int* pairs) {
  const int D = g.D, per_l = D * D + D;
  for (int t = threadIdx.x; t < g.P; t += kFieldThreads) {
    const int l = t / per_l, r = t - l * per_l;
    float* dst = th + l * (D * g.ldw + D);
    if (r < D * D) {
      const int k = r / D, c = r - k * D;
      dst[k * g.ldw + c] = theta[t];
    } else {
      dst[D * g.ldw + (r - D * D)] = theta[t];
    }
  }
  for (int i = threadIdx.x; i < g.F - 1; i += kFieldThreads) {
    const int base = bl_pair_base(i, g.F);
    for (int j = i + 1; j < g.F; ++j) pairs[base + j - i - 1] = (i << 8) | j;
  }
}

// a chunk's x rows -> LDS, then u_i = x_i W_i + b_i for i < F - 1
__device__ inline void bl_stage_x_u(const float* __restrict__ xb, int ne, const BlGeom& g, const float* th, float* ex) {
  const int F = g.F, D = g.D, FD = F * D;
  for (int t = threadIdx.x; t < ne * FD; t += kFieldThreads) {
    const int e = t / FD;
    ex[e * g.per + (t - e * FD)] = xb[t];
  }
  __syncthreads();
  const int nu = (F - 1) * D;
  for (int t = threadIdx.x; t < ne * nu; t += kFieldThreads) {
    const int e = t / nu, r = t - e * nu;
    const int i = r / D, c = r - i * D;
    const float* W = th + (g.nw == 1 ? 0 : i) * (D * g.ldw + D);
    const float* xi = ex + e * g.per + i * D;
    float acc = 0.f;
    for (int k = 0; k < D; ++k) acc += xi[k] * W[k * g.ldw + c];
    ex[e * g.per + FD + r] = acc + W[D * g.ldw + c];
  }
  __syncthreads();
}

__global__ __launch_bounds__(kFieldThreads) void bilinear_fwd_kernel(const float* __restrict__ x,
                                                                   const float* __restrict__ theta, int64_t B, BlGeom g,
                                                                   int epb, float* __restrict__ out) {
  extern __shared__ float lds[];
  float* th = lds;
  int* pairs = reinterpret_cast<int*>(lds + g.lw);
  float* ex = lds + g.fixed;
  const int F = g.F, D = g.D, FD = F * D, np = g.np;
  bl_stage_theta(theta, g, th, pairs);
  const int64_t nchunks = (B + epb - 1) / epb;
  for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int64_t b0 = chunk * epb;
    const int ne = static_cast<int>(min(static_cast<int64_t>(epb), B - b0));
    __syncthreads();  // (theta and the pair table on the first round; the previous chunk's readers after)
    bl_stage_x_u(x + b0 * FD, ne, g, th, ex);
    if (g.plus) {
      float* ob = out + b0 * np;
      for (int t = threadIdx.x; t < ne * np; t += kFieldThreads) {
        const int e = t / np, p = t - e * np;
        const int i = pairs[p] >> 8, j = pairs[p] & 255;
        const float* u = ex + e * g.per + FD + i * D;
        const float* xj = ex + e * g.per + j * D;
        float acc = 0.f;
        for (int c = 0; c < D; ++c) acc += u[c] * xj[c];
        ob[t] = acc;
      }
    } else {
      float* ob = out + b0 * np * D;
      const int n1 = np * D;
      for (int t = threadIdx.x; t < ne * n1; t += kFieldThreads) {
        const int e = t / n1, r = t - e * n1;
        const int p = r / D, c = r - p * D;
        const int i = pairs[p] >> 8, j = pairs[p] & 255;
        ob[t] = ex[e * g.per + FD + i * D + c] * ex[e * g.per + j * D + c];
      }
    }
  }
}

__global__ __launch_bounds__(kFieldThreads) void bilinear_bwd_kernel(const float* __restrict__ x,
                                                                   const float* __restrict__ theta,
                                                                   const float* __restrict__ dout, int64_t B, BlGeom g,
                                                                   int epb, float* __restrict__ dx,
                                                                   float* __restrict__ partials) {
  extern __shared__ float lds[];
  float* th = lds;
  int* pairs = reinterpret_cast<int*>(lds + g.lw);
  float* ex = lds + g.fixed;
  const int F = g.F, D = g.D, FD = F * D, np = g.np, nu = (F - 1) * D;
  const int doff = FD + nu;  // du
  bl_stage_theta(theta, g, th, pairs);
  float* part = partials + static_cast<int64_t>(blockIdx.x) * g.P;
  const int64_t nchunks = (B + epb - 1) / epb;
  for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int64_t b0 = chunk * epb;
    const int ne = static_cast<int>(min(static_cast<int64_t>(epb), B - b0));
    __syncthreads();
    bl_stage_x_u(x + b0 * FD, ne, g, th, ex);
    // du_i = sum_{j > i} dp_ij x_j
    const float* db = dout + b0 * np * (g.plus ? 1 : D);
    for (int t = threadIdx.x; t < ne * nu; t += kFieldThreads) {
      const int e = t / nu, r = t - e * nu;
      const int i = r / D, c = r - i * D;
      const int base = bl_pair_base(i, F);
      const float* X = ex + e * g.per;
      float acc = 0.f;
      if (g.plus) {
        const float* d = db + e * np + base;
        for (int j = i + 1; j < F; ++j) acc += d[j - i - 1] * X[j * D + c];
      } else {
        const float* d = db + (static_cast<int64_t>(e) * np + base) * D + c;
        for (int j = i + 1; j < F; ++j) acc += d[(j - i - 1) * D] * X[j * D + c];
      }
      ex[e * g.per + doff + r] = acc;
    }
    __syncthreads();
    // dx_f = sum_{i < f} dp_if u_i (the field as x_j) + du_f W_f^T (the field as x_i, f < F - 1)
    float* dxb = dx + b0 * FD;
    for (int t = threadIdx.x; t < ne * FD; t += kFieldThreads) {
      const int e = t / FD, r = t - e * FD;
      const int f = r / D, c = r - f * D;
      const float* X = ex + e * g.per;
      float acc = 0.f;
      for (int i = 0; i < f && i < F - 1; ++i) {
        const int p = bl_pair_base(i, F) + f - i - 1;
        const float d = g.plus ? db[e * np + p] : db[(static_cast<int64_t>(e) * np + p) * D + c];
        acc += d * X[FD + i * D + c];
      }
      if (f < F - 1) {
        const float* W = th + (g.nw == 1 ? 0 : f) * (D * g.ldw + D) + c * g.ldw;
        const float* du = X + doff + f * D;
        float a2 = 0.f;
        for (int k = 0; k < D; ++k) a2 += du[k] * W[k];
        acc += a2;
      }
      dxb[t] = acc;
    }
    // theta partials: dW_l[k, c] = sum_e sum_{i of l} x_i[k] du_i[c], db_l[c] = sum_e sum_{i of l} du_i[c]
    const int per_l = D * D + D;
    const bool first = chunk == blockIdx.x;
    for (int t = threadIdx.x; t < g.P; t += kFieldThreads) {
      const int l = t / per_l, r = t - l * per_l;
      const int i0 = g.nw == 1 ? 0 : l, i1 = g.nw == 1 ? F - 1 : l + 1;
      float acc = 0.f;
      if (r < D * D) {
        const int k = r / D, c = r - k * D;
        for (int e = 0; e < ne; ++e)
          for (int i = i0; i < i1; ++i) acc += ex[e * g.per + i * D + k] * ex[e * g.per + doff + i * D + c];
      } else {
        const int c = r - D * D;
        for (int e = 0; e < ne; ++e)
          for (int i = i0; i < i1; ++i) acc += ex[e * g.per + doff + i * D + c];
      }
      part[t] = first ? acc : part[t] + acc;
    }
  }
}

// ------------------------------------------------------------------------------------------------ SENet
// theta: W1 [Z, R], b1 [R], W2 [R, FD], b2 [FD], then gamma [FD], beta [FD] with the layer norm (Z = 2 F G, FD = F D).
struct SeGeom {
  int F, D, G, R, skip, ln;
  int gs, Z, FD;  // columns per squeeze group; squeezed width; row width
  int w1, b1, w2, b2, gm, bt, P;
  int per_f, per_b;  // LDS floats per example, forward / backward
};

__host__ __device__ inline SeGeom se_geom(int F, int D, int G, int R, int skip, int ln) {
  SeGeom g;
  g.F = F;
  g.D = D;
  g.G = G;
  g.R = R;
  g.skip = skip;
  g.ln = ln;
  g.gs = D / G;
  g.Z = 2 * F * G;
  g.FD = F * D;
  g.w1 = 0;
  g.b1 = g.w1 + g.Z * R;
  g.w2 = g.b1 + R;
  g.b2 = g.w2 + R * g.FD;
  g.gm = g.b2 + g.FD;
  g.bt = g.gm + g.FD;
  g.P = ln ? g.bt + g.FD : g.gm;
  g.per_f = 2 * g.FD + g.Z + R + 2;               // x, o, z, a1, (mean, rstd)
  g.per_b = 4 * g.FD + 2 * g.Z + 2 * R + 2;       // x, w, o -> xhat, do -> dw, z, dz, a1, dpre1, (mean, rstd)
  return g;
}

inline bool se_shape_ok(int F, int D, int G, int R) {
  if (F < 1 || F > kFbMaxF || D < 1 || D > kFbMaxD || G < 1 || D % G != 0 || R < 1 || R > 2 * F * G) return false;
  const SeGeom g = se_geom(F, D, G, R, 1, 1);
  return 4 * (g.P + g.per_b) <= kFieldLdsBudget;
}

// x rows -> LDS; z (per field the G group maxima, then the G group means); a1 = relu(z W1 + b1);
// w = a1 W2 + b2 -> wbuf (nullptr: not kept); o = x w (+ x) -> obuf; the rows' mean and 1 / sqrt(var + eps) of o.
// Offsets are per example (floats from the example's base).
__device__ inline void se_forward(const float* __restrict__ xb, int ne, const SeGeom& g, const float* th, float* ex,
                                  int per, int xo, int wo, int oo, int zo, int ao, int so) {
  const int FD = g.FD, Z = g.Z, R = g.R, G = g.G, gs = g.gs;
  for (int t = threadIdx.x; t < ne * FD; t += kFieldThreads) {
    const int e = t / FD;
    ex[e * per + xo + (t - e * FD)] = xb[t];
  }
  __syncthreads();
  const int nz = g.F * G;
  for (int t = threadIdx.x; t < ne * nz; t += kFieldThreads) {
    const int e = t / nz, r = t - e * nz;
    const int f = r / G, q = r - f * G;
    const float* v = ex + e * per + xo + f * g.D + q * gs;
    float m = v[0], s = v[0];
    for (int c = 1; c < gs; ++c) {
      m = fmaxf(m, v[c]);
      s += v[c];
    }
    ex[e * per + zo + f * 2 * G + q] = m;
    ex[e * per + zo + f * 2 * G + G + q] = s / static_cast<float>(gs);
  }
  __syncthreads();
  for (int t = threadIdx.x; t < ne * R; t += kFieldThreads) {
    const int e = t / R, r = t - e * R;
    const float* z = ex + e * per + zo;
    float acc = 0.f;
    for (int k = 0; k < Z; ++k) acc += z[k] * th[g.w1 + k * R + r];
    acc += th[g.b1 + r];
    ex[e * per + ao + r] = acc > 0.f ? acc : 0.f;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < ne * FD; t += kFieldThreads) {
    const int e = t / FD, c = t - e * FD;
    const float* a = ex + e * per + ao;
    float acc = 0.f;
    for (int r = 0; r < R; ++r) acc += a[r] * th[g.w2 + r * FD + c];
    acc += th[g.b2 + c];
    const float xv = ex[e * per + xo + c];
    if (wo >= 0) ex[e * per + wo + c] = acc;
    const float o = xv * acc;
    ex[e * per + oo + c] = g.skip ? o + xv : o;
  }
  __syncthreads();
  if (g.ln) {  // one wave per example, lanes strided over the row
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    for (int e = wave; e < ne; e += kFieldWaves) {
      const float* o = ex + e * per + oo;
      float s = 0.f;
      for (int c = lane; c < FD; c += kWave) s += o[c];
      const float mean = wave_sum(s) / static_cast<float>(FD);
      float q = 0.f;
      for (int c = lane; c < FD; c += kWave) q += (o[c] - mean) * (o[c] - mean);
      const float var = wave_sum(q) / static_cast<float>(FD);
      if (lane == 0) {
        ex[e * per + so] = mean;
        ex[e * per + so + 1] = 1.f / sqrtf(var + kSeLnEps);
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kFieldThreads) void senet_fwd_kernel(const float* __restrict__ x,
                                                                const float* __restrict__ theta, int64_t B, SeGeom g,
                                                                int epb, float* __restrict__ y, float* __restrict__ a1) {
  extern __shared__ float lds[];
  float* th = lds;
  float* ex = lds + g.P;
  const int FD = g.FD, per = g.per_f;
  const int xo = 0, oo = FD, zo = 2 * FD, ao = zo + g.Z, so = ao + g.R;
  for (int t = threadIdx.x; t < g.P; t += kFieldThreads) th[t] = theta[t];
  const int64_t nchunks = (B + epb - 1) / epb;
  for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int64_t b0 = chunk * epb;
    const int ne = static_cast<int>(min(static_cast<int64_t>(epb), B - b0));
    __syncthreads();
    se_forward(x + b0 * FD, ne, g, th, ex, per, xo, -1, oo, zo, ao, so);
    float* yb = y + b0 * FD;
    for (int t = threadIdx.x; t < ne * FD; t += kFieldThreads) {
      const int e = t / FD, c = t - e * FD;
      float o = ex[e * per + oo + c];
      if (g.ln) o = (o - ex[e * per + so]) * ex[e * per + so + 1] * th[g.gm + c] + th[g.bt + c];
      yb[t] = o;
    }
    if (a1 != nullptr) {
      for (int t = threadIdx.x; t < ne * g.R; t += kFieldThreads) {
        const int e = t / g.R;
        a1[b0 * g.R + t] = ex[e * per + ao + (t - e * g.R)];
      }
    }
  }
}

__global__ __launch_bounds__(kFieldThreads) void senet_bwd_kernel(const float* __restrict__ x,
                                                                const float* __restrict__ theta,
                                                                const float* __restrict__ dy, int64_t B, SeGeom g,
                                                                int epb, float* __restrict__ dx,
                                                                float* __restrict__ partials) {
  extern __shared__ float lds[];
  float* th = lds;
  float* ex = lds + g.P;
  const int FD = g.FD, Z = g.Z, R = g.R, G = g.G, gs = g.gs, per = g.per_b;
  const int xo = 0, wo = FD, oo = 2 * FD, go = 3 * FD;  // x, w, o -> xhat, do -> dw
  const int zo = 4 * FD, dzo = zo + Z, ao = dzo + Z, dao = ao + R, so = dao + R;
  for (int t = threadIdx.x; t < g.P; t += kFieldThreads) th[t] = theta[t];
  float* part = partials + static_cast<int64_t>(blockIdx.x) * g.P;
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int64_t nchunks = (B + epb - 1) / epb;
  for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int64_t b0 = chunk * epb;
    const int ne = static_cast<int>(min(static_cast<int64_t>(epb), B - b0));
    const bool first = chunk == blockIdx.x;
    __syncthreads();
    se_forward(x + b0 * FD, ne, g, th, ex, per, xo, wo, oo, zo, ao, so);
    const float* dyb = dy + b0 * FD;
    if (g.ln) {
      // xhat over o; dxhat = dy gamma -> go; then do = rstd (dxhat - mean(dxhat) - xhat mean(dxhat xhat))
      for (int t = threadIdx.x; t < ne * FD; t += kFieldThreads) {
        const int e = t / FD, c = t - e * FD;
        float* E = ex + e * per;
        E[oo + c] = (E[oo + c] - E[so]) * E[so + 1];
        E[go + c] = dyb[t] * th[g.gm + c];
      }
      __syncthreads();
      // dgamma = sum_e dy xhat, dbeta = sum_e dy
      for (int c = threadIdx.x; c < FD; c += kFieldThreads) {
        float ag = 0.f, ab = 0.f;
        for (int e = 0; e < ne; ++e) {
          const float d = dyb[e * FD + c];
          ag += d * ex[e * per + oo + c];
          ab += d;
        }
        part[g.gm + c] = first ? ag : part[g.gm + c] + ag;
        part[g.bt + c] = first ? ab : part[g.bt + c] + ab;
      }
      for (int e = wave; e < ne; e += kFieldWaves) {
        float* E = ex + e * per;
        float s1 = 0.f, s2 = 0.f;
        for (int c = lane; c < FD; c += kWave) {
          s1 += E[go + c];
          s2 += E[go + c] * E[oo + c];
        }
        const float m1 = wave_sum(s1) / static_cast<float>(FD), m2 = wave_sum(s2) / static_cast<float>(FD);
        const float rstd = E[so + 1];
        for (int c = lane; c < FD; c += kWave) E[go + c] = rstd * (E[go + c] - m1 - E[oo + c] * m2);
      }
    } else {
      for (int t = threadIdx.x; t < ne * FD; t += kFieldThreads) {
        const int e = t / FD;
        ex[e * per + go + (t - e * FD)] = dyb[t];
      }
    }
    __syncthreads();
    // dx = do w (+ do) (the squeeze's part is added below by the same thread); dw = do x -> go
    float* dxb = dx + b0 * FD;
    for (int t = threadIdx.x; t < ne * FD; t += kFieldThreads) {
      const int e = t / FD, c = t - e * FD;
      float* E = ex + e * per;
      const float d = E[go + c];
      const float v = d * E[wo + c];
      E[wo + c] = g.skip ? v + d : v;  // (w is not needed after this: the slot carries dx's first part)
      E[go + c] = d * E[xo + c];
    }
    __syncthreads();
    // da1[r] = sum_c dw[c] W2[r, c], through the ReLU: one wave per (example, r)
    for (int t = wave; t < ne * R; t += kFieldWaves) {
      const int e = t / R, r = t - e * R;
      const float* dw = ex + e * per + go;
      const float* W = th + g.w2 + r * FD;
      float s = 0.f;
      for (int c = lane; c < FD; c += kWave) s += dw[c] * W[c];
      s = wave_sum(s);
      if (lane == 0) ex[e * per + dao + r] = ex[e * per + ao + r] > 0.f ? s : 0.f;
    }
    // db2 = sum_e dw, dW2[r, c] = sum_e a1[r] dw[c]
    for (int t = threadIdx.x; t < FD + R * FD; t += kFieldThreads) {
      float acc = 0.f;
      int k;
      if (t < FD) {
        for (int e = 0; e < ne; ++e) acc += ex[e * per + go + t];
        k = g.b2 + t;
      } else {
        const int q = t - FD, r = q / FD, c = q - r * FD;
        for (int e = 0; e < ne; ++e) acc += ex[e * per + ao + r] * ex[e * per + go + c];
        k = g.w2 + q;
      }
      part[k] = first ? acc : part[k] + acc;
    }
    __syncthreads();
    // dz[k] = sum_r dpre1[r] W1[k, r]
    for (int t = threadIdx.x; t < ne * Z; t += kFieldThreads) {
      const int e = t / Z, k = t - e * Z;
      const float* d = ex + e * per + dao;
      float acc = 0.f;
      for (int r = 0; r < R; ++r) acc += d[r] * th[g.w1 + k * R + r];
      ex[e * per + dzo + k] = acc;
    }
    // db1 = sum_e dpre1, dW1[k, r] = sum_e z[k] dpre1[r]
    for (int t = threadIdx.x; t < R + Z * R; t += kFieldThreads) {
      float acc = 0.f;
      int k;
      if (t < R) {
        for (int e = 0; e < ne; ++e) acc += ex[e * per + dao + t];
        k = g.b1 + t;
      } else {
        const int q = t - R, zk = q / R, r = q - zk * R;
        for (int e = 0; e < ne; ++e) acc += ex[e * per + zo + zk] * ex[e * per + dao + r];
        k = g.w1 + q;
      }
      part[k] = first ? acc : part[k] + acc;
    }
    __syncthreads();
    // the squeeze: the mean's share to every column of the group, the max's split evenly among the tied maxima
    for (int t = threadIdx.x; t < ne * FD; t += kFieldThreads) {
      const int e = t / FD, c = t - e * FD;
      const int f = c / g.D, q = (c - f * g.D) / gs;
      const float* E = ex + e * per;
      const float m = E[zo + f * 2 * G + q], xv = E[xo + c];
      float acc = E[wo + c] + E[dzo + f * 2 * G + G + q] / static_cast<float>(gs);
      if (xv == m) {
        const float* v = E + xo + f * g.D + q * gs;
        int ties = 0;
        for (int k = 0; k < gs; ++k) ties += v[k] == m;
        acc += E[dzo + f * 2 * G + q] / static_cast<float>(ties);
      }
      dxb[t] = acc;
    }
  }
}

}  // namespace er

extern "C" {

int64_t er_bilinear_param_count(int32_t F, int32_t D, int each) {
  if (F < 2 || D < 1) return 0;
  return static_cast<int64_t>(each ? F - 1 : 1) * (D * D + D);
}

int64_t er_bilinear_lds_bytes(int32_t F, int32_t D) {
  if (F < 2 || D < 1 || F > 32768 || D > 32768) return 0;
  const int64_t ldw = D | 1;
  return 4 * ((F - 1) * (D * ldw + D) + static_cast<int64_t>(F) * (F - 1) / 2 + static_cast<int64_t>(F) * D +
              2 * static_cast<int64_t>(F - 1) * D);
}

int32_t er_bilinear_epb(int32_t F, int32_t D, int each) {
  if (!er::bl_shape_ok(F, D)) return 0;
  const er::BlGeom g = er::bl_geom(F, D, each, 1);
  return er::epb(g.fixed, g.per);
}

int32_t er_bilinear_grid(int64_t B, int32_t F, int32_t D, int each) {
  const int epb = er_bilinear_epb(F, D, each);
  return epb > 0 && B > 0 ? er::persistent_grid(B, epb) : 0;
}

int er_bilinear_fwd(const float* x, const float* theta, int64_t B, int32_t F, int32_t D, int each, int plus, float* out,
                    er_stream_t stream) {
  ER_REQUIRE(x && theta && out && B > 0, "er_bilinear_fwd: bad arguments");
  ER_REQUIRE(er::bl_shape_ok(F, D), "er_bilinear_fwd: F = %d, D = %d outside the envelope", F, D);
  const er::BlGeom g = er::bl_geom(F, D, each, plus);
  const int epb = er::epb(g.fixed, g.per);
  hipLaunchKernelGGL(er::bilinear_fwd_kernel, dim3(er::persistent_grid(B, epb)), dim3(er::kFieldThreads),
                     4 * (g.fixed + epb * g.per), er::as_stream(stream), x, theta, B, g, epb, out);
  ER_LAUNCH_CHECK();
  return 0;
}

int er_bilinear_bwd(const float* x, const float* theta, const float* dout, int64_t B, int32_t F, int32_t D, int each,
                    int plus, float* dx, float* partials, er_stream_t stream) {
  ER_REQUIRE(x && theta && dout && dx && partials && B > 0, "er_bilinear_bwd: bad arguments");
  ER_REQUIRE(er::bl_shape_ok(F, D), "er_bilinear_bwd: F = %d, D = %d outside the envelope", F, D);
  const er::BlGeom g = er::bl_geom(F, D, each, plus);
  const int epb = er::epb(g.fixed, g.per);
  hipLaunchKernelGGL(er::bilinear_bwd_kernel, dim3(er::persistent_grid(B, epb)), dim3(er::kFieldThreads),
                     4 * (g.fixed + epb * g.per), er::as_stream(stream), x, theta, dout, B, g, epb, dx, partials);
  ER_LAUNCH_CHECK();
  return 0;
}

int64_t er_senet_param_count(int32_t F, int32_t D, int32_t G, int32_t R, int ln) {
  if (F < 1 || D < 1 || G < 1 || R < 1 || F > 32768 || D > 32768 || G > D) return 0;
  const int64_t Z = 2 * static_cast<int64_t>(F) * G, FD = static_cast<int64_t>(F) * D;
  return Z * R + R + R * FD + FD + (ln ? 2 * FD : 0);
}

int64_t er_senet_lds_bytes(int32_t F, int32_t D, int32_t G, int32_t R) {
  const int64_t P = er_senet_param_count(F, D, G, R, 1);
  if (P == 0) return 0;
  const int64_t Z = 2 * static_cast<int64_t>(F) * G, FD = static_cast<int64_t>(F) * D;
  return 4 * (P + 4 * FD + 2 * Z + 2 * R + 2);
}

int32_t er_senet_epb(int32_t F, int32_t D, int32_t G, int32_t R, int ln, int bwd) {
  if (!er::se_shape_ok(F, D, G, R)) return 0;
  const er::SeGeom g = er::se_geom(F, D, G, R, 1, ln);
  return er::epb(g.P, bwd ? g.per_b : g.per_f);
}

int32_t er_senet_grid(int64_t B, int32_t F, int32_t D, int32_t G, int32_t R, int ln) {
  const int epb = er_senet_epb(F, D, G, R, ln, 1);
  return epb > 0 && B > 0 ? er::persistent_grid(B, epb) : 0;
}

int er_senet_fwd(const float* x, const float* theta, int64_t B, int32_t F, int32_t D, int32_t G, int32_t R, int skip,
                 int ln, float* y, float* a1, er_stream_t stream) {
  ER_REQUIRE(x && theta && y && B > 0, "er_senet_fwd: bad arguments");
  ER_REQUIRE(er::se_shape_ok(F, D, G, R), "er_senet_fwd: F = %d, D = %d, G = %d, R = %d outside the envelope", F, D, G, R);
  const er::SeGeom g = er::se_geom(F, D, G, R, skip, ln);
  const int epb = er::epb(g.P, g.per_f);
  hipLaunchKernelGGL(er::senet_fwd_kernel, dim3(er::persistent_grid(B, epb)), dim3(er::kFieldThreads),
                     4 * (g.P + epb * g.per_f), er::as_stream(stream), x, theta, B, g, epb, y, a1);
  ER_LAUNCH_CHECK();
  return 0;
}

int er_senet_bwd(const float* x, const float* theta, const float* dy, int64_t B, int32_t F, int32_t D, int32_t G,
                 int32_t R, int skip, int ln, float* dx, float* partials, er_stream_t stream) {
  ER_REQUIRE(x && theta && dy && dx && partials && B > 0, "er_senet_bwd: bad arguments");
  ER_REQUIRE(er::se_shape_ok(F, D, G, R), "er_senet_bwd: F = %d, D = %d, G = %d, R = %d outside the envelope", F, D, G, R);
  const er::SeGeom g = er::se_geom(F, D, G, R, skip, ln);
  const int epb = er::epb(g.P, g.per_b);
  hipLaunchKernelGGL(er::senet_bwd_kernel, dim3(er::persistent_grid(B, epb)), dim3(er::kFieldThreads),
                     4 * (g.P + epb * g.per_b), er::as_stream(stream), x, theta, dy, B, g, epb, dx, partials);
  ER_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
