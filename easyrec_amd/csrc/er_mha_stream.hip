// K8f-s: the masked multi-head attention core of K8f (er_mha.hip) for sequences whose (example, head) unit does not fit
// in LDS: the keys are streamed in tiles, the softmax is online, and every product is v_mfma_f32_32x32x2_f32.
//
// Split.  A wave owns 32 query rows of one (example, head) unit from the first key tile to the last (forward and the
// dQ pass), or 32 keys from the first query tile to the last (the dK | dV pass): a row's maximum, sum and rescale, and
// every output element's sum, stay inside one wave.  A workgroup is 1, 2 or 4 such waves (by F, or by T in the dK | dV
// pass) that share the streamed tiles: K and V (dK | dV pass: Q and dctx) go through LDS once per workgroup, KT rows at
// the odd pitch P = 32 NB + 1 floats, NB = ceil(ds / 32), columns ds .. 32 NB - 1 and rows past the end zero.  KT = 64 up
// to ds = 64 and 32 above; a tile is worked in sub-tiles of 32 rows.  Workgroups are persistent (at most kStMaxGrid) and
// walk (unit, row block) items grid-stride.
//
// Layouts.  The MFMA takes A[m][k] from lane m + 32 k, B[k][n] from lane n + 32 k, and leaves C[m][n] in lane
// n + 32 hf, register i, with m = (i & 3) + 8 (i >> 2) + 4 hf.  The wave's own 32 rows (Q, dctx; K, V in the dK | dV
// pass) live in registers as a B operand for the whole walk: reg[t] = row[lane & 31][2 t + hf].  The scores are
// computed TRANSPOSED, S^T = K_tile Q^T (A from LDS, B from registers): a lane then holds 16 scores of ONE query, so
// the row maximum and sum are 16 in-lane steps and one exchange with lane ^ 32, and P^T[key][query] already sits where
// the second product wants its B operand.  O^T += V^T P^T pairs the keys as the C layout holds them: step i contracts
// the keys (i & 3) + 8 (i >> 2) and that + 4, so its B operand is register i as it stands - P never leaves the
// registers, neither through LDS nor through HBM.  The output accumulators (O^T, dQ^T, dK^T, dV^T: NB blocks of 32 x 32)
// stay in registers across the walk.  The dK | dV pass runs the same scheme with the roles of queries and keys swapped
// (S = Q_tile K^T, dV^T += dctx^T P, dK^T += Q^T dS).
//
// Backward.  No atomics: launch (a) owns query rows - delta = rowsum(dctx o ctx) in its prologue (as the diagonal of one
// MFMA tile, in the summation order of dP, so that a one-key row has dS = 0 exactly), then dQ; launch (b) owns keys - dK
// and dV.  Both recompute P = exp(s - lse) from q, k and the forward's lse.  Every sum has one owner and a fixed order:
// two runs and a graph replay give the same bits.
#include <math.h>

#include "er_common.h"

namespace er {

typedef float st_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kStMaxGrid = 2048;  // persistent workgroups
constexpr int kStMaxDs = 128;
constexpr int kStMaxLen = 4096;
constexpr int kStMaxThreads = 256;  // 4 waves

template <int NB>
struct StGeom {
  static constexpr int DP = 32 * NB;            // padded head size
  static constexpr int P = DP + 1;              // LDS row pitch (odd: a walk over rows at one column is conflict-free)
  static constexpr int KT = NB <= 2 ? 64 : 32;  // rows of a streamed tile
};

inline int st_blocks(int ds) { return (ds + 31) / 32; }
inline int st_tile(int ds) { return st_blocks(ds) <= 2 ? 64 : 32; }
inline int st_waves(int rows) { return rows <= 32 ? 1 : rows <= 64 ? 2 : 4; }
inline bool st_shape_ok(int F, int T, int H, int ds) {
  return F >= 1 && T >= 1 && H >= 1 && ds >= 1 && ds <= kStMaxDs && F <= kStMaxLen && T <= kStMaxLen;
}

struct StArgs {
  const float* q;
  const float* k;
  const float* v;
  const float* dctx;
  const float* ctx_in;  // the backward's ctx
  const int32_t* mask;
  float* ctx;
  float* lse;    // [B, H, F]: written by the forward, read by the backward
  float* delta;  // [B, H, F]: written by launch (a), read by launch (b)
  float* dq;
  float* dk;
  float* dv;
  int64_t ldq, ldk, ldv, lddq, lddk, lddv;  // row pitches in floats
  int64_t units;                            // B * H
  int F, T, H, ds;
  int vec;  // bit 0 .. 7: q, k, v, dctx | ctx (both ways), dq, dk, dv take 16-byte accesses
  float scale;
};

__device__ __forceinline__ float4 st_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// rows row0 .. row0 + KT - 1 of src (rows >= n_rows and columns >= ds: 0) -> dst at pitch P
template <int NB>
__device__ __forceinline__ void st_stage(int tid, int nthr, const float* __restrict__ src, int64_t pitch, int row0,
                                         int n_rows, int ds, bool vec, float* dst) {
  constexpr int Q4 = StGeom<NB>::DP / 4, P = StGeom<NB>::P, KT = StGeom<NB>::KT;
  for (int t = tid; t < KT * Q4; t += nthr) {
    const int r = t / Q4, c = (t - r * Q4) << 2;
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row0 + r < n_rows) {
      const float* p = src + static_cast<int64_t>(row0 + r) * pitch + c;
      if (vec) {
        if (c < ds) x = st_ld4(p);
      } else {
        if (c < ds) x.x = p[0];
        if (c + 1 < ds) x.y = p[1];
        if (c + 2 < ds) x.z = p[2];
        if (c + 3 < ds) x.w = p[3];
      }
    }
    float* d = dst + r * P + c;
    d[0] = x.x;
    d[1] = x.y;
    d[2] = x.z;
    d[3] = x.w;
  }
}

// the wave's own rows as an MFMA operand: reg[t] = src[row][2 t + hf] (0 past n_rows or ds)
template <int NB>
__device__ __forceinline__ void st_load_rows(const float* __restrict__ src, int64_t pitch, int row, int n_rows, int ds,
                                             bool vec, int hf, float (&reg)[16 * NB]) {
  const bool on = row < n_rows;
  const float* p = src + static_cast<int64_t>(on ? row : 0) * pitch;
  if (vec) {
#pragma unroll
    for (int u = 0; u < 8 * NB; ++u) {
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (on && 4 * u < ds) x = st_ld4(p + 4 * u);
      reg[2 * u] = hf ? x.y : x.x;
      reg[2 * u + 1] = hf ? x.w : x.z;
    }
  } else {
#pragma unroll
    for (int t = 0; t < 16 * NB; ++t) {
      const int c = 2 * t + hf;
      reg[t] = on && c < ds ? p[c] : 0.f;
    }
  }
}

// the largest adder of the example's keys (0 without a mask): every thread of the workgroup calls it
__device__ __forceinline__ float st_mask_top(int tid, int nthr, const int32_t* __restrict__ mrow, int T, float* red) {
  if (mrow == nullptr) return 0.f;
  float top = -INFINITY;
  for (int j = tid; j < T; j += nthr) top = fmaxf(top, (1.0f - static_cast<float>(mrow[j])) * -10000.0f);
  top = wave_max(top);
  if ((tid & (kWave - 1)) == 0) red[tid / kWave] = top;
  __syncthreads();
  float r = red[0];
  for (int w = 1; w < nthr / kWave; ++w) r = fmaxf(r, red[w]);
  __syncthreads();  // (red is written again by the next item)
  return r;
}

// key j's adder relative to the largest; a key past the end: -inf, which makes its probability exactly 0
__device__ __forceinline__ float st_adder(const int32_t* __restrict__ mrow, int j, int T, float top) {
  if (j >= T) return -INFINITY;
  return mrow != nullptr ? (1.0f - static_cast<float>(mrow[j])) * -10000.0f - top : 0.f;
}

// C^T tile [32 tile rows at r0][the wave's 32 rows] = tile . own^T over the padded head size, k ascending
template <int NB>
__device__ __forceinline__ st_f32x16 st_mm_t(const float* tile, int r0, int col, int hf, const float (&own)[16 * NB]) {
  constexpr int P = StGeom<NB>::P;
  const float* ap = tile + (r0 + col) * P + hf;
  st_f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 16 * NB; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * t], own[t], acc, 0, 0, 0);
  return acc;
}

// out^T[blk] [32 columns of the tile][the wave's 32 rows] += tile^T . w over the sub-tile's 32 rows at r0, paired as
// the C layout holds them: step i takes the rows (i & 3) + 8 (i >> 2) (+ 4 in the upper half-wave) and w[i] as it stands
template <int NB>
__device__ __forceinline__ void st_mm_acc(const float* tile, int r0, int col, int hf, const float (&w)[16],
                                          st_f32x16 (&out)[NB]) {
  constexpr int P = StGeom<NB>::P;
  const float* ap = tile + (r0 + 4 * hf) * P + col;
#pragma unroll
  for (int blk = 0; blk < NB; ++blk)
#pragma unroll
    for (int i = 0; i < 16; ++i)
      out[blk] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[((i & 3) + 8 * (i >> 2)) * P + 32 * blk], w[i], out[blk], 0, 0, 0);
}

// out^T -> dst[row][c] = out^T[c][row] * mul for c < ds: the lane's row, four consecutive columns per register group
template <int NB>
__device__ __forceinline__ void st_store_t(const st_f32x16 (&out)[NB], float mul, float* __restrict__ dst, int ds, bool vec,
                                           int hf) {
#pragma unroll
  for (int blk = 0; blk < NB; ++blk)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int c = 32 * blk + 8 * g + 4 * hf;
      const float x0 = out[blk][4 * g] * mul, x1 = out[blk][4 * g + 1] * mul, x2 = out[blk][4 * g + 2] * mul,
                  x3 = out[blk][4 * g + 3] * mul;
      if (vec) {
        if (c < ds) *reinterpret_cast<float4*>(dst + c) = make_float4(x0, x1, x2, x3);
      } else {
        if (c < ds) dst[c] = x0;
        if (c + 1 < ds) dst[c + 1] = x1;
        if (c + 2 < ds) dst[c + 2] = x2;
        if (c + 3 < ds) dst[c + 3] = x3;
      }
    }
}

template <int NB>
__device__ __forceinline__ void st_zero(st_f32x16 (&out)[NB]) {
#pragma unroll
  for (int blk = 0; blk < NB; ++blk)
#pragma unroll
    for (int i = 0; i < 16; ++i) out[blk][i] = 0.f;
}

// ------------------------------------------------------------------------------------------------------ forward
template <int NB>
__global__ __launch_bounds__(kStMaxThreads) void attn_stream_fwd_kernel(StArgs a) {
  constexpr int P = StGeom<NB>::P, KT = StGeom<NB>::KT;
  __shared__ float Ks[KT * P], Vs[KT * P], adds[KT], red[4];
  const int tid = threadIdx.x, nthr = blockDim.x, wave = tid / kWave;
  const int col = tid & 31, hf = (tid >> 5) & 1;
  const int F = a.F, T = a.T, H = a.H, ds = a.ds;
  const int wg_rows = 32 * (nthr / kWave);
  const int64_t rblocks = (F + wg_rows - 1) / wg_rows, items = a.units * rblocks;
  const int64_t dctx = static_cast<int64_t>(H) * ds;
  for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {
    const int64_t u = w / rblocks, b = u / H;
    const int h = static_cast<int>(u - b * H);
    const int row = static_cast<int>(w - u * rblocks) * wg_rows + 32 * wave + col;
    float qr[16 * NB];
    st_load_rows<NB>(a.q + b * F * a.ldq + h * ds, a.ldq, row, F, ds, a.vec & 1, hf, qr);
    const int32_t* mrow = a.mask != nullptr ? a.mask + b * T : nullptr;
    const float top = st_mask_top(tid, nthr, mrow, T, red);
    const float* kp = a.k + b * T * a.ldk + h * ds;
    const float* vp = a.v + b * T * a.ldv + h * ds;
    st_f32x16 o[NB];
    st_zero<NB>(o);
    float m = -INFINITY, l = 0.f;
    for (int j0 = 0; j0 < T; j0 += KT) {
      st_stage<NB>(tid, nthr, kp, a.ldk, j0, T, ds, a.vec & 2, Ks);
      st_stage<NB>(tid, nthr, vp, a.ldv, j0, T, ds, a.vec & 4, Vs);
      for (int j = tid; j < KT; j += nthr) adds[j] = st_adder(mrow, j0 + j, T, top);
      __syncthreads();
      for (int js = 0; js < KT && j0 + js < T; js += 32) {
        const st_f32x16 s = st_mm_t<NB>(Ks, js, col, hf, qr);
        float p[16];
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          p[i] = s[i] * a.scale + adds[js + (i & 3) + 8 * (i >> 2) + 4 * hf];
          mx = fmaxf(mx, p[i]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, kWave));
        const float mnew = fmaxf(m, mx);  // (finite: the sub-tile's first key exists)
        const float alpha = expf(m - mnew);
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          p[i] = expf(p[i] - mnew);
          sum += p[i];
        }
        sum = sum + __shfl_xor(sum, 32, kWave);
        l = l * alpha + sum;
        m = mnew;
#pragma unroll
        for (int blk = 0; blk < NB; ++blk)
#pragma unroll
          for (int i = 0; i < 16; ++i) o[blk][i] *= alpha;
        st_mm_acc<NB>(Vs, js, col, hf, p, o);
      }
      __syncthreads();  // (the next tile restages)
    }
    if (row < F) {
      st_store_t<NB>(o, 1.0f / l, a.ctx + (b * F + row) * dctx + h * ds, ds, a.vec & 16, hf);
      if (hf == 0) a.lse[u * F + row] = m + logf(l);
    }
  }
}

// ------------------------------------------------------------------------------- backward (a): delta, then dQ
template <int NB>
__global__ __launch_bounds__(kStMaxThreads) void attn_stream_bwd_dq_kernel(StArgs a) {
  constexpr int P = StGeom<NB>::P, KT = StGeom<NB>::KT;
  __shared__ float Ks[KT * P], Vs[KT * P], adds[KT], red[4];
  const int tid = threadIdx.x, nthr = blockDim.x, wave = tid / kWave;
  const int col = tid & 31, hf = (tid >> 5) & 1;
  const int F = a.F, T = a.T, H = a.H, ds = a.ds;
  const int wg_rows = 32 * (nthr / kWave);
  const int64_t rblocks = (F + wg_rows - 1) / wg_rows, items = a.units * rblocks;
  const int64_t dctx = static_cast<int64_t>(H) * ds;
  for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {
    const int64_t u = w / rblocks, b = u / H;
    const int h = static_cast<int>(u - b * H);
    const int row = static_cast<int>(w - u * rblocks) * wg_rows + 32 * wave + col;
    float qr[16 * NB], cr[16 * NB];
    st_load_rows<NB>(a.q + b * F * a.ldq + h * ds, a.ldq, row, F, ds, a.vec & 1, hf, qr);
    st_load_rows<NB>(a.dctx + b * F * dctx + h * ds, dctx, row, F, ds, a.vec & 8, hf, cr);
    // delta[row] = sum_c ctx[row][c] dctx[row][c]: the diagonal of ctx . dctx^T, summed as dP's elements are
    float delta;
    {
      float xr[16 * NB];
      st_load_rows<NB>(a.ctx_in + b * F * dctx + h * ds, dctx, row, F, ds, a.vec & 16, hf, xr);
      st_f32x16 dg = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 16 * NB; ++t) dg = __builtin_amdgcn_mfma_f32_32x32x2f32(xr[t], cr[t], dg, 0, 0, 0);
      // C[m][col] with m == col sits in the half-wave (col >> 2) & 1, register (col & 3) + 4 (col >> 3)
      const int isel = (col & 3) + 4 * (col >> 3);
      float d = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) d = i == isel ? dg[i] : d;
      d = hf == ((col >> 2) & 1) ? d : 0.f;
      delta = d + __shfl_xor(d, 32, kWave);  // (one of the two is 0)
    }
    const float lse = row < F ? a.lse[u * F + row] : 0.f;
    if (row < F && hf == 0) a.delta[u * F + row] = delta;
    const int32_t* mrow = a.mask != nullptr ? a.mask + b * T : nullptr;
    const float top = st_mask_top(tid, nthr, mrow, T, red);
    const float* kp = a.k + b * T * a.ldk + h * ds;
    const float* vp = a.v + b * T * a.ldv + h * ds;
    st_f32x16 o[NB];
    st_zero<NB>(o);
    for (int j0 = 0; j0 < T; j0 += KT) {
      st_stage<NB>(tid, nthr, kp, a.ldk, j0, T, ds, a.vec & 2, Ks);
      st_stage<NB>(tid, nthr, vp, a.ldv, j0, T, ds, a.vec & 4, Vs);
      for (int j = tid; j < KT; j += nthr) adds[j] = st_adder(mrow, j0 + j, T, top);
      __syncthreads();
      for (int js = 0; js < KT && j0 + js < T; js += 32) {
        const st_f32x16 s = st_mm_t<NB>(Ks, js, col, hf, qr);
        const st_f32x16 dp = st_mm_t<NB>(Vs, js, col, hf, cr);
        float g[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float p = expf(s[i] * a.scale + adds[js + (i & 3) + 8 * (i >> 2) + 4 * hf] - lse);
          g[i] = p * (dp[i] - delta) * a.scale;
        }
        st_mm_acc<NB>(Ks, js, col, hf, g, o);
      }
      __syncthreads();
    }
    if (row < F) st_store_t<NB>(o, 1.0f, a.dq + (b * F + row) * a.lddq + h * ds, ds, a.vec & 32, hf);
  }
}

// ------------------------------------------------------------------------------- backward (b): dK and dV
template <int NB>
__global__ __launch_bounds__(kStMaxThreads) void attn_stream_bwd_dkv_kernel(StArgs a) {
  constexpr int P = StGeom<NB>::P, KT = StGeom<NB>::KT;
  __shared__ float Qs[KT * P], Cs[KT * P], lses[KT], dels[KT], red[4];
  const int tid = threadIdx.x, nthr = blockDim.x, wave = tid / kWave;
  const int col = tid & 31, hf = (tid >> 5) & 1;
  const int F = a.F, T = a.T, H = a.H, ds = a.ds;
  const int wg_keys = 32 * (nthr / kWave);
  const int64_t kblocks = (T + wg_keys - 1) / wg_keys, items = a.units * kblocks;
  const int64_t dctx = static_cast<int64_t>(H) * ds;
  for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {
    const int64_t u = w / kblocks, b = u / H;
    const int h = static_cast<int>(u - b * H);
    const int key = static_cast<int>(w - u * kblocks) * wg_keys + 32 * wave + col;
    float kr[16 * NB], vr[16 * NB];
    st_load_rows<NB>(a.k + b * T * a.ldk + h * ds, a.ldk, key, T, ds, a.vec & 2, hf, kr);
    st_load_rows<NB>(a.v + b * T * a.ldv + h * ds, a.ldv, key, T, ds, a.vec & 4, hf, vr);
    const int32_t* mrow = a.mask != nullptr ? a.mask + b * T : nullptr;
    const float top = st_mask_top(tid, nthr, mrow, T, red);
    const float add = st_adder(mrow, key < T ? key : 0, T, top);  // (a key past the end is computed and never stored)
    const float* qp = a.q + b * F * a.ldq + h * ds;
    const float* cp = a.dctx + b * F * dctx + h * ds;
    st_f32x16 ok[NB], ov[NB];
    st_zero<NB>(ok);
    st_zero<NB>(ov);
    for (int i0 = 0; i0 < F; i0 += KT) {
      st_stage<NB>(tid, nthr, qp, a.ldq, i0, F, ds, a.vec & 1, Qs);
      st_stage<NB>(tid, nthr, cp, dctx, i0, F, ds, a.vec & 8, Cs);
      for (int r = tid; r < KT; r += nthr) {
        const bool on = i0 + r < F;
        lses[r] = on ? a.lse[u * F + i0 + r] : INFINITY;  // (a row past the end: exp(-inf) = 0)
        dels[r] = on ? a.delta[u * F + i0 + r] : 0.f;
      }
      __syncthreads();
      for (int is = 0; is < KT && i0 + is < F; is += 32) {
        // S[query][key] = Q_tile K^T, dP[query][key] = dctx_tile V^T: the products of launch (a), commuted
        const st_f32x16 s = st_mm_t<NB>(Qs, is, col, hf, kr);
        const st_f32x16 dp = st_mm_t<NB>(Cs, is, col, hf, vr);
        float p[16], g[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int r = is + (i & 3) + 8 * (i >> 2) + 4 * hf;
          p[i] = expf(s[i] * a.scale + add - lses[r]);
          g[i] = p[i] * (dp[i] - dels[r]) * a.scale;
        }
        st_mm_acc<NB>(Cs, is, col, hf, p, ov);
        st_mm_acc<NB>(Qs, is, col, hf, g, ok);
      }
      __syncthreads();
    }
    if (key < T) {
      st_store_t<NB>(ok, 1.0f, a.dk + (b * T + key) * a.lddk + h * ds, ds, a.vec & 64, hf);
      st_store_t<NB>(ov, 1.0f, a.dv + (b * T + key) * a.lddv + h * ds, ds, a.vec & 128, hf);
    }
  }
}

inline bool st_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// workgroups of a pass: 0 forward, 1 backward (a), 2 backward (b)
inline int64_t st_items(int64_t B, int F, int T, int H, int pass) {
  const int rows = pass == 2 ? T : F, per = 32 * st_waves(rows);
  return B * H * ((rows + per - 1) / per);
}

template <int NB>
static void st_launch(int pass, const StArgs& a, int64_t B, hipStream_t s) {
  const int64_t items = st_items(B, a.F, a.T, a.H, pass);
  const dim3 grid(static_cast<unsigned>(items < kStMaxGrid ? items : kStMaxGrid));
  const dim3 block(kWave * st_waves(pass == 2 ? a.T : a.F));
  if (pass == 0)
    hipLaunchKernelGGL(attn_stream_fwd_kernel<NB>, grid, block, 0, s, a);
  else if (pass == 1)
    hipLaunchKernelGGL(attn_stream_bwd_dq_kernel<NB>, grid, block, 0, s, a);
  else
    hipLaunchKernelGGL(attn_stream_bwd_dkv_kernel<NB>, grid, block, 0, s, a);
}

static void st_launch_nb(int pass, const StArgs& a, int64_t B, hipStream_t s) {
  switch (st_blocks(a.ds)) {
    case 1: st_launch<1>(pass, a, B, s); break;
    case 2: st_launch<2>(pass, a, B, s); break;
    case 3: st_launch<3>(pass, a, B, s); break;
    default: st_launch<4>(pass, a, B, s); break;
  }
}

}  // namespace er

extern "C" {

int64_t er_mha_stream_lds_bytes(int32_t ds, int bwd) {
  if (ds < 1 || ds > er::kStMaxDs) return 0;
  // two tiles, the four partial maxima, and the keys' adders (forward, launch (a)) or lse and delta (launch (b))
  const int64_t kt = er::st_tile(ds), p = 32 * er::st_blocks(ds) + 1;
  return 4 * (2 * kt * p + (bwd ? 2 : 1) * kt + 4);
}

int32_t er_mha_stream_grid(int64_t B, int32_t F, int32_t T, int32_t H, int32_t ds, int32_t pass) {
  if (B < 1 || !er::st_shape_ok(F, T, H, ds) || pass < 0 || pass > 2) return 0;
  const int64_t items = er::st_items(B, F, T, H, pass);
  return static_cast<int32_t>(items < er::kStMaxGrid ? items : er::kStMaxGrid);
}

static int mha_stream_fill(const char* what, er::StArgs* a, const float* q, int64_t ldq, const float* k, int64_t ldk,
                           const float* v, int64_t ldv, const int32_t* to_mask, int64_t B, int32_t F, int32_t T, int32_t H,
                           int32_t ds) {
  ER_REQUIRE(q && k && v && B > 0, "%s: bad arguments", what);
  ER_REQUIRE(er::st_shape_ok(F, T, H, ds), "%s: F = %d, T = %d, H = %d, ds = %d outside the envelope", what, F, T, H, ds);
  const int64_t d = static_cast<int64_t>(H) * ds;
  ER_REQUIRE(ldq >= d && ldk >= d && ldv >= d, "%s: a row pitch is below H * ds = %lld", what, static_cast<long long>(d));
  a->q = q;
  a->k = k;
  a->v = v;
  a->mask = to_mask;
  a->ldq = ldq;
  a->ldk = ldk;
  a->ldv = ldv;
  a->units = B * H;
  a->F = F;
  a->T = T;
  a->H = H;
  a->ds = ds;
  a->scale = static_cast<float>(1.0 / sqrt(static_cast<double>(ds)));
  if (ds % 4 == 0) {
    if (ldq % 4 == 0 && er::st_aligned16(q)) a->vec |= 1;
    if (ldk % 4 == 0 && er::st_aligned16(k)) a->vec |= 2;
    if (ldv % 4 == 0 && er::st_aligned16(v)) a->vec |= 4;
  }
  return 0;
}

int er_mha_stream_fwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                      const int32_t* to_mask, int64_t B, int32_t F, int32_t T, int32_t H, int32_t ds, float* ctx,
                      float* lse, er_stream_t stream) {
  er::StArgs a = {};
  if (int rc = mha_stream_fill("er_mha_stream_fwd", &a, q, ldq, k, ldk, v, ldv, to_mask, B, F, T, H, ds)) return rc;
  ER_REQUIRE(ctx && lse, "er_mha_stream_fwd: bad arguments");
  a.ctx = ctx;
  a.lse = lse;
  if (ds % 4 == 0 && er::st_aligned16(ctx)) a.vec |= 16;  // (its pitch H * ds is a multiple of 4 with ds)
  er::st_launch_nb(0, a, B, er::as_stream(stream));
  ER_LAUNCH_CHECK();
  return 0;
}

int er_mha_stream_bwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                      const int32_t* to_mask, const float* dctx, const float* ctx, const float* lse, int64_t B, int32_t F,
                      int32_t T, int32_t H, int32_t ds, float* delta, float* dq, int64_t lddq, float* dk, int64_t lddk,
                      float* dv, int64_t lddv, er_stream_t stream) {
  er::StArgs a = {};
  if (int rc = mha_stream_fill("er_mha_stream_bwd", &a, q, ldq, k, ldk, v, ldv, to_mask, B, F, T, H, ds)) return rc;
  ER_REQUIRE(dctx && ctx && lse && delta && dq && dk && dv, "er_mha_stream_bwd: bad arguments");
  const int64_t d = static_cast<int64_t>(H) * ds;
  ER_REQUIRE(lddq >= d && lddk >= d && lddv >= d, "er_mha_stream_bwd: a row pitch is below H * ds = %lld",
             static_cast<long long>(d));
  a.dctx = dctx;
  a.ctx_in = ctx;
  a.lse = const_cast<float*>(lse);  // (read only by both launches)
  a.delta = delta;
  a.dq = dq;
  a.dk = dk;
  a.dv = dv;
  a.lddq = lddq;
  a.lddk = lddk;
  a.lddv = lddv;
  if (ds % 4 == 0) {
    if (er::st_aligned16(dctx)) a.vec |= 8;
    if (er::st_aligned16(ctx)) a.vec |= 16;
    if (lddq % 4 == 0 && er::st_aligned16(dq)) a.vec |= 32;
    if (lddk % 4 == 0 && er::st_aligned16(dk)) a.vec |= 64;
    if (lddv % 4 == 0 && er::st_aligned16(dv)) a.vec |= 128;
  }
  const hipStream_t s = er::as_stream(stream);
  er::st_launch_nb(1, a, B, s);
  ER_LAUNCH_CHECK();
  er::st_launch_nb(2, a, B, s);
  ER_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
