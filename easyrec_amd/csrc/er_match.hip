// K8f: the head of the two-tower retrieval models (reference model/match_model.py, model/dssm.py): L2 normalisation of
// the tower outputs, and the list-wise in-batch softmax (scale, in-batch mask, softmax, diagonal gather, both losses and
// the whole backward) without the [B, M] logit matrix ever reaching HBM.
//
// Layout of the streaming kernels: a workgroup of 256 threads owns kTA = 32 STATIONARY rows (users; items in the
// backward's column pass) staged once in LDS, and streams tiles of kTB = 64 rows of the other side through LDS.  Rows sit
// at the odd pitch DP + 1, DP = 8 * NK >= D (NK = 4, 8, 16: D <= 32, 64, 128), columns D .. DP - 1 zero.
//   product phase: thread (rg = t / 16, cg = t % 16) holds the 2 x 4 similarities of stationary rows 2 rg, 2 rg + 1 and
//     streamed rows cg, cg + 16, cg + 32, cg + 48; the 16 threads of a stationary row pair are one DPP row.
//   forward: every thread keeps an online (maximum, sum) of its own columns; the 16 are merged once, after the last tile.
//   backward: the tile of d(loss)/d(similarity) goes through LDS ([32, 64] at pitch 65) and thread (r = t / 8,
//     dg = t % 8) adds its row of it times the streamed tile into NK register accumulators (columns dg + 8 k).
// The row pass (stationary users) gives dU and the two scalars' partial sums; the column pass (stationary items) gives
// dI.  Nothing is accumulated with atomics: every output element has one owner thread and one summation order, so two
// runs and a graph replay give the same bits.  fp32 throughout.
#include "er_common.h"

namespace er {

constexpr int kTA = 32;
constexpr int kTB = 64;
constexpr int kDzPitch = kTB + 1;
constexpr int kMatchMaxD = 128;
constexpr float kMaskValue = 1e32f;
constexpr float kNoMax = -3.0e38f;  // below every logit, the mask value included; finite, so that m - m is 0

__host__ __device__ inline int match_nk(int D) { return D <= 32 ? 4 : (D <= 64 ? 8 : 16); }

// LDS bytes of a backward workgroup, the largest of the streaming kernels: both tiles, the gradient tile, the per-row
// statistics (4 x 64 floats) and the ids of both tiles (96 int64).  The forward has no gradient tile; the rank counts keep
// a 4 KB count array in its place.
inline int64_t match_lds_bytes(int D) {
  if (D < 1 || D > kMatchMaxD) return 0;
  const int ldd = match_nk(D) * 8 + 1;
  return 4 * (static_cast<int64_t>(kTA + kTB) * ldd + kTA * kDzPitch + 4 * kTB) + 8 * (kTA + kTB);
}

template <int G>
__device__ __forceinline__ float group_max(float v) {
  if (G >= 2) v = fmaxf(v, dpp_move<0xB1>(v));
  if (G >= 4) v = fmaxf(v, dpp_move<0x4E>(v));
  if (G >= 8) v = fmaxf(v, dpp_move<0x141>(v));
  if (G >= 16) v = fmaxf(v, dpp_move<0x140>(v));
  return v;
}

struct MatchArgs {
  const float* U;         // [B, D]
  const float* I;         // [M, D]
  const float* sim_w;     // [1] or null
  const float* sim_b;     // [1] or null
  const int64_t* ids;     // [M] or null
  const float* weight;    // [B] or null
  int64_t B, M;
  int D, ignore;
  float inv_t;
};

// rows [r0, r0 + nrows) of src [n, D] -> tile (pitch LDD), rows past n zero
template <int LDD>
__device__ __forceinline__ void stage_rows(const float* __restrict__ src, int64_t n, int64_t r0, int nrows, int D,
                                           float* tile) {
  for (int t = threadIdx.x; t < nrows * D; t += kBlock) {
    const int r = t / D, d = t - r * D;
    const int64_t row = r0 + r;
    tile[r * LDD + d] = row < n ? src[row * D + d] : 0.f;
  }
}

template <int LDD>
__device__ __forceinline__ void zero_pad(float* tile, int nrows, int D) {
  const int pad = LDD - D;
  for (int t = threadIdx.x; t < nrows * pad; t += kBlock) {
    const int r = t / pad;
    tile[r * LDD + D + (t - r * pad)] = 0.f;
  }
}

__device__ __forceinline__ void stage_ids(const int64_t* __restrict__ ids, int64_t B, int64_t r0, int nrows,
                                          int64_t* dst) {
  // (only in-batch columns are ever compared: rows >= B get no id)
  for (int t = threadIdx.x; t < nrows; t += kBlock) dst[t] = (ids && r0 + t < B) ? ids[r0 + t] : 0;
}

// the 2 x 4 similarities of this thread
template <int LDD>
__device__ __forceinline__ void tile_products(const float* As, const float* Bs, int D, int rg, int cg, float s[2][4]) {
  const float* a0 = As + (2 * rg) * LDD;
  const float* a1 = a0 + LDD;
  const float* b = Bs + cg * LDD;
#pragma unroll
  for (int c = 0; c < 4; ++c) s[0][c] = s[1][c] = 0.f;
  for (int d = 0; d < D; ++d) {
    const float x0 = a0[d], x1 = a1[d];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float y = b[c * 16 * LDD + d];
      s[0][c] = fmaf(x0, y, s[0][c]);
      s[1][c] = fmaf(x1, y, s[1][c]);
    }
  }
}

// the in-batch mask of match_model.py:50-69 for the pair (user i, item j), ids already looked up
__device__ __forceinline__ bool masked(int64_t i, int64_t j, int64_t B, int ignore, bool has_ids, int64_t id_i,
                                       int64_t id_j) {
  if (j >= B || j == i) return false;
  return ignore ? true : (has_ids && id_i == id_j);
}

__device__ __forceinline__ float logit_of(float s, float inv_t, float aw, float bb) { return (s * inv_t) * aw + bb; }

// ------------------------------------------------------------------------------------------------ forward
// COUNT = false: row maximum, row sum, diagonal logit, hit probability and the workgroup's three loss partial sums.
// COUNT = true: er_match_rank_counts.
template <int NK, bool COUNT>
__global__ __launch_bounds__(kBlock) void match_fwd_kernel(MatchArgs a, float* __restrict__ row_max,
                                                           float* __restrict__ row_sum, float* __restrict__ zdiag,
                                                           float* __restrict__ hit, float* __restrict__ partials,
                                                           int32_t* __restrict__ c_in, int32_t* __restrict__ c_neg) {
  constexpr int LDD = NK * 8 + 1;
  __shared__ float As[kTA * LDD];
  __shared__ float Bs[kTB * LDD];
  __shared__ float st[4 * kTB];        // per stationary row: maximum, sum, diagonal logit, diagonal similarity
  __shared__ int64_t idA[kTA], idB[kTB];
  __shared__ int cnt[COUNT ? 2 * kTA * 16 : 1];
  const int D = a.D, rg = threadIdx.x >> 4, cg = threadIdx.x & 15;
  const int64_t B = a.B, M = a.M, a0 = static_cast<int64_t>(blockIdx.x) * kTA;
  const float aw = a.sim_w ? fabsf(a.sim_w[0]) : 1.f, bb = a.sim_b ? a.sim_b[0] : 0.f;
  const bool has_ids = a.ids != nullptr;
  zero_pad<LDD>(As, kTA, D);
  zero_pad<LDD>(Bs, kTB, D);
  stage_rows<LDD>(a.U, B, a0, kTA, D, As);
  stage_ids(a.ids, B, a0, kTA, idA);
  float m[2] = {kNoMax, kNoMax}, l[2] = {0.f, 0.f};
  int n_in[2] = {0, 0}, n_neg[2] = {0, 0};
  float zd[2] = {0.f, 0.f};
  if (COUNT) {
    // the diagonal logits first: row a0 + r against item a0 + r (B <= M, so the item exists)
    __syncthreads();
    stage_rows<LDD>(a.I, M, a0, kTA, D, Bs);
    __syncthreads();
    if (threadIdx.x < kTA) {
      float s = 0.f;
      for (int d = 0; d < D; ++d) s = fmaf(As[threadIdx.x * LDD + d], Bs[threadIdx.x * LDD + d], s);
      st[2 * kTB + threadIdx.x] = logit_of(s, a.inv_t, aw, bb);
    }
    __syncthreads();
    zd[0] = st[2 * kTB + 2 * rg];
    zd[1] = st[2 * kTB + 2 * rg + 1];
  }
  for (int64_t b0 = 0; b0 < M; b0 += kTB) {
    __syncthreads();  // (the previous tile's readers; the stationary tile on the first round)
    stage_rows<LDD>(a.I, M, b0, kTB, D, Bs);
    stage_ids(a.ids, B, b0, kTB, idB);
    __syncthreads();
    float s[2][4];
    tile_products<LDD>(As, Bs, D, rg, cg, s);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int ia = 2 * rg + r;
      const int64_t i = a0 + ia;
      float z[4];
      float tmax = kNoMax;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int ib = cg + 16 * c;
        const int64_t j = b0 + ib;
        float v = logit_of(s[r][c], a.inv_t, aw, bb);
        const bool live = i < B && j < M;
        const bool mk = masked(i, j, B, a.ignore, has_ids, idA[ia], idB[ib]);
        if (mk) v = v - kMaskValue;
        if (COUNT) {
          if (live && j != i) {
            const bool above = v > zd[r] || (v == zd[r] && j < i);
            if (j < B) n_in[r] += above; else n_neg[r] += v > zd[r];
          }
        } else {
          // a masked entry takes no part: it contributes exactly 0 to the row sum whatever the running maximum is
          z[c] = (live && !mk) ? v : kNoMax;
          tmax = fmaxf(tmax, z[c]);
          if (live && j == i) {
            st[2 * kTB + ia] = v;
            st[3 * kTB + ia] = s[r][c];
          }
        }
      }
      if (!COUNT && tmax > kNoMax) {
        if (tmax > m[r]) {
          l[r] *= expf(m[r] - tmax);
          m[r] = tmax;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (z[c] > kNoMax) l[r] += expf(z[c] - m[r]);
      }
    }
  }
  if (COUNT) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      cnt[(2 * rg + r) * 16 + cg] = n_in[r];
      cnt[(kTA + 2 * rg + r) * 16 + cg] = n_neg[r];
    }
    __syncthreads();
    if (threadIdx.x < kTA && a0 + threadIdx.x < B) {
      int s_in = 0, s_neg = 0;
      for (int k = 0; k < 16; ++k) {
        s_in += cnt[threadIdx.x * 16 + k];
        s_neg += cnt[(kTA + threadIdx.x) * 16 + k];
      }
      c_in[a0 + threadIdx.x] = s_in;
      c_neg[a0 + threadIdx.x] = s_neg;
    }
    return;
  }
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const float mx = group_max<16>(m[r]);
    const float sum = group_sum<16>(l[r] * expf(m[r] - mx));
    if (cg == 0) {
      st[2 * rg + r] = mx;
      st[kTB + 2 * rg + r] = sum;
    }
  }
  __syncthreads();
  // the rows' statistics and the three loss terms; thread 0 adds the 32 rows in order
  float* term = Bs;  // (free now) [3, kTA]
  if (threadIdx.x < kTA) {
    const int64_t i = a0 + threadIdx.x;
    float t0 = 0.f, t1 = 0.f, t2 = 0.f;
    if (i < B) {
      const float mx = st[threadIdx.x], sum = st[kTB + threadIdx.x], z = st[2 * kTB + threadIdx.x];
      const float pos = st[3 * kTB + threadIdx.x];
      const float h = expf(z - mx) / sum;
      const float w = a.weight ? a.weight[i] : 1.f;
      row_max[i] = mx;
      row_sum[i] = sum;
      zdiag[i] = z;
      hit[i] = h;
      t0 = w * logf(h + 1e-12f);
      t1 = w * fmaxf(-pos, 0.f);
      t2 = w;
    }
    term[threadIdx.x] = t0;
    term[kTA + threadIdx.x] = t1;
    term[2 * kTA + threadIdx.x] = t2;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    float acc = 0.f;
    for (int k = 0; k < kTA; ++k) acc += term[threadIdx.x * kTA + k];
    partials[static_cast<int64_t>(blockIdx.x) * 3 + threadIdx.x] = acc;
  }
}

// losses [3] = cross_entropy_loss, reg_pos_loss, sum of the weights: thread c adds column c of partials [rows, 3] over
// 64-row strides (lane r rows r, r + 64, ..), then the 64 lanes' sums in order
__global__ __launch_bounds__(kBlock) void match_loss_finish_kernel(const float* __restrict__ partials, int rows,
                                                                  float* __restrict__ losses) {
  __shared__ float sums[3 * 64];
  if (threadIdx.x < 3 * 64) {
    const int c = threadIdx.x / 64, lane = threadIdx.x % 64;
    float acc = 0.f;
    for (int r = lane; r < rows; r += 64) acc += partials[static_cast<int64_t>(r) * 3 + c];
    sums[threadIdx.x] = acc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float t[3];
    for (int c = 0; c < 3; ++c) {
      float acc = 0.f;
      for (int k = 0; k < 64; ++k) acc += sums[c * 64 + k];
      t[c] = acc;
    }
    losses[0] = -t[0] / t[2];
    losses[1] = t[1] / t[2];
    losses[2] = t[2];
  }
}

// ------------------------------------------------------------------------------------------------ backward
// COLS = false: stationary users [a0, a0 + 32), streamed items: out = dU, and the workgroup's partial sums of
//   (dsim_w, dsim_b) into partials [grid, 2].
// COLS = true: stationary items, streamed users: out = dI.
struct MatchBwdArgs {
  const float* row_max;
  const float* row_sum;
  const float* hit;
  const float* losses;  // [3]: the third entry is the sum of the weights
  const float* g_ce;    // [1]: upstream gradient of cross_entropy_loss
  const float* g_reg;   // [1]: of reg_pos_loss
};

template <int NK, bool COLS>
__global__ __launch_bounds__(kBlock) void match_bwd_kernel(MatchArgs a, MatchBwdArgs g, float* __restrict__ out,
                                                           float* __restrict__ partials) {
  constexpr int LDD = NK * 8 + 1;
  __shared__ float As[kTA * LDD];
  __shared__ float Bs[kTB * LDD];
  __shared__ float dzs[kTA * kDzPitch];
  __shared__ float st[4 * kTB];  // per user of the tile: row maximum, 1 / row sum, g_i, c_i (the reg_pos_loss term)
  __shared__ int64_t idA[kTA], idB[kTB];
  const int D = a.D, rg = threadIdx.x >> 4, cg = threadIdx.x & 15;
  const int64_t B = a.B, M = a.M, a0 = static_cast<int64_t>(blockIdx.x) * kTA;
  const float sw = a.sim_w ? a.sim_w[0] : 1.f;
  const float aw = fabsf(sw), bb = a.sim_b ? a.sim_b[0] : 0.f;
  const float scale = a.inv_t * aw;  // d(logit) / d(similarity)
  const bool has_ids = a.ids != nullptr;
  const float inv_w = 1.f / g.losses[2], g_ce = g.g_ce[0], g_reg = g.g_reg[0];
  const float* Asrc = COLS ? a.I : a.U;
  const float* Bsrc = COLS ? a.U : a.I;
  const int64_t nA = COLS ? M : B, nB = COLS ? B : M;
  constexpr int kUsers = COLS ? kTB : kTA;  // users per tile
  auto stage_users = [&](int64_t u0) {
    for (int t = threadIdx.x; t < kUsers; t += kBlock) {
      const int64_t i = u0 + t;
      float mx = 0.f, il = 0.f, gi = 0.f, ci = 0.f;
      if (i < B) {
        const float w = (a.weight ? a.weight[i] : 1.f) * inv_w, h = g.hit[i];
        mx = g.row_max[i];
        il = 1.f / g.row_sum[i];
        gi = w * (h / (h + 1e-12f)) * g_ce;
        ci = -w * g_reg;
      }
      st[t] = mx;
      st[kTB + t] = il;
      st[2 * kTB + t] = gi;
      st[3 * kTB + t] = ci;
    }
  };
  zero_pad<LDD>(As, kTA, D);
  zero_pad<LDD>(Bs, kTB, D);
  stage_rows<LDD>(Asrc, nA, a0, kTA, D, As);
  stage_ids(a.ids, B, a0, kTA, idA);
  if (!COLS) stage_users(a0);
  float acc[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) acc[k] = 0.f;
  float sum_w = 0.f, sum_b = 0.f;
  const int r2 = threadIdx.x >> 3, dg = threadIdx.x & 7;
  for (int64_t b0 = 0; b0 < nB; b0 += kTB) {
    __syncthreads();
    stage_rows<LDD>(Bsrc, nB, b0, kTB, D, Bs);
    stage_ids(a.ids, B, b0, kTB, idB);
    if (COLS) stage_users(b0);
    __syncthreads();
    float s[2][4];
    tile_products<LDD>(As, Bs, D, rg, cg, s);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int ia = 2 * rg + r;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int ib = cg + 16 * c;
        const int64_t i = COLS ? b0 + ib : a0 + ia;
        const int64_t j = COLS ? a0 + ia : b0 + ib;
        const int u = COLS ? ib : ia;
        float ds = 0.f;
        if (i < B && j < M) {
          const bool mk = masked(i, j, B, a.ignore, has_ids, COLS ? idB[ib] : idA[ia], COLS ? idA[ia] : idB[ib]);
          const float z = logit_of(s[r][c], a.inv_t, aw, bb);
          const float p = mk ? 0.f : expf(z - st[u]) * st[kTB + u];
          const float dz = st[2 * kTB + u] * (p - (i == j ? 1.f : 0.f));
          ds = scale * dz;
          if (i == j && s[r][c] < 0.f) ds += st[3 * kTB + u];
          if (!COLS) {
            sum_w = fmaf(dz, s[r][c], sum_w);
            sum_b += dz;
          }
        }
        dzs[ia * kDzPitch + ib] = ds;
      }
    }
    __syncthreads();
    const float* drow = dzs + r2 * kDzPitch;
    for (int jb = 0; jb < kTB; ++jb) {
      const float v = drow[jb];
      const float* brow = Bs + jb * LDD + dg;
#pragma unroll
      for (int k = 0; k < NK; ++k) acc[k] = fmaf(v, brow[8 * k], acc[k]);
    }
  }
  if (a0 + r2 < nA) {
    float* orow = out + (a0 + r2) * D;
#pragma unroll
    for (int k = 0; k < NK; ++k)
      if (dg + 8 * k < D) orow[dg + 8 * k] = acc[k];
  }
  if (!COLS) {
    // (dsim_w, dsim_b) of this workgroup: the waves' sums, then the four waves in order
    __syncthreads();
    sum_w = wave_sum(sum_w);
    sum_b = wave_sum(sum_b);
    if ((threadIdx.x & 63) == 0) {
      dzs[threadIdx.x >> 6] = sum_w;
      dzs[4 + (threadIdx.x >> 6)] = sum_b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const float sign = sw > 0.f ? 1.f : (sw < 0.f ? -1.f : 0.f);
      partials[2 * static_cast<int64_t>(blockIdx.x)] = sign * a.inv_t * ((dzs[0] + dzs[1]) + (dzs[2] + dzs[3]));
      partials[2 * static_cast<int64_t>(blockIdx.x) + 1] = (dzs[4] + dzs[5]) + (dzs[6] + dzs[7]);
    }
  }
}

// ------------------------------------------------------------------------------------------------ normalisation
// one wave per row: y = x * rsqrt(max(sum x^2, 1e-12))
__global__ __launch_bounds__(kBlock) void match_normalize_fwd_kernel(const float* __restrict__ x, int64_t R, int D,
                                                                    float* __restrict__ y, float* __restrict__ inv) {
  const int64_t row = static_cast<int64_t>(blockIdx.x) * (kBlock / kWave) + (threadIdx.x >> 6);
  if (row >= R) return;
  const int lane = threadIdx.x & 63;
  const float* xr = x + row * D;
  float ss = 0.f;
  for (int d = lane; d < D; d += kWave) ss = fmaf(xr[d], xr[d], ss);
  ss = wave_sum(ss);
  const float r = 1.f / sqrtf(fmaxf(ss, 1e-12f));
  for (int d = lane; d < D; d += kWave) y[row * D + d] = xr[d] * r;
  if (lane == 0) inv[row] = r;
}

// dx = inv * dy - inv^3 * (x . dy) * x; under the floor (sum x^2 < 1e-12) the factor is a constant: dx = inv * dy
__global__ __launch_bounds__(kBlock) void match_normalize_bwd_kernel(const float* __restrict__ x,
                                                                    const float* __restrict__ inv,
                                                                    const float* __restrict__ dy, int64_t R, int D,
                                                                    float* __restrict__ dx) {
  const int64_t row = static_cast<int64_t>(blockIdx.x) * (kBlock / kWave) + (threadIdx.x >> 6);
  if (row >= R) return;
  const int lane = threadIdx.x & 63;
  const float* xr = x + row * D;
  const float* dr = dy + row * D;
  float ss = 0.f, xd = 0.f;
  for (int d = lane; d < D; d += kWave) {
    ss = fmaf(xr[d], xr[d], ss);
    xd = fmaf(xr[d], dr[d], xd);
  }
  ss = wave_sum(ss);
  xd = wave_sum(xd);
  const float r = inv[row];
  const float k = ss < 1e-12f ? 0.f : r * r * r * xd;
  for (int d = lane; d < D; d += kWave) dx[row * D + d] = r * dr[d] - k * xr[d];
}

inline MatchArgs match_args(const float* U, const float* I, int64_t B, int64_t M, int32_t D, float inv_t,
                            const float* sim_w, const float* sim_b, const int64_t* ids, int ignore,
                            const float* weight) {
  MatchArgs a;
  a.U = U;
  a.I = I;
  a.sim_w = sim_w;
  a.sim_b = sim_b;
  a.ids = ids;
  a.weight = weight;
  a.B = B;
  a.M = M;
  a.D = D;
  a.ignore = ignore;
  a.inv_t = inv_t;
  return a;
}

inline const char* match_shape_error(const void* U, const void* I, int64_t B, int64_t M, int32_t D) {
  if (!U || !I) return "null operand";
  if (B < 1 || M < B) return "needs 1 <= B <= M";
  if (D < 1 || D > kMatchMaxD) return "D outside 1 .. 128";
  if ((M + kTA - 1) / kTA > 0x7fffffff) return "too many rows for one grid";
  return nullptr;
}

}  // namespace er

extern "C" {

int64_t er_match_lds_bytes(int32_t D) { return er::match_lds_bytes(D); }

int32_t er_match_grid(int64_t rows) { return static_cast<int32_t>(er::ceil_div(rows, er::kTA)); }

int er_match_normalize_fwd(const float* x, int64_t R, int32_t D, float* y, float* inv_norm, er_stream_t stream) {
  ER_REQUIRE(x && y && inv_norm && R >= 1 && D >= 1, "er_match_normalize_fwd: bad arguments");
  const int64_t grid = er::ceil_div(R, er::kBlock / er::kWave);
  ER_REQUIRE(grid <= 0x7fffffff, "er_match_normalize_fwd: %lld rows are too many", static_cast<long long>(R));
  hipLaunchKernelGGL(er::match_normalize_fwd_kernel, dim3(static_cast<unsigned>(grid)), dim3(er::kBlock), 0,
                     er::as_stream(stream), x, R, D, y, inv_norm);
  ER_LAUNCH_CHECK();
  return 0;
}

int er_match_normalize_bwd(const float* x, const float* inv_norm, const float* dy, int64_t R, int32_t D, float* dx,
                           er_stream_t stream) {
  ER_REQUIRE(x && inv_norm && dy && dx && R >= 1 && D >= 1, "er_match_normalize_bwd: bad arguments");
  const int64_t grid = er::ceil_div(R, er::kBlock / er::kWave);
  ER_REQUIRE(grid <= 0x7fffffff, "er_match_normalize_bwd: %lld rows are too many", static_cast<long long>(R));
  hipLaunchKernelGGL(er::match_normalize_bwd_kernel, dim3(static_cast<unsigned>(grid)), dim3(er::kBlock), 0,
                     er::as_stream(stream), x, inv_norm, dy, R, D, dx);
  ER_LAUNCH_CHECK();
  return 0;
}

#define ER_MATCH_BY_NK(D, LAUNCH)           \
  switch (er::match_nk(D)) {                \
    case 4: { constexpr int NK = 4; LAUNCH; break; }   \
    case 8: { constexpr int NK = 8; LAUNCH; break; }   \
    default: { constexpr int NK = 16; LAUNCH; break; } \
  }

int er_match_softmax_fwd(const float* U, const float* I, int64_t B, int64_t M, int32_t D, float inv_temperature,
                         const float* sim_w, const float* sim_b, const int64_t* item_ids, int ignore_in_batch,
                         const float* sample_weight, float* row_max, float* row_sum, float* zdiag, float* hit,
                         float* partials, float* losses, er_stream_t stream) {
  const char* err = er::match_shape_error(U, I, B, M, D);
  ER_REQUIRE(err == nullptr, "er_match_softmax_fwd: %s (B %lld, M %lld, D %d)", err, static_cast<long long>(B),
             static_cast<long long>(M), D);
  ER_REQUIRE(row_max && row_sum && zdiag && hit && partials && losses, "er_match_softmax_fwd: null output");
  ER_REQUIRE((sim_w == nullptr) == (sim_b == nullptr), "er_match_softmax_fwd: sim_w and sim_b come together");
  const er::MatchArgs a = er::match_args(U, I, B, M, D, inv_temperature, sim_w, sim_b, item_ids, ignore_in_batch,
                                         sample_weight);
  const unsigned grid = static_cast<unsigned>(er_match_grid(B));
  ER_MATCH_BY_NK(D, hipLaunchKernelGGL((er::match_fwd_kernel<NK, false>), dim3(grid), dim3(er::kBlock), 0,
                                       er::as_stream(stream), a, row_max, row_sum, zdiag, hit, partials,
                                       static_cast<int32_t*>(nullptr), static_cast<int32_t*>(nullptr)));
  ER_LAUNCH_CHECK();
  hipLaunchKernelGGL(er::match_loss_finish_kernel, dim3(1), dim3(er::kBlock), 0, er::as_stream(stream), partials,
                     static_cast<int>(grid), losses);
  ER_LAUNCH_CHECK();
  return 0;
}

int er_match_rank_counts(const float* U, const float* I, int64_t B, int64_t M, int32_t D, float inv_temperature,
                         const float* sim_w, const float* sim_b, const int64_t* item_ids, int ignore_in_batch,
                         int32_t* c_in, int32_t* c_neg, er_stream_t stream) {
  const char* err = er::match_shape_error(U, I, B, M, D);
  ER_REQUIRE(err == nullptr, "er_match_rank_counts: %s (B %lld, M %lld, D %d)", err, static_cast<long long>(B),
             static_cast<long long>(M), D);
  ER_REQUIRE(c_in && c_neg, "er_match_rank_counts: null output");
  ER_REQUIRE((sim_w == nullptr) == (sim_b == nullptr), "er_match_rank_counts: sim_w and sim_b come together");
  const er::MatchArgs a = er::match_args(U, I, B, M, D, inv_temperature, sim_w, sim_b, item_ids, ignore_in_batch,
                                         nullptr);
  const unsigned grid = static_cast<unsigned>(er_match_grid(B));
  float* none = nullptr;
  ER_MATCH_BY_NK(D, hipLaunchKernelGGL((er::match_fwd_kernel<NK, true>), dim3(grid), dim3(er::kBlock), 0,
                                       er::as_stream(stream), a, none, none, none, none, none, c_in, c_neg));
  ER_LAUNCH_CHECK();
  return 0;
}

int er_match_softmax_bwd(const float* U, const float* I, int64_t B, int64_t M, int32_t D, float inv_temperature,
                         const float* sim_w, const float* sim_b, const int64_t* item_ids, int ignore_in_batch,
                         const float* sample_weight, const float* row_max, const float* row_sum, const float* hit,
                         const float* losses, const float* g_ce, const float* g_reg, float* dU, float* dI,
                         float* partials, er_stream_t stream) {
  const char* err = er::match_shape_error(U, I, B, M, D);
  ER_REQUIRE(err == nullptr, "er_match_softmax_bwd: %s (B %lld, M %lld, D %d)", err, static_cast<long long>(B),
             static_cast<long long>(M), D);
  ER_REQUIRE(row_max && row_sum && hit && losses && g_ce && g_reg && dU && dI && partials,
             "er_match_softmax_bwd: null argument");
  ER_REQUIRE((sim_w == nullptr) == (sim_b == nullptr), "er_match_softmax_bwd: sim_w and sim_b come together");
  const er::MatchArgs a = er::match_args(U, I, B, M, D, inv_temperature, sim_w, sim_b, item_ids, ignore_in_batch,
                                         sample_weight);
  er::MatchBwdArgs g;
  g.row_max = row_max;
  g.row_sum = row_sum;
  g.hit = hit;
  g.losses = losses;
  g.g_ce = g_ce;
  g.g_reg = g_reg;
  const unsigned grid_u = static_cast<unsigned>(er_match_grid(B)), grid_i = static_cast<unsigned>(er_match_grid(M));
  ER_MATCH_BY_NK(D, hipLaunchKernelGGL((er::match_bwd_kernel<NK, false>), dim3(grid_u), dim3(er::kBlock), 0,
                                       er::as_stream(stream), a, g, dU, partials));
  ER_LAUNCH_CHECK();
  ER_MATCH_BY_NK(D, hipLaunchKernelGGL((er::match_bwd_kernel<NK, true>), dim3(grid_i), dim3(er::kBlock), 0,
                                       er::as_stream(stream), a, g, dI, static_cast<float*>(nullptr)));
  ER_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
