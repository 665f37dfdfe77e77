// K8m: the session-keyed pairwise ranking losses of reference loss/pairwise_loss.py at ohem_ratio == 1 -
// pairwise_loss (deprecated), pairwise_logistic_loss, pairwise_hinge_loss and pairwise_focal_loss (through
// loss/focal_loss.py) - with d loss / d logits and the pair count, in O(B * column splits) memory.
//
// A pair is an ordered (i, j) with y_i > y_j, equal session keys (when given) and, for focal with a hinge margin,
// s_i - s_j < hinge_margin (s = z / T).  The reference gathers the pairs out of [B, B] tensors with a boolean mask; here
// the pair matrix is cut into tiles of 256 rows by a column chunk and never stored:
//
//   pair_kernel     grid (row blocks, column splits).  Thread t of row block r owns example i = 256 r + t and keeps
//                   (s_i, y_i, key_i, w_i) in registers.  The workgroup stages its chunk's (s, y, key, w) in LDS once; in the
//                   column loop every lane reads the SAME LDS word per column (a broadcast: no bank conflict).  y_i > y_j and
//                   y_j > y_i exclude each other, so a column costs ONE pair evaluation: the pair (i, j) adds w_i * loss to
//                   the thread's loss, 1 to its counts and w_i * dl/dd to its dz_i; the pair (j, i) subtracts w_j * dl/dd
//                   from its dz_i.  The thread so leaves the complete d / d s_i of its chunk: no transposed pass, no atomics.
//                   Columns in ascending order from 0.f; the workgroup's loss in block_sum_256's tree.
//   finish_kernel   ceil(B / 256) workgroups.  Each sums all the workgroups' counts itself (integers: no order to fix), then
//                   dz_i = scale * ((sum over the splits 0, 1, .. of the partials) / nz) / T; workgroup 0 also stores
//                   loss_partials[g] = scale * loss[g] / nz - the loss tail's launch sums them - and the pair count.
//
// There is no contraction in this (every pair goes through exp / log1p / a compare), so MFMA does not fit.  fp32, precise
// expf / log1pf / powf, vector stores only, every float sum in one fixed order: two runs and a graph replay give the same
// bits.
#include <math.h>

#include "er_common.h"
#include "er_listwise_sort.h"

namespace er {

constexpr int kPwMaxB = 8192;
constexpr int kPwMaxChunk = 1024;  // columns staged in LDS: 20 bytes each
constexpr int kPwMinChunk = 64;
constexpr int kPwFill = 256;       // the workgroups a launch aims at (one per CU)

struct PwGeom {
  int rb, splits, chunk;
};

// rb row blocks of 256 x `splits` column chunks of `chunk` columns (the last one ragged); chunk <= rb^2 <= 1024
inline PwGeom pw_geom(int64_t B) {
  PwGeom g = {0, 0, 0};
  if (B < 1 || B > kPwMaxB) return g;
  g.rb = static_cast<int>(ceil_div(B, kBlock));
  const int64_t fill = ceil_div(kPwFill, g.rb), most = ceil_div(B, kPwMinChunk);
  const int64_t want = fill < most ? fill : most;
  g.chunk = static_cast<int>(ceil_div(B, want));
  g.splits = static_cast<int>(ceil_div(B, g.chunk));
  return g;
}

struct PwParam {
  float temperature, label_div, margin, hinge_margin, gamma, alpha;
  int label_margin, has_hinge, has_alpha;
};

// tf.nn.sigmoid_cross_entropy_with_logits(labels = 1, logits = x) and its derivative -sigmoid(-x)
__device__ __forceinline__ void pw_softplus(float x, float* l, float* g) {
  const float e = expf(-fabsf(x));
  *l = fmaxf(x, 0.f) - x + log1pf(e);
  *g = -(x >= 0.f ? e / (1.f + e) : 1.f / (1.f + e));
}

// one pair of first member's score above: d = s_first - s_second, dy = y_first - y_second > 0 -> the pair's loss, d loss /
// d d and the weight-free factor that decides whether the pair counts as present; false: the pair is masked out
template <int KIND>
__device__ __forceinline__ bool pw_pair(const PwParam& p, float d, float dy, float* l, float* g, float* present) {
  *present = 1.f;
  if (KIND == ER_PAIR_WISE || KIND == ER_PAIR_LOGISTIC) {
    const float x = d - (p.label_margin ? dy : p.margin);
    pw_softplus(x, l, g);
    // pairwise_logistic_loss spells it relu(-x) + log1p(exp(-|x|)): relu and abs pass no gradient at x == 0
    if (KIND == ER_PAIR_LOGISTIC && x == 0.f) *g = 0.f;
    return true;
  }
  if (KIND == ER_PAIR_HINGE) {
    const float diff = (p.label_margin ? dy : p.margin) - d;
    *l = fmaxf(diff, 0.f);
    *g = diff > 0.f ? -1.f : 0.f;
    return true;
  }
  // focal: w_f = (1 - p)^gamma [* alpha] on p = clip(sigmoid(d), 1e-7, 1 - 1e-7), times the cross entropy; the gradient runs
  // through w_f as the reference's does (clip_by_value passes none outside its bounds)
  if (p.has_hinge && !(d < p.hinge_margin)) return false;
  const float lo = 1e-7f, hi = 1.f - 1e-7f;
  const float e = expf(-fabsf(d));
  const float sig = d >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
  const float nsig = d >= 0.f ? e / (1.f + e) : 1.f / (1.f + e);  // 1 - sigmoid(d) without the cancellation
  const bool inside = sig >= lo && sig <= hi;
  const float pc = fminf(fmaxf(sig, lo), hi);
  const float q = inside ? nsig : 1.f - pc;
  float wf = p.gamma == 2.f ? q * q : powf(q, p.gamma);
  if (p.has_alpha) wf *= p.alpha;
  const float ce = fmaxf(d, 0.f) - d + log1pf(e);
  *l = wf * ce;
  *g = -wf * nsig + (inside ? -p.gamma * wf * pc * ce : 0.f);
  *present = wf;
  return true;
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void pair_kernel(const float* __restrict__ z, int64_t ldz, const float* __restrict__ y,
                                                     const int64_t* __restrict__ keys, const float* __restrict__ w, int B,
                                                     int chunk, PwParam p, float* __restrict__ pdz,
                                                     float* __restrict__ ploss, int32_t* __restrict__ pcnt) {
  __shared__ int64_t s_key[kPwMaxChunk];
  __shared__ float s_s[kPwMaxChunk], s_y[kPwMaxChunk], s_w[kPwMaxChunk];
  __shared__ float red[4];
  __shared__ int ired[8];
  const int tid = static_cast<int>(threadIdx.x);
  const int i = static_cast<int>(blockIdx.x) * kBlock + tid;
  const bool live = i < B;
  const int ii = live ? i : B - 1;
  const float si = z[ii * ldz] / p.temperature, yi = y[ii] / p.label_div, wi = w ? w[ii] : 1.f;
  const int64_t ki = keys ? keys[ii] : 0;
  const int c0 = static_cast<int>(blockIdx.y) * chunk;
  const int n = min(chunk, B - c0);  // (>= 1: splits = ceil(B / chunk))
  for (int t = tid; t < n; t += kBlock) {
    const int j = c0 + t;
    s_s[t] = z[j * ldz] / p.temperature;
    s_y[t] = y[j] / p.label_div;
    s_w[t] = w ? w[j] : 1.f;
    s_key[t] = keys ? keys[j] : 0;
  }
  __syncthreads();
  float loss = 0.f, dzi = 0.f;
  int cnt = 0, nzc = 0;
  if (live) {
    for (int t = 0; t < n; ++t) {
      const float yj = s_y[t];
      const bool first = yi > yj;
      if ((first || yj > yi) && s_key[t] == ki) {
        const float sj = s_s[t];
        const float d = first ? si - sj : sj - si, dy = first ? yi - yj : yj - yi, wt = first ? wi : s_w[t];
        float l, g, present;
        if (pw_pair<KIND>(p, d, dy, &l, &g, &present)) {
          if (first) {
            loss = loss + wt * l;
            dzi = dzi + wt * g;
            cnt += 1;
            nzc += wt * present != 0.f ? 1 : 0;
          } else {
            dzi = dzi - wt * g;
          }
        }
      }
    }
    pdz[static_cast<int64_t>(blockIdx.y) * B + i] = dzi;
  }
  const int g = static_cast<int>(blockIdx.y) * static_cast<int>(gridDim.x) + static_cast<int>(blockIdx.x);
  const float tot = block_sum_256(loss, red);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    cnt += __shfl_xor(cnt, off, kWave);
    nzc += __shfl_xor(nzc, off, kWave);
  }
  if ((tid & 63) == 0) {
    ired[tid >> 6] = cnt;
    ired[4 + (tid >> 6)] = nzc;
  }
  __syncthreads();
  if (tid == 0) {
    ploss[g] = tot;
    pcnt[2 * g] = ired[0] + ired[1] + ired[2] + ired[3];
    pcnt[2 * g + 1] = ired[4] + ired[5] + ired[6] + ired[7];
  }
}

__global__ __launch_bounds__(kBlock) void pair_finish_kernel(const float* __restrict__ pdz, const float* __restrict__ ploss,
                                                            const int32_t* __restrict__ pcnt, int B, int splits, int grid,
                                                            float scale, float temperature, float* __restrict__ dz,
                                                            float* __restrict__ loss_partials,
                                                            int32_t* __restrict__ pair_count) {
  __shared__ int ired[8];
  const int tid = static_cast<int>(threadIdx.x);
  int cnt = 0, nzc = 0;
  for (int g = tid; g < grid; g += kBlock) {
    cnt += pcnt[2 * g];
    nzc += pcnt[2 * g + 1];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    cnt += __shfl_xor(cnt, off, kWave);
    nzc += __shfl_xor(nzc, off, kWave);
  }
  if ((tid & 63) == 0) {
    ired[tid >> 6] = cnt;
    ired[4 + (tid >> 6)] = nzc;
  }
  __syncthreads();
  cnt = ired[0] + ired[1] + ired[2] + ired[3];
  nzc = ired[4] + ired[5] + ired[6] + ired[7];
  const float nz = nzc > 0 ? static_cast<float>(nzc) : 1.f;  // (no pair present: every sum is 0 - loss 0, zero gradient)
  const int i = static_cast<int>(blockIdx.x) * kBlock + tid;
  if (dz && i < B) {
    float s = 0.f;
    for (int c = 0; c < splits; ++c) s = s + pdz[static_cast<int64_t>(c) * B + i];
    dz[i] = scale * ((s / nz) / temperature);
  }
  if (blockIdx.x == 0) {
    if (loss_partials)
      for (int g = tid; g < grid; g += kBlock) loss_partials[g] = scale * (ploss[g] / nz);
    if (pair_count && tid == 0) pair_count[0] = cnt;
  }
}

template <int KIND>
static void pw_launch_pairs(const PwGeom& g, er_stream_t stream, const float* z, int64_t ldz, const float* y,
                            const int64_t* keys, const float* w, int B, const PwParam& p, float* pdz, float* ploss,
                            int32_t* pcnt) {
  hipLaunchKernelGGL(pair_kernel<KIND>, dim3(static_cast<unsigned>(g.rb), static_cast<unsigned>(g.splits)), dim3(kBlock), 0,
                     as_stream(stream), z, ldz, y, keys, w, B, g.chunk, p, pdz, ploss, pcnt);
}

}  // namespace er

extern "C" {

int32_t er_pairwise_grid(int64_t B) {
  const er::PwGeom g = er::pw_geom(B);
  return g.rb * g.splits;
}

int64_t er_pairwise_work_floats(int64_t B) {
  const er::PwGeom g = er::pw_geom(B);
  return static_cast<int64_t>(g.splits) * B + 3 * static_cast<int64_t>(g.rb) * g.splits;
}

int er_pairwise(const float* logits, int64_t ld_logits, const float* labels, const int64_t* session_keys,
                const float* weights, int64_t B, int32_t kind, int32_t flags, float temperature, float label_div,
                float margin, float hinge_margin, float gamma, float alpha, float loss_scale, float* work,
                float* loss_partials, float* dlogits, int32_t* pair_count, er_stream_t stream) {
  const er::PwGeom g = er::pw_geom(B);
  ER_REQUIRE(g.rb > 0, "er_pairwise: B = %lld outside the envelope (1 <= B <= %d)", static_cast<long long>(B), er::kPwMaxB);
  ER_REQUIRE(g.chunk >= 1 && g.chunk <= er::kPwMaxChunk && static_cast<int64_t>(g.splits) * g.chunk >= B,
             "er_pairwise: B = %lld: a column chunk of %d outside [1, %d]", static_cast<long long>(B), g.chunk, er::kPwMaxChunk);
  ER_REQUIRE(logits && labels && work, "er_pairwise: logits, labels and the workspace are required");
  ER_REQUIRE(ld_logits >= 1 && ld_logits <= (1 << 20), "er_pairwise: a logits pitch outside [1, 2^20]");
  ER_REQUIRE(kind >= ER_PAIR_WISE && kind <= ER_PAIR_FOCAL, "er_pairwise: kind %d", kind);
  ER_REQUIRE(temperature > 0.f && label_div > 0.f, "er_pairwise: temperature %g and label_div %g must be positive",
             static_cast<double>(temperature), static_cast<double>(label_div));
  ER_REQUIRE(kind != ER_PAIR_FOCAL || gamma >= 0.f, "er_pairwise: gamma %g below zero", static_cast<double>(gamma));
  er::PwParam p;
  p.temperature = temperature; p.label_div = label_div; p.margin = margin; p.hinge_margin = hinge_margin;
  p.gamma = gamma; p.alpha = alpha;
  p.label_margin = (flags & ER_PAIR_LABEL_MARGIN) ? 1 : 0;
  p.has_hinge = (flags & ER_PAIR_HINGE_MARGIN) ? 1 : 0;
  p.has_alpha = (flags & ER_PAIR_ALPHA) ? 1 : 0;
  const int grid = g.rb * g.splits, Bi = static_cast<int>(B);
  float* pdz = work;
  float* ploss = work + static_cast<int64_t>(g.splits) * B;
  int32_t* pcnt = reinterpret_cast<int32_t*>(ploss + grid);
  switch (kind) {
    case ER_PAIR_WISE:
      er::pw_launch_pairs<ER_PAIR_WISE>(g, stream, logits, ld_logits, labels, session_keys, weights, Bi, p, pdz, ploss, pcnt);
      break;
    case ER_PAIR_LOGISTIC:
      er::pw_launch_pairs<ER_PAIR_LOGISTIC>(g, stream, logits, ld_logits, labels, session_keys, weights, Bi, p, pdz, ploss, pcnt);
      break;
    case ER_PAIR_HINGE:
      er::pw_launch_pairs<ER_PAIR_HINGE>(g, stream, logits, ld_logits, labels, session_keys, weights, Bi, p, pdz, ploss, pcnt);
      break;
    default:
      er::pw_launch_pairs<ER_PAIR_FOCAL>(g, stream, logits, ld_logits, labels, session_keys, weights, Bi, p, pdz, ploss, pcnt);
  }
  ER_LAUNCH_CHECK();
  hipLaunchKernelGGL(er::pair_finish_kernel, dim3(static_cast<unsigned>(g.rb)), dim3(er::kBlock), 0, er::as_stream(stream),
                     pdz, ploss, pcnt, Bi, g.splits, grid, loss_scale, temperature, dlogits, loss_partials, pair_count);
  ER_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"

// K8p: the same losses for 8192 < B <= 131072 on examples sorted by (session key, example index).
//
// K8m evaluates all B x B column positions and keeps `splits x B` gradient partials, whatever the session keys leave of
// them.  After K8o's record sort (er_listwise_sort.h) a session is one run of consecutive positions, so a row's pairs
// lie in [lo, hi), its session's first position and one past its last:
//
//   pws_gather_kernel   one lane per sorted position p: (s, yl, w) through the index, lo and hi by two binary searches
//                       over the B real keys (the padding behind them is never read, so a real INT64_MAX key ends at
//                       B), one 16-byte column record (s, yl, w, lo as bits) and hi.  Without keys position p is
//                       example p and [lo, hi) = [0, B).
//   pws_pair_kernel     one lane per sorted row, 256 rows a workgroup.  The workgroup's columns run from lo of its
//                       first row to hi of its last real row (both ascend with the position) and pass through LDS in
//                       chunks of at most 1024 records; of a chunk a wavefront walks only the columns inside [lo of its
//                       first row, hi of its last real row) - wave-uniform bounds - and every lane reads the SAME LDS
//                       record per column.  A column is of the row's session when lo_j == lo_i; K8m's single pw_pair
//                       evaluation then serves both orientations.  A row sees every column of its session, so dz_i is
//                       complete in the lane's register: no column splits, no partial buffer.
//   pws_finish_kernel   the same grid.  Each workgroup sums the workgroups' 64-bit counts, scales its loss row and its
//                       rows' dz by loss_scale / nz (dz also by 1 / T) and scatters dz through the index.
//
// The float sums run over sorted positions (columns ascending from 0.f, block_sum_256's tree, the rows by the loss tail):
// a pure function of the inputs, not bit-equal to K8m.  No atomics, vector stores only, nothing read back to the host,
// every dependency between workgroups a kernel boundary.
namespace er {

constexpr int kPwsChunk = 1024;  // column records staged in LDS: 16 bytes each

struct PwsWork {  // (host only) the workspace's parts
  int64_t* key[2]; int32_t* idx[2]; float4* rec; int64_t* pcnt; int32_t* hi; float* dzs; float* ploss;
};

// key [2][NP] int64 | index [2][NP] int32 | records [B] 16 bytes | counts [rows][2] int64 | hi [B] | dz [B] | loss [rows]
inline int64_t pws_workspace_bytes(int64_t B, int tile) {
  const int T = lwt_tile(B, tile);
  if (T == 0) return 0;
  const int64_t NP = ceil_div(B, T) * T, rows = ceil_div(B, kBlock);
  return NP * 2 * kLwRecordBytes + 24 * B + 20 * rows;
}

inline PwsWork pws_carve(void* workspace, int64_t B, int T) {
  const int64_t NP = ceil_div(B, T) * T, rows = ceil_div(B, kBlock);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  PwsWork k;
  k.key[0] = reinterpret_cast<int64_t*>(ws);
  k.key[1] = k.key[0] + NP;
  k.idx[0] = reinterpret_cast<int32_t*>(ws + NP * 16);
  k.idx[1] = k.idx[0] + NP;
  ws += NP * 2 * kLwRecordBytes;
  k.rec = reinterpret_cast<float4*>(ws);
  k.pcnt = reinterpret_cast<int64_t*>(ws + 16 * B);
  k.hi = reinterpret_cast<int32_t*>(ws + 16 * B + 16 * rows);
  k.dzs = reinterpret_cast<float*>(ws + 20 * B + 16 * rows);
  k.ploss = k.dzs + B;
  return k;
}

__global__ __launch_bounds__(kBlock) void pws_gather_kernel(const float* __restrict__ z, int64_t ldz,
                                                           const float* __restrict__ y, const float* __restrict__ w,
                                                           const int64_t* __restrict__ skey, const int32_t* __restrict__ sidx,
                                                           int B, float temperature, float label_div,
                                                           float4* __restrict__ rec, int32_t* __restrict__ hi) {
  const int p = static_cast<int>(blockIdx.x) * kBlock + static_cast<int>(threadIdx.x);
  if (p >= B) return;
  int i = p, first = 0, past = B;
  if (skey) {
    i = sidx[p];
    const int64_t k = skey[p];
    int a = 0, b = p;  // the first position whose key is not below k: in [0, p]
    while (a < b) {
      const int mid = (a + b) >> 1;
      if (skey[mid] < k) a = mid + 1; else b = mid;
    }
    first = a;
    a = p + 1; b = B;  // the first position whose key is above k, or B: in [p + 1, B]
    while (a < b) {
      const int mid = (a + b) >> 1;
      if (skey[mid] > k) b = mid; else a = mid + 1;
    }
    past = a;
  }
  rec[p] = make_float4(z[i * ldz] / temperature, y[i] / label_div, w ? w[i] : 1.f, __int_as_float(first));
  hi[p] = past;
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void pws_pair_kernel(const float4* __restrict__ rec, const int32_t* __restrict__ hi,
                                                         int B, PwParam p, float* __restrict__ dzs,
                                                         float* __restrict__ ploss, int64_t* __restrict__ pcnt) {
  __shared__ float4 s_rec[kPwsChunk];
  __shared__ float red[4];
  __shared__ long long lred[8];
  const int tid = static_cast<int>(threadIdx.x), r0 = static_cast<int>(blockIdx.x) * kBlock;
  const int i = r0 + tid;
  const bool live = i < B;
  const float4 me = rec[live ? i : B - 1];
  const float si = me.x, yi = me.y, wi = me.z;
  const int loi = live ? __float_as_int(me.w) : -1;  // (no column's lo is negative: a dead row meets no pair)
  // the workgroup's columns, and inside them the wavefront's (an idle wavefront: none)
  const int c_begin = __float_as_int(rec[r0].w), c_end = hi[min(r0 + kBlock, B) - 1];
  const int wr = r0 + (tid & ~(kWave - 1));
  const int wlo = __builtin_amdgcn_readfirstlane(wr < B ? __float_as_int(rec[wr].w) : 0);
  const int whi = __builtin_amdgcn_readfirstlane(wr < B ? hi[min(wr + kWave, B) - 1] : 0);
  float loss = 0.f, dzi = 0.f;
  int cnt = 0, nzc = 0;
  for (int c0 = c_begin; c0 < c_end; c0 += kPwsChunk) {
    const int n = min(kPwsChunk, c_end - c0);
    if (c0 > c_begin) __syncthreads();  // (the chunk before is read to its end)
    for (int t = tid; t < n; t += kBlock) s_rec[t] = rec[c0 + t];
    __syncthreads();
    const int from = max(c0, wlo), to = min(c0 + n, whi);
    for (int c = from; c < to; ++c) {
      const float4 col = s_rec[c - c0];
      const float yj = col.y;
      const bool first = yi > yj;
      if ((first || yj > yi) && __float_as_int(col.w) == loi) {
        const float sj = col.x;
        const float d = first ? si - sj : sj - si, dy = first ? yi - yj : yj - yi, wt = first ? wi : col.z;
        float l, g, present;
        if (pw_pair<KIND>(p, d, dy, &l, &g, &present)) {
          if (first) {
            loss = loss + wt * l;
            dzi = dzi + wt * g;
            cnt += 1;
            nzc += wt * present != 0.f ? 1 : 0;
          } else {
            dzi = dzi - wt * g;
          }
        }
      }
    }
  }
  if (live) dzs[i] = dzi;
  const float tot = block_sum_256(loss, red);
  long long c64 = cnt, n64 = nzc;  // (a lane meets at most B columns; beyond the lane the counts are 64-bit)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    c64 += __shfl_xor(c64, off, kWave);
    n64 += __shfl_xor(n64, off, kWave);
  }
  if ((tid & 63) == 0) {
    lred[tid >> 6] = c64;
    lred[4 + (tid >> 6)] = n64;
  }
  __syncthreads();
  if (tid == 0) {
    ploss[blockIdx.x] = tot;
    pcnt[2 * blockIdx.x] = lred[0] + lred[1] + lred[2] + lred[3];
    pcnt[2 * blockIdx.x + 1] = lred[4] + lred[5] + lred[6] + lred[7];
  }
}

__global__ __launch_bounds__(kBlock) void pws_finish_kernel(const float* __restrict__ dzs, const float* __restrict__ ploss,
                                                           const int64_t* __restrict__ pcnt,
                                                           const int32_t* __restrict__ sidx, int B, float scale,
                                                           float temperature, float* __restrict__ dz,
                                                           float* __restrict__ loss_partials,
                                                           int64_t* __restrict__ pair_count) {
  __shared__ long long lred[8];
  const int tid = static_cast<int>(threadIdx.x), rows = static_cast<int>(gridDim.x);
  long long cnt = 0, nzc = 0;
  for (int g = tid; g < rows; g += kBlock) {  // (at most 512 rows: two a lane, in workgroup order)
    cnt += pcnt[2 * g];
    nzc += pcnt[2 * g + 1];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    cnt += __shfl_xor(cnt, off, kWave);
    nzc += __shfl_xor(nzc, off, kWave);
  }
  if ((tid & 63) == 0) {
    lred[tid >> 6] = cnt;
    lred[4 + (tid >> 6)] = nzc;
  }
  __syncthreads();
  cnt = lred[0] + lred[1] + lred[2] + lred[3];
  nzc = lred[4] + lred[5] + lred[6] + lred[7];
  const float nz = nzc > 0 ? static_cast<float>(nzc) : 1.f;  // (no pair present: every sum is 0 - loss 0, zero gradient)
  const int i = static_cast<int>(blockIdx.x) * kBlock + tid;
  if (dz && i < B) dz[sidx ? sidx[i] : i] = scale * ((dzs[i] / nz) / temperature);
  if (tid == 0) {
    if (loss_partials) loss_partials[blockIdx.x] = scale * (ploss[blockIdx.x] / nz);
    if (pair_count && blockIdx.x == 0) pair_count[0] = cnt;
  }
}

template <int KIND>
static void pws_launch_pairs(int rows, er_stream_t stream, const PwsWork& k, int B, const PwParam& p) {
  hipLaunchKernelGGL(pws_pair_kernel<KIND>, dim3(static_cast<unsigned>(rows)), dim3(kBlock), 0, as_stream(stream), k.rec, k.hi,
                     B, p, k.dzs, k.ploss, k.pcnt);
}

}  // namespace er

extern "C" {

int32_t er_pairwise_sorted_grid(int64_t B, int32_t tile) {
  return er::lwt_tile(B, tile) > 0 ? static_cast<int32_t>(er::ceil_div(B, er::kBlock)) : 0;
}

int64_t er_pairwise_sorted_workspace_bytes(int64_t B, int32_t tile) { return er::pws_workspace_bytes(B, tile); }

int er_pairwise_sorted(const float* logits, int64_t ld_logits, const float* labels, const int64_t* session_keys,
                       const float* weights, int64_t B, int32_t kind, int32_t flags, float temperature, float label_div,
                       float margin, float hinge_margin, float gamma, float alpha, float loss_scale, int32_t tile,
                       void* workspace, int64_t workspace_bytes, float* loss_partials, float* dlogits, int64_t* pair_count,
                       er_stream_t stream) {
  const int T = er::lwt_tile(B, tile);
  ER_REQUIRE(T > 0, "er_pairwise_sorted: B = %lld, tile = %d outside the envelope (tile 0: %d < B <= %d; tile 1024, 2048, "
             "4096 or 8192: 1 <= B <= %d)", static_cast<long long>(B), tile, er::kLwMaxB, er::kLwtMaxB, er::kLwtMaxB);
  ER_REQUIRE(logits && labels, "er_pairwise_sorted: logits and labels are required");
  ER_REQUIRE(ld_logits >= 1 && ld_logits <= (1 << 20), "er_pairwise_sorted: a logits pitch outside [1, 2^20]");
  ER_REQUIRE(kind >= ER_PAIR_WISE && kind <= ER_PAIR_FOCAL, "er_pairwise_sorted: kind %d", kind);
  ER_REQUIRE(temperature > 0.f && label_div > 0.f, "er_pairwise_sorted: temperature %g and label_div %g must be positive",
             static_cast<double>(temperature), static_cast<double>(label_div));
  ER_REQUIRE(kind != ER_PAIR_FOCAL || gamma >= 0.f, "er_pairwise_sorted: gamma %g below zero", static_cast<double>(gamma));
  ER_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0 &&
                 workspace_bytes >= er::pws_workspace_bytes(B, tile),
             "er_pairwise_sorted: the workspace is missing, not 16-byte aligned or below %lld bytes",
             static_cast<long long>(er::pws_workspace_bytes(B, tile)));
  er::PwParam p;
  p.temperature = temperature; p.label_div = label_div; p.margin = margin; p.hinge_margin = hinge_margin;
  p.gamma = gamma; p.alpha = alpha;
  p.label_margin = (flags & ER_PAIR_LABEL_MARGIN) ? 1 : 0;
  p.has_hinge = (flags & ER_PAIR_HINGE_MARGIN) ? 1 : 0;
  p.has_alpha = (flags & ER_PAIR_ALPHA) ? 1 : 0;
  const er::PwsWork k = er::pws_carve(workspace, B, T);
  const int Bi = static_cast<int>(B), rows = static_cast<int>(er::ceil_div(B, er::kBlock));
  const int64_t* skey = nullptr;
  const int32_t* sidx = nullptr;
  if (session_keys) {
    int cur = 0;
    if (const int rc = er::lwt_sort(session_keys, Bi, T, k.key, k.idx, stream, &cur)) return rc;
    skey = k.key[cur];
    sidx = k.idx[cur];
  }
  hipLaunchKernelGGL(er::pws_gather_kernel, dim3(static_cast<unsigned>(rows)), dim3(er::kBlock), 0, er::as_stream(stream),
                     logits, ld_logits, labels, weights, skey, sidx, Bi, temperature, label_div, k.rec, k.hi);
  ER_LAUNCH_CHECK();
  switch (kind) {
    case ER_PAIR_WISE: er::pws_launch_pairs<ER_PAIR_WISE>(rows, stream, k, Bi, p); break;
    case ER_PAIR_LOGISTIC: er::pws_launch_pairs<ER_PAIR_LOGISTIC>(rows, stream, k, Bi, p); break;
    case ER_PAIR_HINGE: er::pws_launch_pairs<ER_PAIR_HINGE>(rows, stream, k, Bi, p); break;
    default: er::pws_launch_pairs<ER_PAIR_FOCAL>(rows, stream, k, Bi, p);
  }
  ER_LAUNCH_CHECK();
  hipLaunchKernelGGL(er::pws_finish_kernel, dim3(static_cast<unsigned>(rows)), dim3(er::kBlock), 0, er::as_stream(stream),
                     k.dzs, k.ploss, k.pcnt, sidx, Bi, loss_scale, temperature, dlogits, loss_partials, pair_count);
  ER_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
