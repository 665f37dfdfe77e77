// K8n: the session-keyed listwise ranking losses of reference loss/listwise_loss.py - listwise_rank_loss and
// listwise_distill_loss - with d loss / d logits, the scale variables' gradient partials and the session count, in O(B)
// memory and O(B log^2 B) compare-exchanges.
//
// The reference runs tf.unique over the session ids and then tf.map_fn over the sessions, each iteration masking the whole
// batch: O(S * B) work in S dependent steps with data-dependent shapes.  Here ONE workgroup of 1024 lanes
//
//   1. sorts the records (key, example index) in LDS with a bitonic network, lexicographically on (signed key, index): a
//      total order, so the result is a pure function of the data.  Padding records carry INT64_MAX and an index >= B, so
//      a real INT64_MAX key sorts in front of them.  Afterwards a session is one run of positions, its members in
//      ascending example index, and the real records are the positions 0 .. B - 1;
//   2. lets lane l own the E = max(N / 1024, 1) positions l E .. l E + E - 1 in registers: heads and tails by comparing
//      neighbouring keys, z and y gathered through the index.  The key array is dead then and becomes the scratch;
//   3. reduces over the sessions with inclusive segmented scans (seg_scan: the lane's elements, the wavefront by __shfl_up
//      on (head seen, value), the 16 wavefronts through LDS) whose result the session's tail stores at scratch[session
//      number] and every member reads back (seg_total).  The session numbers are the same scan over the head flags;
//   4. sums the terms of the loss and of the scale gradients over the positions in sorted order and scatters dlogits
//      back through the index.
//
// There is no contraction in this, so MFMA does not fit.  fp32, precise expf / logf / log1pf, no atomics, vector stores
// only, every float sum in one fixed order: two runs and a graph replay give the same bits.
#include <math.h>

#include "er_common.h"
#include "er_listwise_sort.h"

namespace er {

constexpr int kLwThreads = 1024;
constexpr int kLwWaves = kLwThreads / kWave;
constexpr int kLwPlainLds = 64 << 10;  // dynamic LDS a launch gets without opting in

// N: the power of two >= max(B, 2); 0 outside the envelope
inline int lw_padded(int64_t B) {
  if (B < 1 || B > kLwMaxB) return 0;
  int n = 2;
  while (n < B) n <<= 1;
  return n;
}

struct LwParam {
  float temperature, clip_max, loss_scale;
  int kind, label_is_logits, label_ready;
};

__device__ __forceinline__ bool lw_before(int64_t ka, int ia, int64_t kb, int ib) {
  return ka < kb || (ka == kb && ia < ib);
}

template <int OP, typename T>  // OP 0: a + b, 1: max(a, b) (floats)
__device__ __forceinline__ T lw_op(T a, T b) {
  if constexpr (OP == 1) {
    return fmaxf(a, b);
  } else {
    return a + b;
  }
}

// Inclusive segmented scan over the positions tid * E + e.  heads: bit e set where element e starts a segment.  carry_val /
// carry_flag: kLwWaves LDS words each; the caller puts a workgroup barrier between this scan's end and the next one's
// start (seg_total's, or its own).
template <int E, int OP, typename T>
__device__ __forceinline__ void seg_scan(T (&v)[E], unsigned heads, T identity, T* carry_val, int* carry_flag) {
  const int lane = static_cast<int>(threadIdx.x) & (kWave - 1), wave = static_cast<int>(threadIdx.x) / kWave;
#pragma unroll
  for (int e = 1; e < E; ++e)
    if (!((heads >> e) & 1u)) v[e] = lw_op<OP>(v[e - 1], v[e]);
  // the lanes of the wavefront on (head seen, the value of the lane's last open segment)
  T val = v[E - 1];
  int flag = heads != 0u ? 1 : 0;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const T pv = __shfl_up(val, off, kWave);
    const int pf = __shfl_up(flag, off, kWave);
    if (lane >= off) {
      if (!flag) val = lw_op<OP>(pv, val);
      flag |= pf;
    }
  }
  if (lane == kWave - 1) {
    carry_val[wave] = val;
    carry_flag[wave] = flag;
  }
  T ex = __shfl_up(val, 1, kWave);  // what reaches this lane from the lanes before it
  int exf = __shfl_up(flag, 1, kWave);
  if (lane == 0) {
    ex = identity;
    exf = 0;
  }
  __syncthreads();
  if (!exf) {  // the segment open at this lane's start reaches back into the wavefronts before: fold them in wave order
    T c = identity;
    for (int u = 0; u < wave; ++u) c = carry_flag[u] ? carry_val[u] : lw_op<OP>(c, carry_val[u]);
    ex = lw_op<OP>(c, ex);
  }
  bool open = true;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    open = open && !((heads >> e) & 1u);
    if (open) v[e] = lw_op<OP>(ex, v[e]);
  }
}

// every member's v <- its session's inclusive-scan value at the tail.  tot: B floats of scratch; a workgroup barrier lies
// between any earlier read of it and this call (seg_scan's).
template <int E>
__device__ __forceinline__ void seg_total(float (&v)[E], unsigned tails, const int (&sid)[E], int nv, float* tot) {
#pragma unroll
  for (int e = 0; e < E; ++e)
    if ((tails >> e) & 1u) tot[sid[e]] = v[e];
  __syncthreads();
#pragma unroll
  for (int e = 0; e < E; ++e)
    if (e < nv) v[e] = tot[sid[e]];
}

template <int E>
__global__ __launch_bounds__(kLwThreads) void listwise_kernel(const float* __restrict__ z, int64_t ldz,
                                                              const float* __restrict__ y,
                                                              const int64_t* __restrict__ keys, int B, int N, LwParam p,
                                                              const float* __restrict__ scale_w,
                                                              const float* __restrict__ scale_b,
                                                              float* __restrict__ loss_partials, float* __restrict__ dz,
                                                              int64_t lddz, float* __restrict__ scale_partials,
                                                              int32_t* __restrict__ num_sessions) {
  extern __shared__ __align__(16) unsigned char lw_lds[];  // key [N] int64 | index [N] int32
  int64_t* s_key = reinterpret_cast<int64_t*>(lw_lds);
  int32_t* s_idx = reinterpret_cast<int32_t*>(lw_lds + static_cast<size_t>(N) * 8);
  __shared__ float s_cv[kLwWaves];
  __shared__ int s_cf[kLwWaves];
  __shared__ float s_red[kLwWaves * 3];
  __shared__ int s_S;
  const int tid = static_cast<int>(threadIdx.x);

  // ---- 1. the sort
  for (int i = tid; i < N; i += kLwThreads) {
    s_key[i] = i < B ? keys[i] : INT64_MAX;
    s_idx[i] = i;
  }
  __syncthreads();
  for (int k = 2; k <= N; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (N >> 1); t += kLwThreads) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const bool up = (lo & k) == 0;
        const int64_t ka = s_key[lo], kb = s_key[hi];
        const int ia = s_idx[lo], ib = s_idx[hi];
        if (lw_before(kb, ib, ka, ia) == up) {  // (the records are distinct: not before = after)
          s_key[lo] = kb; s_key[hi] = ka;
          s_idx[lo] = ib; s_idx[hi] = ia;
        }
      }
      __syncthreads();
    }
  }

  // ---- 2. this lane's positions: heads, tails, the example indices
  const int p0 = tid * E;
  const int nv = min(max(B - p0, 0), E);  // the real records among them: positions below B
  unsigned heads = 0u, tails = 0u;
  int id[E], sid[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int pos = p0 + e;
    id[e] = 0;
    if (e < nv) {
      const int64_t k = s_key[pos];
      id[e] = s_idx[pos];
      if (pos == 0 || s_key[pos - 1] != k) heads |= 1u << e;
      if (pos == B - 1 || s_key[pos + 1] != k) tails |= 1u << e;
    } else {
      heads |= 1u << e;  // (padding: a segment of its own that holds the identity)
    }
  }
  // the session numbers: a plain inclusive scan of the head flags, less one; S is its last value
#pragma unroll
  for (int e = 0; e < E; ++e) sid[e] = (e < nv && ((heads >> e) & 1u)) ? 1 : 0;
  seg_scan<E, 0, int>(sid, tid == 0 ? 1u : 0u, 0, reinterpret_cast<int*>(s_cv), s_cf);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    if (p0 + e == B - 1) s_S = sid[e];
    sid[e] -= 1;
  }
  __syncthreads();  // (every lane is past the keys: their space is scratch from here on)
  const int S = s_S;
  // (one scratch array serves every reduction: between a seg_total's reads and the next one's writes lies the barrier
  // inside the seg_scan that feeds the latter)
  float* tot = reinterpret_cast<float*>(lw_lds);

  // ---- 3. the operands in the reference's order
  const bool scaled = scale_w != nullptr;
  const float w = scaled ? scale_w[0] : 1.f, wa = fabsf(w), b = scaled ? scale_b[0] : 0.f;
  const bool cool = p.temperature != 1.f;
  const float ninf = -INFINITY;
  float zz[E], am[E], ea[E], t[E], v[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    zz[e] = 0.f; am[e] = ninf; t[e] = 0.f;
    if (e < nv) {
      zz[e] = z[id[e] * ldz];
      float a = scaled ? zz[e] * wa + b : zz[e];
      if (cool) a = a / p.temperature;
      am[e] = a;
      float yl = y[id[e]];
      if (!p.label_ready) {
        if (p.kind == ER_LIST_DISTILL) {
          yl = fminf(fmaxf(yl, 1.f), p.clip_max);
          yl = log1pf(p.clip_max) - logf(yl);
        } else if (cool && p.label_is_logits) {
          yl = yl / p.temperature;
        }
      }
      t[e] = yl;
    }
  }
  // m_s and se_s; am <- a - m_s, ea <- exp(a - m_s), later the softmax
#pragma unroll
  for (int e = 0; e < E; ++e) v[e] = am[e];
  seg_scan<E, 1, float>(v, heads, ninf, s_cv, s_cf);
  seg_total<E>(v, tails, sid, nv, tot);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    am[e] = e < nv ? am[e] - v[e] : 0.f;
    ea[e] = e < nv ? expf(am[e]) : 0.f;
    v[e] = ea[e];
  }
  seg_scan<E, 0, float>(v, heads, 0.f, s_cv, s_cf);
  seg_total<E>(v, tails, sid, nv, tot);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    if (e < nv) {
      am[e] = am[e] - logf(v[e]);  // log softmax
      ea[e] = ea[e] / v[e];        // softmax
    }
  }
  // t: the labels' softmax, the labels over their session's sum, or the labels as they are
  const bool soft = p.kind == ER_LIST_RANK && p.label_is_logits;
  if (soft) {
#pragma unroll
    for (int e = 0; e < E; ++e) v[e] = e < nv ? t[e] : ninf;
    seg_scan<E, 1, float>(v, heads, ninf, s_cv, s_cf);
    seg_total<E>(v, tails, sid, nv, tot);
#pragma unroll
    for (int e = 0; e < E; ++e) t[e] = e < nv ? expf(t[e] - v[e]) : 0.f;
  }
  if (soft || p.kind == ER_LIST_DISTILL) {
#pragma unroll
    for (int e = 0; e < E; ++e) v[e] = t[e];
    seg_scan<E, 0, float>(v, heads, 0.f, s_cv, s_cf);
    seg_total<E>(v, tails, sid, nv, tot);
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (e < nv) t[e] = t[e] / v[e];
  }
  // T_s
#pragma unroll
  for (int e = 0; e < E; ++e) v[e] = t[e];
  seg_scan<E, 0, float>(v, heads, 0.f, s_cv, s_cf);
  seg_total<E>(v, tails, sid, nv, tot);

  // ---- 4. the loss, the gradients
  const float c = p.loss_scale / static_cast<float>(S);
  float lsum = 0.f, gz = 0.f, gs = 0.f;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    if (e < nv) {
      lsum = lsum + t[e] * am[e];
      float g = c * (v[e] * ea[e] - t[e]);
      if (cool) g = g / p.temperature;
      gz = gz + g * zz[e];
      gs = gs + g;
      if (dz) dz[id[e] * lddz] = scaled ? g * wa : g;
    }
  }
  lsum = wave_sum(lsum);
  gz = wave_sum(gz);
  gs = wave_sum(gs);
  if ((tid & (kWave - 1)) == 0) {
    s_red[tid / kWave] = lsum;
    s_red[kLwWaves + tid / kWave] = gz;
    s_red[2 * kLwWaves + tid / kWave] = gs;
  }
  __syncthreads();
  if (tid == 0) {
    float r[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      r[q] = 0.f;
      for (int u = 0; u < kLwWaves; ++u) r[q] = r[q] + s_red[q * kLwWaves + u];
    }
    if (loss_partials) loss_partials[0] = p.loss_scale * (-r[0] / static_cast<float>(S));
    if (scale_partials) {
      scale_partials[0] = (w > 0.f ? 1.f : (w < 0.f ? -1.f : 0.f)) * r[1];
      scale_partials[1] = r[2];
    }
    if (num_sessions) num_sessions[0] = S;
  }
}

template <int E>
static int lw_launch(int N, er_stream_t stream, const float* z, int64_t ldz, const float* y, const int64_t* keys, int B,
                     const LwParam& p, const float* sw, const float* sb, float* loss_partials, float* dz, int64_t lddz,
                     float* scale_partials, int32_t* num_sessions) {
  // more than 64 KB of dynamic LDS is opted in to once per kernel (no stream work: safe inside a capture); the flag is per
  // process - the library's scope is one device per process driven by one host thread
  static bool opted = false;
  const int bytes = N * kLwRecordBytes;
  if (bytes > kLwPlainLds && !opted) {
    ER_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(listwise_kernel<E>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, kLwMaxB * kLwRecordBytes));
    opted = true;
  }
  hipLaunchKernelGGL(listwise_kernel<E>, dim3(1), dim3(kLwThreads), static_cast<size_t>(bytes), as_stream(stream), z, ldz, y,
                     keys, B, N, p, sw, sb, loss_partials, dz, lddz, scale_partials, num_sessions);
  ER_LAUNCH_CHECK();
  return 0;
}

}  // namespace er

extern "C" {

int32_t er_listwise_grid(int64_t B) { return er::lw_padded(B) > 0 ? 1 : 0; }

int64_t er_listwise_lds_bytes(int64_t B) { return static_cast<int64_t>(er::lw_padded(B)) * er::kLwRecordBytes; }

int er_listwise(const float* logits, int64_t ld_logits, const float* labels, const int64_t* session_keys, int64_t B,
                int32_t kind, int32_t flags, float temperature, float label_clip_max, const float* scale_w,
                const float* scale_b, float loss_scale, float* loss_partials, float* dlogits, int64_t ld_dlogits,
                float* scale_partials, int32_t* num_sessions, er_stream_t stream) {
  const int N = er::lw_padded(B);
  ER_REQUIRE(N > 0, "er_listwise: B = %lld outside the envelope (1 <= B <= %d)", static_cast<long long>(B), er::kLwMaxB);
  ER_REQUIRE(logits && labels && session_keys, "er_listwise: logits, labels and session_keys are required");
  ER_REQUIRE(ld_logits >= 1 && ld_logits <= (1 << 20), "er_listwise: a logits pitch outside [1, 2^20]");
  ER_REQUIRE(!dlogits || (ld_dlogits >= 1 && ld_dlogits <= (1 << 20)), "er_listwise: a dlogits pitch outside [1, 2^20]");
  ER_REQUIRE(kind == ER_LIST_RANK || kind == ER_LIST_DISTILL, "er_listwise: kind %d", kind);
  ER_REQUIRE(temperature > 0.f, "er_listwise: temperature %g must be positive", static_cast<double>(temperature));
  ER_REQUIRE((scale_w == nullptr) == (scale_b == nullptr), "er_listwise: scale_w and scale_b come together or not at all");
  ER_REQUIRE(!scale_partials || scale_w, "er_listwise: scale_partials without scale_w / scale_b");
  const bool ready = (flags & ER_LIST_LABEL_READY) != 0;
  ER_REQUIRE(kind != ER_LIST_DISTILL || ready || label_clip_max >= 1.f, "er_listwise: label_clip_max %g below 1",
             static_cast<double>(label_clip_max));
  er::LwParam p;
  p.temperature = temperature; p.clip_max = label_clip_max; p.loss_scale = loss_scale;
  p.kind = kind;
  p.label_is_logits = (flags & ER_LIST_LABEL_IS_LOGITS) ? 1 : 0;
  p.label_ready = ready ? 1 : 0;
  const int Bi = static_cast<int>(B);
  switch (N / er::kLwThreads) {
    case 8:
      return er::lw_launch<8>(N, stream, logits, ld_logits, labels, session_keys, Bi, p, scale_w, scale_b, loss_partials,
                              dlogits, ld_dlogits, scale_partials, num_sessions);
    case 4:
      return er::lw_launch<4>(N, stream, logits, ld_logits, labels, session_keys, Bi, p, scale_w, scale_b, loss_partials,
                              dlogits, ld_dlogits, scale_partials, num_sessions);
    case 2:
      return er::lw_launch<2>(N, stream, logits, ld_logits, labels, session_keys, Bi, p, scale_w, scale_b, loss_partials,
                              dlogits, ld_dlogits, scale_partials, num_sessions);
    default:
      return er::lw_launch<1>(N, stream, logits, ld_logits, labels, session_keys, Bi, p, scale_w, scale_b, loss_partials,
                              dlogits, ld_dlogits, scale_partials, num_sessions);
  }
}

}  // extern "C"

// K8o: the same losses for 8192 < B <= 131072 on G = ceil(B / T) workgroups of 1024 lanes, T = 1024 .. 8192 records each.
//
// One workgroup's LDS holds no more than 8192 records, so the sort becomes a tile sort and ceil(log2 G) merge passes, and
// every reduction over the sessions becomes a reduction inside the chunks plus a fold over one carry record per chunk:
//
//   1. listwise_tile_sort_kernel: workgroup g sorts the records g T .. g T + T - 1 in LDS (K8n's network and K8n's padding:
//      (INT64_MAX, position) from position B on) and writes its run to record buffer 0;
//   2. listwise_merge_kernel, once per pass, from one record buffer into the other: neighbouring runs of L records become
//      runs of 2 L.  A workgroup produces T consecutive records of the output: two lanes find the merge-path splits of the
//      chunk's first and last diagonal by binary search in the two runs, the workgroup loads the T records between them -
//      the first run's ascending, the second run's descending behind them: a bitonic sequence - and the log2 T compare-
//      exchange steps of a bitonic merge order them.  A run without a partner is copied.  The records are distinct (every
//      index is unique), so the order is total and the result a pure function of the data;
//   3. listwise_tiled_reduce_kernel in three stages, one launch each, workgroup g on the positions g T .. g T + T - 1 with
//      E = T / 1024 a lane in registers.  Heads and tails are the sessions' true edges (a chunk's first and last position
//      read their neighbour in the next chunk from global memory); inside the chunk the reductions are K8n's seg_scan /
//      seg_total over the LOCAL segments - the true ones cut at the chunk's edges.  Only the chunk's first and last local
//      segment can be a part of a session that goes on in another chunk: each stage leaves their two partials, and the
//      next stage's workgroups fold the carries of the chunks such a session touches in chunk order (lw_fold):
//        stage A  (max a, sum exp(a - max)) and, by the label form, (max y, sum exp(y - max)) or sum y - pairs combine by
//                 rescaling, (m1, s1) + (m2, s2) = (m, s1 e^(m1 - m) + s2 e^(m2 - m)), m = max(m1, m2) - and the chunk's
//                 flags and head count;
//        stage B  with the y totals t_i, and the partials of T_s = sum t_i;
//        stage C  with every total and S = the sum of the head counts: the loss terms, g_i, dlogits scattered back through
//                 the index, and one row of loss and scale partials per workgroup.
//      Each stage recomputes what it needs of the stage before from the inputs - a pure function of them, so the same bits.
//
// Every dependency between workgroups is a kernel boundary: no workgroup waits for another's write, nothing is launched
// cooperatively.  There is no contraction in any of this, so MFMA does not fit.  fp32, precise expf / logf / log1pf, no
// atomics, vector stores only, every float sum in one fixed order: two runs and a graph replay give the same bits.
namespace er {

constexpr int kLwtMaxG = kLwtMaxB / kLwThreads;  // chunks at the smallest tile
// a chunk's carry record, 16 words: slot q (0: the a pair, 1: the y pair or sum, 2: sum t) holds its leading partial at
// words 4 q, 4 q + 1 and its trailing partial at 4 q + 2, 4 q + 3; the flags at word 12, the head count at word 13
constexpr int kLwtCarry = 16;
constexpr int kLwtFlags = 12, kLwtHeads = 13;
enum { kLwtWhole = 1, kLwtOpenStart = 2, kLwtOpenEnd = 4 };

// the steps k = k_from, 2 k_from, .., N of K8n's bitonic network over N records in LDS (k_from = 2: the sort; k_from = N:
// the merge of a bitonic sequence, ascending); a workgroup barrier lies before it and after every step
__device__ __forceinline__ void lwt_network(int64_t* s_key, int32_t* s_idx, int N, int k_from) {
  const int tid = static_cast<int>(threadIdx.x);
  for (int k = k_from; k <= N; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (N >> 1); t += kLwThreads) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const bool up = (lo & k) == 0;
        const int64_t ka = s_key[lo], kb = s_key[hi];
        const int ia = s_idx[lo], ib = s_idx[hi];
        if (lw_before(kb, ib, ka, ia) == up) {
          s_key[lo] = kb; s_key[hi] = ka;
          s_idx[lo] = ib; s_idx[hi] = ia;
        }
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(kLwThreads) void listwise_tile_sort_kernel(const int64_t* __restrict__ keys, int B, int T,
                                                                        int64_t* __restrict__ okey,
                                                                        int32_t* __restrict__ oidx) {
  extern __shared__ __align__(16) unsigned char lw_lds[];  // key [T] int64 | index [T] int32
  int64_t* s_key = reinterpret_cast<int64_t*>(lw_lds);
  int32_t* s_idx = reinterpret_cast<int32_t*>(lw_lds + static_cast<size_t>(T) * 8);
  const int tid = static_cast<int>(threadIdx.x), base = static_cast<int>(blockIdx.x) * T;
  for (int i = tid; i < T; i += kLwThreads) {
    s_key[i] = base + i < B ? keys[base + i] : INT64_MAX;
    s_idx[i] = base + i;
  }
  __syncthreads();
  lwt_network(s_key, s_idx, T, 2);
  for (int i = tid; i < T; i += kLwThreads) {
    okey[base + i] = s_key[i];
    oidx[base + i] = s_idx[i];
  }
}

// One merge pass over NP = G T records in runs of L (a multiple of T): workgroup c writes the records c T .. c T + T - 1.
__global__ __launch_bounds__(kLwThreads) void listwise_merge_kernel(const int64_t* __restrict__ ikey,
                                                                    const int32_t* __restrict__ iidx, int NP, int L, int T,
                                                                    int64_t* __restrict__ okey,
                                                                    int32_t* __restrict__ oidx) {
  extern __shared__ __align__(16) unsigned char lw_lds[];  // key [T] int64 | index [T] int32
  int64_t* s_key = reinterpret_cast<int64_t*>(lw_lds);
  int32_t* s_idx = reinterpret_cast<int32_t*>(lw_lds + static_cast<size_t>(T) * 8);
  __shared__ int s_split[2];
  const int tid = static_cast<int>(threadIdx.x), c0 = static_cast<int>(blockIdx.x) * T;
  const int base = c0 / (2 * L) * (2 * L);  // the pair of runs this chunk lies in: [base, base + L) and what follows
  if (base + L >= NP) {                     // (the same for the whole workgroup) no partner: the run moves as it is
    for (int i = tid; i < T; i += kLwThreads) {
      okey[c0 + i] = ikey[c0 + i];
      oidx[c0 + i] = iidx[c0 + i];
    }
    return;
  }
  const int lenA = L, lenB = min(L, NP - base - L), d0 = c0 - base;  // (d0 + T <= lenA + lenB: NP is a multiple of T)
  const int64_t* ak = ikey + base;
  const int64_t* bk = ikey + base + L;
  const int32_t* ai = iidx + base;
  const int32_t* bi = iidx + base + L;
  if (tid == 0 || tid == kWave) {
    // the merge-path split of diagonal d: how many of the first d merged records the first run gives.  lo <= mid < hi
    // keeps mid < lenA and 0 <= d - 1 - mid < lenB
    const int d = tid == 0 ? d0 : d0 + T;
    int lo = max(0, d - lenB), hi = min(d, lenA);
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (lw_before(ak[mid], ai[mid], bk[d - 1 - mid], bi[d - 1 - mid])) {
        lo = mid + 1;
      } else {
        hi = mid;
      }
    }
    s_split[tid == 0 ? 0 : 1] = lo;
  }
  __syncthreads();
  const int a0 = s_split[0], nA = s_split[1] - a0, b0 = d0 - a0;  // T - nA records of the second run, from b0 on
  for (int i = tid; i < T; i += kLwThreads) {
    if (i < nA) {
      s_key[i] = ak[a0 + i];
      s_idx[i] = ai[a0 + i];
    } else {
      s_key[i] = bk[b0 + (T - 1 - i)];
      s_idx[i] = bi[b0 + (T - 1 - i)];
    }
  }
  __syncthreads();
  lwt_network(s_key, s_idx, T, T);
  for (int i = tid; i < T; i += kLwThreads) {
    okey[c0 + i] = s_key[i];
    oidx[c0 + i] = s_idx[i];
  }
}

// The total of slot q of the session whose first part is chunk h0's trailing segment: that partial, then the leading
// partials of the chunks after it, in chunk order, while the session goes on (the chunk is one segment and open at its
// end).  Called only where chunk h0 is open at its end, so chunk h0 + 1 exists.  car: the carries of all G chunks.
template <bool PAIR>
__device__ __forceinline__ void lw_fold(const float* car, int G, int h0, int q, float& r0, float& r1) {
  float m = car[h0 * kLwtCarry + 4 * q + 2], s = car[h0 * kLwtCarry + 4 * q + 3];
  int cur = h0, f;
  do {
    ++cur;
    const float lm = car[cur * kLwtCarry + 4 * q], ls = car[cur * kLwtCarry + 4 * q + 1];
    if constexpr (PAIR) {
      const float mm = fmaxf(m, lm);
      s = s * expf(m - mm) + ls * expf(lm - mm);
      m = mm;
    } else {
      m = m + lm;
    }
    f = reinterpret_cast<const int*>(car)[cur * kLwtCarry + kLwtFlags];
  } while ((f & kLwtWhole) && (f & kLwtOpenEnd) && cur + 1 < G);
  r0 = m;
  r1 = s;
}

// the local segments' totals of v under OP, read back by every member
template <int E, int OP>
__device__ __forceinline__ void lwt_local(float (&v)[E], unsigned heads, unsigned tails, const int (&sid)[E], int nv,
                                          float identity, float* s_cv, int* s_cf, float* tot) {
  seg_scan<E, OP, float>(v, heads, identity, s_cv, s_cf);
  seg_total<E>(v, tails, sid, nv, tot);
}

// STAGE 0, 1, 2: A, B, C of the header
template <int E, int STAGE>
__global__ __launch_bounds__(kLwThreads) void listwise_tiled_reduce_kernel(
    const float* __restrict__ z, int64_t ldz, const float* __restrict__ y, const int64_t* __restrict__ skey,
    const int32_t* __restrict__ sidx, int B, LwParam p, const float* __restrict__ scale_w,
    const float* __restrict__ scale_b, float* __restrict__ carry, float* __restrict__ loss_partials,
    float* __restrict__ dz, int64_t lddz, float* __restrict__ scale_partials, int32_t* __restrict__ num_sessions) {
  constexpr int T = E * kLwThreads;
  __shared__ float s_tot[T];                     // the local segments' totals
  __shared__ float s_car[kLwtMaxG * kLwtCarry];  // every chunk's carry (stages B and C)
  __shared__ float s_edge[2][3][2];              // [the session open at the start | at the end][slot][word]
  __shared__ float s_cv[kLwWaves];
  __shared__ int s_cf[kLwWaves];
  __shared__ float s_red[kLwWaves * 3];
  __shared__ int s_open[2], s_nseg, s_S;
  const int tid = static_cast<int>(threadIdx.x), g = static_cast<int>(blockIdx.x), G = static_cast<int>(gridDim.x);
  const int c0 = g * T, last = min(B, c0 + T) - 1;  // the chunk's first position and its last real one

  if constexpr (STAGE > 0) {
    for (int i = tid; i < G * kLwtCarry; i += kLwThreads) s_car[i] = carry[i];
  }

  // ---- this lane's positions: the true edges, the local segments (cut at the chunk's edges as well)
  const int p0 = c0 + tid * E;
  const int nv = min(max(B - p0, 0), E);
  unsigned heads = 0u, tails = 0u;
  int id[E], sid[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int pos = p0 + e;
    id[e] = 0;
    if (e < nv) {
      const int64_t k = skey[pos];
      id[e] = sidx[pos];
      bool h = pos == 0 || skey[pos - 1] != k, tl = pos == B - 1 || skey[pos + 1] != k;
      if (pos == c0) {
        s_open[0] = h ? 0 : 1;
        h = true;
      }
      if (pos == c0 + T - 1) {
        s_open[1] = tl ? 0 : 1;
        tl = true;
      }
      if (h) heads |= 1u << e;
      if (tl) tails |= 1u << e;
    } else {
      heads |= 1u << e;  // (padding: a segment of its own that holds the identity)
    }
  }
  if (tid == kLwThreads - 1 && nv < E) s_open[1] = 0;  // (the last chunk ends inside its tile)
#pragma unroll
  for (int e = 0; e < E; ++e) sid[e] = (e < nv && ((heads >> e) & 1u)) ? 1 : 0;
  seg_scan<E, 0, int>(sid, tid == 0 ? 1u : 0u, 0, reinterpret_cast<int*>(s_cv), s_cf);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    if (p0 + e == last) s_nseg = sid[e];
    sid[e] -= 1;
  }
  __syncthreads();
  const int nseg = s_nseg;
  const bool ostart = s_open[0] != 0, oend = s_open[1] != 0;
  const bool whole = ostart && nseg == 1;  // no head of a session in the chunk

  // ---- the totals of the sessions that leave the chunk, S
  if constexpr (STAGE > 0) {
    if (tid < 6) {
      const int edge = tid / 3, q = tid % 3;
      const bool pair = q == 0 || (q == 1 && p.kind == ER_LIST_RANK && p.label_is_logits);
      float r0 = 0.f, r1 = 0.f;
      const bool normed = p.kind == ER_LIST_DISTILL || (p.kind == ER_LIST_RANK && p.label_is_logits);
      // (stage B needs the labels' totals alone; labels taken as they are have none)
      if ((edge == 0 ? ostart : (oend && !whole)) && (STAGE == 2 || q == 1) && (q != 1 || normed)) {
        int h0 = g;
        if (edge == 0) {  // the chunk its session's head lies in: the nearest one before that is not one segment
          h0 = g - 1;
          while (h0 > 0 && (reinterpret_cast<const int*>(s_car)[h0 * kLwtCarry + kLwtFlags] & kLwtWhole)) --h0;
        }
        if (pair) {
          lw_fold<true>(s_car, G, h0, q, r0, r1);
        } else {
          lw_fold<false>(s_car, G, h0, q, r0, r1);
        }
      }
      s_edge[edge][q][0] = r0;
      s_edge[edge][q][1] = r1;
    } else if (tid == 6) {
      int S = 0;
      for (int h = 0; h < G; ++h) S += reinterpret_cast<const int*>(s_car)[h * kLwtCarry + kLwtHeads];
      s_S = S;
    }
    __syncthreads();
  }
  // which total a position takes: 0 its local segment's, 1 the start session's, 2 the end session's
  int from[E];
#pragma unroll
  for (int e = 0; e < E; ++e) from[e] = (ostart && sid[e] == 0) ? 1 : ((oend && sid[e] == nseg - 1) ? 2 : 0);

  // ---- the operands in the reference's order
  const bool scaled = scale_w != nullptr;
  const float w = scaled ? scale_w[0] : 1.f, wa = fabsf(w), b = scaled ? scale_b[0] : 0.f;
  const bool cool = p.temperature != 1.f;
  const float ninf = -INFINITY;
  const bool soft = p.kind == ER_LIST_RANK && p.label_is_logits;
  const bool normed = soft || p.kind == ER_LIST_DISTILL;
  float zz[E], a[E], t[E], v[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    zz[e] = 0.f; a[e] = ninf; t[e] = 0.f;
    if (e < nv) {
      zz[e] = z[id[e] * ldz];
      float aa = scaled ? zz[e] * wa + b : zz[e];
      if (cool) aa = aa / p.temperature;
      a[e] = aa;
      float yl = y[id[e]];
      if (!p.label_ready) {
        if (p.kind == ER_LIST_DISTILL) {
          yl = fminf(fmaxf(yl, 1.f), p.clip_max);
          yl = log1pf(p.clip_max) - logf(yl);
        } else if (cool && p.label_is_logits) {
          yl = yl / p.temperature;
        }
      }
      t[e] = yl;
    }
  }
  const bool first = tid == 0, final = tid == kLwThreads - 1;  // the lanes that hold the leading and the trailing segment
  float* mine = carry + static_cast<size_t>(g) * kLwtCarry;

  // ---- slot 0: m_s and se_s (stages A and C)
  float am[E], ea[E];
  if constexpr (STAGE != 1) {
    float lm[E];
#pragma unroll
    for (int e = 0; e < E; ++e) v[e] = a[e];
    lwt_local<E, 1>(v, heads, tails, sid, nv, ninf, s_cv, s_cf, s_tot);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      lm[e] = v[e];
      v[e] = e < nv ? expf(a[e] - lm[e]) : 0.f;
    }
    lwt_local<E, 0>(v, heads, tails, sid, nv, 0.f, s_cv, s_cf, s_tot);
    if constexpr (STAGE == 0) {
      if (first) { mine[0] = lm[0]; mine[1] = v[0]; }
      if (final) { mine[2] = lm[E - 1]; mine[3] = v[E - 1]; }
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        am[e] = 0.f; ea[e] = 0.f;
        if (e < nv) {
          const float m = from[e] ? s_edge[from[e] - 1][0][0] : lm[e], se = from[e] ? s_edge[from[e] - 1][0][1] : v[e];
          am[e] = a[e] - m;
          ea[e] = expf(am[e]) / se;     // softmax
          am[e] = am[e] - logf(se);     // log softmax
        }
      }
    }
  }

  // ---- slot 1: the labels' totals; t: the labels' softmax, the labels over their session's sum, or the labels as they are
  if (normed) {
    float lm[E];
#pragma unroll
    for (int e = 0; e < E; ++e) lm[e] = 0.f;
    if (soft) {
#pragma unroll
      for (int e = 0; e < E; ++e) v[e] = e < nv ? t[e] : ninf;
      lwt_local<E, 1>(v, heads, tails, sid, nv, ninf, s_cv, s_cf, s_tot);
#pragma unroll
      for (int e = 0; e < E; ++e) lm[e] = v[e];
    }
#pragma unroll
    for (int e = 0; e < E; ++e) v[e] = e < nv ? (soft ? expf(t[e] - lm[e]) : t[e]) : 0.f;
    lwt_local<E, 0>(v, heads, tails, sid, nv, 0.f, s_cv, s_cf, s_tot);
    if constexpr (STAGE == 0) {
      // (a pair as (max, sum); a plain sum in the first word, where lw_fold<false> adds)
      if (first) { mine[4] = soft ? lm[0] : v[0]; mine[5] = soft ? v[0] : 0.f; }
      if (final) { mine[6] = soft ? lm[E - 1] : v[E - 1]; mine[7] = soft ? v[E - 1] : 0.f; }
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        if (e < nv) {
          // (a sum lies in the fold's first word, a pair's sum in its second)
          const float m = from[e] ? s_edge[from[e] - 1][1][0] : lm[e];
          const float sy = from[e] ? s_edge[from[e] - 1][1][soft ? 1 : 0] : v[e];
          t[e] = soft ? expf(t[e] - m) / sy : t[e] / sy;
        }
      }
    }
  }
  if constexpr (STAGE == 0) {
    if (first) {
      reinterpret_cast<int*>(mine)[kLwtFlags] = (whole ? kLwtWhole : 0) | (ostart ? kLwtOpenStart : 0) | (oend ? kLwtOpenEnd : 0);
      reinterpret_cast<int*>(mine)[kLwtHeads] = nseg - (ostart ? 1 : 0);
    }
    return;
  }

  // ---- slot 2: T_s
#pragma unroll
  for (int e = 0; e < E; ++e) v[e] = t[e];
  lwt_local<E, 0>(v, heads, tails, sid, nv, 0.f, s_cv, s_cf, s_tot);
  if constexpr (STAGE == 1) {
    if (first) { mine[8] = v[0]; mine[9] = 0.f; }
    if (final) { mine[10] = v[E - 1]; mine[11] = 0.f; }
    return;
  }

  // ---- the loss, the gradients
  if constexpr (STAGE == 2) {
    const int S = s_S;
    const float c = p.loss_scale / static_cast<float>(S);
    float lsum = 0.f, gz = 0.f, gs = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (e < nv) {
        const float Ts = from[e] ? s_edge[from[e] - 1][2][0] : v[e];
        lsum = lsum + t[e] * am[e];
        float gi = c * (Ts * ea[e] - t[e]);
        if (cool) gi = gi / p.temperature;
        gz = gz + gi * zz[e];
        gs = gs + gi;
        if (dz) dz[id[e] * lddz] = scaled ? gi * wa : gi;
      }
    }
    lsum = wave_sum(lsum);
    gz = wave_sum(gz);
    gs = wave_sum(gs);
    if ((tid & (kWave - 1)) == 0) {
      s_red[tid / kWave] = lsum;
      s_red[kLwWaves + tid / kWave] = gz;
      s_red[2 * kLwWaves + tid / kWave] = gs;
    }
    __syncthreads();
    if (tid == 0) {
      float r[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        r[q] = 0.f;
        for (int u = 0; u < kLwWaves; ++u) r[q] = r[q] + s_red[q * kLwWaves + u];
      }
      if (loss_partials) loss_partials[g] = p.loss_scale * (-r[0] / static_cast<float>(S));
      if (scale_partials) {
        scale_partials[2 * g] = (w > 0.f ? 1.f : (w < 0.f ? -1.f : 0.f)) * r[1];
        scale_partials[2 * g + 1] = r[2];
      }
      if (num_sessions && g == 0) num_sessions[0] = S;
    }
  }
}

struct LwtArgs {  // (host only: what the three stages share)
  const float* z; int64_t ldz; const float* y; const int64_t* skey; const int32_t* sidx; int B, G;
  LwParam p; const float* sw; const float* sb; float* carry; float* loss_partials; float* dz; int64_t lddz;
  float* scale_partials; int32_t* num_sessions;
};

template <int E>
static int lwt_reduce(const LwtArgs& a, er_stream_t stream) {
  hipLaunchKernelGGL((listwise_tiled_reduce_kernel<E, 0>), dim3(a.G), dim3(kLwThreads), 0, as_stream(stream), a.z, a.ldz, a.y,
                     a.skey, a.sidx, a.B, a.p, a.sw, a.sb, a.carry, a.loss_partials, a.dz, a.lddz, a.scale_partials,
                     a.num_sessions);
  ER_LAUNCH_CHECK();
  hipLaunchKernelGGL((listwise_tiled_reduce_kernel<E, 1>), dim3(a.G), dim3(kLwThreads), 0, as_stream(stream), a.z, a.ldz, a.y,
                     a.skey, a.sidx, a.B, a.p, a.sw, a.sb, a.carry, a.loss_partials, a.dz, a.lddz, a.scale_partials,
                     a.num_sessions);
  ER_LAUNCH_CHECK();
  hipLaunchKernelGGL((listwise_tiled_reduce_kernel<E, 2>), dim3(a.G), dim3(kLwThreads), 0, as_stream(stream), a.z, a.ldz, a.y,
                     a.skey, a.sidx, a.B, a.p, a.sw, a.sb, a.carry, a.loss_partials, a.dz, a.lddz, a.scale_partials,
                     a.num_sessions);
  ER_LAUNCH_CHECK();
  return 0;
}

// the workspace: key [2][G T] int64 | index [2][G T] int32 | carry [G][16] words
inline int64_t lwt_workspace_bytes(int64_t B, int tile) {
  const int T = lwt_tile(B, tile);
  if (T == 0) return 0;
  const int64_t G = ceil_div(B, T);
  return G * T * 2 * kLwRecordBytes + G * kLwtCarry * 4;
}

int lwt_sort(const int64_t* keys, int B, int T, int64_t* const key[2], int32_t* const idx[2], er_stream_t stream, int* cur) {
  const int G = static_cast<int>(ceil_div(B, T)), NP = G * T;
  // more than 64 KB of dynamic LDS is opted in to once per kernel (no stream work: safe inside a capture)
  static bool opted = false;
  const int lds = T * kLwRecordBytes;
  if (lds > kLwPlainLds && !opted) {
    ER_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(listwise_tile_sort_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, kLwMaxB * kLwRecordBytes));
    ER_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(listwise_merge_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, kLwMaxB * kLwRecordBytes));
    opted = true;
  }
  hipLaunchKernelGGL(listwise_tile_sort_kernel, dim3(G), dim3(kLwThreads), static_cast<size_t>(lds), as_stream(stream), keys,
                     B, T, key[0], idx[0]);
  ER_LAUNCH_CHECK();
  int c = 0;
  for (int L = T; L < NP; L <<= 1) {  // ceil(log2 G) passes
    hipLaunchKernelGGL(listwise_merge_kernel, dim3(G), dim3(kLwThreads), static_cast<size_t>(lds), as_stream(stream), key[c],
                       idx[c], NP, L, T, key[c ^ 1], idx[c ^ 1]);
    ER_LAUNCH_CHECK();
    c ^= 1;
  }
  *cur = c;
  return 0;
}

}  // namespace er

extern "C" {

int32_t er_listwise_tiled_grid(int64_t B, int32_t tile) {
  const int T = er::lwt_tile(B, tile);
  return T > 0 ? static_cast<int32_t>(er::ceil_div(B, T)) : 0;
}

int64_t er_listwise_tiled_workspace_bytes(int64_t B, int32_t tile) { return er::lwt_workspace_bytes(B, tile); }

int er_listwise_tiled(const float* logits, int64_t ld_logits, const float* labels, const int64_t* session_keys, int64_t B,
                      int32_t kind, int32_t flags, float temperature, float label_clip_max, const float* scale_w,
                      const float* scale_b, float loss_scale, float* loss_partials, float* dlogits, int64_t ld_dlogits,
                      float* scale_partials, int32_t* num_sessions, int32_t tile, void* workspace, int64_t workspace_bytes,
                      er_stream_t stream) {
  const int T = er::lwt_tile(B, tile);
  ER_REQUIRE(T > 0, "er_listwise_tiled: B = %lld, tile = %d outside the envelope (tile 0: %d < B <= %d; tile 1024, 2048, "
             "4096 or 8192: 1 <= B <= %d)", static_cast<long long>(B), tile, er::kLwMaxB, er::kLwtMaxB, er::kLwtMaxB);
  ER_REQUIRE(logits && labels && session_keys, "er_listwise_tiled: logits, labels and session_keys are required");
  ER_REQUIRE(ld_logits >= 1 && ld_logits <= (1 << 20), "er_listwise_tiled: a logits pitch outside [1, 2^20]");
  ER_REQUIRE(!dlogits || (ld_dlogits >= 1 && ld_dlogits <= (1 << 20)), "er_listwise_tiled: a dlogits pitch outside [1, 2^20]");
  ER_REQUIRE(kind == ER_LIST_RANK || kind == ER_LIST_DISTILL, "er_listwise_tiled: kind %d", kind);
  ER_REQUIRE(temperature > 0.f, "er_listwise_tiled: temperature %g must be positive", static_cast<double>(temperature));
  ER_REQUIRE((scale_w == nullptr) == (scale_b == nullptr),
             "er_listwise_tiled: scale_w and scale_b come together or not at all");
  ER_REQUIRE(!scale_partials || scale_w, "er_listwise_tiled: scale_partials without scale_w / scale_b");
  const bool ready = (flags & ER_LIST_LABEL_READY) != 0;
  ER_REQUIRE(kind != ER_LIST_DISTILL || ready || label_clip_max >= 1.f, "er_listwise_tiled: label_clip_max %g below 1",
             static_cast<double>(label_clip_max));
  ER_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0 &&
                 workspace_bytes >= er::lwt_workspace_bytes(B, tile),
             "er_listwise_tiled: the workspace is missing, not 8-byte aligned or below %lld bytes",
             static_cast<long long>(er::lwt_workspace_bytes(B, tile)));
  const int G = static_cast<int>(er::ceil_div(B, T)), NP = G * T, Bi = static_cast<int>(B);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  int64_t* key[2] = {reinterpret_cast<int64_t*>(ws), reinterpret_cast<int64_t*>(ws) + NP};
  int32_t* idx[2] = {reinterpret_cast<int32_t*>(ws + static_cast<size_t>(NP) * 16),
                     reinterpret_cast<int32_t*>(ws + static_cast<size_t>(NP) * 16) + NP};
  float* carry = reinterpret_cast<float*>(ws + static_cast<size_t>(NP) * 24);
  int cur = 0;
  if (const int rc = er::lwt_sort(session_keys, Bi, T, key, idx, stream, &cur)) return rc;
  er::LwtArgs a;
  a.z = logits; a.ldz = ld_logits; a.y = labels; a.skey = key[cur]; a.sidx = idx[cur]; a.B = Bi; a.G = G;
  a.p.temperature = temperature; a.p.clip_max = label_clip_max; a.p.loss_scale = loss_scale;
  a.p.kind = kind;
  a.p.label_is_logits = (flags & ER_LIST_LABEL_IS_LOGITS) ? 1 : 0;
  a.p.label_ready = ready ? 1 : 0;
  a.sw = scale_w; a.sb = scale_b; a.carry = carry; a.loss_partials = loss_partials; a.dz = dlogits; a.lddz = ld_dlogits;
  a.scale_partials = scale_partials; a.num_sessions = num_sessions;
  switch (T / er::kLwThreads) {
    case 8: return er::lwt_reduce<8>(a, stream);
    case 4: return er::lwt_reduce<4>(a, stream);
    case 2: return er::lwt_reduce<2>(a, stream);
    default: return er::lwt_reduce<1>(a, stream);
  }
}

}  // extern "C"
