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

namespace er {

constexpr int kLwMaxB = 8192;
constexpr int kLwThreads = 1024;
constexpr int kLwWaves = kLwThreads / kWave;
constexpr int kLwRecordBytes = 12;     // int64 key + int32 index
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
