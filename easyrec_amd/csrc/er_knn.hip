// K9k: exact top-K item search over the whole corpus, and the hit count of the reference's hit-rate tool (reference
// tools/hit_rate_ds.py, utils/hit_rate_utils.py: g.search + batch_hitrate).  The semantics (scores, the total order, the
// empty slots, the hit rule) are stated in include/easyrec_hip.h next to er_knn_search; this file is three launches.
//
// knn_scan_kernel, grid = query tiles x item slices, 256 threads.  A workgroup keeps kKnnQT = 32 queries stationary in LDS
// and streams its slice of the item table in tiles of kKnnIT = 128 rows; both sit row-major at an even pitch P >= D (the
// columns D .. P - 1 zero), so that a float4 of the tile goes to LDS as two 8-byte stores.  An MFMA operand read is one
// dword per lane (row = lane & 31, column 2 t + (lane >> 5)); the LDS serves such a read in two groups of 32 lanes over 32
// banks, and within a group the addresses are row * P + const: with P even they reach 16 banks, so every operand read is
// a 2-way bank conflict.  (An odd pitch would be free of it at the price of dword staging stores; not measured, not built.)
// Wave w contracts the tile's rows 32 w .. 32 w + 31 (operand A) with the 32 queries (operand B) on
// v_mfma_f32_32x32x2_f32, two columns d = 2 t, 2 t + 1 per instruction in ascending t: bit for bit the fmaf chain over
// ascending d.  A lane then holds 16 scores of ONE query (column lane & 31 of the C tile) and compares them with that
// query's threshold, the score of its current K-th best.  A score that beats the threshold is appended to the query's
// candidate list in LDS behind an LDS atomic counter, as a 64-bit key (the score mapped to an order-preserving unsigned
// integer, above the complemented row) whose unsigned order IS the total order.  A list holds `cap` keys; at the start of
// a tile it holds at most cap - 128, so the 128 rows of a tile always fit.  Between two tiles a wave prunes the lists
// that grew past cap - 128: every key's rank (the number of better keys) is counted, ranks below K move to their rank's
// slot, the threshold becomes the score of rank K - 1.  Rows arrive in ascending order, so a later row with the
// threshold's score loses its tie against every kept key: "strictly better than the threshold" is exact.  WHICH keys are
// in a list at a barrier does not depend on the order of the appends, and the rank sort forgets that order, so the
// outputs are the same bits in every run, under every slice count and in a graph replay.
// The next tile's rows are loaded into registers before the current tile's MFMAs (D a multiple of 4; other D load
// between the barriers).
//
// knn_merge_kernel, one wave per query: lane s walks the sorted partial list of slice s; K times the wave takes the
// largest head key (a butterfly maximum), writes its id / row / distance and advances that lane.
// knn_hits_kernel, one wave per user: er_knn_hits.
#include "er_common.h"

namespace er {

constexpr int kKnnQT = 32;          // queries of a workgroup
constexpr int kKnnIT = 128;         // item rows of a tile: 32 per wave
constexpr int kKnnMaxD = 128;
constexpr int kKnnMaxK = 128;
constexpr int kKnnMaxSlices = 64;   // one lane of the merging wave per slice
constexpr int kKnnMaxCap = 384;     // six keys per lane in the prune
constexpr int kKnnLdsBudget = 152 * 1024;
constexpr int kKnnAutoGrid = 512;   // workgroups slices = 0 aims at: two per compute unit

typedef float knn_f32x16 __attribute__((ext_vector_type(16)));
typedef float knn_f32x4 __attribute__((ext_vector_type(4)));

// columns contracted = the row pitch in floats: even, >= D, P / 2 odd
__host__ __device__ inline int knn_pitch(int D) {
  int p = (D + 1) & ~1;
  if (((p >> 1) & 1) == 0) p += 2;
  return p;
}
__host__ __device__ inline int knn_cols(int D) { return knn_pitch(D); }
// keys a candidate list holds: 128 for the tile's rows + 2 K (at least 64) of slack between two prunes, at most what
// the budget leaves and what the prune's six keys per lane cover; never below 128 + K
__host__ __device__ inline int knn_cap(int D, int K) {
  const int fixed = 4 * (kKnnQT + kKnnIT) * knn_pitch(D) + 4 * kKnnIT + 8 * kKnnQT;
  int cap = kKnnIT + (2 * K > 64 ? 2 * K : 64);
  const int fit = (kKnnLdsBudget - fixed) / (8 * kKnnQT);
  if (cap > fit) cap = fit;
  if (cap > kKnnMaxCap) cap = kKnnMaxCap;
  return cap;
}
inline int64_t knn_lds_bytes(int D, int K) {
  if (D < 1 || D > kKnnMaxD || K < 1 || K > kKnnMaxK) return 0;
  return 4 * static_cast<int64_t>(kKnnQT + kKnnIT) * knn_pitch(D) + 4 * kKnnIT + 8 * kKnnQT +
         8 * static_cast<int64_t>(kKnnQT) * knn_cap(D, K);
}
inline int knn_query_tiles(int64_t nq) { return static_cast<int>(ceil_div(nq, kKnnQT)); }
// slices = 0: enough slices for kKnnAutoGrid workgroups, each of at least 16 tiles
inline int knn_auto_slices(int64_t nq, int64_t n) {
  int64_t s = ceil_div(kKnnAutoGrid, ceil_div(nq, kKnnQT));
  const int64_t most = n / (16 * kKnnIT);
  if (s > most) s = most;
  if (s > kKnnMaxSlices) s = kKnnMaxSlices;
  return s < 1 ? 1 : static_cast<int>(s);
}

// float -> unsigned, ascending; and back
__device__ __forceinline__ uint32_t knn_ord(float f) {
  const uint32_t u = __float_as_uint(f);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float knn_unord(uint32_t k) {
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}
// the key of (score, row): a larger key is a better place in the total order; never 0 (row < 2^31)
__device__ __forceinline__ uint64_t knn_key(float v, int row, int metric) {
  const uint32_t o = knn_ord(v);
  return (static_cast<uint64_t>(metric ? o : ~o) << 32) | (0xFFFFFFFFu - static_cast<uint32_t>(row));
}
__device__ __forceinline__ float knn_key_value(uint64_t key, int metric) {
  const uint32_t hi = static_cast<uint32_t>(key >> 32);
  return knn_unord(metric ? hi : ~hi);
}
__device__ __forceinline__ int knn_key_row(uint64_t key) {
  return static_cast<int>(0xFFFFFFFFu - static_cast<uint32_t>(key & 0xFFFFFFFFull));
}

// rows [r0, r0 + nrows) of src [n, D] -> tile at pitch P, rows at or past `end` and the columns D .. P - 1 zero
__device__ __forceinline__ void knn_stage_rows(const float* __restrict__ src, int64_t end, int64_t r0, int nrows, int D,
                                               int P, float* tile) {
  for (int t = threadIdx.x; t < nrows * P; t += kBlock) {
    const int r = t / P, d = t - r * P;
    const int64_t row = r0 + r;
    tile[t] = (row < end && d < D) ? src[row * D + d] : 0.f;
  }
}

// one wave sorts list [0, c) of one query by rank and keeps the ranks below K: -> the new count; thr (may be null)
// receives the score of rank K - 1
__device__ __forceinline__ int knn_prune(uint64_t* list, int c, int K, int metric, float* thr, int lane) {
  constexpr int U = kKnnMaxCap / kWave;
  uint64_t mine[U];
  int rank[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int e = lane + u * kWave;
    mine[u] = e < c ? list[e] : 0ull;
    rank[u] = 0;
  }
  for (int j = 0; j < c; ++j) {
    const uint64_t kj = list[j];  // (the same address in every lane: a broadcast)
#pragma unroll
    for (int u = 0; u < U; ++u) rank[u] += kj > mine[u];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int e = lane + u * kWave;
    if (e < c && rank[u] < K) {
      list[rank[u]] = mine[u];
      if (thr && rank[u] == K - 1) *thr = knn_key_value(mine[u], metric);
    }
  }
  return c < K ? c : K;
}

struct KnnArgs {
  const float* Q;      // [nq, D]
  const float* X;      // [n, D]
  const float* xx;     // [n] (metric 0)
  int64_t nq, n, slice_len;
  int D, K, metric, cap;
};

// NV > 0: D % 4 == 0 and D <= 8 NV: a thread carries NV float4 of the next tile in registers.  NV == 0: any D.
template <int NV>
__global__ __launch_bounds__(kBlock) void knn_scan_kernel(KnnArgs a, uint64_t* __restrict__ partial) {
  extern __shared__ __align__(16) unsigned char knn_lds[];
  const int D = a.D, K = a.K, P = knn_pitch(D), DC = knn_cols(D), cap = a.cap, metric = a.metric;
  float* Qs = reinterpret_cast<float*>(knn_lds);                        // [kKnnQT, P]
  float* Xs = Qs + kKnnQT * P;                                          // [kKnnIT, P]
  float* xxs = Xs + kKnnIT * P;                                         // [kKnnIT]
  float* thr = xxs + kKnnIT;                                            // [kKnnQT]
  int* cnt = reinterpret_cast<int*>(thr + kKnnQT);                      // [kKnnQT]
  uint64_t* lists = reinterpret_cast<uint64_t*>(cnt + kKnnQT);          // [kKnnQT, cap]
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int half = lane >> 5, col = lane & 31;
  const int64_t q0 = static_cast<int64_t>(blockIdx.x) * kKnnQT;
  const int slice = blockIdx.y;
  int64_t beg = slice * a.slice_len, end = beg + a.slice_len;
  if (beg > a.n) beg = a.n;
  if (end > a.n) end = a.n;

  knn_stage_rows(a.Q, a.nq, q0, kKnnQT, D, P, Qs);
  if (tid < kKnnQT) {
    thr[tid] = __uint_as_float(0x7FC00000u);  // NaN: no threshold yet, every score is taken
    cnt[tid] = 0;
  }
  const int nvec = kKnnIT * D / 4;  // float4 of a tile (NV > 0)
  knn_f32x4 pre[NV > 0 ? NV : 1];
  // a tile's rows are contiguous in memory: float4 number idx of the tile is 4 idx floats past its first row; where it
  // lands in LDS does not change from tile to tile
  int dst_off[NV > 0 ? NV : 1];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int idx = tid + v * kBlock;
    const int r = idx / (D / 4);
    dst_off[v] = idx < nvec ? r * P + 4 * (idx - r * (D / 4)) : -1;
  }
  auto fetch = [&](int64_t r0) {
    const int64_t live = (end - r0) * D;  // floats of the tile that exist
    const float* src = a.X + r0 * D;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int idx = tid + v * kBlock;
      knn_f32x4 z = {0.f, 0.f, 0.f, 0.f};
      if (dst_off[v] >= 0 && 4 * static_cast<int64_t>(idx) < live) z = *reinterpret_cast<const knn_f32x4*>(src + 4 * idx);
      pre[v] = z;
    }
  };
  auto stage = [&](int64_t r0) {
    if (NV > 0) {
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        if (dst_off[v] >= 0) {
          float* dst = Xs + dst_off[v];  // (P is even: 8-byte aligned)
          *reinterpret_cast<float2*>(dst) = make_float2(pre[v][0], pre[v][1]);
          *reinterpret_cast<float2*>(dst + 2) = make_float2(pre[v][2], pre[v][3]);
        }
      }
    } else {
      knn_stage_rows(a.X, end, r0, kKnnIT, D, P, Xs);
    }
    if (metric == 0 && tid < kKnnIT) xxs[tid] = r0 + tid < end ? a.xx[r0 + tid] : 0.f;
  };
  if (NV > 0) {
    for (int t = tid; t < kKnnIT * (P - D); t += kBlock) {  // the pad columns, once: no tile writes them
      const int r = t / (P - D);
      Xs[r * P + D + (t - r * (P - D))] = 0.f;
    }
  }
  if (NV > 0) fetch(beg);
  __syncthreads();  // Qs
  float qq = 0.f;
  if (metric == 0) {
    const float* qrow = Qs + col * P;
    for (int d = 0; d < D; ++d) qq = fmaf(qrow[d], qrow[d], qq);
  }
  stage(beg);
  __syncthreads();

  const float* ap = Xs + (wave * 32 + col) * P + half;
  const float* bp = Qs + col * P + half;
  const bool q_live = q0 + col < a.nq;
  uint64_t* my_list = lists + col * cap;
  for (int64_t r0 = beg; r0 < end; r0 += kKnnIT) {
    if (NV > 0 && r0 + kKnnIT < end) fetch(r0 + kKnnIT);
    knn_f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    int d = 0;
    for (; d + 8 <= DC; d += 8) {
      float av[4], bv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        av[i] = ap[d + 2 * i];
        bv[i] = bp[d + 2 * i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[i], acc, 0, 0, 0);
    }
    for (; d < DC; d += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[d], bp[d], acc, 0, 0, 0);
    // C tile: column = lane & 31 (the query), row = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5) (the item of this wave)
    const float t = thr[col];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int ir = wave * 32 + (i & 3) + 8 * (i >> 2) + 4 * half;
      float v = acc[i] + 0.f;  // (-0 -> +0: one key per value)
      bool better;
      if (metric) {
        better = !(v <= t);
      } else {
        v = fmaxf(0.f, (qq + xxs[ir]) - 2.f * v);
        better = !(v >= t);
      }
      if (better && q_live && r0 + ir < end) {
        const int pos = atomicAdd(&cnt[col], 1);
        if (pos < cap) my_list[pos] = knn_key(v, static_cast<int>(r0 + ir), metric);
      }
    }
    __syncthreads();  // every append is in, every operand read is done
    if (r0 + kKnnIT < end) stage(r0 + kKnnIT);
    // lane q reads query q's count; the wave prunes its share (q % 4 == wave) of the lists that grew past cap - 128
    const int c_lane = lane < kKnnQT ? cnt[lane] : 0;
    unsigned long long grown = __ballot(c_lane > cap - kKnnIT && (lane & (kBlock / kWave - 1)) == wave);
    while (grown) {  // (wave-uniform)
      const int q = __ffsll(grown) - 1;
      grown &= grown - 1;
      const int c = __shfl(c_lane, q, kWave);
      const int kept = knn_prune(lists + q * cap, c < cap ? c : cap, K, metric, thr + q, lane);
      if (lane == 0) cnt[q] = kept;
    }
    __syncthreads();
  }
  // the slice's sorted list of every query: [slice, query, K], empty places key 0
  for (int q = wave; q < kKnnQT; q += kBlock / kWave) {
    if (q0 + q >= a.nq) continue;
    uint64_t* list = lists + q * cap;
    const int c = cnt[q] < cap ? cnt[q] : cap;
    const int kept = knn_prune(list, c, K, metric, nullptr, lane);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    uint64_t* out = partial + (static_cast<int64_t>(slice) * a.nq + q0 + q) * K;
    for (int k = lane; k < K; k += kWave) out[k] = k < kept ? list[k] : 0ull;
  }
}

// xx[r] = the fmaf chain over x_d^2
__global__ __launch_bounds__(kBlock) void knn_norms_kernel(const float* __restrict__ X, int64_t n, int D,
                                                           float* __restrict__ xx) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (r >= n) return;
  const float* x = X + r * D;
  float s = 0.f;
  for (int d = 0; d < D; ++d) s = fmaf(x[d], x[d], s);
  xx[r] = s;
}

__device__ __forceinline__ uint64_t knn_wave_max(uint64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t lo = __shfl_xor(static_cast<uint32_t>(v), off, 64);
    const uint32_t hi = __shfl_xor(static_cast<uint32_t>(v >> 32), off, 64);
    const uint64_t o = (static_cast<uint64_t>(hi) << 32) | lo;
    v = o > v ? o : v;
  }
  return v;
}

// one wave per query, four queries per workgroup
__global__ __launch_bounds__(kBlock) void knn_merge_kernel(const uint64_t* __restrict__ partial,
                                                           const int64_t* __restrict__ table_ids, int64_t nq, int K,
                                                           int slices, int metric, int64_t* __restrict__ out_ids,
                                                           int32_t* __restrict__ out_rows, float* __restrict__ out_dist) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t q = static_cast<int64_t>(blockIdx.x) * (kBlock / kWave) + threadIdx.x / kWave;
  if (q >= nq) return;
  const uint64_t* mine = lane < slices ? partial + (static_cast<int64_t>(lane) * nq + q) * K : nullptr;
  int head = 0;
  uint64_t key = mine ? mine[0] : 0ull;
  for (int k = 0; k < K; ++k) {
    const uint64_t best = knn_wave_max(key);
    if (lane == 0) {
      const int64_t o = q * K + k;
      if (best) {
        const int row = knn_key_row(best);
        out_ids[o] = table_ids[row];
        if (out_rows) out_rows[o] = row;
        out_dist[o] = knn_key_value(best, metric);
      } else {
        out_ids[o] = -1;
        if (out_rows) out_rows[o] = -1;
        out_dist[o] = metric ? -INFINITY : INFINITY;
      }
    }
    if (best && key == best) {  // (keys are unique: one lane)
      ++head;
      key = head < K ? mine[head] : 0ull;
    }
  }
}

// one wave per user; a lane tests one element of the list: a rescan of the elements before it (is it the first of its
// value?), then of the counted ids - len^2 / 2 + len * I * K reads per user, for lists of tens of ids
__global__ __launch_bounds__(kBlock) void knn_hits_kernel(const int64_t* __restrict__ ids, const int32_t* __restrict__ emb_num,
                                                          const int64_t* __restrict__ off, const int64_t* __restrict__ gt,
                                                          int64_t U, int I, int K, int32_t* __restrict__ hits,
                                                          int32_t* __restrict__ gt_count) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t u = static_cast<int64_t>(blockIdx.x) * (kBlock / kWave) + threadIdx.x / kWave;
  if (u >= U) return;
  const int64_t g0 = off[u], len = off[u + 1] - g0;
  int counted = emb_num[u];
  counted = counted < 0 ? 0 : (counted > I ? I : counted);
  const int64_t* mine = ids + u * I * K;
  const int m = counted * K;
  int total = 0;
  for (int64_t gb = 0; gb < len; gb += kWave) {  // (wave-uniform trip count)
    const int64_t g = gb + lane;
    bool hit = false;
    if (g < len) {
      const int64_t id = gt[g0 + g];
      bool first = true;
      for (int64_t e = 0; e < g; ++e) first = first && gt[g0 + e] != id;
      if (first)
        for (int j = 0; j < m; ++j) hit = hit || mine[j] == id;
    }
    total += __popcll(__ballot(hit));
  }
  if (lane == 0) {
    hits[u] = total;
    gt_count[u] = static_cast<int32_t>(len);
  }
}

static int g_knn_lds[4] = {0, 0, 0, 0};  // (per process: one device per process, one launching thread - see er_capsule.hip)

template <int NV>
static int knn_launch_scan(const KnnArgs& a, int qtiles, int slices, int64_t bytes, uint64_t* partial, int slot,
                           hipStream_t stream) {
  const void* fn = reinterpret_cast<const void*>(knn_scan_kernel<NV>);
  if (bytes > 65536 && bytes > g_knn_lds[slot]) {  // (no stream work: safe inside a capture)
    ER_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes)));
    g_knn_lds[slot] = static_cast<int>(bytes);
  }
  hipLaunchKernelGGL(knn_scan_kernel<NV>, dim3(qtiles, slices), dim3(kBlock), static_cast<size_t>(bytes), stream, a,
                     partial);
  ER_LAUNCH_CHECK();
  return 0;
}

}  // namespace er

extern "C" {

int32_t er_knn_query_tile(void) { return er::kKnnQT; }
int32_t er_knn_item_tile(void) { return er::kKnnIT; }

int64_t er_knn_lds_bytes(int32_t D, int32_t K) { return er::knn_lds_bytes(D, K); }

int64_t er_knn_workspace_bytes(int64_t nq, int32_t K, int32_t slices) {
  if (nq < 1 || K < 1 || K > er::kKnnMaxK || slices < 0 || slices > er::kKnnMaxSlices) return 0;
  // slices = 0: the most er_knn_search chooses for nq queries, whatever n is
  const int64_t s = slices ? slices : er::knn_auto_slices(nq, INT64_MAX);
  return 8 * s * nq * K;
}

int er_knn_norms(const float* items, int64_t n, int32_t D, float* xx, er_stream_t stream) {
  ER_REQUIRE(items && xx && n >= 1 && n <= 0x7fffffffll && D >= 1 && D <= er::kKnnMaxD,
             "er_knn_norms: need 1 <= n < 2^31, 1 <= D <= %d (n %lld, D %d)", er::kKnnMaxD, static_cast<long long>(n), D);
  hipLaunchKernelGGL(er::knn_norms_kernel, dim3(static_cast<unsigned>(er::ceil_div(n, er::kBlock))), dim3(er::kBlock), 0,
                     er::as_stream(stream), items, n, D, xx);
  ER_LAUNCH_CHECK();
  return 0;
}

int er_knn_search(const float* Q, const float* items, const float* xx, const int64_t* table_ids, int64_t nq, int64_t n,
                  int32_t D, int32_t K, int32_t metric, int32_t slices, void* workspace, int64_t* out_ids,
                  int32_t* out_rows, float* out_dist, er_stream_t stream) {
  const int64_t bytes = er::knn_lds_bytes(D, K);
  ER_REQUIRE(bytes > 0, "er_knn_search: D %d, K %d outside the envelope 1 .. %d, 1 .. %d", D, K, er::kKnnMaxD,
             er::kKnnMaxK);
  // (nq: the merge launch's grid, one workgroup per four queries, is the narrower of the two)
  ER_REQUIRE(nq >= 1 && nq <= 4ll * 0x7fffffffll && n >= 1 && n <= 0x7fffffffll,
             "er_knn_search: need 1 <= nq < 2^33, 1 <= n < 2^31 (nq %lld, n %lld)", static_cast<long long>(nq),
             static_cast<long long>(n));
  ER_REQUIRE(metric == 0 || metric == 1, "er_knn_search: metric %d (0: l2, 1: inner product)", metric);
  ER_REQUIRE(slices >= 0 && slices <= er::kKnnMaxSlices, "er_knn_search: %d slices, at most %d", slices,
             er::kKnnMaxSlices);
  ER_REQUIRE(Q && items && table_ids && workspace && out_ids && out_dist && (metric == 1 || xx),
             "er_knn_search: null argument");
  const int S = slices ? slices : er::knn_auto_slices(nq, n);
  er::KnnArgs a;
  a.Q = Q; a.X = items; a.xx = xx;
  a.nq = nq; a.n = n; a.slice_len = er::ceil_div(n, S);
  a.D = D; a.K = K; a.metric = metric; a.cap = er::knn_cap(D, K);
  const int qtiles = er::knn_query_tiles(nq);
  uint64_t* partial = static_cast<uint64_t*>(workspace);
  hipStream_t st = er::as_stream(stream);
  const bool vec = D % 4 == 0 && (reinterpret_cast<uintptr_t>(items) & 15) == 0;
  int rc;
  if (!vec) rc = er::knn_launch_scan<0>(a, qtiles, S, bytes, partial, 0, st);
  else if (D <= 32) rc = er::knn_launch_scan<4>(a, qtiles, S, bytes, partial, 1, st);
  else if (D <= 64) rc = er::knn_launch_scan<8>(a, qtiles, S, bytes, partial, 2, st);
  else rc = er::knn_launch_scan<16>(a, qtiles, S, bytes, partial, 3, st);
  if (rc) return rc;
  hipLaunchKernelGGL(er::knn_merge_kernel, dim3(static_cast<unsigned>(er::ceil_div(nq, er::kBlock / er::kWave))),
                     dim3(er::kBlock), 0, st, partial, table_ids, nq, K, S, metric, out_ids, out_rows, out_dist);
  ER_LAUNCH_CHECK();
  return 0;
}

int er_knn_hits(const int64_t* out_ids, const int32_t* user_emb_num, const int64_t* gt_offsets, const int64_t* gt_ids,
                int64_t U, int32_t I, int32_t K, int32_t* hits, int32_t* gt_count, er_stream_t stream) {
  ER_REQUIRE(out_ids && user_emb_num && gt_offsets && hits && gt_count, "er_knn_hits: null argument");
  ER_REQUIRE(U >= 1 && I >= 1 && K >= 1, "er_knn_hits: need U, I, K >= 1 (U %lld, I %d, K %d)", static_cast<long long>(U),
             I, K);
  hipLaunchKernelGGL(er::knn_hits_kernel, dim3(static_cast<unsigned>(er::ceil_div(U, er::kBlock / er::kWave))),
                     dim3(er::kBlock), 0, er::as_stream(stream), out_ids, user_emb_num, gt_offsets, gt_ids, U, I, K, hits,
                     gt_count);
  ER_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
