// K1b: negative_sampler_in_memory on the device (reference core/sampler.py:425-454 `_get_impl`, input/input.py:823-845):
// N rows of the resident item table, uniform without replacement, none of them an item of the batch, appended to every
// attribute column of the batch.  The semantics (the permutation P, the walk, the exclusion) are stated in
// include/easyrec_hip.h next to er_neg_sample; this file is one launch: one workgroup draws, and ceil(B / 1024) more copy the
// batch's own values into [0, B) of the extended columns meanwhile (that half needs nothing of the draw).  The drawing one:
//   1. the batch's B ids into an open-addressing set in LDS (capacity 2^c >= 2 B, home slot mix64(id), linear probing;
//      the compare-and-swap decides only WHERE an id lies, never whether it is a member, so the draw does not depend on
//      the insertion order),
//   2. the candidates P(0), P(1), .. in chunks of the block size: each lane computes one candidate and tests its id, the
//      kept ones are compacted in order of k by a wave ballot plus a prefix over the 16 wave counts in LDS, until N are
//      kept,
//   3. after a barrier, [B, B + N) of every extended column = table_col[sel[j]], a lane loading its row of all columns
//      (eight at a time) before it stores any: the table is far larger than the caches, every load is a miss.
// Nothing here is ordered by timing: two runs and a graph replay give the same bits.  The step is read from the device
// counter, so a replayed graph draws fresh rows.
// K1c, negative_sampler's weighted draw with replacement (er_neg_sample_weighted), follows it below and shares the set,
// the column records and samp_copy_row.
#include "er_common.h"

namespace er {

constexpr int kSampThreads = 1024;
constexpr int kSampWaves = kSampThreads / kWave;
constexpr int kSampMaxB = 4096;
constexpr int kSampMaxCols = 32;
constexpr unsigned long long kSampEmpty = 0x8000000000000000ull;  // INT64_MIN: a batch id of that value is flagged apart

__host__ __device__ inline int samp_capacity(int B) {
  int cap = 64;
  while (cap < 2 * B) cap <<= 1;
  return cap;
}
inline int64_t samp_lds_bytes(int B) {
  if (B < 1 || B > kSampMaxB) return 0;
  return 8 * static_cast<int64_t>(samp_capacity(B)) + 4 * (kSampWaves + 16);
}

struct SampCols {
  const void* table[kSampMaxCols];
  const void* batch[kSampMaxCols];
  void* out[kSampMaxCols];
  uint32_t wide;  // bit c: column c holds 8-byte elements (int64 ids), else 4-byte ones (float values)
  int32_t ncols;
};

struct SampKeys {
  uint64_t key[4];
  uint64_t mask;
  int h;
};

// P(k) on [0, n): a four-round Feistel network over 2 h bits, walked until it lands below n
__host__ __device__ __forceinline__ uint64_t samp_perm(uint64_t k, uint64_t n, const SampKeys& s) {
  uint64_t x = k;
  do {
    uint64_t L = x >> s.h, R = x & s.mask;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint64_t t = L ^ (mix64(s.key[r] ^ R) & s.mask);
      L = R;
      R = t;
    }
    x = (L << s.h) | R;
  } while (x >= n);
  return x;
}

__host__ __device__ inline SampKeys samp_keys(uint64_t seed, uint64_t step, uint64_t n) {
  SampKeys s;
  int bits = 0;
  for (uint64_t v = n - 1; v; v >>= 1) ++bits;
  if (bits < 2) bits = 2;
  s.h = (bits + 1) / 2;
  s.mask = (1ull << s.h) - 1;
  const uint64_t base = mix64(seed ^ mix64(step));
  for (int r = 0; r < 4; ++r) s.key[r] = mix64(base + static_cast<uint64_t>(r) * 0xD1B54A32D192ED03ull);
  return s;
}

// out_c[j] = src_c[r] for every column c, src = the table's columns or the batch's: the loads of (up to) eight columns
// are issued before the first store, so one element per column is in flight per lane instead of one in all
constexpr int kSampColGroup = 8;
__device__ __forceinline__ void samp_copy_row(const SampCols& cols, bool from_table, int64_t r, int64_t j) {
  for (int c0 = 0; c0 < cols.ncols; c0 += kSampColGroup) {
    uint64_t v[kSampColGroup];
#pragma unroll
    for (int u = 0; u < kSampColGroup; ++u) {
      const int c = c0 + u;
      if (c < cols.ncols) {
        const void* src = from_table ? cols.table[c] : cols.batch[c];
        v[u] = ((cols.wide >> c) & 1u) ? static_cast<const uint64_t*>(src)[r] : static_cast<const uint32_t*>(src)[r];
      }
    }
#pragma unroll
    for (int u = 0; u < kSampColGroup; ++u) {
      const int c = c0 + u;
      if (c < cols.ncols) {
        if ((cols.wide >> c) & 1u) static_cast<uint64_t*>(cols.out[c])[j] = v[u];
        else static_cast<uint32_t*>(cols.out[c])[j] = static_cast<uint32_t>(v[u]);
      }
    }
  }
}

// grid = 1 + ceil(B / kSampThreads): workgroup 0 draws and gathers [B, B + N); the others copy the batch's own values
// into [0, B) meanwhile (they need nothing of the draw)
__global__ void __launch_bounds__(kSampThreads) neg_sample_kernel(
    const int64_t* __restrict__ table_ids, int64_t n, const int64_t* __restrict__ batch_ids, int B, int N,
    const int64_t* __restrict__ step, int64_t step_offset, uint64_t seed, int cap, SampCols cols,
    int32_t* __restrict__ sel) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  if (blockIdx.x > 0) {
    const int stride = (gridDim.x - 1) * kSampThreads;
    for (int j = (blockIdx.x - 1) * kSampThreads + tid; j < B; j += stride) samp_copy_row(cols, false, j, j);
    return;
  }
  extern __shared__ __align__(8) unsigned char samp_lds[];
  unsigned long long* set = reinterpret_cast<unsigned long long*>(samp_lds);
  int* wcount = reinterpret_cast<int*>(set + cap);  // [kSampWaves]
  int* has_empty = wcount + kSampWaves;             // [1]: the batch holds the id that doubles as the empty mark
  const unsigned long long slot_mask = static_cast<unsigned long long>(cap - 1);

  // the first chunk of candidates needs nothing of the set: its rows and their ids are in flight while the set is built
  const SampKeys keys = samp_keys(seed, static_cast<uint64_t>(*step + step_offset), static_cast<uint64_t>(n));
  const int total = B + N;  // (the host checked B + N <= n: every k below is a distinct row)
  int32_t row = 0;
  unsigned long long id = 0;
  if (tid < total) {
    row = static_cast<int32_t>(samp_perm(static_cast<uint64_t>(tid), static_cast<uint64_t>(n), keys));
    id = static_cast<unsigned long long>(table_ids[row]);
  }
  // this lane's batch ids (B <= kSampMaxB: at most four), loaded while the set is cleared
  unsigned long long mine[kSampMaxB / kSampThreads];
#pragma unroll
  for (int u = 0; u < kSampMaxB / kSampThreads; ++u) {
    const int i = tid + u * kSampThreads;
    mine[u] = i < B ? static_cast<unsigned long long>(batch_ids[i]) : 0ull;
  }
  for (int i = tid; i < cap; i += kSampThreads) set[i] = kSampEmpty;
  if (tid == 0) *has_empty = 0;
  __syncthreads();
#pragma unroll
  for (int u = 0; u < kSampMaxB / kSampThreads; ++u) {
    if (tid + u * kSampThreads >= B) continue;
    const unsigned long long bid = mine[u];
    if (bid == kSampEmpty) {
      *has_empty = 1;
      continue;
    }
    unsigned long long slot = mix64(bid) & slot_mask;
    for (int probe = 0; probe < cap; ++probe) {  // (at most B < cap slots are ever taken: an empty one is found)
      const unsigned long long prev = atomicCAS(&set[slot], kSampEmpty, bid);
      if (prev == kSampEmpty || prev == bid) break;
      slot = (slot + 1) & slot_mask;
    }
  }
  __syncthreads();
  const bool empty_is_member = *has_empty != 0;

  int kept = 0;
  for (int k0 = 0; k0 < total && kept < N; k0 += kSampThreads) {
    const int k = k0 + tid;
    bool keep = false;
    if (k < total) {
      if (k0 > 0) {
        row = static_cast<int32_t>(samp_perm(static_cast<uint64_t>(k), static_cast<uint64_t>(n), keys));
        id = static_cast<unsigned long long>(table_ids[row]);
      }
      bool member = false;
      if (id == kSampEmpty) {
        member = empty_is_member;
      } else {
        unsigned long long slot = mix64(id) & slot_mask;
        for (int probe = 0; probe < cap; ++probe) {
          const unsigned long long cur = set[slot];
          if (cur == id) { member = true; break; }
          if (cur == kSampEmpty) break;
          slot = (slot + 1) & slot_mask;
        }
      }
      keep = !member;
    }
    const unsigned long long ballot = __ballot(keep);
    const int before_lane = __popcll(ballot & ((1ull << lane) - 1ull));
    if (lane == 0) wcount[wave] = __popcll(ballot);
    __syncthreads();
    int before_wave = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kSampWaves; ++w) {
      const int c = wcount[w];
      before_wave += w < wave ? c : 0;
      all += c;
    }
    const int pos = kept + before_wave + before_lane;
    if (keep && pos < N) sel[pos] = row;
    kept += all;      // (the same value in every thread: the loop's exit is uniform)
    __syncthreads();  // wcount is rewritten by the next chunk
  }
  // a table with duplicate ids (refused when the table is built) could leave fewer than N: row 0, never a stale index
  for (int j = (kept < N ? kept : N) + tid; j < N; j += kSampThreads) sel[j] = 0;
  __threadfence_block();
  __syncthreads();
  for (int j = tid; j < N; j += kSampThreads) samp_copy_row(cols, true, sel[j], static_cast<int64_t>(B) + j);
}

static int g_samp_lds = 0;  // (per process: one device per process, one launching thread - see er_capsule.hip)

// ---- K1c: negative_sampler, the weighted draw with replacement (include/easyrec_hip.h next to er_neg_sample_weighted).
// Every draw is independent, so there is no order to keep: one lane per draw, ceil(N / 256) drawing workgroups, each
// with its own copy of the batch-id set in LDS (the set of the kernel above), and a lane gathers the columns of the row
// it drew itself.  The chain of one draw is alias record -> table id -> column rows, each a miss at a table far larger
// than the caches, so what can be issued early is: the first attempt's alias record is in flight while the set is
// cleared, its id and its first eight columns (read before the id is judged: a first attempt is rejected with
// probability q, the batch's weight mass) while the set is filled.  A rejected lane goes on alone; the attempts and the
// walk behind them are bounded.
constexpr int kWsampThreads = 256;
constexpr int kWsampAttempts = 32;
constexpr int kWsampIdsPerLane = kSampMaxB / kWsampThreads;

inline int64_t wsamp_lds_bytes(int B) {
  if (B < 1 || B > kSampMaxB) return 0;
  return 8 * static_cast<int64_t>(samp_capacity(B)) + 16;
}

__device__ __forceinline__ bool samp_is_member(const unsigned long long* set, unsigned long long slot_mask,
                                               bool empty_is_member, unsigned long long id) {
  if (id == kSampEmpty) return empty_is_member;
  unsigned long long slot = mix64(id) & slot_mask;
  for (unsigned long long probe = 0; probe <= slot_mask; ++probe) {
    const unsigned long long cur = set[slot];
    if (cur == id) return true;
    if (cur == kSampEmpty) return false;
    slot = (slot + 1) & slot_mask;
  }
  return false;
}

// the two halves of samp_copy_row for columns [c0, c0 + kSampColGroup) of the table
__device__ __forceinline__ void samp_load_group(const SampCols& cols, int c0, int64_t r, uint64_t (&v)[kSampColGroup]) {
#pragma unroll
  for (int u = 0; u < kSampColGroup; ++u) {
    const int c = c0 + u;
    if (c < cols.ncols)
      v[u] = ((cols.wide >> c) & 1u) ? static_cast<const uint64_t*>(cols.table[c])[r]
                                     : static_cast<const uint32_t*>(cols.table[c])[r];
  }
}
__device__ __forceinline__ void samp_store_group(const SampCols& cols, int c0, int64_t j, const uint64_t (&v)[kSampColGroup]) {
#pragma unroll
  for (int u = 0; u < kSampColGroup; ++u) {
    const int c = c0 + u;
    if (c < cols.ncols) {
      if ((cols.wide >> c) & 1u) static_cast<uint64_t*>(cols.out[c])[j] = v[u];
      else static_cast<uint32_t*>(cols.out[c])[j] = static_cast<uint32_t>(v[u]);
    }
  }
}

// candidate row of (draw j, attempt a) from its alias record: (k, the record) in two steps so that the record's load
// can be issued apart from its use
__device__ __forceinline__ void wsamp_random(uint64_t base, int j, int a, uint64_t n, uint32_t* k, float* f) {
  const uint64_t r0 = mix64(base ^ mix64((static_cast<uint64_t>(j) << 32) | static_cast<uint64_t>(a)));
  const uint64_t r1 = mix64(r0 + 0xD1B54A32D192ED03ull);
  *k = static_cast<uint32_t>(__umul64hi(r0, n));
  *f = static_cast<float>(static_cast<uint32_t>(r1 >> 40)) * 0x1p-24f;
}
__device__ __forceinline__ uint32_t wsamp_row(uint64_t rec, uint32_t k, float f, uint64_t n) {
  const uint32_t alias = static_cast<uint32_t>(rec >> 32);
  if (f < __uint_as_float(static_cast<uint32_t>(rec))) return k;
  return alias < n ? alias : k;
}

// grid = D + C, D = ceil(N / 256) drawing workgroups, C = ceil(B / 256) that copy the batch's own values into [0, B)
__global__ void __launch_bounds__(kWsampThreads) neg_sample_weighted_kernel(
    const uint64_t* __restrict__ alias_tab, const int64_t* __restrict__ table_ids, int64_t n_rows,
    const int64_t* __restrict__ batch_ids, int B, int N, int draw_groups, const int64_t* __restrict__ step,
    int64_t step_offset, uint64_t seed, int cap, SampCols cols, int32_t* __restrict__ sel) {
  const int tid = threadIdx.x;
  if (static_cast<int>(blockIdx.x) >= draw_groups) {
    const int j = (blockIdx.x - draw_groups) * kWsampThreads + tid;
    if (j < B) samp_copy_row(cols, false, j, j);
    return;
  }
  extern __shared__ __align__(16) unsigned char samp_lds[];
  unsigned long long* set = reinterpret_cast<unsigned long long*>(samp_lds);
  int* has_empty = reinterpret_cast<int*>(set + cap);
  const unsigned long long slot_mask = static_cast<unsigned long long>(cap - 1);
  const uint64_t n = static_cast<uint64_t>(n_rows);
  const int j = blockIdx.x * kWsampThreads + tid;
  const bool draws = j < N;

  // attempt 0: its alias record is in flight while the set is cleared
  const uint64_t base = mix64(seed ^ mix64(static_cast<uint64_t>(*step + step_offset)));
  uint32_t k = 0;
  float f = 0.f;
  uint64_t rec = 0;
  if (draws) {
    wsamp_random(base, j, 0, n, &k, &f);
    rec = alias_tab[k];
  }
  unsigned long long mine[kWsampIdsPerLane];
#pragma unroll
  for (int u = 0; u < kWsampIdsPerLane; ++u) {
    const int i = tid + u * kWsampThreads;
    mine[u] = i < B ? static_cast<unsigned long long>(batch_ids[i]) : 0ull;
  }
  for (int i = tid; i < cap; i += kWsampThreads) set[i] = kSampEmpty;
  if (tid == 0) *has_empty = 0;
  // its id and first column group are in flight while the set is filled
  uint32_t row = 0;
  unsigned long long id = 0;
  uint64_t v[kSampColGroup];
  if (draws) {
    row = wsamp_row(rec, k, f, n);
    id = static_cast<unsigned long long>(table_ids[row]);
    samp_load_group(cols, 0, row, v);
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < kWsampIdsPerLane; ++u) {
    if (tid + u * kWsampThreads >= B) continue;
    const unsigned long long bid = mine[u];
    if (bid == kSampEmpty) {
      *has_empty = 1;
      continue;
    }
    unsigned long long slot = mix64(bid) & slot_mask;
    for (int probe = 0; probe < cap; ++probe) {  // (at most B < cap slots are ever taken: an empty one is found)
      const unsigned long long prev = atomicCAS(&set[slot], kSampEmpty, bid);
      if (prev == kSampEmpty || prev == bid) break;
      slot = (slot + 1) & slot_mask;
    }
  }
  __syncthreads();
  if (!draws) return;  // (no barrier follows)
  const bool empty_is_member = *has_empty != 0;

  bool member = samp_is_member(set, slot_mask, empty_is_member, id);
  if (member) {
    for (int a = 1; a < kWsampAttempts && member; ++a) {
      wsamp_random(base, j, a, n, &k, &f);
      row = wsamp_row(alias_tab[k], k, f, n);
      member = samp_is_member(set, slot_mask, empty_is_member, static_cast<unsigned long long>(table_ids[row]));
    }
    for (int w = 0; w <= B && member; ++w) {  // the weights are left behind: the next eligible row
      row = row + 1 < n ? row + 1 : 0;
      member = samp_is_member(set, slot_mask, empty_is_member, static_cast<unsigned long long>(table_ids[row]));
    }
    samp_load_group(cols, 0, row, v);
  }
  sel[j] = static_cast<int32_t>(row);
  const int64_t out = static_cast<int64_t>(B) + j;
  samp_store_group(cols, 0, out, v);
  for (int c0 = kSampColGroup; c0 < cols.ncols; c0 += kSampColGroup) {
    samp_load_group(cols, c0, row, v);
    samp_store_group(cols, c0, out, v);
  }
}

static int g_wsamp_lds = 0;

}  // namespace er

extern "C" {

int64_t er_neg_sample_lds_bytes(int32_t B) { return er::samp_lds_bytes(B); }

int er_neg_sample(const int64_t* table_ids, int64_t n, const int64_t* batch_ids, int32_t B, int32_t N,
                  const int64_t* step, int64_t step_offset, uint64_t seed, const void* const* table_cols_host,
                  const void* const* batch_cols_host, void* const* out_cols_host, const int32_t* elem_bytes_host,
                  int32_t ncols, int32_t* sel, er_stream_t stream) {
  const int64_t bytes = er::samp_lds_bytes(B);
  ER_REQUIRE(bytes > 0, "er_neg_sample: B %d outside the envelope 1 .. %d", B, er::kSampMaxB);
  ER_REQUIRE(table_ids && batch_ids && step && sel, "er_neg_sample: null argument");
  ER_REQUIRE(N >= 1 && static_cast<int64_t>(B) + N <= n && n <= 0x7fffffffll,
             "er_neg_sample: need 1 <= N and B + N <= n < 2^31 (B %d, N %d, n %lld)", B, N, static_cast<long long>(n));
  ER_REQUIRE(ncols >= 0 && ncols <= er::kSampMaxCols, "er_neg_sample: %d columns, at most %d", ncols, er::kSampMaxCols);
  ER_REQUIRE(ncols == 0 || (table_cols_host && batch_cols_host && out_cols_host && elem_bytes_host),
             "er_neg_sample: null column list");
  er::SampCols cols;
  memset(&cols, 0, sizeof(cols));
  cols.ncols = ncols;
  for (int c = 0; c < ncols; ++c) {
    ER_REQUIRE(table_cols_host[c] && batch_cols_host[c] && out_cols_host[c], "er_neg_sample: column %d: null buffer", c);
    ER_REQUIRE(elem_bytes_host[c] == 4 || elem_bytes_host[c] == 8, "er_neg_sample: column %d: %d-byte elements", c,
               elem_bytes_host[c]);
    cols.table[c] = table_cols_host[c];
    cols.batch[c] = batch_cols_host[c];
    cols.out[c] = out_cols_host[c];
    if (elem_bytes_host[c] == 8) cols.wide |= 1u << c;
  }
  const void* fn = reinterpret_cast<const void*>(er::neg_sample_kernel);
  if (bytes > 65536 && bytes > er::g_samp_lds) {  // (no stream work: safe inside a capture)
    ER_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes)));
    er::g_samp_lds = static_cast<int>(bytes);
  }
  const int grid = 1 + static_cast<int>(er::ceil_div(B, er::kSampThreads));
  hipLaunchKernelGGL(er::neg_sample_kernel, dim3(grid), dim3(er::kSampThreads), static_cast<size_t>(bytes),
                     er::as_stream(stream), table_ids, n, batch_ids, B, N, step, step_offset, seed, er::samp_capacity(B),
                     cols, sel);
  ER_LAUNCH_CHECK();
  return 0;
}

int64_t er_neg_sample_weighted_lds_bytes(int32_t B) { return er::wsamp_lds_bytes(B); }

int er_neg_sample_weighted(const uint64_t* alias_tab, const int64_t* table_ids, int64_t n, const int64_t* batch_ids,
                           int32_t B, int32_t N, const int64_t* step, int64_t step_offset, uint64_t seed,
                           const void* const* table_cols_host, const void* const* batch_cols_host,
                           void* const* out_cols_host, const int32_t* elem_bytes_host, int32_t ncols, int32_t* sel,
                           er_stream_t stream) {
  const int64_t bytes = er::wsamp_lds_bytes(B);
  ER_REQUIRE(bytes > 0, "er_neg_sample_weighted: B %d outside the envelope 1 .. %d", B, er::kSampMaxB);
  ER_REQUIRE(alias_tab && table_ids && batch_ids && step && sel, "er_neg_sample_weighted: null argument");
  ER_REQUIRE(N >= 1 && static_cast<int64_t>(B) + N <= n && n <= 0x7fffffffll,
             "er_neg_sample_weighted: need 1 <= N and B + N <= n < 2^31 (B %d, N %d, n %lld)", B, N,
             static_cast<long long>(n));
  ER_REQUIRE(ncols >= 0 && ncols <= er::kSampMaxCols, "er_neg_sample_weighted: %d columns, at most %d", ncols,
             er::kSampMaxCols);
  ER_REQUIRE(ncols == 0 || (table_cols_host && batch_cols_host && out_cols_host && elem_bytes_host),
             "er_neg_sample_weighted: null column list");
  er::SampCols cols;
  memset(&cols, 0, sizeof(cols));
  cols.ncols = ncols;
  for (int c = 0; c < ncols; ++c) {
    ER_REQUIRE(table_cols_host[c] && batch_cols_host[c] && out_cols_host[c],
               "er_neg_sample_weighted: column %d: null buffer", c);
    ER_REQUIRE(elem_bytes_host[c] == 4 || elem_bytes_host[c] == 8, "er_neg_sample_weighted: column %d: %d-byte elements",
               c, elem_bytes_host[c]);
    cols.table[c] = table_cols_host[c];
    cols.batch[c] = batch_cols_host[c];
    cols.out[c] = out_cols_host[c];
    if (elem_bytes_host[c] == 8) cols.wide |= 1u << c;
  }
  const void* fn = reinterpret_cast<const void*>(er::neg_sample_weighted_kernel);
  if (bytes > 65536 && bytes > er::g_wsamp_lds) {  // (no stream work: safe inside a capture)
    ER_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes)));
    er::g_wsamp_lds = static_cast<int>(bytes);
  }
  const int draw_groups = static_cast<int>(er::ceil_div(N, er::kWsampThreads));
  const int grid = draw_groups + static_cast<int>(er::ceil_div(B, er::kWsampThreads));
  hipLaunchKernelGGL(er::neg_sample_weighted_kernel, dim3(grid), dim3(er::kWsampThreads), static_cast<size_t>(bytes),
                     er::as_stream(stream), alias_tab, table_ids, n, batch_ids, B, N, draw_groups, step, step_offset, seed,
                     er::samp_capacity(B), cols, sel);
  ER_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
