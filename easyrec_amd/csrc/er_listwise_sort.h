// The record sort of K8o (er_listwise.hip: listwise_tile_sort_kernel, listwise_merge_kernel) for the entry points that
// work on examples sorted by (signed key, example index): er_listwise_tiled and er_pairwise_sorted.
#pragma once
#include "er_common.h"

namespace er {

constexpr int kLwMaxB = 8192;          // er_listwise: one workgroup's LDS
constexpr int kLwRecordBytes = 12;     // int64 key + int32 index
constexpr int kLwtMaxB = 131072;
constexpr int kLwtDefaultTile = 1024;  // what tile = 0 selects

// the tile a launch runs at; 0 outside the envelope
inline int lwt_tile(int64_t B, int tile) {
  if (B < 1 || B > kLwtMaxB) return 0;
  if (tile == 0) return B > kLwMaxB ? kLwtDefaultTile : 0;
  return (tile == 1024 || tile == 2048 || tile == 4096 || tile == 8192) ? tile : 0;
}

// The tile sort and the ceil(log2 G) merge passes over NP = G T records, G = ceil(B / T) (positions >= B padded with
// (INT64_MAX, position)), between the record buffers (key[0], idx[0]) and (key[1], idx[1]) of NP entries each; *cur: the
// buffer that holds the sorted records, the real ones at the positions 0 .. B - 1.  Opts in to the kernels' LDS once.
// -> 0, or the error code of a failed runtime call (set_error holds its text).
int lwt_sort(const int64_t* keys, int B, int T, int64_t* const key[2], int32_t* const idx[2], er_stream_t stream, int* cur);

}  // namespace er
