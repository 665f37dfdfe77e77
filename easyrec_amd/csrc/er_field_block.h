// What the field-block kernels (er_bst.hip, er_autoint.hip, er_fibinet.hip) share: one 256-thread workgroup stages
// `epb` examples beside its fixed data in the default 64 KiB of LDS and walks its share of the batch.
#pragma once
#include "er_common.h"

namespace er {

constexpr int kFieldThreads = 256;
constexpr int kFieldWaves = kFieldThreads / kWave;
constexpr int kFieldLdsBudget = 65536;  // bytes per workgroup: no opt-in beyond the default, 2 workgroups per CU
constexpr int kFieldMaxGrid = 512;      // persistent workgroups (2 per CU on MI355X); rows of `partials`
constexpr int kFieldMaxEpb = 8;

// an odd LDS row pitch: a walk down a column is conflict-free
__host__ __device__ inline int odd(int n) { return n | 1; }

// examples per workgroup: what fits beside `fixed` floats at `per` floats each, 8 at most
inline int epb(int fixed, int per) {
  const int n = (kFieldLdsBudget / 4 - fixed) / per;
  return n < kFieldMaxEpb ? n : kFieldMaxEpb;
}

inline int persistent_grid(int64_t B, int epb) {
  const int64_t n = (B + epb - 1) / epb;
  return static_cast<int>(n < kFieldMaxGrid ? n : kFieldMaxGrid);
}

}  // namespace er
