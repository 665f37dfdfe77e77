// The gradient reduce that every block with packed parameters `theta` shares (easyrec_hip.h K8e): the block's backward
// left per-workgroup partial sums in partials [rows, P]; this sums the rows in a fixed order and adds or writes each
// stretch of the result into the matching variable's gradient buffer.  No atomics, so two runs and a graph replay give
// the same bits.
#include "er_common.h"

namespace er {

// The buffers' addresses and first theta entries travel in the kernel arguments, so that a launch inside a stream
// capture needs no device-side table built beforehand.  Capacity: BST's worst case, 6 * 64 + 8 segments; 16-bit starts
// (P < 65536) keep the argument block within 4 KB.
constexpr int kThetaMaxSegs = 392;
struct ThetaReduceArgs {
  const float* partials;
  float* p[kThetaMaxSegs];
  uint16_t start[kThetaMaxSegs];  // first theta entry of each segment
  int rows, P, nseg, row_groups, acc;
};
static_assert(sizeof(ThetaReduceArgs) <= 4096, "er_theta_grad_reduce: the kernel arguments must stay within 4 KB");

// grads[seg][k - start[seg]] (+)= sum over the rows of partials[row, k]: 256 / row_groups columns x row_groups row
// groups per workgroup, each thread its group's rows in order, the groups' sums combined in order
__global__ __launch_bounds__(kBlock) void theta_grad_reduce_kernel(ThetaReduceArgs a) {
  __shared__ float sums[kBlock];
  const int cols = kBlock / a.row_groups;
  const int col = threadIdx.x % cols, rg = threadIdx.x / cols;
  const int k = blockIdx.x * cols + col;
  float s = 0.f;
  if (k < a.P)
    for (int r = rg; r < a.rows; r += a.row_groups) s += a.partials[static_cast<int64_t>(r) * a.P + k];
  sums[threadIdx.x] = s;
  __syncthreads();
  if (rg != 0 || k >= a.P) return;
  for (int i = 1; i < a.row_groups; ++i) s += sums[i * cols + col];
  int lo = 0, hi = a.nseg;  // the segment with start[seg] <= k < start[seg + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (a.start[mid] <= k) lo = mid; else hi = mid;
  }
  float* dst = a.p[lo] + (k - a.start[lo]);
  *dst = a.acc ? *dst + s : s;
}

}  // namespace er

extern "C" {

int er_theta_grad_reduce(const float* partials, int32_t rows, int32_t P, const int32_t* lens_host, int32_t nseg,
                         float* const* grads_host, int32_t row_groups, int acc, er_stream_t stream) {
  ER_REQUIRE(partials && lens_host && grads_host && rows > 0, "er_theta_grad_reduce: bad arguments");
  ER_REQUIRE(row_groups == 1 || row_groups == 8, "er_theta_grad_reduce: row_groups = %d, not 1 or 8", row_groups);
  ER_REQUIRE(P >= 1 && P < 65536, "er_theta_grad_reduce: P = %d outside 1 .. 65535", P);
  ER_REQUIRE(nseg >= 1 && nseg <= er::kThetaMaxSegs, "er_theta_grad_reduce: %d segments outside 1 .. %d", nseg,
             er::kThetaMaxSegs);
  er::ThetaReduceArgs a;
  int o = 0;
  for (int i = 0; i < er::kThetaMaxSegs; ++i) {
    a.p[i] = nullptr;
    a.start[i] = static_cast<uint16_t>(o);
    if (i >= nseg) continue;
    ER_REQUIRE(grads_host[i] != nullptr, "er_theta_grad_reduce: gradient buffer %d is null", i);
    ER_REQUIRE(lens_host[i] >= 1 && lens_host[i] <= P - o,
               "er_theta_grad_reduce: segment %d holds %d floats from %d on, theta %d", i, lens_host[i], o, P);
    a.p[i] = grads_host[i];
    o += lens_host[i];
  }
  ER_REQUIRE(o == P, "er_theta_grad_reduce: segments hold %d floats, theta %d", o, P);
  a.partials = partials;
  a.rows = rows;
  a.P = P;
  a.nseg = nseg;
  a.row_groups = row_groups;
  a.acc = acc;
  hipLaunchKernelGGL(er::theta_grad_reduce_kernel,
                     dim3(static_cast<unsigned>(er::ceil_div(P, er::kBlock / row_groups))), dim3(er::kBlock), 0,
                     er::as_stream(stream), a);
  ER_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
