// xent_sums.h -- what the criterion kernels (xent.hip, dml.hip) share: the workgroup size, the grid caps, the size check and the
// deterministic workgroup sum of per-lane fp64 values.
#pragma once
#include "common.h"

namespace pvcnn {

constexpr int kXentThreads = 256;
constexpr int kXentMaxParts = 1024;            // grid cap of the partials launch: beyond 1024 * 256 points the lanes stride
constexpr int kXentBwdMaxBlocks = 4096;        // grid.x cap of the gradient launch (grid.y walks the classes)
constexpr int kXentBwdMaxClassRows = 32;

__host__ __device__ inline long long xent_parts(long long B, long long S) {
  const long long blocks = (B * S + kXentThreads - 1) / kXentThreads;
  return blocks < kXentMaxParts ? blocks : kXentMaxParts;
}

// B * S points within 2^40, B * C * S elements within 2^46: what the kernels' 64-bit offsets are written for
inline bool xent_points_ok(long long B, long long S) { return B > 0 && S > 0 && B <= (1ll << 40) / S; }
inline bool xent_sizes_ok(long long B, int C, long long S) {
  return B > 0 && C > 0 && S > 0 && B <= (1ll << 40) / S && (long long)C <= (1ll << 46) / (B * S);
}

#ifdef __HIPCC__
// the sums of K per-lane values over the workgroup, in every thread (wave butterfly, then the four wave totals in wave order)
template <int K>
__device__ __forceinline__ void xent_block_sums(double (&v)[K]) {
  __shared__ double s_wave[K][kXentThreads / kWave];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
    if ((threadIdx.x & 63) == 0) s_wave[k][threadIdx.x >> 6] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = ((s_wave[k][0] + s_wave[k][1]) + s_wave[k][2]) + s_wave[k][3];
}
#endif

}  // namespace pvcnn
