// xent_sums.h -- what the criterion kernels (xent.hip, dml.hip) share: the workgroup size, the grid caps, the size check and the
// deterministic workgroup sum of per-lane fp64 values (wave.h: wg_sum).
#pragma once
#include "wave.h"

namespace pvcnn {

constexpr int kXentThreads = 256;
static_assert(kXentThreads == 4 * kWave, "wg_sum adds four wave totals");
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

}  // namespace pvcnn
