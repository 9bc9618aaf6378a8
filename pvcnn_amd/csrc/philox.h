// philox.h -- the counter-based generator shared by the kernels that draw on the device (mask_select.hip, batch.hip).
#pragma once
#include "common.h"

namespace pvcnn {

__device__ __forceinline__ uint32_t mulhi32(uint32_t a, uint32_t b) { return __umulhi(a, b); }

// Philox4x32-10 (Salmon et al., SC'11): counter (c0..c3), key (k0,k1) -> 4 random words
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint2 k) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = mulhi32(M0, c.x), lo0 = M0 * c.x, hi1 = mulhi32(M1, c.z), lo1 = M1 * c.z;
    c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
    k.x += W0; k.y += W1;
  }
  return c;
}

// a standard normal pair from two random words (Box-Muller, fp32): u1 in (0, 1], u2 in [0, 1) -- the datasets' draws (batch.hip,
// frame_store.hip)
__device__ __forceinline__ float2 batch_normal2(uint32_t r1, uint32_t r2) {
  const float u1 = (float)((r1 >> 8) + 1u) * 0x1p-24f, u2 = (float)(r2 >> 8) * 0x1p-24f;
  const float rad = sqrtf(-2.0f * logf(u1)), ang = 6.283185307179586f * u2;
  return make_float2(rad * cosf(ang), rad * sinf(ang));
}

}  // namespace pvcnn
