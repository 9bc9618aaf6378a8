// philox.h -- the one statement of the draw stream of the kernels that draw on the device: batch.hip, frames.hip, frame_store.hip,
// augment.hip, mask_select.hip (and rooms.hip, which takes the key from here and lays out its own counter).
//
// THE STREAM (include/pvcnn_hip.h, "Device draws"; restated in numpy by tests/draws_truth.py): Philox4x32-10; the key is the two
// halves of seed[0]; counter word 2 is the low 32 bits of seed[1]; counter word 3 names the use (the table below); counter words 0
// and 1 are the use's own -- the point (or 0) and the sample.  A loader keys its assembly and its augmentation with the same two
// words: only the table keeps them from drawing the same numbers.
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

// counter word 3: one line per use
constexpr uint32_t kDrawPick = 0u;        // the picks of batch.hip, frames.hip and frame_store.hip; mask_select.hip's selection keys
constexpr uint32_t kDrawJitter = 1u;      // ShapeNet's jitter (batch.hip); mask_select.hip's shuffle keys
constexpr uint32_t kDrawFlipShift = 2u;   // Frustum-KITTI's flip and shift (batch.hip, frame_store.hip)
constexpr uint32_t kDrawBox = 3u;         // the frame store's box perturbation
constexpr uint32_t kDrawAugCloud = 16u;   // .. 19: augment.hip's per-cloud draws
constexpr uint32_t kDrawAugJitter = 20u;  // augment.hip's per-point jitter
constexpr uint32_t kDrawAugKeep = 21u;    // augment.hip's per-point keep
static_assert(kDrawPick < kDrawJitter && kDrawJitter < kDrawFlipShift && kDrawFlipShift < kDrawBox && kDrawBox < kDrawAugCloud &&
                  kDrawAugCloud + 3u < kDrawAugJitter && kDrawAugJitter < kDrawAugKeep,
              "the words a loader can key with one seed are distinct: assembly 0..3, augmentation 16..21");

struct DrawStream {
  uint2 key;
  uint32_t stream;
};

// null: zeros (parity mode draws nothing)
__device__ __forceinline__ DrawStream draw_stream(const int64_t *seed) {
  if (!seed) return {make_uint2(0u, 0u), 0u};
  return {make_uint2((uint32_t)seed[0], (uint32_t)((uint64_t)seed[0] >> 32)), (uint32_t)seed[1]};
}

__device__ __forceinline__ uint4 draw_words(const DrawStream &s, uint32_t a, uint32_t b, uint32_t ctr) {
  return philox4x32_10(make_uint4(a, b, s.stream, ctr), s.key);
}

// uniform on [0, n): every index has floor or ceil of 2^32 / n preimages
__device__ __forceinline__ uint32_t draw_index(const DrawStream &s, uint32_t p, uint32_t b, uint32_t n) {
  return mulhi32(draw_words(s, p, b, kDrawPick).x, n);
}

// the sort word of the selection without replacement: the index in the low half makes all words distinct
__device__ __forceinline__ unsigned long long draw_sort_word(const DrawStream &s, uint32_t i, uint32_t b) {
  return ((unsigned long long)draw_words(s, i, b, kDrawPick).x << 32) | i;
}

// one word -> a number
__device__ __forceinline__ float unit_f32(uint32_t r) { return (float)(r >> 8) * 0x1p-24f; }          // [0, 1), 24 bits
__device__ __forceinline__ double open_f64(uint32_t r) { return ((double)r + 0.5) * 0x1p-32; }        // (0, 1)
__device__ __forceinline__ double unit_f64(uint32_t r) { return (double)r * 0x1p-32; }                // [0, 1)

// a standard normal pair from two words (Box-Muller): u1 in (0, 1], u2 in [0, 1)
__device__ __forceinline__ float2 normal2_f32(uint32_t r1, uint32_t r2) {
  const float u1 = (float)((r1 >> 8) + 1u) * 0x1p-24f, u2 = unit_f32(r2);
  const float rad = sqrtf(-2.0f * logf(u1)), ang = 6.283185307179586f * u2;
  return make_float2(rad * cosf(ang), rad * sinf(ang));
}
__device__ __forceinline__ double2 normal2_f64(uint32_t r1, uint32_t r2) {
  const double u1 = ((double)r1 + 1.0) * 0x1p-32, u2 = unit_f64(r2);
  const double rad = sqrt(-2.0 * log(u1)), ang = 6.283185307179586 * u2;
  return make_double2(rad * cos(ang), rad * sin(ang));
}

// Frustum-KITTI's per-sample draws, from the stream or (parity) from the caller: np.random.random() > 0.5 and np.random.randn()
struct FlipShift {
  bool flipped;
  double z;
};
__device__ __forceinline__ FlipShift draw_flip_shift(const DrawStream &s, uint32_t b, bool random_flip, bool random_shift, bool parity,
                                                     const double *flip, const double *shift) {
  uint4 r4 = make_uint4(0u, 0u, 0u, 0u);
  if (!parity && (random_flip || random_shift)) r4 = draw_words(s, 0u, b, kDrawFlipShift);
  FlipShift d{false, 0.0};
  if (random_flip) d.flipped = parity ? flip[b] > 0.5 : (r4.x >> 31) != 0u;
  if (random_shift) d.z = parity ? shift[b] : (double)normal2_f32(r4.y, r4.z).x;
  return d;
}

}  // namespace pvcnn
