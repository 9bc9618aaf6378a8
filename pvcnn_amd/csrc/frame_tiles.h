// frame_tiles.h -- the point tiles of the KITTI frame stage (frames.hip, frame_store.hip): 64 consecutive points, one bit per point.
#pragma once
#include "common.h"

namespace pvcnn {

constexpr int kFrameTile = PVCNN_FRAME_TILE;   // points per tile = lanes per wave
static_assert(kFrameTile == kWave, "a tile is one wave");

// the position of the r-th (from 0) set bit of a word that has more than r of them
__device__ __forceinline__ int frame_nth_bit(unsigned long long w, int r) {
  int base = 0;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    const unsigned long long lo = w & ((1ull << s) - 1ull);
    const int c = __popcll(lo);
    if (r >= c) { r -= c; w >>= s; base += s; } else { w = lo; }
  }
  return base;
}

}  // namespace pvcnn
