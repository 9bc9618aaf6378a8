// frame_tiles.h -- what the frustum kernels share (frames.hip, frame_store.hip; batch.hip for the item lookup): the point tiles of the
// KITTI frame stage -- 64 consecutive points, one bit per point -- and the frustum geometry, fp64 with one rounding per operation.
#pragma once
#include "common.h"

namespace pvcnn {

constexpr int kFrameTile = PVCNN_FRAME_TILE;   // points per tile = lanes per wave
static_assert(kFrameTile == kWave, "a tile is one wave");

__device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the item of sample b of a batch: order[cursor[0] + b], position and item clamped to the tables (cursor null: 0)
__device__ __forceinline__ long long sample_item(const int64_t *order, const int64_t *cursor, long long order_len, long long W, int b) {
  const long long pos = clampll((cursor ? cursor[0] : 0ll) + b, 0ll, order_len - 1);
  return clampll(order[pos], 0ll, W - 1);
}

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

// the point index of the pos-th selected point of a box: the last tile with prefix <= pos holds it (empty tiles share a prefix with the
// next), then select-k-th-bit of its mask word
__device__ __forceinline__ long long frame_pick(const int *prefix, const unsigned long long *mask, long long tiles, int pos) {
  long long lo = 0, hi = tiles - 1;
  while (lo < hi) {
    const long long mid = (lo + hi + 1) >> 1;
    if (prefix[mid] <= pos) lo = mid; else hi = mid - 1;
  }
  const unsigned long long bits = mask[lo];
  const int r = pos - prefix[lo];
  return lo * kFrameTile + ((r >= 0 && r < (int)__popcll(bits)) ? frame_nth_bit(bits, r) : 0);
}

// rotation about y by the angle of (c, s): x' = x c + z (-s), z' = x s + z c
__device__ __forceinline__ void rotate_y(double &x, double &z, double c, double s) {
  const double x0 = x;
  x = x0 * c + z * (-s);
  z = x0 * s + z * c;
}
// ... of an fp32 row: fp64 from the fp32 values, rounded once
__device__ __forceinline__ void rotate_y(float4 &v, double c, double s) {
  double x = (double)v.x, z = (double)v.z;
  rotate_y(x, z, c, s);
  v.x = (float)x;
  v.z = (float)z;
}

// (dx, dy, dz) from the bottom centre of a 3-D box (h, w, l, cos ry, sin ry) lies in it: the box-frame form of the hull test
__device__ __forceinline__ bool inside_box3d(double dx, double dy, double dz, double h, double w, double l, double c, double s) {
  const double xl = c * dx - s * dz, zl = s * dx + c * dz;
  return fabs(xl) <= l / 2.0 && fabs(zl) <= w / 2.0 && dy <= 0.0 && dy >= -h;
}

// v to point p of the four channel planes of f (4, N)
__device__ __forceinline__ void store_planes4(float *f, int N, int p, float4 v) {
  f[p] = v.x;
  f[(size_t)N + p] = v.y;
  f[(size_t)2 * N + p] = v.z;
  f[(size_t)3 * N + p] = v.w;
}

}  // namespace pvcnn
