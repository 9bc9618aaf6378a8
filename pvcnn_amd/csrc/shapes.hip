// shapes.hip -- the ShapeNet front end: exact k-nearest neighbours over packed ragged clouds, PCA surface normals from them, and the
// per-cloud centroids the "outward" orientation refers to (include/pvcnn_hip.h, "Shapes on the device"; pvcnn_amd/shapes.py).
//
// The reference has no such operator: its ShapeNet recipes read pre-computed normals from the benchmark's text files.  The layout is
// data._Store's: rows (R, ld) fp32 with xyz in the first three columns, cloud w owning rows offsets[w] .. offsets[w + 1].
//
// k_nearest  : ONE WAVE PER QUERY.  Lane l holds the l-th nearest so far as (d, j), ascending in (d, j): the running list lives across
//              the lanes of the wave, not in a per-lane array (which, indexed at run time, would sit in scratch memory).  Per step
//              the 64 lanes compute the distances of 64 consecutive candidates (consecutive rows: coalesced), a ballot keeps those
//              that beat the current k-th, and the survivors are inserted one by one: position = number of list entries below the
//              newcomer (one more ballot), the tail moves up by one lane (a DPP wave shift).  The first tile is not inserted but
//              sorted by rank in the wave: it IS the list.  A newcomer is tested against the k-th entry again
//              right before its insertion, so a tile costs as many insertions as it changes the list.  The four waves of a workgroup
//              take consecutive queries, mostly of one cloud: its rows (12 .. 28 bytes each) stay in the CU's L1 between them.
//              d = ((dx dx) + (dy dy)) + (dz dz), one rounding per operation (the library is built with -ffp-contract=off).
//              Every comparison is on the pair (d, j), so neither the order of insertion nor ties change the result; a NaN
//              distance is never inserted (its slot keeps -1).
// normals    : one lane per point; mean and covariance of the neighbours in fp64 (two passes over the k gathered rows), the covariance
//              divided by its trace, eig3.h's fixed-sweep Jacobi, the unit vector rounded to fp32 once, then the sign.
// centroids  : one wave per cloud, fp64 sums in a fixed order (lane-strided, then wave.h's butterfly), divided once, rounded once.
// Bounds: a cloud's range is clamped into [0, R] before it is used, a neighbour index outside [0, n) is skipped: with offsets or a
// table that break the contract the kernels still read and write inside the arrays they were given.
#include <limits.h>

#include "eig3.h"
#include "wave.h"

namespace pvcnn {

constexpr int kShapesMaxK = PVCNN_K_NEAREST_MAX_K;
constexpr int kEmpty = INT_MAX - kWave + 1;   // list keys kEmpty .. INT_MAX: no candidate (clouds hold at most kEmpty points)
static_assert(kShapesMaxK == kWave, "lane l of a wave holds the l-th nearest neighbour");

// the cloud that owns row r: the largest w in [0, W) with offsets[w] <= r (ends for any table contents)
__device__ __forceinline__ long long cloud_of_row(const int64_t *__restrict__ offsets, long long W, long long r) {
  long long lo = 0, hi = W - 1;
  while (lo < hi) {
    const long long mid = (lo + hi + 1) >> 1;
    if (offsets[mid] <= r) lo = mid; else hi = mid - 1;
  }
  return lo;
}
__device__ __forceinline__ long long clamp_row(long long v, long long R) { return v < 0 ? 0 : (v > R ? R : v); }

__device__ __forceinline__ float lane_value(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }
__device__ __forceinline__ int lane_value(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
// the value of lane l - 1 (lane 0 keeps its own): a DPP wave shift inside the VALU (__shfl_up lowers to ds_bpermute_b32, an LDS round
// trip per insertion -- and the insertions are what a query of a ShapeNet-sized cloud spends its time on)
__device__ __forceinline__ int lane_below(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138 /* wave_shr:1 */, 0xF, 0xF, false); }
__device__ __forceinline__ float lane_below(float v) { return __int_as_float(lane_below(__float_as_int(v))); }
// (d, j) < (e, i), lexicographic; false whenever d is NaN
__device__ __forceinline__ bool pair_less(float d, int j, float e, int i) { return (d < e) | ((d == e) & (j < i)); }   // no branches

__global__ __launch_bounds__(256) void k_nearest_kernel(const float *__restrict__ rows, long long R, int ld,
                                                        const int64_t *__restrict__ offsets, long long W, int k,
                                                        int32_t *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave-uniform
  if (r >= R) return;
  const long long w = cloud_of_row(offsets, W, r);
  const long long a = clamp_row(offsets[w], R), b = clamp_row(offsets[w + 1], R);
  int32_t *o = out + r * k;
  if (r < a || r >= b) {             // a row no cloud owns (a table that does not cover the rows): no neighbours
    if (lane < k) o[lane] = -1;
    return;
  }
  const int n = (int)(b - a);        // R <= kEmpty (host check)
  const float *base = rows + (size_t)a * ld;
  const float *q = base + (size_t)(r - a) * ld;
  const float qx = q[0], qy = q[1], qz = q[2];
  // The first tile IS the list, sorted: every lane counts the candidates below its own (64 lane reads, no dependent insertions) and
  // sends its pair to the lane of that rank.  Lane l then holds the l-th smallest (d, j) seen so far.  An absent candidate -- past the
  // cloud's end, or at a NaN distance -- takes the key (inf, kEmpty + lane): the 64 keys are distinct, the ranks a permutation, and
  // such a key is above every real pair (n <= kEmpty, host check); it is written out as -1.
  float bd;
  int bj;
  {
    const float *p = base + (size_t)min(lane, n - 1) * ld;
    const float dx = p[0] - qx, dy = p[1] - qy, dz = p[2] - qz;
    const float d = (dx * dx + dy * dy) + dz * dz;
    const bool real = lane < n && d == d;
    const float kd = real ? d : INFINITY;
    const int kj = real ? lane : kEmpty + lane;
    int rank = 0;
#pragma unroll
    for (int c = 0; c < kWave; ++c) rank += pair_less(lane_value(kd, c), lane_value(kj, c), kd, kj) ? 1 : 0;
    bd = __int_as_float(__builtin_amdgcn_ds_permute(rank << 2, __float_as_int(kd)));
    bj = __builtin_amdgcn_ds_permute(rank << 2, kj);
  }
  const int last = k - 1;
  for (int j0 = kWave; j0 < n; j0 += kWave) {
    const int j = j0 + lane;
    const float *p = base + (size_t)min(j, n - 1) * ld;
    const float dx = p[0] - qx, dy = p[1] - qy, dz = p[2] - qz;
    const float d = (dx * dx + dy * dy) + dz * dz;
    unsigned long long mask = __ballot(j < n && pair_less(d, j, lane_value(bd, last), lane_value(bj, last)));
    while (mask) {                   // wave-uniform: ascending lanes = ascending candidates
      const int c = __builtin_ctzll(mask);
      mask &= mask - 1;
      const float dc = lane_value(d, c);
      const int jc = j0 + c;
      if (!pair_less(dc, jc, lane_value(bd, last), lane_value(bj, last))) continue;   // an earlier insertion pushed the bar below it
      const int pos = __popcll(__ballot(lane < k && pair_less(bd, bj, dc, jc)));       // < k: the k-th entry is above the newcomer
      const float ud = lane_below(bd);
      const int uj = lane_below(bj);
      if (lane > pos) { bd = ud; bj = uj; }
      else if (lane == pos) { bd = dc; bj = jc; }
    }
  }
  if (lane < k) o[lane] = (bj >= kEmpty) ? -1 : bj;
}

__global__ __launch_bounds__(256) void shape_normals_kernel(const float *__restrict__ rows, long long R, int ld,
                                                            const int64_t *__restrict__ offsets, long long W,
                                                            const int32_t *__restrict__ knn, int k, const float *__restrict__ ref,
                                                            int mode, float *__restrict__ normals, float *__restrict__ curvature) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  const long long w = cloud_of_row(offsets, W, r);
  const long long a = clamp_row(offsets[w], R), b = clamp_row(offsets[w + 1], R);
  float nx = 0.f, ny = 0.f, nz = 0.f, cv = 0.f;
  if (r >= a && r < b) {
    const int n = (int)(b - a);
    const float *base = rows + (size_t)a * ld;
    const int32_t *nb = knn + r * k;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int c = 0;
    for (int t = 0; t < k; ++t) {
      const int j = nb[t];
      if (j < 0 || j >= n) continue;
      const float *p = base + (size_t)j * ld;
      sx += (double)p[0]; sy += (double)p[1]; sz += (double)p[2];
      ++c;
    }
    if (c >= 3) {
      const double mx = sx / c, my = sy / c, mz = sz / c;
      double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0;
      for (int t = 0; t < k; ++t) {
        const int j = nb[t];
        if (j < 0 || j >= n) continue;
        const float *p = base + (size_t)j * ld;
        const double x = (double)p[0] - mx, y = (double)p[1] - my, z = (double)p[2] - mz;
        a00 += x * x; a01 += x * y; a02 += x * z; a11 += y * y; a12 += y * z; a22 += z * z;
      }
      const double tr = (a00 + a11) + a22;
      if (tr > 0.0) {                 // (false for a NaN as well: zeros)
        const double s = 1.0 / tr;
        double e0, e1, e2;
        const double lam = eig3_smallest(a00 * s, a01 * s, a02 * s, a11 * s, a12 * s, a22 * s, e0, e1, e2);
        nx = (float)e0; ny = (float)e1; nz = (float)e2;
        cv = (float)fmax(lam, 0.0);   // of C / trace(C): lambda_0 / trace
        if (mode != 0) {
          const float *pr = base + (size_t)(r - a) * ld;
          const float *rf = ref + w * 3;
          double dot = ((double)nx * ((double)pr[0] - (double)rf[0]) + (double)ny * ((double)pr[1] - (double)rf[1])) +
                       (double)nz * ((double)pr[2] - (double)rf[2]);
          if (mode == 2) dot = -dot;
          if (dot < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
        }
      }
    }
  }
  normals[r * 3 + 0] = nx; normals[r * 3 + 1] = ny; normals[r * 3 + 2] = nz;
  if (curvature) curvature[r] = cv;
}

__global__ __launch_bounds__(256) void cloud_centroids_kernel(const float *__restrict__ rows, long long R, int ld,
                                                              const int64_t *__restrict__ offsets, long long W,
                                                              float *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long w = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave-uniform
  if (w >= W) return;
  const long long a = clamp_row(offsets[w], R), b = clamp_row(offsets[w + 1], R);
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (long long j = a + lane; j < b; j += kWave) {
    const float *p = rows + (size_t)j * ld;
    sx += (double)p[0]; sy += (double)p[1]; sz += (double)p[2];
  }
  sx = wave_sum(sx); sy = wave_sum(sy); sz = wave_sum(sz);
  if (lane < 3) {
    const double s = lane == 0 ? sx : (lane == 1 ? sy : sz);
    out[w * 3 + lane] = b > a ? (float)(s / (double)(b - a)) : 0.f;
  }
}

}  // namespace pvcnn

using namespace pvcnn;

static int check_packed(const char *who, const float *rows, long long R, int ld, const int64_t *offsets, long long W) {
  if (R < 0 || W < 0 || R > (long long)kEmpty) { set_error("%s: R in [0, 2^31 - 64] and W >= 0 expected", who); return PVCNN_ERR_INVALID_ARGUMENT; }
  if (ld < 3) { set_error("%s: rows of at least three columns expected", who); return PVCNN_ERR_INVALID_ARGUMENT; }
  if (R > 0 && (W < 1 || !rows || !offsets)) { set_error("%s: null pointer / rows without a cloud", who); return PVCNN_ERR_INVALID_ARGUMENT; }
  return 0;
}

extern "C" int pvcnn_k_nearest(const float *rows, long long R, int ld, const int64_t *offsets, long long W, int k, int32_t *out,
                               void *stream) {
  if (int e = check_packed("pvcnn_k_nearest", rows, R, ld, offsets, W)) return e;
  PVCNN_REQUIRE(k >= 1 && k <= kShapesMaxK, "k in [1, 64] expected");
  if (R == 0) return 0;
  PVCNN_REQUIRE(out, "null pointer");
  hipLaunchKernelGGL(k_nearest_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), rows, R, ld,
                     offsets, W, k, out);
  return check_launch("k_nearest");
}

extern "C" int pvcnn_shape_normals(const float *rows, long long R, int ld, const int64_t *offsets, long long W, const int32_t *knn,
                                   int k, const float *ref, int mode, float *normals, float *curvature, void *stream) {
  if (int e = check_packed("pvcnn_shape_normals", rows, R, ld, offsets, W)) return e;
  PVCNN_REQUIRE(k >= 1 && k <= kShapesMaxK, "k in [1, 64] expected");
  PVCNN_REQUIRE(mode >= 0 && mode <= 2, "mode 0 (no orientation), 1 (outward) or 2 (towards) expected");
  if (R == 0) return 0;
  PVCNN_REQUIRE(knn && normals && (mode == 0 || ref), "null pointer");
  hipLaunchKernelGGL(shape_normals_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), rows, R,
                     ld, offsets, W, knn, k, ref, mode, normals, curvature);
  return check_launch("shape_normals");
}

extern "C" int pvcnn_cloud_centroids(const float *rows, long long R, int ld, const int64_t *offsets, long long W, float *out,
                                     void *stream) {
  if (int e = check_packed("pvcnn_cloud_centroids", rows, R, ld, offsets, W)) return e;
  if (W == 0) return 0;
  PVCNN_REQUIRE(offsets && out && (rows || R == 0), "null pointer");
  hipLaunchKernelGGL(cloud_centroids_kernel, dim3((unsigned)((W + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), rows, R, ld,
                     offsets, W, out);
  return check_launch("cloud_centroids");
}
