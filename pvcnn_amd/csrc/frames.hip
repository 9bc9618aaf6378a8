// frames.hip -- the front of the Frustum-KITTI pipeline on the device: a LiDAR sweep, a calibration and 2-D boxes -> frustums
// (pvcnn_amd/frames.py).
//
// The reference has no code for this stage (datasets/kitti/frustum.py reads pickles that another project's prepare_data.py writes);
// the definition is written out in include/pvcnn_hip.h and restated in numpy by tests/frames_truth.py.  All geometry is fp64, one
// rounding per operation, sums left to right (the library is built with -ffp-contract=off); no kernel calls a trigonometric function
// (every angle's cosine and sine come from the host in the box table), none allocates, none uses an atomic.
//
// POINT TILES.  A tile is the 64 points one wave holds.  "Point i lies in box m" is one bit of mask[m][tile] (a wave ballot), so a
// box's count over a tile is a popcount, the rank of a point among a box's selected points is prefix[m][tile] + popcount of the lower
// lanes' bits (ascending point index: numpy's boolean indexing), and "the k-th selected point of box m" is a binary search of the
// tile prefix followed by a select-k-th-bit of one word -- no sort, no compaction pass over the scan.
#include "common.h"
#include "frame_tiles.h"
#include "philox.h"

namespace pvcnn {

constexpr int kFrameThreads = 256;             // 4 tiles per workgroup
constexpr int kFrameCols = PVCNN_FRAME_BOX_COLUMNS;
constexpr long long kFrameMaxPoints = 1ll << 30;

__device__ __forceinline__ long long frame_points(long long cap, long long n, const int *count) {
  if (count) n = count[0];
  return n < 0 ? 0 : (n > cap ? cap : n);
}

// rows[i] = (fp32 rect, reflectance), uv[i], in_image[i] of scan point i; zeros beyond the scan's n points
__global__ __launch_bounds__(kFrameThreads) void frame_project_kernel(const float4 *__restrict__ scan, long long cap, long long n_arg,
                                                                      const int *__restrict__ count, const double *__restrict__ calib,
                                                                      double width, double height, double clip, float4 *__restrict__ rows,
                                                                      double2 *__restrict__ uv, unsigned char *__restrict__ in_image) {
  const long long i = (long long)blockIdx.x * kFrameThreads + threadIdx.x;
  if (i >= cap) return;
  const long long n = frame_points(cap, n_arg, count);
  if (i >= n) {
    rows[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    uv[i] = make_double2(0.0, 0.0);
    in_image[i] = 0;
    return;
  }
  const double *P = calib, *V = calib + 12, *R = calib + 24;
  const float4 s = scan[i];
  const double x = (double)s.x, y = (double)s.y, z = (double)s.z;
  double ref[3], rect[3], img[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) ref[k] = ((V[4 * k] * x + V[4 * k + 1] * y) + V[4 * k + 2] * z) + V[4 * k + 3];
#pragma unroll
  for (int k = 0; k < 3; ++k) rect[k] = (R[3 * k] * ref[0] + R[3 * k + 1] * ref[1]) + R[3 * k + 2] * ref[2];
#pragma unroll
  for (int k = 0; k < 3; ++k) img[k] = ((P[4 * k] * rect[0] + P[4 * k + 1] * rect[1]) + P[4 * k + 2] * rect[2]) + P[4 * k + 3];
  const double u = img[0] / img[2], v = img[1] / img[2];
  rows[i] = make_float4((float)rect[0], (float)rect[1], (float)rect[2], s.w);
  uv[i] = make_double2(u, v);
  in_image[i] = (u >= 0.0 && u < width && v >= 0.0 && v < height && x > clip) ? 1 : 0;
}

// mask[m][tile] (and label_mask[m][tile]) of every box over every tile: one wave per tile, the boxes in a uniform loop
__global__ __launch_bounds__(kFrameThreads) void frame_masks_kernel(const double2 *__restrict__ uv, const unsigned char *__restrict__ in_image,
                                                                    const float4 *__restrict__ rows, long long cap, long long tiles,
                                                                    const double *__restrict__ boxes, int M,
                                                                    unsigned long long *__restrict__ mask,
                                                                    unsigned long long *__restrict__ label_mask) {
  const long long tile = (long long)blockIdx.x * (kFrameThreads / kFrameTile) + (threadIdx.x >> 6);
  if (tile >= tiles) return;                   // (whole waves leave: the ballots below see full waves or masked tails)
  const int lane = threadIdx.x & 63;
  const long long i = tile * kFrameTile + lane;
  const bool live = i < cap;
  double2 p = make_double2(0.0, 0.0);
  float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
  bool seen = false;
  if (live) { p = uv[i]; r = rows[i]; seen = in_image[i] != 0; }
  const double X = (double)r.x, Y = (double)r.y, Z = (double)r.z;
  for (int m = 0; m < M; ++m) {
    const double *b = boxes + (size_t)m * kFrameCols;
    const bool in_box = seen && p.x >= b[0] && p.x < b[2] && p.y >= b[1] && p.y < b[3];
    const unsigned long long bits = __ballot(in_box);
    if (lane == 0) mask[(size_t)m * tiles + tile] = bits;
    if (label_mask) {
      bool inside = false;
      if (b[4] != 0.0) {                       // a 3-D box (h, w, l, t, cos ry, sin ry): the box-frame form of the hull test
        inside = in_box && inside_box3d(X - b[8], Y - b[9], Z - b[10], b[5], b[6], b[7], b[11], b[12]);
      }
      const unsigned long long lbits = __ballot(inside);
      if (lane == 0) label_mask[(size_t)m * tiles + tile] = lbits;
    }
  }
}

// prefix[m][0 .. tiles] = exclusive prefix of the tile counts of box m, counts[m] = (selected, positives): one workgroup per box
__global__ __launch_bounds__(kFrameThreads) void frame_prefix_kernel(const unsigned long long *__restrict__ mask,
                                                                     const unsigned long long *__restrict__ label_mask, long long tiles,
                                                                     int *__restrict__ prefix, int *__restrict__ counts) {
  __shared__ int s_scan[kFrameThreads];
  __shared__ int s_pos[kFrameThreads];
  const int m = blockIdx.x, t = threadIdx.x;
  const unsigned long long *mk = mask + (size_t)m * tiles;
  int *pf = prefix + (size_t)m * (tiles + 1);
  int carry = 0, positives = 0;
  for (long long base = 0; base < tiles; base += kFrameThreads) {
    const long long tile = base + t;
    const int v = tile < tiles ? __popcll(mk[tile]) : 0;
    if (label_mask && tile < tiles) positives += __popcll(label_mask[(size_t)m * tiles + tile]);
    s_scan[t] = v;
    __syncthreads();
    for (int o = 1; o < kFrameThreads; o <<= 1) {          // inclusive scan of the chunk
      const int add = t >= o ? s_scan[t - o] : 0;
      __syncthreads();
      s_scan[t] += add;
      __syncthreads();
    }
    if (tile < tiles) pf[tile] = carry + s_scan[t] - v;
    carry += s_scan[kFrameThreads - 1];
    __syncthreads();                                        // the chunk's total has been read before the next chunk overwrites it
  }
  s_pos[t] = positives;
  __syncthreads();
  for (int o = kFrameThreads / 2; o > 0; o >>= 1) {
    if (t < o) s_pos[t] += s_pos[t + o];
    __syncthreads();
  }
  if (t == 0) {
    pf[tiles] = carry;
    counts[2 * m] = carry;
    counts[2 * m + 1] = s_pos[0];
  }
}

// the selected rows (and labels) of kept box w = kept[w] to out_rows[offsets[w] + rank], rank ascending in the point index
__global__ __launch_bounds__(kFrameThreads) void frame_pack_kernel(const float4 *__restrict__ rows, long long cap, long long tiles,
                                                                   const unsigned long long *__restrict__ mask,
                                                                   const unsigned long long *__restrict__ label_mask,
                                                                   const int *__restrict__ prefix, int M, const int64_t *__restrict__ kept,
                                                                   const int64_t *__restrict__ offsets, long long R,
                                                                   float4 *__restrict__ out_rows, unsigned char *__restrict__ out_labels) {
  const long long tile = (long long)blockIdx.x * (kFrameThreads / kFrameTile) + (threadIdx.x >> 6);
  const int w = blockIdx.y, lane = threadIdx.x & 63;
  if (tile >= tiles) return;
  const long long m = kept[w];
  if (m < 0 || m >= M) return;
  const unsigned long long bits = mask[(size_t)m * tiles + tile];
  if (!((bits >> lane) & 1ull)) return;
  const long long i = tile * kFrameTile + lane;
  const long long rank = (long long)prefix[(size_t)m * (tiles + 1) + tile] + __popcll(bits & ((1ull << lane) - 1ull));
  const long long first = offsets[w], dst = first + rank;
  if (i >= cap || first < 0 || dst >= offsets[w + 1] || dst >= R) return;       // never outside the caller's tables
  out_rows[dst] = rows[i];
  if (out_labels) out_labels[dst] = label_mask ? (unsigned char)((label_mask[(size_t)m * tiles + tile] >> lane) & 1ull) : 0;
}

struct FrameBatch {
  const float4 *rows;                          // (cap) fp32 rows of the projection
  const unsigned long long *mask;              // (M, tiles)
  const int *prefix, *counts;                  // (M, tiles + 1), (M, 2)
  const double *boxes;                         // (M, kFrameCols)
  const int32_t *choices;                      // (M, N) or null
  const int64_t *seed;                         // 2 words or null
  long long cap, tiles;
  int M, N, K, rotate, min_points;
  double min_box_height;
  float *features, *one_hot, *rotation_angle;  // (Bmax, 4, N), (Bmax, K), (Bmax)
  double *rgb_score;                           // (Bmax)
  unsigned char *valid;                        // (Bmax)
};

// one workgroup per output row: what one __getitem__ of the rgb-detection loader yields for box m, straight from the scan's tiles
__global__ __launch_bounds__(kFrameThreads) void frame_batch_kernel(FrameBatch a) {
  const int m = blockIdx.x, N = a.N, K = a.K, t = threadIdx.x;
  float *f = a.features + (size_t)m * 4 * N;
  const double *b = a.boxes + (size_t)(m < a.M ? m : 0) * kFrameCols;
  int k = 0;
  bool ok = false;
  if (m < a.M) {
    k = a.counts[2 * m];
    ok = k >= 1 && k >= a.min_points && b[3] - b[1] >= a.min_box_height;
  }
  if (t == 0) {
    a.valid[m] = ok ? 1 : 0;
    a.rotation_angle[m] = ok ? (float)b[15] : 0.f;
    a.rgb_score[m] = ok ? b[17] : 0.0;
  }
  const int cls = ok ? (int)b[16] : -1;
  for (int j = t; j < K; j += kFrameThreads) a.one_hot[(size_t)m * K + j] = j == cls ? 1.f : 0.f;
  if (!ok) {
    for (int p = t; p < 4 * N; p += kFrameThreads) f[p] = 0.f;
    return;
  }
  const unsigned long long *mk = a.mask + (size_t)m * a.tiles;
  const int *pf = a.prefix + (size_t)m * (a.tiles + 1);
  const double c = b[13], s = b[14];
  const DrawStream d = draw_stream(a.choices ? nullptr : a.seed);
  for (int p = t; p < N; p += kFrameThreads) {
    const int pos = a.choices ? min(max(a.choices[(size_t)m * N + p], 0), k - 1) : (int)draw_index(d, p, m, k);
    long long i = frame_pick(pf, mk, a.tiles, pos);
    if (i > a.cap - 1) i = a.cap - 1;
    float4 v = a.rows[i];
    if (a.rotate) rotate_y(v, c, s);
    store_planes4(f, N, p, v);
  }
}

// rows of item w (offsets[w] .. offsets[w + 1]) rotated about y by the item's (cos, sin), in place
__global__ __launch_bounds__(kFrameThreads) void frame_rotate_rows_kernel(float4 *__restrict__ rows, long long R,
                                                                          const int64_t *__restrict__ offsets, long long W,
                                                                          const double *__restrict__ cos_sin) {
  const long long i = (long long)blockIdx.x * kFrameThreads + threadIdx.x;
  if (i >= R) return;
  long long lo = 0, hi = W - 1;                // the last item whose first row is <= i
  while (lo < hi) {
    const long long mid = (lo + hi + 1) >> 1;
    if (offsets[mid] <= i) lo = mid; else hi = mid - 1;
  }
  if (i < offsets[lo] || i >= offsets[lo + 1]) return;      // a row no item owns stays as it is
  float4 v = rows[i];
  rotate_y(v, cos_sin[2 * lo], cos_sin[2 * lo + 1]);
  rows[i] = v;
}

static inline unsigned frame_grid(long long n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

}  // namespace pvcnn

using namespace pvcnn;

extern "C" long long pvcnn_frame_tiles(long long cap) {
  return (cap < 1 || cap > kFrameMaxPoints) ? 0 : (cap + kFrameTile - 1) / kFrameTile;
}

extern "C" int pvcnn_frame_project(const float *scan, long long cap, long long n, const int *count, const double *calib, double width,
                                   double height, double clip_distance, float *rows, double *uv, unsigned char *in_image, void *stream) {
  PVCNN_REQUIRE(cap >= 1 && cap <= kFrameMaxPoints, "a scan buffer holds between 1 and 2^30 points");
  PVCNN_REQUIRE(count || (n >= 0 && n <= cap), "n must lie in [0, cap]");
  PVCNN_REQUIRE(scan && calib && rows && uv && in_image, "null pointer");
  PVCNN_REQUIRE(aligned16(scan) && aligned16(rows) && aligned16(uv), "scan, rows and uv must be 16-byte aligned");
  hipLaunchKernelGGL(frame_project_kernel, dim3(frame_grid(cap, kFrameThreads)), dim3(kFrameThreads), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const float4 *>(scan), cap, n, count, calib, width, height, clip_distance,
                     reinterpret_cast<float4 *>(rows), reinterpret_cast<double2 *>(uv), in_image);
  return check_launch("frame_project");
}

extern "C" int pvcnn_frame_count(const double *uv, const unsigned char *in_image, const float *rows, long long cap, const double *boxes,
                                 int M, unsigned long long *mask, unsigned long long *label_mask, int *prefix, int *counts, void *stream) {
  PVCNN_REQUIRE(cap >= 1 && cap <= kFrameMaxPoints, "a scan buffer holds between 1 and 2^30 points");
  PVCNN_REQUIRE(M >= 0 && M <= PVCNN_FRAME_MAX_BOXES, "too many boxes");
  if (M == 0) return 0;
  PVCNN_REQUIRE(uv && in_image && rows && boxes && mask && prefix && counts, "null pointer");
  PVCNN_REQUIRE(aligned16(rows) && aligned16(uv), "rows and uv must be 16-byte aligned");
  const long long tiles = pvcnn_frame_tiles(cap);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(frame_masks_kernel, dim3(frame_grid(tiles, kFrameThreads / kFrameTile)), dim3(kFrameThreads), 0, s,
                     reinterpret_cast<const double2 *>(uv), in_image, reinterpret_cast<const float4 *>(rows), cap, tiles, boxes, M, mask,
                     label_mask);
  hipLaunchKernelGGL(frame_prefix_kernel, dim3(M), dim3(kFrameThreads), 0, s, mask, label_mask, tiles, prefix, counts);
  return check_launch("frame_count");
}

extern "C" int pvcnn_frame_pack(const float *rows, long long cap, const unsigned long long *mask, const unsigned long long *label_mask,
                                const int *prefix, int M, const long long *kept, const long long *offsets, long long W, long long R,
                                float *out_rows, unsigned char *out_labels, void *stream) {
  PVCNN_REQUIRE(cap >= 1 && cap <= kFrameMaxPoints, "a scan buffer holds between 1 and 2^30 points");
  PVCNN_REQUIRE(M >= 1 && M <= PVCNN_FRAME_MAX_BOXES && W >= 0 && W <= M && R >= 0, "bad sizes");
  if (W == 0 || R == 0) return 0;
  PVCNN_REQUIRE(rows && mask && prefix && kept && offsets && out_rows, "null pointer");
  PVCNN_REQUIRE(aligned16(rows) && aligned16(out_rows), "rows must be 16-byte aligned");
  const long long tiles = pvcnn_frame_tiles(cap);
  hipLaunchKernelGGL(frame_pack_kernel, dim3(frame_grid(tiles, kFrameThreads / kFrameTile), (unsigned)W), dim3(kFrameThreads), 0,
                     static_cast<hipStream_t>(stream), reinterpret_cast<const float4 *>(rows), cap, tiles, mask, label_mask, prefix, M,
                     reinterpret_cast<const int64_t *>(kept), reinterpret_cast<const int64_t *>(offsets), R,
                     reinterpret_cast<float4 *>(out_rows), out_labels);
  return check_launch("frame_pack");
}

extern "C" int pvcnn_frame_batch(const float *rows, long long cap, const unsigned long long *mask, const int *prefix, const int *counts,
                                 const double *boxes, int M, int Bmax, int num_points, int K, int rotate, int min_points,
                                 double min_box_height, const int *choices, const long long *seed, float *features,
                                 float *one_hot_vectors, float *rotation_angle, double *rgb_score, unsigned char *valid, void *stream) {
  PVCNN_REQUIRE(cap >= 1 && cap <= kFrameMaxPoints, "a scan buffer holds between 1 and 2^30 points");
  PVCNN_REQUIRE(M >= 0 && M <= PVCNN_FRAME_MAX_BOXES && Bmax >= M && Bmax <= PVCNN_FRAME_MAX_BOXES, "Bmax >= M boxes, at most 4096");
  PVCNN_REQUIRE(num_points >= 1 && num_points <= (1 << 20) && K >= 1 && K <= 512, "num_points or number of classes out of range");
  if (Bmax == 0) return 0;
  PVCNN_REQUIRE(M == 0 || (rows && mask && prefix && counts && boxes), "null pointer (rows, mask, prefix, counts, boxes)");
  PVCNN_REQUIRE(M == 0 || choices || seed, "either `choices` (parity mode) or a device `seed` (device RNG) is required");
  PVCNN_REQUIRE(features && one_hot_vectors && rotation_angle && rgb_score && valid, "null output");
  PVCNN_REQUIRE(M == 0 || aligned16(rows), "rows must be 16-byte aligned");
  FrameBatch a{};
  a.rows = reinterpret_cast<const float4 *>(rows); a.mask = mask; a.prefix = prefix; a.counts = counts; a.boxes = boxes;
  a.choices = choices; a.seed = reinterpret_cast<const int64_t *>(seed); a.cap = cap; a.tiles = pvcnn_frame_tiles(cap);
  a.M = M; a.N = num_points; a.K = K; a.rotate = rotate; a.min_points = min_points; a.min_box_height = min_box_height;
  a.features = features; a.one_hot = one_hot_vectors; a.rotation_angle = rotation_angle; a.rgb_score = rgb_score; a.valid = valid;
  hipLaunchKernelGGL(frame_batch_kernel, dim3(Bmax), dim3(kFrameThreads), 0, static_cast<hipStream_t>(stream), a);
  return check_launch("frame_batch");
}

extern "C" int pvcnn_frame_rotate_rows(float *rows, long long R, const long long *offsets, long long W, const double *cos_sin,
                                       void *stream) {
  PVCNN_REQUIRE(R >= 0 && R <= (1ll << 40) && W >= 0 && W <= (1ll << 31), "bad sizes");
  if (R == 0 || W == 0) return 0;
  PVCNN_REQUIRE(rows && offsets && cos_sin && aligned16(rows), "null or misaligned pointer");
  PVCNN_REQUIRE((R + kFrameThreads - 1) / kFrameThreads <= 0x7fffffffll, "too many rows for one launch");
  hipLaunchKernelGGL(frame_rotate_rows_kernel, dim3(frame_grid(R, kFrameThreads)), dim3(kFrameThreads), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<float4 *>(rows), R, reinterpret_cast<const int64_t *>(offsets), W, cos_sin);
  return check_launch("frame_rotate_rows");
}
