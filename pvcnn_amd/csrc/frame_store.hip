// frame_store.hip -- Frustum-KITTI training batches straight from the frames: a fresh perturbation of every sample's 2-D box
// (pvcnn_amd/frame_store.py; the definition: include/pvcnn_hip.h, "KITTI frame store"; the numpy truth: tests/frame_store_truth.py).
//
// The original preparation draws five shifted and rescaled copies of every ground-truth 2-D box once, offline, and keeps those that are
// still 25 px high and still hold a point of the object.  A perturbed box selects OTHER points of the sweep, so the draw cannot be made
// on a packed frustum: it is made here, where the sweep is -- the in-image points of every frame live in device memory, and a sample
// is cut out of its frame when the batch is assembled.
//
// ONE WORKGROUP PER SAMPLE, one launch, no scratch in global memory:
//   (a) thread 0 draws (or takes) the perturbed box and its frustum angle;
//   (b) the sixteen waves walk the frame's points once, 64 at a time: a ballot per box gives the tile's mask word of the perturbed and
//       of the unperturbed box (both in LDS), a ballot of "selected and inside the 3-D box" the positives (integer counts: their order
//       of addition is free); then the tile counts are scanned into the two prefixes (wave.h's scan inside a wave, the wave totals
//       through LDS);
//   (c) the perturbed box is used iff it is high enough and holds a positive point, else the item's own box;
//   (d) every output position finds its point through the prefix of the box used (a binary search in LDS, then select-k-th-bit of one
//       mask word, as frames.hip does it), labels it with the box-frame test, rotates, flips, shifts and writes it.
// The frame walk reads 32 bytes per point (uv fp64 x 2, the fp32 row): 640 KB of a 20 k-point frame per sample, from L2 / HBM.
// LDS: 24 bytes per tile of the store's largest frame (48 KB at the cap of 2^17 points).  All geometry is fp64, one rounding per
// operation; no atomics; every index read from device memory is clamped to the store.
#include "common.h"
#include "frame_tiles.h"
#include "philox.h"
#include "wave.h"

namespace pvcnn {

constexpr int kFsThreads = 1024;               // 16 waves: the walk over a 20 k-point frame is 20 trips, the tile scan one
constexpr int kFsWaves = kFsThreads / kWave;
constexpr int kFsItemCols = PVCNN_FRAME_STORE_ITEM_COLUMNS;
constexpr int kFsParams = PVCNN_FRAME_STORE_PARAMS;
constexpr long long kFsMaxPoints = PVCNN_FRAME_STORE_MAX_POINTS;

struct FrameStoreBatch {
  const float4 *rows;                          // (R) fp32 rows of the in-image points of every frame
  const double2 *uv;                           // (R) their image coordinates
  const int64_t *frame_offsets;                // (F + 1)
  const double *item_f64;                      // (W, kFsItemCols)
  const float *item_f32;                       // (W, K + 3): one-hot, size residual
  const int64_t *item_i64;                     // (W, 3): frame, size template id, class id
  const int64_t *order, *cursor, *seed;
  const double *params, *flip, *shift;         // parity draws
  const int32_t *choices;
  long long R, F, W, order_len, max_tiles;
  int K, bins, rotate, random_flip, random_shift, N;
  double shift_ratio, min_box_height;
  float *features, *one_hot, *center, *heading_residual, *size_residual;
  int64_t *mask_logits, *heading_bin_id, *size_template_id, *class_id;
  double *params_out, *flip_out, *shift_out;
  int32_t *used, *choices_out;
};

// numpy's % on doubles: fmod, then the divisor added when the remainder is non-zero and of the other sign (m > 0 here)
__device__ __forceinline__ double fs_floor_mod(double x, double m) {
  const double r = fmod(x, m);
  if (r == 0.0) return 0.0;
  return r < 0.0 ? r + m : r;
}

// pvcnn_amd.data.angle_to_bin_id
__device__ __forceinline__ void fs_angle_to_bin(double angle, int bins, long long &bin, float &residual) {
  const double two_pi = 2.0 * 3.141592653589793;
  const double a = fs_floor_mod(angle, two_pi);
  const double per_bin = two_pi / (double)bins;
  const double shifted = fs_floor_mod(a + per_bin / 2.0, two_pi);
  const int id = (int)(shifted / per_bin);
  bin = id;
  residual = (float)(shifted - ((double)id * per_bin + per_bin / 2.0));
}

__global__ __launch_bounds__(kFsThreads) void frame_store_batch_kernel(FrameStoreBatch a) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long fs_lds[];
  __shared__ double s_box[8];                  // the perturbed box, its rotation angle, cos, sin
  __shared__ int s_tot[2][kFsWaves], s_pos[2][kFsWaves];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6, N = a.N, K = a.K;
  const long long T = a.max_tiles;
  unsigned long long *s_mask = fs_lds;                               // [2][T]: perturbed, unperturbed
  int *s_prefix = reinterpret_cast<int *>(fs_lds + 2 * T);           // [2][T + 1]

  // the item of this sample and the points of its frame (workgroup-uniform)
  const long long item = sample_item(a.order, a.cursor, a.order_len, a.W, b);
  const double *it = a.item_f64 + item * kFsItemCols;
  const long long frame = clampll(a.item_i64[item * 3], 0ll, a.F - 1);
  const long long start = clampll(a.frame_offsets[frame], 0ll, a.R);
  long long room = a.R - start;
  if (room > T * kFrameTile) room = T * kFrameTile;
  const long long n = clampll(a.frame_offsets[frame + 1] - start, 0ll, room);
  const long long tiles = (n + kFrameTile - 1) / kFrameTile;
  const bool parity = a.choices != nullptr, perturb = a.shift_ratio != 0.0;
  const DrawStream d = draw_stream(parity ? nullptr : a.seed);

  // (a) the perturbed box and its frustum angle
  if (t == 0) {
    double u[4] = {0.0, 0.0, 0.0, 0.0}, bx[4] = {it[3], it[4], it[5], it[6]}, ang = it[19], c = it[20], s = it[21];
    if (perturb && parity) {
      const double *p = a.params + (size_t)b * kFsParams;
#pragma unroll
      for (int j = 0; j < 4; ++j) { u[j] = p[j]; bx[j] = p[4 + j]; }
      ang = p[8]; c = p[9]; s = p[10];
    } else if (perturb) {
      const uint4 r4 = draw_words(d, 0u, b, kDrawBox);
      u[0] = unit_f64(r4.x); u[1] = unit_f64(r4.y); u[2] = unit_f64(r4.z); u[3] = unit_f64(r4.w);
      const double r = a.shift_ratio;
      const double w = bx[2] - bx[0], h = bx[3] - bx[1], cx = (bx[0] + bx[2]) / 2.0, cy = (bx[1] + bx[3]) / 2.0;
      const double cx2 = cx + (w * r) * (u[0] * 2.0 - 1.0), cy2 = cy + (h * r) * (u[1] * 2.0 - 1.0);
      const double h2 = h * ((1.0 + (u[2] * 2.0) * r) - r), w2 = w * ((1.0 + (u[3] * 2.0) * r) - r);
      bx[0] = cx2 - w2 / 2.0; bx[1] = cy2 - h2 / 2.0; bx[2] = cx2 + w2 / 2.0; bx[3] = cy2 + h2 / 2.0;
      const double cu = (bx[0] + bx[2]) / 2.0;
      const double X = ((cu - it[1]) * 20.0) / it[0] + it[2] / (-it[0]);
      ang = 1.5707963267948966 + (-atan2(20.0, X));
      c = cos(ang); s = sin(ang);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) s_box[j] = bx[j];
    s_box[4] = ang; s_box[5] = c; s_box[6] = s;
    if (a.params_out) {
      double *p = a.params_out + (size_t)b * kFsParams;
#pragma unroll
      for (int j = 0; j < 4; ++j) { p[j] = u[j]; p[4 + j] = bx[j]; }
      p[8] = ang; p[9] = c; p[10] = s; p[11] = 0.0;
    }
  }
  __syncthreads();

  // (b) one walk over the frame's points: the mask words of both boxes, their positives, then the two prefixes
  const double px0 = s_box[0], py0 = s_box[1], px1 = s_box[2], py1 = s_box[3];
  const double ux0 = it[3], uy0 = it[4], ux1 = it[5], uy1 = it[6];
  const double bh = it[7], bw = it[8], bl = it[9], tx = it[10], ty = it[11], tz = it[12], cr = it[13], sr = it[14];
  const double2 *uvp = a.uv + start;
  const float4 *rp = a.rows + start;
  int positives[2] = {0, 0};                   // wave-uniform
  for (long long tile = wave; tile < tiles; tile += kFsWaves) {
    const long long i = tile * kFrameTile + lane;
    const bool live = i < n;
    double2 p = make_double2(0.0, 0.0);
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) { p = uvp[i]; r = rp[i]; }
    const bool in_p = live && p.x >= px0 && p.x < px1 && p.y >= py0 && p.y < py1;
    const bool in_u = live && p.x >= ux0 && p.x < ux1 && p.y >= uy0 && p.y < uy1;
    const bool inside = inside_box3d((double)r.x - tx, (double)r.y - ty, (double)r.z - tz, bh, bw, bl, cr, sr);
    const unsigned long long mp = __ballot(in_p), mu = __ballot(in_u);
    positives[0] += __popcll(__ballot(in_p && inside));
    positives[1] += __popcll(__ballot(in_u && inside));
    if (lane == 0) { s_mask[tile] = mp; s_mask[T + tile] = mu; }
  }
  if (lane == 0) { s_pos[0][wave] = positives[0]; s_pos[1][wave] = positives[1]; }
  __syncthreads();                             // (also publishes the mask words)
  positives[0] = positives[1] = 0;
#pragma unroll
  for (int w = 0; w < kFsWaves; ++w) { positives[0] += s_pos[0][w]; positives[1] += s_pos[1][w]; }
  int total[2] = {0, 0};
  for (long long base = 0; base < tiles; base += kFsThreads) {
    const long long tile = base + t;
    int v[2], inc[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      v[q] = tile < tiles ? __popcll(s_mask[q * T + tile]) : 0;
      inc[q] = wave_inclusive_scan(v[q], lane);
      if (lane == kWave - 1) s_tot[q][wave] = inc[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      int before = 0, chunk = 0;
#pragma unroll
      for (int w = 0; w < kFsWaves; ++w) {
        const int x = s_tot[q][w];
        if (w < wave) before += x;
        chunk += x;
      }
      if (tile < tiles) s_prefix[q * (T + 1) + tile] = total[q] + before + inc[q] - v[q];
      total[q] += chunk;
    }
    __syncthreads();                           // the wave totals have been read before the next chunk overwrites them
  }
  if (t == 0) { s_prefix[tiles] = total[0]; s_prefix[(T + 1) + tiles] = total[1]; }
  __syncthreads();

  // (c) the original's rule: high enough and one point of the object, else the item's own box with the host's angle
  const bool accept = perturb && (py1 - py0 >= a.min_box_height) && positives[0] > 0;
  const int q = accept ? 0 : 1;
  const int k = total[q];
  const unsigned long long *mk = s_mask + q * T;
  const int *pf = s_prefix + q * (T + 1);
  const double ang = accept ? s_box[4] : it[19], c = accept ? s_box[5] : it[20], s = accept ? s_box[6] : it[21];

  // the targets that depend on the rotation used and on the flip and shift draws
  double cen[3] = {it[16], it[17], it[18]}, heading = it[15];
  if (a.rotate) {
    rotate_y(cen[0], cen[2], c, s);
    heading = heading - ang;
  }
  const double dist = sqrt(cen[0] * cen[0] + cen[1] * cen[1]);
  const FlipShift fs = draw_flip_shift(d, b, a.random_flip, a.random_shift, parity, a.flip, a.shift);
  const bool flipped = fs.flipped;
  // np.clip(randn() * dist * 0.05, dist * 0.8, dist * 1.2): the reference's expression as written
  const double shift = a.random_shift ? fmin(fmax(fs.z * dist * 0.05, dist * 0.8), dist * 1.2) : 0.0;
  if (t == 0) {
    long long bin;
    float residual;
    fs_angle_to_bin(flipped ? 3.141592653589793 - heading : heading, a.bins, bin, residual);
    a.heading_bin_id[b] = bin;
    a.heading_residual[b] = residual;
    a.size_template_id[b] = a.item_i64[item * 3 + 1];
    a.class_id[b] = a.item_i64[item * 3 + 2];
    if (a.used) a.used[b] = accept ? 1 : 0;
    if (a.flip_out) a.flip_out[b] = flipped ? 1.0 : 0.0;
    if (a.shift_out) a.shift_out[b] = fs.z;
  }
  if (t < 3) {
    double v = cen[t];
    if (t == 0 && flipped) v = -v;
    if (t == 2 && a.random_shift) v += shift;
    a.center[(size_t)b * 3 + t] = (float)v;
    a.size_residual[(size_t)b * 3 + t] = a.item_f32[item * (K + 3) + K + t];
  }
  for (int j = t; j < K; j += kFsThreads) a.one_hot[(size_t)b * K + j] = a.item_f32[item * (K + 3) + j];

  // (d) the points
  float *f = a.features + (size_t)b * 4 * N;
  for (int p = t; p < N; p += kFsThreads) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    long long label = 0;
    int pos = 0;
    if (k > 0) {
      pos = parity ? min(max(a.choices[(size_t)b * N + p], 0), k - 1) : (int)draw_index(d, p, b, k);
      long long i = frame_pick(pf, mk, tiles, pos);
      if (i > n - 1) i = n - 1;
      v = rp[i];
      label = inside_box3d((double)v.x - tx, (double)v.y - ty, (double)v.z - tz, bh, bw, bl, cr, sr) ? 1 : 0;
      if (a.rotate) rotate_y(v, c, s);
      if (flipped) v.x = -v.x;
      if (a.random_shift) v.z = (float)((double)v.z + shift);
    }
    store_planes4(f, N, p, v);
    a.mask_logits[(size_t)b * N + p] = label;
    if (a.choices_out) a.choices_out[(size_t)b * N + p] = pos;
  }
}

}  // namespace pvcnn

using namespace pvcnn;

extern "C" size_t pvcnn_frame_store_lds_bytes(long long max_frame_points) {
  if (max_frame_points < 1 || max_frame_points > kFsMaxPoints) return 0;
  const size_t tiles = (size_t)((max_frame_points + kFrameTile - 1) / kFrameTile);
  return 2 * tiles * 8 + ((2 * (tiles + 1) * 4 + 15) & ~(size_t)15);
}

extern "C" int pvcnn_frame_store_batch(const float *rows, const double *uv, const int64_t *frame_offsets, long long F, long long R,
                                       long long max_frame_points, const double *item_f64, const float *item_f32,
                                       const int64_t *item_i64, long long W, int K, int num_heading_angle_bins, int frustum_rotate,
                                       int random_flip, int random_shift, double shift_ratio, double min_box_height,
                                       const int64_t *order, long long order_len, const int64_t *cursor, int B, int N,
                                       const double *params, const int32_t *choices, const double *flip, const double *shift,
                                       const int64_t *seed, float *features, float *one_hot_vectors, int64_t *mask_logits, float *center,
                                       int64_t *heading_bin_id, float *heading_residual, int64_t *size_template_id, float *size_residual,
                                       int64_t *class_id, double *params_out, int32_t *used, int32_t *choices_out, double *flip_out,
                                       double *shift_out, void *stream) {
  PVCNN_REQUIRE(B >= 0 && B <= 65535 && N >= 1 && N <= (1 << 20), "batch size or num_points out of range");
  PVCNN_REQUIRE(F >= 1 && W >= 1 && R >= 1 && order_len >= 1, "empty store or empty order");
  PVCNN_REQUIRE(max_frame_points >= 1 && max_frame_points <= kFsMaxPoints, "a frame holds between 1 and 2^17 in-image points");
  PVCNN_REQUIRE(K >= 1 && K <= 512 && num_heading_angle_bins >= 1, "number of classes or heading bins out of range");
  PVCNN_REQUIRE(shift_ratio >= 0.0 && shift_ratio < 1.0, "shift_ratio must lie in [0, 1)");
  if (B == 0) return 0;
  PVCNN_REQUIRE(rows && uv && frame_offsets && item_f64 && item_f32 && item_i64 && order, "null pointer (store, item tables, order)");
  PVCNN_REQUIRE(aligned16(rows) && aligned16(uv), "rows and uv must be 16-byte aligned");
  PVCNN_REQUIRE(choices || seed, "either `choices` (parity mode) or a device `seed` (device RNG) is required");
  PVCNN_REQUIRE(choices || !(params || flip || shift), "parity draws (`params`, `flip`, `shift`) need `choices`: parity mode takes every draw from the caller");
  PVCNN_REQUIRE(!(choices && shift_ratio != 0.0 && !params), "parity mode with a box perturbation needs the `params` rows (B, 12) fp64");
  PVCNN_REQUIRE(!(choices && random_flip && !flip), "parity mode with random_flip needs the `flip` draws (B) fp64");
  PVCNN_REQUIRE(!(choices && random_shift && !shift), "parity mode with random_shift needs the `shift` draws (B) fp64");
  PVCNN_REQUIRE(features && one_hot_vectors && mask_logits && center && heading_bin_id && heading_residual && size_template_id &&
                    size_residual && class_id, "null output");
  FrameStoreBatch a{};
  a.rows = reinterpret_cast<const float4 *>(rows); a.uv = reinterpret_cast<const double2 *>(uv); a.frame_offsets = frame_offsets;
  a.item_f64 = item_f64; a.item_f32 = item_f32; a.item_i64 = item_i64; a.order = order; a.cursor = cursor; a.seed = seed;
  a.params = params; a.flip = flip; a.shift = shift; a.choices = choices;
  a.R = R; a.F = F; a.W = W; a.order_len = order_len; a.max_tiles = (max_frame_points + kFrameTile - 1) / kFrameTile;
  a.K = K; a.bins = num_heading_angle_bins; a.rotate = frustum_rotate; a.random_flip = random_flip; a.random_shift = random_shift; a.N = N;
  a.shift_ratio = shift_ratio; a.min_box_height = min_box_height;
  a.features = features; a.one_hot = one_hot_vectors; a.center = center; a.heading_residual = heading_residual;
  a.size_residual = size_residual; a.mask_logits = mask_logits; a.heading_bin_id = heading_bin_id; a.size_template_id = size_template_id;
  a.class_id = class_id; a.params_out = params_out; a.flip_out = flip_out; a.shift_out = shift_out; a.used = used;
  a.choices_out = choices_out;
  hipLaunchKernelGGL(frame_store_batch_kernel, dim3(B), dim3(kFsThreads), pvcnn_frame_store_lds_bytes(max_frame_points),
                     static_cast<hipStream_t>(stream), a);
  return check_launch("frame_store_batch");
}
