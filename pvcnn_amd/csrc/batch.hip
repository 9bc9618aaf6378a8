// batch.hip -- training batches assembled on the device from a split that lives in device memory (pvcnn_amd/data.py).
//
// Reference: datasets/s3dis.py:81-94, datasets/shapenet.py:62-81, datasets/kitti/frustum.py:95-147 -- one __getitem__ per cloud on
// the host (numpy draws, a fancy-indexed copy, a transpose), then default_collate, pin and copy.  Here one workgroup per batch sample
// writes the collated batch straight into the caller's tensors: the item is order[cursor[0] + b] (both in DEVICE memory, so a replayed
// graph walks an epoch), the draws come from the caller (`choices` ...: PARITY MODE, bit-identical to the reference for numpy's draws)
// or from a Philox4x32-10 stream keyed by two int64 words in device memory, and everything that does not depend on a draw has been
// computed once on the host when the store was built.
//
// STORE LAYOUT: packed, ragged, ROW-major -- item i owns rows offsets[i] .. offsets[i+1] of `rows` (R, C) fp32, C = 9 / 6 / 4, and of
// `labels` (R) in the narrowest integer type.  Row-major because the access is a gather of random rows: a 36-byte row lies in one or
// two 128-byte lines, the same point in a channel-major item would touch C lines C * n * 4 bytes apart.  The lanes of a wave read 64
// random rows and write 64 consecutive floats of each output channel plane (B, C, N): the writes are coalesced, the reads cannot be.
// All row addressing is 64-bit (a packed split may hold more than 2^31 floats); only an item's own row count must fit an int.
//
// SELECTION in device mode.  With replacement: one Philox word r per output point, index = mulhi(r, n): every index has floor or ceil
// of 2^32 / n preimages, a relative bias of at most n / 2^32 (2e-6 at n = 8192).  Without replacement (S3DIS, n >= N): "N distinct of
// n in random order" = the N smallest of n random 32-bit keys, ordered by key.  The n words key << 32 | index are sorted in LDS by a
// bitonic network (padded to a power of two <= 8192 with all-ones words: 64 KB; log^2 steps of n/2 exchanges instead of the n^2
// comparisons of rank counting).  The index in the low half makes all words distinct, so the network's result is one total order
// whatever the keys; two keys collide with probability 2^-32 per pair and are then ordered by index, which moves a point's inclusion
// probability by less than n * 2^-32 -- the same bound as above.
//
// Positions and items outside [0, order_len) / [0, W) and parity choices outside [0, n) are clamped: the kernels never read outside the
// store, whatever the device words hold.  An empty item yields zeros.
#include "common.h"
#include "frame_tiles.h"
#include "philox.h"

namespace pvcnn {

constexpr int kBatchThreads = 1024;
constexpr int kBatchMaxSort = 8192;            // words of the LDS-resident selection without replacement

struct BatchStore {
  const float *rows;                           // (R, C) fp32
  const void *labels;                          // (R) of label_bytes each (1: uint8, 2: int16, 4: int32, 8: int64); may be null (detection form)
  const int64_t *offsets;                      // (W + 1)
  const int64_t *order, *cursor;               // order (order_len); cursor one word or null (= 0)
  const int32_t *choices;                      // (B, N) or null
  const int64_t *seed;                         // 2 words or null
  long long W, order_len;
  int label_bytes, N;
};

__device__ __forceinline__ long long batch_label(const BatchStore &s, long long row) {
  switch (s.label_bytes) {
    case 1: return static_cast<const uint8_t *>(s.labels)[row];
    case 2: return static_cast<const int16_t *>(s.labels)[row];
    case 4: return static_cast<const int32_t *>(s.labels)[row];
    default: return static_cast<const int64_t *>(s.labels)[row];
  }
}

// the item of sample b: its index, first row and row count (workgroup-uniform)
__device__ __forceinline__ long long batch_item(const BatchStore &s, int b, long long &start, int &n) {
  const long long item = sample_item(s.order, s.cursor, s.order_len, s.W, b);
  start = s.offsets[item];
  n = (int)clampll(s.offsets[item + 1] - start, 0ll, 0x7fffffffll);
  return item;
}

// words[0 .. N) <- N distinct of n in random order (low halves); npad = n rounded up to a power of two <= kBatchMaxSort
__device__ __forceinline__ void batch_sort_select(unsigned long long *words, int n, int b, const DrawStream &d) {
  int npad = 1;
  while (npad < n) npad <<= 1;
  for (int i = threadIdx.x; i < npad; i += kBatchThreads)
    words[i] = i < n ? draw_sort_word(d, i, b) : ~0ull;
  __syncthreads();
  for (int k = 2; k <= npad; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (npad >> 1); t += kBatchThreads) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo + j;
        const unsigned long long x = words[lo], y = words[hi];
        if ((x > y) == ((lo & k) == 0)) { words[lo] = y; words[hi] = x; }
      }
      __syncthreads();
    }
  }
}

// the row (within its item) of output point p
__device__ __forceinline__ int batch_pick(const BatchStore &s, const unsigned long long *words, bool sorted, int b, int p, int n,
                                          const DrawStream &d) {
  if (s.choices) return min(max(s.choices[(size_t)b * s.N + p], 0), n - 1);
  if (sorted) return (int)(uint32_t)words[p];
  return (int)draw_index(d, p, b, n);
}

// ---- S3DIS: features (B, c_out, N) = the first c_out of 9 stored channels, targets (B, N) ----
__global__ __launch_bounds__(kBatchThreads) void batch_s3dis_kernel(BatchStore s, int c_out, int sort_cap, float *__restrict__ features,
                                                                    int64_t *__restrict__ targets) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long batch_words[];
  const int b = blockIdx.x, N = s.N;
  long long start;
  int n;
  batch_item(s, b, start, n);
  float *f = features + (size_t)b * c_out * N;
  int64_t *tg = targets + (size_t)b * N;
  if (n == 0) {
    for (int p = threadIdx.x; p < N; p += kBatchThreads) {
      for (int c = 0; c < c_out; ++c) f[(size_t)c * N + p] = 0.f;
      tg[p] = 0;
    }
    return;
  }
  const DrawStream d = draw_stream(s.choices ? nullptr : s.seed);
  const bool sorted = !s.choices && n >= N && n <= sort_cap;        // np.random.choice(n, N, replace=n < N)
  if (sorted) batch_sort_select(batch_words, n, b, d);
  for (int p = threadIdx.x; p < N; p += kBatchThreads) {
    const long long row = start + batch_pick(s, batch_words, sorted, b, p, n, d);
    const float *r = s.rows + row * 9;
    float v[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) v[c] = r[c];
#pragma unroll
    for (int c = 0; c < 9; ++c)
      if (c < c_out) f[(size_t)c * N + p] = v[c];
    tg[p] = batch_label(s, row);
  }
}

// ---- ShapeNet: features (B, 3 [+3] [+num_shapes], N): jittered coords, normals, one-hot plane; targets (B, N) ----
__global__ __launch_bounds__(kBatchThreads) void batch_shapenet_kernel(BatchStore s, const int32_t *__restrict__ shape_ids, int with_normal,
                                                                       int num_shapes, int jitter_on, const double *__restrict__ jitter,
                                                                       float *__restrict__ features, int64_t *__restrict__ targets) {
  const int b = blockIdx.x, N = s.N;
  long long start;
  int n;
  const long long item = batch_item(s, b, start, n);
  const int c_out = 3 + (with_normal ? 3 : 0) + num_shapes, c_hot = 3 + (with_normal ? 3 : 0);
  const int shape = shape_ids[item];
  float *f = features + (size_t)b * c_out * N;
  int64_t *tg = targets + (size_t)b * N;
  const DrawStream d = draw_stream(s.choices ? nullptr : s.seed);
  for (int p = threadIdx.x; p < N; p += kBatchThreads) {
    float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    long long label = 0;
    if (n > 0) {
      const long long row = start + batch_pick(s, nullptr, false, b, p, n, d);
      const float *r = s.rows + row * 6;
#pragma unroll
      for (int c = 0; c < 6; ++c) v[c] = r[c];
      label = batch_label(s, row);
      if (jitter_on) {                         // fp32(clip(0.01 * z, -0.05, 0.05)) + coord
        if (s.choices) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const double z = jitter[((size_t)b * 3 + c) * N + p];
            v[c] = (float)fmin(fmax(0.01 * z, -0.05), 0.05) + v[c];
          }
        } else {
          const uint4 r4 = draw_words(d, p, b, kDrawJitter);
          const float2 za = normal2_f32(r4.x, r4.y), zb = normal2_f32(r4.z, r4.w);
          v[0] = fminf(fmaxf(0.01f * za.x, -0.05f), 0.05f) + v[0];
          v[1] = fminf(fmaxf(0.01f * za.y, -0.05f), 0.05f) + v[1];
          v[2] = fminf(fmaxf(0.01f * zb.x, -0.05f), 0.05f) + v[2];
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) f[(size_t)c * N + p] = v[c];
    if (with_normal) {
#pragma unroll
      for (int c = 3; c < 6; ++c) f[(size_t)c * N + p] = v[c];
    }
    for (int k = 0; k < num_shapes; ++k) f[(size_t)(c_hot + k) * N + p] = (k == shape && n > 0) ? 1.f : 0.f;
    tg[p] = label;
  }
}

// ---- Frustum-KITTI ----
struct BatchFrustum {
  // per item, computed on the host when the store was built
  const double *item_f64;                      // (W, 4): centre x y z (after the frustum rotation), dist  | detection form (W, 1): rgb_score
  const float *item_f32;                       // (W, K + 5): one-hot, heading residual [no flip, flip], size residual  | (W, K + 1): one-hot, rotation angle
  const int64_t *item_i64;                     // (W, 4): heading bin [no flip, flip], size template id, class id       | null
  const double *flip, *shift;                  // parity draws (B) or null
  int K, random_flip, random_shift, rgb;
  float *features, *one_hot;                   // (B, 4, N), (B, K)
  int64_t *mask_logits;                        // (B, N)
  float *center, *heading_residual, *size_residual;          // (B, 3), (B), (B, 3)
  int64_t *heading_bin_id, *size_template_id, *class_id;     // (B) each
  float *rotation_angle;                       // detection form: (B)
  double *rgb_score;                           //                 (B)
};

__global__ __launch_bounds__(kBatchThreads) void batch_frustum_kernel(BatchStore s, BatchFrustum a) {
  const int b = blockIdx.x, N = s.N, K = a.K;
  long long start;
  int n;
  const long long item = batch_item(s, b, start, n);
  const DrawStream d = draw_stream(s.choices ? nullptr : s.seed);
  bool flipped = false;
  double shift = 0.0;
  if (!a.rgb) {
    const FlipShift fs = draw_flip_shift(d, b, a.random_flip, a.random_shift, s.choices != nullptr, a.flip, a.shift);
    flipped = fs.flipped;
    if (a.random_shift) {                      // np.clip(randn() * dist * 0.05, dist * 0.8, dist * 1.2): the reference's expression as written
      const double dist = a.item_f64[item * 4 + 3];
      shift = fmin(fmax(fs.z * dist * 0.05, dist * 0.8), dist * 1.2);
    }
  }
  float *f = a.features + (size_t)b * 4 * N;
  for (int p = threadIdx.x; p < N; p += kBatchThreads) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    long long label = 0;
    if (n > 0) {
      const long long row = start + batch_pick(s, nullptr, false, b, p, n, d);
      const float *r = s.rows + row * 4;
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = r[c];
      if (!a.rgb) label = batch_label(s, row);
      if (flipped) v[0] = -v[0];
      if (a.random_shift && !a.rgb) v[2] = (float)((double)v[2] + shift);            // fp64 sum, rounded once
    }
    store_planes4(f, N, p, make_float4(v[0], v[1], v[2], v[3]));
    if (!a.rgb) a.mask_logits[(size_t)b * N + p] = label;
  }
  // the per-item words: a few lanes of the first wave
  const int t = threadIdx.x;
  if (a.rgb) {
    const float *i32 = a.item_f32 + item * (K + 1);
    if (t < K) a.one_hot[(size_t)b * K + t] = i32[t];
    if (t == K) a.rotation_angle[b] = i32[K];
    if (t == K + 1) a.rgb_score[b] = a.item_f64[item];
    return;
  }
  const float *i32 = a.item_f32 + item * (K + 5);
  const int fl = flipped ? 1 : 0;
  if (t < K) a.one_hot[(size_t)b * K + t] = i32[t];
  if (t >= K && t < K + 3) {
    const int c = t - K;
    double v = a.item_f64[item * 4 + c];
    if (c == 0 && flipped) v = -v;
    if (c == 2 && a.random_shift) v += shift;
    a.center[(size_t)b * 3 + c] = (float)v;
    a.size_residual[(size_t)b * 3 + c] = i32[K + 2 + c];
  }
  if (t == K + 3) {
    a.heading_bin_id[b] = a.item_i64[item * 4 + fl];
    a.heading_residual[b] = i32[K + fl];
    a.size_template_id[b] = a.item_i64[item * 4 + 2];
    a.class_id[b] = a.item_i64[item * 4 + 3];
  }
}

static int batch_store_check(const char *fn, const BatchStore &s, int B, bool labels_needed) {
#define BATCH_REQ(cond, msg) do { if (!(cond)) { set_error("%s: %s", fn, msg); return PVCNN_ERR_INVALID_ARGUMENT; } } while (0)
  BATCH_REQ(B >= 0 && s.N >= 0 && s.W >= 0 && s.order_len >= 0, "negative size");
  if (B == 0 || s.N == 0) return 1;
  BATCH_REQ(s.W > 0 && s.order_len > 0, "empty store or empty order");
  BATCH_REQ(s.rows && s.offsets && s.order, "null pointer (rows, offsets, order)");
  BATCH_REQ(!labels_needed || s.labels, "null pointer (labels)");
  BATCH_REQ(s.label_bytes == 1 || s.label_bytes == 2 || s.label_bytes == 4 || s.label_bytes == 8, "label_bytes must be 1, 2, 4 or 8");
  BATCH_REQ(s.choices || s.seed, "either `choices` (parity mode) or a device `seed` (device RNG) is required");
  BATCH_REQ(B <= 65535 * 32767, "batch too large");
#undef BATCH_REQ
  return 0;
}

}  // namespace pvcnn

using namespace pvcnn;

extern "C" size_t pvcnn_batch_lds_bytes(int N, int max_n) {
  if (N <= 0 || max_n < N || max_n > kBatchMaxSort) return 0;
  size_t npad = 1;
  while (npad < (size_t)max_n) npad <<= 1;
  return npad * 8;
}

extern "C" int pvcnn_batch_s3dis(const float *rows, const void *labels, int label_bytes, const int64_t *offsets, long long W, int max_n,
                                 const int64_t *order, long long order_len, const int64_t *cursor, int B, int N, int C_out,
                                 const int32_t *choices, const int64_t *seed, float *features, int64_t *targets, void *stream) {
  const BatchStore s{rows, labels, offsets, order, cursor, choices, seed, W, order_len, label_bytes, N};
  const int rc = batch_store_check(__func__, s, B, true);
  if (rc != 0) return rc < 0 ? rc : 0;
  PVCNN_REQUIRE(C_out == 9 || C_out == 6, "C_out must be 9 (with normalised coordinates) or 6");
  PVCNN_REQUIRE(features && targets, "null output");
  PVCNN_REQUIRE(max_n >= 1, "max_n (the largest item of the store) must be positive");
  PVCNN_REQUIRE(choices || max_n < N || max_n <= kBatchMaxSort,
                "sampling without replacement from items beyond the LDS-resident selection (8192 points)");
  const size_t lds = choices ? 0 : pvcnn_batch_lds_bytes(N, max_n);
  hipLaunchKernelGGL(batch_s3dis_kernel, dim3(B), dim3(kBatchThreads), lds, static_cast<hipStream_t>(stream), s, C_out, (int)(lds / 8),
                     features, targets);
  return check_launch("batch_s3dis");
}

extern "C" int pvcnn_batch_shapenet(const float *rows, const void *labels, int label_bytes, const int64_t *offsets, long long W,
                                    const int32_t *shape_ids, const int64_t *order, long long order_len, const int64_t *cursor, int B,
                                    int N, int with_normal, int num_shapes, int jitter_on, const int32_t *choices, const double *jitter,
                                    const int64_t *seed, float *features, int64_t *targets, void *stream) {
  const BatchStore s{rows, labels, offsets, order, cursor, choices, seed, W, order_len, label_bytes, N};
  const int rc = batch_store_check(__func__, s, B, true);
  if (rc != 0) return rc < 0 ? rc : 0;
  PVCNN_REQUIRE(shape_ids && features && targets, "null pointer (shape_ids, features, targets)");
  PVCNN_REQUIRE(num_shapes >= 0 && num_shapes <= 1024, "num_shapes out of range");
  PVCNN_REQUIRE(!(jitter_on && choices && !jitter), "parity mode with jitter needs the `jitter` draws (B, 3, N) fp64");
  hipLaunchKernelGGL(batch_shapenet_kernel, dim3(B), dim3(kBatchThreads), 0, static_cast<hipStream_t>(stream), s, shape_ids, with_normal,
                     num_shapes, jitter_on, jitter, features, targets);
  return check_launch("batch_shapenet");
}

extern "C" int pvcnn_batch_frustum(const float *rows, const void *labels, int label_bytes, const int64_t *offsets, long long W,
                                   const double *item_f64, const float *item_f32, const int64_t *item_i64, int K, int random_flip,
                                   int random_shift, const int64_t *order, long long order_len, const int64_t *cursor, int B, int N,
                                   const int32_t *choices, const double *flip, const double *shift, const int64_t *seed, float *features,
                                   float *one_hot_vectors, int64_t *mask_logits, float *center, int64_t *heading_bin_id,
                                   float *heading_residual, int64_t *size_template_id, float *size_residual, int64_t *class_id,
                                   void *stream) {
  const BatchStore s{rows, labels, offsets, order, cursor, choices, seed, W, order_len, label_bytes, N};
  const int rc = batch_store_check(__func__, s, B, true);
  if (rc != 0) return rc < 0 ? rc : 0;
  PVCNN_REQUIRE(item_f64 && item_f32 && item_i64, "null pointer (item tables)");
  PVCNN_REQUIRE(K >= 1 && K <= 512, "number of classes out of range");
  PVCNN_REQUIRE(features && one_hot_vectors && mask_logits && center && heading_bin_id && heading_residual && size_template_id &&
                    size_residual && class_id, "null output");
  PVCNN_REQUIRE(!(choices && random_flip && !flip), "parity mode with random_flip needs the `flip` draws (B) fp64");
  PVCNN_REQUIRE(!(choices && random_shift && !shift), "parity mode with random_shift needs the `shift` draws (B) fp64");
  BatchFrustum a{};
  a.item_f64 = item_f64; a.item_f32 = item_f32; a.item_i64 = item_i64; a.flip = flip; a.shift = shift;
  a.K = K; a.random_flip = random_flip; a.random_shift = random_shift; a.rgb = 0;
  a.features = features; a.one_hot = one_hot_vectors; a.mask_logits = mask_logits; a.center = center;
  a.heading_residual = heading_residual; a.size_residual = size_residual; a.heading_bin_id = heading_bin_id;
  a.size_template_id = size_template_id; a.class_id = class_id;
  hipLaunchKernelGGL(batch_frustum_kernel, dim3(B), dim3(kBatchThreads), 0, static_cast<hipStream_t>(stream), s, a);
  return check_launch("batch_frustum");
}

extern "C" int pvcnn_batch_frustum_rgb(const float *rows, const int64_t *offsets, long long W, const double *item_f64,
                                       const float *item_f32, int K, const int64_t *order, long long order_len, const int64_t *cursor,
                                       int B, int N, const int32_t *choices, const int64_t *seed, float *features, float *one_hot_vectors,
                                       float *rotation_angle, double *rgb_score, void *stream) {
  const BatchStore s{rows, nullptr, offsets, order, cursor, choices, seed, W, order_len, 1, N};
  const int rc = batch_store_check(__func__, s, B, false);
  if (rc != 0) return rc < 0 ? rc : 0;
  PVCNN_REQUIRE(item_f64 && item_f32, "null pointer (item tables)");
  PVCNN_REQUIRE(K >= 1 && K <= 512, "number of classes out of range");
  PVCNN_REQUIRE(features && one_hot_vectors && rotation_angle && rgb_score, "null output");
  BatchFrustum a{};
  a.item_f64 = item_f64; a.item_f32 = item_f32; a.K = K; a.rgb = 1;
  a.features = features; a.one_hot = one_hot_vectors; a.rotation_angle = rotation_angle; a.rgb_score = rgb_score;
  hipLaunchKernelGGL(batch_frustum_kernel, dim3(B), dim3(kBatchThreads), 0, static_cast<hipStream_t>(stream), s, a);
  return check_launch("batch_frustum_rgb");
}
