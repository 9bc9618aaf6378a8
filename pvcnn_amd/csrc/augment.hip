// augment.hip -- point-cloud augmentation of an assembled batch on the device (pvcnn_amd/augment.py): rotation about an axis, rotation
// perturbation, axis flips, scale, translation, clipped Gaussian jitter, random point dropout.
//
// Not in the reference: its three datasets draw only what batch.hip draws.  The transforms are the usual ones of point-cloud training
// (PointNet++'s provider.py: rotate_point_cloud_z, rotate_perturbation_point_cloud, random_scale / shift_point_cloud,
// jitter_point_cloud, random_point_dropout), fused so that a batch is read once and written once.
//
// TWO LAUNCHES.  augment_draw_kernel: one thread per cloud draws the per-cloud parameters and composes the 3x3 matrix in fp64 -- a row
// of 24 doubles (layout: include/pvcnn_hip.h).  augment_apply_kernel: one thread per point (or per 4 consecutive points, 16-byte
// accesses, when every plane of every tensor is 16-byte aligned) walks the C channel planes of its sample: the planes of a POSITION
// triple become s * (Rp x) + t + jitter, those of a DIRECTION triple Rp x, every other plane is copied.  Its traffic is one read and
// one write of the batch (plus the targets); at the size of a training batch (6 MB) that is under a microsecond of HBM time and the
// launch is bound by the latency of a point's draws instead (profiles/augment.md): see kAugVecMinPoints.
//
// ARITHMETIC.  Every output element is computed in fp64 from the fp32 input in the order
//     r = (Rp[k][0] * x0 + Rp[k][1] * x1) + Rp[k][2] * x2;   y = (s * r + t[k]) + jitter[k]
// and rounded ONCE to fp32.  The library is built with -ffp-contract=off (Makefile): no product is fused into a sum, so the torch
// formulation (augment.py: augment_reference), one rounding per operation, gives the same bits.
//
// DROPOUT as PointNet++ has it: point n > 0 whose uniform u <= ratio takes point 0's place -- the thread of a dropped point simply
// reads point 0 (its planes, its jitter draw, its target) instead of its own, so nothing is read back from `dst` and no thread
// waits for another.  That is also why dst must not overlap src when dropout is on: point 0 would be overwritten while others read it.
//
// RANDOMNESS as batch.hip: the caller's draws (PARITY MODE) or the draw stream of philox.h, keyed by two int64 words in device memory.
// The counter's last word separates the uses of one key (philox.h's table: the assembly takes 0..3, this file 16..21), so a loader
// may key its assembly and its augmentation with the same two words.
#include "common.h"
#include "philox.h"

namespace pvcnn {

constexpr int kAugThreads = 64;                // one wave per workgroup: a training batch is small, its waves should reach every CU
constexpr int kAugMaxBlocksX = 1024;           // blocks along N of one pass: beyond 65536 points (x4 vectorised) the grid strides
// A thread carries a long dependent chain per point (two Philox calls, two Box-Muller pairs, ~40 fp64 operations), so a batch of a few
// 10^4 points is bound by that latency, not by its 6 MB of traffic: below this many points one point per thread (four times the
// waves, a quarter of the chain each) beats the 16-byte accesses, which pay off once the waves fill the machine either way.
constexpr long long kAugVecMinPoints = 1ll << 18;
constexpr int kAugParams = PVCNN_AUGMENT_PARAMS;

struct AugmentConfig {
  int axis;
  double rot_max, perturb_sigma, perturb_clip, flip_x, flip_y, flip_z, scale_lo, scale_hi, translate_max, drop_max;
};

__device__ __forceinline__ double aug_clip(double v, double c) { return fmin(fmax(v, -c), c); }

struct Mat3 { double m[9]; };

// c = a b, every entry (a0 b0 + a1 b1) + a2 b2
__device__ __forceinline__ Mat3 aug_matmul(const Mat3 &a, const Mat3 &b) {
  Mat3 c;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c.m[i * 3 + j] = (a.m[i * 3] * b.m[j] + a.m[i * 3 + 1] * b.m[3 + j]) + a.m[i * 3 + 2] * b.m[6 + j];
  return c;
}

// the right-handed rotation by `angle` about axis 0 (x), 1 (y) or 2 (z):
//   Rx = [1 0 0; 0 c -s; 0 s c]   Ry = [c 0 s; 0 1 0; -s 0 c]   Rz = [c -s 0; s c 0; 0 0 1]
// (every index is a compile-time constant after unrolling: the matrix stays in registers)
__device__ __forceinline__ Mat3 aug_rotation(int axis, double angle) {
  const double c = cos(angle), s = sin(angle);
  const Mat3 rx{{1.0, 0.0, 0.0, 0.0, c, -s, 0.0, s, c}}, ry{{c, 0.0, s, 0.0, 1.0, 0.0, -s, 0.0, c}}, rz{{c, -s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0}};
  Mat3 r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.m[i] = axis == 0 ? rx.m[i] : (axis == 1 ? ry.m[i] : rz.m[i]);
  return r;
}

__global__ __launch_bounds__(kAugThreads) void augment_draw_kernel(AugmentConfig g, int B, const int64_t *__restrict__ seed,
                                                                   double *__restrict__ params) {
  const int b = blockIdx.x * kAugThreads + threadIdx.x;
  if (b >= B) return;
  const DrawStream d = draw_stream(seed);
  const uint4 r0 = draw_words(d, 0u, b, kDrawAugCloud);          // theta, scale, ratio, -
  const uint4 r1 = draw_words(d, 0u, b, kDrawAugCloud + 1u);     // the perturbation's normals
  const uint4 r2 = draw_words(d, 0u, b, kDrawAugCloud + 2u);     // flips, -
  const uint4 r3 = draw_words(d, 0u, b, kDrawAugCloud + 3u);     // translation, -
  // a range that is off leaves its draw at exactly 0 (or 1): no -0.0, no rounding
  const double theta = g.rot_max > 0.0 ? g.rot_max * (2.0 * open_f64(r0.x) - 1.0) : 0.0;
  double pa = 0.0, pb = 0.0, pc = 0.0;
  if (g.perturb_sigma > 0.0) {
    const double2 za = normal2_f64(r1.x, r1.y), zb = normal2_f64(r1.z, r1.w);
    pa = aug_clip(g.perturb_sigma * za.x, g.perturb_clip);
    pb = aug_clip(g.perturb_sigma * za.y, g.perturb_clip);
    pc = aug_clip(g.perturb_sigma * zb.x, g.perturb_clip);
  }
  const double uf[3] = {open_f64(r2.x), open_f64(r2.y), open_f64(r2.z)};
  const bool flip[3] = {uf[0] < g.flip_x, uf[1] < g.flip_y, uf[2] < g.flip_z};
  const double scale = g.scale_lo + (g.scale_hi - g.scale_lo) * open_f64(r0.y);
  const uint32_t rt[3] = {r3.x, r3.y, r3.z};
  double t[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = g.translate_max > 0.0 ? g.translate_max * (2.0 * open_f64(rt[k]) - 1.0) : 0.0;
  const double ratio = open_f64(r0.z) * g.drop_max;
  // Rp = Rx(a) Ry(b) Rz(c) R_axis(theta) diag(+-1)
  Mat3 m = aug_matmul(aug_matmul(aug_rotation(0, pa), aug_rotation(1, pb)), aug_rotation(2, pc));
  m = aug_matmul(m, aug_rotation(g.axis, theta));
  double *row = params + (size_t)b * kAugParams;
#pragma unroll
  for (int i = 0; i < 9; ++i) row[i] = (flip[i % 3] ? -m.m[i] : m.m[i]) + 0.0;           // + 0.0: a -0.0 entry becomes 0.0
  row[9] = scale;
  row[10] = t[0]; row[11] = t[1]; row[12] = t[2];
  row[13] = ratio;
  row[14] = theta; row[15] = pa; row[16] = pb; row[17] = pc;
  row[18] = uf[0]; row[19] = uf[1]; row[20] = uf[2];
  row[21] = 0.0; row[22] = 0.0; row[23] = 0.0;
}

struct AugmentApply {
  const float *src;
  float *dst;
  const int64_t *targets_src;
  int64_t *targets_dst;
  const double *params;                        // (B, 24)
  const float *jitter, *keep;                  // parity draws (B, 3, N), (B, N), or null
  const int64_t *seed;                         // 2 words, or null when no draw is made on the device
  float *jitter_out, *keep_out;                // the draws in use, or null
  long long src_stride, dst_stride, targets_src_stride, targets_dst_stride;   // batch strides in elements
  int B, C, N, jitter_on, drop_on;
  double jitter_sigma, jitter_clip;
  int first0, first1, first2, first3;          // the first plane of each triple (-1: none) ...
  int role0, role1, role2, role3;              // ... and its role
};

// V consecutive floats: one 16-byte access (V = 4, the address is 16-byte aligned) or one scalar
template <int V> struct AugVec { float v[V]; };
template <int V> __device__ __forceinline__ AugVec<V> aug_load(const float *p) {
  AugVec<V> r;
  if constexpr (V == 4) {
    const float4 q = *reinterpret_cast<const float4 *>(p);
    r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w;
  } else {
    r.v[0] = p[0];
  }
  return r;
}
template <int V> __device__ __forceinline__ void aug_store(float *p, const AugVec<V> &r) {
  if constexpr (V == 4) *reinterpret_cast<float4 *>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
  else p[0] = r.v[0];
}

// V points of one plane, each its own or point 0 when it is dropped
template <int V> __device__ __forceinline__ AugVec<V> aug_load_plane(const float *plane, int n0, bool any_dropped, const bool *dropped) {
  AugVec<V> x = aug_load<V>(plane + n0);
  if (any_dropped) {
    const float x0 = plane[0];
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (dropped[j]) x.v[j] = x0;
  }
  return x;
}

// V == 4 requires N % 4 == 0 (so a group never straddles the end of a plane) and every base / stride 16-byte aligned: the host decides.
// src and dst are not __restrict__: without dropout they may be the same view (every thread reads its points before it writes them).
template <int V>
__global__ __launch_bounds__(kAugThreads) void augment_apply_kernel(AugmentApply a) {
  const int N = a.N, C = a.C, groups = N / V;
  const bool draw_jitter = a.jitter_on && !a.jitter, draw_keep = a.drop_on && !a.keep;
  const DrawStream d = draw_stream(draw_jitter || draw_keep ? a.seed : nullptr);
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    const double *prm = a.params + (size_t)b * kAugParams;
    double R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = prm[i];
    const double s = prm[9], ratio = prm[13];
    t[0] = prm[10]; t[1] = prm[11]; t[2] = prm[12];
    const float *src = a.src + (long long)b * a.src_stride;
    float *dst = a.dst + (long long)b * a.dst_stride;
    for (int g = blockIdx.x * kAugThreads + threadIdx.x; g < groups; g += gridDim.x * kAugThreads) {
      const int n0 = g * V;
      // which point each of the V outputs is made of: its own, or point 0 when it is dropped
      bool dropped[V];
      bool any_dropped = false;
#pragma unroll
      for (int j = 0; j < V; ++j) dropped[j] = false;
      if (a.drop_on) {
        AugVec<V> u;
        if (a.keep) {
          u = aug_load<V>(a.keep + (size_t)b * N + n0);
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j) u.v[j] = unit_f32(draw_words(d, n0 + j, b, kDrawAugKeep).x);
        }
        if (a.keep_out) aug_store<V>(a.keep_out + (size_t)b * N + n0, u);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          dropped[j] = n0 + j > 0 && (double)u.v[j] <= ratio;
          any_dropped |= dropped[j];
        }
      }
      // the jitter of the point each output is made of: clip(sigma z, +-clip) in fp64
      double jit[3][V];
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int j = 0; j < V; ++j) jit[k][j] = 0.0;
      if (a.jitter_on) {
        AugVec<V> z[3];
        if (a.jitter) {
#pragma unroll
          for (int k = 0; k < 3; ++k) z[k] = aug_load<V>(a.jitter + ((size_t)b * 3 + k) * N + n0);
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const uint4 r4 = draw_words(d, n0 + j, b, kDrawAugJitter);
            const float2 za = normal2_f32(r4.x, r4.y), zb = normal2_f32(r4.z, r4.w);
            z[0].v[j] = za.x; z[1].v[j] = za.y; z[2].v[j] = zb.x;
          }
        }
        if (a.jitter_out) {
#pragma unroll
          for (int k = 0; k < 3; ++k) aug_store<V>(a.jitter_out + ((size_t)b * 3 + k) * N + n0, z[k]);
        }
        if (any_dropped) {                     // point 0's own draw is the one a dropped point carries
          float z0[3];
          if (a.jitter) {
#pragma unroll
            for (int k = 0; k < 3; ++k) z0[k] = a.jitter[((size_t)b * 3 + k) * N];
          } else {
            const uint4 r4 = draw_words(d, 0u, b, kDrawAugJitter);
            const float2 za = normal2_f32(r4.x, r4.y), zb = normal2_f32(r4.z, r4.w);
            z0[0] = za.x; z0[1] = za.y; z0[2] = zb.x;
          }
#pragma unroll
          for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int j = 0; j < V; ++j)
              if (dropped[j]) z[k].v[j] = z0[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
          for (int j = 0; j < V; ++j) jit[k][j] = aug_clip(a.jitter_sigma * (double)z[k].v[j], a.jitter_clip);
      }
      // the channel planes
      for (int c = 0; c < C;) {
        const int role = c == a.first0 ? a.role0 : (c == a.first1 ? a.role1 : (c == a.first2 ? a.role2 : (c == a.first3 ? a.role3 : 0)));
        if (role == 0) {
          aug_store<V>(dst + (size_t)c * N + n0, aug_load_plane<V>(src + (size_t)c * N, n0, any_dropped, dropped));
          c += 1;
          continue;
        }
        const AugVec<V> x0 = aug_load_plane<V>(src + (size_t)c * N, n0, any_dropped, dropped);
        const AugVec<V> x1 = aug_load_plane<V>(src + (size_t)(c + 1) * N, n0, any_dropped, dropped);
        const AugVec<V> x2 = aug_load_plane<V>(src + (size_t)(c + 2) * N, n0, any_dropped, dropped);
        const bool position = role == PVCNN_AUGMENT_POSITION;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          AugVec<V> y;
#pragma unroll
          for (int j = 0; j < V; ++j) {
            double v = (R[k * 3] * (double)x0.v[j] + R[k * 3 + 1] * (double)x1.v[j]) + R[k * 3 + 2] * (double)x2.v[j];
            if (position) {
              v = s * v + t[k];
              if (a.jitter_on) v = v + jit[k][j];
            }
            y.v[j] = (float)v;
          }
          aug_store<V>(dst + (size_t)(c + k) * N + n0, y);
        }
        c += 3;
      }
      if (a.targets_src) {
        const int64_t *ts = a.targets_src + (long long)b * a.targets_src_stride;
        int64_t *td = a.targets_dst + (long long)b * a.targets_dst_stride;
#pragma unroll
        for (int j = 0; j < V; ++j) td[n0 + j] = ts[dropped[j] ? 0 : n0 + j];
      }
    }
  }
}

// [p, p + count) and [q, q + count) of `size`-byte elements share a byte
static bool aug_overlap(const void *p, const void *q, long long count, size_t size) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q), len = (uintptr_t)count * size;
  return a < b + len && b < a + len;
}

}  // namespace pvcnn

using namespace pvcnn;

extern "C" int pvcnn_augment_draw(int B, int axis, double rot_max, double perturb_sigma, double perturb_clip, double flip_x,
                                  double flip_y, double flip_z, double scale_lo, double scale_hi, double translate_max,
                                  double drop_max, const int64_t *seed, double *params, void *stream) {
  PVCNN_REQUIRE(B >= 0, "negative batch size");
  PVCNN_REQUIRE(axis >= 0 && axis <= 2, "axis must be 0, 1 or 2");
  // (a NaN fails every one of these comparisons)
  PVCNN_REQUIRE(rot_max >= 0.0 && rot_max <= 1e6 && perturb_sigma >= 0.0 && perturb_sigma <= 1e6 && perturb_clip >= 0.0,
                "rot_max and perturb_sigma must lie in [0, 1e6], perturb_clip must not be negative");
  PVCNN_REQUIRE(flip_x >= 0.0 && flip_x <= 1.0 && flip_y >= 0.0 && flip_y <= 1.0 && flip_z >= 0.0 && flip_z <= 1.0,
                "flip probabilities must lie in [0, 1]");
  PVCNN_REQUIRE(scale_lo <= scale_hi && scale_lo >= -1e30 && scale_hi <= 1e30, "scale_lo <= scale_hi (finite) expected");
  PVCNN_REQUIRE(translate_max >= 0.0 && translate_max <= 1e30, "translate_max must be finite and not negative");
  PVCNN_REQUIRE(drop_max >= 0.0 && drop_max <= 1.0, "drop_max must lie in [0, 1]");
  if (B == 0) return 0;
  PVCNN_REQUIRE(seed && params, "null pointer (seed, params)");
  const AugmentConfig g{axis, rot_max, perturb_sigma, perturb_clip, flip_x, flip_y, flip_z, scale_lo, scale_hi, translate_max, drop_max};
  hipLaunchKernelGGL(augment_draw_kernel, dim3((B + kAugThreads - 1) / kAugThreads), dim3(kAugThreads), 0,
                     static_cast<hipStream_t>(stream), g, B, seed, params);
  return check_launch("augment_draw");
}

extern "C" int pvcnn_augment_apply(const float *src, long long src_batch_stride, const int64_t *targets_src,
                                   long long targets_src_batch_stride, int B, int C, int N, const int32_t *layout, int num_triples,
                                   const double *params, double jitter_sigma, double jitter_clip, int jitter_on, int drop_on,
                                   const float *jitter, const float *keep, const int64_t *seed, float *dst,
                                   long long dst_batch_stride, int64_t *targets_dst, long long targets_dst_batch_stride,
                                   float *jitter_out, float *keep_out, void *stream) {
  PVCNN_REQUIRE(B >= 0 && C >= 0 && N >= 0, "negative size");
  PVCNN_REQUIRE(num_triples >= 0 && num_triples <= PVCNN_AUGMENT_MAX_TRIPLES && (num_triples == 0 || layout),
                "a layout holds at most four triples");
  int first[PVCNN_AUGMENT_MAX_TRIPLES] = {-1, -1, -1, -1}, role[PVCNN_AUGMENT_MAX_TRIPLES] = {0, 0, 0, 0};
  for (int q = 0; q < num_triples; ++q) {
    role[q] = layout[2 * q];
    first[q] = layout[2 * q + 1];
    PVCNN_REQUIRE(role[q] == PVCNN_AUGMENT_POSITION || role[q] == PVCNN_AUGMENT_DIRECTION, "a triple's role must be POSITION or DIRECTION");
    PVCNN_REQUIRE(first[q] >= 0 && (long long)first[q] + 3 <= C, "a triple's planes exceed the C channels");
    for (int p = 0; p < q; ++p) PVCNN_REQUIRE(first[q] >= first[p] + 3 || first[q] + 3 <= first[p], "triples overlap");
  }
  PVCNN_REQUIRE(jitter_sigma >= 0.0 && jitter_clip >= 0.0, "jitter_sigma and jitter_clip must not be negative");
  PVCNN_REQUIRE((long long)C * N <= 0x7fffffffll, "a sample holds at most 2^31 - 1 floats");
  if (B == 0 || C == 0 || N == 0) return 0;
  const long long sample = (long long)C * N;
  PVCNN_REQUIRE(src && dst && params, "null pointer (src, dst, params)");
  PVCNN_REQUIRE(B == 1 || (src_batch_stride >= sample && dst_batch_stride >= sample), "a batch stride is shorter than a sample");
  PVCNN_REQUIRE((targets_src != nullptr) == (targets_dst != nullptr), "targets_src and targets_dst go together");
  PVCNN_REQUIRE(!targets_src || B == 1 || (targets_src_batch_stride >= N && targets_dst_batch_stride >= N),
                "a batch stride of the targets is shorter than a row");
  PVCNN_REQUIRE(!((jitter_on && !jitter) || (drop_on && !keep)) || seed,
                "a stage without its draws (`jitter`, `keep`: parity mode) needs a device `seed`");
  AugmentApply a{};
  a.src_stride = B > 1 ? src_batch_stride : 0; a.dst_stride = B > 1 ? dst_batch_stride : 0;
  a.targets_src_stride = B > 1 ? targets_src_batch_stride : 0; a.targets_dst_stride = B > 1 ? targets_dst_batch_stride : 0;
  // aliasing: elementwise (the same addresses, the same strides) without dropout; otherwise the extents must be disjoint
  const long long src_extent = (B - 1) * a.src_stride + sample, dst_extent = (B - 1) * a.dst_stride + sample;
  const bool same = static_cast<const float *>(dst) == src && a.src_stride == a.dst_stride;
  PVCNN_REQUIRE(!(drop_on && same), "with dropout on, dst must not alias src (a dropped point reads point 0 while another thread writes it)");
  PVCNN_REQUIRE(same || !aug_overlap(src, dst, src_extent > dst_extent ? src_extent : dst_extent, sizeof(float)),
                "dst overlaps src without being the same view");
  if (targets_src) {
    const long long ts_extent = (B - 1) * a.targets_src_stride + N, td_extent = (B - 1) * a.targets_dst_stride + N;
    const bool tsame = static_cast<const int64_t *>(targets_dst) == targets_src && a.targets_src_stride == a.targets_dst_stride;
    PVCNN_REQUIRE(!(drop_on && tsame), "with dropout on, targets_dst must not alias targets_src");
    PVCNN_REQUIRE(tsame || !aug_overlap(targets_src, targets_dst, ts_extent > td_extent ? ts_extent : td_extent, sizeof(int64_t)),
                  "targets_dst overlaps targets_src without being the same view");
  }
  a.src = src; a.dst = dst; a.targets_src = targets_src; a.targets_dst = targets_dst; a.params = params;
  a.jitter = jitter_on ? jitter : nullptr; a.keep = drop_on ? keep : nullptr; a.seed = seed;
  a.jitter_out = jitter_on ? jitter_out : nullptr; a.keep_out = drop_on ? keep_out : nullptr;
  a.B = B; a.C = C; a.N = N; a.jitter_on = jitter_on != 0; a.drop_on = drop_on != 0;
  a.jitter_sigma = jitter_sigma; a.jitter_clip = jitter_clip;
  a.first0 = first[0]; a.first1 = first[1]; a.first2 = first[2]; a.first3 = first[3];
  a.role0 = role[0]; a.role1 = role[1]; a.role2 = role[2]; a.role3 = role[3];
  const bool vec = (long long)B * N >= kAugVecMinPoints && N % 4 == 0 && aligned16(src) && aligned16(dst) && a.src_stride % 4 == 0 && a.dst_stride % 4 == 0 &&
                   aligned16(a.jitter) && aligned16(a.keep) && aligned16(a.jitter_out) && aligned16(a.keep_out);
  const int groups = vec ? N / 4 : N;
  int gx = (groups + kAugThreads - 1) / kAugThreads;
  if (gx > kAugMaxBlocksX) gx = kAugMaxBlocksX;
  const dim3 grid(gx, B < 65535 ? B : 65535), block(kAugThreads);
  if (vec) hipLaunchKernelGGL(augment_apply_kernel<4>, grid, block, 0, static_cast<hipStream_t>(stream), a);
  else hipLaunchKernelGGL(augment_apply_kernel<1>, grid, block, 0, static_cast<hipStream_t>(stream), a);
  return check_launch("augment_apply");
}
