// evaluate.hip -- evaluation on the device: vote tiling, per-vote confidence, the vote merge, segmentation statistics and the
// per-step meters of train.py.
//
// Reference: evaluate/s3dis/eval.py:139-216 and evaluate/shapenet/eval.py:124-200 tile and shuffle the points on the host, run
// F.softmax(model(x), 1).max(1), copy both results back and merge the votes in a numba loop (update_scene_predictions /
// update_shape_predictions), then count with another (update_stats); meters/s3dis.py and meters/shapenet.py make one .item() per class
// and batch.  Here every one of those steps is a launch on the caller's stream; nothing is read back until the caller asks.
// Integer atomics only: every output is bitwise deterministic.  Histograms are privatised in LDS, one global add per non-zero bin per
// workgroup.
#include <algorithm>

#include "common.h"

namespace pvcnn {

constexpr int kEvalThreads = 256;
constexpr int kEvalMaxClasses = 4096;     // LDS histograms of 3 * C words (48 KiB at the cap)
constexpr int kEvalMaxParts = 64;         // part classes of one ShapeNet shape (the dataset has at most 6)

inline unsigned eval_grid(long long n) {
  return (unsigned)std::min<long long>((n + kEvalThreads - 1) / kEvalThreads, 8192);
}

// ---- repeat / shuffle / tile: out[b*E+e, c, j] = src[b*bstride + shuffled[b, e*np+j]*pstride + c*cstride] --------------------------
// grid.x = one output row (b*E+e, c), grid.y = 256-point slices of the row.  An index outside [0, src_points) reads nothing and writes
// a quiet NaN (the caller built the indices; a bad one must not become an out-of-bounds read).
__global__ __launch_bounds__(kEvalThreads) void eval_tile_kernel(const float *__restrict__ src, const long long *__restrict__ shuffled,
                                                                int E, int np, int C, int V, long long src_points, long long bstride,
                                                                long long pstride, long long cstride, float *__restrict__ out) {
  const int j = blockIdx.y * kEvalThreads + threadIdx.x;
  if (j >= np) return;
  const unsigned row = blockIdx.x;
  const int c = (int)(row % (unsigned)C);
  const unsigned be = row / (unsigned)C;
  const int b = (int)(be / (unsigned)E), e = (int)(be % (unsigned)E);
  const long long idx = shuffled[(long long)b * V + (long long)e * np + j];
  out[(long long)row * np + j] =
      (idx >= 0 && idx < src_points) ? src[(long long)b * bstride + idx * pstride + (long long)c * cstride] : __builtin_nanf("");
}

// ---- softmax over the classes + max over [lo, hi): F.softmax(x, 1)[:, lo:hi].max(1) --------------------------------------------------
// One thread per point (rows of N points are read coalesced).  m = max over all C; s = sum of expf(x_c - m) in class order;
// p_k = expf(x_k - m) / s (torch's epilogue); the first k of the largest p_k wins.
__global__ __launch_bounds__(kEvalThreads) void vote_confidence_kernel(const float *__restrict__ x, long long total, int C, int N, int c0,
                                                                      int c1, const int *__restrict__ ranges, float *__restrict__ conf,
                                                                      int *__restrict__ pred) {
  for (long long i = (long long)blockIdx.x * kEvalThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kEvalThreads) {
    const long long b = i / N;
    const int n = (int)(i - b * N);
    const float *row = x + b * C * (long long)N + n;
    int lo = c0, hi = c1;
    if (ranges != nullptr) {
      lo = max(ranges[2 * b], 0);
      hi = min(ranges[2 * b + 1], C);
    }
    if (lo >= hi) {                       // empty class range (a bad table row): no vote
      conf[i] = 0.0f;
      pred[i] = -1;
      continue;
    }
    float m = row[0];
    for (int c = 1; c < C; ++c) {
      const float v = row[(long long)c * N];
      m = v > m ? v : m;
    }
    float s = 0.0f;
    for (int c = 0; c < C; ++c) s += expf(row[(long long)c * N] - m);
    float best = expf(row[(long long)lo * N] - m) / s;
    int k = lo;
    for (int c = lo + 1; c < hi; ++c) {
      const float p = expf(row[(long long)c * N] - m) / s;
      if (p > best) {
        best = p;
        k = c;
      }
    }
    conf[i] = best;
    pred[i] = k;
  }
}

// ---- the sequential merge "if conf > state[t]: state[t] = conf; pred_state[t] = pred", in (b, p) order ------------------------------
// key = conf bits << 32 | (0xFFFFFFFF - g), g = b*V + p: the largest key is the largest confidence, and among equal ones the first
// vote.  A positive float's bits order like the float.  Votes with conf <= 0 or NaN are dropped: they never beat the state, which
// starts at 0 and only grows.
__device__ __forceinline__ bool vote_target(long long g, int V, const long long *__restrict__ shuffled,
                                            const long long *__restrict__ mapping, long long map_stride, long long P, long long &t) {
  const long long idx = shuffled[g];
  if (mapping != nullptr) {
    if (idx < 0 || idx >= map_stride) return false;
    t = mapping[(g / V) * map_stride + idx];
  } else {
    t = idx;
  }
  return t >= 0 && t < P;
}

__global__ __launch_bounds__(kEvalThreads) void vote_merge_keys_kernel(const float *__restrict__ conf, const long long *__restrict__ shuffled,
                                                                      const long long *__restrict__ mapping, long long map_stride, int V,
                                                                      long long total, long long P, unsigned long long *keys) {
  for (long long g = (long long)blockIdx.x * kEvalThreads + threadIdx.x; g < total; g += (long long)gridDim.x * kEvalThreads) {
    const float c = conf[g];
    long long t;
    if (!(c > 0.0f) || !vote_target(g, V, shuffled, mapping, map_stride, P, t)) continue;
    const unsigned long long key = ((unsigned long long)__float_as_uint(c) << 32) | (0xFFFFFFFFull - (unsigned long long)g);
    atomicMax(keys + t, key);
  }
}

// The vote whose key is the point's maximum (exactly one per point that received a valid vote) compares it with the state, writes,
// and zeroes the key for the next call.  The other votes of the point read either that key or 0: neither is theirs.
__global__ __launch_bounds__(kEvalThreads) void vote_merge_apply_kernel(const float *__restrict__ conf, const int *__restrict__ pred,
                                                                       const long long *__restrict__ shuffled,
                                                                       const long long *__restrict__ mapping, long long map_stride, int V,
                                                                       long long total, long long P, unsigned long long *keys,
                                                                       float *scene_conf, long long *scene_pred) {
  for (long long g = (long long)blockIdx.x * kEvalThreads + threadIdx.x; g < total; g += (long long)gridDim.x * kEvalThreads) {
    const float c = conf[g];
    long long t;
    if (!(c > 0.0f) || !vote_target(g, V, shuffled, mapping, map_stride, P, t)) continue;
    const unsigned long long key = ((unsigned long long)__float_as_uint(c) << 32) | (0xFFFFFFFFull - (unsigned long long)g);
    if (keys[t] != key) continue;
    if (c > scene_conf[t]) {
      scene_conf[t] = c;
      scene_pred[t] = pred[g];
    }
    keys[t] = 0ull;
  }
}

// ---- class histograms ----------------------------------------------------------------------------------------------------------------
// wrap != 0: numpy indexing -- a value in [-C, 0) counts for class value + C (the reference's stats[1, -1] for an unvoted point);
// otherwise, and for anything else outside [0, C), the value is counted nowhere.
__device__ __forceinline__ int class_slot(long long v, int C, int wrap) {
  if (wrap && v < 0 && v >= -C) v += C;
  return (v >= 0 && v < C) ? (int)v : -1;
}

__device__ __forceinline__ void flush_hist(const unsigned *h, int n, unsigned long long *dst) {
  for (int i = threadIdx.x; i < n; i += kEvalThreads)
    if (h[i] != 0u) atomicAdd(dst + i, (unsigned long long)h[i]);
}

// counts (3, C) += [seen; positive; correct] of (gt, pred) over P points (evaluate/s3dis/eval.py:205-213)
__global__ __launch_bounds__(kEvalThreads) void seg_counts_kernel(const long long *__restrict__ gt, const long long *__restrict__ pd,
                                                                 long long P, int C, int wrap, unsigned long long *counts) {
  extern __shared__ unsigned eval_hist[];
  for (int i = threadIdx.x; i < 3 * C; i += kEvalThreads) eval_hist[i] = 0u;
  __syncthreads();
  for (long long p = (long long)blockIdx.x * kEvalThreads + threadIdx.x; p < P; p += (long long)gridDim.x * kEvalThreads) {
    const long long g = gt[p], q = pd[p];
    const int gi = class_slot(g, C, wrap), qi = class_slot(q, C, wrap);
    if (gi >= 0) atomicAdd(eval_hist + gi, 1u);
    if (qi >= 0) atomicAdd(eval_hist + C + qi, 1u);
    if (g == q && gi >= 0) atomicAdd(eval_hist + 2 * C + gi, 1u);
  }
  __syncthreads();
  flush_hist(eval_hist, 3 * C, counts);
}

// first maximum of row[c * N] over [lo, hi) (torch.argmax: a NaN wins against numbers)
__device__ __forceinline__ int first_argmax(const float *row, int N, int lo, int hi) {
  float best = row[(long long)lo * N];
  int k = lo;
  for (int c = lo + 1; c < hi; ++c) {
    const float v = row[(long long)c * N];
    if (v > best || (v != v && best == best)) {
      best = v;
      k = c;
    }
  }
  return k;
}

// MeterS3DIS.update: counts [seen C | positive C | correct C | numel | correct] += this batch
__global__ __launch_bounds__(kEvalThreads) void seg_meter_s3dis_kernel(const float *__restrict__ x, const long long *__restrict__ targets,
                                                                      long long total, int C, int N, unsigned long long *counts) {
  extern __shared__ unsigned eval_hist[];
  for (int i = threadIdx.x; i < 3 * C + 1; i += kEvalThreads) eval_hist[i] = 0u;
  __syncthreads();
  for (long long i = (long long)blockIdx.x * kEvalThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kEvalThreads) {
    const long long b = i / N;
    const int n = (int)(i - b * N);
    const int k = first_argmax(x + b * C * (long long)N + n, N, 0, C);
    const long long t = targets[i];
    atomicAdd(eval_hist + C + k, 1u);
    if (t >= 0 && t < C) {
      atomicAdd(eval_hist + t, 1u);
      if (t == k) {
        atomicAdd(eval_hist + 2 * C + t, 1u);
        atomicAdd(eval_hist + 3 * C, 1u);
      }
    }
  }
  __syncthreads();
  flush_hist(eval_hist, 3 * C, counts);
  if (threadIdx.x == 0) {
    if (eval_hist[3 * C] != 0u) atomicAdd(counts + 3 * C + 1, (unsigned long long)eval_hist[3 * C]);
    if (blockIdx.x == 0) atomicAdd(counts + 3 * C, (unsigned long long)total);
  }
}

// MeterShapeNet.update: one workgroup per cloud.  Row r = *cursor + b of rows (capacity, max_parts + 1, 2) int32 gets (s, e) and then
// (intersection, union) of every part class s .. e-1 (zeros after); a row at or beyond the capacity is not written.
__global__ __launch_bounds__(kEvalThreads) void seg_meter_shapenet_kernel(const float *__restrict__ x, const long long *__restrict__ targets,
                                                                         int C, int N, const int *__restrict__ ranges, int nranges,
                                                                         int max_parts, int *rows, const long long *__restrict__ cursor,
                                                                         long long capacity) {
  __shared__ unsigned h[2 * kEvalMaxParts];
  const int b = blockIdx.x;
  const long long *tg = targets + (long long)b * N;
  const long long label = tg[0];
  int s = 0, e = 0;
  if (label >= 0 && label < nranges) {
    s = ranges[2 * label];
    e = ranges[2 * label + 1];
    if (s < 0 || e > C || s >= e || e - s > max_parts) s = e = 0;   // a bad table row: (0, 0), which the host refuses
  }
  for (int i = threadIdx.x; i < 2 * kEvalMaxParts; i += kEvalThreads) h[i] = 0u;
  __syncthreads();
  if (s < e) {
    const float *xb = x + (long long)b * C * N;
    for (int n = threadIdx.x; n < N; n += kEvalThreads) {
      const int k = first_argmax(xb + n, N, s, e);
      const long long t = tg[n];
      if (t == k) {
        atomicAdd(h + 2 * (k - s), 1u);
        atomicAdd(h + 2 * (k - s) + 1, 1u);
      } else {
        atomicAdd(h + 2 * (k - s) + 1, 1u);
        if (t >= s && t < e) atomicAdd(h + 2 * (t - s) + 1, 1u);
      }
    }
  }
  __syncthreads();
  const long long r = (cursor != nullptr ? *cursor : 0) + b;
  if (r < 0 || r >= capacity) return;
  int *out = rows + r * (long long)(max_parts + 1) * 2;
  for (int i = threadIdx.x; i < 2 * (max_parts + 1); i += kEvalThreads)
    out[i] = i == 0 ? s : i == 1 ? e : (int)h[i - 2];
}

}  // namespace pvcnn

using namespace pvcnn;

extern "C" int pvcnn_eval_tile(const float *src, long long batch_stride, long long point_stride, long long chan_stride, long long src_points,
                               const long long *shuffled, int B, int V, int num_points, int C, float *out, void *stream) {
  PVCNN_REQUIRE(B >= 0 && V >= 0 && C > 0 && num_points > 0, "bad sizes");
  PVCNN_REQUIRE(V % num_points == 0, "V must be a multiple of num_points");
  PVCNN_REQUIRE(num_points <= 65535 * kEvalThreads, "num_points too large");
  const long long rows = (long long)B * (V / num_points) * C;
  PVCNN_REQUIRE(rows < (1ll << 31), "B * E * C must be < 2^31");
  if (rows == 0) return 0;
  PVCNN_REQUIRE(src && shuffled && out, "null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(eval_tile_kernel, dim3((unsigned)rows, (unsigned)ceil_div(num_points, kEvalThreads)), dim3(kEvalThreads), 0, s,
                     src, shuffled, V / num_points, num_points, C, V, src_points, batch_stride, point_stride, chan_stride, out);
  return check_launch("eval_tile");
}

extern "C" int pvcnn_vote_confidence(const float *logits, int B, int C, int N, int c0, int c1, const int *ranges, float *conf, int *pred,
                                     void *stream) {
  PVCNN_REQUIRE(B >= 0 && C > 0 && N >= 0, "bad sizes");
  PVCNN_REQUIRE(ranges != nullptr || (0 <= c0 && c0 < c1 && c1 <= C), "class range must satisfy 0 <= c0 < c1 <= C");
  const long long total = (long long)B * N;
  if (total == 0) return 0;
  PVCNN_REQUIRE(logits && conf && pred, "null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(vote_confidence_kernel, dim3(eval_grid(total)), dim3(kEvalThreads), 0, s, logits, total, C, N, c0, c1, ranges, conf,
                     pred);
  return check_launch("vote_confidence");
}

extern "C" size_t pvcnn_vote_merge_workspace_bytes(long long P) { return P > 0 ? (size_t)P * sizeof(unsigned long long) : 0; }

extern "C" int pvcnn_vote_merge(const float *conf, const int *pred, const long long *shuffled, const long long *mapping, long long map_stride,
                                int B, int V, long long P, float *scene_conf, long long *scene_pred, void *workspace, size_t workspace_bytes,
                                void *stream) {
  PVCNN_REQUIRE(B >= 0 && V >= 0 && P >= 0, "bad sizes");
  PVCNN_REQUIRE((long long)B * V < (1ll << 32), "B * V must be < 2^32 (the vote order is packed into 32 bits)");
  PVCNN_REQUIRE(P < (1ll << 31), "P must be < 2^31");
  PVCNN_REQUIRE(mapping == nullptr || map_stride > 0, "map_stride must be > 0 with a mapping");
  const long long total = (long long)B * V;
  if (total == 0 || P == 0) return 0;
  PVCNN_REQUIRE(conf && pred && shuffled && scene_conf && scene_pred && workspace, "null pointer");
  PVCNN_REQUIRE(workspace_bytes >= pvcnn_vote_merge_workspace_bytes(P), "workspace too small");
  PVCNN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "workspace must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned long long *keys = static_cast<unsigned long long *>(workspace);
  hipLaunchKernelGGL(vote_merge_keys_kernel, dim3(eval_grid(total)), dim3(kEvalThreads), 0, s, conf, shuffled, mapping, map_stride, V, total,
                     P, keys);
  if (int rc = check_launch("vote_merge_keys")) return rc;
  hipLaunchKernelGGL(vote_merge_apply_kernel, dim3(eval_grid(total)), dim3(kEvalThreads), 0, s, conf, pred, shuffled, mapping, map_stride,
                     V, total, P, keys, scene_conf, scene_pred);
  return check_launch("vote_merge_apply");
}

extern "C" int pvcnn_seg_counts(const long long *gt, const long long *pred, long long P, int C, int wrap_negative, long long *counts,
                                void *stream) {
  PVCNN_REQUIRE(P >= 0 && P < (1ll << 31), "P must be in [0, 2^31)");
  PVCNN_REQUIRE(C > 0 && C <= kEvalMaxClasses, "C must be in [1, 4096]");
  if (P == 0) return 0;
  PVCNN_REQUIRE(gt && pred && counts, "null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(seg_counts_kernel, dim3(std::min(eval_grid(P), 1024u)), dim3(kEvalThreads), 3 * C * sizeof(unsigned), s, gt, pred, P,
                     C, wrap_negative, reinterpret_cast<unsigned long long *>(counts));
  return check_launch("seg_counts");
}

extern "C" int pvcnn_seg_meter_update(const float *logits, const long long *targets, int B, int C, int N, const int *part_ranges,
                                      int num_part_classes, int max_parts, long long *counts, int *rows, const long long *row_cursor,
                                      long long row_capacity, void *stream) {
  PVCNN_REQUIRE(B >= 0 && N >= 0 && C > 0 && C <= kEvalMaxClasses, "bad sizes (C must be in [1, 4096])");
  const long long total = (long long)B * N;
  PVCNN_REQUIRE(total < (1ll << 31), "B * N must be < 2^31");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (part_ranges == nullptr) {
    if (total == 0) return 0;
    PVCNN_REQUIRE(logits && targets && counts, "null pointer");
    hipLaunchKernelGGL(seg_meter_s3dis_kernel, dim3(std::min(eval_grid(total), 1024u)), dim3(kEvalThreads), (3 * C + 1) * sizeof(unsigned),
                       s, logits, targets, total, C, N, reinterpret_cast<unsigned long long *>(counts));
    return check_launch("seg_meter_s3dis");
  }
  PVCNN_REQUIRE(max_parts > 0 && max_parts <= kEvalMaxParts, "max_parts must be in [1, 64]");
  PVCNN_REQUIRE(num_part_classes > 0 && row_capacity >= 0, "bad part table / row capacity");
  if (B == 0) return 0;
  PVCNN_REQUIRE(N > 0, "clouds need at least one point");
  PVCNN_REQUIRE(logits && targets && rows, "null pointer");
  hipLaunchKernelGGL(seg_meter_shapenet_kernel, dim3((unsigned)B), dim3(kEvalThreads), 0, s, logits, targets, C, N, part_ranges,
                     num_part_classes, max_parts, rows, row_cursor, row_capacity);
  return check_launch("seg_meter_shapenet");
}
