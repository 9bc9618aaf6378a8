// xent.hip -- the segmentation criterion (torch.nn.functional.cross_entropy on (B, C, S) logits with int64 (B, S) targets, class
// weights, ignore_index, label smoothing, reduction mean / sum) as three launches: two for the loss, one for its gradient.
//
//   per point i:   m = max_c x_c,  s = sum_c expf(x_c - m),  logp_c = (x_c - m) - logf(s)
//                  nll_i    = w_t * ((m - x_t) + logf(s))                       (t = the point's target)
//                  smooth_i = -sum_c w_c logp_c = W logf(s) - sum_c w_c (x_c - m)     (W = sum_c w_c; label smoothing only:
//                             the points add up logf(s) and the weighted sum apart, W -- one fp64 sum -- is applied once, in the
//                             finalize, and is the W the gradient uses)
//   loss = [(1 - eps) sum_i nll_i + eps / C sum_i smooth_i] / den,    den = sum_i w_t  (mean; 1 for sum)
//   d loss / d x_j = g / den * [(1 - eps) w_t (p_j - [j == t]) + eps / C (W p_j - w_j)],   p_j = expf(x_j - m) / s
//
// As torch ops this is five to six launches that read or write the logits about eight times.  Here the logits are read twice for
// the loss (the second time from cache: C is a run-time value, a per-class register array would live in scratch) and once more for
// the gradient, which is written once.  Lanes run along the points, so a wave reads one class row of its 64 points as one request.
//
// A point whose target equals ignore_index contributes nothing.  A target outside [0, C) that is NOT ignore_index is treated the
// same way and counted (torch's device-side assert would be a GPU fault): it is never used as an index.
//
// Deterministic: no float atomics, no ticket fold.  A workgroup adds its lanes' fp64 sums by a fixed butterfly, the one-workgroup
// finalize adds the per-workgroup partials in a fixed order in fp64.  Every word of every output is written; nothing is memset.
#include "xent_sums.h"

namespace pvcnn {

constexpr size_t kXentStateBytes = 16;         // workspace: [den, W, -, -] floats | kXentSums x parts doubles | (m, s) per point
constexpr int kXentSums = 5;

// parts[k * gridDim.x + workgroup], k = 0: sum nll_i, 1: sum of logf(s_i), 2: sum w_t, 3: number of out-of-range targets,
// 4: sum_i sum_c w_c (x_c - m) -- 1 and 4 over the live points, with label smoothing only (else 0);
// save[i] = (m, s) of EVERY point i = b * S + position (ignored ones too: backward does not read them, but no word stays unwritten)
__global__ __launch_bounds__(kXentThreads) void xent_partials_kernel(const float *__restrict__ x, size_t x_bstride,
                                                                     const long long *__restrict__ target, size_t t_bstride,
                                                                     const float *__restrict__ weight, long long B, int C, long long S,
                                                                     long long ignore_index, int smoothing, double *__restrict__ parts,
                                                                     float2 *__restrict__ save) {
  const long long P = B * S, stride = (long long)gridDim.x * kXentThreads;
  double acc[kXentSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (long long i = (long long)blockIdx.x * kXentThreads + threadIdx.x; i < P; i += stride) {
    const long long b = i / S, pos = i - b * S;
    const float *__restrict__ xp = x + (size_t)b * x_bstride + (size_t)pos;
    float m = xp[0];
    for (int c = 1; c < C; ++c) m = fmaxf(m, xp[(size_t)c * (size_t)S]);
    float s = 0.0f, wx = 0.0f;
    if (smoothing) {
      for (int c = 0; c < C; ++c) {
        const float d = xp[(size_t)c * (size_t)S] - m, wc = weight ? weight[c] : 1.0f;
        s += expf(d);
        wx += wc * d;
      }
    } else {
      for (int c = 0; c < C; ++c) s += expf(xp[(size_t)c * (size_t)S] - m);
    }
    save[i] = make_float2(m, s);
    const long long t = target[(size_t)b * t_bstride + (size_t)pos];
    if (t != ignore_index) {
      if ((unsigned long long)t < (unsigned long long)C) {
        const float wt = weight ? weight[t] : 1.0f, ls = logf(s);
        acc[0] += (double)(wt * ((m - xp[(size_t)t * (size_t)S]) + ls));
        if (smoothing) { acc[1] += (double)ls; acc[4] += (double)wx; }
        acc[2] += (double)wt;
      } else {
        acc[3] += 1.0;
      }
    }
  }
  wg_sum(acc);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < kXentSums; ++k) parts[(size_t)k * gridDim.x + blockIdx.x] = acc[k];
  }
}

// One workgroup: thread t adds partials t, t + 256, ... in index order, the 256 sums meet by the fixed butterfly; everything fp64.
__global__ __launch_bounds__(kXentThreads) void xent_finalize_kernel(const double *__restrict__ parts, int nparts,
                                                                     const float *__restrict__ weight, int C, double eps, int mean,
                                                                     float *__restrict__ state, float *__restrict__ loss,
                                                                     long long *bad_targets) {
  double acc[kXentSums + 1] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};            // [kXentSums]: W
  for (int i = threadIdx.x; i < nparts; i += kXentThreads) {
#pragma unroll
    for (int k = 0; k < kXentSums; ++k) acc[k] += parts[(size_t)k * nparts + i];
  }
  if (weight)
    for (int c = threadIdx.x; c < C; c += kXentThreads) acc[kXentSums] += (double)weight[c];
  wg_sum(acc);
  if (threadIdx.x == 0) {
    const double W = weight ? acc[kXentSums] : (double)C, den = acc[2];
    const double num = (1.0 - eps) * acc[0] + eps / (double)C * (W * acc[1] - acc[4]);
    loss[0] = (float)(mean ? num / den : num);                 // every point ignored under mean: 0 / 0 = NaN, as torch
    state[0] = (float)den;
    state[1] = (float)W;
    state[2] = 0.0f;
    state[3] = 0.0f;
    if (bad_targets) bad_targets[0] += (long long)acc[3];
  }
}

// grid.x strides the points, grid.y the classes: grad[b][c][pos] for every element (ignored and out-of-range points: zeros)
__global__ __launch_bounds__(kXentThreads) void xent_bwd_kernel(const float *__restrict__ x, size_t x_bstride,
                                                                const long long *__restrict__ target, size_t t_bstride,
                                                                const float *__restrict__ weight, const float *__restrict__ grad_out,
                                                                long long B, int C, long long S, long long ignore_index, float eps,
                                                                int mean, const float *__restrict__ state,
                                                                const float2 *__restrict__ save, float *__restrict__ grad) {
  const long long P = B * S, stride = (long long)gridDim.x * kXentThreads;
  const float scale = mean ? grad_out[0] / state[0] : grad_out[0];
  const float k_nll = scale * (1.0f - eps), k_smooth = scale * (eps / (float)C), wsum = state[1];
  for (long long i = (long long)blockIdx.x * kXentThreads + threadIdx.x; i < P; i += stride) {
    const long long b = i / S, pos = i - b * S;
    const long long t = target[(size_t)b * t_bstride + (size_t)pos];
    const bool live = t != ignore_index && (unsigned long long)t < (unsigned long long)C;
    const float *__restrict__ xp = x + (size_t)b * x_bstride + (size_t)pos;
    float *__restrict__ gp = grad + (size_t)b * (size_t)C * (size_t)S + (size_t)pos;
    const float2 ms = save[i];
    const float a = live ? k_nll * (weight ? weight[t] : 1.0f) : 0.0f;
    for (int c = blockIdx.y; c < C; c += gridDim.y) {
      float g = 0.0f;
      if (live) {
        const float p = expf(xp[(size_t)c * (size_t)S] - ms.x) / ms.y;
        g = a * (p - (c == t ? 1.0f : 0.0f));
        if (eps != 0.0f) g += k_smooth * (wsum * p - (weight ? weight[c] : 1.0f));
      }
      gp[(size_t)c * (size_t)S] = g;
    }
  }
}

}  // namespace pvcnn

using namespace pvcnn;

extern "C" size_t pvcnn_xent_parts(long long B, long long S) {
  if (B <= 0 || S <= 0 || B > (1ll << 40) / S) return 0;
  return (size_t)xent_parts(B, S);
}

extern "C" size_t pvcnn_xent_workspace_bytes(long long B, long long S) {
  if (B <= 0 || S <= 0 || B > (1ll << 40) / S) return 0;
  return kXentStateBytes + kXentSums * sizeof(double) * (size_t)xent_parts(B, S) + sizeof(float2) * (size_t)(B * S);
}

extern "C" int pvcnn_xent_partials(const float *x, long long x_bstride, const long long *target, long long t_bstride, const float *weight,
                                   long long B, int C, long long S, long long ignore_index, int smoothing, void *workspace, void *stream) {
  // (values first, pointers second: a call with a bad value is refused whatever its pointers are)
  PVCNN_REQUIRE(xent_sizes_ok(B, C, S), "bad size");
  PVCNN_REQUIRE(x_bstride >= (long long)C * S && t_bstride >= S, "batch strides: logits >= C * S, targets >= S");
  PVCNN_REQUIRE(x && target && workspace, "null pointer");
  PVCNN_REQUIRE(aligned16(workspace), "the workspace must be 16-byte aligned");
  const long long nparts = xent_parts(B, S);
  double *parts = reinterpret_cast<double *>(static_cast<char *>(workspace) + kXentStateBytes);
  float2 *save = reinterpret_cast<float2 *>(parts + kXentSums * nparts);
  hipLaunchKernelGGL(xent_partials_kernel, dim3((unsigned)nparts), dim3(kXentThreads), 0, static_cast<hipStream_t>(stream), x,
                     (size_t)x_bstride, target, (size_t)t_bstride, weight, B, C, S, ignore_index, smoothing, parts, save);
  return check_launch("xent_partials");
}

extern "C" int pvcnn_xent_finalize(const float *weight, long long B, int C, long long S, double label_smoothing, int mean, void *workspace,
                                   float *loss, long long *bad_targets, void *stream) {
  PVCNN_REQUIRE(xent_sizes_ok(B, C, S), "bad size");
  PVCNN_REQUIRE(label_smoothing >= 0.0 && label_smoothing <= 1.0, "label_smoothing must be in [0, 1]");
  PVCNN_REQUIRE(workspace && loss, "null pointer");
  PVCNN_REQUIRE(aligned16(workspace), "the workspace must be 16-byte aligned");
  float *state = static_cast<float *>(workspace);
  const double *parts = reinterpret_cast<const double *>(static_cast<char *>(workspace) + kXentStateBytes);
  hipLaunchKernelGGL(xent_finalize_kernel, dim3(1), dim3(kXentThreads), 0, static_cast<hipStream_t>(stream), parts,
                     (int)xent_parts(B, S), weight, C, label_smoothing, mean, state, loss, bad_targets);
  return check_launch("xent_finalize");
}

extern "C" int pvcnn_xent_bwd(const float *x, long long x_bstride, const long long *target, long long t_bstride, const float *weight,
                              const float *grad_out, long long B, int C, long long S, long long ignore_index, float label_smoothing,
                              int mean, const void *workspace, float *grad_x, void *stream) {
  PVCNN_REQUIRE(xent_sizes_ok(B, C, S), "bad size");
  PVCNN_REQUIRE(x_bstride >= (long long)C * S && t_bstride >= S, "batch strides: logits >= C * S, targets >= S");
  PVCNN_REQUIRE(label_smoothing >= 0.0f && label_smoothing <= 1.0f, "label_smoothing must be in [0, 1]");
  PVCNN_REQUIRE(x && target && grad_out && workspace && grad_x, "null pointer");
  PVCNN_REQUIRE(aligned16(workspace), "the workspace must be 16-byte aligned");
  const float *state = static_cast<const float *>(workspace);
  const float2 *save = reinterpret_cast<const float2 *>(static_cast<const char *>(workspace) + kXentStateBytes +
                                                        kXentSums * sizeof(double) * (size_t)xent_parts(B, S));
  const long long blocks = (B * S + kXentThreads - 1) / kXentThreads;
  const dim3 grid((unsigned)(blocks < kXentBwdMaxBlocks ? blocks : kXentBwdMaxBlocks),
                  (unsigned)(C < kXentBwdMaxClassRows ? C : kXentBwdMaxClassRows));
  hipLaunchKernelGGL(xent_bwd_kernel, grid, dim3(kXentThreads), 0, static_cast<hipStream_t>(stream), x, (size_t)x_bstride, target,
                     (size_t)t_bstride, weight, grad_out, B, C, S, ignore_index, label_smoothing, mean, state, save, grad_x);
  return check_launch("xent_bwd");
}
