// optim.hip -- the optimizer update of the data-parallel step on FLAT buffers.
//
// Reference: train.py:96-119 steps torch.optim.Adam over ~100 separate parameter tensors; torch's fused multi-tensor Adam needs
// 2 launches of 72 us for PVCNN's 9.8 MiB of parameters (70 MB of traffic that streams in ~15 us): the per-tensor chunking, not the
// arithmetic, is the cost.  pvcnn_amd/dp.py already keeps the gradients in a few flat buckets (what RCCL all-reduces); with the
// parameters laid out the same way (GradBucketReducer.flatten_parameters) the update is ONE elementwise pass per bucket.
// Arithmetic = torch.optim.Adam, fp32, step counter on the device (graph-capturable: nothing is read back by the host):
//     g   = coef * grad                             (coef: the clip coefficient of the status block; 1 without one)
//     g   = g + wd * p                              (L2)          or      p = p * (1 - lr * wd)      (decoupled: torch's AdamW order)
//     m   = m + (g - m) * (1 - b1)                  (torch: exp_avg.lerp_)
//     v   = b2 * v + (1 - b2) * g * g
//     vmax = max(vmax, v)                           (amsgrad only; then vmax replaces v below)
//     p  -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps),        t = *step + 1
// The hyper-parameters (lr, beta1, beta2, eps, weight_decay) are read from DEVICE memory too: a learning-rate schedule changes five
// floats there, and a hipGraph that captured this launch follows it (a scalar kernel argument would be frozen at capture time).
//
// Three launches share that arithmetic (adam_upd):
//   * adam_flat_kernel: one set of hyper-parameters for the whole buffer (pvcnn_adam_step);
//   * adam_grouped_kernel: parameter GROUPS (pvcnn_adam_step_grouped).  A bucket holds its parameters back to back and unpadded, so
//     a group boundary falls on any element, inside a float4 too.  The caller describes the bucket by a RUN TABLE in device memory --
//     (end offset, group id) pairs, ends strictly increasing, the last one = n -- and a (G, 5) hyper block.  Every workgroup copies
//     the table into LDS, derives each group's coefficients once, and each lane finds the run of its float4 by a binary search
//     there (PVCNN's buckets have 21 and 15 runs: 5 LDS reads next to 7 or 9 16-byte memory transactions).  A float4 inside one run --
//     all but (runs - 1) of them -- is updated with one set of coefficients; one that straddles a boundary, and the scalar tail,
//     take each element's own.  Loads and stores stay 16 bytes wide either way.  With every group holding the same
//     hyper-parameters the result is bit-identical to adam_flat_kernel's (same expressions, -ffp-contract=off).
//   * the gradient norm (pvcnn_grad_sqsum + pvcnn_grad_norm_finalize): sum of squares per buffer on a FIXED grid into caller-owned
//     per-workgroup partials (fp32 per lane, fp64 from the lane totals up), then one workgroup adds all partials in a fixed order
//     and writes the status block: norm, clip coefficient min(1, max_norm / (norm + 1e-6)) (torch's clip_grad_norm_), a skip flag
//     (sum not finite and skipping enabled) and the running count of skipped steps.  No float atomics: bit-reproducible.  The
//     update kernels multiply the gradient by the coefficient in registers (the gradient buffers are not rewritten) and, with the
//     skip flag set, write nothing and leave the step counter alone.
#include <algorithm>

#include "wave.h"

namespace pvcnn {

// what one update needs of a set of hyper-parameters at step t (= updates done so far + 1)
struct AdamCoef {
  float lr, b1, b2, eps, wd, step_size, bc2_sqrt;
};

__device__ __forceinline__ AdamCoef adam_coef(const float *__restrict__ hyper, float t) {
  AdamCoef c;
  c.lr = hyper[0]; c.b1 = hyper[1]; c.b2 = hyper[2]; c.eps = hyper[3]; c.wd = hyper[4];
  const float bc1 = 1.0f - powf(c.b1, t);
  c.bc2_sqrt = sqrtf(1.0f - powf(c.b2, t));
  c.step_size = c.lr / bc1;
  return c;
}

// one element; gg is the (already clipped) gradient, vx the amsgrad maximum (untouched without AMSGRAD)
template <bool DECOUPLED, bool AMSGRAD>
__device__ __forceinline__ void adam_upd(const AdamCoef &c, float &pp, float gg, float &mm, float &vv, float &vx) {
  if (DECOUPLED) pp = pp * (1.0f - c.lr * c.wd);
  else gg = gg + c.wd * pp;
  mm = mm + (gg - mm) * (1.0f - c.b1);
  vv = c.b2 * vv + (1.0f - c.b2) * gg * gg;
  float second = vv;
  if (AMSGRAD) {
    vx = fmaxf(vx, vv);
    second = vx;
  }
  const float denom = sqrtf(second) / c.bc2_sqrt + c.eps;
  pp = pp - c.step_size * (mm / denom);
}

__global__ __launch_bounds__(256) void adam_flat_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                                                        float *__restrict__ v, size_t n, const float *__restrict__ step,
                                                        const float *__restrict__ hyper) {
  const AdamCoef c = adam_coef(hyper, *step + 1.0f);
  const size_t n4 = n >> 2, stride = (size_t)gridDim.x * 256;
  float unused = 0.0f;
  auto upd = [&](float &pp, float gg, float &mm, float &vv) { adam_upd<false, false>(c, pp, gg, mm, vv, unused); };
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    float4 pv = reinterpret_cast<float4 *>(p)[i], mv = reinterpret_cast<float4 *>(m)[i], vv = reinterpret_cast<float4 *>(v)[i];
    const float4 gv = reinterpret_cast<const float4 *>(g)[i];
    upd(pv.x, gv.x, mv.x, vv.x); upd(pv.y, gv.y, mv.y, vv.y); upd(pv.z, gv.z, mv.z, vv.z); upd(pv.w, gv.w, mv.w, vv.w);
    reinterpret_cast<float4 *>(p)[i] = pv; reinterpret_cast<float4 *>(m)[i] = mv; reinterpret_cast<float4 *>(v)[i] = vv;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const size_t i = (n4 << 2) + threadIdx.x;
    upd(p[i], g[i], m[i], v[i]);
  }
}

__global__ void adam_step_inc_kernel(float *step) { *step += 1.0f; }

// ---- the status block of the gradient norm (include/pvcnn_hip.h): what the finalize writes and the update kernels read ----
enum { kStNorm = 0, kStCoef = 1, kStSkip = 2, kStSkipped = 3, kStMaxNorm = 4, kStSkipEnabled = 5 };

__global__ void adam_step_inc_guarded_kernel(float *step, const float *__restrict__ status) {
  if (status == nullptr || status[kStSkip] == 0.0f) *step += 1.0f;
}

// LDS: nruns run ends | nruns group ids | ngroups AdamCoef.  A lane's element index e lies in the first run whose end is > e.
template <bool DECOUPLED, bool AMSGRAD>
__global__ __launch_bounds__(256) void adam_grouped_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                                                           float *__restrict__ v, float *__restrict__ vmax, size_t n,
                                                           const float *__restrict__ step, const float *__restrict__ hyper,
                                                           int ngroups, const int *__restrict__ runs, int nruns,
                                                           const float *__restrict__ status) {
  extern __shared__ int s_table[];
  if (status != nullptr && status[kStSkip] != 0.0f) return;          // (uniform: the whole launch writes nothing)
  uint32_t *s_end = reinterpret_cast<uint32_t *>(s_table);
  int *s_gid = s_table + nruns;
  AdamCoef *s_coef = reinterpret_cast<AdamCoef *>(s_table + 2 * nruns);
  const float t = *step + 1.0f;
  for (int r = threadIdx.x; r < nruns; r += 256) {
    s_end[r] = (uint32_t)runs[2 * r];
    s_gid[r] = min(max(runs[2 * r + 1], 0), ngroups - 1);            // (a bad id reads a neighbour's coefficients, never outside LDS)
  }
  for (int k = threadIdx.x; k < ngroups; k += 256) s_coef[k] = adam_coef(hyper + 5 * (size_t)k, t);
  __syncthreads();
  const float clip = status != nullptr ? status[kStCoef] : 1.0f;
  const int last = nruns - 1;
  auto find = [&](uint32_t e) {
    int lo = 0, hi = last;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_end[mid] > e) hi = mid; else lo = mid + 1;
    }
    return lo;
  };
  // one element with the coefficients of ITS run: r follows e upwards
  auto one = [&](int &r, uint32_t e, float &pp, float gg, float &mm, float &vv, float &vx) {
    while (r < last && s_end[r] <= e) ++r;
    const AdamCoef c = s_coef[s_gid[r]];
    adam_upd<DECOUPLED, AMSGRAD>(c, pp, clip * gg, mm, vv, vx);
  };
  const size_t n4 = n >> 2, stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    const uint32_t e = (uint32_t)(i << 2);
    int r = find(e);
    float4 pv = reinterpret_cast<float4 *>(p)[i], mv = reinterpret_cast<float4 *>(m)[i], vv = reinterpret_cast<float4 *>(v)[i];
    const float4 gv = reinterpret_cast<const float4 *>(g)[i];
    float4 xv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (AMSGRAD) xv = reinterpret_cast<float4 *>(vmax)[i];
    if (r == last || s_end[r] >= e + 4) {                            // the whole float4 in one run
      const AdamCoef c = s_coef[s_gid[r]];
      adam_upd<DECOUPLED, AMSGRAD>(c, pv.x, clip * gv.x, mv.x, vv.x, xv.x);
      adam_upd<DECOUPLED, AMSGRAD>(c, pv.y, clip * gv.y, mv.y, vv.y, xv.y);
      adam_upd<DECOUPLED, AMSGRAD>(c, pv.z, clip * gv.z, mv.z, vv.z, xv.z);
      adam_upd<DECOUPLED, AMSGRAD>(c, pv.w, clip * gv.w, mv.w, vv.w, xv.w);
    } else {                                                         // a group boundary inside it: element by element
      one(r, e, pv.x, gv.x, mv.x, vv.x, xv.x);
      one(r, e + 1, pv.y, gv.y, mv.y, vv.y, xv.y);
      one(r, e + 2, pv.z, gv.z, mv.z, vv.z, xv.z);
      one(r, e + 3, pv.w, gv.w, mv.w, vv.w, xv.w);
    }
    reinterpret_cast<float4 *>(p)[i] = pv; reinterpret_cast<float4 *>(m)[i] = mv; reinterpret_cast<float4 *>(v)[i] = vv;
    if (AMSGRAD) reinterpret_cast<float4 *>(vmax)[i] = xv;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const size_t i = (n4 << 2) + threadIdx.x;
    int r = find((uint32_t)i);
    float unused = 0.0f;
    one(r, (uint32_t)i, p[i], g[i], m[i], v[i], AMSGRAD ? vmax[i] : unused);
  }
}

// partials[blockIdx.x] = the sum of g[i]^2 over this workgroup's share (float4 index = workgroup * 256 + lane, stride grid * 256;
// the n & 3 tail elements go to lanes 0..2 of workgroup 0).  Every lane adds its squares in index order in four fp32 sums.
__global__ __launch_bounds__(256) void grad_sqsum_kernel(const float *__restrict__ g, size_t n, float *__restrict__ partials) {
  const size_t n4 = n >> 2, stride = (size_t)gridDim.x * 256;
  float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    const float4 gv = reinterpret_cast<const float4 *>(g)[i];
    a0 += gv.x * gv.x; a1 += gv.y * gv.y; a2 += gv.z * gv.z; a3 += gv.w * gv.w;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const float t = g[(n4 << 2) + threadIdx.x];
    a0 += t * t;
  }
  const double total = wg_sum(((double)a0 + (double)a1) + ((double)a2 + (double)a3));
  if (threadIdx.x == 0) partials[blockIdx.x] = (float)total;
}

__global__ __launch_bounds__(256) void grad_norm_finalize_kernel(const float *__restrict__ partials, int nparts, float *status) {
  double s = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) s += (double)partials[i];
  const double total = wg_sum(s);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(total);
    const bool skip = !isfinite(total) && status[kStSkipEnabled] != 0.0f;
    status[kStNorm] = norm;
    status[kStCoef] = fminf(1.0f, status[kStMaxNorm] / (norm + 1e-6f));
    status[kStSkip] = skip ? 1.0f : 0.0f;
    if (skip) status[kStSkipped] += 1.0f;
  }
}

}  // namespace pvcnn

using namespace pvcnn;

// One Adam update of n contiguous fp32 parameters (p, m = exp_avg, v = exp_avg_sq updated in place; g read).  `step` = one float in
// device memory, the number of updates done so far; inc_step != 0 increments it behind the update (pass it with the LAST buffer of an
// optimizer step when the parameters live in several buffers).  hyper: five floats in device memory (lr, beta1, beta2, eps, weight_decay).
extern "C" int pvcnn_adam_step(float *p, const float *g, float *m, float *v, size_t n, float *step, const float *hyper, int inc_step,
                               void *stream) {
  PVCNN_REQUIRE(step && hyper, "null step counter / hyper-parameter block");
  PVCNN_REQUIRE(n == 0 || (p && g && m && v), "null pointer");
  PVCNN_REQUIRE(n == 0 || (aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v)), "buffers must be 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n > 0) {
    const unsigned grid = (unsigned)std::min<size_t>(2048, (n / 4 + 255) / 256 + 1);
    hipLaunchKernelGGL(adam_flat_kernel, dim3(grid), dim3(256), 0, s, p, g, m, v, n, step, hyper);
    if (int rc = check_launch("adam_flat")) return rc;
  }
  if (inc_step) {
    hipLaunchKernelGGL(adam_step_inc_kernel, dim3(1), dim3(1), 0, s, step);
    return check_launch("adam_step_inc");
  }
  return 0;
}

// The same update with parameter groups, the AdamW / amsgrad variants and the clip coefficient / skip flag of a status block
// (include/pvcnn_hip.h has the contract).  One launch for the buffer, whatever the number of groups.
extern "C" int pvcnn_adam_step_grouped(float *p, const float *g, float *m, float *v, float *vmax, size_t n, float *step,
                                       const float *hyper, int ngroups, const int *runs, int nruns, const float *status,
                                       int decoupled, int inc_step, void *stream) {
  PVCNN_REQUIRE(step && hyper, "null step counter / hyper-parameter block");
  PVCNN_REQUIRE(ngroups >= 1 && ngroups <= 256, "1 <= ngroups <= 256");
  PVCNN_REQUIRE(n == 0 || (p && g && m && v), "null pointer");
  PVCNN_REQUIRE(n == 0 || (runs && nruns >= 1 && nruns <= 4096), "a run table of 1 ... 4096 runs");
  PVCNN_REQUIRE(n <= (size_t)0x7fffffff, "run ends are int32: n < 2^31");
  PVCNN_REQUIRE(n == 0 || (aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && aligned16(vmax)),
                "buffers must be 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n > 0) {
    const unsigned grid = (unsigned)std::min<size_t>(2048, (n / 4 + 255) / 256 + 1);
    const size_t lds = (size_t)nruns * 2 * sizeof(int) + (size_t)ngroups * sizeof(AdamCoef);
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds, s, p, g, m, v, vmax, n, step, hyper, ngroups, runs, nruns, status);
    };
    if (vmax != nullptr) {
      if (decoupled) launch(adam_grouped_kernel<true, true>); else launch(adam_grouped_kernel<false, true>);
    } else {
      if (decoupled) launch(adam_grouped_kernel<true, false>); else launch(adam_grouped_kernel<false, false>);
    }
    if (int rc = check_launch("adam_grouped")) return rc;
  }
  if (inc_step) {
    hipLaunchKernelGGL(adam_step_inc_guarded_kernel, dim3(1), dim3(1), 0, s, step, status);
    return check_launch("adam_step_inc_guarded");
  }
  return 0;
}

// partials[0 .. nparts) = per-workgroup sums of g[i]^2 over n elements (nparts workgroups: the caller fixes the grid, and with it the
// order of every addition).  n == 0 writes zeros.
extern "C" int pvcnn_grad_sqsum(const float *g, size_t n, float *partials, int nparts, void *stream) {
  PVCNN_REQUIRE(partials && nparts >= 1 && nparts <= 65535, "partials: 1 ... 65535 floats");
  PVCNN_REQUIRE(n == 0 || g, "null pointer");
  PVCNN_REQUIRE(n == 0 || aligned16(g), "the gradient buffer must be 16-byte aligned");
  hipLaunchKernelGGL(grad_sqsum_kernel, dim3((unsigned)nparts), dim3(256), 0, static_cast<hipStream_t>(stream), g, n, partials);
  return check_launch("grad_sqsum");
}

// status <- norm, clip coefficient, skip flag, skipped count from the nparts partials of ALL buffers (one workgroup, fixed order)
extern "C" int pvcnn_grad_norm_finalize(const float *partials, int nparts, float *status, void *stream) {
  PVCNN_REQUIRE(partials && status && nparts >= 1, "null partials / status block");
  hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), partials, nparts, status);
  return check_launch("grad_norm_finalize");
}
