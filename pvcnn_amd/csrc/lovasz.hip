// lovasz.hip -- the Lovasz-Softmax criterion (Berman et al., CVPR 2018; per_image, classes 'present' / 'all', ignore_index) on
// (B, C, S) logits or probabilities with int64 (B, S) targets, and its gradient: three launches forward (two on probabilities),
// one backward.  The definition is stated once, in include/pvcnn_hip.h ("The Lovasz-Softmax criterion"); in short, per cloud b and
// class c, over the live points (target != ignore_index and inside [0, C)):
//
//   e_i = fg_i ? 1.0f - p_i : p_i                      (fg_i = target_i == c; ONE fp32 subtraction)
//   order: e descending, ties by ascending point index
//   walking the order (i = 1, 2, ...; cf = foreground seen so far; G = foreground in all): I = G - cf, U = G + i - cf,
//   step_i = 1 / U (foreground), I / (U (U - 1)) (background), 1 for the first element of a list without foreground    [fp64]
//   loss(b, c) = sum_i e_(i) step_i                                                                                  [fp64]
//
// One list (N = 2048 / 4096 / 8192 points) fits in the LDS of one workgroup, and the B x C lists are independent: lovasz_sort_kernel
// runs one workgroup per list.  A point becomes one 64-bit word, (order-reversing bits of e) << 32 | index << 1 | fg: all words of a
// list differ, so the bitonic network's result is ONE total order -- the stable descending order of the definition -- whatever the
// network's exchange pattern; a dead point is the all-ones word and sorts behind every live one.  After the sort a thread owns a
// run of consecutive positions: one workgroup scan of the fg bits gives it cf in front of its run, it walks the run, adds e * step
// in fp64 and scatters -step / +step (d loss(b, c) / d p) to the point's place in grad_p.
//
// Deterministic: no float atomics; a thread's sum runs in position order, the threads' sums meet by the fixed butterfly (wave.h) and
// the wave totals are added in wave order; the finalize is one workgroup.  Every word of every output is written; nothing is memset.
#include "xent_sums.h"

namespace pvcnn {

constexpr int kLovaszMaxPoints = 16384;        // one list's words in LDS: 128 KiB of the CU's 160
constexpr int kLovaszMaxThreads = 1024;
constexpr int kLovaszMaxWaves = kLovaszMaxThreads / kWave;
constexpr int kLovaszMaxBatch = 65535;         // grid.y of the sort launch
constexpr int kLovaszParts = 4;                // per list, fp64: loss, foreground points, live points, out-of-range targets
constexpr unsigned long long kLovaszDead = ~0ull;

inline bool lovasz_sizes_ok(long long B, int C, long long S) {
  return xent_sizes_ok(B, C, S) && S <= kLovaszMaxPoints && B <= kLovaszMaxBatch;
}
inline size_t lovasz_scale_bytes(long long B) { return ((size_t)B * sizeof(float) + 15) & ~(size_t)15; }
inline int lovasz_npad(long long S) {
  int npad = 1;
  while (npad < S) npad <<= 1;
  return npad;
}
// four words per thread (two exchanges per step of the network), within [one wave, 1024 threads]
inline int lovasz_threads(int npad) {
  const int t = npad / 4;
  return t < kWave ? kWave : (t > kLovaszMaxThreads ? kLovaszMaxThreads : t);
}

// p[b][c][pos] = expf(x_c - max) / sum_c expf(x_c - max): lanes along the points, like xent_partials_kernel
__global__ __launch_bounds__(kXentThreads) void lovasz_probs_kernel(const float *__restrict__ x, size_t x_bstride, long long B, int C,
                                                                    long long S, float *__restrict__ p) {
  const long long P = B * S, stride = (long long)gridDim.x * kXentThreads;
  for (long long i = (long long)blockIdx.x * kXentThreads + threadIdx.x; i < P; i += stride) {
    const long long b = i / S, pos = i - b * S;
    const float *__restrict__ xp = x + (size_t)b * x_bstride + (size_t)pos;
    float *__restrict__ pp = p + (size_t)b * (size_t)C * (size_t)S + (size_t)pos;
    float m = xp[0];
    for (int c = 1; c < C; ++c) m = fmaxf(m, xp[(size_t)c * (size_t)S]);
    float s = 0.0f;
    for (int c = 0; c < C; ++c) s += expf(xp[(size_t)c * (size_t)S] - m);
    for (int c = 0; c < C; ++c) pp[(size_t)c * (size_t)S] = expf(xp[(size_t)c * (size_t)S] - m) / s;
  }
}

// e >= 0 descending == word ascending: the bits of a float order like the float once the sign is folded in; ~ reverses them
__device__ __forceinline__ uint32_t lovasz_key(float e) {
  const uint32_t u = __float_as_uint(e + 0.0f);                // (-0 -> +0: the two are one value to the order)
  return ~((u & 0x80000000u) ? ~u : (u | 0x80000000u));
}
__device__ __forceinline__ float lovasz_error(uint32_t key) {
  const uint32_t u = ~key;
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// (x, y) in order: ascending when up, else descending
__device__ __forceinline__ void lovasz_exchange(unsigned long long &x, unsigned long long &y, bool up) {
  const bool swap = (x > y) == up;
  const unsigned long long lo = swap ? y : x, hi = swap ? x : y;
  x = lo; y = hi;
}

// The sums of three ints over the workgroup (<= 16 waves), in every thread.  Two barriers; s (3 x 16 words) is free again after it.
__device__ __forceinline__ void lovasz_wg_sum3(int (&v)[3], int *s) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int t = wave_sum(v[k]);
    if (lane == 0) s[k * kLovaszMaxWaves + wave] = t;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    int t = 0;
    for (int w = 0; w < nwaves; ++w) t += s[k * kLovaszMaxWaves + w];
    v[k] = t;
  }
  __syncthreads();
}

// grid (C, B), blockDim = lovasz_threads(npad), npad * 8 bytes of dynamic LDS.  parts[(b * C + c) * 4 ..]: see kLovaszParts.
// grad_p[b][c][.] (packed) gets d loss(b, c) / d p: zeros for a dead point and for a whole class that is not counted.
__global__ __launch_bounds__(kLovaszMaxThreads) void lovasz_sort_kernel(const float *__restrict__ p, size_t p_bstride,
                                                                        const long long *__restrict__ target, size_t t_bstride, int C,
                                                                        int S, int npad, long long ignore_index, int classes_all,
                                                                        double *__restrict__ parts, float *__restrict__ grad_p) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long lovasz_words[];
  __shared__ int s_int[3 * kLovaszMaxWaves];
  __shared__ double s_sum[kLovaszMaxWaves];
  const int c = blockIdx.x, b = blockIdx.y, nthreads = blockDim.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = nthreads >> 6;
  const float *__restrict__ pr = p + (size_t)b * p_bstride + (size_t)c * (size_t)S;
  const long long *__restrict__ tr = target + (size_t)b * t_bstride;
  float *__restrict__ gr = grad_p + ((size_t)b * (size_t)C + (size_t)c) * (size_t)S;
  double *__restrict__ out = parts + ((size_t)b * (size_t)C + (size_t)c) * kLovaszParts;

  int cnt[3] = {0, 0, 0};                                     // foreground, live, out of range
  for (int i = threadIdx.x; i < S; i += nthreads) {
    const long long t = tr[i];
    if (t != ignore_index) {
      if ((unsigned long long)t < (unsigned long long)C) { cnt[1] += 1; cnt[0] += (t == c) ? 1 : 0; }
      else cnt[2] += 1;
    }
  }
  lovasz_wg_sum3(cnt, s_int);
  const int G = cnt[0], n = cnt[1];
  const bool counted = classes_all ? n > 0 : G > 0;
  if (!counted) {                                             // (workgroup-uniform)
    for (int i = threadIdx.x; i < S; i += nthreads) gr[i] = 0.0f;
    if (threadIdx.x == 0) { out[0] = 0.0; out[1] = (double)G; out[2] = (double)n; out[3] = (double)cnt[2]; }
    return;
  }

  for (int i = threadIdx.x; i < npad; i += nthreads) {
    unsigned long long w = kLovaszDead;
    if (i < S) {
      const long long t = tr[i];
      if (t != ignore_index && (unsigned long long)t < (unsigned long long)C) {
        const float pi = pr[i];
        const bool fg = t == c;
        const float e = fg ? 1.0f - pi : pi;
        w = ((unsigned long long)lovasz_key(e) << 32) | ((unsigned long long)i << 1) | (fg ? 1ull : 0ull);
      } else {
        gr[i] = 0.0f;
      }
    }
    lovasz_words[i] = w;
  }
  __syncthreads();
  // The bitonic network, two steps per pass over the LDS: the steps j and h = j / 2 of a phase touch, from a word whose bits j and h
  // are 0, the four words base, base + h, base + j, base + j + h and no others, so a thread that holds the four does both steps in
  // registers (half the LDS traffic and half the barriers of one step per pass: measured, profiles/criterion.md).  A phase with an odd
  // number of steps does its first step (j = k / 2) alone.  Ascending where bit k of the position is 0 -- the same for all four.
  for (int k = 2, steps = 1; k <= npad; k <<= 1, ++steps) {
    int j = k >> 1;
    if (steps & 1) {
      for (int t = threadIdx.x; t < (npad >> 1); t += nthreads) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo + j;
        const unsigned long long x = lovasz_words[lo], y = lovasz_words[hi];
        if ((x > y) == ((lo & k) == 0)) { lovasz_words[lo] = y; lovasz_words[hi] = x; }
      }
      __syncthreads();
      j >>= 1;
    }
    for (; j >= 2; j >>= 2) {
      const int h = j >> 1;
      for (int q = threadIdx.x; q < (npad >> 2); q += nthreads) {
        const int base = ((q & ~(h - 1)) << 2) | (q & (h - 1));
        const bool up = (base & k) == 0;
        unsigned long long a0 = lovasz_words[base], a1 = lovasz_words[base + h], a2 = lovasz_words[base + j],
                           a3 = lovasz_words[base + j + h];
        lovasz_exchange(a0, a2, up);
        lovasz_exchange(a1, a3, up);
        lovasz_exchange(a0, a1, up);
        lovasz_exchange(a2, a3, up);
        lovasz_words[base] = a0; lovasz_words[base + h] = a1; lovasz_words[base + j] = a2; lovasz_words[base + j + h] = a3;
      }
      __syncthreads();
    }
  }

  // positions [first, last) of the sorted list are this thread's; cf in front of them by one scan over the threads
  const int per = (npad + nthreads - 1) / nthreads;
  const int first = min((int)threadIdx.x * per, n), last = min(first + per, n);
  int mine = 0;
  for (int i = first; i < last; ++i) mine += (int)(lovasz_words[i] & 1ull);
  const int incl = wave_inclusive_scan(mine, lane);
  if (lane == 63) s_int[wave] = incl;
  __syncthreads();
  int cf = incl - mine;
  for (int w = 0; w < wave; ++w) cf += s_int[w];

  double acc = 0.0;
  for (int i = first; i < last; ++i) {
    const unsigned long long w = lovasz_words[i];
    const bool fg = (w & 1ull) != 0;
    const int idx = (int)((uint32_t)w >> 1);
    cf += fg ? 1 : 0;
    const int I = G - cf, U = G + (i + 1) - cf;               // U >= 1
    double step;
    if (fg) step = 1.0 / (double)U;
    else step = U == 1 ? 1.0 : (double)I / ((double)U * (double)(U - 1));   // U == 1: no foreground at all, the first element
    acc += (double)lovasz_error((uint32_t)(w >> 32)) * step;
    gr[idx] = fg ? -(float)step : (float)step;
  }
  acc = wave_sum(acc);
  if (lane == 0) s_sum[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = s_sum[0];
    for (int w = 1; w < nwaves; ++w) total += s_sum[w];
    out[0] = total; out[1] = (double)G; out[2] = (double)n; out[3] = (double)cnt[2];
  }
}

// One workgroup.  A thread owns the clouds t, t + 256, ...: counted classes k_b, the cloud's mean, scale[b] = 1 / (k_b B) (0 for a
// cloud without counted classes); the threads' sums meet by wg_sum.  loss[0] = sum_b cloud_b / B.
__global__ __launch_bounds__(kXentThreads) void lovasz_finalize_kernel(const double *__restrict__ parts, int B, int C, int classes_all,
                                                                       float *__restrict__ scale, float *__restrict__ loss,
                                                                       long long *bad_targets) {
  double acc[2] = {0.0, 0.0};                                 // sum of the cloud losses, out-of-range targets
  for (int b = threadIdx.x; b < B; b += kXentThreads) {
    const double *row = parts + (size_t)b * (size_t)C * kLovaszParts;
    double sum = 0.0;
    int k = 0;
    for (int c = 0; c < C; ++c) {
      sum += row[(size_t)c * kLovaszParts];
      k += row[(size_t)c * kLovaszParts + 1] > 0.0 ? 1 : 0;
    }
    if (classes_all) k = row[2] > 0.0 ? C : 0;
    acc[0] += k > 0 ? sum / (double)k : 0.0;
    acc[1] += row[3];
    scale[b] = k > 0 ? (float)(1.0 / ((double)k * (double)B)) : 0.0f;
  }
  wg_sum(acc);
  if (threadIdx.x == 0) {
    loss[0] = (float)(acc[0] / (double)B);
    if (bad_targets) bad_targets[0] += (long long)acc[1];
  }
}

// grid.x strides the points, grid.y the classes.  g_c = grad_out scale[b] grad_p[b][c][pos] is d loss / d p_c;
// probabilities: grad[b][c][pos] = g_c; logits: p_c (g_c - sum_j p_j g_j) (every grid.y row forms the same sum in the same order)
__global__ __launch_bounds__(kXentThreads) void lovasz_bwd_kernel(const float *__restrict__ p, size_t p_bstride,
                                                                  const float *__restrict__ grad_p, const float *__restrict__ grad_out,
                                                                  const float *__restrict__ scale, long long B, int C, long long S,
                                                                  int probas, float *__restrict__ grad) {
  const long long P = B * S, stride = (long long)gridDim.x * kXentThreads;
  const float g0 = grad_out[0];
  for (long long i = (long long)blockIdx.x * kXentThreads + threadIdx.x; i < P; i += stride) {
    const long long b = i / S, pos = i - b * S;
    const float k = g0 * scale[b];
    const float *__restrict__ pp = p + (size_t)b * p_bstride + (size_t)pos;
    const float *__restrict__ gp = grad_p + (size_t)b * (size_t)C * (size_t)S + (size_t)pos;
    float *__restrict__ out = grad + (size_t)b * (size_t)C * (size_t)S + (size_t)pos;
    if (probas) {
      for (int c = blockIdx.y; c < C; c += gridDim.y) out[(size_t)c * (size_t)S] = k * gp[(size_t)c * (size_t)S];
      continue;
    }
    // g_j - sum_c p_c g_c cancels to nothing at a saturated point (p one-hot: the difference is of the order of 1 - p_max while the
    // terms are of the order of g): the products of two fp32 values are exact in fp64, the sum and the difference are formed there,
    // and the result is rounded to fp32 once -- an fp32 sum leaves an error of eps * |g|, far above such a point's gradient
    double dot = 0.0;
    for (int c = 0; c < C; ++c) dot += (double)pp[(size_t)c * (size_t)S] * ((double)k * (double)gp[(size_t)c * (size_t)S]);
    for (int c = blockIdx.y; c < C; c += gridDim.y) {
      const double g = (double)k * (double)gp[(size_t)c * (size_t)S];
      out[(size_t)c * (size_t)S] = (float)((double)pp[(size_t)c * (size_t)S] * (g - dot));
    }
  }
}

}  // namespace pvcnn

using namespace pvcnn;

extern "C" size_t pvcnn_lovasz_workspace_bytes(long long B, int C, long long S) {
  if (!lovasz_sizes_ok(B, C, S)) return 0;
  return lovasz_scale_bytes(B) + kLovaszParts * sizeof(double) * (size_t)B * (size_t)C;
}

extern "C" int pvcnn_lovasz_probs(const float *x, long long x_bstride, long long B, int C, long long S, float *p, void *stream) {
  PVCNN_REQUIRE(lovasz_sizes_ok(B, C, S), "bad size");
  PVCNN_REQUIRE(x_bstride >= (long long)C * S, "batch stride: logits >= C * S");
  PVCNN_REQUIRE(x && p, "null pointer");
  hipLaunchKernelGGL(lovasz_probs_kernel, dim3((unsigned)xent_parts(B, S)), dim3(kXentThreads), 0, static_cast<hipStream_t>(stream), x,
                     (size_t)x_bstride, B, C, S, p);
  return check_launch("lovasz_probs");
}

extern "C" int pvcnn_lovasz_sort(const float *p, long long p_bstride, const long long *target, long long t_bstride, long long B, int C,
                                 long long S, long long ignore_index, int classes_all, void *workspace, float *grad_p, void *stream) {
  PVCNN_REQUIRE(lovasz_sizes_ok(B, C, S), "bad size");
  PVCNN_REQUIRE(p_bstride >= (long long)C * S && t_bstride >= S, "batch strides: probabilities >= C * S, targets >= S");
  PVCNN_REQUIRE(p && target && workspace && grad_p, "null pointer");
  PVCNN_REQUIRE(aligned16(workspace), "the workspace must be 16-byte aligned");
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(lovasz_sort_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       kLovaszMaxPoints * (int)sizeof(unsigned long long));
    if (e != hipSuccess) { set_error("lovasz_sort: LDS attribute: %s", hipGetErrorString(e)); return (int)e; }
    attr_set = true;
  }
  const int npad = lovasz_npad(S);
  double *parts = reinterpret_cast<double *>(static_cast<char *>(workspace) + lovasz_scale_bytes(B));
  hipLaunchKernelGGL(lovasz_sort_kernel, dim3((unsigned)C, (unsigned)B), dim3(lovasz_threads(npad)), (size_t)npad * sizeof(unsigned long long),
                     static_cast<hipStream_t>(stream), p, (size_t)p_bstride, target, (size_t)t_bstride, C, (int)S, npad, ignore_index,
                     classes_all, parts, grad_p);
  return check_launch("lovasz_sort");
}

extern "C" int pvcnn_lovasz_finalize(long long B, int C, long long S, int classes_all, void *workspace, float *loss,
                                     long long *bad_targets, void *stream) {
  PVCNN_REQUIRE(lovasz_sizes_ok(B, C, S), "bad size");
  PVCNN_REQUIRE(workspace && loss, "null pointer");
  PVCNN_REQUIRE(aligned16(workspace), "the workspace must be 16-byte aligned");
  float *scale = static_cast<float *>(workspace);
  const double *parts = reinterpret_cast<const double *>(static_cast<char *>(workspace) + lovasz_scale_bytes(B));
  hipLaunchKernelGGL(lovasz_finalize_kernel, dim3(1), dim3(kXentThreads), 0, static_cast<hipStream_t>(stream), parts, (int)B, C,
                     classes_all, scale, loss, bad_targets);
  return check_launch("lovasz_finalize");
}

extern "C" int pvcnn_lovasz_bwd(const float *p, long long p_bstride, const float *grad_p, const float *grad_out, long long B, int C,
                                long long S, int probas, const void *workspace, float *grad, void *stream) {
  PVCNN_REQUIRE(lovasz_sizes_ok(B, C, S), "bad size");
  PVCNN_REQUIRE(p_bstride >= (long long)C * S, "batch stride: probabilities >= C * S");
  PVCNN_REQUIRE(p && grad_p && grad_out && workspace && grad, "null pointer");
  PVCNN_REQUIRE(aligned16(workspace), "the workspace must be 16-byte aligned");
  const long long blocks = (B * S + kXentThreads - 1) / kXentThreads;
  // every class row of the grid forms the point's whole sum again: only as many rows as it takes to fill the chip
  long long rows = (4 * kNumCU + blocks - 1) / blocks;
  rows = rows < 1 ? 1 : (rows > kXentBwdMaxClassRows ? kXentBwdMaxClassRows : rows);
  const dim3 grid((unsigned)(blocks < kXentBwdMaxBlocks ? blocks : kXentBwdMaxBlocks), (unsigned)(C < rows ? C : rows));
  hipLaunchKernelGGL(lovasz_bwd_kernel, grid, dim3(kXentThreads), 0, static_cast<hipStream_t>(stream), p, (size_t)p_bstride, grad_p, grad_out,
                     static_cast<const float *>(workspace), B, C, S, probas, grad);
  return check_launch("lovasz_bwd");
}
