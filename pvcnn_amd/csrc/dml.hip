// dml.hip -- the deep-mutual-learning criterion on two (B, C, S) logit tensors a (the first network) and b (the student):
//
//   per point i:   m_a = max_c a_c,  s_a = sum_c expf(a_c - m_a),  la_c = (a_c - m_a) - logf(s_a),  p_c = expf(a_c - m_a) / s_a
//                  m_b, s_b, lb_c, q_c likewise for b
//                  KL(p || q)_i = sum_c p_c (la_c - lb_c),   KL(q || p)_i = sum_c q_c (lb_c - la_c)
//
//   KL alone (kl_loss(x, y), x -> a, y -> b):  loss = sum_i KL(p || q)_i / (B S),  d loss / d y_j = g (q_j - p_j) / (B S); x is a
//     constant (the reference detaches it).  Three launches: partials, finalize, bwd.
//   Pair (the four terms of a DML step from one pass over both tensors):
//     loss[0] = sum_i w_t ((m_a - a_t) + logf(s_a)) / den + sum_i KL(q || p)_i / (B S)        den = sum_i w_t over the live points
//     loss[1] = sum_i w_t ((m_b - b_t) + logf(s_b)) / den + sum_i KL(p || q)_i / (B S)
//     d loss[side] / d x_j = g [w_t (x_p_j - [j == t]) / den + (x_p_j - other_p_j) / (B S)]   (x = a, other = b for side 0)
//   The cross-entropy terms are xent.hip's (class weights, ignore_index, reduction mean, no label smoothing), operation for
//   operation.  A point whose target is ignore_index, or outside [0, C) (counted, never used as an index), adds nothing to them and
//   gets no cross-entropy gradient; the KL terms take EVERY point -- the reference's KLLoss never sees the targets.  With every
//   point ignored den = 0: both losses are NaN (0 / 0, as torch), the gradients hold the KL part alone and no NaN.
//
// log p is formed as (a_c - m_a) - logf(s_a), never as logf(p_c): a class far below the maximum gives p_c = 0 and a finite log p_c,
// so the term is 0 where softmax(x) * log(softmax(x)) in fp32 is 0 * -inf = NaN.
//
// Conventions of xent.hip: lanes run along the points (a wave reads one class row of its 64 points as one request), C is a run-time
// value and the class loops re-read the logits from cache (no per-class register array), no float atomics, no ticket fold: per-lane
// fp64 sums meet by the fixed butterfly, one finalize workgroup adds the per-workgroup partials in index order in fp64.  Every word
// of every output and of the workspace is written; nothing is memset.
//
// workspace: [den, 1 / (B S), 0, 0] fp32 | (m_a, s_a, m_b, s_b) fp32 per point | K x xent_parts(B, S) fp64 partials (KL alone: K = 1,
// den = 0; pair: K = 6).  The per-point block comes first so that its 16-byte words stay aligned whatever the number of partials.
#include "xent_sums.h"

namespace pvcnn {

constexpr size_t kDmlStateBytes = 16;
constexpr int kDmlPairSums = 6;                // nll_a, nll_b, den, out-of-range targets, KL(q || p), KL(p || q)

// kPair: parts[k * gridDim.x + workgroup], k as in kDmlPairSums; else parts[workgroup] = sum KL(p || q) and the targets are not read.
// save[i] = (m_a, s_a, m_b, s_b) of every point i = b * S + position.
template <bool kPair>
__global__ __launch_bounds__(kXentThreads) void dml_partials_kernel(const float *__restrict__ a, size_t a_bstride,
                                                                    const float *__restrict__ b, size_t b_bstride,
                                                                    const long long *__restrict__ target, size_t t_bstride,
                                                                    const float *__restrict__ weight, long long B, int C, long long S,
                                                                    long long ignore_index, double *__restrict__ parts,
                                                                    float4 *__restrict__ save) {
  constexpr int K = kPair ? kDmlPairSums : 1;
  const long long P = B * S, stride = (long long)gridDim.x * kXentThreads;
  double acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0;
  for (long long i = (long long)blockIdx.x * kXentThreads + threadIdx.x; i < P; i += stride) {
    const long long n = i / S, pos = i - n * S;
    const float *__restrict__ ap = a + (size_t)n * a_bstride + (size_t)pos;
    const float *__restrict__ bp = b + (size_t)n * b_bstride + (size_t)pos;
    float ma = ap[0], mb = bp[0];
    for (int c = 1; c < C; ++c) {
      ma = fmaxf(ma, ap[(size_t)c * (size_t)S]);
      mb = fmaxf(mb, bp[(size_t)c * (size_t)S]);
    }
    float sa = 0.0f, sb = 0.0f;
    for (int c = 0; c < C; ++c) {
      sa += expf(ap[(size_t)c * (size_t)S] - ma);
      sb += expf(bp[(size_t)c * (size_t)S] - mb);
    }
    save[i] = make_float4(ma, sa, mb, sb);
    const float lsa = logf(sa), lsb = logf(sb);
    float kl_pq = 0.0f, kl_qp = 0.0f;
    for (int c = 0; c < C; ++c) {
      const float da = ap[(size_t)c * (size_t)S] - ma, db = bp[(size_t)c * (size_t)S] - mb;
      const float la = da - lsa, lb = db - lsb;
      kl_pq += expf(da) / sa * (la - lb);
      if constexpr (kPair) kl_qp += expf(db) / sb * (lb - la);
    }
    if constexpr (kPair) {
      acc[4] += (double)kl_qp;
      acc[5] += (double)kl_pq;
      const long long t = target[(size_t)n * t_bstride + (size_t)pos];
      if (t != ignore_index) {
        if ((unsigned long long)t < (unsigned long long)C) {
          const float wt = weight ? weight[t] : 1.0f;
          acc[0] += (double)(wt * ((ma - ap[(size_t)t * (size_t)S]) + lsa));
          acc[1] += (double)(wt * ((mb - bp[(size_t)t * (size_t)S]) + lsb));
          acc[2] += (double)wt;
        } else {
          acc[3] += 1.0;
        }
      }
    } else {
      acc[0] += (double)kl_pq;
    }
  }
  wg_sum(acc);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) parts[(size_t)k * gridDim.x + blockIdx.x] = acc[k];
  }
}

// One workgroup: thread t adds partials t, t + 256, ... in index order, the 256 sums meet by the fixed butterfly; everything fp64.
template <bool kPair>
__global__ __launch_bounds__(kXentThreads) void dml_finalize_kernel(const double *__restrict__ parts, int nparts, double points,
                                                                    float *__restrict__ state, float *__restrict__ loss,
                                                                    long long *bad_targets) {
  constexpr int K = kPair ? kDmlPairSums : 1;
  double acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kXentThreads) {
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] += parts[(size_t)k * nparts + i];
  }
  wg_sum(acc);
  if (threadIdx.x == 0) {
    if constexpr (kPair) {
      const double den = acc[2];                               // every point ignored: 0 / 0 = NaN, as torch
      loss[0] = (float)(acc[0] / den + acc[4] / points);
      loss[1] = (float)(acc[1] / den + acc[5] / points);
      state[0] = (float)den;
      if (bad_targets) bad_targets[0] += (long long)acc[3];
    } else {
      loss[0] = (float)(acc[0] / points);
      state[0] = 0.0f;
    }
    state[1] = (float)(1.0 / points);
    state[2] = 0.0f;
    state[3] = 0.0f;
  }
}

// grid.x strides the points, grid.y the classes: grad[n][c][pos] for every element.  x is the network the gradient is for, o the other
// one; `side` says which half of the saved (m_a, s_a, m_b, s_b) is x's.  target == nullptr: the KL gradient alone (kl_loss's, with
// x = y: side 1).  The cross-entropy factor g / den is only ever multiplied into a live point, so den = 0 leaves no NaN behind.
__global__ __launch_bounds__(kXentThreads) void dml_bwd_kernel(const float *__restrict__ x, size_t x_bstride,
                                                               const float *__restrict__ o, size_t o_bstride,
                                                               const long long *__restrict__ target, size_t t_bstride,
                                                               const float *__restrict__ weight, const float *__restrict__ grad_out,
                                                               long long B, int C, long long S, long long ignore_index, int side,
                                                               const float *__restrict__ state, const float4 *__restrict__ save,
                                                               float *__restrict__ grad) {
  const long long P = B * S, stride = (long long)gridDim.x * kXentThreads;
  const float k_ce = target ? grad_out[0] / state[0] : 0.0f, k_kl = grad_out[0] * state[1];
  for (long long i = (long long)blockIdx.x * kXentThreads + threadIdx.x; i < P; i += stride) {
    const long long n = i / S, pos = i - n * S;
    const long long t = target ? target[(size_t)n * t_bstride + (size_t)pos] : ignore_index;
    const bool live = target && t != ignore_index && (unsigned long long)t < (unsigned long long)C;
    const float *__restrict__ xp = x + (size_t)n * x_bstride + (size_t)pos;
    const float *__restrict__ op = o + (size_t)n * o_bstride + (size_t)pos;
    float *__restrict__ gp = grad + (size_t)n * (size_t)C * (size_t)S + (size_t)pos;
    const float4 ms = save[i];
    const float mx = side ? ms.z : ms.x, sx = side ? ms.w : ms.y, mo = side ? ms.x : ms.z, so = side ? ms.y : ms.w;
    const float k_t = live ? k_ce * (weight ? weight[t] : 1.0f) : 0.0f;
    for (int c = blockIdx.y; c < C; c += gridDim.y) {
      const float px = expf(xp[(size_t)c * (size_t)S] - mx) / sx, po = expf(op[(size_t)c * (size_t)S] - mo) / so;
      float g = k_kl * (px - po);
      if (live) g = k_t * (px - (c == t ? 1.0f : 0.0f)) + g;
      gp[(size_t)c * (size_t)S] = g;
    }
  }
}

static size_t dml_workspace_bytes(long long B, long long S, int sums) {
  if (!xent_points_ok(B, S)) return 0;
  return kDmlStateBytes + sizeof(float4) * (size_t)(B * S) + (size_t)sums * sizeof(double) * (size_t)xent_parts(B, S);
}
static float4 *dml_save(void *workspace) { return reinterpret_cast<float4 *>(static_cast<char *>(workspace) + kDmlStateBytes); }
static double *dml_parts(void *workspace, long long B, long long S) { return reinterpret_cast<double *>(dml_save(workspace) + B * S); }

static dim3 dml_bwd_grid(long long B, int C, long long S) {
  const long long blocks = (B * S + kXentThreads - 1) / kXentThreads;
  return dim3((unsigned)(blocks < kXentBwdMaxBlocks ? blocks : kXentBwdMaxBlocks),
              (unsigned)(C < kXentBwdMaxClassRows ? C : kXentBwdMaxClassRows));
}

}  // namespace pvcnn

using namespace pvcnn;

extern "C" size_t pvcnn_kl_workspace_bytes(long long B, long long S) { return dml_workspace_bytes(B, S, 1); }

extern "C" size_t pvcnn_dml_pair_workspace_bytes(long long B, long long S) { return dml_workspace_bytes(B, S, kDmlPairSums); }

extern "C" int pvcnn_kl_partials(const float *x, long long x_bstride, const float *y, long long y_bstride, long long B, int C, long long S,
                                 void *workspace, void *stream) {
  // (values first, pointers second: a call with a bad value is refused whatever its pointers are)
  PVCNN_REQUIRE(xent_sizes_ok(B, C, S), "bad size");
  PVCNN_REQUIRE(x_bstride >= (long long)C * S && y_bstride >= (long long)C * S, "batch strides: logits >= C * S");
  PVCNN_REQUIRE(x && y && workspace, "null pointer");
  PVCNN_REQUIRE(aligned16(workspace), "the workspace must be 16-byte aligned");
  hipLaunchKernelGGL(dml_partials_kernel<false>, dim3((unsigned)xent_parts(B, S)), dim3(kXentThreads), 0, static_cast<hipStream_t>(stream),
                     x, (size_t)x_bstride, y, (size_t)y_bstride, (const long long *)nullptr, (size_t)0, (const float *)nullptr, B, C, S, 0ll,
                     dml_parts(workspace, B, S), dml_save(workspace));
  return check_launch("kl_partials");
}

extern "C" int pvcnn_kl_finalize(long long B, int C, long long S, void *workspace, float *loss, void *stream) {
  PVCNN_REQUIRE(xent_sizes_ok(B, C, S), "bad size");
  PVCNN_REQUIRE(workspace && loss, "null pointer");
  PVCNN_REQUIRE(aligned16(workspace), "the workspace must be 16-byte aligned");
  hipLaunchKernelGGL(dml_finalize_kernel<false>, dim3(1), dim3(kXentThreads), 0, static_cast<hipStream_t>(stream),
                     dml_parts(workspace, B, S), (int)xent_parts(B, S), (double)(B * S), static_cast<float *>(workspace), loss,
                     (long long *)nullptr);
  return check_launch("kl_finalize");
}

extern "C" int pvcnn_kl_bwd(const float *x, long long x_bstride, const float *y, long long y_bstride, const float *grad_out, long long B,
                            int C, long long S, const void *workspace, float *grad_y, void *stream) {
  PVCNN_REQUIRE(xent_sizes_ok(B, C, S), "bad size");
  PVCNN_REQUIRE(x_bstride >= (long long)C * S && y_bstride >= (long long)C * S, "batch strides: logits >= C * S");
  PVCNN_REQUIRE(x && y && grad_out && workspace && grad_y, "null pointer");
  PVCNN_REQUIRE(aligned16(workspace), "the workspace must be 16-byte aligned");
  void *ws = const_cast<void *>(workspace);
  hipLaunchKernelGGL(dml_bwd_kernel, dml_bwd_grid(B, C, S), dim3(kXentThreads), 0, static_cast<hipStream_t>(stream), y, (size_t)y_bstride, x,
                     (size_t)x_bstride, (const long long *)nullptr, (size_t)0, (const float *)nullptr, grad_out, B, C, S, 0ll, 1,
                     static_cast<const float *>(workspace), (const float4 *)dml_save(ws), grad_y);
  return check_launch("kl_bwd");
}

extern "C" int pvcnn_dml_pair_partials(const float *a, long long a_bstride, const float *b, long long b_bstride, const long long *target,
                                       long long t_bstride, const float *weight, long long B, int C, long long S, long long ignore_index,
                                       void *workspace, void *stream) {
  PVCNN_REQUIRE(xent_sizes_ok(B, C, S), "bad size");
  PVCNN_REQUIRE(a_bstride >= (long long)C * S && b_bstride >= (long long)C * S && t_bstride >= S,
                "batch strides: logits >= C * S, targets >= S");
  PVCNN_REQUIRE(a && b && target && workspace, "null pointer");
  PVCNN_REQUIRE(aligned16(workspace), "the workspace must be 16-byte aligned");
  hipLaunchKernelGGL(dml_partials_kernel<true>, dim3((unsigned)xent_parts(B, S)), dim3(kXentThreads), 0, static_cast<hipStream_t>(stream), a,
                     (size_t)a_bstride, b, (size_t)b_bstride, target, (size_t)t_bstride, weight, B, C, S, ignore_index,
                     dml_parts(workspace, B, S), dml_save(workspace));
  return check_launch("dml_pair_partials");
}

extern "C" int pvcnn_dml_pair_finalize(long long B, int C, long long S, void *workspace, float *loss, long long *bad_targets, void *stream) {
  PVCNN_REQUIRE(xent_sizes_ok(B, C, S), "bad size");
  PVCNN_REQUIRE(workspace && loss, "null pointer");
  PVCNN_REQUIRE(aligned16(workspace), "the workspace must be 16-byte aligned");
  hipLaunchKernelGGL(dml_finalize_kernel<true>, dim3(1), dim3(kXentThreads), 0, static_cast<hipStream_t>(stream),
                     dml_parts(workspace, B, S), (int)xent_parts(B, S), (double)(B * S), static_cast<float *>(workspace), loss, bad_targets);
  return check_launch("dml_pair_finalize");
}

extern "C" int pvcnn_dml_pair_bwd(const float *a, long long a_bstride, const float *b, long long b_bstride, const long long *target,
                                  long long t_bstride, const float *weight, const float *grad_out, long long B, int C, long long S,
                                  long long ignore_index, int side, const void *workspace, float *grad, void *stream) {
  PVCNN_REQUIRE(xent_sizes_ok(B, C, S), "bad size");
  PVCNN_REQUIRE(a_bstride >= (long long)C * S && b_bstride >= (long long)C * S && t_bstride >= S,
                "batch strides: logits >= C * S, targets >= S");
  PVCNN_REQUIRE(side == 0 || side == 1, "side must be 0 (the first network) or 1 (the student)");
  PVCNN_REQUIRE(a && b && target && grad_out && workspace && grad, "null pointer");
  PVCNN_REQUIRE(aligned16(workspace), "the workspace must be 16-byte aligned");
  void *ws = const_cast<void *>(workspace);
  hipLaunchKernelGGL(dml_bwd_kernel, dml_bwd_grid(B, C, S), dim3(kXentThreads), 0, static_cast<hipStream_t>(stream), side ? b : a,
                     (size_t)(side ? b_bstride : a_bstride), side ? a : b, (size_t)(side ? a_bstride : b_bstride), target,
                     (size_t)t_bstride, weight, grad_out, B, C, S, ignore_index, side, static_cast<const float *>(workspace),
                     (const float4 *)dml_save(ws), grad);
  return check_launch("dml_pair_bwd");
}
