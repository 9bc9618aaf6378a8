// wave.h -- the fixed-order reductions and scans of the kernels, over a wave (64 lanes) and over a workgroup's waves (device code).
//
// The bit-exact, deterministic results of this library rest on the ORDER of these additions; the oracle parity tests and the "same bits
// as the kernel it replaces" tests pin it.  A kernel that needs one of them calls it here, it does not write the loop again.
//   * wave_sum / wave_sum2 / wave_max / wave_min: the xor butterfly over the lane bits 5, 4, 3, 2, 1, 0 (offsets 32, 16, 8, 4, 2, 1), in
//     that order; the result is in EVERY lane.
//   * wave_inclusive_scan: the __shfl_up scan, offsets 1, 2, 4, 8, 16, 32.
//   * wg_sum: the wave totals of a 256-thread workgroup, added in wave order: ((w0 + w1) + w2) + w3.
//   * wg_max: the wave maxima of a workgroup (order-free), in thread 0.
//   * half_wave_sum16 / half_wave_sum8: 16 / 8 sums over a half-wave at once (the GEMM epilogues' statistics).
//   * amax_table_max_wave / amax_table_value: the maximum of an amax buffer's table.
// PRECONDITION of all of them: every lane of the calling wave is active (a lane that is not would hand the shuffle an undefined value:
// undefined totals, undefined winners); wg_sum / wg_max contain a barrier, so every thread of the workgroup must call them.  Where the
// lane count depends on an argument, the host entry checks it (pvcnn_bnact_apply_rowmax: 256 % amax_seg == 0).
// Not here, because they are other patterns: the DPP maxima of fps.hip, the argmax reductions with a tie rule (pool.hip, kitti_ap.hip:
// wave_best), butterflies over 2 or 4 lanes, and a few loops that fold two different operations per step (csr.h, rooms.hip).
#pragma once
#include "common.h"

namespace pvcnn {

#ifdef __HIPCC__
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// two sums at once, their steps interleaved (the sum and the sum of squares of the BatchNorm passes)
template <typename T>
__device__ __forceinline__ void wave_sum2(T &a, T &b) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
}
// (bit patterns of non-negative floats, mostly: they order like the floats)
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
  return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {     // fmaxf: a NaN loses
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// lane l ends with v of the lanes 0 .. l; `lane` = the caller's lane index in its wave
template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T v, int lane) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const T up = __shfl_up(v, o);
    if (lane >= o) v += up;
  }
  return v;
}

// The sums of K per-lane values over a workgroup of 256 threads, in every thread: lane 0 of each wave writes its wave_sum, one barrier,
// the four totals are added in wave order.  K * 4 words of LDS of its own per instantiation: a kernel that calls the same instantiation
// twice puts a barrier between the calls.
template <typename T, int K>
__device__ __forceinline__ void wg_sum(T (&v)[K]) {
  __shared__ T s_wave[K][4];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    T t = v[k];                                               // wave_sum, written out: called inside this loop the compiler hoists
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);   // every step's lane arithmetic out of it: other code than the kernels had
    v[k] = t;
    if ((threadIdx.x & 63) == 0) s_wave[k][threadIdx.x >> 6] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = ((s_wave[k][0] + s_wave[k][1]) + s_wave[k][2]) + s_wave[k][3];
}
template <typename T>
__device__ __forceinline__ T wg_sum(T v) {
  T a[1] = {v};
  wg_sum(a);
  return a[0];
}

// The maximum of v over a workgroup, in THREAD 0 (the other threads get their wave's): lane 0 of each wave writes its wave_max to
// s_wave[wave] (the caller's LDS, one word per wave), one barrier, thread 0 folds the other waves' words into its own.  NW = the
// workgroup's waves where the kernel fixes them, 0 = by blockDim.x.
template <int NW = 0>
__device__ __forceinline__ uint32_t wg_max(uint32_t v, uint32_t *s_wave) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nwaves = NW ? NW : (int)((blockDim.x + 63) >> 6);
    for (int w = 1; w < nwaves; ++w) v = max(v, s_wave[w]);
  }
  return v;
}

// Sum each of 16 per-lane values over the 32 lanes of a half-wave (lanes that differ in bits 0..4) with a
// transposing butterfly: every step halves the number of values a lane carries (the lane keeps one half and
// ships the other), so it takes 8+4+2+1+1 = 16 shuffles instead of 16*5.  Returns, in lane j, the total of
// value index (j >> 1) & 15 (both lanes of a pair hold the same total).
__device__ __forceinline__ float half_wave_sum16(const float (&v)[16], int lane) {
  float a[8], b[4], c[2];
  const bool b4 = lane & 16, b3 = lane & 8, b2 = lane & 4, b1 = lane & 2;
#pragma unroll
  for (int r = 0; r < 8; ++r) a[r] = (b4 ? v[r + 8] : v[r]) + __shfl_xor(b4 ? v[r] : v[r + 8], 16);
#pragma unroll
  for (int r = 0; r < 4; ++r) b[r] = (b3 ? a[r + 4] : a[r]) + __shfl_xor(b3 ? a[r] : a[r + 4], 8);
#pragma unroll
  for (int r = 0; r < 2; ++r) c[r] = (b2 ? b[r + 2] : b[r]) + __shfl_xor(b2 ? b[r] : b[r + 2], 4);
  float d = (b1 ? c[1] : c[0]) + __shfl_xor(b1 ? c[0] : c[1], 2);
  d += __shfl_xor(d, 1);
  return d;
}
// The same for 8 values per lane (7 + 2 shuffles): returns, in lane j, the total of value index (j >> 2) & 7.  Every total is the
// butterfly over the lane bits 4, 3, 2, 1, 0 in that order, like half_wave_sum16's: value q of an 8-value call carries the same
// bits as value q of a 16-value call on the same numbers (fp32 addition commutes; the tree is the same).
__device__ __forceinline__ float half_wave_sum8(const float (&v)[8], int lane) {
  float a[4], b[2];
  const bool b4 = lane & 16, b3 = lane & 8, b2 = lane & 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) a[r] = (b4 ? v[r + 4] : v[r]) + __shfl_xor(b4 ? v[r] : v[r + 4], 16);
#pragma unroll
  for (int r = 0; r < 2; ++r) b[r] = (b3 ? a[r + 2] : a[r]) + __shfl_xor(b3 ? a[r] : a[r + 2], 8);
  float c = (b2 ? b[1] : b[0]) + __shfl_xor(b2 ? b[0] : b[1], 4);
  c += __shfl_xor(c, 2);
  c += __shfl_xor(c, 1);
  return c;
}

// out[0] = max over the table out[1 .. T] of an amax buffer, by the calling workgroup (every thread calls; <= 1024 threads).  Used by
// the workgroup that takes the last ticket in the kernels that PUBLISH the table (common.h: ticket_take): the entries are peeked.
// (single wave: the 64 lanes of the wave that took the last ticket; T small -- see the callers' bounds)
__device__ __forceinline__ void amax_table_max_wave(uint32_t *out, long T) {
  uint32_t m = 0;
  for (long i = threadIdx.x & 63; i < T; i += 64) m = max(m, peek32(out + 1 + i));
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) out[0] = m;
}

// (ABI v12) max |x| of the tensor behind an amax buffer, for every thread of the calling workgroup (all of them call; two barriers):
// T > 0: the maximum of the table buf[1 .. T] -- word [0] is not read, its producer may have left it unwritten (PVCNN_TABLE_ONLY:
// no one-workgroup launch behind the table pass); T == 0: buf[0] (a 1-word buffer, or an amax buffer with its word [0]).
__device__ __forceinline__ uint32_t amax_table_value(const uint32_t *__restrict__ buf, long T) {
  if (T <= 0) return buf[0];
  __shared__ uint32_t s_amax_val[17];
  uint32_t m = 0;
  for (long i = threadIdx.x; i < T; i += blockDim.x) m = max(m, buf[1 + i]);
  m = wg_max(m, s_amax_val);
  if (threadIdx.x == 0) s_amax_val[16] = m;
  __syncthreads();
  return s_amax_val[16];
}
#endif

}  // namespace pvcnn
