// split16.h -- fp32 operands as 16-bit pieces for the bf16 / fp16 matrix cores (shared by the conv3d / pointwise *_bf16.hip and
// *_wgrad_f16.hip units; the arithmetic is described at the top of conv3d_bf16.hip).
#pragma once
#include "common.h"

namespace pvcnn {

using f32x16 = __attribute__((ext_vector_type(16))) float;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// round-to-nearest-even fp32 -> bf16 (bits); inputs are finite in this path
__device__ __forceinline__ uint32_t bf16_bits(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
// v -> NS bf16 pieces with v = p0 + p1 + p2 (exactly, up to the last piece's rounding at 2^-24 |v|)
template <int NS>
__device__ __forceinline__ void split_bf16(float v, uint32_t (&p)[NS]) {
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    p[s] = bf16_bits(v);
    if (s + 1 < NS) v = v - __uint_as_float(p[s] << 16);         // exact: the residual fits fp32
  }
}

// Two neighbouring channels at once, packed (first value in the low half): v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32 round to nearest
// even in hardware.  NS = 1, 3: bf16 pieces as in split_bf16.  NS = 2: fp16 "hi + lo" of PRE-SCALED values (|v| < 2^15, see
// scale_shift): hi = fp16(v) keeps 11 bits, lo = fp16(v - hi) the next 11.
template <int NS>
__device__ __forceinline__ void split_pair(float a, float b, uint32_t (&w)[NS]) {
  f32x2 v = {a, b};
  if constexpr (NS == 2) {
    const f16x2 h = __builtin_convertvector(v, f16x2);
    w[0] = __builtin_bit_cast(uint32_t, h);
    v = v - __builtin_convertvector(h, f32x2);                   // exact
    w[1] = __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2));
  } else {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      w[s] = __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
      if (s + 1 < NS) {
        const f32x2 back = {__uint_as_float(w[s] << 16), __uint_as_float(w[s] & 0xffff0000u)};
        v = v - back;                                            // exact: the residual fits fp32
      }
    }
  }
}

// fp16 has 5 exponent bits: operands of the f16x2 mode are scaled by a power of two that puts the largest magnitude of the
// tensor (bits of max |x|, from absmax_kernel; of a weight row, in the split kernel) into [2^13, 2^14).  Everything within
// 2^-17 of the maximum then keeps 22 bits in hi + lo; smaller elements lose low bits gradually (absolute error <= 2^-38 of
// the maximum).  Zero / inf / NaN maxima: no scaling (inf and NaN then propagate as they would in fp32).
__device__ __forceinline__ int scale_shift(uint32_t absmax_bits) {
  const int e = (int)((absmax_bits >> 23) & 0xffu);
  if (e == 0 || e == 255) return 0;
  return min(max(140 - e, -100), 100);                           // 13 - (e - 127)
}
__device__ __forceinline__ float exp2_int(int s) { return __uint_as_float((uint32_t)(s + 127) << 23); }

template <int NS>
__device__ __forceinline__ f32x16 mfma16(const uint4 &a, const uint4 &b, const f32x16 &c) {
  if constexpr (NS == 2) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// One 16-deep k-step of a wave's MBW x NBW tiles on split operands: plane 0 is the leading piece.  NS = 1: one product; NS = 2
// (f16x2): lo x hi, hi x lo, then hi x hi; NS = 3 (bf16x3): the six partial products >= 2^-16 of the leading one, smallest first.
// Consecutive MFMAs go to different accumulators (MBW * NBW independent tiles between two partial products of one tile).  Every
// kernel that shares this ladder adds the same products in the same order per output element: the cross-kernel bit-identity
// tests rest on it (the two persistent wide kernels spell the same order out in their pinned slots).
template <int NS, int MBW, int NBW>
__device__ __forceinline__ void split_products(f32x16 (&acc)[MBW][NBW], const uint4 (&af)[MBW][NS], const uint4 (&bf)[NBW][NS]) {
  auto product = [&](int sa, int sb) {
#pragma unroll
    for (int nb = 0; nb < NBW; ++nb)
#pragma unroll
      for (int mb = 0; mb < MBW; ++mb) acc[mb][nb] = mfma16<NS>(af[mb][sa], bf[nb][sb], acc[mb][nb]);
  };
  if constexpr (NS == 1) {
    product(0, 0);
  } else if constexpr (NS == 2) {
    product(1, 0); product(0, 1);
    product(0, 0);
  } else {
    product(2, 0); product(1, 1); product(0, 2);
    product(1, 0); product(0, 1);
    product(0, 0);
  }
}

}  // namespace pvcnn
