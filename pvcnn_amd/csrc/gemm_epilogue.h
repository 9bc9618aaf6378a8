// gemm_epilogue.h -- the epilogue of the tile-per-workgroup MFMA GEMMs (conv3d_igemm_kernel, conv3d_igemm_bf16_kernel,
// conv3d_igemm_f16_pipe_kernel, pw_gemm_bf16_kernel, pw_gemm_f16_pipe_kernel).  pw_gemm_kernel (pointwise.hip) and the two persistent
// wide kernels keep texts of their own and follow the same contract.
#pragma once
#include "wave.h"
#include "split16.h"
#include <type_traits>

namespace pvcnn {

// A workgroup of four waves owns ROWS output rows (channels) x (4 / WM) column groups x NBW blocks of 32 columns (voxels / points);
// wave = wm + WM * wn holds the row blocks wm * MBW .. + MBW - 1 of column group wn.  C/D map of the 32x32 MFMAs: lane -> column
// j = lane & 31 of a block, register r -> row (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) of a 32-row block.  acc(mbl, nb, r) is the
// accumulator of the wave's row block mbl, column block nb; rows are row0 + ... < row_limit, yb[row * row_stride + col_off[nb]] is
// stored where col_ok[nb].  Per element, in this order:
//   v = acc (UNSCALE: * 2^-wexp[row] * 2^-x_shift -- powers of two, exact; wexp covers the padded rows of the tile);
//   statistics;  v += bias[row];  store.
// THE STATISTICS CONTRACT (stats_part != nullptr; what bn_finalize_kernel and the BatchNorm nodes rely on):
//   * they are the sum and the sum of squares of (y - bias), v BEFORE the bias is added: the shift keeps E[a^2] - E[a]^2 well
//     conditioned when the bias dwarfs the spread (bn_finalize adds it back);
//   * a masked column (!col_ok) contributes +0 to both;
//   * the order of the additions is fixed: a lane adds its column blocks nb = 0 .. NBW - 1, half_wave_sum16 adds the 32 lanes of a
//     block row (lane j ends up with the totals of register (j >> 1) & 15), the column groups meet in stat_lds[group][ROWS] and are
//     added group 0 first;
//   * one float2 (sum, sum of squares) per row < row_limit: stats_part[row * stats_stride + stats_slot], written by exactly one
//     workgroup -- the partials are combined by bn_finalize in fp64.
// stat_lds: (4 / WM) * ROWS float pairs of LDS that no wave reads any more (the caller's barrier); contains one __syncthreads().
//
// THE ACTIVATION TAIL (Tail = ActAmaxTail: the folded-inference products, whose BatchNorm sits in the weights).  Selected at compile
// time: with Tail = NoTail (every training instantiation) none of it exists.  Behind the bias:
//   v = v > 0 ? v : v * slope  (slope 0: ReLU);  store;
//   amax emission (table != nullptr): the consumer of y is another f16x2 product and scales its operand by y's amax buffer
//   (include/pvcnn_hip.h).  Of the STORED elements only (col_ok && row < row_limit) a lane keeps the largest |v| per column block (fmaxf: the
//   inputs are finite; a NaN would not be recorded), the lanes of the workgroup meet in one LDS word per position segment of the tile (seg_local(nb): the lane's segment
//   inside the tile, < nseg <= 256), and one vector atomicMax per (workgroup, segment) combines the row tiles in table[1 + seg_index(l)]
//   (seg_index(l) < 0: a segment of the tile outside the tensor).  Non-negative floats order like their bit patterns, so the result
//   does not depend on the order; the caller has zeroed the table.  Word [0] is never written (a table-only buffer).
//   The tail brings three barriers of its own and needs no barrier from the caller; every thread of the workgroup must arrive.
struct NoTail {};
template <class SegLocal, class SegIndex>
struct ActAmaxTail {
  float slope;
  uint32_t *table;
  int nseg;
  SegLocal seg_local;          // (column block nb) -> the lane's segment inside the tile; asked after the stores, not kept across them
  SegIndex seg_index;
};
template <class SegLocal, class SegIndex>
__device__ __forceinline__ ActAmaxTail<SegLocal, SegIndex> act_amax_tail(float slope, uint32_t *table, int nseg, SegLocal seg_local, SegIndex seg_index) {
  return ActAmaxTail<SegLocal, SegIndex>{slope, table, nseg, seg_local, seg_index};
}
// kernel arguments of the tail: nothing for the instantiations without it
template <bool ACT> struct ActArgs {};
template <> struct ActArgs<true> { float slope; uint32_t *amax; };
__device__ __forceinline__ float act_tail(float v, float slope) { return v > 0.0f ? v : v * slope; }
__device__ __forceinline__ uint32_t act_abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }
// segment l of a Conv3d tile = its z row (xt, yt) = (l / TY, l % TY)  ->  row (b, x0 + xt, y0 + yt) of the (B, R, R) table
template <int TY>
struct ZRowIndex {
  int b, R, x0, y0;
  __device__ __forceinline__ long operator()(int l) const {
    const int gx = x0 + l / TY, gy = y0 + l % TY;
    return (gx < R && gy < R) ? ((long)b * R + gx) * R + gy : -1L;
  }
};
// a 1x1 tile is one 256-point segment: the tile's index
struct TileIndex {
  long tile;
  __device__ __forceinline__ long operator()(int) const { return tile; }
};

template <bool UNSCALE, int MBW, int NBW, int WM, int ROWS, class Acc, class Off, class Tail = NoTail>
__device__ __forceinline__ void gemm_tile_epilogue(Acc acc, float *__restrict__ yb, size_t row_stride, const Off (&col_off)[NBW],
                                                   const bool (&col_ok)[NBW], int row0, int row_limit, const float *__restrict__ bias,
                                                   const int *__restrict__ wexp, int x_shift, float2 *__restrict__ stats_part,
                                                   size_t stats_stride, size_t stats_slot, float2 *stat_lds, const Tail &tail = Tail{}) {
  constexpr bool ACT = !std::is_same<Tail, NoTail>::value;
  [[maybe_unused]] float am[NBW];                              // max |v| of the lane's stored elements per column block
  if constexpr (ACT) {
#pragma unroll
    for (int nb = 0; nb < NBW; ++nb) am[nb] = 0.0f;
  }
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, kh = lane >> 5;
  const int wm = wave % WM, wn = wave / WM;
  const bool want_stats = stats_part != nullptr;
#pragma unroll
  for (int mbl = 0; mbl < MBW; ++mbl) {
    const int mb = wm * MBW + mbl;                              // 32-row block inside the workgroup tile
    float bv[16], unscale[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = row0 + mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
      bv[r] = (bias != nullptr && row < row_limit) ? bias[row] : 0.0f;
      if constexpr (UNSCALE) unscale[r] = exp2_int(-wexp[row]);
    }
    const float x_unscale = exp2_int(-x_shift);
    float ss[16], qq[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) ss[r] = qq[r] = 0.0f;
#pragma unroll
    for (int nb = 0; nb < NBW; ++nb) {
      float *__restrict__ col = yb + col_off[nb];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = row0 + mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        float v = acc(mbl, nb, r);
        if constexpr (UNSCALE) v = v * unscale[r] * x_unscale;
        if (want_stats) {
          const float m = col_ok[nb] ? v : 0.0f;
          ss[r] += m;
          qq[r] += m * m;
        }
        v += bv[r];
        if constexpr (ACT) {
          v = act_tail(v, tail.slope);
          if (col_ok[nb] && row < row_limit) am[nb] = fmaxf(am[nb], fabsf(v));
        }
        if (col_ok[nb] && row < row_limit) col[(size_t)row * row_stride] = v;
      }
    }
    if (want_stats) {
      const float st = half_wave_sum16(ss, j), qt = half_wave_sum16(qq, j);
      const int rr = (j >> 1) & 15;
      if ((j & 1) == 0) stat_lds[wn * ROWS + mb * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * kh] = make_float2(st, qt);
    }
  }
  if (want_stats) {
    __syncthreads();
    if (tid < ROWS && row0 + tid < row_limit) {
      float2 t = stat_lds[tid];
#pragma unroll
      for (int w = 1; w < 4 / WM; ++w) { t.x += stat_lds[w * ROWS + tid].x; t.y += stat_lds[w * ROWS + tid].y; }
      stats_part[(size_t)(row0 + tid) * stats_stride + stats_slot] = t;
    }
  }
  if constexpr (ACT) {
    if (tail.table != nullptr) {                                // (uniform: a kernel argument)
      uint32_t *amax_lds = reinterpret_cast<uint32_t *>(stat_lds);
      __syncthreads();                                          // the tile / the statistics in this LDS have been read
      if (tid < tail.nseg) amax_lds[tid] = 0u;
      __syncthreads();
#pragma unroll
      for (int nb = 0; nb < NBW; ++nb) {
        const uint32_t mine = __float_as_uint(am[nb]);
        const uint32_t m = max(mine, (uint32_t)__shfl_xor((int)mine, 32));         // the two row halves of the lane's column
        if (kh == 0 && m != 0u) atomicMax(&amax_lds[tail.seg_local(nb)], m);       // (m != 0: the column was stored)
      }
      __syncthreads();
      if (tid < tail.nseg) {
        const uint32_t m = amax_lds[tid];
        int l = tid;
        asm volatile("" : "+v"(l));                             // (derived here: hoisted to the kernel's start, l / TY costs the 256-register tiles a spill)
        const long t = tail.seg_index(l);
        if (m != 0u && t >= 0) atomicMax(tail.table + 1 + t, m);
      }
    }
  }
}

}  // namespace pvcnn
