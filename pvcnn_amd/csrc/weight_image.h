// weight_image.h -- the split-weight image: the pre-split, pre-swizzled weights the f16x2 / bf16 / bf16x3 GEMM kernels of
// conv3d_bf16.hip and pointwise_bf16.hip read.  The ABI calls it opaque (include/pvcnn_hip.h); this header is the ONE statement of its
// format -- geometry, swizzle, writers, refresh kernels and the host side of the fourteen pvcnn_*_weight_split* entries.
//
// A weight becomes a matrix of `rows` output rows x `depth` reduction channels x taps (forward: rows = Co, depth = Ci; backward-data:
// the transposed, tap-flipped weight, rows = Ci, depth = Co).  The image is nsplit planes of 16-bit pieces (split16.h) in the order
//     [chunk of 16 reduction channels][dxy][row tile][dz][plane][row of the tile][16 channels]
// with rows and depth zero-padded to whole tiles and chunks, so one (chunk, dxy, row tile) block is what a workgroup streams per
// (dx, dy) and one (dz, plane) slab of it is an MFMA A operand.  Inside a 16-channel row the two 8-channel halves are swapped in rows
// with bit 3 set (image_half_word): the 16-byte fragment reads of 32 consecutive rows then hit distinct banks.  An f16x2 image
// (nsplit 2) is followed by one int32 power-of-two shift per padded row (scale_shift of the row's largest magnitude).
//
// What differs between the two kinds is in the descriptors ConvImage and PwImage; everything else is written once, on them.
// The geometry part is plain C++ (constexpr: host and device); the writers, kernels and host entries need hipcc.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "route.h"

namespace pvcnn {

constexpr int kImageK = 16;        // reduction channels per chunk = MFMA K = elements of an image row

// Conv3d: 27 taps, a block per (dx, dy) holding the three dz taps; 64-row tiles.  w is (Co, Ci, 27).
struct ConvImage {
  static constexpr const char *kOp = "conv3d";
  static constexpr int kDxy = 9, kDz = 3;
  static constexpr int row_tile(int /* rows */) { return route::kCoTileB; }
  // backward-data computes grad_x = conv(grad_y, w') with w'[ci][co][tap] = w[co][ci][26 - tap]
  static constexpr size_t source(int Ci, int row, int k, int tap, bool bwd) {
    return bwd ? ((size_t)k * Ci + row) * 27 + (26 - tap) : ((size_t)row * Ci + k) * 27 + tap;
  }
  static constexpr long long entry_tm(int /* tile_f */, int /* tile_b */) { return 0; }
};

// 1x1: one tap; the row tile is the GEMM's, 64 or 128 rows by the row count (route.h: pb_mb).  w is (Co, Ci).
struct PwImage {
  static constexpr const char *kOp = "pwconv";
  static constexpr int kDxy = 1, kDz = 1;
  static constexpr int row_tile(int rows) { return 32 * route::pb_mb(rows); }
  static constexpr size_t source(int Ci, int row, int k, int /* tap */, bool bwd) {
    return bwd ? (size_t)k * Ci + row : (size_t)row * Ci + k;
  }
  // (SplitEntry::tm, pinned by the ABI; the kernels take both tiles from the row counts)
  static constexpr long long entry_tm(int tile_f, int tile_b) { return (long long)tile_f | ((long long)tile_b << 32); }
};

// 32-bit word, inside an image row (8 words), at which the 8-channel half `h` of row `row` starts
constexpr int image_half_word(int row, int h) { return (h ^ ((row >> 3) & 1)) * 4; }
// elements of one (dz, plane) slab and of one (chunk, dxy, row tile) block
constexpr int image_slab(int tile) { return tile * kImageK; }
template <class K>
constexpr int image_block(int nsplit, int tile) { return K::kDz * nsplit * image_slab(tile); }

template <class K>
struct ImageGeom {
  int depth, rows;                 // reduction channels and output rows of THIS image
  int tile, chunks, tiles;
  constexpr ImageGeom(int Co, int Ci, bool bwd)
      : depth(bwd ? Co : Ci), rows(bwd ? Ci : Co), tile(K::row_tile(rows)), chunks(route::ceil_div(depth, kImageK)),
        tiles(route::ceil_div(rows, tile)) {}
  constexpr int padded_rows() const { return tiles * tile; }       // = workgroups of an f16x2 refresh, entries of the shift table
  constexpr long elems() const { return (long)chunks * K::kDxy * tiles * K::kDz * image_slab(tile); }      // of one plane
  constexpr long bf16_blocks() const { return (elems() + 255) / 256; }                                     // workgroups of a bf16 / bf16x3 refresh
  constexpr size_t image_bytes(int nsplit) const { return (size_t)elems() * nsplit * sizeof(uint16_t); }
  constexpr size_t total_bytes(int nsplit) const { return image_bytes(nsplit) + (nsplit == 2 ? padded_rows() * sizeof(int) : 0); }
  // the shift table of an f16x2 image
  int *shifts(void *wts) const { return reinterpret_cast<int *>(static_cast<char *>(wts) + image_bytes(2)); }
  const int *shifts(const void *wts) const { return shifts(const_cast<void *>(wts)); }
  // element offset of reduction channel k (0 .. 15 of the chunk) of a row
  constexpr size_t at(int nsplit, int chunk, int dxy, int ti, int dz, int plane, int row, int k) const {
    return (((size_t)chunk * K::kDxy + dxy) * tiles + ti) * image_block<K>(nsplit, tile) + ((size_t)(dz * nsplit + plane) * tile + row) * kImageK +
           2 * image_half_word(row, k >> 3) + (k & 7);
  }
};

}  // namespace pvcnn

#ifdef __HIPCC__
#include <stdio.h>
#include <string.h>

#include "common.h"
#include "split16.h"
#include "wave.h"

namespace pvcnn {

// ---- device writers -----------------------------------------------------------------------------------------------------------------

// f16x2: one workgroup per (padded) row m finds the row's largest magnitude, writes the shift and the row's hi / lo planes, as
// channel pairs (one word per plane)
template <class K>
__device__ __forceinline__ void weight_split_f16_row(const float *__restrict__ w, int Co, int Ci, int bwd, uint16_t *__restrict__ wts,
                                                     int *__restrict__ wexp, int m) {
  constexpr int kTaps = K::kDxy * K::kDz;
  const ImageGeom<K> g(Co, Ci, bwd);
  const int ti = m / g.tile, row = m - ti * g.tile, tid = threadIdx.x;
  auto load = [&](int k, int tap) { return w[K::source(Ci, m, k, tap, bwd)]; };
  __shared__ uint32_t red[4];
  uint32_t mx = 0;
  if (m < g.rows)
    for (int i = tid; i < g.depth * kTaps; i += 256) mx = max(mx, __float_as_uint(fabsf(load(i / kTaps, i % kTaps))));
  mx = wave_max(mx);
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  const int shift = scale_shift(max(max(red[0], red[1]), max(red[2], red[3])));
  if (tid == 0) wexp[m] = shift;
  const float scale = exp2_int(shift);
  uint32_t *img = reinterpret_cast<uint32_t *>(wts);
  for (int i = tid; i < g.chunks * kTaps * 8; i += 256) {          // item = (chunk, tap, channel pair)
    const int cp = i & 7, tap = (i >> 3) % kTaps, chunk = (i >> 3) / kTaps;
    const int k = chunk * kImageK + 2 * cp, dxy = tap / K::kDz, dz = tap - dxy * K::kDz;
    const float a = (m < g.rows && k < g.depth) ? load(k, tap) * scale : 0.0f;
    const float b = (m < g.rows && k + 1 < g.depth) ? load(k + 1, tap) * scale : 0.0f;
    uint32_t p[2];
    split_pair<2>(a, b, p);
#pragma unroll
    for (int s = 0; s < 2; ++s) img[g.at(2, chunk, dxy, ti, dz, s, row, 2 * cp) >> 1] = p[s];
  }
}

// bf16 / bf16x3: one thread per element e = (chunk, dxy, row tile, dz, row, k) of a plane writes its NS pieces
template <class K, int NS>
__device__ __forceinline__ void weight_split_elem(const float *__restrict__ w, int Co, int Ci, int bwd, uint16_t *__restrict__ wts, long e) {
  const ImageGeom<K> g(Co, Ci, bwd);
  if (e >= g.elems()) return;
  const int k_l = (int)(e % kImageK), row = (int)((e / kImageK) % g.tile);
  long rest = e / ((long)kImageK * g.tile);
  const int dz = (int)(rest % K::kDz); rest /= K::kDz;
  const int ti = (int)(rest % g.tiles); rest /= g.tiles;
  const int dxy = (int)(rest % K::kDxy), chunk = (int)(rest / K::kDxy);
  const int k = chunk * kImageK + k_l, m = ti * g.tile + row;
  const float v = (k < g.depth && m < g.rows) ? w[K::source(Ci, m, k, dxy * K::kDz + dz, bwd)] : 0.0f;
  uint32_t p[NS];
  split_bf16<NS>(v, p);
#pragma unroll
  for (int s = 0; s < NS; ++s) wts[g.at(NS, chunk, dxy, ti, dz, s, row, k_l)] = (uint16_t)p[s];
}

// ---- kernels: one image; the forward AND backward-data image of one weight (a training step needs both; the weights do not change in
// between); ... of EVERY registered weight of a model (SplitEntry, common.h: one launch per kind and optimizer step) ------------------

template <class K>
__global__ __launch_bounds__(256) void weight_split_f16_kernel(const float *__restrict__ w, int Co, int Ci, int bwd, uint16_t *__restrict__ wts,
                                                               int *__restrict__ wexp) {
  weight_split_f16_row<K>(w, Co, Ci, bwd, wts, wexp, blockIdx.x);
}

template <class K>
__global__ __launch_bounds__(256) void weight_split_f16_pair_kernel(const float *__restrict__ w, int Co, int Ci, int rows_fwd,
                                                                    uint16_t *__restrict__ wts_f, int *__restrict__ wexp_f,
                                                                    uint16_t *__restrict__ wts_b, int *__restrict__ wexp_b) {
  if ((int)blockIdx.x < rows_fwd) weight_split_f16_row<K>(w, Co, Ci, 0, wts_f, wexp_f, blockIdx.x);
  else weight_split_f16_row<K>(w, Co, Ci, 1, wts_b, wexp_b, blockIdx.x - rows_fwd);
}

template <class K>
__global__ __launch_bounds__(256) void weight_split_f16_batch_kernel(const SplitEntry *__restrict__ tab, int n) {
  const SplitEntry e = split_entry_of(tab, n, blockIdx.x);
  const int row = (int)(blockIdx.x - e.row_begin);
  if (row < (int)e.rows_f) weight_split_f16_row<K>(e.w, (int)e.Co, (int)e.Ci, 0, e.wts_f, e.wexp_f, row);
  else weight_split_f16_row<K>(e.w, (int)e.Co, (int)e.Ci, 1, e.wts_b, e.wexp_b, row - (int)e.rows_f);
}

template <class K, int NS>
__global__ __launch_bounds__(256) void weight_split_kernel(const float *__restrict__ w, int Co, int Ci, int bwd, uint16_t *__restrict__ wts) {
  weight_split_elem<K, NS>(w, Co, Ci, bwd, wts, (long)blockIdx.x * 256 + threadIdx.x);
}

// the plain-bf16 (torch.autocast) pairs: an entry's rows are 256-element blocks here, rows_f of the forward image first; no shifts
template <class K>
__global__ __launch_bounds__(256) void weight_split_bf16_batch_kernel(const SplitEntry *__restrict__ tab, int n) {
  const SplitEntry e = split_entry_of(tab, n, blockIdx.x);
  const long local = (long)(blockIdx.x - e.row_begin);
  if (local < (long)e.rows_f) weight_split_elem<K, 1>(e.w, (int)e.Co, (int)e.Ci, 0, e.wts_f, local * 256 + threadIdx.x);
  else weight_split_elem<K, 1>(e.w, (int)e.Co, (int)e.Ci, 1, e.wts_b, (local - (long)e.rows_f) * 256 + threadIdx.x);
}

// ---- host side of pvcnn_<K::kOp>_weight_split<entry> (the extern "C" functions are one-line calls; errors carry their names) ---------

#define PVCNN_IMAGE_REQUIRE(entry, cond, msg)                                    \
  do {                                                                           \
    if (!(cond)) {                                                               \
      set_error("pvcnn_%s_weight_split%s: %s", K::kOp, entry, msg);              \
      return PVCNN_ERR_INVALID_ARGUMENT;                                         \
    }                                                                            \
  } while (0)

template <class K>
int image_check_launch(const char *entry) {
  char what[64];
  snprintf(what, sizeof(what), "%s_weight_split%s", K::kOp, entry);
  return check_launch(what);
}

// nsplit: 1 = bf16, 3 = bf16x3, 2 = f16x2 (image followed by one int32 shift per padded row)
template <class K>
size_t weight_split_bytes(int Co, int Ci, int bwd, int nsplit) {
  if (Co <= 0 || Ci <= 0 || nsplit < 1 || nsplit > 3) return 0;
  return ImageGeom<K>(Co, Ci, bwd).total_bytes(nsplit);
}

template <class K>
int weight_split(const float *w, int Co, int Ci, int bwd, int nsplit, void *wts, void *stream) {
  PVCNN_IMAGE_REQUIRE("", w && wts && Co > 0 && Ci > 0, "bad argument");
  PVCNN_IMAGE_REQUIRE("", nsplit >= 1 && nsplit <= 3, "nsplit must be 1 (bf16), 2 (f16x2) or 3 (bf16x3)");
  PVCNN_IMAGE_REQUIRE("", aligned16(wts), "wts must be 16-byte aligned");
  const ImageGeom<K> g(Co, Ci, bwd);
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint16_t *img = static_cast<uint16_t *>(wts);
  if (nsplit == 2) {
    hipLaunchKernelGGL(weight_split_f16_kernel<K>, dim3(g.padded_rows()), dim3(256), 0, s, w, Co, Ci, bwd, img, g.shifts(wts));
    return image_check_launch<K>("_f16");
  }
  const dim3 grid((unsigned)g.bf16_blocks());
  if (nsplit == 1) hipLaunchKernelGGL((weight_split_kernel<K, 1>), grid, dim3(256), 0, s, w, Co, Ci, bwd, img);
  else             hipLaunchKernelGGL((weight_split_kernel<K, 3>), grid, dim3(256), 0, s, w, Co, Ci, bwd, img);
  return image_check_launch<K>("");
}

// both f16x2 images of w in one launch; buffers sized by weight_split_bytes(.., 0 / 1, 2)
template <class K>
int weight_split_pair(const float *w, int Co, int Ci, void *wts_fwd, void *wts_bwd, void *stream) {
  PVCNN_IMAGE_REQUIRE("_pair", w && wts_fwd && wts_bwd && Co > 0 && Ci > 0, "bad argument");
  PVCNN_IMAGE_REQUIRE("_pair", aligned16(wts_fwd) && aligned16(wts_bwd), "images must be 16-byte aligned");
  const ImageGeom<K> f(Co, Ci, false), b(Co, Ci, true);
  hipLaunchKernelGGL(weight_split_f16_pair_kernel<K>, dim3(f.padded_rows() + b.padded_rows()), dim3(256), 0, static_cast<hipStream_t>(stream), w,
                     Co, Ci, f.padded_rows(), static_cast<uint16_t *>(wts_fwd), f.shifts(wts_fwd), static_cast<uint16_t *>(wts_bwd),
                     b.shifts(wts_bwd));
  return image_check_launch<K>("_pair");
}

// batched form of weight_split_pair: `entry` (host, 10 int64) describes one weight and its two image buffers (nsplit 2: f16x2; 1: plain
// bf16) and returns the number of workgroups it takes; the caller sets word [9] (row_begin) to the running sum and copies the table to
// the device.
template <class K>
long weight_split_pair_entry(const float *w, int Co, int Ci, void *wts_fwd, void *wts_bwd, long long *entry, int nsplit) {
  if (!w || !wts_fwd || !wts_bwd || !entry || Co <= 0 || Ci <= 0 || !aligned16(wts_fwd) || !aligned16(wts_bwd)) return -1;
  const ImageGeom<K> f(Co, Ci, false), b(Co, Ci, true);
  const bool f16 = nsplit == 2;
  SplitEntry e;
  e.w = w;
  e.wts_f = static_cast<uint16_t *>(wts_fwd); e.wexp_f = f16 ? f.shifts(wts_fwd) : nullptr;
  e.wts_b = static_cast<uint16_t *>(wts_bwd); e.wexp_b = f16 ? b.shifts(wts_bwd) : nullptr;
  e.Co = Co; e.Ci = Ci; e.rows_f = f16 ? f.padded_rows() : f.bf16_blocks(); e.tm = K::entry_tm(f.tile, b.tile); e.row_begin = 0;
  memcpy(entry, &e, sizeof(e));
  return (long)e.rows_f + (f16 ? b.padded_rows() : b.bf16_blocks());
}

template <class K>
int weight_split_pair_batch(const void *table, int n, long total_rows, void *stream, int nsplit) {
  const char *entry = nsplit == 2 ? "_pair_batch" : "_pair_batch_bf16";
  PVCNN_IMAGE_REQUIRE(entry, n >= 0 && total_rows >= 0 && total_rows <= 0x7fffffffL, "bad size");
  if (n == 0 || total_rows == 0) return 0;
  PVCNN_IMAGE_REQUIRE(entry, table && (reinterpret_cast<uintptr_t>(table) & 7) == 0, "null or misaligned table");
  auto kernel = nsplit == 2 ? weight_split_f16_batch_kernel<K> : weight_split_bf16_batch_kernel<K>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)total_rows), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const SplitEntry *>(table), n);
  return image_check_launch<K>(entry);
}

#undef PVCNN_IMAGE_REQUIRE

}  // namespace pvcnn
#endif  // __HIPCC__
