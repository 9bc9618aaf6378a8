// rooms.hip -- S3DIS room preparation on the device: a raw scan (N, 6) fp64 -> blocks, merged blocks, resampled cells, windows,
// packed rows, labels and indices_split_to_full.
//
// Reference: data/s3dis/prepare_data.py:119-282 (numpy, one Python loop iteration per occupied grid cell).  Here every step is a
// launch over points, cells, blocks or entries on the caller's stream.  The two orderings (points by (merged block, cell key), entries
// by (block, shuffle key)) are sorts the host does between the calls; every VALUE is computed here:
//   * all fp64 expressions in the reference's order of operations, one rounding each (the translation unit is built with
//     -ffp-contract=off: no multiply-add is ever fused across them);
//   * int(mean(counts)) and ceil(avg / c) as integer floor / ceiling divisions (exact below 2^31);
//   * minima through integer atomicMin on the bit pattern (shifted coordinates are >= +0.0, where the bits order like the value),
//     counts through integer atomicAdd: no float atomics, every table is order-free and two runs are bit-identical;
//   * the draws from Philox4x32-10 (philox.h) keyed by two int64 words in device memory.
// Shifted coordinate of axis a: p[a] - extent[a] (prepare_data.py:120); the room's minimum is then exactly 0 and its maximum
// extent[3 + a] - extent[a] (max_room_*), because the subtraction is monotone.
#include <algorithm>

#include "wave.h"
#include "philox.h"

namespace pvcnn {

constexpr int kRoomThreads = 256;
constexpr int kRoomScanTile = 4 * kRoomThreads;          // items one workgroup scans
constexpr long long kRoomMaxPoints = 1ll << 29;          // entries <= 2 N stay below 2^31
constexpr long long kRoomMaxBlocks = 1ll << 24;          // dense (bx, by) table
constexpr int kRoomCellBits = 21;                        // per-axis cell index inside a merged block
constexpr long long kRoomLaneCopies = 2048;              // c * r up to here: one lane per cell; above: one workgroup per cell
constexpr int kRoomLdsBlocks = 1024;                     // block tables up to here are privatised in LDS: one global atomic per
                                                         // (workgroup, touched block) instead of one per point
constexpr unsigned long long kRoomInfBits = 0x7FF0000000000000ull;
constexpr uint32_t kStreamLane = 0x524f4f31u, kStreamBig = 0x524f4f32u, kStreamShuffle = 0x524f4f33u;
// status words
enum { kStCells = 0, kStEntries = 1, kStWindows = 2, kStError = 3, kStBigCells = 4, kStWords = 5 };
enum { kErrBlockRange = 1, kErrCellRange = 2 };

inline unsigned room_grid(long long n) {
  return (unsigned)std::min<long long>(std::max<long long>((n + kRoomThreads - 1) / kRoomThreads, 1), 4096);
}
inline long long scan_parts(long long n) { return (n + kRoomScanTile - 1) / kRoomScanTile; }

#define ROOM_FOR(i, n) for (long long i = (long long)blockIdx.x * kRoomThreads + threadIdx.x; i < (n); i += (long long)gridDim.x * kRoomThreads)

// ---- workgroup helpers (256 threads) ------------------------------------------------------------------------------------------------
// exclusive prefix of v over the workgroup; total = the workgroup's sum (two barriers)
__device__ __forceinline__ long long wg_exscan(long long v, long long &total) {
  __shared__ long long s_wave[kRoomThreads / kWave];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long x = wave_inclusive_scan(v, lane);
  __syncthreads();                                         // the previous call's readers are done
  if (lane == kWave - 1) s_wave[w] = x;
  __syncthreads();
  long long base = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < kRoomThreads / kWave; ++i) {
    if (i < w) base += s_wave[i];
    total += s_wave[i];
  }
  return base + x - v;
}

// ---- exclusive scan of n ints: reduce tiles, scan the tile sums in one workgroup, apply -----------------------------------------------
__global__ __launch_bounds__(kRoomThreads) void room_scan_reduce_kernel(const int *__restrict__ in, long long n, int *__restrict__ part) {
  const long long base = (long long)blockIdx.x * kRoomScanTile + threadIdx.x * 4;
  long long s = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (base + q < n) s += in[base + q];
  long long total;
  wg_exscan(s, total);
  if (threadIdx.x == 0) part[blockIdx.x] = (int)total;
}

__global__ __launch_bounds__(kRoomThreads) void room_scan_parts_kernel(int *part, long long np, int *total_out) {
  long long carry = 0;
  for (long long b = 0; b < np; b += kRoomThreads) {
    const long long i = b + threadIdx.x;
    const long long v = i < np ? part[i] : 0;
    long long total;
    const long long ex = wg_exscan(v, total);
    if (i < np) part[i] = (int)(carry + ex);
    carry += total;
  }
  if (threadIdx.x == 0 && total_out != nullptr) *total_out = (int)carry;
}

__global__ __launch_bounds__(kRoomThreads) void room_scan_apply_kernel(const int *in, long long n, const int *__restrict__ part, int *out) {
  const long long base = (long long)blockIdx.x * kRoomScanTile + threadIdx.x * 4;
  int v[4];
  long long s = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    v[q] = base + q < n ? in[base + q] : 0;
    s += v[q];
  }
  long long total;
  long long ex = wg_exscan(s, total) + part[blockIdx.x];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (base + q < n) out[base + q] = (int)ex;
    ex += v[q];
  }
}

// out[i] = sum of in[0 .. i) (in == out allowed); *total = sum of all.  part: scan_parts(n) ints of scratch.
static int room_scan(const int *in, int *out, long long n, int *total, int *part, hipStream_t s) {
  const long long np = scan_parts(n);
  hipLaunchKernelGGL(room_scan_reduce_kernel, dim3((unsigned)np), dim3(kRoomThreads), 0, s, in, n, part);
  hipLaunchKernelGGL(room_scan_parts_kernel, dim3(1), dim3(kRoomThreads), 0, s, part, np, total);
  hipLaunchKernelGGL(room_scan_apply_kernel, dim3((unsigned)np), dim3(kRoomThreads), 0, s, in, n, part, out);
  return check_launch("room_scan");
}

// ---- step 1: room extent, two stages ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ void extent_fold(double (&lo)[3], double (&hi)[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double l = __shfl_xor(lo[a], o), h = __shfl_xor(hi[a], o);
      lo[a] = l < lo[a] ? l : lo[a];
      hi[a] = h > hi[a] ? h : hi[a];
    }
}

// rows of `stride` doubles; part (gridDim.x, 6); stage 2 runs it with one workgroup over the partial rows (lo from columns 0..2, hi from 3..5)
__global__ __launch_bounds__(kRoomThreads) void room_extent_kernel(const double *__restrict__ src, long long n, int stride, int hi_col,
                                                                  double *__restrict__ part) {
  __shared__ double s_lo[kRoomThreads / kWave][3], s_hi[kRoomThreads / kWave][3];
  double lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = __builtin_inf();
    hi[a] = -__builtin_inf();
  }
  ROOM_FOR(i, n) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double l = src[i * stride + a], h = src[i * stride + hi_col + a];
      lo[a] = l < lo[a] ? l : lo[a];
      hi[a] = h > hi[a] ? h : hi[a];
    }
  }
  extent_fold(lo, hi);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      s_lo[w][a] = lo[a];
      s_hi[w][a] = hi[a];
    }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int a = threadIdx.x;
    double l = s_lo[0][a], h = s_hi[0][a];
    for (int i = 1; i < kRoomThreads / kWave; ++i) {
      l = s_lo[i][a] < l ? s_lo[i][a] : l;
      h = s_hi[i][a] > h ? s_hi[i][a] : h;
    }
    part[(long long)blockIdx.x * 6 + a] = l;
    part[(long long)blockIdx.x * 6 + 3 + a] = h;
  }
}

// ---- step 2: block keys and counts ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double shifted(const double *__restrict__ xyzrgb, long long i, int a, const double *__restrict__ ext) {
  return xyzrgb[i * 6 + a] - ext[a];
}

__global__ __launch_bounds__(kRoomThreads) void room_block_keys_kernel(const double *__restrict__ xyzrgb, long long n,
                                                                      const double *__restrict__ ext, double offset, double block_size,
                                                                      int gx, int gy, int *__restrict__ point_block, int *block_count,
                                                                      int *status) {
  __shared__ int s_count[kRoomLdsBlocks];
  const int G = gx * gy;
  const bool lds = G <= kRoomLdsBlocks;
  if (lds) {
    for (int g = threadIdx.x; g < G; g += kRoomThreads) s_count[g] = 0;
    __syncthreads();
  }
  const double min_o = 0.0 - offset;                       // amin(xyz) - offset of the shifted room
  ROOM_FOR(i, n) {
    const double fx = floor((shifted(xyzrgb, i, 0, ext) - min_o) / block_size);
    const double fy = floor((shifted(xyzrgb, i, 1, ext) - min_o) / block_size);
    long long bx = (long long)fx, by = (long long)fy;
    if (!(fx >= 0.0 && fx < (double)gx && fy >= 0.0 && fy < (double)gy)) {   // (also NaN) cannot happen for finite input: the host sized
      atomicOr(status + kStError, kErrBlockRange);                           // the table from the same expressions
      bx = by = 0;
    }
    const int key = (int)(bx * gy + by);                   // lexicographic (bx, by): np.unique(axis=0)'s block order
    point_block[i] = key;
    atomicAdd(lds ? s_count + key : block_count + key, 1);
  }
  if (lds) {
    __syncthreads();
    for (int g = threadIdx.x; g < G; g += kRoomThreads)
      if (s_count[g] != 0) atomicAdd(block_count + g, s_count[g]);
  }
}

// ---- step 3: the merge map, one lane per block (every decision reads the ORIGINAL counts) -----------------------------------------------
__global__ __launch_bounds__(kRoomThreads) void room_merge_kernel(const int *__restrict__ block_count, int gx, int gy, int max_num_points,
                                                                 int *__restrict__ block_target, int *__restrict__ occupied) {
  const long long G = (long long)gx * gy;
  ROOM_FOR(g, G) {
    const int cnt = block_count[g];
    int target = (int)g;
    // count < max_num_points / 10  <=>  10 * count < max_num_points (count is an integer)
    if (cnt > 0 && 10ll * cnt < max_num_points) {
      const int bx = (int)(g / gy), by = (int)(g % gy);
      // the neighbours (0,1) (1,0) (0,-1) (-1,0) (-1,1) (1,1) (1,-1) (-1,-1), each offset + 1 in two bits (no indexed local array)
      constexpr unsigned kDx = 0x2819u, kDy = 0x0A46u;
      for (int k = 0; k < 8; ++k) {
        const int nx = bx + (int)((kDx >> (2 * k)) & 3u) - 1, ny = by + (int)((kDy >> (2 * k)) & 3u) - 1;
        if (nx < 0 || nx >= gx || ny < 0 || ny >= gy) continue;
        const int c2 = block_count[(long long)nx * gy + ny];
        if (c2 > 0 && 10ll * c2 >= max_num_points) {
          target = nx * gy + ny;
          break;
        }
      }
    }
    block_target[g] = target;
    occupied[g] = cnt > 0 ? 1 : 0;
  }
}

// ---- step 4a: merged block of every point, per-block minimum, cell keys ----------------------------------------------------------------
__global__ __launch_bounds__(kRoomThreads) void room_fill_u64_kernel(unsigned long long *p, long long n, unsigned long long v) {
  ROOM_FOR(i, n) p[i] = v;
}

__global__ __launch_bounds__(kRoomThreads) void room_block_min_kernel(const double *__restrict__ xyzrgb, long long n,
                                                                     const double *__restrict__ ext, long long G,
                                                                     const int *__restrict__ block_target, int *point_block,
                                                                     unsigned long long *block_min) {
  __shared__ unsigned long long s_min[3 * kRoomLdsBlocks];
  const bool lds = G <= kRoomLdsBlocks;
  if (lds) {
    for (int k = threadIdx.x; k < 3 * (int)G; k += kRoomThreads) s_min[k] = kRoomInfBits;
    __syncthreads();
  }
  ROOM_FOR(i, n) {
    int g = point_block[i];
    g = (g >= 0 && g < G) ? block_target[g] : 0;
    g = (g >= 0 && g < G) ? g : 0;
    point_block[i] = g;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double v = shifted(xyzrgb, i, a, ext);
      if (v >= 0.0) atomicMin(lds ? s_min + g * 3 + a : block_min + (long long)g * 3 + a, (unsigned long long)__double_as_longlong(v + 0.0));
    }
  }
  if (lds) {
    __syncthreads();
    for (int k = threadIdx.x; k < 3 * (int)G; k += kRoomThreads)
      if (s_min[k] != kRoomInfBits) atomicMin(block_min + k, s_min[k]);
  }
}

__global__ __launch_bounds__(kRoomThreads) void room_cell_keys_kernel(const double *__restrict__ xyzrgb, long long n,
                                                                     const double *__restrict__ ext, double grid_size,
                                                                     const int *__restrict__ point_block,
                                                                     const unsigned long long *__restrict__ block_min,
                                                                     long long *__restrict__ cell_key, int *status) {
  ROOM_FOR(i, n) {
    const int g = point_block[i];
    long long key = 0;
    bool bad = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double bmin = __longlong_as_double((long long)block_min[(long long)g * 3 + a]);
      const double f = floor((shifted(xyzrgb, i, a, ext) - bmin) / grid_size);
      if (!(f >= 0.0 && f < (double)(1 << kRoomCellBits))) bad = true;
      key = (key << kRoomCellBits) | (bad ? 0ll : (long long)f);
    }
    if (bad) atomicOr(status + kStError, kErrCellRange);
    cell_key[i] = key;
  }
}

// ---- step 4b / 5: cells, averages, output counts, windows (points are sorted by (merged block, cell key)) -----------------------------------
__global__ __launch_bounds__(kRoomThreads) void room_heads_kernel(const int *__restrict__ sb, const long long *__restrict__ sk, long long n,
                                                                 int *__restrict__ head) {
  ROOM_FOR(j, n) head[j] = (j == 0 || sb[j] != sb[j - 1] || sk[j] != sk[j - 1]) ? 1 : 0;
}

__global__ __launch_bounds__(kRoomThreads) void room_cell_starts_kernel(const int *__restrict__ head, const int *__restrict__ excl, long long n,
                                                                       int *__restrict__ point_cell, int *__restrict__ cell_start,
                                                                       int *status) {
  ROOM_FOR(j, n) {
    const int cid = excl[j] + head[j] - 1;
    point_cell[j] = cid;
    if (head[j]) cell_start[cid] = (int)j;
    if (j == n - 1) {
      cell_start[cid + 1] = (int)n;
      status[kStCells] = cid + 1;
    }
  }
}

__global__ __launch_bounds__(kRoomThreads) void room_zero_kernel(int *p, long long n) {
  ROOM_FOR(i, n) p[i] = 0;
}

// block tables (5, G): points, cells, resampled total, first entry, first window
__global__ __launch_bounds__(kRoomThreads) void room_cell_counts_kernel(const int *__restrict__ sb, const int *__restrict__ cell_start,
                                                                       const int *__restrict__ status, long long G, int *tables) {
  const long long ncells = status[kStCells];
  ROOM_FOR(k, ncells) {
    const int a = cell_start[k], g = sb[a];
    atomicAdd(tables + g, cell_start[k + 1] - a);
    atomicAdd(tables + G + g, 1);
  }
}

__device__ __forceinline__ int block_avg(const int *__restrict__ tables, long long G, int g) {
  return tables[g] / tables[G + g];                       // int(np.average(grid_point_counts)): floor of an exact quotient
}

__global__ __launch_bounds__(kRoomThreads) void room_cell_out_kernel(const int *__restrict__ sb, const int *__restrict__ cell_start,
                                                                    int *status, long long n, long long G, int *tables,
                                                                    int *__restrict__ cell_out) {
  const long long ncells = status[kStCells];
  ROOM_FOR(k, n) {
    int out = 0;
    if (k < ncells) {
      const int a = cell_start[k], g = sb[a], c = cell_start[k + 1] - a;
      const int avg = block_avg(tables, G, g);
      out = avg > c ? avg : c;                             // ceil(avg / c) > 1 <=> avg > c: the first avg of the c * r copies; else the c points
      atomicAdd(tables + 2 * G + g, out);
      if (avg > c && (long long)c * ((avg + c - 1) / c) > kRoomLaneCopies) atomicAdd(status + kStBigCells, 1);
    }
    cell_out[k] = out;
  }
}

__global__ __launch_bounds__(kRoomThreads) void room_window_counts_kernel(const int *__restrict__ tables, long long G, int max_num_points,
                                                                         int *__restrict__ nwin) {
  ROOM_FOR(g, G) {
    const int total = tables[2 * G + g];
    nwin[g] = total > 0 ? (int)(((long long)total + max_num_points - 1) / max_num_points) : 0;
  }
}

// ---- step 4c: the resampling fill ----------------------------------------------------------------------------------------------------------
struct RoomSeed {
  uint2 key;
  uint32_t c2, c3;
};
__device__ __forceinline__ RoomSeed room_seed(const long long *__restrict__ seed) {
  const DrawStream d = draw_stream(reinterpret_cast<const int64_t *>(seed));           // this file's counter: c2 ^ use, c3
  return {d.key, d.stream, (uint32_t)((unsigned long long)seed[1] >> 32)};
}
__device__ __forceinline__ uint4 room_draw(const RoomSeed &s, uint32_t stream, uint32_t a, uint32_t b) {
  return philox4x32_10(make_uint4(a, b, s.c2 ^ stream, s.c3), s.key);
}

// cells that keep their points (c >= avg): one lane per sorted point
__global__ __launch_bounds__(kRoomThreads) void room_fill_keep_kernel(const int *__restrict__ perm, const int *__restrict__ sb,
                                                                     const int *__restrict__ point_cell, const int *__restrict__ cell_start,
                                                                     const int *__restrict__ cell_out_start, const int *__restrict__ tables,
                                                                     long long n, long long G, long long E, int *__restrict__ entry_point,
                                                                     int *__restrict__ entry_block) {
  ROOM_FOR(j, n) {
    const int k = point_cell[j], a = cell_start[k], g = sb[j];
    if (cell_start[k + 1] - a < block_avg(tables, G, g)) continue;
    const long long e = (long long)cell_out_start[k] + (j - a);
    if (e < E) {
      entry_point[e] = perm[j];
      entry_block[e] = g;
    }
  }
}

// cells that draw (c < avg, r = ceil(avg / c), the copies a a .. b b ..): avg of the c * r copies, uniformly without replacement.
// One lane per cell: selection sampling (copy t is taken with probability need / remaining) -- every subset of avg copies is equally
// likely, which is what "shuffle, keep the first avg" gives.  The 64-bit draw is scaled by the high product: bias below 2^-32.
__global__ __launch_bounds__(kRoomThreads) void room_fill_draw_kernel(const int *__restrict__ perm, const int *__restrict__ sb,
                                                                     const int *__restrict__ cell_start, const int *__restrict__ cell_out_start,
                                                                     const int *__restrict__ tables, const int *__restrict__ status, long long G,
                                                                     long long E, const long long *__restrict__ seed,
                                                                     int *__restrict__ entry_point, int *__restrict__ entry_block) {
  const long long ncells = status[kStCells];
  const RoomSeed sd = room_seed(seed);
  ROOM_FOR(k, ncells) {
    const int a = cell_start[k], g = sb[a], c = cell_start[k + 1] - a;
    const int avg = block_avg(tables, G, g);
    if (avg <= c) continue;
    const int r = (avg + c - 1) / c;
    const long long total = (long long)c * r;
    if (total > kRoomLaneCopies) continue;
    long long e = cell_out_start[k];
    int need = avg;
    uint4 w = make_uint4(0, 0, 0, 0);
    for (int t = 0; t < (int)total && need > 0; ++t) {
      if ((t & 1) == 0) w = room_draw(sd, kStreamLane, (uint32_t)k, (uint32_t)(t >> 1));
      const unsigned long long u = (t & 1) ? (((unsigned long long)w.w << 32) | w.z) : (((unsigned long long)w.y << 32) | w.x);
      const unsigned long long remaining = (unsigned long long)(total - t);
      if (__umul64hi(u, remaining) < (unsigned long long)need) {
        if (e < E) {
          entry_point[e] = perm[a + t / r];
          entry_block[e] = g;
        }
        ++e;
        --need;
      }
    }
  }
}

__device__ __forceinline__ unsigned long long big_copy_key(const RoomSeed &sd, long long k, long long t) {
  const uint4 w = room_draw(sd, kStreamBig, (uint32_t)k, (uint32_t)t);
  return ((unsigned long long)w.y << 32) | w.x;
}

// count of copies t in [0, total) with key <= bound (le != 0) or key < bound, over the workgroup
__device__ __forceinline__ long long big_count(const RoomSeed &sd, long long k, long long total, unsigned long long bound, int le) {
  long long mine = 0;
  for (long long t = threadIdx.x; t < total; t += kRoomThreads) {
    const unsigned long long key = big_copy_key(sd, k, t);
    mine += (le ? key <= bound : key < bound) ? 1 : 0;
  }
  long long sum;
  wg_exscan(mine, sum);
  return sum;
}

// the same selection for cells of more than kRoomLaneCopies copies, one workgroup per cell: every copy gets a 64-bit Philox key, the avg
// smallest keys are kept (ties, if any, by copy order).  The avg-th smallest key is found by bisection over the key's 64 bits (keys are
// recomputed, nothing is stored), then the kept copies are written in copy order through a workgroup prefix sum.
__global__ __launch_bounds__(kRoomThreads) void room_fill_draw_big_kernel(const int *__restrict__ perm, const int *__restrict__ sb,
                                                                         const int *__restrict__ cell_start,
                                                                         const int *__restrict__ cell_out_start,
                                                                         const int *__restrict__ tables, const int *__restrict__ status,
                                                                         long long G, long long E, const long long *__restrict__ seed,
                                                                         int *__restrict__ entry_point, int *__restrict__ entry_block) {
  if (status[kStBigCells] == 0) return;                    // the usual room: no cell that large
  const long long ncells = status[kStCells];
  const RoomSeed sd = room_seed(seed);
  for (long long k = blockIdx.x; k < ncells; k += gridDim.x) {
    const int a = cell_start[k], g = sb[a], c = cell_start[k + 1] - a;
    const int avg = block_avg(tables, G, g);
    if (avg <= c) continue;                                // (uniform over the workgroup)
    const int r = (avg + c - 1) / c;
    const long long total = (long long)c * r;
    if (total <= kRoomLaneCopies) continue;
    unsigned long long lo = 0ull, hi = ~0ull;              // smallest T with #(key <= T) >= avg
    while (lo < hi) {
      const unsigned long long mid = lo + ((hi - lo) >> 1);
      if (big_count(sd, k, total, mid, 1) >= avg) hi = mid; else lo = mid + 1;
    }
    const unsigned long long T = lo;
    const long long need_eq = avg - big_count(sd, k, total, T, 0);
    long long run_lt = 0, run_eq = 0;
    const long long e0 = cell_out_start[k];
    for (long long base = 0; base < total; base += kRoomThreads) {
      const long long t = base + threadIdx.x;
      const unsigned long long key = t < total ? big_copy_key(sd, k, t) : ~0ull;
      const bool lt = t < total && key < T, eq = t < total && key == T;
      long long sum;
      const long long ex = wg_exscan((lt ? 1ll : 0ll) | (eq ? (1ll << 32) : 0ll), sum);
      const long long lt_before = run_lt + (ex & 0xFFFFFFFFll), eq_before = run_eq + (ex >> 32);
      if (lt || (eq && eq_before < need_eq)) {
        const long long e = e0 + lt_before + (eq_before < need_eq ? eq_before : need_eq);
        if (e < E) {
          entry_point[e] = perm[a + t / r];
          entry_block[e] = g;
        }
      }
      run_lt += sum & 0xFFFFFFFFll;
      run_eq += sum >> 32;
    }
  }
}

// the block shuffle's keys: 63 random bits per entry (the host orders the entries by (block, key))
__global__ __launch_bounds__(kRoomThreads) void room_shuffle_keys_kernel(long long E, const long long *__restrict__ seed,
                                                                        long long *__restrict__ entry_key) {
  const RoomSeed sd = room_seed(seed);
  ROOM_FOR(e, E) {
    const uint4 w = room_draw(sd, kStreamShuffle, (uint32_t)e, (uint32_t)(e >> 32));
    entry_key[e] = (long long)((((unsigned long long)w.y << 32) | w.x) >> 1);
  }
}

// ---- step 6: per-block minima over the resampled entries, the packed rows, the window table ---------------------------------------------
__global__ __launch_bounds__(kRoomThreads) void room_entry_min_kernel(const double *__restrict__ xyzrgb, long long n,
                                                                     const double *__restrict__ ext, const int *__restrict__ entry_point,
                                                                     const int *__restrict__ entry_block, long long E, long long G,
                                                                     unsigned long long *block_minxy) {
  __shared__ unsigned long long s_min[2 * kRoomLdsBlocks];
  const bool lds = G <= kRoomLdsBlocks;
  if (lds) {
    for (int k = threadIdx.x; k < 2 * (int)G; k += kRoomThreads) s_min[k] = kRoomInfBits;
    __syncthreads();
  }
  ROOM_FOR(e, E) {
    const int p = entry_point[e], g = entry_block[e];
    if (p < 0 || p >= n || g < 0 || g >= G) continue;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const double v = shifted(xyzrgb, p, a, ext);
      if (v >= 0.0) atomicMin(lds ? s_min + g * 2 + a : block_minxy + (long long)g * 2 + a, (unsigned long long)__double_as_longlong(v + 0.0));
    }
  }
  if (lds) {
    __syncthreads();
    for (int k = threadIdx.x; k < 2 * (int)G; k += kRoomThreads)
      if (s_min[k] != kRoomInfBits) atomicMin(block_minxy + k, s_min[k]);
  }
}

__global__ __launch_bounds__(kRoomThreads) void room_pack_kernel(const double *__restrict__ xyzrgb, const int *__restrict__ labels, long long n,
                                                                const double *__restrict__ ext, double half_block,
                                                                const int *__restrict__ entry_point, const int *__restrict__ entry_block,
                                                                long long E, long long G, const unsigned long long *__restrict__ block_minxy,
                                                                float *__restrict__ rows, int *__restrict__ labels_out,
                                                                int *__restrict__ indices) {
  const double max_room[3] = {ext[3] - ext[0], ext[4] - ext[1], ext[5] - ext[2]};
  ROOM_FOR(e, E) {
    int p = entry_point[e], g = entry_block[e];
    p = (p >= 0 && p < n) ? p : 0;
    g = (g >= 0 && g < G) ? g : 0;
    const double x = shifted(xyzrgb, p, 0, ext), y = shifted(xyzrgb, p, 1, ext), z = shifted(xyzrgb, p, 2, ext);
    const double minx = __longlong_as_double((long long)block_minxy[(long long)g * 2]);
    const double miny = __longlong_as_double((long long)block_minxy[(long long)g * 2 + 1]);
    float *row = rows + e * 9;
    row[0] = (float)(x - (minx + half_block));
    row[1] = (float)(y - (miny + half_block));
    row[2] = (float)z;
    row[3] = (float)(xyzrgb[(long long)p * 6 + 3] / 255.0);
    row[4] = (float)(xyzrgb[(long long)p * 6 + 4] / 255.0);
    row[5] = (float)(xyzrgb[(long long)p * 6 + 5] / 255.0);
    row[6] = (float)(x / max_room[0]);
    row[7] = (float)(y / max_room[1]);
    row[8] = (float)(z / max_room[2]);
    if (labels != nullptr) labels_out[e] = labels[p];
    indices[e] = p;
  }
}

// one lane per block: s = ceil(total / max_num_points) windows of ceil(total / s) entries, the last one takes the rest
__global__ __launch_bounds__(kRoomThreads) void room_windows_kernel(const int *__restrict__ tables, const int *__restrict__ block_rank,
                                                                   long long G, int max_num_points, long long E, long long W,
                                                                   long long *__restrict__ offsets, int *__restrict__ window_block) {
  ROOM_FOR(g, G) {
    if (g == 0) offsets[W] = E;
    const int total = tables[2 * G + g];
    if (total <= 0) continue;
    const int s = (int)(((long long)total + max_num_points - 1) / max_num_points);
    const int len = (total + s - 1) / s;
    const long long w0 = tables[4 * G + g], e0 = tables[3 * G + g];
    for (int k = 0; k < s; ++k) {
      if (w0 + k >= W) break;
      offsets[w0 + k] = e0 + (long long)k * len;
      window_block[w0 + k] = block_rank[g];
    }
  }
}

static inline bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace pvcnn

using namespace pvcnn;

extern "C" size_t pvcnn_room_workspace_bytes(long long n, long long num_blocks) {
  if (n < 0 || num_blocks < 0) return 0;
  const long long extent = (long long)room_grid(n) * 6 * 8;
  const long long ints = 2 * n + 2 * num_blocks + scan_parts(std::max(n, num_blocks)) + 64;
  return (size_t)std::max(extent, ints * 4);
}

extern "C" int pvcnn_room_extent(const double *xyzrgb, long long n, double *extent, void *workspace, size_t workspace_bytes, void *stream) {
  PVCNN_REQUIRE(n >= 1 && n <= kRoomMaxPoints, "a room needs between 1 and 2^29 points");
  PVCNN_REQUIRE(xyzrgb && extent && workspace && aligned8(workspace), "null or misaligned pointer");
  PVCNN_REQUIRE(workspace_bytes >= pvcnn_room_workspace_bytes(n, 0), "workspace too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  double *part = static_cast<double *>(workspace);
  const unsigned grid = room_grid(n);
  hipLaunchKernelGGL(room_extent_kernel, dim3(grid), dim3(kRoomThreads), 0, s, xyzrgb, n, 6, 0, part);
  hipLaunchKernelGGL(room_extent_kernel, dim3(1), dim3(kRoomThreads), 0, s, part, (long long)grid, 6, 3, extent);
  return check_launch("room_extent");
}

extern "C" int pvcnn_room_blocks(const double *xyzrgb, long long n, const double *extent, double offset, double block_size, int gx, int gy,
                                 int max_num_points, int *point_block, int *block_count, int *block_target, int *block_rank, int *status,
                                 void *workspace, size_t workspace_bytes, void *stream) {
  PVCNN_REQUIRE(n >= 1 && n <= kRoomMaxPoints, "a room needs between 1 and 2^29 points");
  PVCNN_REQUIRE(gx >= 1 && gy >= 1 && (long long)gx * gy <= kRoomMaxBlocks, "the block table holds at most 2^24 blocks");
  PVCNN_REQUIRE(max_num_points >= 1 && block_size > 0.0 && offset >= 0.0, "bad options");
  PVCNN_REQUIRE(xyzrgb && extent && point_block && block_count && block_target && block_rank && status && workspace, "null pointer");
  const long long G = (long long)gx * gy;
  PVCNN_REQUIRE(workspace_bytes >= pvcnn_room_workspace_bytes(n, G), "workspace too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int *ws = static_cast<int *>(workspace);
  hipLaunchKernelGGL(room_zero_kernel, dim3(room_grid(G)), dim3(kRoomThreads), 0, s, block_count, G);
  hipLaunchKernelGGL(room_zero_kernel, dim3(1), dim3(kRoomThreads), 0, s, status, (long long)kStWords);
  hipLaunchKernelGGL(room_block_keys_kernel, dim3(room_grid(n)), dim3(kRoomThreads), 0, s, xyzrgb, n, extent, offset, block_size, gx, gy,
                     point_block, block_count, status);
  hipLaunchKernelGGL(room_merge_kernel, dim3(room_grid(G)), dim3(kRoomThreads), 0, s, block_count, gx, gy, max_num_points, block_target,
                     block_rank);
  if (int rc = check_launch("room_blocks")) return rc;
  return room_scan(block_rank, block_rank, G, nullptr, ws, s);       // occupied flags -> the reference's block number
}

extern "C" int pvcnn_room_cells(const double *xyzrgb, long long n, const double *extent, double grid_size, long long num_blocks,
                                const int *block_target, int *point_block, unsigned long long *block_min, long long *cell_key, int *status,
                                void *stream) {
  PVCNN_REQUIRE(n >= 1 && n <= kRoomMaxPoints && num_blocks >= 1 && num_blocks <= kRoomMaxBlocks, "bad sizes");
  PVCNN_REQUIRE(grid_size > 0.0, "grid_size must be positive");
  PVCNN_REQUIRE(xyzrgb && extent && block_target && point_block && block_min && cell_key && status, "null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(room_fill_u64_kernel, dim3(room_grid(3 * num_blocks)), dim3(kRoomThreads), 0, s, block_min, 3 * num_blocks, kRoomInfBits);
  hipLaunchKernelGGL(room_block_min_kernel, dim3(room_grid(n)), dim3(kRoomThreads), 0, s, xyzrgb, n, extent, num_blocks, block_target,
                     point_block, block_min);
  hipLaunchKernelGGL(room_cell_keys_kernel, dim3(room_grid(n)), dim3(kRoomThreads), 0, s, xyzrgb, n, extent, grid_size, point_block,
                     block_min, cell_key, status);
  return check_launch("room_cells");
}

extern "C" int pvcnn_room_plan(const int *sorted_block, const long long *sorted_key, long long n, long long num_blocks, int max_num_points,
                               int *point_cell, int *cell_start, int *cell_out, int *cell_out_start, int *block_tables, int *status,
                               void *workspace, size_t workspace_bytes, void *stream) {
  PVCNN_REQUIRE(n >= 1 && n <= kRoomMaxPoints && num_blocks >= 1 && num_blocks <= kRoomMaxBlocks && max_num_points >= 1, "bad sizes");
  PVCNN_REQUIRE(sorted_block && sorted_key && point_cell && cell_start && cell_out && cell_out_start && block_tables && status && workspace,
                "null pointer");
  PVCNN_REQUIRE(workspace_bytes >= pvcnn_room_workspace_bytes(n, num_blocks), "workspace too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long G = num_blocks;
  int *head = static_cast<int *>(workspace), *excl = head + n, *nwin = excl + n, *part = nwin + 2 * G;
  hipLaunchKernelGGL(room_heads_kernel, dim3(room_grid(n)), dim3(kRoomThreads), 0, s, sorted_block, sorted_key, n, head);
  if (int rc = room_scan(head, excl, n, nullptr, part, s)) return rc;
  hipLaunchKernelGGL(room_cell_starts_kernel, dim3(room_grid(n)), dim3(kRoomThreads), 0, s, head, excl, n, point_cell, cell_start, status);
  hipLaunchKernelGGL(room_zero_kernel, dim3(room_grid(5 * G)), dim3(kRoomThreads), 0, s, block_tables, 5 * G);
  hipLaunchKernelGGL(room_cell_counts_kernel, dim3(room_grid(n)), dim3(kRoomThreads), 0, s, sorted_block, cell_start, status, G, block_tables);
  hipLaunchKernelGGL(room_cell_out_kernel, dim3(room_grid(n)), dim3(kRoomThreads), 0, s, sorted_block, cell_start, status, n, G, block_tables,
                     cell_out);
  if (int rc = check_launch("room_plan")) return rc;
  if (int rc = room_scan(cell_out, cell_out_start, n, status + kStEntries, part, s)) return rc;
  hipLaunchKernelGGL(room_window_counts_kernel, dim3(room_grid(G)), dim3(kRoomThreads), 0, s, block_tables, G, max_num_points, nwin);
  if (int rc = room_scan(nwin, block_tables + 4 * G, G, status + kStWindows, part, s)) return rc;
  return room_scan(block_tables + 2 * G, block_tables + 3 * G, G, nullptr, part, s);
}

extern "C" int pvcnn_room_fill(const int *perm, const int *sorted_block, const int *point_cell, const int *cell_start,
                               const int *cell_out_start, const int *block_tables, const int *status, long long n, long long num_blocks,
                               long long num_entries, const long long *seed, int *entry_point, int *entry_block, long long *entry_key,
                               void *stream) {
  PVCNN_REQUIRE(n >= 1 && n <= kRoomMaxPoints && num_blocks >= 1 && num_blocks <= kRoomMaxBlocks, "bad sizes");
  PVCNN_REQUIRE(num_entries >= 1 && num_entries < (1ll << 31), "bad entry count");
  PVCNN_REQUIRE(perm && sorted_block && point_cell && cell_start && cell_out_start && block_tables && status && seed && entry_point &&
                    entry_block && entry_key, "null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long G = num_blocks, E = num_entries;
  hipLaunchKernelGGL(room_fill_keep_kernel, dim3(room_grid(n)), dim3(kRoomThreads), 0, s, perm, sorted_block, point_cell, cell_start,
                     cell_out_start, block_tables, n, G, E, entry_point, entry_block);
  hipLaunchKernelGGL(room_fill_draw_kernel, dim3(room_grid(n)), dim3(kRoomThreads), 0, s, perm, sorted_block, cell_start, cell_out_start,
                     block_tables, status, G, E, seed, entry_point, entry_block);
  hipLaunchKernelGGL(room_fill_draw_big_kernel, dim3(kNumCU), dim3(kRoomThreads), 0, s, perm, sorted_block, cell_start, cell_out_start,
                     block_tables, status, G, E, seed, entry_point, entry_block);
  hipLaunchKernelGGL(room_shuffle_keys_kernel, dim3(room_grid(E)), dim3(kRoomThreads), 0, s, E, seed, entry_key);
  return check_launch("room_fill");
}

extern "C" int pvcnn_room_pack(const double *xyzrgb, const int *labels, long long n, const double *extent, double half_block,
                               const int *entry_point, const int *entry_block, long long num_entries, long long num_blocks,
                               int max_num_points, long long num_windows, const int *block_tables, const int *block_rank,
                               unsigned long long *block_minxy, float *rows, int *labels_out, int *indices, long long *offsets,
                               int *window_block, void *stream) {
  PVCNN_REQUIRE(n >= 1 && n <= kRoomMaxPoints && num_blocks >= 1 && num_blocks <= kRoomMaxBlocks && max_num_points >= 1, "bad sizes");
  PVCNN_REQUIRE(num_entries >= 1 && num_entries < (1ll << 31) && num_windows >= 1 && num_windows <= num_entries, "bad entry / window count");
  PVCNN_REQUIRE(xyzrgb && extent && entry_point && entry_block && block_tables && block_rank && block_minxy && rows && indices && offsets &&
                    window_block, "null pointer");
  PVCNN_REQUIRE((labels == nullptr) == (labels_out == nullptr), "labels and labels_out go together");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long G = num_blocks, E = num_entries;
  hipLaunchKernelGGL(room_fill_u64_kernel, dim3(room_grid(2 * G)), dim3(kRoomThreads), 0, s, block_minxy, 2 * G, kRoomInfBits);
  hipLaunchKernelGGL(room_entry_min_kernel, dim3(room_grid(E)), dim3(kRoomThreads), 0, s, xyzrgb, n, extent, entry_point, entry_block, E, G,
                     block_minxy);
  hipLaunchKernelGGL(room_pack_kernel, dim3(room_grid(E)), dim3(kRoomThreads), 0, s, xyzrgb, labels, n, extent, half_block, entry_point,
                     entry_block, E, G, block_minxy, rows, labels_out, indices);
  hipLaunchKernelGGL(room_windows_kernel, dim3(room_grid(G)), dim3(kRoomThreads), 0, s, block_tables, block_rank, G, max_num_points, E,
                     num_windows, offsets, window_block);
  return check_launch("room_pack");
}
