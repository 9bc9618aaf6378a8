// sparse.hip -- the submanifold sparse 3x3x3 convolution on the occupied voxels of a cloud (include/pvcnn_hip.h, "Sparse voxels";
// pvcnn_amd/modules/functional/sparse.py).  The definition is in the header; tests/sparse_conv_truth.py restates it in torch fp64.
//
// map      : the active voxels of (B, R^3) counts, ascending in the flat voxel number, by a deterministic compaction -- flags counted
//            per chunk of 1024, the chunk counts scanned by one workgroup, every chunk writes its voxels at its prefix -- plus one
//            launch for the table of the 27 neighbour rows.  No atomics: the same counts give the same map.  The active count stays
//            on the device (offsets[B]); every later launch is sized by the static capacity `cap` and bounded by that word.
// gather   : (B, C, R^3) -> rows (cap, C), a 64 x 64 transposition through LDS: the grid side is read along the voxels, the row side
// scatter  : written along the channels, full lines both ways.  scatter is the inverse walk over ALL voxels (zeros where inactive).
// conv     : implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32 operands, fp32 accumulate: the arithmetic of conv3d.hip).
//            M = 64 consecutive rows, N = 64 output channels, K = (tap, ci) in chunks of CIC channels; a workgroup of 4 waves, each
//            one 32 x 32 accumulator.  Per (tap, chunk) the tap's weight slab (CIC, 64) and the 64 neighbour rows -- fetched through
//            the table, zeros where it says -1 -- are staged in LDS; the next step's global loads are issued before the products of
//            this one.  A tap at which NO row of the tile has a neighbour (one ballot per tap) is left out whole: it would only add
//            products with an exact zero, so the result is the same bits (pvcnn_sparse_debug_skip switches the skip off; the tests
//            compare).  A:(row, k) is read from xs[k][row], B:(k, co) from ws[k][co]: consecutive lanes, consecutive words.
//            Backward-data is this kernel on the weights flipped and transposed (sparse_weight_transform_kernel).
// wgrad    : grad_w[co, ci, tap] = sum_j gy[j, co] x[nbr[j, tap], ci]: M = co, N = ci, K = rows.  Workgroup (p, tap, tile) sums the
//            rows of chunk p (1024 rows, in steps of 32, steps without a neighbour at the tap left out) into a partial; the partials
//            are added in ascending p by a second launch.  No float atomics.  The tap-13 workgroups (a row is its own neighbour
//            there) add the column sums of gy for grad_bias.
// Bounds: a table entry outside [0, count) is treated as -1, rows are checked against cap, channels against C: with a map that breaks
// the contract the kernels still read and write inside the arrays they were given.
#include "common.h"
#include "wave.h"

namespace pvcnn {

constexpr int kSpRows = PVCNN_SPARSE_ROW_TILE;       // rows of a convolution tile
constexpr int kSpCo = 64;                            // output channels of a convolution tile
constexpr int kSpScan = 1024;                        // flags per workgroup of the compaction
constexpr int kSpWgChunk = PVCNN_SPARSE_WGRAD_CHUNK; // rows per partial of backward-weight
constexpr int kSpWgStep = 32;                        // rows per staged step of backward-weight
constexpr unsigned kAllTaps = (1u << 27) - 1u;
static_assert(kSpRows == 64 && kSpCo == 64, "four waves of one 32 x 32 accumulator each");

typedef float f32x16 __attribute__((ext_vector_type(16)));

static int g_sparse_skip = 1;                        // pvcnn_sparse_debug_skip

static bool sparse_supported(long long B, long long R) {
  return B >= 1 && R >= 1 && R <= PVCNN_SPARSE_MAX_R && B * R * R * R < (1ll << 31);
}

// ---------------------------------------------------------------------------------------------------------------- the map
__global__ __launch_bounds__(256) void sparse_count_kernel(const int32_t *__restrict__ cnt, long long T, int32_t *__restrict__ sums) {
  const long long base = (long long)blockIdx.x * kSpScan + threadIdx.x * 4;
  int c = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) c += (base + i < T && cnt[base + i] > 0) ? 1 : 0;
  c = wg_sum(c);
  if (threadIdx.x == 0) sums[blockIdx.x] = c;
}

// sums[0 .. n) -> their exclusive prefixes, in place; the total -> the count word (clamped to cap) and the overflow flag
__global__ __launch_bounds__(1024) void sparse_scan_kernel(int32_t *__restrict__ sums, int n, int cap, int32_t *__restrict__ count_word,
                                                           int32_t *__restrict__ overflow) {
  __shared__ int s_part[1024];
  const int t = threadIdx.x;
  const int per = (n + 1023) / 1024;
  const int a = min(t * per, n), b = min(a + per, n);
  int s = 0;
  for (int i = a; i < b; ++i) s += sums[i];
  s_part[t] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int v = t >= o ? s_part[t - o] : 0;
    __syncthreads();
    s_part[t] += v;
    __syncthreads();
  }
  int run = s_part[t] - s;
  for (int i = a; i < b; ++i) { const int v = sums[i]; sums[i] = run; run += v; }
  if (t == 1023) {
    const int total = s_part[1023];
    *count_word = min(total, cap);
    *overflow = total > cap ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void sparse_fill_kernel(const int32_t *__restrict__ cnt, long long T, int R3,
                                                          const int32_t *__restrict__ prefix, int cap, int32_t *__restrict__ voxel,
                                                          int32_t *__restrict__ index, int32_t *__restrict__ offsets) {
  __shared__ int s_wave[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long base = (long long)blockIdx.x * kSpScan + threadIdx.x * 4;
  bool f[4];
  int c = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) { f[i] = base + i < T && cnt[base + i] > 0; c += f[i] ? 1 : 0; }
  const int incl = wave_inclusive_scan(c, lane);
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  int run = prefix[blockIdx.x] + (incl - c);
  for (int w = 0; w < wave; ++w) run += s_wave[w];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long e = base + i;
    if (e >= T) break;
    if (e % R3 == 0) offsets[e / R3] = min(run, cap);      // the first row of the cloud that begins here
    int row = -1;
    if (f[i]) {
      if (run < cap) { row = run; voxel[run] = (int32_t)e; }
      ++run;
    }
    index[e] = row;
  }
}

// one thread per (row, tap); the rows past the count get voxel = -1 here (the fill launch wrote the others)
__global__ __launch_bounds__(256) void sparse_nbr_kernel(int32_t *__restrict__ voxel, const int32_t *__restrict__ index,
                                                         const int32_t *__restrict__ count_word, int cap, int R,
                                                         int32_t *__restrict__ nbr) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)cap * 27) return;
  const int row = (int)(e / 27), tap = (int)(e % 27);
  const int count = min(*count_word, cap);
  int out = -1;
  if (row < count) {
    int v = voxel[row];
    const int z = v % R; v /= R;
    const int y = v % R; v /= R;
    const int x = v % R;
    const int b = v / R;
    const int nx = x + tap / 9 - 1, ny = y + (tap / 3) % 3 - 1, nz = z + tap % 3 - 1;
    if (nx >= 0 && nx < R && ny >= 0 && ny < R && nz >= 0 && nz < R) {
      out = index[(((long long)b * R + nx) * R + ny) * R + nz];
      if (out >= count) out = -1;
    }
  } else if (tap == 0) {
    voxel[row] = -1;
  }
  nbr[e] = out;
}

// ------------------------------------------------------------------------------------------- rows in and out of dense grids
__global__ __launch_bounds__(256) void sparse_gather_kernel(const float *__restrict__ grid, const int32_t *__restrict__ voxel,
                                                            const int32_t *__restrict__ count_word, int cap, int C, int R3,
                                                            long long T, float *__restrict__ rows) {
  __shared__ float tile[64][65];
  __shared__ int s_v[64];
  const int t = threadIdx.x, lo = t & 63, hi = t >> 6;
  const int row0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  const int count = min(*count_word, cap);
  if (t < 64) {
    const int j = row0 + t;
    const int v = j < count ? voxel[j] : -1;
    s_v[t] = (v >= 0 && v < T) ? v : -1;
  }
  __syncthreads();
  {
    const int v = s_v[lo];
    const float *base = grid + ((size_t)(v < 0 ? 0 : v / R3) * C) * R3 + (v < 0 ? 0 : v % R3);
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
      const int c = hi + 4 * i;
      tile[lo][c] = (v >= 0 && c0 + c < C) ? base[(size_t)(c0 + c) * R3] : 0.f;
    }
  }
  __syncthreads();
  if (c0 + lo < C) {
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
      const int r = hi + 4 * i;
      if (row0 + r < cap) rows[(size_t)(row0 + r) * C + c0 + lo] = tile[r][lo];
    }
  }
}

__global__ __launch_bounds__(256) void sparse_scatter_kernel(const float *__restrict__ rows, const int32_t *__restrict__ index,
                                                             const int32_t *__restrict__ count_word, int cap, int C, int R3,
                                                             long long T, float *__restrict__ grid) {
  __shared__ float tile[64][65];
  __shared__ int s_i[64];
  const int t = threadIdx.x, lo = t & 63, hi = t >> 6;
  const long long e0 = (long long)blockIdx.x * 64;
  const int c0 = blockIdx.y * 64;
  const int count = min(*count_word, cap);
  if (t < 64) {
    const int j = e0 + t < T ? index[e0 + t] : -1;
    s_i[t] = (j >= 0 && j < count) ? j : -1;
  }
  __syncthreads();
#pragma unroll 4
  for (int i = 0; i < 16; ++i) {
    const int p = hi + 4 * i;
    const int j = s_i[p];
    tile[p][lo] = (j >= 0 && c0 + lo < C) ? rows[(size_t)j * C + c0 + lo] : 0.f;
  }
  __syncthreads();
  const long long e = e0 + lo;
  if (e < T) {
    float *base = grid + ((size_t)(e / R3) * C) * R3 + e % R3;
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
      const int c = hi + 4 * i;
      if (c0 + c < C) base[(size_t)(c0 + c) * R3] = tile[lo][c];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------- the convolution
// (Co, Ci, 27) -> (27, Ci, Co)                      [forward]
// (Co, Ci, 27) -> (27, Co, Ci) with taps reversed   [backward-data: the same convolution with Ci' = Co, Co' = Ci; slab t of the image
//                                                    is tap 26 - t of the weight, so the table is read at 26 - tap of the weight]
__global__ __launch_bounds__(256) void sparse_weight_transform_kernel(const float *__restrict__ w, int Co, int Ci, int for_bwd_data,
                                                                      float *__restrict__ wt) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= Co * Ci * 27) return;
  const int tap = e % 27, ci = (e / 27) % Ci, co = e / (27 * Ci);
  if (!for_bwd_data) wt[((size_t)tap * Ci + ci) * Co + co] = w[e];
  else               wt[((size_t)(26 - tap) * Co + co) * Ci + ci] = w[e];
}

// four channels c .. c + 3 of a row of C channels, zeros past C
__device__ __forceinline__ float4 row_quad(const float *__restrict__ row, int c, int C, bool vec) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (vec) {
    if (c < C) v = *reinterpret_cast<const float4 *>(row + c);
  } else {
    if (c < C) v.x = row[c];
    if (c + 1 < C) v.y = row[c + 1];
    if (c + 2 < C) v.z = row[c + 2];
    if (c + 3 < C) v.w = row[c + 3];
  }
  return v;
}

template <int CIC>
__global__ __launch_bounds__(256) void sparse_conv_kernel(const float *__restrict__ x, const float *__restrict__ wt,
                                                          const float *__restrict__ bias, const int32_t *__restrict__ nbr,
                                                          const int32_t *__restrict__ count_word, int cap, int Ci, int Co, int vec,
                                                          int skip, float *__restrict__ y) {
  constexpr int XS = kSpRows + 2;                    // xs[k][row]: the staging writes (4 lanes per row, 4 k each) hit 32 banks
  constexpr int NQ = CIC / 16, NW = CIC / 4;
  __shared__ float xs[CIC * XS];
  __shared__ float ws[CIC * kSpCo];
  __shared__ int s_nbr[kSpRows * 27];
  __shared__ unsigned s_mask;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int row0 = blockIdx.x * kSpRows, co0 = blockIdx.y * kSpCo;
  const int count = min(*count_word, cap);
  for (int e = t; e < kSpRows * 27; e += 256) {
    const long long g = (long long)row0 * 27 + e;
    const int n = (g < (long long)cap * 27 && row0 + e / 27 < count) ? nbr[g] : -1;
    s_nbr[e] = (n >= 0 && n < count) ? n : -1;
  }
  __syncthreads();
  if (wave == 0) {
    unsigned m = 0;
    for (int tap = 0; tap < 27; ++tap)
      if (__ballot(s_nbr[lane * 27 + tap] >= 0) != 0ull) m |= 1u << tap;
    if (lane == 0) s_mask = skip ? m : kAllTaps;
  }
  __syncthreads();
  const unsigned mask = (unsigned)__builtin_amdgcn_readfirstlane((int)s_mask);

  const int wm = wave >> 1, wn = wave & 1;
  const int srow = t >> 2, sq = t & 3;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  float4 xv[NQ];
  float wv[NW];
  // the global loads of step (tap, c0) into registers
  auto fetch = [&](int tap, int c0) {
    const int n = s_nbr[srow * 27 + tap];
    const float *xr = x + (size_t)(n < 0 ? 0 : n) * Ci;
#pragma unroll
    for (int h = 0; h < NQ; ++h)
      xv[h] = n >= 0 ? row_quad(xr, c0 + 4 * sq + 16 * h, Ci, vec != 0) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float *wtap = wt + (size_t)tap * Ci * Co;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int c = c0 + wave + 4 * i;
      wv[i] = (c < Ci && co0 + lane < Co) ? wtap[(size_t)c * Co + co0 + lane] : 0.f;
    }
  };
  auto advance = [&](int &tap, int &c0) {
    c0 += CIC;
    if (c0 >= Ci) {
      c0 = 0;
      do ++tap; while (tap < 27 && !((mask >> tap) & 1u));
    }
  };

  int tap = 0, c0 = 0;
  while (tap < 27 && !((mask >> tap) & 1u)) ++tap;
  if (tap < 27) fetch(tap, c0);
  while (tap < 27) {
#pragma unroll
    for (int h = 0; h < NQ; ++h) {
      const int k = 4 * sq + 16 * h;
      xs[(k + 0) * XS + srow] = xv[h].x;
      xs[(k + 1) * XS + srow] = xv[h].y;
      xs[(k + 2) * XS + srow] = xv[h].z;
      xs[(k + 3) * XS + srow] = xv[h].w;
    }
#pragma unroll
    for (int i = 0; i < NW; ++i) ws[(wave + 4 * i) * kSpCo + lane] = wv[i];
    __syncthreads();
    advance(tap, c0);
    if (tap < 27) fetch(tap, c0);                    // in flight behind this step's products
    const float *ap = xs + (lane >> 5) * XS + wm * 32 + (lane & 31);
    const float *bp = ws + (lane >> 5) * kSpCo + wn * 32 + (lane & 31);
#pragma unroll
    for (int kk = 0; kk < CIC / 2; ++kk)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * kk * XS], bp[2 * kk * kSpCo], acc, 0, 0, 0);
    __syncthreads();
  }

  const int co = co0 + wn * 32 + (lane & 31);
  if (co < Co) {
    const float bv = bias ? bias[co] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = row0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (row < cap) y[(size_t)row * Co + co] = row < count ? acc[r] + bv : 0.f;
    }
  }
}

// part (P, 27, Co, Ci), part_b (P, Co); grid (P, 27, co tiles x ci tiles)
__global__ __launch_bounds__(256) void sparse_wgrad_kernel(const float *__restrict__ x, const float *__restrict__ gy,
                                                           const int32_t *__restrict__ nbr, const int32_t *__restrict__ count_word,
                                                           int cap, int Ci, int Co, int vecx, int vecg, int skip,
                                                           float *__restrict__ part, float *__restrict__ part_b) {
  __shared__ __attribute__((aligned(16))) float gs[kSpWgStep * 64];   // [row][co]
  __shared__ __attribute__((aligned(16))) float xs[kSpWgStep * 64];   // [row][ci]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int p = blockIdx.x, tap = blockIdx.y;
  const int ntc = (Ci + 63) / 64;
  const int co0 = (blockIdx.z / ntc) * 64, ci0 = (blockIdx.z % ntc) * 64;
  const int count = min(*count_word, cap);
  const int rbeg = p * kSpWgChunk, rend = min(rbeg + kSpWgChunk, count);
  const int wm = wave >> 1, wn = wave & 1;
  const int srow = t >> 3, sc = (t & 7) * 4;
  const bool do_bias = tap == 13 && ci0 == 0 && t < 64;
  float bsum = 0.f;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int r0 = rbeg; r0 < rend; r0 += kSpWgStep) {
    const int j = r0 + srow;
    int n = j < rend ? nbr[(size_t)j * 27 + tap] : -1;
    if (n >= count) n = -1;
    const int any = __syncthreads_or(n >= 0);        // (also: the previous step's LDS reads are over)
    if (skip && !any) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int col = sc + 32 * i;
      float4 gv = make_float4(0.f, 0.f, 0.f, 0.f), xv = gv;
      if (n >= 0) {
        gv = row_quad(gy + (size_t)j * Co, co0 + col, Co, vecg != 0);
        xv = row_quad(x + (size_t)n * Ci, ci0 + col, Ci, vecx != 0);
      }
      *reinterpret_cast<float4 *>(gs + srow * 64 + col) = gv;
      *reinterpret_cast<float4 *>(xs + srow * 64 + col) = xv;
    }
    __syncthreads();
    const float *ap = gs + (lane >> 5) * 64 + wm * 32 + (lane & 31);
    const float *bp = xs + (lane >> 5) * 64 + wn * 32 + (lane & 31);
#pragma unroll
    for (int kk = 0; kk < kSpWgStep / 2; ++kk)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * kk * 64], bp[2 * kk * 64], acc, 0, 0, 0);
    if (do_bias) {
#pragma unroll 8
      for (int k = 0; k < kSpWgStep; ++k) bsum += gs[k * 64 + t];
    }
  }
  const int ci = ci0 + wn * 32 + (lane & 31);
  if (ci < Ci) {
    float *o = part + ((size_t)p * 27 + tap) * Co * Ci;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (co < Co) o[(size_t)co * Ci + ci] = acc[r];
    }
  }
  if (do_bias && co0 + t < Co) part_b[(size_t)p * Co + co0 + t] = bsum;
}

// the partials in ascending p; thread e walks the partial's own (tap, co, ci) order
__global__ __launch_bounds__(256) void sparse_wgrad_reduce_kernel(const float *__restrict__ part, const float *__restrict__ part_b,
                                                                  int P, int Ci, int Co, float *__restrict__ grad_w,
                                                                  float *__restrict__ grad_b) {
  const int n = 27 * Co * Ci;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < n) {
    if (!grad_w) return;
    float s = 0.f;
    for (int p = 0; p < P; ++p) s += part[(size_t)p * n + e];
    const int ci = e % Ci, co = (e / Ci) % Co, tap = e / (Ci * Co);
    grad_w[((size_t)co * Ci + ci) * 27 + tap] = s;
  } else if (e < n + Co && grad_b) {
    const int co = e - n;
    float s = 0.f;
    for (int p = 0; p < P; ++p) s += part_b[(size_t)p * Co + co];
    grad_b[co] = s;
  }
}

}  // namespace pvcnn

using namespace pvcnn;

static bool conv_sizes_ok(long long cap, int Ci, int Co) {
  return cap >= 1 && cap < (1ll << 31) / 27 && Ci >= 1 && Co >= 1 && Ci <= 4096 && Co <= 4096;
}

extern "C" int pvcnn_sparse_debug_skip(int on) {
  const int was = g_sparse_skip;
  if (on >= 0) g_sparse_skip = on ? 1 : 0;
  return was;
}

extern "C" size_t pvcnn_sparse_map_workspace_bytes(int B, int R) {
  if (!sparse_supported(B, R)) return 0;
  const long long T = (long long)B * R * R * R;
  return (size_t)((T + kSpScan - 1) / kSpScan) * sizeof(int32_t);
}

extern "C" size_t pvcnn_sparse_map_bytes(int B, int R, long long cap) {
  if (!sparse_supported(B, R) || cap < 1 || cap >= (1ll << 31) / 27) return 0;
  const long long T = (long long)B * R * R * R;
  return (size_t)(cap + T + (B + 1) + 27 * cap + 1) * sizeof(int32_t);
}

extern "C" int pvcnn_sparse_map(const int32_t *cnt, int B, int R, long long cap, int32_t *voxel, int32_t *index, int32_t *offsets,
                                int32_t *nbr, int32_t *overflow, void *workspace, size_t workspace_bytes, void *stream) {
  PVCNN_REQUIRE(sparse_supported(B, R), "B >= 1, 1 <= R <= 128 and B R^3 < 2^31 expected");
  PVCNN_REQUIRE(cap >= 1 && cap < (1ll << 31) / 27, "cap in [1, 2^31 / 27) expected");
  PVCNN_REQUIRE(cnt && voxel && index && offsets && nbr && overflow && workspace, "null pointer");
  PVCNN_REQUIRE(workspace_bytes >= pvcnn_sparse_map_workspace_bytes(B, R), "workspace too small");
  const long long T = (long long)B * R * R * R;
  const int R3 = R * R * R;
  const unsigned nblk = (unsigned)((T + kSpScan - 1) / kSpScan);
  hipStream_t s = static_cast<hipStream_t>(stream);
  int32_t *sums = static_cast<int32_t *>(workspace);
  hipLaunchKernelGGL(sparse_count_kernel, dim3(nblk), dim3(256), 0, s, cnt, T, sums);
  hipLaunchKernelGGL(sparse_scan_kernel, dim3(1), dim3(1024), 0, s, sums, (int)nblk, (int)cap, offsets + B, overflow);
  hipLaunchKernelGGL(sparse_fill_kernel, dim3(nblk), dim3(256), 0, s, cnt, T, R3, sums, (int)cap, voxel, index, offsets);
  hipLaunchKernelGGL(sparse_nbr_kernel, dim3((unsigned)((cap * 27 + 255) / 256)), dim3(256), 0, s, voxel, index, offsets + B,
                     (int)cap, R, nbr);
  return check_launch("sparse_map");
}

extern "C" int pvcnn_sparse_gather(const float *grid, const int32_t *voxel, const int32_t *count, int B, int C, int R, long long cap,
                                   float *rows, void *stream) {
  PVCNN_REQUIRE(sparse_supported(B, R), "B >= 1, 1 <= R <= 128 and B R^3 < 2^31 expected");
  PVCNN_REQUIRE(conv_sizes_ok(cap, C, C) && C <= 64 * 65535, "cap in [1, 2^31 / 27) and C >= 1 expected");
  PVCNN_REQUIRE(grid && voxel && count && rows, "null pointer");
  hipLaunchKernelGGL(sparse_gather_kernel, dim3((unsigned)((cap + 63) / 64), (unsigned)((C + 63) / 64)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), grid, voxel, count, (int)cap, C, R * R * R, (long long)B * R * R * R, rows);
  return check_launch("sparse_gather");
}

extern "C" int pvcnn_sparse_scatter(const float *rows, const int32_t *index, const int32_t *count, int B, int C, int R, long long cap,
                                    float *grid, void *stream) {
  PVCNN_REQUIRE(sparse_supported(B, R), "B >= 1, 1 <= R <= 128 and B R^3 < 2^31 expected");
  PVCNN_REQUIRE(conv_sizes_ok(cap, C, C) && C <= 64 * 65535, "cap in [1, 2^31 / 27) and C >= 1 expected");
  PVCNN_REQUIRE(rows && index && count && grid, "null pointer");
  const long long T = (long long)B * R * R * R;
  hipLaunchKernelGGL(sparse_scatter_kernel, dim3((unsigned)((T + 63) / 64), (unsigned)((C + 63) / 64)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), rows, index, count, (int)cap, C, R * R * R, T, grid);
  return check_launch("sparse_scatter");
}

extern "C" int pvcnn_sparse_conv3d_weight_transform(const float *w, int Co, int Ci, int for_bwd_data, float *wt, void *stream) {
  PVCNN_REQUIRE(conv_sizes_ok(1, Ci, Co), "channel counts in [1, 4096] expected");
  PVCNN_REQUIRE(w && wt, "null pointer");
  hipLaunchKernelGGL(sparse_weight_transform_kernel, dim3((unsigned)((Co * Ci * 27 + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), w, Co, Ci, for_bwd_data, wt);
  return check_launch("sparse_conv3d_weight_transform");
}

extern "C" int pvcnn_sparse_conv3d_fwd(const float *x, const float *wt, const float *bias, const int32_t *nbr, const int32_t *count,
                                       long long cap, int Ci, int Co, float *y, void *stream) {
  PVCNN_REQUIRE(conv_sizes_ok(cap, Ci, Co), "cap in [1, 2^31 / 27) and channel counts in [1, 4096] expected");
  PVCNN_REQUIRE(x && wt && nbr && count && y, "null pointer");
  const int vec = (Ci % 4 == 0 && aligned16(x)) ? 1 : 0;
  const dim3 grid((unsigned)((cap + kSpRows - 1) / kSpRows), (unsigned)((Co + kSpCo - 1) / kSpCo));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (Ci <= 16)
    hipLaunchKernelGGL(sparse_conv_kernel<16>, grid, dim3(256), 0, s, x, wt, bias, nbr, count, (int)cap, Ci, Co, vec, g_sparse_skip, y);
  else
    hipLaunchKernelGGL(sparse_conv_kernel<32>, grid, dim3(256), 0, s, x, wt, bias, nbr, count, (int)cap, Ci, Co, vec, g_sparse_skip, y);
  return check_launch("sparse_conv3d_fwd");
}

extern "C" size_t pvcnn_sparse_conv3d_bwd_weight_workspace_bytes(long long cap, int Ci, int Co) {
  if (!conv_sizes_ok(cap, Ci, Co)) return 0;
  const size_t P = (size_t)((cap + kSpWgChunk - 1) / kSpWgChunk);
  return P * ((size_t)27 * Co * Ci + Co) * sizeof(float);
}

extern "C" int pvcnn_sparse_conv3d_bwd_weight(const float *x, const float *grad_y, const int32_t *nbr, const int32_t *count,
                                              long long cap, int Ci, int Co, float *grad_w, float *grad_bias, void *workspace,
                                              size_t workspace_bytes, void *stream) {
  PVCNN_REQUIRE(conv_sizes_ok(cap, Ci, Co), "cap in [1, 2^31 / 27) and channel counts in [1, 4096] expected");
  PVCNN_REQUIRE(x && grad_y && nbr && count && workspace, "null pointer");
  PVCNN_REQUIRE(workspace_bytes >= pvcnn_sparse_conv3d_bwd_weight_workspace_bytes(cap, Ci, Co) && aligned16(workspace),
                "workspace too small or not 16-byte aligned");
  if (!grad_w && !grad_bias) return 0;
  const int P = (int)((cap + kSpWgChunk - 1) / kSpWgChunk);
  PVCNN_REQUIRE((long long)((Co + 63) / 64) * ((Ci + 63) / 64) <= 65535, "too many channel tiles");
  float *part = static_cast<float *>(workspace);
  float *part_b = part + (size_t)P * 27 * Co * Ci;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int vecx = (Ci % 4 == 0 && aligned16(x)) ? 1 : 0, vecg = (Co % 4 == 0 && aligned16(grad_y)) ? 1 : 0;
  hipLaunchKernelGGL(sparse_wgrad_kernel, dim3((unsigned)P, 27, (unsigned)(((Co + 63) / 64) * ((Ci + 63) / 64))), dim3(256), 0, s, x,
                     grad_y, nbr, count, (int)cap, Ci, Co, vecx, vecg, g_sparse_skip, part, part_b);
  hipLaunchKernelGGL(sparse_wgrad_reduce_kernel, dim3((unsigned)((27 * Co * Ci + Co + 255) / 256)), dim3(256), 0, s, part, part_b, P,
                     Ci, Co, grad_w, grad_bias);
  return check_launch("sparse_conv3d_bwd_weight");
}
