// route.h -- the launch plans of the split (f16x2 / bf16 / bf16x3) forward and backward-data ops: which kernel runs, on which tile,
// on which grid, and how many BatchNorm partial-sum slots per channel the caller allocates.  ONE function per op; the stats_parts and
// route queries and the launch itself (conv3d_bf16.hip, pointwise_bf16.hip) all read its result.  Host-only, plain C++17, no HIP
// include: tools/route_table.cpp compiles it alone and tests/test_route_host.py checks it on a CPU.
#pragma once
#include <stddef.h>

#include <algorithm>

#include "switches.h"

namespace pvcnn {
namespace route {

// (the kernels' own constants; the translation units that launch from a plan static_assert that these equal theirs)
constexpr int kNumCU = 256;        // MI355X
constexpr int kCoTileB = 64;       // Conv3d: output channels (weight rows) per workgroup tile
constexpr int kKc = 16;            // Conv3d: input channels per chunk
constexpr int kPbN = 256;          // 1x1 GEMM: points per workgroup tile

constexpr int ceil_div(int a, int b) { return (a + b - 1) / b; }

// ---- Conv3d -----------------------------------------------------------------------------------------------------------------------

// Workgroup tile and staging path.  Vector staging (whole z rows as 16-byte loads) needs R % 4 == 0 and a tile that spans z:
// tz = 8 / 16 / 32 for R <= 8 / 16 / 32.  At 16 < R <= 32 a 512-voxel tile (a wave owns 64 channels x 128 voxels: every weight
// fragment feeds four MFMA column blocks, the halo overhead drops from 3.0x to 2.25x) when that still leaves two workgroups for
// every CU; the six-product bf16x3 mode has neither the registers nor the LDS for it.  (Measured, (16,64,64,32^3), f16x2:
// scalar staging 0.354 ms, vector 0.320 ms, vector + 512-voxel tile 0.309 ms; a (4,8,16) tile at R = 16 spills and loses.)
struct SplitTile { int tx, ty, tz; bool vec; };
inline SplitTile split_tiles(int B, int Co, int R, int nsplit) {
  const bool vec = R % 4 == 0 && R <= 32;
  if (R <= 8) {  // tiny grids (PVCNN++ at R = 8, B = 8: 16 tiles of 256 voxels per 64 channels): halve the tile while the chip is not full
    const long per = (long)B * ceil_div(R, 8) * ceil_div(Co, kCoTileB);
    // (measured, f16x2 forward, (8,128,128,8): 38.5 -> 28.4 us; (8,256,256,8): 71.3 -> 61.6; PVCNN++ step 574.7 -> 581.0 clouds/s in one call)
    if (per * ceil_div(R, 2) < kNumCU) return SplitTile{1, 8, 8, vec};
    return per * ceil_div(R, 4) < kNumCU ? SplitTile{2, 8, 8, vec} : SplitTile{4, 8, 8, vec};
  }
  if (!vec) return {4, 4, 16, false};
  if (R <= 16)   // too few 256-voxel tiles to give every SIMD two waves (R = 16, B = 16: 256 per 64 channels): halve them
    return (long)B * ceil_div(R, 4) * ceil_div(R, 4) * ceil_div(Co, kCoTileB) < 768 ? SplitTile{2, 4, 16, true} : SplitTile{4, 4, 16, true};
  const bool big = nsplit != 3 && (long)B * ceil_div(R, 4) * ceil_div(R, 4) * ceil_div(Co, kCoTileB) >= 512;
  return big ? SplitTile{4, 4, 32, true} : SplitTile{2, 4, 32, true};
}

enum class ConvKernel {
  Igemm,       // conv3d_igemm_bf16_kernel<nsplit, tx, ty, tz, vec>: several workgroups per CU, one tile each
  IgemmCo32,   // ... with a 32-row weight tile: no MFMAs on the padded half (f16x2, the default arithmetic, only)
  Pipe,        // conv3d_igemm_f16_pipe_kernel<2, 4>: the pipelined 128-voxel kernel (f16x2 only).  Round 3, 64 -> 64 at 16^3 x 16: see
               // profiles/ab/r03u_convbench.jsonl
  Wide,        // conv3d_igemm_f16_wide_kernel<R>: round 6, whole 16-channel chunks at R = 32 / 16, one persistent workgroup per CU
};

struct ConvFwdPlan {
  ConvKernel kernel;
  int tx, ty, tz;        // voxels of a workgroup's tile (Wide: of an item, always 4 x 4 x R)
  bool vec;              // Igemm: z rows staged as 16-byte loads (x must be 16-byte aligned)
  int rows;              // weight rows (output channels) per item
  unsigned grid_x, grid_y;
  // BatchNorm partial sums, per channel.  stats_slots is what the caller allocates and bn_finalize sums over (the bits of the
  // statistics depend on the count): ALWAYS the tile count of split_tiles()'s tile, whichever kernel runs.  tiles_written is how many
  // of them the kernel fills with sums: all of them, except the Wide kernel where a small batch would have taken the 256-voxel
  // (2, 4, 32) tile -- then stats_slots == 2 * tiles_written and the kernel's epilogue writes zeros to the surplus half.
  size_t stats_slots;
  size_t tiles_written;
  bool offsets32;        // every byte offset inside x and y fits 32 bits: what the Wide kernel's buffer descriptors address
};

inline ConvFwdPlan conv3d_fwd_split_plan(int B, int Ci, int Co, int R, int nsplit, const Switches &sw) {
  const SplitTile t = split_tiles(B, Co, R, nsplit);
  ConvFwdPlan p;
  p.kernel = ConvKernel::Igemm;
  p.tx = t.tx; p.ty = t.ty; p.tz = t.tz; p.vec = t.vec;
  p.rows = kCoTileB;
  const long tiles = (long)B * ceil_div(R, t.tx) * ceil_div(R, t.ty) * ceil_div(R, t.tz);
  p.grid_x = (unsigned)tiles; p.grid_y = (unsigned)ceil_div(Co, kCoTileB);
  p.stats_slots = p.tiles_written = (size_t)tiles;
  p.offsets32 = (long)B * std::max(Ci, Co) * R * R * R * 4 < 0xffffffffL;
  // (R = 16: measured -- tools/calls_r06/r06_call10: 6 .. 9 % faster per launch than conv3d_igemm_f16_pipe_kernel, 44.8 / 80.2 / 144.0 us
  //  against 47.6 / 87.5 / 156.3 at 64 -> 64 / 64 -> 128 / 128 -> 128, but nothing in the step: 6.076 / 6.083 ms with, 6.066 / 6.060
  //  without -- one item per workgroup at Co = 64, nothing for the persistence to hide.  Opt-in: PVCNN_CONV_WIDE16=1; tested either way)
  if (sw.conv_wide && nsplit == 2 && (R == 32 || (R == 16 && sw.conv_wide16)) && Co > 32 && Ci % kKc == 0 && Ci >= 2 * kKc &&
      p.offsets32) {
    const int cotiles = ceil_div(Co, kCoTileB), n_tiles = B * (R / 4) * (R / 4);
    const long per_xcd = (long)((n_tiles + 7) / 8) * cotiles;
    p.kernel = ConvKernel::Wide;
    p.tx = 4; p.ty = 4; p.tz = R; p.vec = true;
    p.grid_x = 8u * (unsigned)std::min<long>(kNumCU / 8, per_xcd); p.grid_y = 1;
    p.tiles_written = (size_t)n_tiles;
  } else if (t.tz == 16 && t.vec && t.tx == 2 && nsplit == 2 && Ci % kKc == 0) {
    p.kernel = ConvKernel::Pipe;                                 // (the same (2, 4, 16) tile)
  } else if (t.tz == 32 && Co <= 32 && nsplit == 2) {
    p.kernel = ConvKernel::IgemmCo32;
    p.rows = 32;
  }
  return p;
}

// ---- 1x1 GEMM ---------------------------------------------------------------------------------------------------------------------

constexpr int pb_mb(int M) { return M > 64 ? 4 : 2; }     // 32-row blocks of a weight tile (and of the weight image's row padding)

enum class PwKernel {
  Gemm,   // pw_gemm_bf16_kernel<nsplit, mb, pf, vec>
  // measured (profiles/ab/r03k_*, 1472 -> 512 over 65 536 points, forward): round-3 start 0.483 ms; straight-line chunk loop
  // (VEC) 0.347 ms; + conversion between the MFMAs, one barrier per chunk (pipe kernel) 0.306 ms; the step 1925 -> 2103 -> 2108 clouds/s
  Pipe,   // pw_gemm_f16_pipe_kernel<nsplit>: 128 rows, f16x2 or (autocast) bf16 operands: the same pipelined structure with one plane
  Wide,   // pw_gemm_f16_wide_kernel<wmw>: round 6: 256 output channels per workgroup, one persistent workgroup per CU
};

struct PwFwdPlan {
  PwKernel kernel;
  int mb;                // Gemm / Pipe: 32-row blocks of the weight tile
  int pf;                // Gemm: prefetch depth
  int wmw;               // Wide: 128-row blocks of an item (2: 256 x 256 items, 4: 512 x 128), else 0
  bool vec;              // straight-line chunk loop (see the kernels): N % 4 == 0 and x 16-byte aligned
  int rows;              // weight rows (output channels) per item
  int tiles_n;           // 256-point tiles per cloud
  long tiles_total;      // ... of the batch
  long grid;
  size_t stats_slots;    // BatchNorm partial sums per channel: one per point tile; every kernel fills all of them
  bool offsets32;        // every byte offset inside x and y fits 32 bits (buffer descriptors: 32-bit byte offsets inside a tensor)
};

inline PwFwdPlan pwconv_fwd_split_plan(int B, int K, int M, int N, int nsplit, bool x_vec_ok, const Switches &sw) {
  PwFwdPlan p;
  p.kernel = PwKernel::Gemm;
  p.mb = pb_mb(M); p.pf = 1; p.wmw = 0;
  p.vec = N % 4 == 0 && N >= 4 && x_vec_ok;
  p.rows = 32 * p.mb;
  p.tiles_n = ceil_div(N, kPbN);
  p.tiles_total = (long)B * p.tiles_n;
  p.grid = ((p.tiles_total + 7) / 8) * 8 * ceil_div(M, p.rows);       // tiles padded to the 8 XCDs
  p.stats_slots = (size_t)p.tiles_total;
  p.offsets32 = (long)B * std::max(K, M) * N * 4 < 0xffffffffL;
  const int mtiles128 = ceil_div(M, 128);
  if (nsplit == 2 && sw.pw_wide != 0 && p.mb == 4 && p.vec && K % 64 == 0 && N % kPbN == 0 && M >= 256 && mtiles128 % 2 == 0 &&
      p.offsets32) {
    // 512 x 128 items (4 x 1 waves) where the image has a multiple of four 128-row blocks (PVCNN_PW_WIDE=2: the 256 x 256 items only)
    // (K >= 256: with a handful of steps per item -- 128 -> 1024: eight -- the launch is its epilogues and stores, and the 256 x 256
    //  items are faster: 79 vs 94 us, tools/calls_r06/r06_call13)
    p.kernel = PwKernel::Wide;
    p.wmw = (sw.pw_wide != 2 && mtiles128 % 4 == 0 && K >= 256) ? 4 : 2;
    p.rows = 128 * p.wmw;
    const long turns_local = ((p.tiles_total + 7) / 8) * (mtiles128 / p.wmw);      // (a turn = one 256-point tile x one row group)
    p.grid = 8 * std::min<long>(kNumCU / 8, turns_local);
  } else if (nsplit != 3 && p.mb == 4 && p.vec) {
    p.kernel = PwKernel::Pipe;
  } else if (nsplit == 2 && p.mb == 4) {
    // prefetch depth of the wide f16x2 tile, measured (profiles/ab/r03c_pwbench_pf*.jsonl, 1472 -> 512 over 65 536 points): PF = 1 / 2 / 3
    // = 0.576 / 0.538 / 0.523 ms forward, 1788 / 1820 / 1824 clouds/s in the step; PF = 2 is kept (232 VGPRs; PF = 3 needs 252 of 256)
    p.pf = 2;
  }
  return p;
}

}  // namespace route
}  // namespace pvcnn
