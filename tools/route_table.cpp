// route_table.cpp -- the launch plans of pvcnn_amd/csrc/route.h over the sweep of tests/golden/gen_routes_golden.py (the 1x1 GEMM
// with three more channel counts: 512, 1024, 1472 -- the sizes with 512-row items), one line per problem size.
// Includes route.h alone: the plans are host code, checkable without HIP or a GPU.
//   g++ -std=c++17 -fsanitize=address,undefined tools/route_table.cpp -o route_table && ./route_table [conv_wide conv_wide16 pw_wide]
// (the three arguments stand for PVCNN_CONV_WIDE, PVCNN_CONV_WIDE16, PVCNN_PW_WIDE; without them: the defaults)
//   conv B Ci Co R nsplit  kernel tx ty tz rows grid_x grid_y stats_slots tiles_written offsets32
//   pw   B K  M  N nsplit  kernel rows grid stats_slots offsets32                     (x 16-byte aligned)
// tests/test_route_host.py compares the lines with what the library's queries return.
// Second mode, `./route_table - [conv_wide conv_wide16 pw_wide]`: the plans of the problems named on stdin, one per line, as
//   conv B Ci Co R nsplit            -> the conv columns above, then vec
//   pw   B K  M  N nsplit [x_vec_ok] -> the pw columns above, then vec mb pf wmw      (x_vec_ok: x 16-byte aligned, default 1)
// tests/test_products_truth_host.py asks it which instantiation each of its shapes takes.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../pvcnn_amd/csrc/route.h"

int main(int argc, char **argv) {
  using namespace pvcnn;
  Switches sw;
  const bool from_stdin = argc >= 2 && strcmp(argv[1], "-") == 0;
  if (from_stdin) { --argc; ++argv; }
  if (argc == 4) {
    sw.conv_wide = atoi(argv[1]) != 0;
    sw.conv_wide16 = atoi(argv[2]) != 0;
    sw.pw_wide = atoi(argv[3]);
  } else if (argc != 1) {
    fprintf(stderr, "usage: %s [-] [conv_wide conv_wide16 pw_wide]\n", argv[0]);
    return 2;
  }
  if (from_stdin) {
    char line[256], kind[8];
    while (fgets(line, sizeof line, stdin)) {
      int v[6] = {0, 0, 0, 0, 0, 1};
      const int n = sscanf(line, "%7s %d %d %d %d %d %d", kind, &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]);
      if (n == 6 && strcmp(kind, "conv") == 0) {
        const route::ConvFwdPlan p = route::conv3d_fwd_split_plan(v[0], v[1], v[2], v[3], v[4], sw);
        printf("conv %d %d %d %d %d  %d %d %d %d %d %u %u %zu %zu %d %d\n", v[0], v[1], v[2], v[3], v[4], (int)p.kernel, p.tx, p.ty, p.tz,
               p.rows, p.grid_x, p.grid_y, p.stats_slots, p.tiles_written, (int)p.offsets32, (int)p.vec);
      } else if (n >= 6 && strcmp(kind, "pw") == 0) {
        const route::PwFwdPlan p = route::pwconv_fwd_split_plan(v[0], v[1], v[2], v[3], v[4], v[5] != 0, sw);
        printf("pw %d %d %d %d %d  %d %d %ld %zu %d %d %d %d %d\n", v[0], v[1], v[2], v[3], v[4], (int)p.kernel, p.rows, p.grid,
               p.stats_slots, (int)p.offsets32, (int)p.vec, p.mb, p.pf, p.wmw);
      } else if (n > 0) {
        fprintf(stderr, "%s: cannot read '%s'\n", argv[0], line);
        return 2;
      }
    }
    return 0;
  }
  const int Bs[] = {1, 2, 3, 5, 8, 16, 20, 40}, Cs[] = {3, 9, 10, 13, 16, 20, 32, 48, 64, 96, 128, 256};
  const int Rs[] = {4, 6, 8, 12, 16, 20, 32, 33}, Ns[] = {1, 255, 256, 1024, 2048, 4096, 4100};
  for (int B : Bs)
    for (int Ci : Cs)
      for (int Co : Cs)
        for (int R : Rs)
          for (int nsplit = 1; nsplit <= 3; ++nsplit) {
            const route::ConvFwdPlan p = route::conv3d_fwd_split_plan(B, Ci, Co, R, nsplit, sw);
            printf("conv %d %d %d %d %d  %d %d %d %d %d %u %u %zu %zu %d\n", B, Ci, Co, R, nsplit, (int)p.kernel, p.tx, p.ty, p.tz, p.rows,
                   p.grid_x, p.grid_y, p.stats_slots, p.tiles_written, (int)p.offsets32);
          }
  const int PwCs[] = {3, 9, 10, 13, 16, 20, 32, 48, 64, 96, 128, 256, 512, 1024, 1472};
  for (int B : Bs)
    for (int K : PwCs)
      for (int M : PwCs)
        for (int N : Ns)
          for (int nsplit = 1; nsplit <= 3; ++nsplit) {
            const route::PwFwdPlan p = route::pwconv_fwd_split_plan(B, K, M, N, nsplit, true, sw);
            printf("pw %d %d %d %d %d  %d %d %ld %zu %d\n", B, K, M, N, nsplit, (int)p.kernel, p.rows, p.grid, p.stats_slots, (int)p.offsets32);
          }
  return 0;
}
