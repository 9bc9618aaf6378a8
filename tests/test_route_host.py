"""The launch plans of csrc/route.h (which kernel, tile, grid and how many BatchNorm partial-sum slots the split Conv3d / 1x1 GEMM take)
on the CPU: the library's host-only queries over the sweep of tests/golden/routes.json equal what the commit before the plans returned,
except where pvcnn_conv3d_fwd_split_route now reports the persistent kernel it used to be blind to; and tools/route_table.cpp -- route.h
compiled ALONE by g++ -- prints the same plans the library answers with.

Where the persistent Conv3d kernel runs is computed here from its documented rule, not from the plan: f16x2 (nsplit 2); R = 32 (R = 16
only with PVCNN_CONV_WIDE16=1); Ci % 16 == 0; Ci >= 32; Co > 32; the larger tensor under 4 GiB; PVCNN_CONV_WIDE not 0.  Its tile is
4 x 4 x R voxels (n_tiles = B * (R / 4)^2): 512 at R = 32, 256 at R = 16.  Likewise the persistent 1x1 GEMM: f16x2; K % 64 == 0;
M >= 256 with an even number of 128-row blocks; N % 256 == 0; under 4 GiB; 512-row items where the blocks are a multiple of four and
K >= 256 (never with PVCNN_PW_WIDE=2), else 256-row items; every other launch has 128-row items for M > 64 and 64-row ones below."""
import itertools
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

GOLDEN = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'routes.json')))
AXES = GOLDEN['axes']
PW_CHANNELS = AXES['C'] + [512, 1024, 1472]          # tools/route_table.cpp's 1x1 sweep


def first(name):
    return os.environ.get(name, '')[:1]


def env_switches():
    """(conv_wide, conv_wide16, pw_wide) as csrc/api.hip reads them"""
    return first('PVCNN_CONV_WIDE') != '0', first('PVCNN_CONV_WIDE16') == '1', {'0': 0, '2': 2}.get(first('PVCNN_PW_WIDE'), 1)


def conv_is_wide(b, ci, co, r, nsplit, conv_wide, conv_wide16):
    return (conv_wide and nsplit == 2 and (r == 32 or (r == 16 and conv_wide16)) and ci % 16 == 0 and ci >= 32 and co > 32
            and b * max(ci, co) * r ** 3 * 4 < 0xffffffff)


def pw_rows(b, k, m, n, nsplit, pw_wide):
    blocks = (m + 127) // 128
    if (pw_wide and nsplit == 2 and k % 64 == 0 and m >= 256 and blocks % 2 == 0 and n % 256 == 0
            and b * max(k, m) * n * 4 < 0xffffffff):
        return 512 if pw_wide != 2 and blocks % 4 == 0 and k >= 256 else 256
    return 128 if m > 64 else 64


def product(*axes):
    return itertools.product(*(AXES[a] for a in axes))


@pytest.fixture(scope='module')
def lib():
    from pvcnn_amd import _lib
    return _lib.load()


def test_the_queries_equal_the_commit_before_the_plans_over_the_whole_sweep(lib):
    assert GOLDEN['abi_version'] == 16 and len(GOLDEN['conv_route']) == 8 * 12 * 12 * 8 * 3
    for args, want in zip(product('B', 'C', 'R', 'nsplit'), GOLDEN['conv_stats_parts']):
        assert lib.pvcnn_conv3d_fwd_split_stats_parts(*args) == want, args
    for args, want in zip(product('B', 'N'), GOLDEN['pw_stats_parts']):
        assert lib.pvcnn_pwconv_fwd_split_stats_parts(*args) == want, args
    for args, want in zip(product('B', 'C', 'C', 'R'), GOLDEN['conv_wgrad_bytes']):
        assert lib.pvcnn_conv3d_bwd_weight_f16_workspace_bytes(*args) == want, args
    for args, want in zip(product('B', 'C', 'C', 'N'), GOLDEN['pw_wgrad_bytes']):
        assert lib.pvcnn_pwconv_bwd_weight_f16_workspace_bytes(*args) == want, args
    conv_wide, conv_wide16, _ = env_switches()
    served = 0
    for args, want in zip(product('B', 'C', 'C', 'R', 'nsplit'), GOLDEN['conv_route']):
        got = lib.pvcnn_conv3d_fwd_split_route(*args)
        if conv_is_wide(*args, conv_wide, conv_wide16):
            served += 1
            assert got >> 8 == 4 * 4 * args[3] and got & 0xff == want & 0xff == 64, (args, got, want)
        else:
            assert got == want, (args, got, want)
    # (B x Ci in {32, 48, 64, 96, 128, 256} x Co in {48 .. 256} at R = 32, and as many at R = 16 when that route is switched on)
    assert served == 8 * 6 * 5 * (int(conv_wide) + int(conv_wide and conv_wide16))


def test_the_1x1_route_follows_its_documented_rule(lib):
    pw_wide = env_switches()[2]
    seen = set()
    for b, k, m, n, nsplit in itertools.product(AXES['B'], PW_CHANNELS, PW_CHANNELS, AXES['N'], AXES['nsplit']):
        got = lib.pvcnn_pwconv_fwd_split_route(b, k, m, n, nsplit)
        assert got == pw_rows(b, k, m, n, nsplit, pw_wide), (b, k, m, n, nsplit, got)
        seen.add(got)
    assert seen == ({64, 128, 256, 512} if pw_wide == 1 else {64, 128, 256} if pw_wide else {64, 128})
    assert lib.pvcnn_pwconv_fwd_split_route(0, 64, 64, 256, 2) == 0 and lib.pvcnn_pwconv_fwd_split_route(1, 64, 64, 256, 4) == 0


def route_table(binary, *switch_args):
    text = subprocess.run([binary, *map(str, switch_args)], check=True, capture_output=True, text=True).stdout
    conv, pw = {}, {}
    for line in text.splitlines():
        kind, *v = line.split()
        v = [int(t) for t in v]
        (conv if kind == 'conv' else pw)[tuple(v[:5])] = v[5:]
    assert len(conv) == len(GOLDEN['conv_route']) and len(pw) == 8 * len(PW_CHANNELS) ** 2 * 7 * 3
    return conv, pw


def test_route_h_compiles_alone_and_its_plans_are_what_the_library_answers(lib, tmp_path):
    assert shutil.which('g++'), 'g++ is needed to compile tools/route_table.cpp'
    binary = str(tmp_path / 'route_table')
    subprocess.run(['g++', '-std=c++17', '-Wall', '-Wextra', '-Werror', os.path.join(ROOT, 'tools', 'route_table.cpp'), '-o', binary], check=True)
    conv_wide, conv_wide16, pw_wide = env_switches()
    conv, pw = route_table(binary, int(conv_wide), int(conv_wide16), pw_wide)
    for (b, ci, co, r, nsplit), (kernel, tx, ty, tz, rows, grid_x, grid_y, slots, written, fits) in conv.items():
        assert slots == lib.pvcnn_conv3d_fwd_split_stats_parts(b, co, r, nsplit)
        assert ((tx * ty * tz) << 8) | rows == lib.pvcnn_conv3d_fwd_split_route(b, ci, co, r, nsplit)
        # the slots the caller allocates against the slots the kernel fills with sums: the persistent kernel (3) alone may fill half
        # (its epilogue zero-fills the other half), every other kernel fills all and has one workgroup per slot and 64-row block
        if kernel == 3:
            assert conv_is_wide(b, ci, co, r, nsplit, conv_wide, conv_wide16) and written == b * (r // 4) ** 2 and slots in (written, 2 * written)
            assert grid_y == 1 and grid_x == 8 * min(32, (written + 7) // 8 * ((co + 63) // 64))
        else:
            assert not conv_is_wide(b, ci, co, r, nsplit, conv_wide, conv_wide16)
            assert written == slots == grid_x and grid_y == (co + 63) // 64
        assert fits == (b * max(ci, co) * r ** 3 * 4 < 0xffffffff)
    for (b, k, m, n, nsplit), (kernel, rows, grid, slots, fits) in pw.items():
        assert rows == lib.pvcnn_pwconv_fwd_split_route(b, k, m, n, nsplit)
        assert slots == lib.pvcnn_pwconv_fwd_split_stats_parts(b, n) == b * ((n + 255) // 256)
        assert (kernel == 2) == (rows >= 256) and fits == 1
        assert grid == (8 * min(32, (slots + 7) // 8 * ((m + 127) // 128 * 128 // rows)) if kernel == 2 else (slots + 7) // 8 * 8 * ((m + rows - 1) // rows))

    # the switches, without a process per setting: the same program with the values they stand for
    golden_route = dict(zip(product('B', 'C', 'C', 'R', 'nsplit'), GOLDEN['conv_route']))
    off_conv, off_pw = route_table(binary, 0, 0, 0)
    for key, (kernel, tx, ty, tz, rows, *_rest) in off_conv.items():
        assert kernel != 3 and ((tx * ty * tz) << 8) | rows == golden_route[key], key     # PVCNN_CONV_WIDE=0: the two-workgroup tile
    assert {v[1] for v in off_pw.values()} == {64, 128}
    on_conv, on_pw = route_table(binary, 1, 1, 2)
    for key, (kernel, tx, ty, tz, rows, *_rest) in on_conv.items():
        wide = conv_is_wide(*key, True, True)
        assert (kernel == 3) == wide, key
        assert ((tx * ty * tz) << 8) | rows == (((16 * key[3]) << 8) | 64 if wide else golden_route[key]), key
    assert sum(v[0] == 3 and key[3] == 16 for key, v in on_conv.items()) == 8 * 6 * 5      # the opt-in R = 16 route is exercised
    for key, v in on_pw.items():
        assert v[1] == pw_rows(*key, 2), key
