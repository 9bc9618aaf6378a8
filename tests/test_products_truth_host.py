"""tests/products_truth.py proven on the CPU before it judges a kernel: the integer model of the bf16 rounding against torch's own,
the exactness of the three-way bf16 split and of the f16x2 scaling on the value sets the GPU tests draw, the one-product
expectations against fp64 convolutions, and the coverage guard -- every instantiation csrc/route.h selects over a sweep of shapes is
taken by a row of ROUTE_CASES, and every row takes the instantiation it is listed for (tools/route_table.cpp, stdin mode)."""
import itertools
import json
import os
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

import products_truth as pt
from conftest import ROOT


# ---- the conversions ---------------------------------------------------------------------------------------------------------------

def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_bf16_rne_is_torchs_bfloat16_rounding(gen):
    ties, extreme = pt.tie_set(), pt.extreme_set()
    for t in (torch.randn(1 << 20, generator=gen), pt.decade_normals((2, 9, 4096), gen), ties, extreme,
              ties * 2.0 ** 40, ties * 2.0 ** -40):
        assert _same_bits(pt.bf16_rne(t), t.bfloat16().float())
    bits = lambda v: v.view(torch.int32).to(torch.int64) & 0xffffffff
    # a tie goes to the even upper half, whichever side that is; one ulp off a tie goes to the nearer one
    want = {0x3f808000: 0x3f80, 0x3f818000: 0x3f82, 0x3f807fff: 0x3f80, 0x3f808001: 0x3f81, 0x3f817fff: 0x3f81, 0x3f818001: 0x3f82,
            0x3fff8000: 0x4000, 0x3fffc000: 0x4000, 0x3f7fffff: 0x3f80}                      # the last three: into the next binade
    got = dict(zip(bits(ties).tolist(), (bits(pt.bf16_rne(ties)) >> 16).tolist()))
    for u, hi in want.items():
        assert got[u] == hi and got[u | 0x80000000] == hi | 0x8000, hex(u)
    # the largest finite fp32 rounds to infinity, the largest value below that tie stays finite
    big = dict(zip(bits(extreme).tolist(), (bits(pt.bf16_rne(extreme)) >> 16).tolist()))
    assert big[0x7f7fffff] == 0x7f80 and big[0x7f7f8000] == 0x7f80 and big[0x7f7f7fff] == 0x7f7f and big[0x7f7e8000] == 0x7f7e


def _gpu_value_sets(gen):
    """What tests/test_gpu_products_exact.py multiplies in the fp32 / bf16 / bf16x3 modes."""
    yield pt.decade_normals((2, 16, 12, 12, 12), gen, ties=True)
    yield pt.decade_normals((1, 130, 513), gen, ties=True)
    yield torch.randn(64, 27, generator=gen)                                  # the weights of the second variant
    yield torch.randn(1 << 20, generator=gen)
    yield pt.tie_set()


def test_three_bf16_pieces_sum_back_in_the_order_of_the_product_ladder(gen):
    """split_products<3> adds, for a one-piece other factor q, p2 * q, then p1 * q, then p0 * q: (p2 + p1) + p0 must be the value."""
    for v in _gpu_value_sets(gen):
        p0, p1, p2 = pt.split3_bf16(v)
        for p in (p0, p1, p2):
            assert _same_bits(pt.bf16_rne(p), p)                              # each piece IS a bf16 number
        assert torch.equal((p2 + p1) + p0, v)
        assert torch.equal((p2.double() + p1.double()) + p0.double(), v.double())     # (and nothing was lost to an fp32 rounding)
        for q in (0.25, -8.0):                                                # times a power of two: still exact
            assert torch.equal((p2 * q + p1 * q) + p0 * q, v * q)
    one = pt.signed_pow2((4096,), gen)
    p0, p1, p2 = pt.split3_bf16(one)
    assert torch.equal(p0, one) and not p1.any() and not p2.any()             # a power of two is one piece


def test_short_integers_survive_the_f16x2_scaling(gen):
    for shift in (-20, -3, 0, 5, 30):
        for bound in (1023, 255, 1):
            v = pt.short_ints((1 << 16,), gen, bound, shift)
            v[0] = bound * 2.0 ** shift
            hi, lo, s = pt.f16x2_pieces(v)
            assert 2.0 ** 13 <= v.abs().max().item() * 2.0 ** s < 2.0 ** 14
            assert torch.equal(hi * 2.0 ** -s, v) and not lo.any()
            # under a larger maximum of the same tensor (a tile's scale is the maximum of the rows it touches) as well
            hi, lo, s = pt.f16x2_pieces(v, absmax=1023 * 2.0 ** shift)
            assert torch.equal(hi * 2.0 ** -s, v) and not lo.any()
    p = pt.signed_pow2((4096,), gen, zeros=True)
    hi, lo, s = pt.f16x2_pieces(p)
    assert torch.equal(hi * 2.0 ** -s, p) and not lo.any()
    # and a value with twelve significant bits does not: the model would notice
    hi, lo, s = pt.f16x2_pieces(torch.tensor([2049.0, 4096.0]))
    assert lo.any()


def test_exact_sum_bound():
    for count in (2 * 32 ** 3, 3 * 12 ** 3, 2 * 260):
        assert pt.exact_sum_bound(count) * count < 1 << 24 and (pt.exact_sum_bound(count) == 1023 or (pt.exact_sum_bound(count) + 1) * count >= 1 << 24)


# ---- the one-product expectations against fp64 -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('b,ci,co,r', [(2, 5, 7, 6), (1, 16, 24, 8), (2, 8, 3, 5)])
def test_single_product_weights_make_shifted_copies(gen, b, ci, co, r):
    x = pt.decade_normals((b, ci, r, r, r), gen, ties=True).double()
    gy = pt.decade_normals((b, co, r, r, r), gen).double()
    seen = set()
    for taps in pt.tap_groups(min(ci, co), gen):
        w, live = pt.single_product_weights(co, ci, taps, gen, pt.signed_pow2((27,), gen))
        assert (w != 0).sum().item() == len(live) == len(taps) <= min(ci, co)
        assert ((w != 0).sum(dim=(1, 2, 3, 4)) <= 1).all() and ((w != 0).sum(dim=(0, 2, 3, 4)) <= 1).all()
        assert [t for _, _, t, _ in live] == taps and all(w[o, c][pt.TAPS[t]] == v for o, c, t, v in live)
        seen.update(taps)
        xd = x.clone().requires_grad_()
        y = F.conv3d(xd, w.double(), padding=1)
        y.backward(gy)
        assert torch.equal(y.detach(), pt.single_product_forward(x, live, co))
        assert torch.equal(xd.grad, pt.single_product_backward_data(gy, live, ci))
    assert seen == set(range(27))
    # shift3d by hand: tap (0, 1, 2) reads x[p + (-1, 0, +1)]
    s = pt.shift3d(x, pt.TAPS.index((0, 1, 2)))
    assert torch.equal(s[..., 1:, :, :-1], x[..., :-1, :, 1:]) and not s[..., 0, :, :].any() and not s[..., :, :, -1].any()


def test_single_product_weights_of_a_1x1_product(gen):
    x, gy = pt.decade_normals((2, 9, 37), gen).double(), pt.decade_normals((2, 13, 37), gen).double()
    w, live = pt.single_product_weights(13, 9, None, gen, torch.randn(9, generator=gen))
    assert len(live) == 9 and ((w != 0).sum(dim=1) <= 1).all() and ((w != 0).sum(dim=0) <= 1).all()
    xd = x.clone().requires_grad_()
    y = F.conv1d(xd, w.double().unsqueeze(-1))
    y.backward(gy)
    assert torch.equal(y.detach(), pt.single_product_forward(x, live, 13))
    assert torch.equal(xd.grad, pt.single_product_backward_data(gy, live, 9))
    rounded = pt.bf16_rne(torch.tensor([v for *_, v in live]))
    assert torch.equal(pt.single_product_forward(x, live, 13, weights=rounded), F.conv1d(x, pt.bf16_rne(w).double().unsqueeze(-1)))


@pytest.mark.parametrize('b,ci,co,r', [(2, 9, 5, 8), (1, 40, 3, 12), (2, 16, 4, 32)])
def test_live_voxels_give_one_product_per_weight_gradient(gen, b, ci, co, r):
    positions = pt.voxel_positions(b, r)
    assert len(positions) == len(set(positions)) == len({0, b - 1}) * 2 * 4 * (4 if r == 32 else 2)
    assert {p[3] for p in positions} >= ({0, 15, 16, 31} if r == 32 else {0, r - 1}) and {p[2] for p in positions} == {0, 3, 4, r - 1}
    bound = pt.exact_sum_bound(b * r ** 3)
    gy = pt.short_ints((b, co, r, r, r), gen, bound)
    for launch in range(2):
        x, live = pt.live_voxel_inputs(b, ci, r, gen, pt.rotated(positions, launch * ci))
        assert ((x != 0).sum(dim=(0, 2, 3, 4)) == 1).all() and x.abs().max() <= 1023 and torch.equal(x, x.round())
        want = pt.live_voxel_grad_w(live, gy)
        assert torch.equal(torch.nn.grad.conv3d_weight(x.double(), (co, ci, 3, 3, 3), gy.double(), padding=1), want.double())
        assert want.abs().max() < 1 << 24 and (want == 0).any() and (want != 0).any()      # border positions lose taps
    assert gy.double().sum(dim=(0, 2, 3, 4)).abs().max() < 1 << 24 and gy.abs().sum(dim=(0, 2, 3, 4)).max() < 1 << 24


def test_live_points_give_one_product_per_weight_gradient(gen):
    for b, ci, co, n in [(2, 9, 24, 260), (3, 40, 7, 516)]:
        positions = pt.point_positions(b, n)
        assert {p[1] for p in positions} == {0, 255, 256, n - 1}
        gy = pt.short_ints((b, co, n), gen, pt.exact_sum_bound(b * n))
        x, live = pt.live_point_inputs(b, ci, n, gen, positions)
        assert ((x != 0).sum(dim=(0, 2)) == 1).all()
        want = pt.live_point_grad_w(live, gy)
        assert torch.equal(torch.einsum('bon,bcn->oc', gy.double(), x.double()), want.double())


# ---- the coverage guard --------------------------------------------------------------------------------------------------------------------

SWEEP_B = [1, 2, 3, 5, 8, 16, 20, 22, 32, 40, 48, 64, 90, 128, 130]
SWEEP_R = [2, 4, 5, 6, 8, 10, 12, 16, 20, 32, 33]
SWEEP_N = [1, 4, 37, 255, 256, 262, 300, 512, 1024, 4100]


@pytest.fixture(scope='module')
def plans(tmp_path_factory):
    """-> ask(lines): the plans tools/route_table.cpp (route.h compiled alone, default switches) prints for `conv B Ci Co R nsplit` /
    `pw B K M N nsplit [x_vec_ok]` lines, as signatures of products_truth."""
    assert shutil.which('g++'), 'g++ is needed to compile tools/route_table.cpp'
    binary = str(tmp_path_factory.mktemp('route') / 'route_table')
    subprocess.run(['g++', '-std=c++17', '-Wall', '-Wextra', '-Werror', os.path.join(ROOT, 'tools', 'route_table.cpp'), '-o', binary], check=True)

    def ask(lines):
        text = subprocess.run([binary, '-'], input='\n'.join(lines) + '\n', check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(text) == len(lines)
        out = []
        for asked, line in zip(lines, text):
            kind, *v = line.split()
            v = [int(t) for t in v]
            assert asked.split()[:6] == [kind, *map(str, v[:5])]
            if kind == 'conv':      # B Ci Co R nsplit  kernel tx ty tz rows grid_x grid_y stats_slots tiles_written offsets32 vec
                out.append(pt.conv_signature(v[5], v[4], v[6], v[7], v[8], v[15], v[9]))
            else:                   # B K M N nsplit  kernel rows grid stats_slots offsets32 vec mb pf wmw
                out.append(pt.pw_signature(v[5], v[4], v[11], v[12], v[13], v[10]))
        return out
    return ask


def test_every_route_case_takes_the_instantiation_it_is_listed_for(plans):
    keys = [(row, d, ns) for row in pt.ROUTE_CASES for d in ('fwd', 'bwd') for ns in (1, 2, 3)]
    lines = [f"{row['kind']} " + ' '.join(map(str, pt.direction_shape(row, d))) + f' {ns}' for row, d, ns in keys]
    for (row, d, ns), got in zip(keys, plans(lines)):
        assert got == row['listed'][d, ns], (row['id'], d, ns, got)
    assert len({row['id'] for row in pt.ROUTE_CASES}) == len(pt.ROUTE_CASES)
    # the rows no other kernel-level test reaches carry their tile in the id the GPU tests are named by
    unreached = {row['id'] for row in pt.ROUTE_CASES if row['unreached']}
    assert unreached == {'conv-90x3x8x6-tile2x8x8-scalar', 'conv-130x3x8x5-tile4x8x8-scalar', 'conv-8x9x64x32-tile4x4x32-vec'}
    by_id = {row['id']: row for row in pt.ROUTE_CASES}
    assert by_id['conv-8x9x64x32-tile4x4x32-vec']['listed']['fwd', 2] == 'igemm<2,4,4,32,vec>r64'
    for ns in (1, 2, 3):
        assert by_id['conv-90x3x8x6-tile2x8x8-scalar']['listed']['fwd', ns] == f'igemm<{ns},2,8,8,scalar>r64'
        assert by_id['conv-130x3x8x5-tile4x8x8-scalar']['listed']['fwd', ns] == f'igemm<{ns},4,8,8,scalar>r64'


def test_route_cases_reach_every_instantiation_of_the_sweep(plans):
    """Default switches (the opt-in PVCNN_CONV_WIDE16 route stays with tests/test_gpu_conv_wide.py).  The set is computed, not counted
    by hand; it is printed so that a run shows what was checked."""
    channels = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'routes.json')))['axes']['C']
    conv = [f'conv {b} {ci} {co} {r} {ns}' for b, ci, co, r, ns in itertools.product(SWEEP_B, channels, channels, SWEEP_R, (1, 2, 3))]
    gemm_channels = sorted(set(channels) | {1, 512, 1024, 1472})
    pw = [f'pw {b} {k} {m} {n} {ns} {aligned}'
          for b, k, m, n, ns, aligned in itertools.product(SWEEP_B, gemm_channels, gemm_channels, SWEEP_N, (1, 2, 3), (1, 0))]
    swept = {'conv': set(plans(conv)), 'pw': set(plans(pw))}
    for kind in ('conv', 'pw'):
        listed = {sig for row in pt.ROUTE_CASES if row['kind'] == kind for sig in row['listed'].values()}
        print(f'[coverage guard] {kind}: {len(swept[kind])} signatures over the sweep, {len(listed)} in ROUTE_CASES')
        for sig in sorted(swept[kind]):
            print(f'[coverage guard]   {sig}')
        assert swept[kind] <= listed, f'{kind}: no ROUTE_CASES row takes {sorted(swept[kind] - listed)}'
        assert listed <= swept[kind], f'{kind}: ROUTE_CASES lists {sorted(listed - swept[kind])}, which the sweep never meets'
