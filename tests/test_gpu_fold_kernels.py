"""The activation tail of the forward product kernels (csrc/gemm_epilogue.h; include/pvcnn_hip.h: the *_act entry points), kernels
alone -- no fold arithmetic here.  For every shape:

  * the route is read off the library's own queries (pvcnn_conv3d_fwd_split_route / pvcnn_pwconv_fwd_split_route), so a change in the
    ladder cannot quietly drop a kernel from this file's coverage;
  * y_act is torch.equal to leaky_relu(y_plain, slope), y_plain from the existing entry point on the same operands, slope 0 and 0.1;
  * the emitted table is torch.equal to absmax_tiles(y_act, seg, want_global=False)[1:];
  * table slots beyond the tensor's segments stay zero, and so does word [0] (a table-only buffer);
  * HipBackend's *_act methods return the same y and the same table.

Inputs are finite; one input channel carries a 2^10 outlier inside one tile, so a table that took the wrong segment shows, and the
upper half of every grid is exact zeros, so the Conv3d kernels' zero-input-tile shortcut is taken with the tail as well.

Two 1x1 shapes are routed to the persistent wide kernel by the plain entry point; with the tail that kernel would spill, and the *_act
entry point sends them to the 128-row kernels, which compute the same bits (tests/test_gpu_pw_wide.py) -- the equality below holds
across the two.  The wide Conv3d kernel carries the tail itself."""
import pytest
import torch

from pvcnn_amd.modules.functional import backend as seam
from pvcnn_amd.modules.functional._product import CONV, PW

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SLOPES = (0.0, 0.1)
PAD = 3                      # table slots allocated beyond the tensor's segments


def act_call(be, p, name, x, args_front, y_shape, slope, tiles, seg, args_mid=()):
    """One *_act entry point on a table with PAD slots to spare -> (y, the whole table)."""
    y = torch.empty(y_shape, dtype=torch.float32, device=x.device)
    table = torch.zeros((1 + tiles + PAD,), dtype=torch.int32, device=x.device)
    seam._run(p.entry(be.lib, name), name, x, x, *args_front, y, *args_mid, float(slope), table, seg)
    return y, table


def check(be, p, y_plain, y_act, table, slope, seg):
    want = torch.nn.functional.leaky_relu(y_plain, slope)
    assert torch.isfinite(y_plain).all()
    assert torch.equal(y_act, want), (y_act - want).abs().max().item()
    b, l = y_act.shape[0], y_act.shape[2]
    tiles = p.amax_tiles(b, l, seg)
    ref = be.absmax_tiles(y_act.view(b, y_act.shape[1], -1), seg, want_global=False)
    assert ref.numel() == 1 + tiles
    assert torch.equal(table[1:1 + tiles], ref[1:]), (table[1:1 + tiles] != ref[1:]).nonzero().flatten().tolist()[:8]
    assert int(table[0]) == 0 and not table[1 + tiles:].any()
    assert table[1:1 + tiles].max() > 0


def grid_input(b, ci, r, g):
    x = torch.randn(b, ci, r, r, r, generator=g)
    x[:, :, r // 2:] = 0.0                                       # zero-input tiles
    x[b - 1, ci // 2, 1, 2, :] *= 1024.0                          # the outlier: one z row of one channel
    return x.to(DEV)


# (B, Ci, Co, R) -> (voxels of a workgroup tile, weight rows): what pvcnn_conv3d_fwd_split_route answers for nsplit 2
CONV_SHAPES = [
    ((2, 16, 32, 8), (64, 64)),        # conv3d_igemm_bf16_kernel, the 64-voxel tile of small grids
    ((1, 16, 40, 12), (128, 64)),      # the 128-voxel tile with tz = 16 > R: ragged z rows, Co not a multiple of the row tile
    ((1, 16, 40, 10), (256, 64)),      # R % 4 != 0: scalar staging, tz > R
    ((2, 32, 64, 16), (128, 64)),      # conv3d_igemm_f16_pipe_kernel
    ((1, 16, 20, 32), (256, 32)),      # the 32-row weight tile of Co <= 32 at R = 32
    ((1, 32, 64, 32), (512, 64)),      # conv3d_igemm_f16_wide_kernel
    ((1, 32, 96, 32), (512, 64)),      # ... with a half-empty second row tile
    ((64, 16, 64, 8), (128, 64)),      # the (2, 8, 8) tile of R = 8
    ((128, 16, 64, 8), (256, 64)),     # the (4, 8, 8) tile of R = 8: the instantiation with no register to spare
]


@pytest.mark.parametrize('shape,route', CONV_SHAPES, ids=[str(s) for s, _ in CONV_SHAPES])
def test_conv3d_split_kernels_f16x2(hip, shape, route):
    b, ci, co, r = shape
    code = hip.lib.pvcnn_conv3d_fwd_split_route(b, ci, co, r, 2)
    assert (code >> 8, code & 255) == route, (code >> 8, code & 255)
    g = torch.Generator().manual_seed(sum(shape))
    x = grid_input(b, ci, r, g)
    w = (torch.randn(co, ci, 3, 3, 3, generator=g) * 0.1).to(DEV)
    bias = torch.randn(co, generator=g).to(DEV)
    wts, amax = hip._conv_wsplit(w, False, 2), hip.conv_amax(x, want_global=False)
    for bias_ in (bias, None):
        y_plain = hip.conv3d_igemm_split(x, wts, bias_, co, 2, amax=amax)
        for slope in SLOPES:
            y_act, table = act_call(hip, CONV, 'fwd_split_act', x, (wts, bias_, b, ci, co, r, 2, amax, r), y_plain.shape, slope, b * r * r, r,
                                    args_mid=(None,))
            check(hip, CONV, y_plain, y_act, table, slope, r)
    y_be, table_be = hip.conv3d_igemm_split_act(x, wts, None, co, 2, SLOPES[-1], amax=amax)
    assert torch.equal(y_be, y_act) and torch.equal(table_be, table[:table_be.numel()])
    y_be, table_be = hip.conv3d_igemm_split_act(x, wts, None, co, 2, SLOPES[-1], amax=amax, emit_amax=False)
    assert torch.equal(y_be, y_act) and table_be is None


@pytest.mark.parametrize('shape,nsplit', [((2, 16, 32, 8), 1), ((1, 32, 64, 16), 1), ((1, 16, 40, 12), 3)], ids=str)
def test_conv3d_split_kernels_bf16_and_bf16x3(hip, shape, nsplit):
    b, ci, co, r = shape
    g = torch.Generator().manual_seed(sum(shape) + nsplit)
    x = grid_input(b, ci, r, g)
    w = (torch.randn(co, ci, 3, 3, 3, generator=g) * 0.1).to(DEV)
    bias = torch.randn(co, generator=g).to(DEV)
    wts = hip._conv_wsplit(w, False, nsplit)
    y_plain = hip.conv3d_igemm_split(x, wts, bias, co, nsplit)
    for slope in SLOPES:
        y_act, table = act_call(hip, CONV, 'fwd_split_act', x, (wts, bias, b, ci, co, r, nsplit, None, 0), y_plain.shape, slope, b * r * r, r,
                                args_mid=(None,))
        check(hip, CONV, y_plain, y_act, table, slope, r)


@pytest.mark.parametrize('shape', [(1, 16, 40, 12), (2, 6, 70, 8), (1, 8, 16, 32), (20, 8, 64, 16)], ids=str)
def test_conv3d_fp32_mfma_kernel(hip, shape):
    b, ci, co, r = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = grid_input(b, ci, r, g)
    w = (torch.randn(co, ci, 3, 3, 3, generator=g) * 0.1).to(DEV)
    bias = torch.randn(co, generator=g).to(DEV)
    wt = hip._conv_wt(w, False)
    y_plain = hip.conv3d_forward(x, w, bias)
    for slope in SLOPES:
        y_act, table = act_call(hip, CONV, 'fwd_act', x, (wt, bias, b, ci, co, r), y_plain.shape, slope, b * r * r, r)
        check(hip, CONV, y_plain, y_act, table, slope, r)
    y_be, table_be = hip.conv3d_forward_act(x, wt, bias, co, SLOPES[-1])
    assert torch.equal(y_be, y_act) and torch.equal(table_be, table[:table_be.numel()])


def point_input(b, k, n, g):
    x = torch.randn(b, k, n, generator=g)
    x[b - 1, k // 2, max(n - 40, 0):] *= 1024.0                  # the outlier: the last point tile of the last cloud
    return x.to(DEV)


# (B, K, M, N) -> weight rows per workgroup item of the PLAIN launch (pvcnn_pwconv_fwd_split_route, nsplit 2)
PW_SHAPES = [
    ((2, 9, 64, 300), 64),             # pw_gemm_bf16_kernel, mb = 2, ragged last tile, N % 4 != 0
    ((1, 64, 128, 262), 128),          # pw_gemm_bf16_kernel, mb = 4, prefetch depth 2 (N % 4 != 0: no vector loads)
    ((2, 64, 128, 512), 128),          # pw_gemm_f16_pipe_kernel
    ((1, 64, 256, 512), 256),          # plain: the wide kernel, 256 x 256 items; with the tail: the pipe kernel
    ((1, 256, 512, 256), 512),         # plain: the wide kernel, 512 x 128 items; with the tail: the pipe kernel
    ((1, 64, 200, 512), 128),          # rows not a multiple of the tile
]


@pytest.mark.parametrize('shape,rows', PW_SHAPES, ids=[str(s) for s, _ in PW_SHAPES])
def test_pointwise_split_kernels_f16x2(hip, shape, rows):
    b, k, m, n = shape
    assert hip.lib.pvcnn_pwconv_fwd_split_route(b, k, m, n, 2) == rows
    g = torch.Generator().manual_seed(sum(shape))
    x = point_input(b, k, n, g)
    w = (torch.randn(m, k, generator=g) * 0.1).to(DEV)
    bias = torch.randn(m, generator=g).to(DEV)
    wts, amax = hip._pw_wsplit(w, False, 2), hip.pw_amax(x, want_global=False)
    tiles = b * ((n + 255) // 256)
    for bias_ in (bias, None):
        y_plain = hip.pwconv_gemm_split(x, wts, bias_, m, 2, amax=amax)
        for slope in SLOPES:
            y_act, table = act_call(hip, PW, 'fwd_split_act', x, (wts, bias_, b, k, m, n, 2, amax, 256), y_plain.shape, slope, tiles, 256,
                                    args_mid=(None,))
            check(hip, PW, y_plain, y_act, table, slope, 256)
    y_be, table_be = hip.pwconv_gemm_split_act(x, wts, None, m, 2, SLOPES[-1], amax=amax)
    assert torch.equal(y_be, y_act) and torch.equal(table_be, table[:table_be.numel()])


@pytest.mark.parametrize('shape,nsplit', [((2, 64, 128, 512), 1), ((2, 9, 64, 300), 1), ((1, 64, 128, 262), 3)], ids=str)
def test_pointwise_split_kernels_bf16_and_bf16x3(hip, shape, nsplit):
    b, k, m, n = shape
    g = torch.Generator().manual_seed(sum(shape) + nsplit)
    x = point_input(b, k, n, g)
    w = (torch.randn(m, k, generator=g) * 0.1).to(DEV)
    bias = torch.randn(m, generator=g).to(DEV)
    wts = hip._pw_wsplit(w, False, nsplit)
    y_plain = hip.pwconv_gemm_split(x, wts, bias, m, nsplit)
    for slope in SLOPES:
        y_act, table = act_call(hip, PW, 'fwd_split_act', x, (wts, bias, b, k, m, n, nsplit, None, 0), y_plain.shape, slope,
                                b * ((n + 255) // 256), 256, args_mid=(None,))
        check(hip, PW, y_plain, y_act, table, slope, 256)


@pytest.mark.parametrize('shape', [(1, 16, 32, 256), (2, 9, 40, 300), (3, 32, 128, 512), (1, 70, 200, 100)], ids=str)
def test_pointwise_fp32_mfma_kernel(hip, shape):
    """The route small products take (below HipBackend.pw_split_min_macs): pw_gemm_kernel, fast and bounds-checked paths, both heights."""
    b, k, m, n = shape
    assert shape != (1, 16, 32, 256) or b * k * m * n < hip.pw_split_min_macs
    g = torch.Generator().manual_seed(sum(shape))
    x = point_input(b, k, n, g)
    w = (torch.randn(m, k, generator=g) * 0.1).to(DEV)
    bias = torch.randn(m, generator=g).to(DEV)
    wt = hip.pwconv_weight_transposed(w)
    tiles = b * ((n + 255) // 256)
    for bias_ in (bias, None):
        y_plain = hip.pwconv_forward(x, w, bias_)
        for slope in SLOPES:
            y_act, table = act_call(hip, PW, 'fwd_act', x, (wt, wt.shape[0], bias_, b, k, m, n), y_plain.shape, slope, tiles, 256)
            check(hip, PW, y_plain, y_act, table, slope, 256)
    y_be, table_be = hip.pwconv_forward_act(x, wt, None, m, SLOPES[-1])
    assert torch.equal(y_be, y_act) and torch.equal(table_be, table[:table_be.numel()])
