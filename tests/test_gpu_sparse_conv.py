"""The sparse voxel operators on the device (csrc/sparse.hip) against the truth (tests/sparse_conv_truth.py): the map, gather / scatter,
the convolution's forward, backward-data, backward-weight + bias, and SparseConv3d through autograd.

Two modes.  EXACT, torch.equal: one-hot weights (the output is a shifted copy of the input or 0) at every tap, and short integers
(x, grad_y in [-3, 3], w in [-2, 2]: forward sums stay under 27 * 130 * 6 < 2^24, weight-gradient sums under 4096 * 9 < 2^24, so every
fp32 sum is exact in any order).  RANDOM, the bar of tests/test_gpu_conv3d.py: N(0, 1) inputs, 0.1 N(0, 1) weights,
max|err| / max|truth| < 1e-5 against fp64 for all four results.  The cases (sparse_conv_truth.CASES) are the smallest shapes at which
each thing can go wrong: one voxel; a full grid; an empty middle cloud with rows adjacent across a cloud boundary and across the end
of a z row; a count that is no multiple of the tile with several ci chunks; ragged Co tiles with many row tiles and most taps skipped."""
import functools

import pytest
import torch

import sparse_conv_truth as T
from conftest import SEED

pytestmark = pytest.mark.gpu
BAR = 1e-5
ALL = ['a', 'b', 'c', 'd', 'e']


@functools.lru_cache(maxsize=None)
def _case(case, extra=0):
    """-> (cnt on the host, the truth's map at cap = count + extra rounded up to the row tile when extra == 0)."""
    b, r, _, _ = T.CASES[case]
    cnt = T.make_cnt(case)
    count = int((cnt > 0).sum())
    cap = count + extra if extra else (count + 63) // 64 * 64
    return cnt, T.truth_map(cnt, r, cap)


def _dev_map(case, extra=0):
    import pvcnn_amd.modules.functional as F
    cnt, tm = _case(case, extra)
    return F.sparse_map(cnt.cuda(), tm['r'], cap=tm['cap']), tm


def _gen(seed):
    return torch.Generator().manual_seed(SEED + seed)


def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=_gen(seed)).float()


def _rel(got, want):
    want = want.double()
    return ((got.detach().cpu().double() - want).abs().max() / want.abs().max().clamp_min(1e-30)).item()


def _layer_results(case, x, w, bias, gy):
    """The four results of SparseConv3d through autograd on the device: (y, grad_x, grad_w, grad_b)."""
    from pvcnn_amd.modules import SparseConv3d
    m, tm = _dev_map(case)
    layer = SparseConv3d(w.shape[1], w.shape[0]).cuda()
    with torch.no_grad():
        layer.weight.copy_(w); layer.bias.copy_(bias)
    xd = x.cuda().requires_grad_()
    y = layer(xd, m)
    y.backward(gy.cuda())
    return (y.detach(), xd.grad, layer.weight.grad, layer.bias.grad), tm


@pytest.mark.parametrize('case', ALL)
def test_map_equals_the_truth(case):
    m, tm = _dev_map(case)
    torch.cuda.synchronize()
    assert int(m.overflow) == 0 and int(m.count) == tm['count'] and m.cap == tm['cap']
    for name in ('voxel', 'index', 'offsets', 'nbr'):
        assert torch.equal(getattr(m, name).cpu().long(), tm[name]), name


@pytest.mark.parametrize('case', ALL)
def test_gather_and_scatter(case):
    import pvcnn_amd.modules.functional as F
    b, r, ci, _ = T.CASES[case]
    m, tm = _dev_map(case)
    grid = torch.randn((b, ci, r, r, r), generator=_gen(1))
    gd = grid.cuda().requires_grad_()
    rows = F.sparse_gather(gd, m)
    assert torch.equal(rows.detach().cpu().double(), T.truth_gather(grid, tm))
    back = F.sparse_scatter(rows, m)
    mask = (_case(case)[0] > 0).reshape(b, 1, r, r, r)
    assert torch.equal(back.detach().cpu(), grid * mask)                        # scatter(gather(g)) == g masked, every word written
    go = torch.randn(back.shape, generator=_gen(2))
    back.backward(go.cuda())                                                    # through both: each is the other's backward
    assert torch.equal(gd.grad.cpu(), go * mask)
    rd = torch.randn((tm['cap'], ci), generator=_gen(3)).cuda().requires_grad_()
    F.sparse_scatter(rd, m).backward(go.cuda())
    assert torch.equal(rd.grad.cpu().double(), T.truth_gather(go, tm))


@pytest.mark.parametrize('case', ['a', 'b', 'c', 'd'])
def test_one_hot_weights_shift_the_input_at_every_tap(case):
    import pvcnn_amd.modules.functional as F
    _, _, ci, co = T.CASES[case]
    m, tm = _dev_map(case)
    x = torch.randn((tm['cap'], ci), generator=_gen(4))
    gy = torch.randn((tm['cap'], co), generator=_gen(5))
    xd, gd = x.cuda(), gy.cuda()
    nbr = tm['nbr']
    for tap in range(27):
        src = [(o + tap) % ci for o in range(co)]
        w = torch.zeros((co, ci, 27))
        w[torch.arange(co), torch.tensor(src), tap] = 1.0
        w = w.reshape(co, ci, 3, 3, 3)
        xr, wr = xd.clone().requires_grad_(), w.cuda().requires_grad_()
        y = F.sparse_conv3d(xr, wr, None, m)
        y.backward(gd)
        n = nbr[:, tap]
        want = torch.where((n >= 0)[:, None], x[n.clamp_min(0)][:, src], torch.zeros(()))          # the shifted copy, or 0
        assert torch.equal(y.detach().cpu(), want), tap
        if tap in (0, 13, 14, 26) or case != 'd':                                                    # and the truth says the same
            assert torch.equal(y.detach().cpu().double(), T.truth_conv(x, w, None, tm)), tap
            gx, gw, _ = T.truth_grads(x, w, None, gy, tm)
            if co <= ci:                                                         # one output channel per input channel: a copy again
                assert torch.equal(xr.grad.cpu().double(), gx), tap
            assert _rel(xr.grad, gx) < BAR and _rel(wr.grad, gw) < BAR, tap     # (sums of normals and of their products: not exact)


@pytest.mark.parametrize('case', ALL)
def test_short_integers_are_exact(case):
    _, _, ci, co = T.CASES[case]
    cap = _case(case)[1]['cap']
    x, gy = _ints((cap, ci), -3, 3, 6), _ints((cap, co), -3, 3, 7)
    w, bias = _ints((co, ci, 3, 3, 3), -2, 2, 8), _ints((co,), -2, 2, 9)
    (y, gx, gw, gb), tm = _layer_results(case, x, w, bias, gy)
    ty = T.truth_conv(x, w, bias, tm)
    tgx, tgw, tgb = T.truth_grads(x, w, bias, gy, tm)
    assert torch.equal(y.cpu().double(), ty)
    assert torch.equal(gx.cpu().double(), tgx)
    assert torch.equal(gw.cpu().double(), tgw)
    assert torch.equal(gb.cpu().double(), tgb)


@pytest.mark.parametrize('case', ALL)
def test_random_inputs_meet_the_bar(case):
    _, _, ci, co = T.CASES[case]
    cap = _case(case)[1]['cap']
    x, gy = torch.randn((cap, ci), generator=_gen(10)), torch.randn((cap, co), generator=_gen(11))
    w, bias = 0.1 * torch.randn((co, ci, 3, 3, 3), generator=_gen(12)), 0.1 * torch.randn((co,), generator=_gen(13))
    (y, gx, gw, gb), tm = _layer_results(case, x, w, bias, gy)
    ty = T.truth_conv(x, w, bias, tm)
    tgx, tgw, tgb = T.truth_grads(x, w, bias, gy, tm)
    errs = {'y': _rel(y, ty), 'grad_x': _rel(gx, tgx), 'grad_w': _rel(gw, tgw), 'grad_b': _rel(gb, tgb)}
    print(case, errs)
    assert all(e < BAR for e in errs.values()), errs
    assert torch.equal(y[tm['count']:].cpu(), torch.zeros((cap - tm['count'], co)))
    assert torch.equal(gx[tm['count']:].cpu(), torch.zeros((cap - tm['count'], ci)))


@pytest.mark.parametrize('case', ['c', 'd'])
def test_pad_rows_are_never_read_and_come_out_as_zeros(case, hip):
    """cap = count + 200, NaN in the input rows >= count and in every output buffer beforehand."""
    _, _, ci, co = T.CASES[case]
    m, tm = _dev_map(case, extra=200)
    count, cap = tm['count'], tm['cap']
    assert cap == count + 200
    x, gy = torch.randn((cap, ci), generator=_gen(14)), torch.randn((cap, co), generator=_gen(15))
    w, bias = 0.1 * torch.randn((co, ci, 3, 3, 3), generator=_gen(16)), 0.1 * torch.randn((co,), generator=_gen(17))
    x[count:] = float('nan'); gy[count:] = float('nan')
    xd, gd, wd = x.cuda(), gy.cuda(), w.cuda()
    nan = lambda *shape: torch.full(shape, float('nan'), device='cuda')
    y = hip.sparse_conv3d_forward(xd, hip.sparse_conv3d_weight_image(wd), bias.cuda(), m.nbr, m.count, out=nan(cap, co))
    gx = hip.sparse_conv3d_forward(gd, hip.sparse_conv3d_weight_image(wd, True), None, m.nbr, m.count, out=nan(cap, ci))
    gw, gb = hip.sparse_conv3d_backward_weight(xd, gd, m.nbr, m.count, out=nan(co, ci, 3, 3, 3), out_bias=nan(co))
    grid = hip.sparse_scatter(xd, m.index, m.count, m.batch, m.resolution, out=nan(m.batch, ci, m.resolution ** 3))
    rows = hip.sparse_gather(grid, m.voxel, m.count, out=nan(cap, ci))
    for name, t in (('y', y), ('gx', gx), ('gw', gw), ('gb', gb), ('grid', grid), ('rows', rows)):
        assert not torch.isnan(t).any(), name
    for name, t in (('y', y), ('gx', gx), ('rows', rows)):
        assert torch.equal(t[count:].cpu(), torch.zeros_like(t[count:]).cpu()), name
    tgx, tgw, tgb = T.truth_grads(x, w, bias, gy, tm)
    assert _rel(y, T.truth_conv(x, w, bias, tm)) < BAR and _rel(gx, tgx) < BAR and _rel(gw, tgw) < BAR and _rel(gb, tgb) < BAR
    assert torch.equal(rows[:count].cpu(), x[:count])


def test_zero_active_voxels():
    import pvcnn_amd.modules.functional as F
    from pvcnn_amd.modules import SparseConv3d
    b, r, ci, co = 2, 4, 5, 7
    m = F.sparse_map(torch.zeros((b, r ** 3), dtype=torch.int32, device='cuda'), r, cap=128)
    assert int(m.count) == 0 and int(m.overflow) == 0 and m.offsets.tolist() == [0, 0, 0]
    assert (m.voxel == -1).all() and (m.index == -1).all() and (m.nbr == -1).all()
    layer = SparseConv3d(ci, co).cuda()
    grid = torch.randn((b, ci, r, r, r), device='cuda', requires_grad=True)
    rows = F.sparse_gather(grid, m)
    y = layer(rows, m)
    out = F.sparse_scatter(y, m)
    out.backward(torch.randn_like(out))
    torch.cuda.synchronize()
    for t in (rows, y, out, grid.grad, layer.weight.grad, layer.bias.grad):
        assert torch.equal(t.detach().cpu(), torch.zeros(t.shape))


def _guarded(shapes, dtype, fill):
    """One allocation holding a view per shape with 256 poisoned words before, between and after them -> (views, check)."""
    guard = 256
    sizes = [int(torch.tensor(s).prod()) for s in shapes]
    whole = torch.full((guard + sum(n + guard for n in sizes),), fill, dtype=dtype, device='cuda')
    views, keep, at = [], torch.ones(whole.shape, dtype=torch.bool), guard
    for s, n in zip(shapes, sizes):
        views.append(whole[at:at + n].view(s))
        keep[at:at + n] = False
        at += n + guard
    keep = keep.cuda()

    def check():
        g = whole[keep]
        assert bool((g != g).all()) if fill != fill else bool((g == fill).all()), 'a guard word was written'
    return views, check


def test_map_overflow_sets_the_flag_and_writes_inside_the_buffers(hip):
    cnt, full = _case('c')
    b, r, ci, co = T.CASES['c']
    cap = full['count'] - 37
    tm = T.truth_map(cnt, r, cap)
    views, check_map = _guarded([(cap,), (b * r ** 3,), (b + 1,), (cap, 27), (1,)], torch.int32, 0x5A5A5A5A)
    voxel, index, offsets, nbr, overflow = hip.sparse_map(cnt.cuda(), r, cap, out=views)
    torch.cuda.synchronize()
    check_map()
    assert int(overflow) == 1 and int(offsets[b]) == cap
    for got, name in ((voxel, 'voxel'), (index, 'index'), (offsets, 'offsets'), (nbr, 'nbr')):
        assert torch.equal(got.cpu().long(), tm[name]), name
    # the truncated map serves the other launches, inside their buffers
    x, gy = torch.randn((cap, ci), generator=_gen(18)), torch.randn((cap, co), generator=_gen(19))
    w = 0.1 * torch.randn((co, ci, 3, 3, 3), generator=_gen(20))
    (y, gx, gw, gb, grid, rows), check = _guarded([(cap, co), (cap, ci), (co, ci, 3, 3, 3), (co,), (b, ci, r ** 3), (cap, ci)], torch.float32,
                                                  float('nan'))
    count = offsets[b:]
    xd, gd, wd = x.cuda(), gy.cuda(), w.cuda()
    hip.sparse_conv3d_forward(xd, hip.sparse_conv3d_weight_image(wd), None, nbr, count, out=y)
    hip.sparse_conv3d_forward(gd, hip.sparse_conv3d_weight_image(wd, True), None, nbr, count, out=gx)
    hip.sparse_conv3d_backward_weight(xd, gd, nbr, count, out=gw, out_bias=gb)
    hip.sparse_scatter(xd, index, count, b, r, out=grid)
    hip.sparse_gather(grid, voxel, count, out=rows)
    torch.cuda.synchronize()
    check()
    tgx, tgw, tgb = T.truth_grads(x, w, None, gy, tm)
    assert _rel(y, T.truth_conv(x, w, None, tm)) < BAR and _rel(gx, tgx) < BAR and _rel(gw, tgw) < BAR
    assert _rel(gb, gy.double().sum(0)) < BAR and torch.equal(rows.cpu(), x)
    assert torch.equal(grid.cpu().double().reshape(b, ci, r, r, r), T.truth_scatter(x, tm))


def test_agrees_with_the_dense_kernels(hip):
    """Case d: sparse_scatter(sparse_conv3d(...)) against hip.conv3d_forward of the zero-filled grid, at the active voxels."""
    import pvcnn_amd.modules.functional as F
    b, r, ci, co = T.CASES['d']
    m, tm = _dev_map('d')
    x = torch.randn((tm['cap'], ci), generator=_gen(21)).cuda()
    w, bias = (0.1 * torch.randn((co, ci, 3, 3, 3), generator=_gen(22))).cuda(), (0.1 * torch.randn((co,), generator=_gen(23))).cuda()
    mask = (_case('d')[0] > 0).reshape(b, 1, r, r, r).cuda()
    sparse = F.sparse_scatter(F.sparse_conv3d(x, w, bias, m), m)
    dense = hip.conv3d_forward(F.sparse_scatter(x, m).contiguous(), w, bias) * mask
    assert torch.equal(sparse * mask, sparse)
    assert _rel(sparse, dense.cpu()) < BAR


@pytest.mark.parametrize('case', ['sheet', 'd', 'e'])
def test_skip_switch_and_reruns_give_the_same_bits(case, hip):
    import pvcnn_amd.modules.functional as F
    if case == 'sheet':                    # one z plane of a 16^3 grid, 4 tiles: no row has a neighbour at the 18 taps with dz != 0
        ci, co, cap = 16, 32, 256
        cnt = torch.zeros((1, 16, 16, 16), dtype=torch.int32)
        cnt[0, :, :, 5] = 1
        m = F.sparse_map(cnt.reshape(1, -1).cuda(), 16, cap=cap)
        present = (m.nbr.view(cap // 64, 64, 27) >= 0).any(1).cpu()
        assert present.tolist() == [[tap % 3 == 1 for tap in range(27)]] * 4 and int(m.count) == cap
    else:
        _, _, ci, co = T.CASES[case]
        m, tm = _dev_map(case)
        cap = tm['cap']
    x, gy = torch.randn((cap, ci), generator=_gen(24)).cuda(), torch.randn((cap, co), generator=_gen(25)).cuda()
    w, bias = (0.1 * torch.randn((co, ci, 3, 3, 3), generator=_gen(26))).cuda(), (0.1 * torch.randn((co,), generator=_gen(27))).cuda()

    def run():
        y = hip.sparse_conv3d_forward(x, hip.sparse_conv3d_weight_image(w), bias, m.nbr, m.count)
        gx = hip.sparse_conv3d_forward(gy, hip.sparse_conv3d_weight_image(w, True), None, m.nbr, m.count)
        return (y, gx) + hip.sparse_conv3d_backward_weight(x, gy, m.nbr, m.count)
    assert hip.sparse_skip() is True
    first, again = run(), run()
    if case == 'sheet':                    # (and the skipped taps were the right ones to skip)
        tm = T.truth_map(cnt.reshape(1, -1), 16, cap)
        tgx, tgw, tgb = T.truth_grads(x.cpu(), w.cpu(), bias.cpu(), gy.cpu(), tm)
        assert _rel(first[0], T.truth_conv(x.cpu(), w.cpu(), bias.cpu(), tm)) < BAR
        assert _rel(first[1], tgx) < BAR and _rel(first[2], tgw) < BAR and _rel(first[3], tgb) < BAR
    try:
        assert hip.sparse_skip(False) is True
        without = run()
    finally:
        hip.sparse_skip(True)
    assert hip.sparse_skip() is True
    for k, (a, b_, c) in enumerate(zip(first, again, without)):
        assert torch.equal(a.view(torch.int32), b_.view(torch.int32)), k
        assert torch.equal(a.view(torch.int32), c.view(torch.int32)), k


def test_a_captured_chain_replays_on_another_occupancy():
    import pvcnn_amd.modules.functional as F
    from pvcnn_amd.modules import SparseConv3d
    b, r, ci, mid = 2, 16, 16, 32
    first, second = T.make_cnt('d', seed=11), T.make_cnt('d', seed=12)
    assert int((first > 0).sum()) != int((second > 0).sum())
    cap = F.sparse_default_cap(b, r, 300)
    torch.manual_seed(SEED)
    l1, l2 = SparseConv3d(ci, mid).cuda(), SparseConv3d(mid, ci).cuda()
    params = list(l1.parameters()) + list(l2.parameters())
    grids = [torch.randn((b, ci, r, r, r), generator=_gen(28 + i)).cuda() for i in range(2)]
    go = torch.randn((b, ci, r, r, r), generator=_gen(30)).cuda()
    s_cnt, s_grid = first.cuda().clone(), grids[0].clone().requires_grad_()

    def chain(cnt, grid):
        m = F.sparse_map(cnt, r, cap=cap)
        out = F.sparse_scatter(l2(l1(F.sparse_gather(grid, m), m), m), m)
        return (out,) + torch.autograd.grad(out, [grid] + params, go)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain(s_cnt, s_grid)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s_out = chain(s_cnt, s_grid)
    with torch.no_grad():
        s_cnt.copy_(second.cuda()); s_grid.copy_(grids[1])
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in s_out]
    eager = chain(second.cuda(), grids[1].clone().requires_grad_())
    assert replayed[0].abs().sum() > 0
    for k, (a, e) in enumerate(zip(replayed, eager)):
        assert torch.equal(a.view(torch.int32), e.view(torch.int32)), k
