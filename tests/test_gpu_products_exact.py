"""The Conv3d and 1x1 product kernels (csrc/conv3d.hip, conv3d_bf16.hip, conv3d_wgrad_f16.hip, pointwise.hip, pointwise_bf16.hip,
pointwise_wgrad_f16.hip) against the exact truths of tests/products_truth.py, on every instantiation csrc/route.h selects
(products_truth.ROUTE_CASES; tests/test_products_truth_host.py proves the truths and the coverage on the CPU).

  (a) single-product weights: every output element is one product, the result a shifted copy of the input -- `torch.equal`, forward
      and backward-data, fp32 MFMA / bf16 / f16x2 / bf16x3, all 27 taps per row and mode; once with the mantissa in the activations
      (weights +-2^k) and once with it in the weights (activations 0, +-2^j): the operand conversions bit for bit.
  (b) one live voxel (point) per input channel: every element of grad_w is one product of two short integers -- `torch.equal` for the
      fp32-MFMA and the f16x2 backward-weight kernels (flat one-word amax and the row table); grad_bias is an exact integer sum.
  (c) plain bf16 (nsplit 1, the arithmetic under torch.autocast(bfloat16)) against fp64 on the RNE-bf16-rounded operands at the
      fp32-accumulation bar of tests/test_gpu_conv3d.py (TOL = 1e-5), per (cloud, output channel), weight rows six decades apart; the
      same through autograd under autocast.  The lines `[matched bf16]` of a `pytest -s` run are profiles/products_exact_parity.log.
  (d) the tiles no other kernel-level test launches, judged as test_conv3d_on_the_bf16_matrix_cores judges its cases."""
import pytest
import torch
import torch.nn.functional as F

import products_truth as pt
from test_gpu_conv3d import TOL, test_conv3d_on_the_bf16_matrix_cores as _judged_like_every_other_tile
from test_gpu_math_modes import modes          # noqa: F401  (fixture: switches of the live backend for one test)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

MODES = {'fp32': 0, 'bf16': 1, 'f16x2': 2, 'bf16x3': 3}            # -> nsplit (0: the fp32-MFMA entries)
ROWS = pt.ROUTE_CASES
ROW_IDS = [row['id'] for row in ROWS]


def _spatial(row):
    return (row['shape'][3],) * (3 if row['kind'] == 'conv' else 1)


def _products(hip, kind, nsplit):
    """-> (forward(x, w, bias=None, **kw), backward_data(grad_y, w)) of a kind in a math mode"""
    c = 'conv3d' if kind == 'conv' else 'pwconv'
    if nsplit == 0:
        fwd, bwd = getattr(hip, c + '_forward'), getattr(hip, c + '_backward_data')
        return (lambda x, w, bias=None, **kw: fwd(x, w, bias, **kw)), bwd
    fwd, bwd = getattr(hip, c + '_forward_split'), getattr(hip, c + '_backward_data_split')
    return (lambda x, w, bias=None, **kw: fwd(x, w, bias, nsplit, **kw)), (lambda g, w: bwd(g, w, nsplit))


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------------

def _decades(n, gen):
    return torch.randn(n, generator=gen) * 10.0 ** ((torch.arange(n) % 7) - 3).float()


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('row', ROWS, ids=ROW_IDS)
def test_single_product_weights_copy_the_input_bit_for_bit(hip, gen, row, mode):
    """Expectations (products_truth, proven in test_products_truth_host.py): fp32 and bf16x3 value * shift(x) for arbitrary normal x
    and value = +-2^k; bf16 value * shift(bf16_rne(x)), x with the tie set in cloud 0; f16x2 the same for x = integers |v| <= 1023
    times one power of two.  Second variant, x in {0, +-2^j}: w * x (fp32, bf16x3; f16x2 with 11-bit integer weights times a power
    of two), bf16_rne(w) * x (bf16, ties among the weights)."""
    kind, (b, ci, co, _), sp = row['kind'], row['shape'], _spatial(row)
    forward, backward_data = _products(hip, kind, MODES[mode])
    groups = pt.tap_groups(min(ci, co), gen) if kind == 'conv' else [None]
    rounded = pt.bf16_rne if mode == 'bf16' else (lambda t: t)

    def check(x, gy, values_of, x_seen, gy_seen, weights_seen):
        for taps in groups:
            values = values_of()
            w, live = pt.single_product_weights(co, ci, taps, gen, values[torch.randperm(len(values), generator=gen)])
            seen = weights_seen(torch.tensor([v for *_, v in live]))
            wd = w.to(DEV)
            assert torch.equal(forward(x, wd), pt.single_product_forward(x_seen, live, co, weights=seen)), (row['id'], mode, 'forward', taps)
            assert torch.equal(backward_data(gy, wd), pt.single_product_backward_data(gy_seen, live, ci, weights=seen)), \
                (row['id'], mode, 'backward-data', taps)

    # the mantissa in the activations
    if mode == 'f16x2':
        x, gy = pt.short_ints((b, ci, *sp), gen, shift=-5).to(DEV), pt.short_ints((b, co, *sp), gen, shift=7).to(DEV)
    else:
        x = pt.decade_normals((b, ci, *sp), gen, ties=mode == 'bf16').to(DEV)
        gy = pt.decade_normals((b, co, *sp), gen, ties=mode == 'bf16').to(DEV)
    check(x, gy, lambda: pt.signed_pow2((27,), gen, -4, 4), rounded(x.cpu()).to(DEV), rounded(gy.cpu()).to(DEV), lambda v: v)
    # the mantissa in the weights
    x = pt.signed_pow2((b, ci, *sp), gen, zeros=True).to(DEV)
    gy = pt.signed_pow2((b, co, *sp), gen, zeros=True).to(DEV)
    if mode == 'f16x2':
        values_of = lambda: pt.short_ints((27,), gen, shift=-4, nonzero=True)
    elif mode == 'bf16':
        values_of = lambda: torch.cat([pt.tie_set()[torch.randperm(28, generator=gen)[:13]], _decades(14, gen)])
    else:
        values_of = lambda: _decades(27, gen)
    check(x, gy, values_of, x, gy, rounded)


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------------

WGRAD_KERNELS = ['fp32', 'f16x2-flat-amax', 'f16x2-row-table']


def _backward_weight(hip, kind, kernel, x, gy):
    c = 'conv3d' if kind == 'conv' else 'pwconv'
    if kernel == 'fp32':
        return getattr(hip, c + '_backward_weight')(x, gy, with_bias=True)
    amax = hip.absmax_bits if kernel == 'f16x2-flat-amax' else (hip.conv_amax if kind == 'conv' else hip.pw_amax)
    return getattr(hip, c + '_backward_weight_f16')(x, gy, amax(x), amax(gy), with_bias=True)


@pytest.mark.parametrize('kernel', WGRAD_KERNELS)
@pytest.mark.parametrize('b,ci,co,r', [(2, 9, 24, 32), (2, 16, 70, 32), (3, 40, 24, 12), (2, 16, 24, 16), (2, 9, 70, 8), (2, 40, 70, 16)])
def test_one_live_voxel_per_channel_gives_the_weight_gradient_bit_for_bit(hip, gen, b, ci, co, r, kernel):
    """grad_w[o, c, tap] = grad_y[cloud_c, o, v_c - offset(tap)] * x[cloud_c, c, v_c] (0 outside the grid), integers below 2^24: exact in
    every kernel.  The positions (products_truth.voxel_positions) go round the channels over as many launches as Ci needs.  With the
    row table nearly every z row of x is empty: the live-row skipping must not lose a product.  Ci = 9: the (dx, ci)-packed kernel."""
    positions = pt.voxel_positions(b, r)
    gy = pt.short_ints((b, co, r, r, r), gen, pt.exact_sum_bound(b * r ** 3)).to(DEV)
    bias_want = gy.double().sum(dim=(0, 2, 3, 4))
    assert bias_want.abs().max().item() < 1 << 24
    for launch in range((len(positions) + ci - 1) // ci):
        x, live = pt.live_voxel_inputs(b, ci, r, gen, pt.rotated(positions, launch * ci))
        gw, gb = _backward_weight(hip, 'conv', kernel, x.to(DEV), gy)
        assert torch.equal(gw, pt.live_voxel_grad_w(live, gy)), (kernel, launch, [(bi, v) for bi, v, _ in live])
        assert torch.equal(gb.double(), bias_want), (kernel, launch)


@pytest.mark.parametrize('kernel', WGRAD_KERNELS)
@pytest.mark.parametrize('b,ci,co,n', [(2, 9, 24, 260), (3, 40, 70, 516), (2, 16, 24, 516), (2, 130, 70, 260)])
def test_one_live_point_per_channel_gives_the_weight_gradient_bit_for_bit(hip, gen, b, ci, co, n, kernel):
    """The 1x1 analogue: points 0, 255, 256 (the tile seam) and N - 1 of the first and the last cloud."""
    positions = pt.point_positions(b, n)
    gy = pt.short_ints((b, co, n), gen, pt.exact_sum_bound(b * n)).to(DEV)
    bias_want = gy.double().sum(dim=(0, 2))
    for launch in range((len(positions) + ci - 1) // ci):
        x, live = pt.live_point_inputs(b, ci, n, gen, pt.rotated(positions, launch * ci))
        gw, gb = _backward_weight(hip, 'pw', kernel, x.to(DEV), gy)
        assert torch.equal(gw, pt.live_point_grad_w(live, gy)), (kernel, launch)
        assert torch.equal(gb.double(), bias_want), (kernel, launch)


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------------

def _rel(a, b):
    return (a.double() - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def _per_channel(got, ref):
    """The largest error of a (cloud, channel) slice over that slice's own largest reference entry."""
    dims = tuple(range(2, ref.dim()))
    return ((got.double() - ref).abs().amax(dim=dims) / ref.abs().amax(dim=dims).clamp_min(1e-30)).max().item()


def _conv64(kind, x, w, bias=None):
    if kind == 'conv':
        return F.conv3d(x, w, bias, padding=1)
    y = torch.einsum('oc,bcn->bon', w, x)
    return y if bias is None else y + bias.view(1, -1, 1)


def _conv64_input(kind, shape, w, gy):
    return torch.nn.grad.conv3d_input(shape, w, gy, padding=1) if kind == 'conv' else torch.einsum('oc,bon->bcn', w, gy)


def _rows_apart(n):
    return torch.logspace(-3, 3, n) if n > 1 else torch.ones(1)


def _matched(t):
    return pt.bf16_rne(t.cpu()).to(DEV).double()


@pytest.mark.parametrize('row', ROWS, ids=ROW_IDS)
def test_plain_bf16_meets_the_fp32_bar_on_matched_operands(hip, gen, row):
    """ref = conv_fp64(bf16_rne(x), bf16_rne(w)) + bias: products of bf16 numbers are exact in fp32, only the fp32 accumulation rounds,
    so TOL of test_gpu_conv3d.py holds -- taken per (cloud, output channel), with the weight rows (for backward-data: the weight
    columns, its output channels) scaled over logspace(-3, 3) so that a wrong row cannot hide under a large neighbour.  A kernel
    that truncated, rounded the weight image another way or dropped a K tail misses this bar by two orders of magnitude.

    The BatchNorm partial sums of the launch with bias are judged against the kernel's own output like everywhere else, at 1e-5: the
    largest error over the largest sum of all channels, and -- the rows being six decades apart -- per channel as well, sum y over
    sum |y| and sum y^2 over itself.  "Its own output" is the output of the launch WITHOUT bias, which is what the statistics sum
    (csrc: "statistics of (y - bias)"): subtracting the bias from y = fl(acc + bias) instead adds that rounding to every term, and
    with one row dominating the quotient it showed as 1.60e-05 on (8, 4, 8, 32) (262 144 terms) where the sums are within 2.4e-07
    of those of the kernel's output."""
    kind, (b, ci, co, _), sp = row['kind'], row['shape'], _spatial(row)
    forward, backward_data = _products(hip, kind, 1)
    tail = [1] * (3 if kind == 'conv' else 0)
    w0 = torch.randn(co, ci, *([3] * len(tail)), generator=gen) * 0.1
    x = torch.randn(b, ci, *sp, generator=gen).to(DEV)
    gy = torch.randn(b, co, *sp, generator=gen).to(DEV)
    bias = torch.randn(co, generator=gen).to(DEV)
    w = (w0 * _rows_apart(co).view(-1, 1, *tail)).to(DEV)
    w_cols = (w0 * _rows_apart(ci).view(1, -1, *tail)).to(DEV)
    ref = _conv64(kind, _matched(x), _matched(w))
    y, part = forward(x, w, bias, want_stats=True)
    e_bias = _per_channel(y, ref + bias.double().view(1, -1, *[1] * len(sp)))
    y_plain = forward(x, w)
    e_plain = _per_channel(y_plain, ref)
    e_data = _per_channel(backward_data(gy, w_cols), _conv64_input(kind, x.shape, _matched(w_cols), _matched(gy)))
    centred = y_plain.double().transpose(0, 1).reshape(co, -1)     # (y - bias would add the rounding of y + bias to the small rows)
    sums = part.double().sum(dim=1)
    e_sum = ((sums[:, 0] - centred.sum(dim=1)).abs() / centred.abs().sum(dim=1).clamp_min(1e-30)).max().item()
    e_sq = ((sums[:, 1] - (centred * centred).sum(dim=1)).abs() / (centred * centred).sum(dim=1).clamp_min(1e-30)).max().item()
    as_elsewhere = max(_rel(sums[:, 0], centred.sum(dim=1)), _rel(sums[:, 1], (centred * centred).sum(dim=1)))
    unmatched = _per_channel(y, _conv64(kind, x.double(), w.double(), bias.double()))
    print(f"[matched bf16] {row['id']} forward {row['listed']['fwd', 1]} backward-data {row['listed']['bwd', 1]}: y+bias {e_bias:.2e} "
          f'y {e_plain:.2e} grad_x {e_data:.2e} stats {e_sum:.2e} {e_sq:.2e} (over the largest sum of all channels: {as_elsewhere:.2e}; '
          f'y to the unrounded fp64: {unmatched:.2e})')
    assert e_bias < TOL and e_plain < TOL and e_data < TOL
    assert e_sum < 1e-5 and e_sq < 1e-5 and as_elsewhere < 1e-5
    assert unmatched > 1e-4                                   # really bf16 operands


def _autocast_case(label, layer, x, weight, bias, gy, kind):
    """One layer under torch.autocast(bfloat16) through autograd.  The arithmetic (functional/_product.py): forward and backward-data
    on bf16 operands -- matched at TOL per (cloud, channel) --; backward-weight on the UNROUNDED x and grad_y (the f16x2 kernel where
    it serves, else the fp32-MFMA one) with the bias gradient in the same pass: against the fp64 gradient of the unrounded tensors at
    TOL of the tensor's largest entry, the bar of the backward-weight tests of test_gpu_conv3d.py / test_gpu_pwconv.py."""
    x = x.requires_grad_()
    with torch.autocast('cuda', dtype=torch.bfloat16):
        y = layer(x)
    assert y.dtype == torch.float32
    y.backward(gy)
    wk = weight.detach() if kind == 'conv' else weight.detach().view(weight.shape[0], weight.shape[1])
    ref = _conv64(kind, _matched(x.detach()), _matched(wk), bias.detach().double())
    e_y = _per_channel(y.detach(), ref)
    e_x = _per_channel(x.grad, _conv64_input(kind, x.shape, _matched(wk), _matched(gy)))
    xd, gd = x.detach().double(), gy.double()
    gw_ref = (torch.nn.grad.conv3d_weight(xd, wk.shape, gd, padding=1) if kind == 'conv' else torch.einsum('bon,bcn->oc', gd, xd))
    e_w = _rel(weight.grad.view(gw_ref.shape), gw_ref)
    e_b = _rel(bias.grad, gd.sum(dim=[0] + list(range(2, gd.dim()))))
    unmatched = _per_channel(y.detach(), _conv64(kind, xd, wk.double(), bias.detach().double()))
    print(f'[matched bf16] autocast {label}: y {e_y:.2e} grad_x {e_x:.2e} grad_w {e_w:.2e} grad_bias {e_b:.2e} '
          f'(y to the unrounded fp64: {unmatched:.2e})')
    assert e_y < TOL and e_x < TOL and e_w < TOL and e_b < TOL
    assert unmatched > 1e-4                                   # the launches really took bf16 operands


@pytest.mark.parametrize('b,ci,co,r', [(2, 16, 24, 12), (1, 16, 40, 32)])
def test_voxel_conv_under_autocast_on_matched_operands(hip, gen, modes, b, ci, co, r):
    from pvcnn_amd.modules.pvconv import _VoxelConv3d
    modes()                                                   # (default switches; the memo and the weight bank emptied)
    torch.manual_seed(0)
    conv = _VoxelConv3d(ci, co, 3, stride=1, padding=1).to(DEV)
    with torch.no_grad():
        conv.weight.mul_(_rows_apart(co).view(-1, 1, 1, 1, 1).to(DEV))
    x = torch.randn(b, ci, r, r, r, generator=gen).to(DEV)
    gy = torch.randn(b, co, r, r, r, generator=gen).to(DEV)
    _autocast_case(f'_VoxelConv3d B={b} Ci={ci} Co={co} R={r}', conv, x, conv.weight, conv.bias, gy, 'conv')


@pytest.mark.parametrize('b,ci,co,n', [(2, 64, 128, 512), (1, 64, 128, 262)])
def test_pointwise_conv_under_autocast_on_matched_operands(hip, gen, modes, b, ci, co, n):
    """What the code says (functional/pwconv.py): the arithmetic is decided where the convolution is CALLED -- inside the autograd node
    autocast is switched off already -- so the layer is called as functional/bnact.py calls it, with `pw_nsplit(x, weight)` taken
    under autocast; and both products lie below `pw_split_min_macs` (2^24 multiply-adds), under which a 1x1 product keeps to the
    fp32 kernels in every mode, autocast included: the bar is lowered to 0 for the test, as tests/test_gpu_math_modes.py does, so
    that the shapes of the route table (the pipelined kernel and the scalar four-block tile) run as bf16 launches."""
    from pvcnn_amd.modules.functional.pwconv import pointwise_conv, pw_nsplit
    modes(pw_split_min_macs=0)
    w = (torch.randn(co, ci, 1, generator=gen) * 0.1 * _rows_apart(co).view(-1, 1, 1)).to(DEV).requires_grad_()
    bias = torch.randn(co, generator=gen).to(DEV).requires_grad_()
    x = torch.randn(b, ci, n, generator=gen).to(DEV)
    gy = torch.randn(b, co, n, generator=gen).to(DEV)
    _autocast_case(f'pointwise_conv B={b} K={ci} M={co} N={n}', lambda t: pointwise_conv(t, w, bias, False, pw_nsplit(t, w)), x, w, bias, gy, 'pw')


# ---- (d) ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('row', [row for row in ROWS if row['unreached']], ids=[row['id'] for row in ROWS if row['unreached']])
def test_the_unreached_tiles_against_fp64_in_every_mode(hip, row):
    """The scalar-staging (2,8,8) and (4,8,8) tiles and the first convolution of the benched PVCNN step ((4,4,32) tile, 64 weight rows,
    f16x2): nsplit 1, 2 and 3, forward, backward-data and statistics at the bars of test_conv3d_on_the_bf16_matrix_cores."""
    _judged_like_every_other_tile(hip, *row['shape'])
