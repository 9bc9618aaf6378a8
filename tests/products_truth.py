"""Exact truths for the matrix kernels (csrc/conv3d*.hip, csrc/pointwise*.hip): the 3x3x3 Conv3d and the 1x1 product, forward,
backward-data and backward-weight.  torch on the CPU only; neither the package nor the oracle is imported here.

Two instruments:

  one-product sums   operands for which EVERY output element is a sum with at most one non-zero product.  The result is then known
                     without a summation order: a shifted copy of the input times one weight (forward, backward-data), or one
                     product of two short integers (backward-weight), and `torch.equal` is the bar.  What makes the single product
                     itself exact in each arithmetic mode:
                       fp32     one factor is a power of two: the fp32 product is exact.
                       bf16     the kernel rounds both operands to bf16 (round to nearest, ties to even: `bf16_rne`); a product of
                                two bf16 numbers has 16 significant bits and is exact in fp32.
                       bf16x3   `split3_bf16`: three bf16 pieces with v = (p2 + p1) + p0 exactly, the order in which
                                split_products<3> of csrc/split16.h adds the partial products when the other factor is one piece.
                       f16x2    operands are scaled by a power of two that puts the largest magnitude into [2^13, 2^14): an integer
                                |v| <= 1023 times a power of two is then an fp16 number, the `lo` piece is 0 (`f16x2_pieces`).
  matched bf16       plain-bf16 launches against fp64 on the `bf16_rne`-rounded operands: only the fp32 accumulation rounds.

`ROUTE_CASES` lists the smallest shapes that take each instantiation csrc/route.h can select, with the instantiation per direction
and math mode; tests/test_products_truth_host.py holds the list against tools/route_table.cpp."""
import itertools

import torch

TAPS = list(itertools.product(range(3), repeat=3))        # tap t = (dx * 3 + dy) * 3 + dz is weight[..., dx, dy, dz]


# ------------------------------------------------------------------------------------------------
# operand conversions of csrc/split16.h, modelled on integers
# ------------------------------------------------------------------------------------------------

def bf16_rne(t):
    """fp32 -> the fp32 value of its bf16 rounding, by the integer formula of bf16_bits: (u + 0x7fff + ((u >> 16) & 1)) >> 16."""
    assert t.dtype == torch.float32
    u = t.contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
    r = (((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16) & 0xffffffff
    r = torch.where(r >= 1 << 31, r - (1 << 32), r).to(torch.int32)
    return r.view(torch.float32).view(t.shape)


def split3_bf16(t):
    """split_bf16<3>: (p0, p1, p2), each a bf16 number held in fp32, every residual formed in fp32 as the kernel forms it."""
    p0 = bf16_rne(t)
    r1 = t - p0
    p1 = bf16_rne(r1)
    r2 = r1 - p1
    return p0, p1, bf16_rne(r2)


def f16x2_shift(absmax):
    """scale_shift of csrc/split16.h for a finite non-zero maximum: the power of two that puts it into [2^13, 2^14)."""
    e = (torch.tensor(float(absmax), dtype=torch.float32).view(torch.int32).item() >> 23) & 0xff
    assert 0 < e < 255
    return min(max(140 - e, -100), 100)


def f16x2_pieces(t, absmax=None):
    """(hi, lo, shift) of the f16x2 split of t scaled by its own (or the given) maximum: hi = fp16(v), lo = fp16(v - hi)."""
    shift = f16x2_shift(t.abs().max() if absmax is None else absmax)
    v = t * 2.0 ** shift
    hi = v.half().float()
    return hi, (v - hi).half().float(), shift


# ------------------------------------------------------------------------------------------------
# the value sets the tests draw
# ------------------------------------------------------------------------------------------------

# fp32 bit patterns around bf16's rounding decisions, exponents near 1: ties (low half 0x8000) under an even and an odd upper half,
# one ulp on either side of a tie, a tie and a near-tie that round up into the next binade; each also with the sign bit
_TIE_BITS = [0x3f808000, 0x3f818000, 0x3f807fff, 0x3f808001, 0x3f817fff, 0x3f818001, 0x3fff8000, 0x3fffc000, 0x3f7fffff,
             0x40490fdb, 0x3eaa8000, 0x3eab8000, 0x41200001, 0x3f800000]
# host test only (the GPU tests keep to finite results): the largest finite fp32 rounds to inf, the largest that stays finite
_EXTREME_BITS = [0x7f7fffff, 0x7f7f7fff, 0x7f7f8000, 0x7f7e8000]


def _from_bits(bits):
    b = torch.tensor(bits, dtype=torch.int64)
    b = torch.cat([b, b | 0x80000000])
    return torch.where(b >= 1 << 31, b - (1 << 32), b).to(torch.int32).view(torch.float32)


def tie_set():
    """fp32 values on and next to bf16 rounding ties, both signs (finite after rounding)."""
    return _from_bits(_TIE_BITS)


def extreme_set():
    return _from_bits(_EXTREME_BITS)


def decade_normals(shape, gen, ties=False):
    """Normal fp32 values, channel c (dim 1) scaled by 10^k, k cycling over -3 .. 3: exponents well inside the range of fp32 and of
    every piece of the splits.  ties=True overwrites the head of every channel's slice of cloud 0 with `tie_set()`."""
    x = torch.randn(shape, generator=gen)
    scale = 10.0 ** ((torch.arange(shape[1]) % 7) - 3).float()
    x = x * scale.view(1, -1, *([1] * (len(shape) - 2)))
    if ties:
        t = tie_set()
        flat = x[0].view(shape[1], -1)
        n = min(t.numel(), flat.shape[1])
        flat[:, :n] = t[:n]
    return x


def short_ints(shape, gen, bound=1023, shift=0, nonzero=False):
    """Integers |v| <= bound (<= 1023: 11 bits, an fp16 significand) times 2^shift, as fp32."""
    assert 0 < bound <= 1023
    v = torch.randint(-bound, bound + 1, shape, generator=gen)
    if nonzero:
        v = torch.where(v == 0, torch.full_like(v, bound), v)
    return v.float() * 2.0 ** shift


def signed_pow2(shape, gen, lo=-3, hi=3, zeros=False):
    """+-2^j, j in [lo, hi]; zeros=True: about a quarter of the entries are 0."""
    j = torch.randint(lo, hi + 1, shape, generator=gen)
    s = torch.randint(0, 2, shape, generator=gen) * 2 - 1
    v = s.float() * torch.exp2(j.float())
    if zeros:
        v = v * (torch.randint(0, 4, shape, generator=gen) != 0)
    return v


# ------------------------------------------------------------------------------------------------
# one product per output element: forward and backward-data
# ------------------------------------------------------------------------------------------------

def single_product_weights(co, ci, taps, gen, values):
    """-> (weight, live): weight (co, ci, 3, 3, 3), or (co, ci) when taps is None, with n = min(co, ci, len(taps)) non-zero entries;
    every output channel holds at most one, every input channel is used by at most one output channel (so backward-data sums one
    product as well), surplus channels stay all-zero.  Which channels are live is drawn from `gen`; entry i takes taps[i] and
    values[i % len(values)].  live = [(o, c, tap, value)] (tap None for the 1x1 weight)."""
    n = min(co, ci) if taps is None else min(co, ci, len(taps))
    outs = torch.randperm(co, generator=gen)[:n].tolist()
    ins = torch.randperm(ci, generator=gen)[:n].tolist()
    w = torch.zeros((co, ci) if taps is None else (co, ci, 3, 3, 3))
    live = []
    for i, (o, c) in enumerate(zip(outs, ins)):
        v = float(values[i % len(values)])
        assert v != 0.0
        if taps is None:
            w[o, c] = v
            live.append((o, c, None, v))
        else:
            w[o, c][TAPS[taps[i]]] = v
            live.append((o, c, int(taps[i]), v))
    return w, live


def shift3d(x, tap):
    """The zero-padded shifted copy a single tap of a padding-1 convolution produces: out[..., p] = x[..., p + d - 1], d = TAPS[tap]."""
    r = x.shape[-1]
    out = torch.zeros_like(x)
    dst, src = [], []
    for d in TAPS[tap]:
        o = d - 1
        dst.append(slice(max(0, -o), r - max(0, o)))
        src.append(slice(max(0, o), r - max(0, -o)))
    out[(..., *dst)] = x[(..., *src)]
    return out


def mirrored(tap):
    """The tap backward-data reads through: grad_x[p] = sum_d w[d] grad_y[p - (d - 1)]."""
    return None if tap is None else 26 - tap


def single_product_forward(x, live, co, weights=None):
    """y (B, co, ...) = conv(x, w) for a single-product w: channel o is value * shift3d(x[:, c], tap) in x's dtype (one rounding at
    most: none when a factor is a power of two).  weights: the values to multiply by instead of live's (e.g. their bf16 roundings)."""
    y = torch.zeros((x.shape[0], co, *x.shape[2:]), dtype=x.dtype, device=x.device)
    for i, (o, c, tap, v) in enumerate(live):
        v = v if weights is None else float(weights[i])
        y[:, o] = (x[:, c] if tap is None else shift3d(x[:, c], tap)) * v
    return y


def single_product_backward_data(gy, live, ci, weights=None):
    """grad_x (B, ci, ...) for a single-product w: channel c is value * shift3d(gy[:, o], mirrored tap)."""
    gx = torch.zeros((gy.shape[0], ci, *gy.shape[2:]), dtype=gy.dtype, device=gy.device)
    for i, (o, c, tap, v) in enumerate(live):
        v = v if weights is None else float(weights[i])
        gx[:, c] = (gy[:, o] if tap is None else shift3d(gy[:, o], mirrored(tap))) * v
    return gx


def tap_groups(n, gen):
    """The 27 taps in a drawn order, cut into launches of at most n (the live channels of one single-product weight)."""
    order = torch.randperm(27, generator=gen).tolist()
    return [order[i:i + n] for i in range(0, 27, n)]


# ------------------------------------------------------------------------------------------------
# one product per weight-gradient element: one live position per input channel
# ------------------------------------------------------------------------------------------------

def live_voxel_inputs(b, ci, r, gen, positions, bound=1023):
    """-> (x, live): x (b, ci, r, r, r) with exactly one non-zero voxel per input channel, a non-zero integer |v| <= bound; channel c
    sits at positions[c % len(positions)] = (cloud, ix, iy, iz).  live = [(cloud, (ix, iy, iz), value)] per channel.  Then
    grad_w[o, c, tap] = grad_y[cloud_c, o, v_c - offset(tap)] * x[cloud_c, c, v_c], offset = TAPS[tap] - 1, 0 where that falls outside
    the grid: `live_voxel_grad_w`."""
    x = torch.zeros(b, ci, r, r, r)
    vals = short_ints((ci,), gen, bound, nonzero=True)
    live = []
    for c in range(ci):
        bi, ix, iy, iz = positions[c % len(positions)]
        x[bi, c, ix, iy, iz] = vals[c]
        live.append((bi, (ix, iy, iz), float(vals[c])))
    return x, live


def live_voxel_grad_w(live, gy):
    r = gy.shape[-1]
    gw = torch.zeros((gy.shape[1], len(live), 3, 3, 3), dtype=gy.dtype, device=gy.device)
    for c, (bi, v, val) in enumerate(live):
        for d in TAPS:
            p = [v[a] - (d[a] - 1) for a in range(3)]
            if all(0 <= q < r for q in p):
                gw[:, c][(slice(None), *d)] = gy[bi, :, p[0], p[1], p[2]] * val
    return gw


def voxel_positions(b, r):
    """Where the backward-weight kernels can go wrong: both ends of z (and the k-step seam z = 15 | 16 at R = 32), the four-row ring's
    wraps y = 0, 3, 4, R - 1, both ends of x, the first and the last cloud."""
    zs = [0, r - 1] + ([15, 16] if r == 32 else [])
    return [(bi, ix, iy, iz) for bi in sorted({0, b - 1}) for ix in (0, r - 1) for iy in (0, 3, 4, r - 1) for iz in zs]


def live_point_inputs(b, ci, n, gen, positions, bound=1023):
    """The 1x1 analogue: x (b, ci, n) with one non-zero point per channel at positions[c % len] = (cloud, point);
    grad_w[o, c] = grad_y[cloud_c, o, n_c] * x[cloud_c, c, n_c]: `live_point_grad_w`."""
    x = torch.zeros(b, ci, n)
    vals = short_ints((ci,), gen, bound, nonzero=True)
    live = []
    for c in range(ci):
        bi, pt = positions[c % len(positions)]
        x[bi, c, pt] = vals[c]
        live.append((bi, pt, float(vals[c])))
    return x, live


def live_point_grad_w(live, gy):
    gw = torch.zeros((gy.shape[1], len(live)), dtype=gy.dtype, device=gy.device)
    for c, (bi, pt, val) in enumerate(live):
        gw[:, c] = gy[bi, :, pt] * val
    return gw


def point_positions(b, n):
    return [(bi, pt) for bi in sorted({0, b - 1}) for pt in (0, 255, 256, n - 1)]


def rotated(positions, k):
    """positions rotated by k: launch l of a sweep hands channel c the entry c + l * ci."""
    k %= len(positions)
    return positions[k:] + positions[:k]


def exact_sum_bound(count):
    """Largest |v| for which a sum of `count` integers stays below 2^24 in any order (every fp32 partial sum is then exact)."""
    return min(1023, ((1 << 24) - 1) // count)


# ------------------------------------------------------------------------------------------------
# the instantiations csrc/route.h selects, and the smallest shapes that take them
# ------------------------------------------------------------------------------------------------

CONV_KERNELS = {0: 'igemm', 1: 'igemm32', 2: 'pipe', 3: 'wide'}         # route::ConvKernel; igemm32: the 32-row weight tile
PW_KERNELS = {0: 'gemm', 1: 'pipe', 2: 'wide'}                          # route::PwKernel


def conv_signature(kernel, nsplit, tx, ty, tz, vec, rows):
    return f'{CONV_KERNELS[kernel]}<{nsplit},{tx},{ty},{tz},{"vec" if vec else "scalar"}>r{rows}'


def pw_signature(kernel, nsplit, mb, pf, wmw, vec):
    return f'{PW_KERNELS[kernel]}<{nsplit},mb{mb},pf{pf},wmw{wmw},{"vec" if vec else "scalar"}>'


def _conv_row(shape, tile, vec, special=None, tile3=None, unreached=False):
    """One Conv3d row: Igemm on `tile` in every mode and both directions (`tile3`: the tile of bf16x3, which never takes the
    512-voxel one), except the (direction, nsplit) entries of `special` = {(dir, nsplit): (kernel id, rows)}."""
    listed = {}
    for direction in ('fwd', 'bwd'):
        for nsplit in (1, 2, 3):
            kernel, rows = (special or {}).get((direction, nsplit), (0, 64))
            t = tile3 if nsplit == 3 and tile3 else tile
            if kernel == 3:
                t = (4, 4, shape[3])
            listed[direction, nsplit] = conv_signature(kernel, nsplit, *t, vec, rows)
    return {'kind': 'conv', 'shape': shape, 'listed': listed, 'unreached': unreached,
            'id': 'conv-' + 'x'.join(map(str, shape)) + '-tile' + 'x'.join(map(str, tile)) + ('-vec' if vec else '-scalar')}


def _pw_row(shape, fwd, bwd, tag):
    """One 1x1 row: fwd / bwd = per nsplit 1, 2, 3 the (kernel id, mb, pf, wmw, vec) of the direction."""
    listed = {(d, ns): pw_signature(v[0], ns, *v[1:]) for d, per in (('fwd', fwd), ('bwd', bwd)) for ns, v in zip((1, 2, 3), per)}
    return {'kind': 'pw', 'shape': shape, 'listed': listed, 'unreached': False, 'id': 'pw-' + 'x'.join(map(str, shape)) + '-' + tag}


def _gemm(mb, vec, pf2=False):
    """Gemm in all three modes (pf = 2 at nsplit 2 on the four-block tile without the straight-line loop)."""
    return [(0, mb, 1, 0, vec), (0, mb, 2 if pf2 else 1, 0, vec), (0, mb, 1, 0, vec)]


def _pipe(wide=0):
    """The four-block vector tile: Pipe at nsplit 1 and 2 (or Wide with `wide`-block items at nsplit 2), Gemm at nsplit 3."""
    return [(1, 4, 1, 0, 1), (2, 4, 1, wide, 1) if wide else (1, 4, 1, 0, 1), (0, 4, 1, 0, 1)]


# (B, Ci, Co, R) resp. (B, K, M, N); backward-data is the same product with the two channel counts exchanged.  `unreached`: the rows
# whose tiles no other kernel-level test launches -- the scalar-staging (2,8,8) and (4,8,8) tiles in every mode and
# conv3d_igemm_bf16_kernel<2,4,4,32,true> with the 64-row weight tile, the first convolution of the benched PVCNN step.
ROUTE_CASES = [
    _conv_row((1, 16, 24, 8), (1, 8, 8), 1),
    _conv_row((64, 4, 8, 8), (2, 8, 8), 1),
    _conv_row((128, 4, 8, 8), (4, 8, 8), 1),
    _conv_row((2, 5, 7, 6), (1, 8, 8), 0),
    _conv_row((90, 3, 8, 6), (2, 8, 8), 0, unreached=True),
    _conv_row((130, 3, 8, 5), (4, 8, 8), 0, unreached=True),
    _conv_row((1, 5, 7, 10), (4, 4, 16), 0),
    _conv_row((2, 8, 12, 12), (2, 4, 16), 1),
    _conv_row((2, 16, 24, 12), (2, 4, 16), 1, {('fwd', 2): (2, 64)}),                         # Ci % 16 == 0: the pipe kernel
    _conv_row((48, 4, 8, 16), (4, 4, 16), 1),
    _conv_row((1, 4, 8, 32), (2, 4, 32), 1, {('fwd', 2): (1, 32), ('bwd', 2): (1, 32)}),
    _conv_row((1, 16, 40, 32), (2, 4, 32), 1, {('bwd', 2): (1, 32)}),
    _conv_row((8, 4, 8, 32), (4, 4, 32), 1, {('fwd', 2): (1, 32), ('bwd', 2): (1, 32)}, tile3=(2, 4, 32)),
    _conv_row((8, 9, 64, 32), (4, 4, 32), 1, {('bwd', 2): (1, 32)}, tile3=(2, 4, 32), unreached=True),
    _conv_row((1, 32, 64, 32), (2, 4, 32), 1, {('fwd', 2): (3, 64), ('bwd', 2): (1, 32)}),    # the persistent wide kernel
    _pw_row((2, 9, 64, 300), _gemm(2, 1), _gemm(2, 1), 'gemm-mb2-vec'),
    _pw_row((1, 5, 7, 37), _gemm(2, 0), _gemm(2, 0), 'gemm-mb2-scalar'),
    _pw_row((1, 64, 128, 262), _gemm(4, 0, pf2=True), _gemm(2, 0), 'gemm-mb4-scalar-pf2'),
    _pw_row((2, 64, 128, 512), _pipe(), _gemm(2, 1), 'pipe'),
    _pw_row((2, 24, 128, 260), _pipe(), _gemm(2, 1), 'pipe-ntail'),
    _pw_row((1, 64, 256, 512), _pipe(wide=2), _gemm(2, 1), 'wide-256rows'),
    _pw_row((1, 256, 512, 256), _pipe(wide=4), _pipe(wide=2), 'wide-512rows'),
    _pw_row((1, 130, 70, 513), _gemm(4, 0, pf2=True), _gemm(4, 0, pf2=True), 'gemm-mb4-ragged'),
]


def direction_shape(row, direction):
    """The (B, Cin, Cout, L) a direction's launch is planned with: backward-data exchanges the channel counts."""
    b, ci, co, l = row['shape']
    return (b, ci, co, l) if direction == 'fwd' else (b, co, ci, l)
