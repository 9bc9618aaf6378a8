"""The training kernels on OFFSET VIEWS INSIDE POISONED ALLOCATIONS (tests/embedded.py): what a parameter inside
GradBucketReducer's `pflat`, a gradient slot of a flat bucket or a channel slice of a concatenation is to a kernel -- a pointer
4, 8 or 12 bytes off a 16-byte boundary with live memory right in front of and behind it.

Every case has one form.  EXPECTED is the same backend call on ordinary fresh tensors with the same values (a CPU oracle or an
fp64 evaluation next to it where the sibling test has one).  ACTUAL is the call with ONE role at a time embedded at offsets
0, 1, 2, 3 elements behind a 16-byte boundary, everything else fresh.  After each call: (a) the result against the expectation,
(b) the sentinel around the embedded tensor bit for bit, (c) no NaN in the result.  Offset 0 keeps the vector path and adds only
the NaN surroundings.

Bars.  torch.equal at offset 0, at every offset of the ops the numerics contract of include/pvcnn_hip.h calls bit-exact and for
moved gradient destinations (the same sums stored elsewhere).  Where an offset changes the GEMM / convolution kernel that runs --
`x` of the products, the weight where it is a GEMM operand as stored -- the sibling tests' bars against fp64: 1e-5 of the
result's largest entry for fp32 / f16x2 / bf16x3, 4e-3 for plain bf16, 1e-5 for the statistics partials.

Refusals.  At this level a call on a misaligned operand may end in a RuntimeError that names the alignment, raised by a
PVCNN_REQUIRE in front of every launch; REFUSALS is the literal table of the (entry, role) pairs that may.  Any other pair that
raises fails its test; a pair of the table that succeeds is held to the same bars as everything else.

`[embedded] entry: role=....` lines (one mark per offset: `.` ran, `x` refused) are the record of what ran."""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

import embedded as E
from conftest import grid_coords, synth_cloud

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
OFFS = (0, 1, 2, 3)

# (HipBackend method, role) -> the PVCNN_REQUIRE that may refuse a pointer off a 16-byte boundary
REFUSALS = {
    ('conv3d_forward_split', 'x'): 'conv3d_bf16.hip conv3d_fwd_split_impl: !p.vec || aligned16(x)',
    ('conv3d_backward_data_split', 'grad_y'): 'the same launch with Ci and Co exchanged',
    ('conv3d_backward_weight_f16', 'x'): 'conv3d_wgrad_f16.hip: aligned16(x) && aligned16(grad_y)',
    ('conv3d_backward_weight_f16', 'grad_y'): 'conv3d_wgrad_f16.hip: aligned16(x) && aligned16(grad_y)',
    ('pwconv_backward_weight_f16', 'x'): 'pointwise_wgrad_f16.hip: aligned16(x) && aligned16(grad_y)',
    ('pwconv_backward_weight_f16', 'grad_y'): 'pointwise_wgrad_f16.hip: aligned16(x) && aligned16(grad_y)',
    ('neighbor_max_forward', 'x'): 'pool.hip pvcnn_neighbor_max_fwd: aligned16(x)',
    ('row_argmax', 'x'): 'pool.hip pvcnn_row_argmax: aligned16(x)',
    ('adam_step', 'p'): 'optim.hip: aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v)',
    ('adam_step', 'g'): 'optim.hip', ('adam_step', 'm'): 'optim.hip', ('adam_step', 'v'): 'optim.hip',
    # `part` is an array of (sum, sum) pairs read as 8-byte elements: refused 4 bytes off an 8-byte boundary (offsets 1 and 3)
    ('se_excite_forward', 'part'): 'se.hip pvcnn_se_excite_fwd: part 8-byte aligned',
    ('se_excite_backward', 'part'): 'se.hip pvcnn_se_excite_bwd: part 8-byte aligned',
    # the slot the pass writes into: HipBackend.bnact_apply_rowmax checks it itself, in front of bnact.hip's aligned16(y)
    ('bnact_apply_rowmax', 'out'): 'backend.py bnact_apply_rowmax: out 16-byte aligned rows (bnact.hip pvcnn_bnact_apply_rowmax: aligned16(y))',
}
# Alignment REQUIREs with no caller role at this level, hence no row: pool.hip pvcnn_neighbor_max_bwd's grad_x, the 8-byte `part` of
# bnact.hip pvcnn_bnact_partial_sums and the stats_part of the product entries (outputs the wrappers allocate), the 16-byte weight
# images and workspaces (allocated by the wrappers, too); pvcnn_absmax_bits' and pvcnn_bnact_apply_rowmax's x get an aligned copy.


def _rel(a, b):
    return (a.double() - b.double()).abs().max().item() / max(b.double().abs().max().item(), 1e-30)


def _flat(res):
    if isinstance(res, torch.Tensor):
        return (res,)
    return tuple(t for t in res if isinstance(t, torch.Tensor))


def _same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k)
        assert torch.equal(g, w), (what, f'output {k}', (g.double() - w.double()).abs().max().item())


def sweep(entry, call, args, roles, judge=None, pads=None, rows=None, index=(), mutated=(), offs=None):
    """call(**args) -> tensor(s).  One role at a time embedded at each offset (args are cloned per call: in-place state starts
    equal), compared with the fresh call.  judge = {role: f(outputs)}: the bar at offsets != 0 where the kernel changes;
    pads = {role: elements}; rows = {role: extra channels} (embed_rows: a batch-strided channel slice); index: roles whose
    values are followed (INDEX_SENTINEL); mutated: roles the call writes (they are outputs, too); offs = {role: offsets}."""
    def fresh():
        return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in args.items()}
    want = _flat(call(**fresh()))
    assert not any(E.has_nan(t) for t in want), entry
    marks, key = {}, entry.split(' ')[0]                  # (the HipBackend method: REFUSALS' first column)
    for role in roles:
        marks[role] = ''
        for off in (offs or {}).get(role, OFFS):
            a = fresh()
            what = (entry, role, off)
            if rows and role in rows:
                view, whole = E.embed_rows(a[role], off, rows[role])
                ok = lambda: E.rows_intact(whole, view)
            else:
                sentinel = E.INDEX_SENTINEL if role in index else None
                view, whole = E.embed(a[role], off, (pads or {}).get(role, E.MIN_PAD), sentinel)
                ok = lambda: E.intact(whole, view, sentinel)
            before = view.clone()
            a[role] = view
            try:
                got = _flat(call(**a))
            except RuntimeError as err:
                assert off != 0 and (key, role) in REFUSALS and 'align' in str(err), (what, str(err))
                assert ok() and torch.equal(view, before), what
                for name in mutated:                      # in front of every launch: nothing the call writes has moved
                    if name != role:
                        assert torch.equal(a[name], args[name]), (what, name, 'written before the refusal')
                marks[role] += 'x'
                continue
            assert ok(), (what, 'the sentinel around the embedded tensor changed')
            if role not in mutated:
                assert torch.equal(view, before), (what, 'an input was written')
            assert not any(E.has_nan(t) for t in got), (what, 'NaN in the result')
            if off == 0 or not judge or role not in judge:
                _same(got, want, what)
            else:
                judge[role](got)
            marks[role] += '.'
    print(f'[embedded] {entry}: ' + ' '.join(f'{r}={m}' for r, m in marks.items()))
    return marks


def destinations(entry, call, shapes, want, offs=OFFS):
    """Gradient destinations.  call(**{name: view}) -> tensors in the order of `shapes` (a dict name -> shape); want: what the call
    without destinations returned.  Every destination alone, then all of them back to back in one allocation with no gap, in the
    given and in the reverse order (as a bucket lays them out), at every offset: bit-equal, the surroundings intact."""
    names = list(shapes)
    layouts = [[n] for n in names] + ([names, names[::-1]] if len(names) > 1 else [])
    for off in offs:
        for layout in layouts:
            views, whole = E.back_to_back([shapes[n] for n in layout], off, DEV)
            kw = dict(zip(layout, views))
            got = _flat(call(**kw))
            what = (entry, '|'.join(layout), off)
            assert E.group_intact(whole, views), (what, 'a store outside the destinations')
            assert not any(E.has_nan(t) for t in got), (what, 'NaN in the result')
            _same(got, want, what)
            for n, v in kw.items():
                assert got[names.index(n)].data_ptr() == v.data_ptr(), (what, n, 'the destination was not used')
    print(f'[embedded] {entry}: destinations ' + ' '.join('[' + '|'.join(l) + ']' for l in layouts) + f' at offsets {tuple(offs)}')


def _stats_ok(y, part, bias_d, co):
    centred = (y.double() - bias_d.view(1, -1, *([1] * (y.dim() - 2)))).transpose(0, 1).reshape(co, -1)
    sums = part.double().sum(dim=1)
    assert _rel(sums[:, 0], centred.sum(dim=1)) < 1e-5 and _rel(sums[:, 1], (centred * centred).sum(dim=1)) < 1e-5


# ---- 1x1 products ------------------------------------------------------------------------------------------------------------------
# (B, K, M, N), the weight rows per item pvcnn_pwconv_fwd_split_route reports for f16x2 on an aligned x, and route.h's kernel for it
# (Pipe and the Gemm tile with mb = 4 share the code 128, and the query assumes an aligned x: that an x off a 16-byte boundary takes
# the non-vector Gemm kernel -- mb = 4, pf = 2 at the tile-aligned shape -- is route.h's `vec` rule as read, not something this
# file can observe; what it asserts there is the result)
PW_CASES = [((1, 9, 64, 256), 64, 'Gemm mb=2'),
            ((1, 64, 128, 256), 128, 'Pipe; off != 0: Gemm mb=4 pf=2 at a tile-aligned shape'),
            ((1, 64, 256, 256), 256, 'Wide wmw=2'),
            ((1, 256, 512, 256), 512, 'Wide wmw=4'),
            ((2, 35, 70, 260), 128, 'Pipe, ragged K, M and N')]


@pytest.mark.parametrize('shape,rows,kernel', PW_CASES, ids=['x'.join(map(str, c[0])) for c in PW_CASES])
def test_pointwise_products(hip, shape, rows, kernel):
    b, k, m, n = shape
    assert hip.lib.pvcnn_pwconv_fwd_split_route(b, k, m, n, 2) == rows, kernel
    g = torch.Generator().manual_seed(k * 131 + m)
    x, gy = torch.randn(b, k, n, generator=g).to(DEV), torch.randn(b, m, n, generator=g).to(DEV)
    w, bias = (torch.randn(m, k, generator=g) * 0.1).to(DEV), torch.randn(m, generator=g).to(DEV)
    ref_y = torch.einsum('oc,bcn->bon', w.double(), x.double()) + bias.double().view(1, -1, 1)
    ref_gx = torch.einsum('oc,bon->bcn', w.double(), gy.double())
    pad = max(E.MIN_PAD, 64 * n + 256)                     # a whole chunk of rows behind the tensor is still the sentinel
    for nsplit in (0, 1, 2, 3):
        tol = 4e-3 if nsplit == 1 else 1e-5

        def fwd(x, weight, bias):
            if nsplit == 0:
                return hip.pwconv_forward(x, weight, bias, want_stats=True)
            return hip.pwconv_forward_split(x, weight, bias, nsplit, want_stats=True)

        def bwd(grad_y, weight):
            return hip.pwconv_backward_data(grad_y, weight) if nsplit == 0 else hip.pwconv_backward_data_split(grad_y, weight, nsplit)

        def judge_fwd(got):
            assert _rel(got[0], ref_y) < tol, (shape, nsplit, _rel(got[0], ref_y))
            if nsplit != 1:
                _stats_ok(got[0], got[1], bias.double(), m)

        def judge_bwd(got):
            assert _rel(got[0], ref_gx) < tol, (shape, nsplit, _rel(got[0], ref_gx))

        name = 'pwconv_forward' if nsplit == 0 else 'pwconv_forward_split'
        sweep(f'{name} {shape} nsplit={nsplit}', fwd, dict(x=x, weight=w, bias=bias), ['x', 'weight', 'bias'], judge={'x': judge_fwd}, pads={'x': pad})
        # (fp32 backward-data reads the weight AS STORED as its GEMM operand: its alignment picks the staging path)
        name = 'pwconv_backward_data' if nsplit == 0 else 'pwconv_backward_data_split'
        sweep(f'{name} {shape} nsplit={nsplit}', bwd, dict(grad_y=gy, weight=w), ['grad_y', 'weight'],
              judge={'grad_y': judge_bwd, **({'weight': judge_bwd} if nsplit == 0 else {})}, pads={'grad_y': pad})


# ---- Conv3d ------------------------------------------------------------------------------------------------------------------------
# (B, Ci, Co, R), pvcnn_conv3d_fwd_split_route's code for f16x2 ((voxels per tile) << 8 | weight rows), route.h's kernel and tile
# (Wide and the (4,4,32) tile share the code 512 << 8 | 64: Wide is Ci % 16 == 0, Ci >= 32, Co > 32 at R = 32)
CONV_CASES = [((1, 16, 64, 8), (64 << 8) | 64, 'Igemm (1,8,8)'),
              ((64, 16, 64, 8), (128 << 8) | 64, 'Igemm (2,8,8)'),
              ((64, 16, 128, 8), (256 << 8) | 64, 'Igemm (4,8,8)'),
              ((3, 20, 64, 6), (64 << 8) | 64, 'Igemm (1,8,8), scalar staging'),
              ((2, 16, 64, 10), (256 << 8) | 64, 'Igemm (4,4,16), scalar staging'),
              ((48, 16, 64, 16), (256 << 8) | 64, 'Igemm (4,4,16)'),
              ((1, 16, 64, 16), (128 << 8) | 64, 'Pipe (2,4,16)'),
              ((1, 32, 40, 12), (128 << 8) | 64, 'Pipe (2,4,16), the fourth z quad of a row is padding'),
              ((1, 16, 32, 32), (256 << 8) | 32, 'IgemmCo32 (2,4,32)'),
              ((1, 32, 64, 32), (512 << 8) | 64, 'Wide (4,4,32) items'),
              ((8, 16, 64, 32), (512 << 8) | 64, 'Igemm (4,4,32)')]


@pytest.mark.parametrize('shape,code,kernel', CONV_CASES, ids=['x'.join(map(str, c[0])) for c in CONV_CASES])
def test_conv3d_products(hip, shape, code, kernel):
    b, ci, co, r = shape
    assert hip.lib.pvcnn_conv3d_fwd_split_route(b, ci, co, r, 2) == code, kernel
    g = torch.Generator().manual_seed(ci * 131 + co + r)
    x, gy = torch.randn(b, ci, r, r, r, generator=g).to(DEV), torch.randn(b, co, r, r, r, generator=g).to(DEV)
    w, bias = (torch.randn(co, ci, 3, 3, 3, generator=g) * 0.1).to(DEV), torch.randn(co, generator=g).to(DEV)
    truth = {}

    def ref():                                            # fp64, once, only where an offset changes the kernel
        if not truth:
            xd = x.double().requires_grad_()
            y = F.conv3d(xd, w.double(), bias.double(), padding=1)
            y.backward(gy.double())
            truth['y'], truth['gx'] = y.detach(), xd.grad
        return truth
    # a whole 16-channel chunk plus the halo behind (and in front of) the tensor is still the sentinel
    pad = max(E.MIN_PAD, 16 * r ** 3 + r * r + r + 1)
    for nsplit in (0, 1, 2, 3):
        tol = 4e-3 if nsplit == 1 else 1e-5

        def fwd(x, weight, bias):
            if nsplit == 0:
                return hip.conv3d_forward(x, weight, bias, want_stats=True)
            return hip.conv3d_forward_split(x, weight, bias, nsplit, want_stats=True)

        def bwd(grad_y, weight):
            return hip.conv3d_backward_data(grad_y, weight) if nsplit == 0 else hip.conv3d_backward_data_split(grad_y, weight, nsplit)

        def judge_fwd(got):
            assert _rel(got[0], ref()['y']) < tol, (shape, nsplit, _rel(got[0], ref()['y']))
            if nsplit != 1:
                _stats_ok(got[0], got[1], bias.double(), co)

        def judge_bwd(got):
            assert _rel(got[0], ref()['gx']) < tol, (shape, nsplit, _rel(got[0], ref()['gx']))

        name = 'conv3d_forward' if nsplit == 0 else 'conv3d_forward_split'
        marks = sweep(f'{name} {shape} nsplit={nsplit}', fwd, dict(x=x, weight=w, bias=bias), ['x', 'weight', 'bias'], judge={'x': judge_fwd}, pads={'x': pad})
        if nsplit == 0 or r % 4:                          # nothing to refuse: no vector staging of x
            assert marks['x'] == '....', (shape, nsplit, marks)
        name = 'conv3d_backward_data' if nsplit == 0 else 'conv3d_backward_data_split'
        marks = sweep(f'{name} {shape} nsplit={nsplit}', bwd, dict(grad_y=gy, weight=w), ['grad_y', 'weight'], judge={'grad_y': judge_bwd}, pads={'grad_y': pad})
        if nsplit == 0 or r % 4:
            assert marks['grad_y'] == '....', (shape, nsplit, marks)


# ---- backward-weight: destinations inside a bucket, amax buffers inside a larger one -----------------------------------------------
PW_WGRAD = [(2, 35, 70, 260), (1, 130, 200, 516), (1, 256, 256, 4)]
CONV_WGRAD = [(2, 9, 7, 8), (1, 33, 70, 12), (1, 10, 64, 16), (1, 3, 40, 32)]


def _wgrad(hip, kind, f16, shape):
    b, ci, co, l = shape
    g = torch.Generator().manual_seed(ci * 7 + co)
    sp = (l, l, l) if kind == 'conv3d' else (l,)
    x, gy = torch.randn(b, ci, *sp, generator=g).to(DEV), torch.randn(b, co, *sp, generator=g).to(DEV)
    entry = f'{kind}_backward_weight' + ('_f16' if f16 else '')
    fn = getattr(hip, entry)
    wshape = (co, ci, 3, 3, 3) if kind == 'conv3d' else (co, ci)
    want = _flat(fn(x, gy, with_bias=True))
    assert not any(E.has_nan(t) for t in want)
    truth = (F.grad.conv3d_weight(x.double(), wshape, gy.double(), padding=1) if kind == 'conv3d'
             else torch.einsum('bon,bcn->oc', gy.double(), x.double()))
    assert _rel(want[0], truth) < 1e-5 and _rel(want[1], gy.double().sum(dim=(0, *range(2, gy.dim())))) < 1e-5
    destinations(f'{entry} {shape}', lambda **kw: fn(x, gy, with_bias=True, **kw), {'out_w': wshape, 'out_b': (co,)}, want)
    _same(_flat(fn(x, gy, out_w=torch.empty(wshape, device=DEV))), want[:1], (entry, 'no bias'))
    if not f16:
        return
    amax = getattr(hip, 'conv_amax' if kind == 'conv3d' else 'pw_amax')
    for tables in (True, False):                          # amax buffers with a table, and 1-word ones
        xa, ga = (amax(x), amax(gy)) if tables else (hip.absmax_bits(x), hip.absmax_bits(gy))
        sweep(f'{entry} {shape}', lambda x_amax, gy_amax: fn(x, gy, x_amax, gy_amax, with_bias=True),
              dict(x_amax=xa, gy_amax=ga), ['x_amax', 'gy_amax'])
        _same(_flat(fn(x, gy, xa, ga, with_bias=True)), want, (entry, 'amax given'))


@pytest.mark.parametrize('shape', PW_WGRAD, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('f16', [False, True])
def test_pointwise_backward_weight_destinations(hip, shape, f16):
    _wgrad(hip, 'pwconv', f16, shape)


@pytest.mark.parametrize('shape', CONV_WGRAD, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('f16', [False, True])
def test_conv3d_backward_weight_destinations(hip, shape, f16):
    _wgrad(hip, 'conv3d', f16, shape)


def test_refusals_come_in_front_of_every_launch(hip):
    """The pairs of REFUSALS that can be handed a destination: x / grad_y of the f16x2 backward-weight entries off a 16-byte
    boundary with both destinations pre-filled -- a refusal leaves them untouched (the PVCNN_REQUIRE stands in front of the first
    launch); a success is held to the usual bar."""
    for kind, shape in (('pwconv', (2, 35, 70, 260)), ('conv3d', (2, 9, 7, 8))):
        b, ci, co, l = shape
        sp = (l, l, l) if kind == 'conv3d' else (l,)
        g = torch.Generator().manual_seed(5)
        x, gy = torch.randn(b, ci, *sp, generator=g).to(DEV), torch.randn(b, co, *sp, generator=g).to(DEV)
        entry = f'{kind}_backward_weight_f16'
        fn = getattr(hip, entry)
        wshape = (co, ci, 3, 3, 3) if kind == 'conv3d' else (co, ci)
        want = _flat(fn(x, gy, with_bias=True))
        xa, ga = hip.absmax_bits(x), hip.absmax_bits(gy)
        marks = {'x': '', 'grad_y': ''}
        for role in ('x', 'grad_y'):
            for off in OFFS:
                view, whole = E.embed(x if role == 'x' else gy, off, max(E.MIN_PAD, 16 * l ** 3 if kind == 'conv3d' else 64 * l))
                (out_w, out_b), dst = E.back_to_back([wshape, (co,)], 1, DEV)
                try:
                    got = _flat(fn(view if role == 'x' else x, view if role == 'grad_y' else gy, xa, ga, with_bias=True, out_w=out_w, out_b=out_b))
                except RuntimeError as err:
                    assert off != 0 and (entry, role) in REFUSALS and 'align' in str(err), (entry, role, off, str(err))
                    assert bool((dst.view(torch.int32) == E.NAN_BITS).all()), (entry, role, off, 'a launch ran before the refusal')
                    marks[role] += 'x'
                else:
                    _same(got, want, (entry, role, off))
                    assert E.group_intact(dst, [out_w, out_b])
                    marks[role] += '.'
                assert E.intact(whole, view)
        print(f'[embedded] {entry} {shape}: ' + ' '.join(f'{r}={m}' for r, m in marks.items()))


# ---- BatchNorm + activation ----------------------------------------------------------------------------------------------------------
def _bn_inputs(c, s, b=2, seed=0):
    g = torch.Generator().manual_seed(1000 * c + s + seed)
    x = (torch.randn(b, c, s, generator=g) * 2 + 0.7).to(DEV)
    gy = torch.randn(b, c, s, generator=g).to(DEV)
    gamma, beta = (torch.rand(c, generator=g) + 0.5).to(DEV), torch.randn(c, generator=g).to(DEV)
    return x, gy, gamma, beta


@pytest.mark.parametrize('c', [5, 67])
@pytest.mark.parametrize('s', [256, 1000])
def test_bnact_backward(hip, c, s):
    x, gy, gamma, beta = _bn_inputs(c, s)
    _, mean, rstd = hip.bnact_forward(x, gamma, beta, None, None, True, 0.1, 1e-5, 0.1)
    seed = torch.tensor([0x1234567], dtype=torch.int64, device=DEV)
    for training, amax_seg, drop in ((True, 0, None), (False, 0, None), (True, 4, None), (False, 4, None), (True, 4, (seed, 0.3))):
        def call(x, grad_y, gamma, beta, mean, rstd, **dst):
            return hip.bnact_backward(x, grad_y, gamma, beta, mean, rstd, 0.1, training, amax_seg=amax_seg, drop=drop, **dst)
        args = dict(x=x, grad_y=gy, gamma=gamma, beta=beta, mean=mean, rstd=rstd)
        tag = f'bnact_backward C={c} S={s} training={training} amax_seg={amax_seg} drop={drop is not None}'
        sweep(tag, call, args, ['x', 'grad_y', 'gamma', 'beta', 'mean', 'rstd'])
        sweep(tag + ' [strided grad_y]', call, args, ['grad_y'], rows={'grad_y': 3})
        want = _flat(call(**args))
        pick = lambda res: (res[1], res[2], res[0]) + tuple(res[3:])          # (grad_gamma, grad_beta) first: the destinations
        destinations(tag, lambda **kw: pick(call(**args, **kw)), {'out_w': (c,), 'out_b': (c,)}, pick(want))


@pytest.mark.parametrize('c,s', [(5, 256), (67, 1000)])
def test_bnact_forward_and_slices(hip, c, s):
    x, gy, gamma, beta = _bn_inputs(c, s, seed=1)
    rm, rv = torch.randn(c, device=DEV) * 0.2, torch.rand(c, device=DEV) + 0.5
    for training, amax_seg in ((True, 0), (False, 0), (True, 4), (False, 4)):
        def call(x, gamma, beta, running_mean, running_var):
            res = hip.bnact_forward(x, gamma, beta, running_mean, running_var, training, 0.1, 1e-5, 0.1, amax_seg=amax_seg)
            return tuple(res) + (running_mean, running_var)
        sweep(f'bnact_forward C={c} S={s} training={training} amax_seg={amax_seg}', call,
              dict(x=x, gamma=gamma, beta=beta, running_mean=rm, running_var=rv),
              ['x', 'gamma', 'beta', 'running_mean', 'running_var'], mutated=('running_mean', 'running_var') if training else ())
    _, mean, rstd = hip.bnact_forward(x, gamma, beta, None, None, True, 0.1, 1e-5, 0.1)
    # statistics given (a convolution epilogue + bn_finalize): the apply pass alone
    sweep(f'bnact_forward C={c} S={s} stats given', lambda x, gamma, beta, mean, rstd:
          hip.bnact_forward(x, gamma, beta, None, None, True, 0.1, 1e-5, 0.1, stats=(mean, rstd), amax_seg=4)[::3],
          dict(x=x, gamma=gamma, beta=beta, mean=mean, rstd=rstd), ['x', 'gamma', 'beta', 'mean', 'rstd'])
    sweep(f'bn_stats C={c} S={s}', lambda x: hip.bn_stats(x, None, None, 0.1, 1e-5), dict(x=x), ['x'])
    for with_gy in (True, False):
        def slices(x, grad_y, gamma, beta, mean, rstd):
            return hip.bnact_partial_sums_raw(x, grad_y if with_gy else None, gamma, beta, mean, rstd, 0.1)
        args = dict(x=x, grad_y=gy, gamma=gamma, beta=beta, mean=mean, rstd=rstd)
        sweep(f'bnact_partial_sums_raw C={c} S={s} grad_y={with_gy}', slices, args, ['x', 'grad_y', 'gamma', 'beta', 'mean', 'rstd'])
        if with_gy:
            sweep(f'bnact_partial_sums_raw C={c} S={s} [strided grad_y]', slices, args, ['grad_y'], rows={'grad_y': 3})
    P, Q = hip.bnact_partial_sums(x, gy, gamma, beta, mean, rstd, 0.1)
    sweep(f'bnact_backward_apply C={c} S={s}', lambda x, grad_y, gamma, beta, mean, rstd, sum_gamma, sum_beta, bc_mul, bc_add:
          hip.bnact_backward_apply(x, grad_y, gamma, beta, mean, rstd, sum_gamma, sum_beta, 0.1, True, bc_mul, bc_add, amax_seg=4),
          dict(x=x, grad_y=gy, gamma=gamma, beta=beta, mean=mean, rstd=rstd, sum_gamma=Q.sum(0), sum_beta=P.sum(0),
               bc_mul=torch.rand(2, c, device=DEV) + 0.5, bc_add=torch.randn(2, c, device=DEV) * 0.1),
          ['x', 'grad_y', 'gamma', 'beta', 'mean', 'rstd', 'sum_gamma', 'sum_beta', 'bc_mul', 'bc_add'])


@pytest.mark.parametrize('c,s', [(5, 512), (67, 256)])
def test_bnact_apply_rowmax_and_its_slot(hip, c, s):
    b, seg = 2, 256
    x, _, gamma, beta = _bn_inputs(c, s, seed=2)
    mean, rstd = x.mean(dim=(0, 2)), 1.0 / torch.sqrt(x.var(dim=(0, 2), unbiased=False) + 1e-5)

    def call(x, gamma, beta, mean, rstd, out=None):
        whole, amax, keys = hip.amax_and_row_keys(b, c, s, seg, DEV)
        whole.zero_()
        y, winners, values = hip.bnact_apply_rowmax(x, gamma, beta, mean, rstd, 0.0, seg, amax, keys, out=out)
        return y, winners, values, amax.clone()
    args = dict(x=x, gamma=gamma, beta=beta, mean=mean, rstd=rstd)
    sweep(f'bnact_apply_rowmax C={c} S={s}', call, args, ['x', 'gamma', 'beta', 'mean', 'rstd'])
    want = _flat(call(**args))
    plain = hip.bnact_forward(x, gamma, beta, None, None, False, 0.1, 1e-5, 0.0, stats=(mean, rstd), amax_seg=seg)
    assert torch.equal(want[0], plain[0]) and torch.equal(want[3], plain[3]) and torch.equal(want[1], plain[0].max(dim=-1).indices)
    # out=: the channel slice of a wider tensor (the classifier's concatenation) -- everything outside the slice is intact
    slot, wide = E.embed_rows(torch.zeros(b, c, s, device=DEV), 0, 6)
    got = _flat(call(**args, out=slot))
    assert got[0].data_ptr() == slot.data_ptr() and E.rows_intact(wide, slot)
    assert not any(E.has_nan(t) for t in got)
    _same(got, want, ('bnact_apply_rowmax', 'out='))
    # a slot off a 16-byte boundary (the package's own is a fresh buffer with S % 256 == 0: always on one) may be refused
    # (REFUSALS), in front of the launch: the slot and everything around it untouched
    for off in (1, 2, 3):
        slot, wide = E.embed_rows(torch.zeros(b, c, s, device=DEV), off, 6)
        try:
            got = _flat(call(**args, out=slot))
        except RuntimeError as err:
            assert ('bnact_apply_rowmax', 'out') in REFUSALS and 'align' in str(err), str(err)
            assert E.rows_intact(wide, slot) and not bool(slot.any()), ('bnact_apply_rowmax', 'out', off, 'written before the refusal')
        else:
            assert E.rows_intact(wide, slot) and not any(E.has_nan(t) for t in got)
            _same(got, want, ('bnact_apply_rowmax', 'out=', off))


@pytest.mark.parametrize('n', [1024, 1000])
def test_concat_points(hip, n):
    b = 2
    g = torch.Generator().manual_seed(n)
    srcs = dict(s0=torch.randn(b, 9, n, generator=g).to(DEV), s1=torch.randn(b, 16, n, generator=g).to(DEV),
                s2=torch.randn(b, 130, n, generator=g).to(DEV), bc=torch.randn(b, 7, generator=g).to(DEV),
                out=torch.zeros(b, 9 + 16 + 130 + 7, n, device=DEV))

    def call(s0, s1, s2, bc, out):
        return hip.concat_points([s0, s1, s2, bc.unsqueeze(-1).expand(-1, -1, n)], out=out)
    want = _flat(call(**{k: v.clone() for k, v in srcs.items()}))
    assert torch.equal(want[0], torch.cat([srcs['s0'], srcs['s1'], srcs['s2'], srcs['bc'].unsqueeze(-1).expand(-1, -1, n)], dim=1))
    assert torch.equal(want[1], hip.absmax_tiles(want[0], 256))
    sweep(f'concat_points N={n}', call, srcs, ['s0', 's1', 's2', 'bc', 'out'], mutated=('out',))
    sweep(f'concat_points N={n} [channel-slice sources]', call, srcs, ['s0', 's1', 's2'], rows={'s0': 3, 's1': 5, 's2': 2})


@pytest.mark.parametrize('b,c,n,r', [(2, 5, 64, 4), (1, 16, 1024, 16)])
def test_trilinear_devoxelize_bnact_forward(hip, gen, b, c, n, r):
    grid = torch.randn(b, c, r ** 3, generator=gen).to(DEV)
    coords = grid_coords(gen, b, n, r).to(DEV)
    gamma, beta = (torch.rand(c, generator=gen) + 0.5).to(DEV), torch.randn(c, generator=gen).to(DEV)
    mean, rstd = grid.mean(dim=(0, 2)), 1.0 / torch.sqrt(grid.var(dim=(0, 2), unbiased=False) + 1e-4)
    addend, se = torch.randn(b, c, n, generator=gen).to(DEV), torch.rand(b, c, generator=gen).to(DEV)
    for training in (True, False):
        def call(coords, features, gamma, beta, mean, rstd, addend, se_scale):
            res = hip.trilinear_devoxelize_bnact_forward(r, training, coords, features, gamma, beta, mean, rstd, 0.1, addend, se_scale)
            return res if training else res[:1]
        sweep(f'trilinear_devoxelize_bnact_forward R={r} training={training}', call,
              dict(coords=coords, features=grid, gamma=gamma, beta=beta, mean=mean, rstd=rstd, addend=addend, se_scale=se),
              ['coords', 'features', 'gamma', 'beta', 'mean', 'rstd', 'addend', 'se_scale'])
    # the fused gather IS devoxelize(leaky_relu(bn(grid)) * se) + addend
    act = hip.bnact_forward(grid, gamma, beta, None, None, False, 0.1, 1e-4, 0.1, stats=(mean, rstd))[0]
    fused = hip.trilinear_devoxelize_bnact_forward(r, False, coords, grid, gamma, beta, mean, rstd, 0.1)[0]
    assert torch.equal(fused, hip.trilinear_devoxelize_forward(r, False, coords, act)[0])


# ---- Linear + BatchNorm1d + ReLU on a handful of rows ----------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,cin,cout', [(16, 259, 256), (3, 5, 7), (32, 515, 512)])
def test_dense_bn_relu(hip, rows, cin, cout):
    assert hip.dense_bn_relu_supported(rows, cin, cout)
    g = torch.Generator().manual_seed(rows * cin)
    x, gy = torch.randn(rows, cin, generator=g).to(DEV), torch.randn(rows, cout, generator=g).to(DEV)
    w, bias = (torch.randn(cout, cin, generator=g) * 0.1).to(DEV), torch.randn(cout, generator=g).to(DEV)
    gamma, beta = (torch.rand(cout, generator=g) + 0.5).to(DEV), torch.randn(cout, generator=g).to(DEV)
    rm, rv = (torch.randn(cout, generator=g) * 0.2).to(DEV), (torch.rand(cout, generator=g) + 0.5).to(DEV)

    def fwd(x, weight, bias, gamma, beta, running_mean, running_var):
        counter = torch.zeros((), dtype=torch.int64, device=DEV)
        res = hip.dense_bn_relu_forward(x, weight, bias, gamma, beta, running_mean, running_var, counter, 1e-5, 0.1)
        return tuple(res) + (running_mean, running_var, counter)
    fargs = dict(x=x, weight=w, bias=bias, gamma=gamma, beta=beta, running_mean=rm, running_var=rv)
    sweep(f'dense_bn_relu_forward {(rows, cin, cout)}', fwd, fargs, list(fargs), mutated=('running_mean', 'running_var'))
    y, z, mean, rstd = hip.dense_bn_relu_forward(x, w, bias, gamma, beta, None, None, None, 1e-5, 0.1)
    lin = x.double() @ w.double().t() + bias.double()
    bn = (lin - lin.mean(0)) / torch.sqrt(lin.var(0, unbiased=False) + 1e-5) * gamma.double() + beta.double()
    assert _rel(z, lin) < 1e-5 and _rel(y, torch.relu(bn)) < 1e-5

    def bwd(x, grad_y, z, mean, rstd, gamma, beta, **dst):
        return hip.dense_bn_relu_backward(x, grad_y, z, mean, rstd, gamma, beta, **dst)
    bargs = dict(x=x, grad_y=gy, z=z, mean=mean, rstd=rstd, gamma=gamma, beta=beta)
    sweep(f'dense_bn_relu_backward {(rows, cin, cout)}', bwd, bargs, list(bargs))
    want = _flat(bwd(**bargs))
    pick = lambda res: tuple(res[1:]) + (res[0],)
    destinations(f'dense_bn_relu_backward {(rows, cin, cout)}', lambda **kw: pick(bwd(**bargs, **kw)),
                 {'out_w': (cout, cin), 'out_b': (cout,), 'out_gamma': (cout,), 'out_beta': (cout,)}, pick(want))


# ---- scatter / gather family ---------------------------------------------------------------------------------------------------------
def _vox_inputs(gen, b, c, n, r):
    feat = torch.randn(b, c, n, generator=gen)
    co = synth_cloud(gen, b, n, 'cube')
    co = co / co.amax(dim=(1, 2), keepdim=True).clamp(min=1e-6)
    norm = torch.clamp(co * r, 0, r - 1)
    return feat, torch.round(norm).to(torch.int32).contiguous(), norm.contiguous()


@pytest.mark.parametrize('b,c,n,r', [(2, 5, 64, 4), (1, 16, 1024, 16)])
def test_voxelize_and_devoxelize(hip, oracle, gen, b, c, n, r):
    feat, vox, norm = _vox_inputs(gen, b, c, n, r)
    gy_grid, gy_pts = torch.randn(b, c, r ** 3, generator=gen), torch.randn(b, c, n, generator=gen)
    o_out, o_ind, o_cnt = oracle.avg_voxelize_forward(feat, vox, r)
    h_out, h_ind, h_cnt = hip.avg_voxelize_forward(feat.to(DEV), vox.to(DEV), r)
    assert torch.equal(h_out.cpu(), o_out) and torch.equal(h_ind.cpu(), o_ind) and torch.equal(h_cnt.cpu(), o_cnt)
    for memo in (True, False):                            # the plan-and-apply route, and the one-shot C entry
        hip.seam_plan_memo = memo
        try:
            sweep(f'avg_voxelize_forward R={r} plan memo={memo}', lambda features, coords: hip.avg_voxelize_forward(features, coords, r),
                  dict(features=feat.to(DEV), coords=vox.to(DEV)), ['features', 'coords'], index=('coords',))
        finally:
            del hip.seam_plan_memo
    assert torch.equal(hip.avg_voxelize_backward(gy_grid.to(DEV), h_ind, h_cnt).cpu(), oracle.avg_voxelize_backward(gy_grid, o_ind, o_cnt))
    sweep(f'avg_voxelize_backward R={r}', hip.avg_voxelize_backward, dict(grad_y=gy_grid.to(DEV), indices=h_ind, cnt=h_cnt),
          ['grad_y', 'indices', 'cnt'], index=('indices',))
    grid = torch.randn(b, c, r ** 3, generator=gen)
    co = grid_coords(gen, b, n, r)
    o = oracle.trilinear_devoxelize_forward(r, True, co, grid)
    h = hip.trilinear_devoxelize_forward(r, True, co.to(DEV), grid.to(DEV))
    for a, e in zip(h, o):
        assert torch.equal(a.cpu(), e)
    for training in (True, False):
        sweep(f'trilinear_devoxelize_forward R={r} training={training}',
              lambda coords, features: hip.trilinear_devoxelize_forward(r, training, coords, features)[:3 if training else 1],
              dict(coords=co.to(DEV), features=grid.to(DEV)), ['coords', 'features'])
    assert torch.equal(hip.trilinear_devoxelize_backward(gy_pts.to(DEV), h[1], h[2], r).cpu(), oracle.trilinear_devoxelize_backward(gy_pts, o[1], o[2], r))
    for memo in (True, False):
        hip.seam_plan_memo = memo
        try:
            bargs = dict(grad_y=gy_pts.to(DEV), indices=h[1], weights=h[2])
            call = lambda grad_y, indices, weights: hip.trilinear_devoxelize_backward(grad_y, indices, weights, r)
            sweep(f'trilinear_devoxelize_backward R={r} plan memo={memo}', call, bargs, ['grad_y', 'indices', 'weights'], index=('indices',))
            sweep(f'trilinear_devoxelize_backward R={r} plan memo={memo} [strided grad_y]', call, bargs, ['grad_y'], rows={'grad_y': 3})
        finally:
            del hip.seam_plan_memo
    sweep(f'voxel_coords R={r}', lambda coords: hip.voxel_coords(coords, r, True, 0.0), dict(coords=norm.to(DEV)), ['coords'])


@pytest.mark.parametrize('b,c,n,m,u', [(1, 7, 256, 33, 8), (2, 5, 64, 16, 4)])
def test_grouping_gather_and_interpolation(hip, oracle, gen, b, c, n, m, u):
    f = torch.randn(b, c, n, generator=gen)
    idx = torch.randint(0, n, (b, m, u), generator=gen, dtype=torch.int32)
    idx[:, :, u // 2:] = idx[:, :, :1]
    g4 = torch.randn(b, c, m, u, generator=gen)
    assert torch.equal(hip.grouping_forward(f.to(DEV), idx.to(DEV)).cpu(), oracle.grouping_forward(f, idx))
    assert torch.equal(hip.grouping_backward(g4.to(DEV), idx.to(DEV), n).cpu(), oracle.grouping_backward(g4, idx, n))
    sweep('grouping_forward', hip.grouping_forward, dict(features=f.to(DEV), indices=idx.to(DEV)), ['features', 'indices'], index=('indices',))
    sweep('grouping_backward', lambda grad_y, indices: hip.grouping_backward(grad_y, indices, n),
          dict(grad_y=g4.to(DEV), indices=idx.to(DEV)), ['grad_y', 'indices'], index=('indices',))
    for mm in (m, 32):                                    # 32: a multiple of 4 (the vector path of the gather)
        idx2 = torch.randint(0, n, (b, mm), generator=gen, dtype=torch.int32)
        g3 = torch.randn(b, c, mm, generator=gen)
        assert torch.equal(hip.gather_features_forward(f.to(DEV), idx2.to(DEV)).cpu(), oracle.gather_features_forward(f, idx2))
        assert torch.equal(hip.gather_features_backward(g3.to(DEV), idx2.to(DEV), n).cpu(), oracle.gather_features_backward(g3, idx2, n))
        sweep(f'gather_features_forward M={mm}', hip.gather_features_forward, dict(features=f.to(DEV), indices=idx2.to(DEV)),
              ['features', 'indices'], index=('indices',))
        sweep(f'gather_features_backward M={mm}', lambda grad_y, indices: hip.gather_features_backward(grad_y, indices, n),
              dict(grad_y=g3.to(DEV), indices=idx2.to(DEV)), ['grad_y', 'indices'], index=('indices',))
    pts = synth_cloud(gen, b, n, 's3dis')
    ctr = pts[:, :, torch.randperm(n, generator=gen)[:m]].contiguous()
    feats = torch.randn(b, c, m, generator=gen)
    o = oracle.three_nearest_neighbors_interpolate_forward(pts, ctr, feats)
    h = hip.three_nearest_neighbors_interpolate_forward(pts.to(DEV), ctr.to(DEV), feats.to(DEV))
    for a, e in zip(h, o):
        assert torch.equal(a.cpu(), e)
    sweep('three_nearest_neighbors_interpolate_forward', hip.three_nearest_neighbors_interpolate_forward,
          dict(points_coords=pts.to(DEV), centers_coords=ctr.to(DEV), centers_features=feats.to(DEV)),
          ['points_coords', 'centers_coords', 'centers_features'])
    g3 = torch.randn(b, c, n, generator=gen)
    assert torch.equal(hip.three_nearest_neighbors_interpolate_backward(g3.to(DEV), h[1], h[2], m).cpu(),
                       oracle.three_nearest_neighbors_interpolate_backward(g3, o[1], o[2], m))
    sweep('three_nearest_neighbors_interpolate_backward',
          lambda grad_y, indices, weights: hip.three_nearest_neighbors_interpolate_backward(grad_y, indices, weights, m),
          dict(grad_y=g3.to(DEV), indices=h[1], weights=h[2]), ['grad_y', 'indices', 'weights'], index=('indices',))
    assert torch.equal(hip.ball_query(ctr.to(DEV), pts.to(DEV), 0.3, u).cpu(), oracle.ball_query(ctr, pts, 0.3, u))
    sweep('ball_query', lambda centers_coords, points_coords: hip.ball_query(centers_coords, points_coords, 0.3, u),
          dict(centers_coords=ctr.to(DEV), points_coords=pts.to(DEV)), ['centers_coords', 'points_coords'])


@pytest.mark.parametrize('b,n,m', [(1, 1024, 64), (1, 512, 17)])
def test_furthest_point_sampling(hip, oracle, gen, b, n, m):
    pts = synth_cloud(gen, b, n, 's3dis')
    assert torch.equal(hip.furthest_point_sampling(pts.to(DEV), m).cpu(), oracle.furthest_point_sampling(pts, m))
    sweep(f'furthest_point_sampling N={n} M={m}', lambda coords: hip.furthest_point_sampling(coords, m), dict(coords=pts.to(DEV)), ['coords'])


# ---- pooling, SE, mask selection, the box loss, Adam -----------------------------------------------------------------------------------
def test_pooling(hip, gen):
    from pvcnn_amd import workload
    from pvcnn_amd.modules.functional.pooling import neighbor_max
    x = torch.relu(torch.randn(2, 5, 33, 8, generator=gen)).mul(4).round().div(4).to(DEV)
    ref = x.max(dim=-1)
    out, winners = hip.neighbor_max_forward(x)
    assert torch.equal(out, ref.values) and torch.equal(winners.long(), ref.indices)
    sweep('neighbor_max_forward', hip.neighbor_max_forward, dict(x=x), ['x'])
    g = torch.randn(2, 5, 33, generator=gen).to(DEV)
    sweep('neighbor_max_backward', lambda grad_out: hip.neighbor_max_backward(grad_out, winners, 8), dict(grad_out=g), ['grad_out'])
    rows = torch.relu(torch.randn(3, 7, 260, generator=gen)).mul(2).round().div(2).to(DEV)
    w, v = hip.row_argmax(rows, with_values=True)
    assert torch.equal(w, rows.max(dim=-1).indices) and torch.equal(v, rows.max(dim=-1).values)
    sweep('row_argmax', lambda x: hip.row_argmax(x, with_values=True), dict(x=rows), ['x'])
    # through the functions the models call, nothing may raise: a misaligned input is copied (or takes torch.max)
    for off in OFFS:
        xe = E.embed(x, off)[0].requires_grad_()
        (neighbor_max(xe) * g).sum().backward()
        assert torch.equal(xe.grad, torch.zeros_like(x).scatter_(-1, ref.indices.unsqueeze(-1), g.unsqueeze(-1)))
        re_, whole = E.embed(rows, off)
        re_.requires_grad_()
        tap, pooled = workload.tap_and_pool(re_)
        assert torch.equal(pooled, rows.max(dim=-1).values) and E.intact(whole, re_)


def test_se_excitation(hip):
    torch.manual_seed(5)
    c, b, slices, h, s3 = 20, 3, 4, 6, 4096
    part_a = torch.randn(c, b, slices, 2, device=DEV) * (s3 / slices) ** 0.5
    part_p = torch.randn(c, b, slices, 2, device=DEV) * (s3 / slices) ** 0.5
    gam, bet = torch.randn(c, device=DEV), torch.randn(c, device=DEV)
    w1, w2 = torch.randn(h, c, device=DEV) / c ** 0.5 * 8, torch.randn(c, h, device=DEV) / h ** 0.5
    # `part` is an array of (sum, sum) PAIRS the kernels read as 8-byte elements: off its element's natural alignment (offsets 1
    # and 3) the entries refuse it (REFUSALS; every output is the wrapper's own allocation, so what the sweep can see of "in
    # front of the launch" is the untouched operand); every other operand is an array of floats
    marks = sweep('se_excite_forward', lambda part, gamma, beta, w1, w2: hip.se_excite_forward(part, gamma, beta, w1, w2, s3),
                  dict(part=part_a, gamma=gam, beta=bet, w1=w1, w2=w2), ['part', 'gamma', 'beta', 'w1', 'w2'])
    assert marks['part'][0] == marks['part'][2] == '.', marks
    a_sum, ax_sum, sq, hd, ex = hip.se_excite_forward(part_a, gam, bet, w1, w2, s3)
    bargs = dict(part=part_p, a_sum=a_sum, ax_sum=ax_sum, gamma=gam, beta=bet, squeezed=sq, hidden=hd, excite=ex, w1=w1, w2=w2)
    marks = sweep('se_excite_backward', lambda **a: hip.se_excite_backward(*a.values(), s3), bargs, list(bargs))
    assert marks['part'][0] == marks['part'][2] == '.', marks


def test_mask_select_and_box_loss(hip, gen):
    from test_gpu_frustum_loss import _case
    b, n, m = 3, 1000, 64
    mask = torch.rand(b, n, generator=gen) < 0.3
    mask[1] = False
    choices = torch.randint(0, 1 << 20, (b, m), generator=gen, dtype=torch.int32)
    sweep('mask_select', lambda choices: hip.mask_select(mask.to(DEV), m, choices=choices), dict(choices=choices.to(DEV)),
          ['choices'], index=('choices',))
    # the mask is bytes (tests/embedded.py lays out 4-byte elements): the same construction by hand, at byte offsets 0..3, with a
    # non-zero sentinel -- a byte read past a cloud's row would count as foreground and move every pick
    want = hip.mask_select(mask.to(DEV), m, choices=choices.to(DEV))
    for off in OFFS:
        whole = torch.full((E.MIN_PAD + off + b * n + E.MIN_PAD,), 0xA5, dtype=torch.uint8, device=DEV)
        view = whole[E.MIN_PAD + off:E.MIN_PAD + off + b * n].view(b, n)
        view.copy_(mask.to(DEV))
        assert torch.equal(hip.mask_select(view, m, choices=choices.to(DEV)), want), off
        assert torch.equal(hip.mask_select(view.view(torch.bool), m, seed=torch.tensor([42, 0], device=DEV)),
                           hip.mask_select(mask.to(DEV), m, seed=torch.tensor([42, 0], device=DEV))), off
        assert bool((whole[:E.MIN_PAD + off] == 0xA5).all()) and bool((whole[E.MIN_PAD + off + b * n:] == 0xA5).all())
        assert torch.equal(view, mask.to(DEV).view(torch.uint8))
    nh, ns = 12, 8
    templates, inp, tgt = _case(5, nh, ns, 8, 3, 1.0)
    names = ['center', 'center_reg', 'heading_scores', 'size_scores', 'heading_residuals_normalized', 'size_residuals_normalized',
             'heading_residuals', 'size_residuals']
    args = {k: inp[k].to(DEV) for k in names}
    args.update(heading_residual=tgt['heading_residual'].to(DEV), size_residual=tgt['size_residual'].to(DEV),
                center_t=tgt['center'].to(DEV), templates=templates.to(DEV),
                bin_centers=(torch.arange(nh, dtype=torch.float32) * (2 * math.pi / nh)).to(DEV))
    hid, sid = tgt['heading_bin_id'].to(DEV), tgt['size_template_id'].to(DEV)

    def loss(**a):
        return hip.frustum_box_loss(*[a[k] for k in names], hid, sid, a['heading_residual'], a['size_residual'], a['center_t'],
                                    a['templates'], a['bin_centers'], 2 * math.pi / nh, 1.0, 1.0, 10.0)
    sweep('frustum_box_loss', loss, args, list(args))


def test_adam_step(hip):
    from pvcnn_amd.modules.functional.backend import _run
    hyper = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 1e-4], device=DEV)

    def step(p, g, m, v):
        count = torch.full((1,), 3.0, device=DEV)
        _run(hip.lib.pvcnn_adam_step, 'adam_step', count, p, g, m, v, p.numel(), count, hyper, 1)
        return p, m, v, count
    gen = torch.Generator().manual_seed(1)
    for n in (1021, 1022, 1023, 4096, 5):                 # n = 1, 2, 3 (mod 4): the elements behind n in all four buffers
        p, g = torch.randn(n, generator=gen).to(DEV), torch.randn(n, generator=gen).to(DEV)
        m, v = (torch.randn(n, generator=gen) * 0.1).to(DEV), (torch.rand(n, generator=gen) * 0.01).to(DEV)
        marks = sweep(f'adam_step n={n}', step, dict(p=p, g=g, m=m, v=v), ['p', 'g', 'm', 'v'], mutated=('p', 'm', 'v'))
        assert all(mk[0] == '.' for mk in marks.values())
        # ... and all four inside poisoned allocations at once, as the buckets are
        bufs = [E.embed(t, 0) for t in (p, g, m, v)]
        got = step(*[view for view, _ in bufs])
        _same(got, step(p.clone(), g.clone(), m.clone(), v.clone()), ('adam_step', n, 'all four'))
        assert all(E.intact(whole, view) for view, whole in bufs)
        # torch.optim.Adam's arithmetic in fp64
        t = 4.0
        gd = g.double() + 1e-4 * p.double()
        md = m.double() + (gd - m.double()) * (1 - 0.9)
        vd = 0.999 * v.double() + (1 - 0.999) * gd * gd
        pd = p.double() - 1e-3 / (1 - 0.9 ** t) * md / (vd.sqrt() / math.sqrt(1 - 0.999 ** t) + 1e-8)
        assert _rel(got[0], pd) < 1e-5 and got[3].item() == 4.0


# ---- the modules: nothing raises for a contiguous float32 input at any offset -----------------------------------------------------------
def test_product_functions_take_misaligned_inputs(hip, monkeypatch):
    """voxel_conv3d and pointwise_conv, forward and backward, on an x (and a grad_y) one element off a 16-byte boundary, against
    fp64 at the usual 1e-5: the entries that refuse such a pointer (vector-staging Conv3d, both f16x2 backward-weight kernels) get
    an aligned copy from the autograd node."""
    from pvcnn_amd.modules.functional.conv3d import voxel_conv3d
    from pvcnn_amd.modules.functional.pwconv import pointwise_conv
    monkeypatch.setattr(type(hip), 'pw_wgrad_f16_min_macs', 0)          # the f16x2 backward-weight kernel at this small shape, too
    calls = []                                                          # ... and it is the kernel that ran
    for name in ('conv3d_backward_weight_f16', 'pwconv_backward_weight_f16'):
        def spy(self, *a, _orig=getattr(type(hip), name), _name=name, **k):
            calls.append(_name)
            return _orig(self, *a, **k)
        monkeypatch.setattr(type(hip), name, spy)
    g = torch.Generator().manual_seed(3)
    for kind, xs, ws in (('conv', (2, 16, 8, 8, 8), (24, 16, 3, 3, 3)), ('conv', (1, 16, 16, 16, 16), (64, 16, 3, 3, 3)),
                         ('pw', (2, 64, 1024), (128, 64))):
        x0, w0 = torch.randn(*xs, generator=g).to(DEV), (torch.randn(*ws, generator=g) * 0.1).to(DEV)
        b0, gy0 = torch.randn(ws[0], generator=g).to(DEV), torch.randn(xs[0], ws[0], *xs[2:], generator=g).to(DEV)
        xd, wd, bd = x0.double().requires_grad_(), w0.double().requires_grad_(), b0.double().requires_grad_()
        yd = F.conv3d(xd, wd, bd, padding=1) if kind == 'conv' else torch.einsum('oc,bcn->bon', wd, xd) + bd.view(1, -1, 1)
        yd.backward(gy0.double())
        for off in OFFS:
            (x, xw), (gy, gw) = E.embed(x0, off), E.embed(gy0, off)
            x.requires_grad_()
            w, bias = w0.clone().requires_grad_(), b0.clone().requires_grad_()
            del calls[:]
            y = voxel_conv3d(x, w, bias, False, 2) if kind == 'conv' else pointwise_conv(x, w, bias, False, 2)
            y.backward(gy)
            assert calls == [('conv3d' if kind == 'conv' else 'pwconv') + '_backward_weight_f16'], calls
            assert E.intact(xw, x) and E.intact(gw, gy)
            for got, want in ((y.detach(), yd.detach()), (x.grad, xd.grad), (w.grad, wd.grad), (bias.grad, bd.grad)):
                assert not E.has_nan(got) and _rel(got, want) < 1e-5, (kind, xs, off, _rel(got, want))


def test_modules_take_misaligned_inputs(hip, gen):
    """The module level -- _VoxelConv3d, SharedMLP, the BatchNorm functionals, the functional.* names the reference's models call --
    on inputs at every offset: the same bits as on a fresh tensor with the same values."""
    import torch.nn as nn
    from pvcnn_amd.modules import SharedMLP
    from pvcnn_amd.modules import functional as PF
    from pvcnn_amd.modules.functional.bnact import run_layers
    from pvcnn_amd.modules.pvconv import _VoxelConv3d
    torch.manual_seed(2)

    def both_ways(net, x0, tag):
        outs = []
        for off in (None,) + OFFS:
            x = (x0.clone() if off is None else E.embed(x0, off)[0]).requires_grad_()
            net.zero_grad(set_to_none=True)
            y = net(x)
            y.square().mean().backward()
            outs.append([y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in net.parameters()])
        for off, o in zip(OFFS, outs[1:]):
            _same(o, outs[0], (tag, off))
            assert not any(E.has_nan(t) for t in o)
    both_ways(_VoxelConv3d(16, 24, 3, stride=1, padding=1).to(DEV), torch.randn(2, 16, 8, 8, 8, device=DEV), '_VoxelConv3d')
    both_ways(SharedMLP(64, [128, 35]).to(DEV).train(), torch.randn(2, 64, 1024, device=DEV), 'SharedMLP')
    both_ways(SharedMLP(9, 16, dim=2).to(DEV).train(), torch.randn(2, 9, 33, 8, device=DEV), 'SharedMLP 2d')
    bn = nn.Sequential(nn.BatchNorm1d(67), nn.ReLU(True)).to(DEV).train()

    class Pair(nn.Module):
        def __init__(self):
            super().__init__()
            self.layers = bn

        def forward(self, x):
            return run_layers(self.layers, x)
    both_ways(Pair(), torch.randn(2, 67, 1000, device=DEV), 'BatchNorm + ReLU')

    b, c, n, r, m, u = 2, 5, 256, 8, 32, 8
    feat, vox, norm = (t.to(DEV) for t in _vox_inputs(gen, b, c, n, r))
    grid = torch.randn(b, c, r, r, r, generator=gen).to(DEV)
    idx3 = torch.randint(0, n, (b, m, u), generator=gen, dtype=torch.int32).to(DEV)
    idx2 = torch.randint(0, n, (b, m), generator=gen, dtype=torch.int32).to(DEV)
    ctr, cfeat = feat[:, :3, :m].contiguous(), torch.randn(b, c, m, generator=gen).to(DEV)
    cases = {
        'avg_voxelize': (lambda f, v: PF.avg_voxelize(f, v, r), [feat, vox]),
        'trilinear_devoxelize': (lambda gr, co: PF.trilinear_devoxelize(gr, co, r, True), [grid, norm]),
        'grouping': (PF.grouping, [feat, idx3]),
        'gather': (PF.gather, [feat, idx2]),
        'nearest_neighbor_interpolate': (PF.nearest_neighbor_interpolate, [norm, ctr, cfeat]),
        'ball_query': (lambda ce, p: PF.ball_query(ce, p, 2.0, u), [ctr, norm]),
        'furthest_point_sample': (lambda p: PF.furthest_point_sample(p, m), [norm]),
    }
    # logits_mask, kl_loss, huber_loss: torch reductions around (at most) the selection kernel.  The mask and the picks are exact;
    # a torch sum over n fp32 terms may take another order for another pointer: n * 2^-23 of the largest magnitude involved
    logits = torch.randn(b, 2, n, generator=gen).to(DEV)
    choices = torch.randint(0, 1 << 20, (b, m), generator=gen, dtype=torch.int32).to(DEV)
    err = torch.randn(b, 3, 40, generator=gen).to(DEV)
    want_sel, want_mean, want_mask = PF.logits_mask(norm.clone(), logits.clone(), m, choices=choices)
    want_kl, want_hub = PF.kl_loss(logits.clone(), logits.flip(1)), PF.huber_loss(err.clone(), 1.0)
    for off in OFFS:
        for k in range(2):
            a = [norm.clone(), logits.clone()]
            a[k], whole = E.embed(a[k], off)
            sel, mean, mask = PF.logits_mask(a[0], a[1], m, choices=choices)
            bound = n * 2.0 ** -23 * norm.abs().max().item()
            assert torch.equal(mask, want_mask) and E.intact(whole, a[k]) and not E.has_nan(sel) and not E.has_nan(mean), ('logits_mask', k, off)
            assert (mean - want_mean).abs().max().item() <= bound and (sel - want_sel).abs().max().item() <= 2 * bound, ('logits_mask', k, off)
        le, whole = E.embed(logits, off)
        kl = PF.kl_loss(le, logits.flip(1))
        assert E.intact(whole, le) and abs(kl.item() - want_kl.item()) <= 2 * b * n * 2.0 ** -23 * max(abs(want_kl.item()), 1.0), ('kl_loss', off)
        ee, whole = E.embed(err, off)
        hub = PF.huber_loss(ee, 1.0)
        assert E.intact(whole, ee) and abs(hub.item() - want_hub.item()) <= err.numel() * 2.0 ** -23 * want_hub.item(), ('huber_loss', off)
    for name, (fn, tensors) in cases.items():
        want = fn(*[t.clone() for t in tensors])
        for off in OFFS:
            for k in range(len(tensors)):
                a = [t.clone() for t in tensors]
                sentinel = E.INDEX_SENTINEL if a[k].dtype == torch.int32 else None
                a[k], whole = E.embed(a[k], off, sentinel=sentinel)
                got = fn(*a)
                assert torch.equal(got, want) and not E.has_nan(got) and E.intact(whole, a[k], sentinel), (name, k, off)


# ---- one step on packed parameters -------------------------------------------------------------------------------------------------
def test_a_step_on_packed_parameters_and_gradient_slots(hip):
    """A reduced-width PVCNN (the builder of test_gpu_train_parity.py; 13 classes: the classifier's 13-float bias is the first
    parameter of the first bucket, so everything behind it starts off a 16-byte boundary) with GradBucketReducer's packed
    parameters and gradient slots, one forward + backward: every gradient bit-equal to the same step of an identical model
    without a reducer, the parameters unchanged -- the packed layout as a whole is harmless, not only each kernel alone."""
    from pvcnn_amd import workload
    from pvcnn_amd.dp import GradBucketReducer
    from test_gpu_train_parity import NETS
    build, batch = NETS['PVCNN']
    torch.manual_seed(7)
    net = build(workload).to(DEV).train()
    for mod in net.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    twin = copy.deepcopy(net)
    x, y = (t.to(DEV) for t in batch(workload))
    reducer = GradBucketReducer(net).flatten_parameters()                   # (one bucket: the 13 floats shift everything behind them)
    try:
        params = dict(net.named_parameters())
        off_boundary = [n for n, p in params.items() if p.data_ptr() % 16]
        assert len(off_boundary) > len(params) // 2, (len(reducer.buckets), len(off_boundary), len(params))
        before = {n: p.detach().clone() for n, p in params.items()}
        slots = {n: p.grad.data_ptr() for n, p in params.items()}          # (the views of the flat buckets)
        reducer.zero_grad()
        oa = net(x)
        F.cross_entropy(oa, y).backward()
        in_slot = sum(p.grad is not None and p.grad.data_ptr() == slots[n] for n, p in params.items())
        reducer.finish()
        ob = twin(x)
        F.cross_entropy(ob, y).backward()
        assert in_slot > len(params) // 2, (in_slot, len(params))           # the kernels wrote into the buckets
        # (the logits, not the loss: torch's mean over B * N terms is not bit-reproducible from call to call on this device)
        assert not E.has_nan(oa) and torch.equal(oa, ob)
        for (n1, p1), (n2, p2) in zip(net.named_parameters(), twin.named_parameters()):
            assert p1.grad.data_ptr() == slots[n1]
            assert not E.has_nan(p1.grad) and torch.equal(p1.grad, p2.grad), (n1, p1.data_ptr() % 16, (p1.grad - p2.grad).abs().max().item())
            assert torch.equal(p1.detach(), before[n1]) and torch.equal(p1.detach(), p2.detach()), n1
        for (n1, b1), (n2, b2) in zip(net.named_buffers(), twin.named_buffers()):
            assert torch.equal(b1, b2), n1
        print(f'[embedded] packed step: {len(params)} parameters in {len(reducer.buckets)} buckets, {len(off_boundary)} off a 16-byte '
              f'boundary, {in_slot} gradients written into their slots')
    finally:
        reducer.remove()
