"""The `fp32` and `bf16x3` arithmetic modes and the python-level switches of the live backend, THROUGH the modules' glue.

`HipBackend.conv_math` / `pw_math` select the arithmetic of the Conv3d / 1x1 products; the glue branches on them in
functional/conv3d.py (conv_nsplit), functional/pwconv.py (pw_nsplit), functional/bnact.py (_amax_seg_for: the BatchNorm passes emit
and hand over amax tables only for an f16x2 consumer), workload.py (the concatenation's amax tag), functional/_product.py (which
backward-weight kernel serves, whether x_amax is kept) and the weight bank (image pairs keyed by nsplit).  The kernel tests call the
kernels with an explicit nsplit; everything that goes through autograd elsewhere runs in the default mode.  Here the switches are set
as plain attributes on the LIVE backend object (`functional.backend._backend`, what the modules see -- not the `hip` fixture, a
fresh HipBackend the modules never meet), in-process, no environment variable, no child process.

Every test wraps the backend's product methods (test_gpu_train_parity.count_native_calls, plus the `nsplit` argument of the split
launches) and asserts WHICH kernel family served -- a test that sets `conv_math = 'fp32'` and then runs f16x2 kernels fails on the call
record alone, whatever its numbers say:
  fp32    no *_split / *_igemm_split / *_gemm_split call, the fp32 entry points serve, backward-weight on the fp32-MFMA kernel;
  bf16x3  the split launches, each with nsplit == 3; backward-weight on the fp32-MFMA kernel (_product.backward: the f16x2 kernel
          serves nsplit 1 and 2 only);
  f16x2   the split launches with nsplit == 2; backward-weight on the f16x2 kernel where it serves (Conv3d: R in {8, 12, 16, 32};
          1x1: N % 4 == 0 and the product at or above `pw_wgrad_f16_min_macs`), else on the fp32-MFMA kernel;
  a 1x1 product below `pw_split_min_macs` multiply-adds takes the fp32 kernels in every mode.
`_expected` restates these rules from the shapes; it reads nothing from the code under test.

  A  voxel_conv3d / pointwise_conv through autograd vs F.conv3d / F.conv1d in fp64, bar 1e-5 (tests/test_gpu_fuzz.py's);
  B  one training PVConv in five (conv_math, pw_math) pairs vs the oracle stack and the fp64 truth
     (test_gpu_train_parity.check_pvconv_train_gradients: its bars, its printed distances).  Both 1x1 thresholds are lowered to 0
     there, so that at these sizes the point branch's product follows `pw_math` as well (at the default thresholds it is an fp32
     launch in every mode -- that route of the same layer is C's and the default-mode test's);
  C  a SharedMLP and a classifier head (workload._classify) in the same pairs, thresholds at 0 and at their defaults, vs the same
     modules in fp64 on the CPU: 1e-5 for forward-only quantities, TOL_LAYER for gradients; f16x2 twice from one state: equal bits;
     and an armed weight bank across a change of mode (its pairs are f16x2 images: served in f16x2, never in bf16x3);
  D  `has_pvconv_plans = False` and `amax_global = True` on one PVConv: equal bits to the default, and the launches really changed.

What stays default-mode only: the reduced-width and full-width WHOLE-NETWORK parity tests (test_gpu_train_parity.py,
test_gpu_parity_as_benched.py) -- a network in fp32 / bf16x3 is run by no test; the glue is pinned here one module at a time.
No shape of the lists below had to be replaced: the call records show each reaches the route it was chosen for."""
import contextlib
import inspect

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from test_gpu_train_parity import (DEV, TOL_LAYER, _grads, _scale, check_pvconv_train_gradients, count_native_calls, is_forward_only)

pytestmark = pytest.mark.gpu

TOL = 1e-5                       # the fp32-class bar of tests/test_gpu_fuzz.py (its `< 1e-5`), per tensor relative to its largest entry
TOL_FWD = 1e-5                   # forward-only quantities: test_gpu_train_parity.FLOOR_FWD; gradients: TOL_LAYER (= its FLOOR_T)
NSPLIT = {'f16x2': 2, 'bf16x3': 3, 'fp32': 0}
DEFAULTS = {'conv_math': 'f16x2', 'pw_math': 'f16x2', 'pw_split_min_macs': 1 << 24, 'pw_wgrad_f16_min_macs': 1 << 32,
            'has_pvconv_plans': True, 'amax_global': False}
MODE_PAIRS = [('fp32', 'fp32'), ('bf16x3', 'bf16x3'), ('fp32', 'f16x2'), ('f16x2', 'fp32'), ('bf16x3', 'f16x2')]

SPLIT = {'conv': ('conv3d_igemm_split', 'conv3d_forward_split', 'conv3d_backward_data_split', 'conv3d_igemm_split_act'),
         'pw': ('pwconv_gemm_split', 'pwconv_forward_split', 'pwconv_backward_data_split', 'pwconv_gemm_split_act')}
FP32 = {'conv': ('conv3d_forward', 'conv3d_backward_data'), 'pw': ('pwconv_forward', 'pwconv_backward_data')}
WGRAD = {'conv': ('conv3d_backward_weight', 'conv3d_backward_weight_f16'), 'pw': ('pwconv_backward_weight', 'pwconv_backward_weight_f16')}


def _live():
    from pvcnn_amd.modules.functional import backend as seam
    from pvcnn_amd.modules.functional._autograd import native
    assert seam._backend is native() and type(seam._backend).__name__ == 'HipBackend'
    return seam._backend


@pytest.fixture()
def modes(monkeypatch):
    """-> set(conv_math=, pw_math=, pw_split_min_macs=, ...): the switches as attributes of the live backend object for one test, the
    memo and the weight bank emptied on entry, at every change and on exit.  Afterwards the instance carries no attribute of its own
    for them: it reads the class's defaults again, and a later test that patches the class still reaches it."""
    from pvcnn_amd.modules.functional import _cache
    be = _live()
    own = {n for n in DEFAULTS if n in vars(be)}

    def flush():
        _cache.clear()
        be.weight_bank_invalidate()

    def set_(**switches):
        assert set(switches) <= set(DEFAULTS), switches
        for name, value in switches.items():
            monkeypatch.setattr(be, name, value)
        flush()
        return be
    flush()
    try:
        yield set_
    finally:
        monkeypatch.undo()                    # (setattr on an instance is undone by a setattr: take that shadow away as well)
        for name in DEFAULTS:
            if name not in own:
                vars(be).pop(name, None)
        flush()


class _Record:
    def __init__(self, counts, nsplits):
        self.counts, self.nsplits = counts, nsplits

    def family(self, kind):
        """-> (split launches, their nsplit arguments sorted, fp32 forward launches, fp32 backward-data launches, fp32-MFMA weight
        gradients, f16x2 weight gradients) of one kind."""
        return (sum(self.counts[n] for n in SPLIT[kind]), sorted(v for n in SPLIT[kind] for v in self.nsplits[n]),
                self.counts[FP32[kind][0]], self.counts[FP32[kind][1]], self.counts[WGRAD[kind][0]], self.counts[WGRAD[kind][1]])

    def line(self, label):
        parts = []
        for kind in ('conv', 'pw'):
            split, ns, fwd, bwd, wg, wg16 = self.family(kind)
            parts.append(f'{kind}: split x{split} nsplit {ns}, fp32 forward x{fwd} backward-data x{bwd}, '
                         f'backward-weight fp32 x{wg} f16x2 x{wg16}')
        print(f'[call record] {label}: ' + '; '.join(parts))


@contextlib.contextmanager
def call_record():
    """count_native_calls over the product methods of both kinds; of the split launches also the `nsplit` argument of every call."""
    be = _live()
    names = [n for group in (SPLIT, FP32, WGRAD) for kind in group for n in group[kind]]
    with count_native_calls(names) as counts:
        nsplits = {n: [] for kind in SPLIT for n in SPLIT[kind]}
        counting = {n: vars(be)[n] for n in nsplits}
        for n, inner in counting.items():
            sig = inspect.signature(getattr(type(be), n))

            def recording(*a, _inner=inner, _n=n, _sig=sig, **kw):
                nsplits[_n].append(int(_sig.bind(be, *a, **kw).arguments['nsplit']))
                return _inner(*a, **kw)
            setattr(be, n, recording)
        try:
            yield _Record(counts, nsplits)
        finally:
            for n, inner in counting.items():
                setattr(be, n, inner)


def _layer(kind, math, b, ci, co, l, split_min=0, wgrad_min=0):
    """One convolution layer whose input wants a gradient -> (kind, nsplit its products must run in, whether the f16x2 backward-weight
    kernel must serve): l = R (Conv3d) or N (1x1); the rules of the module docstring."""
    nsplit = NSPLIT[math]
    if kind == 'pw' and b * ci * co * l < split_min:
        nsplit = 0
    if kind == 'conv':
        f16 = nsplit == 2 and l in (8, 12, 16, 32)
    else:
        f16 = nsplit == 2 and l % 4 == 0 and b * ci * co * l >= wgrad_min
    return kind, nsplit, f16


def _expected(rec, label, layers):
    """Print the call record and hold it against `layers` (_layer): per layer one forward and one backward-data launch of its family
    with its nsplit, and one weight gradient on the kernel named for it."""
    rec.line(label)
    for kind in ('conv', 'pw'):
        mine = [(ns, f16) for k, ns, f16 in layers if k == kind]
        want = (2 * sum(1 for ns, _ in mine if ns), sorted(ns for ns, _ in mine if ns for _ in (0, 1)),
                sum(1 for ns, _ in mine if not ns), sum(1 for ns, _ in mine if not ns),
                sum(1 for _, f16 in mine if not f16), sum(1 for _, f16 in mine if f16))
        assert rec.family(kind) == want, f'{label}: {kind} launches {rec.family(kind)}, expected {want} (split, nsplits, fp32 forward, ' \
                                         f'fp32 backward-data, backward-weight fp32, backward-weight f16x2)'


def _rel(a, b):
    return (a.double() - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


# ---- the fixture itself ---------------------------------------------------------------------------------------------------------------
def test_the_fixture_sets_the_switches_on_the_live_backend(modes):
    from pvcnn_amd.modules.functional.conv3d import conv_nsplit
    from pvcnn_amd.modules.functional.pwconv import pw_nsplit
    be = modes(conv_math='fp32', pw_math='bf16x3', pw_split_min_macs=0, pw_wgrad_f16_min_macs=0)
    assert be is _live() and (be.conv_math, be.pw_math, be.pw_split_min_macs, be.pw_wgrad_f16_min_macs) == ('fp32', 'bf16x3', 0, 0)
    x, w = torch.empty(1, 4, 8, device=DEV), torch.empty(4, 4, device=DEV)
    assert conv_nsplit() == 0 and pw_nsplit(x, w) == 3
    modes(conv_math='bf16x3', pw_math='f16x2', pw_split_min_macs=1 << 24)
    assert conv_nsplit() == 3 and pw_nsplit(x, w) == 0
    modes(pw_split_min_macs=0)
    assert pw_nsplit(x, w) == 2


def test_the_defaults_are_back_after_the_fixture():
    """Runs right behind the test above: the live backend reads the defaults again, from the class (no instance attribute left)."""
    from pvcnn_amd.modules.functional.conv3d import conv_nsplit
    be = _live()
    for name, value in DEFAULTS.items():
        assert getattr(be, name) == value and name not in vars(be), name
    assert conv_nsplit() == 2
    assert not [n for group in (SPLIT, FP32, WGRAD) for kind in group for n in group[kind] if n in vars(be)]     # no wrapper left


# ---- A. the product functions through autograd, vs fp64 ------------------------------------------------------------------------------
# (B, Ci, Co, R): scalar staging where the f16x2 backward-weight kernel does not serve; the Frustum grid with its ragged z rows; R = 8;
# the pipelined kernel's shape in the default mode; R = 32 at Co <= 32
CONV_SHAPES = [(1, 5, 7, 5), (2, 16, 40, 12), (2, 16, 32, 8), (1, 32, 64, 16), (1, 16, 20, 32)]
# (B, Ci, Co, N): all below 2^24 multiply-adds; the last is the persistent kernel's shape in the default mode
PW_SHAPES = [(2, 9, 64, 300), (1, 64, 128, 262), (2, 64, 128, 512), (1, 64, 256, 512)]


def _against_fp64(label, got, want):
    errs = {k: _rel(got[k], want[k]) for k in want}
    print(f'[math modes] {label}: ' + ' '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, f'{label}: beyond {TOL:g} of the fp64 result: {bad}'


@pytest.mark.parametrize('b,ci,co,r', CONV_SHAPES)
@pytest.mark.parametrize('math', ['fp32', 'bf16x3'])
def test_voxel_conv3d_through_autograd_matches_fp64(modes, math, b, ci, co, r):
    from pvcnn_amd.modules.functional.conv3d import conv_nsplit, voxel_conv3d
    modes(conv_math=math)
    torch.manual_seed(1000 * r + ci)
    x = torch.randn(b, ci, r, r, r, device=DEV, requires_grad=True)
    w = (torch.randn(co, ci, 3, 3, 3, device=DEV) * 0.1).requires_grad_()
    bias = torch.randn(co, device=DEV, requires_grad=True)
    gy = torch.randn(b, co, r, r, r, device=DEV)
    with call_record() as rec:
        y = voxel_conv3d(x, w, bias, False, conv_nsplit())           # (as modules/pvconv.py calls it)
        y.backward(gy)
        torch.cuda.synchronize()
    label = f'voxel_conv3d {math} B={b} Ci={ci} Co={co} R={r}'
    _expected(rec, label, [_layer('conv', math, b, ci, co, r)])
    xd, wd, bd = x.detach().double().requires_grad_(), w.detach().double().requires_grad_(), bias.detach().double().requires_grad_()
    yd = F.conv3d(xd, wd, bd, padding=1)
    yd.backward(gy.double())
    _against_fp64(label, {'y': y.detach(), 'x.grad': x.grad, 'w.grad': w.grad, 'bias.grad': bias.grad},
                  {'y': yd.detach(), 'x.grad': xd.grad, 'w.grad': wd.grad, 'bias.grad': bd.grad})


@pytest.mark.parametrize('b,ci,co,n', PW_SHAPES)
@pytest.mark.parametrize('thresholds', ['thresholds_0', 'thresholds_default'])
@pytest.mark.parametrize('math', ['fp32', 'bf16x3', 'f16x2'])
def test_pointwise_conv_through_autograd_matches_fp64(modes, math, thresholds, b, ci, co, n):
    """Thresholds at 0: the split forward / backward-data kernels (and in f16x2 the f16x2 backward-weight kernel, where N % 4 == 0) at
    these small sizes; at their defaults the same products take the fp32 kernels in EVERY mode.  (f16x2 is the default mode: listed
    with the two others because no other test reaches its split 1x1 route through autograd below 2^24 multiply-adds.)"""
    from pvcnn_amd.modules.functional.pwconv import pointwise_conv
    lowered = {'pw_split_min_macs': 0, 'pw_wgrad_f16_min_macs': 0} if thresholds == 'thresholds_0' else {}
    be = modes(pw_math=math, **lowered)
    torch.manual_seed(n + ci)
    x = torch.randn(b, ci, n, device=DEV, requires_grad=True)
    w = (torch.randn(co, ci, 1, device=DEV) * 0.2).requires_grad_()
    bias = torch.randn(co, device=DEV, requires_grad=True)
    gy = torch.randn(b, co, n, device=DEV)
    with call_record() as rec:
        y = pointwise_conv(x, w, bias)
        y.backward(gy)
        torch.cuda.synchronize()
    label = f'pointwise_conv {math} ({thresholds}) B={b} Ci={ci} Co={co} N={n}'
    layer = _layer('pw', math, b, ci, co, n, be.pw_split_min_macs, be.pw_wgrad_f16_min_macs)
    assert lowered or layer == ('pw', 0, False)                      # below the default bar: fp32 kernels whatever the mode
    _expected(rec, label, [layer])
    xd, wd, bd = x.detach().double().requires_grad_(), w.detach().double().requires_grad_(), bias.detach().double().requires_grad_()
    yd = F.conv1d(xd, wd, bd)
    yd.backward(gy.double())
    _against_fp64(label, {'y': y.detach(), 'x.grad': x.grad, 'w.grad': w.grad, 'bias.grad': bias.grad},
                  {'y': yd.detach(), 'x.grad': xd.grad, 'w.grad': wd.grad, 'bias.grad': bd.grad})


# ---- B. one training PVConv in every mode pair, vs the oracle stack and the fp64 truth -----------------------------------------------
# (cin, cout, R, N, se, normalize) at B = 3: the two smallest configurations of test_pvconv_train_gradients_match_the_oracle_stack and
# one grid the f16x2 backward-weight kernel does not serve
PVCONVS = [(16, 32, 8, 777, True, True), (6, 16, 12, 1024, True, False), (9, 16, 5, 300, False, True)]


@pytest.mark.parametrize('cin,cout,r,n,se,normalize', PVCONVS)
@pytest.mark.parametrize('conv_math,pw_math', MODE_PAIRS)
def test_pvconv_train_step_in_every_mode_pair(modes, oracle, conv_math, pw_math, cin, cout, r, n, se, normalize):
    """The mixed pairs are where a producer's amax tag meets a consumer that must ignore it, and the reverse.  Bars: the helper's own
    (TOL_LAYER per tensor against the oracle stack, running statistics included; TOL_LOSS on the loss); its `[train parity]` line
    prints the HIP path's distance from the oracle stack and from the fp64 truth, and the oracle stack's own from the truth."""
    modes(conv_math=conv_math, pw_math=pw_math, pw_split_min_macs=0, pw_wgrad_f16_min_macs=0)
    label = f'PVConv({cin}->{cout}, R={r}, N={n}) [{conv_math}/{pw_math}]'
    with call_record() as rec:
        try:
            check_pvconv_train_gradients(oracle, cin, cout, r, n, se, normalize, mode=f' [{conv_math}/{pw_math}]')
        except BaseException:
            rec.line(label)                   # (a missed bar: the record of what ran goes with it)
            raise
    _expected(rec, label, [_layer('conv', conv_math, 3, cin, cout, r), _layer('conv', conv_math, 3, cout, cout, r),
                           _layer('pw', pw_math, 3, cin, cout, n)])


# ---- C. a point branch and a classifier head in every mode pair, vs the same modules in fp64 on the CPU ------------------------------
def _shared_mlp():
    from pvcnn_amd.modules import SharedMLP
    return SharedMLP(64, [128, 128])


def _head():
    from pvcnn_amd.modules import SharedMLP
    return nn.Sequential(SharedMLP(128, 64), nn.Dropout(0.0), nn.Conv1d(64, 13, 1))


def _classify(head, x):
    from pvcnn_amd import workload
    return workload._classify(head, x)


# name -> (build, how the GPU path runs it, input (B, C, N), the 1x1 layers (Ci, Co) in forward order)
POINT_CASES = {'SharedMLP(64, [128, 128])': (_shared_mlp, lambda net, x: net(x), (2, 64, 1024), [(64, 128), (128, 128)]),
               'head [SharedMLP(128, 64), Dropout(0), Conv1d(64, 13, 1)]': (_head, _classify, (2, 128, 1024), [(128, 64), (64, 13)])}
_POINT_TRUTH = {}


def _point_loss(y, tgt):
    return (y * tgt).mean() + y.square().mean()


def _point_truth(name):
    """-> (state dict, input, loss weights, the fp64 CPU result of _grads): computed once per case, shared by every mode, never changed."""
    if name not in _POINT_TRUTH:
        build, _, shape, _ = POINT_CASES[name]
        torch.manual_seed(23)
        net = build().train()
        for m in net.modules():                                   # (BatchNorm's initial 1 / 0 would hide a swapped gamma / beta)
            if isinstance(m, nn.modules.batchnorm._BatchNorm):
                nn.init.uniform_(m.weight, 0.5, 1.5)
                nn.init.normal_(m.bias, 0.0, 0.2)
        state = {k: v.clone() for k, v in net.state_dict().items()}
        x0 = torch.randn(shape)
        tgt = torch.randn(shape[0], POINT_CASES[name][3][-1][1], shape[2])
        net = net.double()
        x = x0.double().requires_grad_()
        y = net(x)                                                # the plain modules: nn.Sequential.forward on CPU tensors
        _point_loss(y, tgt.double()).backward()
        _POINT_TRUTH[name] = (state, x0, tgt, _grads(net, x, y))
    return _POINT_TRUTH[name]


def _point_net(name):
    net = POINT_CASES[name][0]()
    net.load_state_dict(_point_truth(name)[0])
    return net.to(DEV).train()


def _point_run(name, net=None):
    run = POINT_CASES[name][1]
    _, x0, tgt, _ = _point_truth(name)
    net = net if net is not None else _point_net(name)
    x = x0.to(DEV).requires_grad_()
    y = run(net, x)
    _point_loss(y, tgt.to(DEV)).backward()
    torch.cuda.synchronize()
    return _grads(net, x, y)


def _point_layers(name, pw_math, be):
    b, _, n = POINT_CASES[name][2]
    return [_layer('pw', pw_math, b, ci, co, n, be.pw_split_min_macs, be.pw_wgrad_f16_min_macs) for ci, co in POINT_CASES[name][3]]


def _point_check(label, got, truth):
    assert got.keys() == truth.keys()
    rows = [(k, (got[k] - truth[k]).abs().max().item() / _scale(truth, k), TOL_FWD if is_forward_only(k) else TOL_LAYER) for k in truth]
    fwd = max((r for r in rows if r[2] == TOL_FWD), key=lambda r: r[1])
    grad = max((r for r in rows if r[2] == TOL_LAYER), key=lambda r: r[1])
    print(f'[math modes] {label}: {len(rows)} tensors vs fp64; worst forward-only {fwd[1]:.2e} ({fwd[0]}), worst gradient {grad[1]:.2e} ({grad[0]})')
    bad = [(k, e, bar) for k, e, bar in rows if not e <= bar]
    assert not bad, f'{label}: {bad[:6]}'


@pytest.mark.parametrize('name', list(POINT_CASES), ids=['shared_mlp', 'head'])
@pytest.mark.parametrize('thresholds', ['thresholds_0', 'thresholds_default'])
@pytest.mark.parametrize('conv_math,pw_math', MODE_PAIRS)
def test_point_modules_in_every_mode_pair(modes, conv_math, pw_math, thresholds, name):
    """Outputs, running statistics (1e-5), input gradient and every parameter gradient (TOL_LAYER) of the GPU path in train mode at
    dropout p = 0 against the same modules in fp64 on the CPU with the state dict copied.  At the default thresholds the three wide
    layers (2^24 and 2^25 multiply-adds) still take the split forward / backward-data kernels, the 64 -> 13 convolution does not, and
    no weight gradient takes the f16x2 kernel."""
    lowered = {'pw_split_min_macs': 0, 'pw_wgrad_f16_min_macs': 0} if thresholds == 'thresholds_0' else {}
    be = modes(conv_math=conv_math, pw_math=pw_math, **lowered)
    truth = _point_truth(name)[3]
    with call_record() as rec:
        got = _point_run(name)
    label = f'{name} [{conv_math}/{pw_math}, {thresholds}]'
    _expected(rec, label, _point_layers(name, pw_math, be))
    _point_check(label, got, truth)


@pytest.mark.parametrize('name', list(POINT_CASES), ids=['shared_mlp', 'head'])
def test_point_modules_in_f16x2_repeat_their_bits(modes, name):
    """The default arithmetic with both thresholds at 0 (split products and the f16x2 backward-weight kernel at these sizes): two runs
    from the same state give equal bits, and meet the bars of the test above."""
    be = modes(pw_split_min_macs=0, pw_wgrad_f16_min_macs=0)
    with call_record() as rec:
        first = _point_run(name)
    label = f'{name} [f16x2/f16x2, thresholds 0]'
    _expected(rec, label, _point_layers(name, 'f16x2', be))
    second = _point_run(name)
    differ = [k for k in first if not torch.equal(first[k], second[k])]
    assert not differ, f'{label}: not the same bits in a second run: {differ}'
    _point_check(label, first, _point_truth(name)[3])


@contextlib.contextmanager
def _launch_labels():
    """-> list of the labels of every native launch inside (backend._run)."""
    from pvcnn_amd.modules.functional import backend as seam
    seen, run = [], seam._run

    def spy(fn, label, ref, *args):
        seen.append(label)
        return run(fn, label, ref, *args)
    seam._run = spy
    try:
        yield seen
    finally:
        seam._run = run


def test_an_armed_weight_bank_serves_f16x2_pairs_and_no_other_mode(modes):
    """The weight bank's image pairs are keyed by nsplit (HipBackend._weight_images takes them for nsplit 2, and 1 under autocast).  One
    registered SharedMLP, thresholds at 0, every run from the same state: a first f16x2 step splits its own weights; after a refresh
    the pairs come from the bank's batched launch -- same bits; with the pairs armed and `pw_math` switched to bf16x3 the products run
    with nsplit 3 on images of their own and meet the bars against fp64; back in f16x2 the bank serves again, same bits as the first."""
    name = 'SharedMLP(64, [128, 128])'
    be = modes(pw_split_min_macs=0, pw_wgrad_f16_min_macs=0)
    net = _point_net(name)
    be.weight_bank_register(net)

    def step(refresh):
        net.load_state_dict(_point_truth(name)[0])            # (in place: the parameters keep their addresses, the bank's keys)
        net.zero_grad(set_to_none=True)
        with _launch_labels() as labels, call_record() as rec:
            if refresh:
                be.weight_bank_refresh()
            return _point_run(name, net), labels, rec
    first, labels, rec = step(refresh=False)
    _expected(rec, f'{name} [f16x2, bank not armed]', _point_layers(name, 'f16x2', be))
    assert labels.count('pwconv_weight_split_pair') == 2 and 'weight_split_pair_batch' not in labels, labels
    banked, labels, rec = step(refresh=True)
    _expected(rec, f'{name} [f16x2, bank armed]', _point_layers(name, 'f16x2', be))
    assert 'weight_split_pair_batch' in labels and 'pwconv_weight_split_pair' not in labels, labels
    assert not [k for k in first if not torch.equal(first[k], banked[k])]
    modes(pw_math='bf16x3')
    other, labels, rec = step(refresh=True)                   # (the f16x2 pairs are armed again: nobody may take them)
    _expected(rec, f'{name} [bf16x3, f16x2 pairs armed]', _point_layers(name, 'bf16x3', be))
    assert labels.count('pwconv_weight_split') == 4 and 'pwconv_weight_split_pair' not in labels, labels
    _point_check(f'{name} [bf16x3, f16x2 pairs armed]', other, _point_truth(name)[3])
    modes(pw_math='f16x2')
    again, labels, rec = step(refresh=True)
    _expected(rec, f'{name} [f16x2 again, bank armed]', _point_layers(name, 'f16x2', be))
    assert 'pwconv_weight_split_pair' not in labels and 'pwconv_weight_split' not in labels, labels
    assert not [k for k in first if not torch.equal(first[k], again[k])]


# ---- D. python-level switches on one PVConv: equal bits to the default ----------------------------------------------------------------
@contextlib.contextmanager
def _absmax_launches():
    """-> list, one entry per pvcnn_absmax_tiles launch: True when it was asked for word [0] (a ticket), False when table-only.
    `amax_global` acts inside HipBackend.absmax_tiles (`want_global or self.amax_global`): the callers' own argument stays False, so
    the launch's last argument is where the switch shows."""
    from pvcnn_amd.modules.functional import backend as seam
    be, seen, run = _live(), [], seam._run

    def spy(fn, label, ref, *args):
        if label == 'absmax_tiles':
            seen.append(args[-1] is not be._TABLE_ONLY)
        return run(fn, label, ref, *args)
    seam._run = spy
    try:
        yield seen
    finally:
        seam._run = run


def _pvconv_state():
    from pvcnn_amd.modules import PVConv
    from pvcnn_amd import workload
    torch.manual_seed(31)
    state = {k: v.clone() for k, v in PVConv(16, 32, 3, 8, with_se=True, normalize=True).state_dict().items()}
    x0, _ = workload.make_s3dis_batch(3, 777)
    return state, torch.cat([x0, torch.randn(3, 7, 777)], dim=1), torch.randn(3, 32, 777)


def _pvconv_run(state, x0, wgt):
    from pvcnn_amd.modules import PVConv
    net = PVConv(16, 32, 3, 8, with_se=True, normalize=True)
    net.load_state_dict(state)
    net = net.to(DEV).train()
    x = x0.clone().to(DEV).requires_grad_()
    out = net((x, x[:, :3, :]))
    ((out[0] * wgt.to(DEV)).mean() + out[0].square().mean()).backward()
    torch.cuda.synchronize()
    return _grads(net, x, out)


PLAN_CALLS = ['pvconv_plans', 'avg_voxelize_plan', 'trilinear_devoxelize_backward_plan', 'absmax_tiles', 'conv_amax']


@pytest.mark.parametrize('switch,value', [('has_pvconv_plans', False), ('amax_global', True)])
def test_pvconv_under_a_python_level_switch_has_the_bits_of_the_default(modes, switch, value):
    """PVConv(16 -> 32, R = 8, N = 777, SE) forward and backward, once with the defaults and once with the switch set on the live
    backend, same state dict and inputs, memo and weight bank emptied around each run: torch.equal on the outputs, the input
    gradient, every parameter gradient and every buffer.
      has_pvconv_plans = False: the two plans of the geometry come from their own launch chains -- the same plans
        (HipBackend.pvconv_plans builds "what avg_voxelize_plan and trilinear_devoxelize_backward_plan build"), so the scatters sum in
        the same order;
      amax_global = True: every absmax_tiles launch also writes word [0].  No consumer of a buffer WITH a table reads that word
        (csrc/wave.h: with a segment length > 0 the maximum is taken over the table; HipBackend._amax_for passes the segment length for
        every buffer of 1 + tiles words), so no tensor rounds differently and none is held to a looser bar."""
    state, x0, wgt = _pvconv_state()
    results, launches = {}, {}
    for variant in ('default', switch):
        modes(**({switch: value} if variant == switch else {}))
        with count_native_calls(PLAN_CALLS) as calls, _absmax_launches() as absmax:
            results[variant] = _pvconv_run(state, x0, wgt)
        launches[variant] = (dict(calls), list(absmax))
        print(f'[call record] PVConv(16->32, R=8, N=777) [{variant}]: {dict(calls)}, absmax_tiles launches with word [0]: {list(absmax)}')
    (calls_d, absmax_d), (calls_s, absmax_s) = launches['default'], launches[switch]
    assert calls_d['pvconv_plans'] == 1 and calls_d['avg_voxelize_plan'] == 0 and calls_d['trilinear_devoxelize_backward_plan'] == 0, calls_d
    assert absmax_d and not any(absmax_d) and len(absmax_d) == calls_d['absmax_tiles'] and calls_d['conv_amax'] >= 1, (calls_d, absmax_d)
    if switch == 'has_pvconv_plans':
        assert calls_s['pvconv_plans'] == 0 and calls_s['avg_voxelize_plan'] == 1 and calls_s['trilinear_devoxelize_backward_plan'] == 1, calls_s
        assert absmax_s == absmax_d
    else:
        assert calls_s['pvconv_plans'] == 1 and len(absmax_s) == len(absmax_d) and all(absmax_s), (calls_s, absmax_s)
    assert results['default'].keys() == results[switch].keys()
    differ = [k for k in results['default'] if not torch.equal(results['default'][k], results[switch][k])]
    assert not differ, f'{switch} = {value}: other bits than the default in {differ}'
