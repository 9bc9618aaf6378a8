"""Folded inference, host side (no GPU): the fold arithmetic, the public pair fold_batchnorm / unfold_batchnorm, the rule that a
snapshot is never stale, and the C ABI of the activation-tail entry points.

`folded_parameters(conv, bn)` is checked against an fp64 evaluation of act(bn(conv(x))) on torch CPU.  The folded weights are the fp64
fold rounded once to fp32, so evaluated in fp64 they differ from the truth by that rounding alone: 2^-24 relative per weight, summed
over at most Ci * 27 = 108 products of magnitude |w' x| -- about 1e-7 * (1 + |truth|) at these sizes.  The bar is
1e-6 * (1 + |truth|)."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

import pvcnn_amd
from conftest import ROOT
from pvcnn_amd.modules import PVConv, SharedMLP
from pvcnn_amd.modules.functional import _fold
from pvcnn_amd.modules.functional.bnact import folded_parameters, folded_snapshot

ACT_ENTRIES = ('pvcnn_conv3d_fwd_split_act', 'pvcnn_conv3d_fwd_act', 'pvcnn_pwconv_fwd_split_act', 'pvcnn_pwconv_fwd_act')


def nontrivial_bn_(bn, g):
    """Running variance in [0.25, 4], non-zero running means, gamma with negative entries and one exact zero."""
    c = bn.num_features
    with torch.no_grad():
        bn.running_var.copy_(0.25 + 3.75 * torch.rand(c, generator=g))
        bn.running_mean.copy_(torch.randn(c, generator=g) + 0.5)
        if bn.weight is not None:
            gamma = torch.randn(c, generator=g)
            gamma[0], gamma[1], gamma[2] = -abs(gamma[0]) - 0.1, 0.0, abs(gamma[2]) + 0.1
            bn.weight.copy_(gamma)
            bn.bias.copy_(torch.randn(c, generator=g))
    return bn


CASES = [
    ('conv1d', lambda bias: nn.Conv1d(9, 8, 1, bias=bias), nn.BatchNorm1d, (3, 9, 40)),
    ('conv2d', lambda bias: nn.Conv2d(7, 8, 1, bias=bias), nn.BatchNorm2d, (2, 7, 10, 4)),
    ('conv3d', lambda bias: nn.Conv3d(4, 8, 3, padding=1, bias=bias), nn.BatchNorm3d, (2, 4, 6, 6, 6)),
]


@pytest.mark.parametrize('name,make_conv,norm,shape', CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize('bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('eps', [1e-4, 1e-5])
@pytest.mark.parametrize('affine', [True, False], ids=['affine', 'plain'])
def test_folded_parameters_reproduce_the_three_modules_in_fp64(name, make_conv, norm, shape, bias, eps, affine):
    g = torch.Generator().manual_seed(20 + len(name) + int(bias) + int(affine))
    conv = make_conv(bias)
    bn = nontrivial_bn_(norm(8, eps=eps, affine=affine), g).eval()
    x = torch.randn(*shape, generator=g, dtype=torch.float64)
    w, b = folded_parameters(conv, bn)
    assert w.dtype == b.dtype == torch.float32 and w.shape == conv.weight.shape and b.shape == (8,)
    convolve = {1: nn.functional.conv1d, 2: nn.functional.conv2d, 3: nn.functional.conv3d}[len(shape) - 2]
    pad = conv.padding
    for slope in (0.0, 0.1):
        with torch.no_grad():
            truth = nn.functional.leaky_relu(bn.double()(conv.double()(x)), slope)
            got = nn.functional.leaky_relu(convolve(x, w.double(), b.double(), padding=pad), slope)
        conv.float(), bn.float()
        err = ((got - truth).abs() / (1 + truth.abs())).max().item()
        print(f'{name} bias={bias} eps={eps} affine={affine} slope={slope}: {err:.2e}')
        assert err <= 1e-6, err


def _model():
    torch.manual_seed(3)
    m = nn.Sequential(SharedMLP(9, [16, 16]), SharedMLP(16, 8, dim=1))
    layer = PVConv(9, 16, kernel_size=3, resolution=4)
    g = torch.Generator().manual_seed(4)
    for mod in list(m.modules()) + list(layer.modules()):
        if isinstance(mod, nn.modules.batchnorm._BatchNorm):
            nontrivial_bn_(mod, g)
    return m, layer


def test_fold_keeps_the_state_dict_and_unfold_leaves_nothing_behind():
    for model in _model():
        model.train()
        before = {k: v.clone() for k, v in model.state_dict().items()}
        names = [n for n, _ in model.named_parameters()], [n for n, _ in model.named_buffers()]
        assert pvcnn_amd.fold_batchnorm(model) is model and not model.training
        folded = [m for m in model.modules() if hasattr(m, _fold.ATTR)]
        assert folded and all(isinstance(m, (nn.Conv1d, nn.Conv3d)) for m in folded)
        after = model.state_dict()
        assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
        assert names == ([n for n, _ in model.named_parameters()], [n for n, _ in model.named_buffers()])
        assert pvcnn_amd.unfold_batchnorm(model) is model
        assert not any(_fold.ATTR in m.__dict__ for m in model.modules())


def test_every_change_invalidates_the_snapshot():
    from pvcnn_amd.modules.functional._autograd import native
    mlp = SharedMLP(9, 16)
    conv, bn, act = mlp.layers
    nontrivial_bn_(bn, torch.Generator().manual_seed(5))

    def ready():
        with torch.no_grad():
            return folded_snapshot(conv, bn, act) is not None

    assert not ready()                                          # never folded
    pvcnn_amd.fold_batchnorm(mlp)
    assert ready() and ready()
    # an in-place change to any of the six tensors: the snapshot is dropped, not only refused
    for tensor in (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var):
        pvcnn_amd.fold_batchnorm(mlp)
        assert ready()
        with torch.no_grad():
            tensor.mul_(2)
        assert not ready() and not hasattr(conv, _fold.ATTR)
    # parameters written behind torch's back (FlatAdam) announce themselves through the weight bank's epoch
    pvcnn_amd.fold_batchnorm(mlp)
    assert ready()
    native().weight_bank_invalidate()
    assert not ready() and not hasattr(conv, _fold.ATTR)
    # a re-seated tensor (load_state_dict copies in place: caught by the version; `.data =` by the address)
    pvcnn_amd.fold_batchnorm(mlp)
    conv.weight.data = conv.weight.data.clone()
    assert not ready()
    # training mode and enabled gradients switch the fold off without dropping it
    pvcnn_amd.fold_batchnorm(mlp)
    mlp.train()
    assert not ready()
    mlp.eval()
    assert ready()
    assert folded_snapshot(conv, bn, act) is None               # gradients enabled here
    assert ready()
    with torch.inference_mode():
        assert folded_snapshot(conv, bn, act) is not None
    # not a triple: no activation behind the BatchNorm
    with torch.no_grad():
        assert folded_snapshot(conv, bn, nn.Identity()) is None and folded_snapshot(conv, nn.Identity(), act) is None


def test_folded_and_unfolded_modules_agree_on_the_cpu():
    """On CPU tensors run_layers never takes the folded product: a folded model computes exactly what the modules compute."""
    m, _ = _model()
    x = torch.randn(2, 9, 32, generator=torch.Generator().manual_seed(6))
    m.eval()
    with torch.no_grad():
        want = m(x)
        got = pvcnn_amd.fold_batchnorm(m)(x)
    assert torch.equal(got, want)


def test_header_exports_and_binding_agree_on_the_activation_tail_entry_points():
    from pvcnn_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pvcnn_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'PVCNN_API\s+[\w\s\*]+?\b(pvcnn_\w+)\s*\(', text))
    assert re.search(r'#define\s+PVCNN_ABI_VERSION\s+17\b', text) and _lib.ABI_VERSION == 17
    assert os.path.exists(_lib.LIB_PATH), 'libpvcnn_hip.so not built (run __graft_entry__.build())'
    exported = ctypes.CDLL(_lib.LIB_PATH)
    for name in ACT_ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(exported, name), name
        plain = name[:-len('_act')]
        res, args = _lib.SIGNATURES[name]
        pres, pargs = _lib.SIGNATURES[plain]
        # the namesake's arguments, then slope, y's amax buffer and its segment length in front of the stream
        assert res is pres and args == pargs[:-1] + [ctypes.c_float, ctypes.c_void_p, ctypes.c_int] + pargs[-1:], name
        # ... and the same in the header's parameter lists
        params = lambda n: [p.strip() for p in re.search(r'\b' + n + r'\s*\(([^;]*?)\)\s*;', text, flags=re.S).group(1).split(',')]
        tail = params(name)[len(params(plain)) - 1:]
        assert params(name)[:len(params(plain)) - 1] == params(plain)[:-1], name
        assert [re.sub(r'\s+', ' ', t) for t in tail] == ['float slope', 'void *y_amax', 'int y_amax_seg', 'void *stream'], (name, tail)
    assert _lib.load().pvcnn_version() == 17
    # the shape checks shared with the plain entry points answer with an error, not a launch (nothing here touches a device)
    lib = _lib.load()
    null, f = ctypes.c_void_p(None), ctypes.c_float(0.0)
    assert lib.pvcnn_conv3d_fwd_split_act(null, null, null, 1, 0, 4, 8, 2, null, 0, null, null, f, null, 8, null) != 0
    assert lib.pvcnn_pwconv_fwd_split_act(null, null, null, 1, 4, 4, 8, 5, null, 0, null, null, f, null, 256, null) != 0
    assert lib.pvcnn_conv3d_fwd_act(null, null, null, 1, 4, 0, 8, null, f, null, 8, null) != 0
    assert lib.pvcnn_pwconv_fwd_act(null, null, 4, null, 1, 0, 4, 8, null, f, null, 256, null) != 0
    one = ctypes.c_void_p(16)
    assert lib.pvcnn_conv3d_fwd_split_act(null, null, null, 1, 4, 4, 8, 2, one, 0, null, null, f, one, 7, null) != 0     # y_amax_seg != R
    assert lib.pvcnn_pwconv_fwd_split_act(null, null, null, 1, 4, 4, 8, 2, one, 0, null, null, f, one, 128, null) != 0   # y_amax_seg != 256
    assert b'y_amax_seg' in lib.pvcnn_last_error_string()
