"""Host side of "the point branch's BatchNorm + ReLU in the devoxelize gather" (modules/pvconv.py, functional/bnact.py), on the CPU:

  * the predicate that selects the new path says no to everything it does not serve -- eval mode, a hooked module, a folded snapshot,
    autocast, squeeze-and-excitation, a tensor that is not fp32 on the GPU, a backend without the capability flag;
  * on a backend WITHOUT the flag (the recording stand-ins of the pinned host tests, the CPU oracle) a PVConv forward + backward asks
    the backend for exactly what it asks with the flag set on a backend that cannot serve it: the call sequence does not depend on
    the new code, and no call carries the new keyword."""
import types

import pytest
import torch
import torch.nn as nn

from pvcnn_amd.modules import PVConv
from pvcnn_amd.modules.functional import _fold, bnact
from pvcnn_amd.modules.functional import backend as seam


class _Capable:
    """What the predicate asks of a backend."""
    has_point_branch_fused = has_pwconv = has_bnact = True


def _gpu_like(dtype=torch.float32, dim=3, numel=2 * 8 * 16):
    """A stand-in for point features on the GPU: the predicate only looks at these attributes."""
    return types.SimpleNamespace(is_cuda=True, dtype=dtype, dim=lambda: dim, numel=lambda: numel)


@pytest.fixture()
def capable(monkeypatch):
    monkeypatch.setattr(seam, '_backend', _Capable())


def _layer(**kw):
    return PVConv(8, 16, 3, resolution=4, **kw).train()


def test_the_predicate_accepts_the_plain_training_case(capable):
    layer = _layer()
    conv, bn, slope = bnact.point_bn_fusable(layer.point_features.layers, _gpu_like(), True)
    assert conv is layer.point_features.layers[0] and bn is layer.point_features.layers[1] and slope == 0.0
    assert layer._point_branch_in_gather(_gpu_like(), layer.voxel_layers[4], None) == (bn, 0.0)
    layer.point_features.layers[2] = nn.LeakyReLU(0.2)
    assert bnact.point_bn_fusable(layer.point_features.layers, _gpu_like(), True)[2] == pytest.approx(0.2)


def test_the_predicate_refuses_what_the_path_does_not_serve(capable, monkeypatch):
    x = _gpu_like()
    ok = lambda layer, feats=x: layer._point_branch_in_gather(feats, layer.voxel_layers[4], None)
    assert ok(_layer()) is not None
    # eval mode: of the layer, of the point branch's BatchNorm alone, of the grid's BatchNorm alone
    assert ok(_layer().eval()) is None
    layer = _layer(); layer.point_features.layers[1].eval()
    assert ok(layer) is None
    layer = _layer(); layer.voxel_layers[4].eval()
    assert ok(layer) is None
    # hooks: on a module of the stack, on the Sequential, on the SharedMLP
    for pick in (lambda l: l.point_features.layers[0], lambda l: l.point_features.layers[1], lambda l: l.point_features.layers,
                 lambda l: l.point_features):
        layer = _layer()
        pick(layer).register_forward_hook(lambda m, i, o: None)
        assert ok(layer) is None
    layer = _layer(); layer.point_features.layers[0].register_forward_pre_hook(lambda m, i: None)
    assert ok(layer) is None
    # a folded snapshot on the convolution
    layer = _layer(); setattr(layer.point_features.layers[0], _fold.ATTR, object())
    assert ok(layer) is None
    # squeeze-and-excitation keeps the separate pass
    layer = _layer(with_se=True)
    assert layer._point_branch_in_gather(x, layer.voxel_layers[4], layer.voxel_layers[6]) is None
    # another stack than [1x1 conv, BatchNorm1d, ReLU | LeakyReLU]
    layer = _layer(); layer.point_features.layers.append(nn.Dropout(0.1))
    assert ok(layer) is None
    layer = _layer(); layer.point_features.layers[2] = nn.Tanh()
    assert ok(layer) is None
    layer = _layer(); layer.point_features.layers[0] = nn.Conv1d(8, 16, 3, padding=1)
    assert ok(layer) is None
    layer = _layer(); layer.point_features = nn.Identity()
    assert ok(layer) is None
    # tensors: not fp32, not on the GPU, not (B, C, N), empty
    for feats in (_gpu_like(dtype=torch.bfloat16), _gpu_like(dtype=torch.float64), _gpu_like(dim=4), _gpu_like(numel=0), torch.zeros(2, 8, 16)):
        assert ok(_layer(), feats) is None
    # autocast, gradients disabled
    with monkeypatch.context() as m:             # (torch.autocast('cuda') switches itself off on a host without a GPU)
        m.setattr(torch, 'is_autocast_enabled', lambda *a: True)
        assert ok(_layer()) is None
    assert ok(_layer()) is not None
    with torch.no_grad():
        assert ok(_layer()) is None
    # the capability flag: absent, or switched off
    monkeypatch.setattr(seam, '_backend', types.SimpleNamespace(has_pwconv=True, has_bnact=True))
    assert ok(_layer()) is None
    monkeypatch.setattr(seam, '_backend', types.SimpleNamespace(has_pwconv=True, has_bnact=True, has_point_branch_fused=False))
    assert ok(_layer()) is None


def test_the_flag_is_read_from_the_environment_once():
    import inspect
    src = inspect.getsource(seam.HipBackend)
    assert "has_point_branch_fused = os.environ.get('PVCNN_POINT_FUSED', '1') != '0'" in src
    assert isinstance(seam.HipBackend.has_point_branch_fused, bool)


class _Recording:
    """The CPU oracle behind a log of (method, keyword names): what a PVConv asks of its backend."""

    def __init__(self, inner, **flags):
        self._inner, self.log = inner, []
        for k, v in flags.items():
            setattr(self, k, v)

    def __getattr__(self, name):
        target = getattr(self._inner, name)
        if not callable(target):
            return target

        def call(*a, **kw):
            self.log.append((name, tuple(sorted(kw))))
            return target(*a, **kw)
        return call


def _fwd_bwd(backend, monkeypatch, **layer_kw):
    monkeypatch.setattr(seam, '_backend', backend)
    torch.manual_seed(5)
    layer = PVConv(8, 16, 3, resolution=4, **layer_kw).train()
    g = torch.Generator().manual_seed(6)
    feats = torch.randn(2, 8, 32, generator=g).requires_grad_()
    coords = torch.rand(2, 3, 32, generator=g)
    y, _ = layer((feats, coords))
    y.square().sum().backward()
    grads = [p.grad.clone() for p in layer.parameters()]
    return backend.log, y.detach(), feats.grad.clone(), grads


@pytest.mark.parametrize('with_se', [False, True])
def test_a_backend_without_the_flag_is_asked_for_what_it_was(oracle, monkeypatch, with_se):
    absent = _fwd_bwd(_Recording(oracle), monkeypatch, with_se=with_se)
    set_ = _fwd_bwd(_Recording(oracle, has_point_branch_fused=True), monkeypatch, with_se=with_se)
    assert absent[0] and absent[0] == set_[0]
    assert not any('addend_bn' in kws for _, kws in absent[0])
    assert [name for name, _ in absent[0]][:2] == ['avg_voxelize_forward', 'trilinear_devoxelize_forward']
    assert torch.equal(absent[1], set_[1]) and torch.equal(absent[2], set_[2])
    for a, b in zip(absent[3], set_[3]):
        assert torch.equal(a, b)
