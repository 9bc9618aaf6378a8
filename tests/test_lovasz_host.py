"""PF.lovasz_softmax / modules.LovaszSoftmax / modules.CrossEntropyLovasz away from the GPU: the numpy truth checks itself, the
torch composition (what every call the kernels do not serve runs) follows the truth, the predicate says what is fused, the modules
are the functional calls, and the C entry points refuse bad values."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, SEED

import lovasz_truth as T
import pvcnn_amd.modules as M
import pvcnn_amd.modules.functional as PF
from pvcnn_amd.modules.functional import loss as L


# ---- the truth against itself

def test_truth_hand_case():
    """Sorted errors 0.9 (fg), 0.6 (bg), 0.2 (fg), G = 2: steps 1/2, 1/6, 1/3, loss 0.9/2 + 0.6/6 + 0.2/3."""
    st = T.steps([True, False, True])
    assert np.allclose(st, [1 / 2, 1 / 6, 1 / 3], rtol=1e-15, atol=0)
    loss, grad = T.list_loss(np.array([0.2, 0.9, 0.6]), [True, True, False])          # (given out of order)
    assert abs(loss - (0.9 / 2 + 0.6 / 6 + 0.2 / 3)) < 1e-15 and abs(loss - 0.616667) < 1e-6
    assert np.allclose(grad, [1 / 3, 1 / 2, 1 / 6], rtol=1e-15, atol=0)


def test_truth_closed_form_steps_are_the_jaccard_differences():
    rng = np.random.default_rng(SEED)
    lists = [np.zeros(7, bool), np.ones(7, bool), np.array([True]), np.array([False]), rng.random(300) < 0.3, rng.random(4096) < 0.01]
    for fg in lists:
        st = T.steps(fg)
        assert np.abs(st - T.jaccard_differences(fg)).max() <= 1e-15
        assert (st >= 0).all() and abs(st.sum() - 1.0) <= 1e-13                      # (non-negative, summing to 1: 1-Lipschitz in e)
    assert T.steps(np.zeros(5, bool)).tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]           # G = 0
    assert np.allclose(T.steps(np.ones(4, bool)), [1 / 4] * 4)                         # G = n: U stays G


def test_truth_loss_does_not_depend_on_the_order_of_exact_ties():
    rng = np.random.default_rng(SEED + 1)
    e = rng.integers(0, 4, 200).astype(np.float32) / 4                                 # four distinct values: ties everywhere
    fg = rng.random(200) < 0.4
    want, _ = T.list_loss(e, fg)
    for _ in range(5):
        # permuting the points moves tied elements of DIFFERENT kind past each other in the index tie rule
        perm = rng.permutation(200)
        got, _ = T.list_loss(e[perm], fg[perm])
        assert abs(got - want) <= 1e-13 * want


# ---- the composition against the truth

def _targets(g, b, c, s, absent_half=True, ignored=0.1):
    present = torch.arange(c)[::2] if absent_half and c > 1 else torch.arange(c)
    t = present[torch.randint(0, len(present), (b, s), generator=g)]
    return torch.where(torch.rand(b, s, generator=g) < ignored, torch.full_like(t, -100), t)


@functools.lru_cache(maxsize=None)
def _case(name):
    g = torch.Generator().manual_seed(SEED + len(name))
    if name == '2x13x4096':
        x, t = 3.0 * torch.randn(2, 13, 4096, generator=g), _targets(g, 2, 13, 4096)
    elif name == '3x5x300-saturated':                                                  # thousands of exact ties; cloud 1 all ignored
        x, t = 180.0 * torch.randn(3, 5, 300, generator=g), _targets(g, 3, 5, 300)
        t[1] = -100
    elif name == '2x4x1':
        x, t = 3.0 * torch.randn(2, 4, 1, generator=g), torch.tensor([[2], [0]])
    else:
        x, t = 3.0 * torch.randn(1, 50, 2048, generator=g), _targets(g, 1, 50, 2048)
    return x, t


@pytest.mark.parametrize('classes', ['present', 'all'])
@pytest.mark.parametrize('name', ['2x13x4096', '3x5x300-saturated', '2x4x1', '1x50x2048'])
def test_composition_follows_the_truth(name, classes):
    x, t = _case(name)
    assert not PF.lovasz_softmax_is_fused(x, t)
    loss, p, grad_p = PF.lovasz_softmax_parts(x, t, classes=classes)
    assert loss.dtype == torch.float64 and p.dtype == torch.float32 and torch.equal(p, torch.softmax(x, 1))
    want, want_grad, _ = T.lovasz_softmax(p.numpy(), t.numpy(), classes)               # ranked on the SAME fp32 probabilities
    if name == '3x5x300-saturated':
        e = np.where(t.numpy()[0][None] == np.arange(5)[:, None], 1 - p.numpy()[0], p.numpy()[0])
        assert e.size - np.unique(e).size > 1000                                      # the case is what it says
    err_g = np.abs(grad_p.numpy() - want_grad).max() / np.abs(want_grad).max()
    print(f'{name} {classes}: loss {loss.item():.17g} truth {want:.17g}; grad err / max {err_g:.3e}')
    assert abs(loss.item() - want) <= 1e-12 * abs(want)
    assert err_g <= 1e-6
    assert (grad_p.numpy()[want_grad == 0] == 0).all()
    # the public call: the same value rounded to fp32 once, and autograd's gradient for the logits is the fp64 chain's
    xg = x.clone().requires_grad_()
    out = PF.lovasz_softmax(xg, t, classes=classes)
    assert out.dtype == torch.float32 and out.item() == np.float32(loss.item())
    out.backward()
    chain = T.logits_gradient(p.numpy(), want_grad)
    assert np.abs(xg.grad.numpy() - chain).max() <= 1e-5 * np.abs(chain).max()


def test_composition_whole_batch_as_one_list_and_probabilities():
    x, t = _case('3x5x300-saturated')
    x = x / 60.0
    loss, p, grad_p = PF.lovasz_softmax_parts(x, t, per_cloud=False)
    assert p.shape == (1, 5, 900)
    want, want_grad, _ = T.lovasz_softmax(p.numpy(), t.reshape(1, -1).numpy())
    assert abs(loss.item() - want) <= 1e-12 * abs(want)
    assert np.abs(grad_p.numpy() - want_grad).max() <= 1e-6 * np.abs(want_grad).max()
    probs = torch.softmax(x, 1)
    a, b = PF.lovasz_softmax(probs, t, probas=True), PF.lovasz_softmax(x, t)
    assert torch.equal(a, b)
    # out-of-range targets behave as ignored ones
    t_bad, t_clean = t.clone(), t.clone()
    t_bad[0, :4], t_clean[0, :4] = torch.tensor([5, -1, 2 ** 40, 77]), -100
    assert torch.equal(PF.lovasz_softmax(x, t_bad), PF.lovasz_softmax(x, t_clean))
    assert PF.lovasz_softmax(x, torch.full_like(t, -100)).item() == 0.0


def test_gradcheck_on_a_tie_free_input():
    x = torch.tensor([[[0.3, -1.1, 0.7, 2.0, -0.4, 1.3], [1.9, 0.2, -0.8, 0.5, 1.1, -1.6], [-0.6, 0.9, 1.5, -1.2, 0.1, 0.4]]],
                     dtype=torch.float64, requires_grad=True)
    t = torch.tensor([[0, 2, 1, 0, -100, 2]])
    for classes in ('present', 'all'):
        assert torch.autograd.gradcheck(lambda v: PF.lovasz_softmax(v, t, classes=classes), (x,), eps=1e-7, atol=1e-6)


def test_bad_arguments_raise():
    x, t = _case('2x4x1')
    with pytest.raises(ValueError, match='classes'):
        PF.lovasz_softmax(x, t, classes='some')
    with pytest.raises(ValueError, match='expected'):
        PF.lovasz_softmax(x, t[:, :0])
    with pytest.raises(ValueError, match='classes'):
        M.LovaszSoftmax(classes=[1, 2])


# ---- dispatch

class _OnDevice:
    """Stands in for a tensor's `is_cuda` / `device` so that the predicate's other clauses can be asked without a GPU."""

    def __init__(self, t, device='cuda:0'):
        self._t, self.is_cuda, self.device = t, True, torch.device(device)

    def __getattr__(self, name):
        return getattr(self._t, name)


def test_the_predicate_refuses_what_the_kernels_do_not_serve(monkeypatch):
    x, t = _case('3x5x300-saturated')
    dx, dt = _OnDevice(x), _OnDevice(t)
    monkeypatch.setattr(L, 'lovasz_enabled', True)
    assert L.lovasz_softmax_is_fused(dx, dt)                                          # the served case, for contrast
    assert L.lovasz_softmax_is_fused(_OnDevice(x[:1]), _OnDevice(t[:1]), per_cloud=False)    # one cloud IS one list
    assert L.lovasz_softmax_is_fused(_OnDevice(x.half()), dt)
    assert not L.lovasz_softmax_is_fused(x, t)                                        # CPU tensors
    assert not L.lovasz_softmax_is_fused(dx, dt, per_cloud=False)                     # several clouds as one list
    assert not L.lovasz_softmax_is_fused(dx, _OnDevice(t.int()))
    assert not L.lovasz_softmax_is_fused(dx, _OnDevice(t, 'cuda:1'))
    assert not L.lovasz_softmax_is_fused(_OnDevice(x.double()), dt)
    assert not L.lovasz_softmax_is_fused(dx, _OnDevice(t[:, :5]))
    wide = torch.zeros(1, 2, 16385)
    assert L.lovasz_softmax_is_fused(_OnDevice(wide[:, :, :16384]), _OnDevice(torch.zeros(1, 16384, dtype=torch.int64)))
    assert not L.lovasz_softmax_is_fused(_OnDevice(wide), _OnDevice(torch.zeros(1, 16385, dtype=torch.int64)))   # the capacity
    asked = []
    monkeypatch.setattr(L, '_lovasz_workspace_bytes', lambda *a: asked.append(a) or 0)
    assert not L.lovasz_softmax_is_fused(dx, dt) and asked == [(3, 5, 300)]           # the workspace query says no
    monkeypatch.undo()
    monkeypatch.setattr(L, 'lovasz_enabled', False)                                   # PVCNN_FUSED_LOVASZ=0
    assert not L.lovasz_softmax_is_fused(dx, dt)


def test_the_switch_is_read_from_the_environment_once():
    code = 'import pvcnn_amd.modules.functional.loss as L; print(int(L.lovasz_enabled))'
    assert L.lovasz_enabled == (os.environ.get('PVCNN_FUSED_LOVASZ', '1') != '0')
    env = dict(os.environ, PVCNN_FUSED_LOVASZ='0', PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, check=True).stdout
    assert out.strip().splitlines()[-1] == '0'


# ---- modules

def test_modules_are_the_functional_calls():
    x, t = _case('3x5x300-saturated')
    x = x / 60.0
    for kw in (dict(), dict(classes='all'), dict(per_cloud=False), dict(ignore_index=2)):
        assert torch.equal(M.LovaszSoftmax(**kw)(x, t), PF.lovasz_softmax(x, t, **kw))
    w = torch.rand(5, generator=torch.Generator().manual_seed(1)) + 0.5
    t = torch.where(t == -100, torch.full_like(t, 2), t)                              # (torch's CPU cross entropy raises on a stray -100)
    crit =M.CrossEntropyLovasz(0.7, classes='all', weight=w, ignore_index=2, label_smoothing=0.1)
    want = PF.cross_entropy(x, t, w, ignore_index=2, label_smoothing=0.1) + 0.7 * PF.lovasz_softmax(x, t, classes='all', ignore_index=2)
    assert torch.equal(crit(x, t), want) and crit.bad_targets is None
    assert list(crit.state_dict()) == ['cross_entropy.weight']
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    a, b = M.CrossEntropyLovasz(lovasz_weight=0, weight=w)(xa, t), M.CrossEntropyLoss(weight=w)(xb, t)
    assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))          # bit for bit
    a.backward(); b.backward()
    assert torch.equal(xa.grad.view(torch.int32), xb.grad.view(torch.int32))
    for name in ('LovaszSoftmax', 'CrossEntropyLovasz'):
        assert name in M.__all__
    for name in ('lovasz_softmax', 'lovasz_softmax_is_fused', 'lovasz_softmax_parts'):
        assert name in PF.__all__


# ---- the C boundary

def test_the_abi_stays_at_17_and_the_entry_points_refuse_bad_values():
    from pvcnn_amd import _lib
    lib = _lib.load()
    assert lib.pvcnn_version() == 17 == _lib.ABI_VERSION
    q = lib.pvcnn_lovasz_workspace_bytes
    # per-cloud scales padded to 16 bytes, then four fp64 words per list
    assert q(16, 13, 4096) == 64 + 32 * 16 * 13 and q(1, 2, 1) == 16 + 64 and q(3, 50, 16384) == 16 + 32 * 150
    assert q(1, 4, 16385) == 0 and q(0, 4, 8) == 0 and q(2, 0, 8) == 0 and q(2, 4, -1) == 0 and q(65536, 1, 8) == 0
    null = ctypes.c_void_p(None)

    def refused(rc, why):
        assert rc == -1 and why in lib.pvcnn_last_error_string().decode()
    refused(lib.pvcnn_lovasz_probs(null, 10, 1, 2, 16385, null, null), 'bad size')
    refused(lib.pvcnn_lovasz_probs(null, 9, 1, 2, 5, null, null), 'batch stride')
    refused(lib.pvcnn_lovasz_probs(null, 10, 1, 2, 5, null, null), 'null pointer')
    refused(lib.pvcnn_lovasz_sort(null, 10, null, 5, 1, 2, 16385, -100, 0, null, null, null), 'bad size')
    refused(lib.pvcnn_lovasz_sort(null, 10, null, 4, 1, 2, 5, -100, 0, null, null, null), 'batch strides')
    refused(lib.pvcnn_lovasz_sort(null, 10, null, 5, 1, 2, 5, -100, 0, null, null, null), 'null pointer')
    refused(lib.pvcnn_lovasz_finalize(0, 2, 5, 0, null, null, null, null), 'bad size')
    refused(lib.pvcnn_lovasz_finalize(1, 2, 5, 0, null, null, null, null), 'null pointer')
    refused(lib.pvcnn_lovasz_bwd(null, 9, null, null, 1, 2, 5, 0, null, null, null), 'batch stride')
    refused(lib.pvcnn_lovasz_bwd(null, 10, null, null, 1, 2, 5, 0, null, null, null), 'null pointer')
