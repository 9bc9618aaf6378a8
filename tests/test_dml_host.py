"""PF.dml_pair_loss / modules.DMLPairLoss / PF.kl_loss away from the GPU: whatever the kernels do not serve IS the reference's
composition (train_dml.py:125-137: criterion + KLLoss, twice), bit for bit; the predicates say so; one Adam over both networks with
one summed backward is the training of the recipe's two; the ABI stays at 17 with the eight new symbols."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as tf

from conftest import ROOT, SEED

import pvcnn_amd.modules as M
import pvcnn_amd.modules.functional as PF


def _data(b=3, c=5, s=17, seed=SEED):
    g = torch.Generator().manual_seed(seed)
    x = 4.0 * torch.randn(b, c, s, generator=g)
    y = 4.0 * torch.randn(b, c, s, generator=g)
    t = torch.randint(0, c, (b, s), generator=g)
    w = torch.rand(c, generator=g) + 0.5
    return x, y, t, w


def _reference_kl(x, y):
    """modules/functional/loss.py:7-10 of the reference."""
    x = tf.softmax(x.detach(), dim=1)
    y = tf.log_softmax(y, dim=1)
    return torch.mean(torch.sum(x * (torch.log(x) - y), dim=1))


def _reference_pair(o, os_, t, **kw):
    """train_dml.py:125-137 with criterion = nn.CrossEntropyLoss(**kw), criterion_dml = KLLoss()."""
    crit = nn.CrossEntropyLoss(**kw)
    return crit(o, t) + _reference_kl(os_, o), crit(os_, t) + _reference_kl(o, os_)


CASES = {
    'plain': dict(),
    'weight': dict(weight=True),
    'ignore_index': dict(ignore_index=2),
    'smoothing': dict(label_smoothing=0.1),
    'sum': dict(reduction='sum'),
    'all': dict(weight=True, ignore_index=2, label_smoothing=0.1, reduction='sum'),
}


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('case', sorted(CASES))
def test_cpu_tensors_get_the_bits_of_the_reference_composition(case):
    x, y, t, w = _data()
    kw = dict(CASES[case])
    if kw.pop('weight', False):
        kw['weight'] = w
    want_in = [x.clone().requires_grad_(), y.clone().requires_grad_()]
    want = _reference_pair(*want_in, t, **kw)
    want[0].backward(); want[1].backward()
    for fn in (lambda a, b: PF.dml_pair_loss(a, b, t, **kw), lambda a, b: M.DMLPairLoss(nn.CrossEntropyLoss(**kw))(a, b, t),
               lambda a, b: M.DMLPairLoss(M.CrossEntropyLoss(**kw))(a, b, t)):
        a, b = x.clone().requires_grad_(), y.clone().requires_grad_()
        got = fn(a, b)
        assert isinstance(got, tuple) and len(got) == 2
        assert _same(got[0], want[0]) and _same(got[1], want[1])
        got[0].backward(); got[1].backward()
        assert _same(a.grad, want_in[0].grad) and _same(b.grad, want_in[1].grad)
    assert not PF.dml_pair_loss_is_fused(x, y, t, kw.get('weight'), kw.get('ignore_index', -100), kw.get('reduction', 'mean'),
                                         kw.get('label_smoothing', 0.0))
    assert _same(PF.kl_loss(x, y), _reference_kl(x, y)) and _same(M.KLLoss()(x, y), _reference_kl(x, y))
    assert not PF.kl_loss_is_fused(x, y)


def test_the_module_takes_over_the_criterion():
    _, _, _, w = _data()
    assert M.DMLPairLoss().criterion.reduction == 'mean' and M.DMLPairLoss().bad_targets is None
    pair = M.DMLPairLoss(nn.CrossEntropyLoss(weight=w, ignore_index=3, reduction='sum', label_smoothing=0.25))
    c = pair.criterion
    assert isinstance(c, M.CrossEntropyLoss) and torch.equal(c.weight, w)
    assert (c.ignore_index, c.reduction, c.label_smoothing) == (3, 'sum', 0.25)
    assert list(pair.state_dict()) == ['criterion.weight']
    with pytest.raises(TypeError):
        M.DMLPairLoss(nn.NLLLoss())
    for name in ('KLLoss', 'DMLPairLoss'):
        assert name in M.__all__
    for name in ('kl_loss', 'kl_loss_is_fused', 'dml_pair_loss', 'dml_pair_loss_is_fused'):
        assert name in PF.__all__


class _OnDevice:
    """Stands in for a tensor's `is_cuda` / `device` so that the predicates' other clauses can be asked without a GPU."""

    def __init__(self, t, device='cuda:0'):
        self._t, self.is_cuda, self.device = t, True, torch.device(device)

    def __getattr__(self, name):
        return getattr(self._t, name)


def test_the_predicates_refuse_every_case_the_kernels_do_not_serve(monkeypatch):
    from pvcnn_amd.modules.functional import loss as L
    x, y, t, w = _data()
    dx, dy, dt, dw = _OnDevice(x), _OnDevice(y), _OnDevice(t), _OnDevice(w)
    monkeypatch.setattr(L, 'fused_enabled', True)
    monkeypatch.setattr(L, 'dml_enabled', True)
    # the served cases, for contrast
    assert L.kl_loss_is_fused(dx, dy) and L.kl_loss_is_fused(_OnDevice(x.half()), _OnDevice(y.bfloat16()))
    assert L.kl_loss_is_fused(_OnDevice(x.view(3, 5, 17, 1)), _OnDevice(y.view(3, 5, 17, 1)))
    assert L.dml_pair_loss_is_fused(dx, dy, dt) and L.dml_pair_loss_is_fused(dx, dy, dt, dw, 2, 'mean', 0.0)
    # CPU tensors (one or both)
    assert not L.kl_loss_is_fused(x, y) and not L.kl_loss_is_fused(dx, y) and not L.kl_loss_is_fused(x, dy)
    assert not L.dml_pair_loss_is_fused(x, y, t) and not L.dml_pair_loss_is_fused(dx, y, dt) and not L.dml_pair_loss_is_fused(dx, dy, t)
    # a mismatched shape
    assert not L.kl_loss_is_fused(dx, _OnDevice(y[:, :4])) and not L.kl_loss_is_fused(dx, _OnDevice(y[:, :, :5]))
    assert not L.dml_pair_loss_is_fused(dx, _OnDevice(y[:, :4]), dt) and not L.dml_pair_loss_is_fused(dx, dy, _OnDevice(t[:, :5]))
    # a 2-D (B, C) input
    assert not L.kl_loss_is_fused(_OnDevice(x[:, :, 0]), _OnDevice(y[:, :, 0]))
    assert not L.dml_pair_loss_is_fused(_OnDevice(x[:, :, 0]), _OnDevice(y[:, :, 0]), _OnDevice(t[:, 0]))
    # an integer dtype, fp64
    assert not L.kl_loss_is_fused(_OnDevice(x.long()), dy) and not L.kl_loss_is_fused(dx, _OnDevice(y.int()))
    assert not L.kl_loss_is_fused(_OnDevice(x.double()), _OnDevice(y.double()))
    assert not L.dml_pair_loss_is_fused(_OnDevice(x.long()), dy, dt) and not L.dml_pair_loss_is_fused(dx, _OnDevice(y.double()), dt)
    # another device, an empty tensor
    assert not L.kl_loss_is_fused(dx, _OnDevice(y, 'cuda:1')) and not L.dml_pair_loss_is_fused(dx, _OnDevice(y, 'cuda:1'), dt)
    assert not L.kl_loss_is_fused(_OnDevice(x[:0]), _OnDevice(y[:0]))
    # what stays composed: sum, smoothing, a weight the cross entropy does not serve, a non-int ignore_index
    assert not L.dml_pair_loss_is_fused(dx, dy, dt, None, -100, 'sum') and not L.dml_pair_loss_is_fused(dx, dy, dt, None, -100, 'mean', 0.1)
    assert not L.dml_pair_loss_is_fused(dx, dy, dt, w) and not L.dml_pair_loss_is_fused(dx, dy, dt, None, 2.0)
    # the switches: PVCNN_FUSED_DML=0 turns both off, PVCNN_FUSED_XENT=0 the pair only (its promise is torch's cross_entropy everywhere)
    monkeypatch.setattr(L, 'dml_enabled', False)
    assert not L.kl_loss_is_fused(dx, dy) and not L.dml_pair_loss_is_fused(dx, dy, dt)
    monkeypatch.setattr(L, 'dml_enabled', True)
    monkeypatch.setattr(L, 'fused_enabled', False)
    assert L.kl_loss_is_fused(dx, dy) and not L.dml_pair_loss_is_fused(dx, dy, dt)


def test_the_switch_is_read_from_the_environment_once():
    import subprocess
    import sys
    from pvcnn_amd.modules.functional import loss as L
    assert L.dml_enabled == (os.environ.get('PVCNN_FUSED_DML', '1') != '0')
    code = 'import pvcnn_amd.modules.functional.loss as L; print(int(L.dml_enabled), int(L.fused_enabled))'
    env = dict(os.environ, PVCNN_FUSED_DML='0', PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    env.pop('PVCNN_FUSED_XENT', None)
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, check=True).stdout
    assert out.strip().splitlines()[-1] == '0 1'


def _mlp_pair(seed):
    torch.manual_seed(seed)
    return nn.ModuleList([nn.Sequential(nn.Conv1d(4, 8, 1), nn.ReLU(), nn.Conv1d(8, 5, 1)) for _ in range(2)])


def test_one_adam_over_both_networks_is_the_training_of_the_recipes_two():
    """train_dml.py: loss.backward(); optimizer.step(); loss_student.backward(); optimizer_student.step() -- against one summed
    backward and one Adam over both.  kl_loss detaches its first argument, so each loss reaches its own network only, and Adam is
    element-wise: the parameters are bit-equal after three steps."""
    g = torch.Generator().manual_seed(SEED)
    x, t = torch.randn(2, 4, 17, generator=g), torch.randint(0, 5, (2, 17), generator=g)
    recipe, summed = _mlp_pair(3), _mlp_pair(3)
    pair = M.DMLPairLoss(nn.CrossEntropyLoss())
    opt, opt_student = torch.optim.Adam(recipe[0].parameters(), lr=1e-2), torch.optim.Adam(recipe[1].parameters(), lr=1e-2)
    opt_both = torch.optim.Adam(summed.parameters(), lr=1e-2)
    for _ in range(3):
        outputs, outputs_student = recipe[0](x), recipe[1](x)
        assert tuple(outputs.shape) == (2, 5, 17)
        loss, loss_student = pair(outputs, outputs_student, t)
        opt.zero_grad()
        loss.backward()
        opt.step()
        opt_student.zero_grad()
        loss_student.backward()
        opt_student.step()
        both, both_student = pair(summed[0](x), summed[1](x), t)
        assert _same(both.detach(), loss.detach()) and _same(both_student.detach(), loss_student.detach())
        opt_both.zero_grad()
        (both + both_student).backward()
        opt_both.step()
    moved = _mlp_pair(3)
    for p, q, r in zip(recipe.parameters(), summed.parameters(), moved.parameters()):
        assert _same(p.detach(), q.detach()) and not torch.equal(p.detach(), r.detach())


NAMES = ('pvcnn_kl_workspace_bytes', 'pvcnn_kl_partials', 'pvcnn_kl_finalize', 'pvcnn_kl_bwd', 'pvcnn_dml_pair_workspace_bytes',
         'pvcnn_dml_pair_partials', 'pvcnn_dml_pair_finalize', 'pvcnn_dml_pair_bwd')


def test_the_abi_stays_at_17_and_lists_the_new_entry_points():
    from pvcnn_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'pvcnn_hip.h')).read()
    assert re.search(r'#define\s+PVCNN_ABI_VERSION\s+17\b', header) and _lib.ABI_VERSION == 17
    for name in NAMES:
        assert name in _lib.SIGNATURES and re.search(r'PVCNN_API\s+\w+\s+' + name + r'\(', header), name
    lib = _lib.load()
    assert lib.pvcnn_version() == 17
    # 16 bytes of state, four floats per point, one (KL alone) or six (pair) fp64 sums per slot of pvcnn_xent_parts
    assert lib.pvcnn_xent_parts(16, 4096) == 256
    assert lib.pvcnn_kl_workspace_bytes(16, 4096) == 16 + 16 * 16 * 4096 + 8 * 256
    assert lib.pvcnn_dml_pair_workspace_bytes(16, 4096) == 16 + 16 * 16 * 4096 + 6 * 8 * 256
    assert lib.pvcnn_kl_workspace_bytes(0, 5) == 0 and lib.pvcnn_dml_pair_workspace_bytes(0, 5) == 0
    assert lib.pvcnn_kl_workspace_bytes(5, -1) == 0 and lib.pvcnn_dml_pair_workspace_bytes(2 ** 21, 2 ** 20) == 0


def test_the_launchers_refuse_bad_arguments_before_any_launch():
    """Every pointer is NULL: a bad value is refused before the pointers are looked at, and a call that got past the value under
    test would still be refused for its null pointers -- nothing is ever launched."""
    from pvcnn_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(None)

    def refused(rc, why):
        assert rc == -1 and why in lib.pvcnn_last_error_string().decode()
    # (B, C, S) = (1, 2, 5): logits batch stride 10, targets 5
    refused(lib.pvcnn_kl_partials(null, 10, null, 10, 1, 0, 5, null, null), 'bad size')
    refused(lib.pvcnn_kl_partials(null, 10, null, 9, 1, 2, 5, null, null), 'batch strides')
    refused(lib.pvcnn_kl_partials(null, 9, null, 10, 1, 2, 5, null, null), 'batch strides')
    refused(lib.pvcnn_kl_partials(null, 10, null, 10, 1, 2, 5, null, null), 'null pointer')
    refused(lib.pvcnn_kl_finalize(1, 2, 0, null, null, null), 'bad size')
    refused(lib.pvcnn_kl_finalize(1, 2, 5, null, null, null), 'null pointer')
    refused(lib.pvcnn_kl_bwd(null, 10, null, 10, null, -1, 2, 5, null, null, null), 'bad size')
    refused(lib.pvcnn_kl_bwd(null, 10, null, 9, null, 1, 2, 5, null, null, null), 'batch strides')
    refused(lib.pvcnn_kl_bwd(null, 10, null, 10, null, 1, 2, 5, null, null, null), 'null pointer')
    refused(lib.pvcnn_dml_pair_partials(null, 10, null, 10, null, 5, null, 1, 2, 2 ** 41, -100, null, null), 'bad size')
    refused(lib.pvcnn_dml_pair_partials(null, 10, null, 9, null, 5, null, 1, 2, 5, -100, null, null), 'batch strides')
    refused(lib.pvcnn_dml_pair_partials(null, 10, null, 10, null, 4, null, 1, 2, 5, -100, null, null), 'batch strides')
    refused(lib.pvcnn_dml_pair_partials(null, 10, null, 10, null, 5, null, 1, 2, 5, -100, null, null), 'null pointer')
    refused(lib.pvcnn_dml_pair_finalize(0, 2, 5, null, null, null, null), 'bad size')
    refused(lib.pvcnn_dml_pair_finalize(1, 2, 5, null, null, null, null), 'null pointer')
    refused(lib.pvcnn_dml_pair_bwd(null, 10, null, 10, null, 5, null, null, 1, 0, 5, -100, 0, null, null, null), 'bad size')
    refused(lib.pvcnn_dml_pair_bwd(null, 9, null, 10, null, 5, null, null, 1, 2, 5, -100, 0, null, null, null), 'batch strides')
    refused(lib.pvcnn_dml_pair_bwd(null, 10, null, 10, null, 4, null, null, 1, 2, 5, -100, 1, null, null, null), 'batch strides')
    refused(lib.pvcnn_dml_pair_bwd(null, 10, null, 10, null, 5, null, null, 1, 2, 5, -100, 2, null, null, null), 'side')
    refused(lib.pvcnn_dml_pair_bwd(null, 10, null, 10, null, 5, null, null, 1, 2, 5, -100, -1, null, null, null), 'side')
    refused(lib.pvcnn_dml_pair_bwd(null, 10, null, 10, null, 5, null, null, 1, 2, 5, -100, 1, null, null, null), 'null pointer')
