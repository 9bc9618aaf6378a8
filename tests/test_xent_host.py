"""PF.cross_entropy / modules.CrossEntropyLoss away from the GPU: whatever the kernels do not serve IS torch's cross_entropy, bit for
bit and exception for exception; the predicate says so; from_torch keeps the criterion; the ABI stays at 17 with the new symbols."""
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
    t = torch.randint(0, c, (b, s), generator=g)
    w = torch.rand(c, generator=g) + 0.5
    return x, t, w


CASES = {
    'mean': dict(),
    'sum': dict(reduction='sum'),
    'none': dict(reduction='none'),
    'weight': dict(weight=True),
    'ignore_index': dict(ignore_index=2),
    'smoothing': dict(label_smoothing=0.1),
    'all': dict(weight=True, ignore_index=2, label_smoothing=0.1),
    'all_sum': dict(weight=True, ignore_index=2, label_smoothing=0.1, reduction='sum'),
}


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('case', sorted(CASES))
def test_cpu_tensors_get_torchs_bits(case):
    x, t, w = _data()
    kw = dict(CASES[case])
    if kw.pop('weight', False):
        kw['weight'] = w
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    got, want = PF.cross_entropy(xa, t, **kw), tf.cross_entropy(xb, t, **kw)
    assert _same(got, want)
    got.sum().backward(); want.sum().backward()
    assert _same(xa.grad, xb.grad)
    mod = M.CrossEntropyLoss(**kw)
    assert _same(mod(x, t), want.detach()) and mod.bad_targets is None
    assert not PF.cross_entropy_is_fused(x, t, kw.get('weight'), kw.get('reduction', 'mean'))


def test_two_dim_input_and_probability_targets_are_torchs():
    x, t, w = _data()
    x2, t2 = x[:, :, 0].contiguous(), t[:, 0].contiguous()
    assert _same(PF.cross_entropy(x2, t2, w, label_smoothing=0.2), tf.cross_entropy(x2, t2, w, label_smoothing=0.2))
    probs = torch.softmax(torch.randn(3, 5, 17, generator=torch.Generator().manual_seed(1)), dim=1)
    assert _same(PF.cross_entropy(x, probs, weight=w), tf.cross_entropy(x, probs, weight=w))
    assert _same(M.CrossEntropyLoss(label_smoothing=0.1)(x, probs), tf.cross_entropy(x, probs, label_smoothing=0.1))
    assert not PF.cross_entropy_is_fused(x2, t2) and not PF.cross_entropy_is_fused(x, probs)


def test_bad_shapes_raise_what_torch_raises():
    x, t, w = _data()
    for args, kw in (((x, t[:, :5]), {}), ((x, t), dict(weight=w[:3])), ((x, t), dict(reduction='median')),
                     ((x, t), dict(label_smoothing=1.5)), ((x[0, 0], t[0]), {})):
        with pytest.raises(Exception) as want:
            tf.cross_entropy(*args, **kw)
        with pytest.raises(type(want.value), match=re.escape(str(want.value))):
            PF.cross_entropy(*args, **kw)
        assert not PF.cross_entropy_is_fused(args[0], args[1], kw.get('weight'), kw.get('reduction', 'mean'))


class _OnDevice:
    """Stands in for a tensor's `is_cuda` / `device` so that the predicate's other clauses can be asked without a GPU."""

    def __init__(self, t, device='cuda:0'):
        self._t, self.is_cuda, self.device = t, True, torch.device(device)

    def __getattr__(self, name):
        return getattr(self._t, name)


def test_the_predicate_refuses_every_case_the_kernels_do_not_serve(monkeypatch):
    from pvcnn_amd.modules.functional import loss as L
    x, t, w = _data()
    dx, dt, dw = _OnDevice(x), _OnDevice(t), _OnDevice(w)
    monkeypatch.setattr(L, 'fused_enabled', True)
    assert L.cross_entropy_is_fused(dx, dt) and L.cross_entropy_is_fused(dx, dt, dw, 'sum')          # the served case, for contrast
    assert L.cross_entropy_is_fused(_OnDevice(x.view(3, 5, 17, 1)), _OnDevice(t.view(3, 17, 1)))     # trailing dimensions
    assert not L.cross_entropy_is_fused(x, t)                                                        # CPU tensors
    assert not L.cross_entropy_is_fused(_OnDevice(x[:, :, 0]), _OnDevice(t[:, 0]))                   # 2-D (B, C) input
    assert not L.cross_entropy_is_fused(dx, _OnDevice(torch.softmax(x, 1)))                          # class-probability targets
    assert not L.cross_entropy_is_fused(dx, dt, None, 'none')                                        # reduction='none'
    assert not L.cross_entropy_is_fused(dx, _OnDevice(t.int()))                                      # non-int64 targets
    assert not L.cross_entropy_is_fused(dx, dt, w)                                                   # weight on another device
    assert not L.cross_entropy_is_fused(dx, dt, _OnDevice(w.double()))                               # weight of another dtype
    strided = torch.stack([w, w], dim=1)[:, 0]
    assert not strided.is_contiguous() and L.cross_entropy_is_fused(dx, dt, _OnDevice(strided))      # served: packed before the launch
    assert L.cross_entropy_is_fused(dx, dt, _OnDevice(torch.ones(1).expand(5)))                      # (stride 0 too)
    assert not L.cross_entropy_is_fused(dx, _OnDevice(t, 'cuda:1'))                                  # targets on another device
    assert not L.cross_entropy_is_fused(_OnDevice(x.double()), dt)                                   # fp64 logits
    assert not L.cross_entropy_is_fused(dx, _OnDevice(t[:, :5]))                                     # shapes that do not match
    monkeypatch.setattr(L, 'fused_enabled', False)                                                   # PVCNN_FUSED_XENT=0
    assert not L.cross_entropy_is_fused(dx, dt)


def test_the_switch_is_read_from_the_environment_once():
    import subprocess
    import sys
    code = 'import pvcnn_amd.modules.functional.loss as L; print(int(L.fused_enabled))'
    from pvcnn_amd.modules.functional import loss as L
    assert L.fused_enabled == (os.environ.get('PVCNN_FUSED_XENT', '1') != '0')       # this process: on unless it was started with 0
    env = dict(os.environ, PVCNN_FUSED_XENT='0', PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, check=True).stdout
    assert out.strip().splitlines()[-1] == '0'


def test_from_torch_keeps_the_criterion():
    _, _, w = _data()
    for ref in (nn.CrossEntropyLoss(), nn.CrossEntropyLoss(weight=w, ignore_index=3, reduction='sum', label_smoothing=0.25)):
        mine = M.CrossEntropyLoss.from_torch(ref)
        assert isinstance(mine, nn.CrossEntropyLoss) and isinstance(mine, M.CrossEntropyLoss)
        assert (mine.ignore_index, mine.reduction, mine.label_smoothing) == (ref.ignore_index, ref.reduction, ref.label_smoothing)
        assert (mine.weight is None) == (ref.weight is None) and (ref.weight is None or torch.equal(mine.weight, ref.weight))
        assert list(mine.state_dict()) == list(ref.state_dict())
        ref.load_state_dict(mine.state_dict())
    with pytest.raises(TypeError):
        M.CrossEntropyLoss.from_torch(nn.NLLLoss())
    # the constructor is nn.CrossEntropyLoss's
    assert M.CrossEntropyLoss(w, None, 7, None, 'sum', 0.5).reduction == 'sum'
    assert 'CrossEntropyLoss' in M.__all__ and 'cross_entropy' in PF.__all__ and 'cross_entropy_is_fused' in PF.__all__


def test_the_abi_stays_at_17_and_lists_the_new_entry_points():
    from pvcnn_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'pvcnn_hip.h')).read()
    assert re.search(r'#define\s+PVCNN_ABI_VERSION\s+17\b', header) and _lib.ABI_VERSION == 17
    names = ('pvcnn_xent_parts', 'pvcnn_xent_workspace_bytes', 'pvcnn_xent_partials', 'pvcnn_xent_finalize', 'pvcnn_xent_bwd')
    for name in names:
        assert name in _lib.SIGNATURES and re.search(r'PVCNN_API\s+\w+\s+' + name + r'\(', header), name
    lib = _lib.load()
    assert lib.pvcnn_version() == 17
    # the host-only queries: one slot per 256 points up to the grid cap of 1024 workgroups; 16 bytes of state, five fp64 sums per
    # slot, two floats per point
    assert lib.pvcnn_xent_parts(16, 4096) == 256 and lib.pvcnn_xent_parts(1, 1) == 1 and lib.pvcnn_xent_parts(3, 100000) == 1024
    assert lib.pvcnn_xent_workspace_bytes(16, 4096) == 16 + 5 * 8 * 256 + 8 * 16 * 4096
    assert lib.pvcnn_xent_parts(0, 5) == 0 and lib.pvcnn_xent_workspace_bytes(5, -1) == 0
    # a rejected argument is a return code, not a launch.  Every pointer is NULL: a bad value is refused before the pointers are
    # looked at, and a call that got past the value under test would still be refused for its null pointers
    import ctypes
    null = ctypes.c_void_p(None)

    def refused(rc, why):
        assert rc == -1 and why in lib.pvcnn_last_error_string().decode()
    refused(lib.pvcnn_xent_partials(null, 10, null, 5, null, 1, 0, 5, -100, 0, null, null), 'bad size')
    refused(lib.pvcnn_xent_partials(null, 9, null, 5, null, 1, 2, 5, -100, 0, null, null), 'batch strides')       # stride < C * S
    refused(lib.pvcnn_xent_partials(null, 10, null, 5, null, 1, 2, 5, -100, 0, null, null), 'null pointer')
    refused(lib.pvcnn_xent_finalize(null, 1, 2, 5, 1.5, 1, null, null, null, null), 'label_smoothing')             # smoothing beyond 1
    refused(lib.pvcnn_xent_finalize(null, 1, 2, 5, 0.5, 1, null, null, null, null), 'null pointer')
    refused(lib.pvcnn_xent_bwd(null, 10, null, 4, null, null, 1, 2, 5, -100, 0.0, 1, null, null, null), 'batch strides')
    refused(lib.pvcnn_xent_bwd(null, 10, null, 5, null, null, 1, 2, 5, -100, -0.5, 1, null, null, null), 'label_smoothing')
    refused(lib.pvcnn_xent_bwd(null, 10, null, 5, null, null, 1, 2, 5, -100, 0.0, 1, null, null, null), 'null pointer')
