"""Folded inference end to end (pvcnn_amd.fold_batchnorm; functional/_fold.py, functional/bnact.py: run_layers).

Stack level: a folded and an unfolded eval forward of the same nn.Sequential against its fp64 torch-CPU evaluation.  The bar on the
folded path is the project's fp32 tolerance, 1e-5 * (1 + |truth|) per element (README, test_gpu_conv3d.py); the unfolded path's error
is printed and carried in the assertion message next to it.
Network level: the golden eval vectors (tests/golden/pvconv_eval.pt, pvcnn_c0p125_eval.pt) at 1e-5 * (1 + |reference|); a reduced-width
PVCNN++ and the three sub-networks of a reduced-width Frustum-PVCNN, folded against unfolded, at the same bar.  (The Frustum network's
sub-networks are compared one by one on fixed inputs: between them sits a discrete foreground selection, where a last-bit difference
of two logits picks other points -- a property of the network, not of the fold.)
The fold is taken: counted on the backend's methods.  The fallbacks fall back: bit for bit the unfolded path."""
import contextlib
import copy
import os

import pytest
import torch
import torch.nn as nn

import pvcnn_amd
from pvcnn_amd import workload
from pvcnn_amd.modules import PVConv, SharedMLP
from pvcnn_amd.modules.functional import backend as seam
from pvcnn_amd.modules.functional.bnact import run_layers
from test_fold_host import nontrivial_bn_

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
BAR = 1e-5


def rel(got, want):
    want = want.to(torch.float64)
    return ((got.detach().cpu().to(torch.float64) - want.cpu()).abs() / (1 + want.cpu().abs())).max().item()


def load_bn_state(stack, seed):
    g = torch.Generator().manual_seed(seed)
    for m in stack.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            nontrivial_bn_(m, g)
    return stack


def stacks():
    torch.manual_seed(11)
    g = torch.Generator().manual_seed(12)
    yield 'SharedMLP 9-64-64', load_bn_state(SharedMLP(9, [64, 64]).layers, 1), torch.randn(2, 9, 4096, generator=g)
    yield 'SharedMLP 9-64-64 small', load_bn_state(SharedMLP(9, [64, 64]).layers, 2), torch.randn(2, 9, 300, generator=g)
    yield 'SharedMLP dim=2 19-32', load_bn_state(SharedMLP(19, 32, dim=2).layers, 3), torch.randn(2, 19, 64, 8, generator=g)
    for r in (8, 16):
        grid = torch.randn(2, 16, r, r, r, generator=g)
        grid[:, :, :, : r // 2] = 0.0                           # a voxelised cloud leaves most of the cube empty
        yield f'PVConv voxel_layers R={r}', load_bn_state(PVConv(16, 32, 3, r).voxel_layers, 4 + r), grid


@pytest.mark.parametrize('case', list(stacks()), ids=lambda c: c[0])
def test_folded_stack_against_fp64(hip, case):
    name, stack, x = case
    stack.eval()
    with torch.no_grad():
        truth = copy.deepcopy(stack).double()(x.double())
        on_gpu = copy.deepcopy(stack).to(DEV)
        unfolded = run_layers(on_gpu, x.to(DEV))
        pvcnn_amd.fold_batchnorm(on_gpu)
        with count_calls(seam._backend, ['bnact_forward']) as calls:
            folded = run_layers(on_gpu, x.to(DEV))
    assert calls['bnact_forward'] == 0, calls
    e_folded, e_unfolded = rel(folded, truth), rel(unfolded, truth)
    print(f'[fold] {name}: folded {e_folded:.2e}, unfolded {e_unfolded:.2e} (x 1 + |truth|)')
    assert e_folded <= BAR, f'{name}: folded {e_folded:.2e} vs unfolded {e_unfolded:.2e}'


@contextlib.contextmanager
def count_calls(be, names, on_call=None):
    """Count calls of the backend's methods `names` (an instance attribute in front of each; removed afterwards)."""
    counts = {n: 0 for n in names}
    for n in names:
        orig = getattr(be, n)

        def wrapped(*a, _o=orig, _n=n, **kw):
            counts[_n] += 1
            out = _o(*a, **kw)
            if on_call is not None:
                on_call(_n, a, out)
            return out
        setattr(be, n, wrapped)
    try:
        yield counts
    finally:
        for n in names:
            delattr(be, n)


def golden(name):
    return torch.load(os.path.join(GOLD, f'{name}.pt'), weights_only=True)


def golden_pvcnn():
    g = golden('pvcnn_c0p125_eval')
    net = workload.PVCNN(13, 6, width_multiplier=0.125)
    net.load_state_dict(g['state'])
    return net.to(DEV).eval(), g['x'].to(DEV), g


def test_folded_networks_reproduce_the_golden_vectors(hip):
    g = golden('pvconv_eval')
    layer = PVConv(**g['ctor'])
    layer.load_state_dict(g['state'])
    layer = pvcnn_amd.fold_batchnorm(layer.to(DEV))
    x = g['x'].to(DEV)
    with torch.no_grad():
        y, _ = layer((x, x[:, :3, :]))
    e_layer = rel(y, g['y'])
    net, x, g = golden_pvcnn()
    with torch.no_grad():
        e_plain = rel(net(x), g['logits'] if 'logits' in g else g['y'])
        e_net = rel(pvcnn_amd.fold_batchnorm(net)(x), g['logits'] if 'logits' in g else g['y'])
    print(f'[fold] golden PVConv: folded {e_layer:.2e}; golden PVCNN c=0.125: folded {e_net:.2e}, unfolded {e_plain:.2e} (x 1 + |reference|)')
    assert e_layer <= BAR and e_net <= BAR, (e_layer, e_net, e_plain)


def test_folded_pvcnnpp_and_frustum_against_unfolded(hip):
    torch.manual_seed(21)
    net = load_bn_state(workload.PVCNN2(13, 6, width_multiplier=0.25), 22).to(DEV).eval()
    x, _ = workload.make_s3dis_batch(2, 2048)
    x = x.to(DEV)
    with torch.no_grad():
        want = net(x)
        got = pvcnn_amd.fold_batchnorm(net)(x)
    e_pp = rel(got, want)
    print(f'[fold] PVCNN++ c=0.25 B=2 N=2048: folded vs unfolded {e_pp:.2e}')
    assert e_pp <= BAR, e_pp

    fr = load_bn_state(workload.FrustumPVCNNE(3, 12, 8, 128, workload.frustum_size_templates(), 1, 0.25), 23).to(DEV).eval()
    inputs, _ = workload.make_frustum_batch(4, 1024, device=DEV)
    g = torch.Generator().manual_seed(24)
    cloud = {'coords': torch.randn(4, 3, 128, generator=g).to(DEV), 'one_hot_vectors': inputs['one_hot_vectors']}
    runs = [('inst_seg_net', inputs), ('center_reg_net', cloud), ('box_est_net', cloud)]
    with torch.no_grad():
        want = [getattr(fr, name)(arg) for name, arg in runs]
        pvcnn_amd.fold_batchnorm(fr)
        got = [getattr(fr, name)(arg) for name, arg in runs]
    for (name, _), a, b in zip(runs, got, want):
        e = rel(a, b)
        print(f'[fold] Frustum-PVCNN c=0.25 {name}: folded vs unfolded {e:.2e}')
        assert e <= BAR, (name, e)


PREP = ['_weight_split', '_weight_images', '_conv_wt', 'pwconv_weight_transposed']
PLAIN = ['_product_split', 'conv3d_forward', 'pwconv_forward']
ACT = ['conv3d_igemm_split_act', 'pwconv_gemm_split_act', 'conv3d_forward_act', 'pwconv_forward_act']


def test_the_fold_is_taken(hip):
    be = seam._backend
    net, x, _ = golden_pvcnn()
    watched = ['bnact_forward', 'absmax_tiles'] + PREP + PLAIN + ACT
    with torch.no_grad():
        with count_calls(be, watched) as plain:
            net(x)
        assert plain['bnact_forward'] > 0 and sum(plain[n] for n in ACT) == 0, plain
        pvcnn_amd.fold_batchnorm(net)
        net(x)                                                   # the first folded forward makes the weight images
        produced, measured = [], []

        def note(name, args, out):
            if name in ACT:
                produced.append(out[0])                          # (kept alive: an address is never reused while this test looks at it)
            elif name == 'absmax_tiles':
                measured.append(args[0])
        with count_calls(be, watched, note) as folded:
            net(x)
    print(f'[fold] PVCNN c=0.125 calls per forward: unfolded {plain}, folded {folded}')
    n_act = sum(folded[n] for n in ACT)
    # every [conv, BatchNorm, activation] triple outside the PVConv tails (which ride on the devoxelize gather) folds: no BatchNorm pass is left
    assert n_act > 0 and folded['bnact_forward'] == 0, folded
    assert n_act + sum(folded[n] for n in PLAIN) == sum(plain[n] for n in PLAIN), (plain, folded)
    # no re-read of a folded product's output for its scale table
    ptrs = {t.data_ptr() for t in produced}
    assert not any(t.data_ptr() in ptrs for t in measured), 'absmax_tiles on the output of a folded product'
    assert folded['absmax_tiles'] <= plain['absmax_tiles'], (plain, folded)
    # the weight images of the folded products were made by the first forward: what is prepared now belongs to the products left unfused
    # (pwconv_forward transposes its weight itself: one launch inside the method, not one of PREP)
    assert sum(folded[n] for n in PREP) == folded['_product_split'] + folded['conv3d_forward'], folded


def test_the_fallbacks_fall_back(hip):
    net, x, _ = golden_pvcnn()
    twin = copy.deepcopy(net)
    pvcnn_amd.fold_batchnorm(net)
    with torch.no_grad():
        folded = net(x)
    # gradients enabled: the modules as they are
    with count_calls(seam._backend, ACT) as calls:
        got, want = net(x), twin(x)
    assert sum(calls.values()) == 0 and torch.equal(got, want)
    # a BatchNorm buffer changed in place: that triple (and only that one) runs unfused, on the CURRENT state
    bn = next(m for m in net.modules() if isinstance(m, nn.BatchNorm1d))
    bn_twin = next(m for m in twin.modules() if isinstance(m, nn.BatchNorm1d))
    with torch.no_grad():
        bn.running_var.mul_(2)
        bn_twin.running_var.mul_(2)
        changed = net(x)
        pvcnn_amd.unfold_batchnorm(net)
        assert torch.equal(net(x), twin(x))
        assert not torch.equal(changed, folded)
    # ... compared with an unfolded copy: every triple of the copy unfused
    net2, x, _ = golden_pvcnn()
    twin2 = copy.deepcopy(net2)
    pvcnn_amd.fold_batchnorm(net2)
    for m, t in zip(net2.modules(), twin2.modules()):
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            with torch.no_grad():
                m.running_var.mul_(2)
                t.running_var.mul_(2)
    with torch.no_grad():
        assert torch.equal(net2(x), twin2(x))
