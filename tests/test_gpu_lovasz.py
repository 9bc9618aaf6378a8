"""csrc/lovasz.hip behind PF.lovasz_softmax / modules.LovaszSoftmax / modules.CrossEntropyLovasz on the device, against the numpy truth
of tests/lovasz_truth.py.

Two truths per case.  (A) on an fp64 softmax of the same logits: the loss is 1-Lipschitz in the sup norm of the errors (the steps are
non-negative and add up to 1), so |loss - truth| <= tol = 2^-23 * (16 + max|x|), the expf bound of tests/test_gpu_xent.py applied
absolutely.  (B) on the fp32 probabilities the DEVICE produced (PF.lovasz_softmax_parts): one adjacent swap of a foreground /
background pair moves a gradient entry by up to 0.14 of the largest one (list of 64), so only a truth that ranks the same values can
judge the gradient; against it the loss holds 1e-6 relative (an fp64 sum of non-negative terms, rounded to fp32 once), every entry of
d loss / d probabilities holds 1e-6 relative (at most four fp32 roundings from an exact rational) and is exactly 0 where the truth is
(dead points, classes that are not counted, background behind the last foreground), and the gradient for the logits holds 1e-5 of
its largest entry against the fp64 softmax Jacobian on those probabilities."""
import copy
import functools

import numpy as np
import pytest
import torch

import lovasz_truth as T
import pvcnn_amd.modules as M
import pvcnn_amd.modules.functional as PF
from pvcnn_amd.modules.functional import loss as L

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# (1, 2, 1): one point; (2, 3, 63): below a wave, no power of two; (2, 13, 256): no padding; (3, 13, 300): padding, cloud 1 entirely
# ignored; (2, 50, 2048): ShapeNet's class count; (1, 4, 16384): the capacity of a workgroup's LDS
SHAPES = [(1, 2, 1), (2, 3, 63), (2, 13, 256), (3, 13, 300), (2, 50, 2048), (1, 4, 16384)]
REFUSED = (1, 4, 16385)
SCALES = {'n3': 3.0, 'saturated': 180.0}            # N(0, 3), and N(0, 3) x 60: exact ties, the index tie rule decides


@functools.lru_cache(maxsize=None)
def _inputs(shape, scale, one_class=False):
    """(logits fp32, targets) on the CPU: about 10 % of the points ignored, every second class absent."""
    b, c, s = shape
    g = torch.Generator().manual_seed(sum(shape) * 131 + int(scale))
    x = scale * torch.randn(b, c, s, generator=g)
    present = torch.arange(c)[::2]
    t = present[torch.randint(0, len(present), (b, s), generator=g)]
    if one_class:
        t = torch.full_like(t, c - 1)                                                  # G = n for that class
    if s > 1:
        t = torch.where(torch.rand(b, s, generator=g) < 0.1, torch.full_like(t, -100), t)
    if shape == (3, 13, 300):
        t[1] = -100
    return x, t


def _bits(t):
    return t.clone().view(torch.int32 if t.element_size() == 4 else torch.int64)


def _check(x, t, classes, what, expect_fused=True, probas=False, ignore_index=-100):
    """Every bar of the module docstring on one case; x: logits (or, under probas, probabilities) on the CPU."""
    xg, tg = x.to(DEV).requires_grad_(), t.to(DEV)
    kw = dict(classes=classes, ignore_index=ignore_index, probas=probas)
    assert PF.lovasz_softmax_is_fused(xg, tg) == expect_fused
    loss, p, grad_p = PF.lovasz_softmax_parts(xg, tg, **kw)
    out = PF.lovasz_softmax(xg, tg, **kw)
    out.backward()
    assert out.dim() == 0 and out.dtype == torch.float32 and xg.grad.shape == x.shape and xg.grad.is_contiguous()
    if expect_fused:
        assert torch.equal(_bits(out.detach()), _bits(loss))
    pn, gn = p.cpu().numpy().reshape(x.shape), grad_p.double().cpu().numpy().reshape(x.shape)
    got, tn = float(out.item()), t.numpy()
    if not probas:                                                                     # (A)
        want_a, _, _ = T.lovasz_softmax(T.softmax64(x.numpy()), tn, classes, ignore_index)
        tol = 2.0 ** -23 * (16.0 + x.abs().max().item())
        print(f'{what}: loss {got:.9g}; fp64-softmax truth {want_a:.9g}, distance {abs(got - want_a):.3e} (tol {tol:.3e})')
        assert abs(got - want_a) <= tol, what
    want, want_grad, _ = T.lovasz_softmax(pn, tn, classes, ignore_index)               # (B)
    zero = want_grad == 0
    rel = np.abs(gn - want_grad)[~zero] / np.abs(want_grad)[~zero] if (~zero).any() else np.zeros(1)
    chain = want_grad if probas else T.logits_gradient(pn, want_grad)
    grad = xg.grad.double().cpu().numpy()
    err_x = np.abs(grad - chain).max() / max(np.abs(chain).max(), 1e-300)
    print(f'{what}: own-probabilities truth {want:.9g}, rel {abs(got - want) / max(abs(want), 1e-300):.3e}; grad_p worst entry rel '
          f'{rel.max():.3e}, exact zeros {int(zero.sum())}; grad_x err / max {err_x:.3e}')
    assert abs(got - want) <= 1e-6 * abs(want), what
    assert rel.max() <= 1e-6 and (gn[zero] == 0).all(), what
    assert not np.isnan(grad).any() and err_x <= 1e-5, what
    return out.detach(), xg.grad


@pytest.mark.parametrize('classes', ['present', 'all'])
@pytest.mark.parametrize('scale', sorted(SCALES))
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_loss_and_gradients_follow_the_truth(hip, shape, scale, classes):
    x, t = _inputs(shape, SCALES[scale])
    _check(x, t, classes, (shape, scale, classes))


@pytest.mark.parametrize('classes', ['present', 'all'])
def test_every_live_point_of_one_class(hip, classes):
    x, t = _inputs((2, 13, 256), 3.0, one_class=True)
    assert set(t.unique().tolist()) == {-100, 12}
    _check(x, t, classes, ('G = n', classes))


@pytest.mark.parametrize('classes', ['present', 'all'])
def test_a_list_beyond_the_capacity_is_not_fused_and_still_right(hip, classes):
    x, t = _inputs(REFUSED, 3.0)
    _check(x, t, classes, (REFUSED, classes), expect_fused=False)


@pytest.mark.parametrize('classes', ['present', 'all'])
def test_probabilities_as_input(hip, classes):
    for shape, scale in (((3, 13, 300), 3.0), ((2, 3, 63), 180.0)):
        x, t = _inputs(shape, scale)
        _check(torch.softmax(x, 1), t, classes, ('probas', shape, classes), probas=True)


def test_an_ignore_index_inside_the_classes_and_every_point_ignored(hip):
    x, t = _inputs((2, 13, 256), 3.0)
    _check(x, t, 'all', 'ignore_index=4', ignore_index=4)                               # class 4's points are dead, its list has G = 0
    loss, grad = _check(x, torch.full_like(t, -100), 'all', 'all ignored')
    assert loss.item() == 0.0 and torch.equal(grad, torch.zeros_like(grad))


def test_out_of_range_targets_are_ignored_and_counted(hip):
    shape, c = (3, 13, 300), 13
    x, t = _inputs(shape, 3.0)
    t = t.clone()
    spots = [(0, 0), (0, 299), (2, 7), (2, 33)]
    clean = t.clone()
    for (b, s), bad in zip(spots, (c, c + 7, -1, 2 ** 40)):
        t[b, s], clean[b, s] = bad, -100
    assert T.lovasz_softmax(torch.softmax(x, 1).numpy(), t.numpy())[2] == len(spots)
    for classes in ('present', 'all'):
        crit = M.LovaszSoftmax(classes).to(DEV)
        xg, xc = x.to(DEV).requires_grad_(), x.to(DEV).requires_grad_()
        loss = crit(xg, t.to(DEV))
        loss.backward()
        want = PF.lovasz_softmax(xc, clean.to(DEV), classes=classes)
        want.backward()
        assert torch.equal(_bits(loss.detach()), _bits(want.detach())) and torch.equal(_bits(xg.grad), _bits(xc.grad))
        for b, s in spots:
            assert torch.equal(xg.grad[b, :, s], torch.zeros(c, device=DEV))
        assert crit.bad_targets.dtype == torch.int64 and crit.bad_targets.item() == len(spots)
        crit(xg, t.to(DEV))
        assert crit.bad_targets.item() == 2 * len(spots)
    counter = torch.zeros((), dtype=torch.int64, device=DEV)
    PF.lovasz_softmax(x.to(DEV), clean.to(DEV), bad_targets=counter)
    assert counter.item() == 0
    both = M.CrossEntropyLovasz().to(DEV)
    both(x.to(DEV), t.to(DEV))
    assert both.bad_targets.item() == len(spots) and both.lovasz.bad_targets is None     # counted once, by the cross-entropy term


def test_two_runs_give_the_same_bits(hip):
    for shape, scale in (((2, 50, 2048), 180.0), ((1, 4, 16384), 3.0)):
        x, t = _inputs(shape, scale)
        runs = []
        for _ in range(2):
            xg = x.to(DEV).requires_grad_()
            loss = PF.lovasz_softmax(xg, t.to(DEV), classes='all')
            loss.backward()
            runs.append((loss.detach(), xg.grad))
        assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1]))


def _call_log(monkeypatch):
    """Every native call of the criteria, as (label, stream handle, captured?), through the `_run` the loss functions hold."""
    lib, run, ok = L._native()
    log = []

    def logged(fn, label, ref, *args):
        log.append((label, torch.cuda.current_stream(ref.device).cuda_stream, torch.cuda.is_current_stream_capturing()))
        return run(fn, label, ref, *args)
    monkeypatch.setattr(L, '_NATIVE', (lib, logged, ok))
    return log


def test_the_fused_path_is_taken(hip, monkeypatch):
    log = _call_log(monkeypatch)
    x, t = _inputs((3, 13, 300), 3.0)
    xg, tg = x.to(DEV).requires_grad_(), t.to(DEV)
    M.LovaszSoftmax()(xg, tg).backward()
    assert [e[0] for e in log] == ['lovasz_probs', 'lovasz_sort', 'lovasz_finalize', 'lovasz_bwd']
    del log[:]
    PF.lovasz_softmax(torch.softmax(xg, 1), tg, probas=True).backward()
    assert [e[0] for e in log] == ['lovasz_sort', 'lovasz_finalize', 'lovasz_bwd']
    del log[:]
    half = PF.lovasz_softmax(xg.detach().half(), tg)                                   # evaluated in fp32 on the same kernels
    assert half.dtype == torch.float32 and [e[0] for e in log] == ['lovasz_probs', 'lovasz_sort', 'lovasz_finalize']
    del log[:]
    x, t = _inputs(REFUSED, 3.0)
    xg = x.to(DEV).requires_grad_()
    PF.lovasz_softmax(xg, t.to(DEV)).backward()                                        # the refused shape: the composition
    x, t = _inputs((3, 13, 300), 3.0)
    PF.lovasz_softmax(x.to(DEV), t.to(DEV), per_cloud=False)
    assert log == []


@pytest.mark.parametrize('probas', [False, True])
def test_views_inside_larger_allocations(hip, probas):
    """Logits (or probabilities) a channel slice of a NaN-filled wider tensor, targets a column slice of a garbage-filled one, the
    upstream gradient an element of a larger tensor: the bits of the packed call, and the allocations around the views untouched."""
    shape = (3, 13, 300)
    b, c, s = shape
    x, t = _inputs(shape, 3.0)
    if probas:
        x = torch.softmax(x, 1)
    wide = torch.full((b, c + 5, s), float('nan'), device=DEV)
    wide[:, 3:3 + c, :] = x.to(DEV)
    pad = torch.full((b, s + 7), 2 ** 50, dtype=torch.int64, device=DEV)               # read by mistake: counted as a bad target
    pad[:, 2:2 + s] = t.to(DEV)
    ups = torch.full((8,), float('nan'), device=DEV)
    ups[3] = 0.37
    before = [_bits(wide), _bits(pad), _bits(ups)]
    xv = wide[:, 3:3 + c, :].detach().requires_grad_()
    tv = pad[:, 2:2 + s]
    assert not xv.is_contiguous() and not tv.is_contiguous() and PF.lovasz_softmax_is_fused(xv, tv)
    counter = torch.zeros((), dtype=torch.int64, device=DEV)
    loss = PF.lovasz_softmax(xv, tv, classes='all', probas=probas, bad_targets=counter)
    loss.backward(ups[3])
    xp = x.to(DEV).requires_grad_()
    want = PF.lovasz_softmax(xp, t.to(DEV), classes='all', probas=probas)
    want.backward(torch.tensor(0.37, device=DEV))
    assert torch.equal(_bits(loss.detach()), _bits(want.detach())) and torch.equal(_bits(xv.grad), _bits(xp.grad))
    assert xv.grad.is_contiguous() and counter.item() == 0 and not torch.isnan(xv.grad).any()
    for was, now in zip(before, (wide, pad, ups)):
        assert torch.equal(was, _bits(now))


class _Logits(torch.nn.Module):
    """A bare logits parameter behind a 1x1 (diagonal) product: the smallest thing a criterion can train."""

    def __init__(self, x):
        super().__init__()
        self.logits = torch.nn.Parameter(x.clone())
        self.gain = torch.nn.Parameter(torch.ones(1, x.shape[1], 1))

    def forward(self):
        return self.logits * self.gain


def test_captured_step_replays_the_eager_steps_bit_for_bit(hip, monkeypatch):
    """CrossEntropyLovasz inside a GraphedTrainStep: three warm-up steps + three replays give the bits of six eagerly issued steps,
    losses and parameters; the out-of-range labels are counted on every step; and every launch of the criterion goes to the one
    stream of the capture, in order -- the captured criterion is a single chain without parallel branches."""
    from pvcnn_amd.dp import GradBucketReducer
    from pvcnn_amd.graph import GraphedTrainStep
    from pvcnn_amd.optim import FlatAdam
    log = _call_log(monkeypatch)
    x, t = _inputs((3, 13, 300), 3.0)
    y = t.to(DEV).clone()
    y[0, :5] = 13                                                                     # out of range
    model = _Logits(x).to(DEV)
    twin = copy.deepcopy(model)

    def build(mod, crit, capture):
        red = GradBucketReducer(mod)
        opt = FlatAdam(red, lr=1e-2)
        return GraphedTrainStep(mod, lambda: crit(mod(), y), opt, red, warmup=3, capture=capture)
    crit_g, crit_e = M.CrossEntropyLovasz(0.5), M.CrossEntropyLovasz(0.5)
    graphed = build(model, crit_g, True)
    assert graphed.mode == 'graph'
    captured = [e for e in log if e[2]]
    assert [e[0] for e in captured[:5]] == ['xent_partials', 'xent_finalize', 'lovasz_probs', 'lovasz_sort', 'lovasz_finalize']
    assert sorted(e[0] for e in captured[5:]) == ['lovasz_bwd', 'xent_bwd'] and len({e[1] for e in captured}) == 1
    got = [graphed().item() for _ in range(3)]
    eager = build(twin, crit_e, False)
    want = [eager().item() for _ in range(6)]
    print('graph', got, 'eager', want)
    assert got == want[3:] and want[5] < want[0]                                       # the same bits, and it trains
    assert all(torch.equal(_bits(a.detach()), _bits(b.detach())) for a, b in zip(model.parameters(), twin.parameters()))
    assert crit_g.bad_targets.item() == crit_e.bad_targets.item() == 6 * 5
