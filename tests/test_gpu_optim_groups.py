"""FlatAdam beyond the reference's one-group Adam (pvcnn_amd/optim.py, csrc/optim.hip): parameter groups through the run tables, the
AdamW and amsgrad variants, the global gradient norm with its clip coefficient and skip guard, checkpoints in torch's grouped
layout, all of it inside a captured step -- and the three new entry points on offset views inside poisoned allocations.

Bars.  torch.equal wherever the same arithmetic runs through another kernel (a group against a one-group optimizer with that
group's hyper-parameters, clipping with a coefficient of exactly 1, a skipped step, two runs of one norm).  Against torch.optim.Adam:
tests/test_gpu_optim.py's rtol=1e-5, atol=1e-7 over six steps.  The norm against fp64: its relative error may not exceed the larger
of 4 x the error of torch.nn.utils.get_total_norm on the same device tensors and 2^-21 (the roundings of the finalize and the root)."""
import copy
import math

import pytest
import torch
import torch.nn as nn

import embedded as E

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RTOL, ATOL = 1e-5, 1e-7
HA = dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2)
HB = dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.0)


def _toy():
    torch.manual_seed(0)                                   # parameter sizes 231, 33, 33, 33, 165, 5, 324, 4
    return nn.Sequential(nn.Conv1d(7, 33, 1), nn.BatchNorm1d(33), nn.ReLU(), nn.Conv1d(33, 5, 1), nn.Conv3d(3, 4, 3)).to(DEV)


def _split(net, how='decay'):
    """Two lists of parameter INDICES: weights / everything else, or every other parameter (a boundary behind each tensor)."""
    params = list(net.parameters())
    if how == 'decay':
        first = [i for i, p in enumerate(params) if p.dim() > 1]
    else:
        first = list(range(0, len(params), 2))
    return first, [i for i in range(len(params)) if i not in first]


def _groups(net, split, ha=HA, hb=HB):
    params = list(net.parameters())
    return [dict(params=[params[i] for i in split[0]], **ha), dict(params=[params[i] for i in split[1]], **hb)]


def _fake_grads(nets, gen, scale=1.0):
    for ps in zip(*[n.parameters() for n in nets]):
        grad = torch.randn(ps[0].shape, device=DEV, generator=gen) * scale
        for p in ps:
            p.grad = grad.clone()


def _close(nets, what):
    for k, ps in enumerate(zip(*[n.parameters() for n in nets])):
        assert torch.allclose(ps[0], ps[1], rtol=RTOL, atol=ATOL), (what, k, (ps[0] - ps[1]).abs().max().item())


def _bits(t):
    return t.detach().clone().view(torch.int32)


def _snapshot(opt):
    bufs = [b.pflat for b in opt.reducer.buckets] + opt.exp_avg + opt.exp_avg_sq + (opt.max_exp_avg_sq or []) + [opt.step_count]
    return [_bits(t) for t in bufs]


def _norm_errors(opt, grads, what):
    """(FlatAdam's, torch's) relative error of the total norm against fp64; asserts the issue's bar."""
    n64 = math.sqrt(sum((g.double() ** 2).sum().item() for g in grads))
    theirs = abs(torch.nn.utils.get_total_norm(grads).item() - n64) / n64
    mine = abs(opt.grad_norm.item() - n64) / n64
    print(f'[optim_groups] {what}: norm {n64:.9g}  rel. error FlatAdam {mine:.3e}  torch.get_total_norm {theirs:.3e}')
    assert mine <= max(4 * theirs, 2.0 ** -21), (what, mine, theirs)
    return n64


# ---- 1. the run tables index the hyper block: exact ------------------------------------------------------------------------------
@pytest.mark.parametrize('bucket_mb', [8.0, 0.001])
@pytest.mark.parametrize('how', ['decay', 'alternate'])
def test_each_group_gets_its_own_hyper_parameters_bit_for_bit(hip, bucket_mb, how):
    from pvcnn_amd.dp import GradBucketReducer
    from pvcnn_amd.optim import FlatAdam
    net, one_a, one_b, same, one_same = _toy(), _toy(), _toy(), _toy(), _toy()
    split = _split(net, how)
    reds = [GradBucketReducer(n, bucket_mb=bucket_mb) for n in (net, one_a, one_b, same, one_same)]
    assert len(reds[0].buckets) >= (1 if bucket_mb > 1 else 2)
    opts = [FlatAdam(reds[0], param_groups=_groups(net, split)), FlatAdam(reds[1], **HA), FlatAdam(reds[2], **HB),
            FlatAdam(reds[3], param_groups=_groups(same, split, HA, HA)), FlatAdam(reds[4], **HA)]
    assert tuple(opts[0].hyper.shape) == (2, 5) and tuple(opts[1].hyper.shape) == (5,)
    gen = torch.Generator(device=DEV).manual_seed(1)
    for _ in range(6):
        _fake_grads([net, one_a, one_b, same, one_same], gen)
        for red, opt in zip(reds, opts):
            red.finish()
            opt.step()
    twins = (list(one_a.parameters()), list(one_b.parameters()))
    for gid in (0, 1):
        for i in split[gid]:
            p, q = list(net.parameters())[i], twins[gid][i]
            assert torch.equal(p, q), (gid, i, (p - q).abs().max().item())
            for key in ('exp_avg', 'exp_avg_sq'):
                assert torch.equal(opts[0].state[p][key], opts[1 + gid].state[q][key]), (gid, i, key)
    for p, q in zip(same.parameters(), one_same.parameters()):               # both groups equal: the one-group kernel's bits
        assert torch.equal(p, q)
        assert torch.equal(opts[3].state[p]['exp_avg_sq'], opts[4].state[q]['exp_avg_sq'])
    assert opts[0].step_count.item() == 6
    for red in reds:
        red.remove()


# ---- 2. against torch.optim.Adam -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('amsgrad', [False, True])
@pytest.mark.parametrize('decoupled', [False, True])
@pytest.mark.parametrize('grouped', [False, True])
def test_variants_match_torch_adam(hip, grouped, decoupled, amsgrad):
    from pvcnn_amd.dp import GradBucketReducer
    from pvcnn_amd.optim import FlatAdam
    net, twin = _toy(), _toy()
    red = GradBucketReducer(net, bucket_mb=0.001)
    if grouped:
        opt = FlatAdam(red, param_groups=_groups(net, _split(net)), decoupled_weight_decay=decoupled, amsgrad=amsgrad)
        ref = torch.optim.Adam(_groups(twin, _split(twin)), amsgrad=amsgrad, decoupled_weight_decay=decoupled)
    else:
        opt = FlatAdam(red, **HA, decoupled_weight_decay=decoupled, amsgrad=amsgrad)
        ref = torch.optim.Adam(twin.parameters(), **HA, amsgrad=amsgrad, decoupled_weight_decay=decoupled)
    gen = torch.Generator(device=DEV).manual_seed(1)
    for step in range(6):
        _fake_grads([net, twin], gen, scale=(10.0, 0.01)[step % 2])
        red.finish()
        opt.step()
        ref.step()
        _close([net, twin], step)
    if amsgrad:
        for p, q in zip(net.parameters(), twin.parameters()):
            assert torch.allclose(opt.state[p]['max_exp_avg_sq'], ref.state[q]['max_exp_avg_sq'], rtol=RTOL, atol=ATOL)
    red.remove()


# ---- 3. clipping -----------------------------------------------------------------------------------------------------------------
def test_a_clip_coefficient_of_one_changes_no_bit(hip):
    from pvcnn_amd.dp import GradBucketReducer
    from pvcnn_amd.optim import FlatAdam
    net, twin = _toy(), _toy()
    red, red2 = GradBucketReducer(net, bucket_mb=0.001), GradBucketReducer(twin, bucket_mb=0.001)
    opt = FlatAdam(red, param_groups=_groups(net, _split(net)), max_grad_norm=1e30)
    plain = FlatAdam(red2, param_groups=_groups(twin, _split(twin)))
    assert plain.grad_norm is None and opt.grad_norm is not None
    gen = torch.Generator(device=DEV).manual_seed(4)
    for _ in range(3):
        _fake_grads([net, twin], gen)
        red.finish(), red2.finish()
        opt.step(), plain.step()
    for p, q in zip(net.parameters(), twin.parameters()):
        assert torch.equal(p, q)
    red.remove(), red2.remove()


def test_clipping_matches_clip_grad_norm_then_step(hip):
    from pvcnn_amd.dp import GradBucketReducer
    from pvcnn_amd.optim import FlatAdam
    net, again, twin = _toy(), _toy(), _toy()
    red, red2 = GradBucketReducer(net, bucket_mb=0.001), GradBucketReducer(again, bucket_mb=0.001)
    opt = FlatAdam(red, param_groups=_groups(net, _split(net)), max_grad_norm=0.5)
    opt2 = FlatAdam(red2, param_groups=_groups(again, _split(again)), max_grad_norm=0.5)
    ref = torch.optim.Adam(_groups(twin, _split(twin)))
    gen = torch.Generator(device=DEV).manual_seed(5)
    clipped = []
    for step in range(6):
        _fake_grads([net, again, twin], gen, scale=(1.0, 1e-3)[step % 2])    # ~29 and ~0.029: every other step clips
        grads = [p.grad.clone() for p in net.parameters()]
        red.finish(), red2.finish()
        opt.step(), opt2.step()
        n64 = _norm_errors(opt, grads, f'toy net, step {step}')
        assert torch.equal(_bits(opt.grad_norm), _bits(opt2.grad_norm))       # the same step twice: the same bits
        coef = min(1.0, 0.5 / (n64 + 1e-6))
        clipped.append(coef < 1.0)
        for q in twin.parameters():
            q.grad.mul_(coef)
        ref.step()
        _close([net, twin], step)
        for p, g in zip(net.parameters(), grads):                             # p.grad stays the UNCLIPPED gradient
            assert torch.equal(p.grad, g)
    assert clipped == [True, False] * 3
    assert opt.skipped_steps.item() == 0
    red.remove(), red2.remove()


# ---- 4. non-finite gradients -----------------------------------------------------------------------------------------------------
def test_a_nonfinite_gradient_skips_the_step_and_the_next_one_is_unaffected(hip):
    from pvcnn_amd.dp import GradBucketReducer
    from pvcnn_amd.optim import FlatAdam
    net, twin = _toy(), _toy()
    red, red2 = GradBucketReducer(net, bucket_mb=0.001), GradBucketReducer(twin, bucket_mb=0.001)
    assert len(red.buckets) > 1
    make = lambda r, n: FlatAdam(r, param_groups=_groups(n, _split(n)), amsgrad=True, skip_nonfinite=True)      # no max_grad_norm:
    opt, opt2 = make(red, net), make(red2, twin)                                                                   # the norm pass runs for the guard alone
    assert opt.grad_norm is not None and opt.max_grad_norm is None
    gen = torch.Generator(device=DEV).manual_seed(6)
    for _ in range(2):
        _fake_grads([net, twin], gen)
        red.finish(), red2.finish()
        opt.step(), opt2.step()
    before = _snapshot(opt)
    _fake_grads([net], torch.Generator(device=DEV).manual_seed(7))
    red.buckets[-1].params[-1].grad.view(-1)[1] = float('nan')                # ONE element of the last bucket
    red.finish()
    opt.step()
    assert all(torch.equal(a, b) for a, b in zip(before, _snapshot(opt)))     # parameters, three moments, the counter: bit-unchanged
    assert opt.step_count.item() == 2 and opt.skipped_steps.item() == 1 and math.isnan(opt.grad_norm.item())
    _fake_grads([net, twin], gen)
    red.finish(), red2.finish()
    opt.step(), opt2.step()
    for a, b in zip(_snapshot(opt), _snapshot(opt2)):                         # as if the NaN had never been seen
        assert torch.equal(a, b)
    assert opt.step_count.item() == 3 and opt.skipped_steps.item() == 1 and opt2.skipped_steps.item() == 0
    red.remove(), red2.remove()


# ---- 5. more than one sweep of the grid, a scalar tail, a boundary inside a float4 ------------------------------------------------------
def test_grid_stride_and_tail_of_a_large_bucket(hip):
    from pvcnn_amd.dp import GradBucketReducer
    from pvcnn_amd.optim import FlatAdam
    torch.manual_seed(0)
    net = nn.Conv1d(1024, 2101, 1).to(DEV)
    twin = copy.deepcopy(net)
    red = GradBucketReducer(net, bucket_mb=16.0)
    n = red.buckets[0].flat.numel()
    assert len(red.buckets) == 1 and n == 2153525 and n // 4 > 2048 * 256 and n % 4 == 1      # bias (2101 = 4 * 525 + 1) | weight
    # eps = 1e-3: a step moves an element by lr * g / (|g| + eps) with g = coef * grad + wd * p, two terms of ~3e-4 each here.  Among
    # two million elements some cancel to |g| ~ 1e-8, where the 2e-11 the two roundings of coef * grad may differ by is 1e-3 of g:
    # with Adam's 1e-8 such an element moves by up to lr * 2e-11 / 2e-8 = 1e-5 more or less (3e-5 seen), a property of lr / eps and
    # the cancellation, not of the kernel (tests/test_gpu_optim.py's graphed step takes eps = 1e-3 for the same reason)
    ha, hb = dict(HA, eps=1e-3), dict(HB, eps=1e-3)
    groups = lambda m: [dict(params=[m.weight], **ha), dict(params=[m.bias], **hb)]
    opt = FlatAdam(red, param_groups=groups(net), max_grad_norm=0.5)
    ref = torch.optim.Adam(groups(twin))
    gen = torch.Generator(device=DEV).manual_seed(8)
    for step in range(2):
        _fake_grads([net, twin], gen, scale=(1.0, 1e-4)[step])
        grads = [p.grad.clone() for p in net.parameters()]
        red.finish()
        opt.step()
        n64 = _norm_errors(opt, grads, f'2 153 525 elements, step {step}')
        coef = min(1.0, 0.5 / (n64 + 1e-6))
        assert (coef < 1.0) == (step == 0)
        for q in twin.parameters():
            q.grad.mul_(coef)
        ref.step()
        _close([net, twin], step)
    red.remove()


# ---- 6. checkpoints --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('amsgrad', [False, True])
def test_grouped_checkpoints_round_trip_with_torch_adam(hip, amsgrad):
    from pvcnn_amd.dp import GradBucketReducer
    from pvcnn_amd.optim import FlatAdam
    a, b = _toy(), _toy()
    ref = torch.optim.Adam(_groups(a, _split(a)), amsgrad=amsgrad)
    gen = torch.Generator(device=DEV).manual_seed(1)
    for _ in range(3):
        _fake_grads([a], gen)
        ref.step()
    b.load_state_dict(a.state_dict())
    red = GradBucketReducer(b, bucket_mb=0.001)
    wrong = dict(lr=5e-1, betas=(0.5, 0.5), eps=1e-2, weight_decay=0.5)      # the checkpoint's hyper-parameters must win, per group
    flat = FlatAdam(red, param_groups=_groups(b, _split(b), wrong, wrong), amsgrad=amsgrad)
    flat.load_state_dict(ref.state_dict())
    assert flat.step_count.item() == 3
    for g, h in zip(flat.param_groups, (HA, HB)):
        assert all(g[k] == h[k] for k in h)
    assert torch.allclose(flat.hyper.cpu(), torch.tensor([[h['lr'], *h['betas'], h['eps'], h['weight_decay']] for h in (HA, HB)]))
    for _ in range(2):
        _fake_grads([a, b], gen)
        ref.step()
        red.finish()
        flat.step()
    _close([a, b], 'torch -> FlatAdam')
    # ... and back: FlatAdam's state_dict into a fresh grouped torch.optim.Adam on a third copy
    c = _toy()
    c.load_state_dict(b.state_dict())
    back = torch.optim.Adam(_groups(c, _split(c), wrong, wrong), amsgrad=amsgrad)
    sd = flat.state_dict()
    assert [g['params'] for g in sd['param_groups']] == [[0, 1, 2], [3, 4, 5, 6, 7]]
    assert ('max_exp_avg_sq' in sd['state'][0]) == amsgrad
    back.load_state_dict(sd)
    assert back.param_groups[1]['lr'] == HB['lr'] and back.param_groups[0]['weight_decay'] == HA['weight_decay']
    for _ in range(2):
        _fake_grads([b, c], gen)
        red.finish()
        flat.step()
        back.step()
    _close([b, c], 'FlatAdam -> torch')
    red.remove()


def test_a_checkpoint_with_other_group_sizes_is_refused_and_touches_nothing(hip):
    from pvcnn_amd.dp import GradBucketReducer
    from pvcnn_amd.optim import FlatAdam
    a, b = _toy(), _toy()
    params = list(a.parameters())
    ref = torch.optim.Adam([dict(params=params[:4], **HA), dict(params=params[4:], **HB)])      # 4 + 4, not 3 + 5
    gen = torch.Generator(device=DEV).manual_seed(2)
    _fake_grads([a], gen)
    ref.step()
    red = GradBucketReducer(b, bucket_mb=0.001)
    flat = FlatAdam(red, param_groups=_groups(b, _split(b)), amsgrad=False)
    _fake_grads([b], gen)
    red.finish()
    flat.step()
    before, hyper = _snapshot(flat), _bits(flat.hyper)
    with pytest.raises(ValueError, match='sizes'):
        flat.load_state_dict(ref.state_dict())
    three = torch.optim.Adam([dict(params=params[:2]), dict(params=params[2:5]), dict(params=params[5:])])
    with pytest.raises(ValueError, match='3 param groups'):
        flat.load_state_dict(three.state_dict())
    with pytest.raises(ValueError, match='amsgrad'):
        flat.load_state_dict(torch.optim.Adam(_groups(a, _split(a)), amsgrad=True).state_dict())
    assert all(torch.equal(x, y) for x, y in zip(before, _snapshot(flat))) and torch.equal(hyper, _bits(flat.hyper))
    assert flat.param_groups[0]['lr'] == HA['lr'] and flat.param_groups[1]['lr'] == HB['lr']
    with pytest.raises(NotImplementedError):
        flat.add_param_group({'params': [torch.zeros(3, device=DEV, requires_grad=True)]})
    red.remove()


# ---- 7. inside a captured step ---------------------------------------------------------------------------------------------------
def test_groups_clipping_and_a_scheduler_in_a_captured_step(hip):
    """tests/test_gpu_optim.py::test_flat_adam_trains_a_graphed_step's setup and bar (the replays continue the eager trajectory of an
    identically built twin within 1e-3), with two groups, a clip threshold and a StepLR that halves both rates between the steps."""
    import torch.nn.functional as tf
    from pvcnn_amd import workload
    from pvcnn_amd.dp import GradBucketReducer
    from pvcnn_amd.graph import GraphedTrainStep
    from pvcnn_amd.optim import FlatAdam
    torch.manual_seed(0)
    model = workload.PVCNN(13, 6, width_multiplier=0.25).to(DEV).train()
    for m in model.modules():
        if isinstance(m, nn.Dropout):
            m.p = 0.0
    x, y = workload.make_s3dis_batch(2, 1024, device=DEV, seed=3)
    twin = copy.deepcopy(model)
    ha, hb = dict(lr=1e-3, eps=1e-3, weight_decay=1e-4), dict(lr=2e-3, eps=1e-3, weight_decay=0.0)

    def build(net):
        red = GradBucketReducer(net)
        opt = FlatAdam(red, param_groups=_groups(net, _split(net), ha, hb), max_grad_norm=0.1)
        return red, opt, torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    red, opt, sched = build(model)
    red2, opt2, sched2 = build(twin)

    def eager():
        red2.zero_grad()
        loss = tf.cross_entropy(twin(x), y)
        loss.backward()
        red2.finish()
        opt2.step()
        return loss.item(), opt2.grad_norm.item()
    same = [eager() for _ in range(3)]                            # what the three warm-up steps of the captured one do
    sched2.step()
    same.append(eager())
    sched2.step()
    same.append(eager())
    assert any(norm > 0.1 for _, norm in same), same               # the threshold is in play
    step = GraphedTrainStep(model, lambda: tf.cross_entropy(model(x), y), opt, red, warmup=3)
    assert step.graph is not None

    class Watched:                                                  # what the device block holds when the replay is launched
        def __init__(self, graph):
            self.graph, self.seen = graph, []

        def replay(self):
            self.seen.append(opt.hyper[:, 0].cpu().tolist())
            self.graph.replay()
    step.graph = watched = Watched(step.graph)
    got = []
    for _ in range(2):
        sched.step()
        got.append(step().item())
    assert len(watched.seen) == 2 and watched.seen[0] == pytest.approx([0.5e-3, 1e-3], rel=1e-6), watched.seen
    assert watched.seen[1] == pytest.approx([0.25e-3, 0.5e-3], rel=1e-6), watched.seen
    assert abs(got[0] - same[3][0]) <= 1e-3 * abs(same[3][0]) and abs(got[1] - same[4][0]) <= 1e-3 * abs(same[4][0]), (same, got)
    assert math.isfinite(opt.grad_norm.item()) and opt.grad_norm.item() > 0.0
    assert opt.step_count.item() == 5 and opt.skipped_steps.item() == 0


def test_a_captured_step_skips_a_nonfinite_replay_and_trains_on(hip):
    """A plain torch net, so that only the optimizer's kernels meet the non-finite values: the loss is multiplied by a static device
    scalar, and one replay with the scalar at NaN leaves the parameters and the counter as they were."""
    import torch.nn.functional as tf
    from pvcnn_amd.dp import GradBucketReducer
    from pvcnn_amd.graph import GraphedTrainStep
    from pvcnn_amd.optim import FlatAdam
    net = _toy()[:4]
    x = torch.randn(4, 7, 64, device=DEV)
    y = torch.randint(0, 5, (4, 64), device=DEV)
    scale = torch.ones((), device=DEV)
    red = GradBucketReducer(net)
    opt = FlatAdam(red, param_groups=_groups(net, _split(net)), skip_nonfinite=True)
    step = GraphedTrainStep(net, lambda: tf.cross_entropy(net(x), y) * scale, opt, red, warmup=2)
    assert step.graph is not None
    step()
    torch.cuda.synchronize()
    assert opt.step_count.item() == 3 and opt.skipped_steps.item() == 0
    before = _snapshot(opt)
    scale.fill_(float('nan'))
    step()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, _snapshot(opt)))
    assert opt.step_count.item() == 3 and opt.skipped_steps.item() == 1
    scale.fill_(1.0)
    step()
    torch.cuda.synchronize()
    after = _snapshot(opt)
    assert all(not torch.equal(a, b) for a, b in zip(before[:len(red.buckets)], after[:len(red.buckets)]))
    assert opt.step_count.item() == 4 and opt.skipped_steps.item() == 1 and math.isfinite(opt.grad_norm.item())


# ---- 8. the entry points on offset views inside NaN-filled allocations -----------------------------------------------------------------
OFFS = (0, 1, 2, 3)


def _sweep(entry, call, args, roles, mutated, may_refuse=()):
    """call(**args) -> the tensors it wrote.  One role at a time embedded 0..3 elements behind a 16-byte boundary inside a
    sentinel-filled allocation (tests/embedded.py), everything else fresh: the sentinel intact, inputs unwritten, the results
    bit-equal to the plain call's.  may_refuse: the roles whose misalignment a PVCNN_REQUIRE may refuse -- before anything is written."""
    fresh = lambda: {k: v.clone() for k, v in args.items()}
    want = call(**fresh())
    assert not any(E.has_nan(t) for t in want), entry
    marks = {}
    for role in roles:
        marks[role] = ''
        for off in OFFS:
            a = fresh()
            view, whole = E.embed(a[role], off)
            held = view.clone()
            a[role] = view
            what = (entry, role, off)
            try:
                got = call(**a)
            except RuntimeError as err:
                assert off != 0 and role in may_refuse and 'align' in str(err), (what, str(err))
                assert E.intact(whole, view) and torch.equal(view, held), what
                for name in mutated:
                    if name != role:
                        assert torch.equal(_bits(a[name]), _bits(args[name])), (what, name, 'written before the refusal')
                marks[role] += 'x'
                continue
            assert E.intact(whole, view), (what, 'the sentinel around the embedded tensor changed')
            if role not in mutated:
                assert torch.equal(view, held), (what, 'an input was written')
            assert len(got) == len(want)
            for k, (g, w) in enumerate(zip(got, want)):
                assert torch.equal(g, w), (what, f'output {k}')
            marks[role] += '.'
    print(f'[embedded] {entry}: ' + ' '.join(f'{r}={m}' for r, m in marks.items()))
    return marks


def test_new_entry_points_on_embedded_operands(hip):
    from pvcnn_amd.modules.functional.backend import _run
    lib = hip.lib
    gen = torch.Generator().manual_seed(1)
    inf = float('inf')

    def sqsum(g, partials):
        _run(lib.pvcnn_grad_sqsum, 'grad_sqsum', partials, g, g.numel(), partials, partials.numel())
        return (partials,)

    def finalize(partials, status):
        _run(lib.pvcnn_grad_norm_finalize, 'grad_norm_finalize', status, partials, partials.numel(), status)
        return (status,)

    for n in (1021, 1022, 1023, 4096, 5):                   # n = 1, 2, 3 (mod 4): the elements behind n
        g = torch.randn(n, generator=gen).to(DEV)
        parts = torch.full((3,), 7.0, device=DEV)
        marks = _sweep(f'grad_sqsum n={n}', sqsum, dict(g=g, partials=parts), ['g', 'partials'], ('partials',), may_refuse=('g',))
        assert marks['partials'] == '....' and marks['g'][0] == '.'
        total = sqsum(g, parts.clone())[0].double().sum().item()
        assert abs(total - (g.double() ** 2).sum().item()) <= 1e-6 * total
        # status block: norm, coef, skip, skipped | max_norm, skip_nonfinite | reserved
        status = torch.tensor([9.0, 9.0, 9.0, 2.0, 0.5, 1.0, 0.0, 0.0], device=DEV)
        filled = sqsum(g, parts.clone())[0]
        marks = _sweep(f'grad_norm_finalize n={n}', finalize, dict(partials=filled, status=status), ['partials', 'status'], ('status',))
        assert marks == {'partials': '....', 'status': '....'}
        st = finalize(filled.clone(), status.clone())[0].tolist()
        norm = math.sqrt(total)
        assert abs(st[0] - norm) <= 1e-6 * norm and abs(st[1] - min(1.0, 0.5 / (norm + 1e-6))) <= 1e-6 and st[2:] == [0.0, 2.0, 0.5, 1.0, 0.0, 0.0]

    hyper = torch.tensor([[1e-3, 0.9, 0.999, 1e-8, 1e-4], [2e-3, 0.8, 0.99, 1e-6, 0.0]], device=DEV)
    status = torch.tensor([3.0, 0.25, 0.0, 0.0, inf, 1.0, 0.0, 0.0], device=DEV)          # a coefficient of 1/4, no skip

    def grouped(p, g, m, v, vmax, step, hyper, runs, status):
        _run(lib.pvcnn_adam_step_grouped, 'adam_step_grouped', p, p, g, m, v, vmax, p.numel(), step, hyper, hyper.shape[0], runs,
             runs.shape[0], status, 0, 1)
        return p, m, v, vmax, step

    for n in (1021, 1022, 1023, 4096, 5):
        p, g = torch.randn(n, generator=gen).to(DEV), torch.randn(n, generator=gen).to(DEV)
        m, v = (torch.randn(n, generator=gen) * 0.1).to(DEV), (torch.rand(n, generator=gen) * 0.01).to(DEV)
        vmax = (torch.rand(n, generator=gen) * 0.02).to(DEV)
        runs = torch.tensor([[n // 3 | 1, 0], [n // 2 + 1, 1], [n, 0]], dtype=torch.int32, device=DEV)      # boundaries inside float4s
        args = dict(p=p, g=g, m=m, v=v, vmax=vmax, step=torch.full((1,), 3.0, device=DEV), hyper=hyper, runs=runs, status=status)
        marks = _sweep(f'adam_step_grouped n={n}', grouped, args, list(args), ('p', 'm', 'v', 'vmax', 'step'),
                       may_refuse=('p', 'g', 'm', 'v', 'vmax'))
        assert all(mk[0] == '.' for mk in marks.values()) and all(marks[r] == '....' for r in ('step', 'hyper', 'runs', 'status'))
        # all of them inside poisoned allocations at once, as the optimizer's buffers are
        bufs = {k: E.embed(t, 0) for k, t in args.items()}
        got = grouped(**{k: view for k, (view, _) in bufs.items()})
        want = grouped(**{k: t.clone() for k, t in args.items()})
        assert all(torch.equal(a, b) for a, b in zip(got, want)) and want[4].item() == 4.0
        assert all(E.intact(whole, view) for view, whole in bufs.values())
        # torch.optim.Adam(amsgrad=True)'s arithmetic in fp64 on the clipped gradient, each element with its group's row
        gid = torch.zeros(n, dtype=torch.long)
        gid[n // 3 | 1:n // 2 + 1] = 1
        h = hyper.double().cpu()[gid].T.to(DEV)
        gd = 0.25 * g.double() + h[4] * p.double()
        md = m.double() + (gd - m.double()) * (1 - h[1])
        vd = h[2] * v.double() + (1 - h[2]) * gd * gd
        xd = torch.maximum(vmax.double(), vd)
        pd = p.double() - h[0] / (1 - h[1] ** 4) * md / (xd.sqrt() / (1 - h[2] ** 4).sqrt() + h[3])
        assert ((want[0].double() - pd).abs().max() / pd.abs().max()).item() < 1e-5
        # the skip flag: nothing is written, the counter stays
        skip = status.clone()
        skip[2] = 1.0
        held = {k: t.clone() for k, t in args.items()}
        got = grouped(**dict(held, status=skip))
        assert all(torch.equal(_bits(a), _bits(args[k])) for a, k in zip(got, ('p', 'm', 'v', 'vmax', 'step')))
