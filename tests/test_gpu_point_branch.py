"""PVConv's point branch handed to the devoxelize gather PRE-BatchNorm (csrc/slab.h AddBnAct, pvcnn_trilinear_devox_bnact_addbn_fwd,
functional/bnact.py BatchNormActDevoxelizePointBN): the gather applies the point branch's BatchNorm + ReLU | LeakyReLU to the addend
quad it adds in its store, so the activated point branch is never written.

  * kernel : the fused gather == bnact_forward on the addend, then the gather with the activated addend, BIT FOR BIT (outputs, inds,
             wgts), through all three gather kernels: the generic one (R = 8; R = 16 / 32 under PVCNN_GATHER_PIPE=0 in a child process,
             the switch being read once per process), the two-row pipeline (R = 16) and the single-row pipeline (R = 32);
  * views  : operands 0..3 elements off a 16-byte boundary inside NaN-filled allocations (tests/embedded.py);
  * module : a training-mode PVConv with the path on (default) against PVCNN_POINT_FUSED=0 in a child process -- the backward runs the
             same passes on the same numbers, the forward the same expressions: outputs and BatchNorm statistics bit for bit, gradients
             within the product bar (1e-5 of the largest reference magnitude; they are printed, and in fact equal);
  * graph  : one captured replay of a width-0.125 PVCNN step equals its eager step."""
import copy
import itertools
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT
import embedded

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BAR = 1e-5            # the project's product bar: max abs error over max abs reference (tests/test_gpu_conv3d.py)


# ---- the kernel, bit for bit ----------------------------------------------------------------------------------------------------------
def forward_cases():
    """(R, B, C, N, slope, affine).  R = 8: the generic kernel (N = 64 one quad row, 192 three); R = 16 with 1024 < N <= 4096: the
    two-row pipeline (C = 5: the last slab holds ONE row); R = 32: the single-row pipeline."""
    out = [(8, 2, c, n, slope, affine) for c, n, slope, affine in itertools.product((5, 64, 128), (64, 192), (0.0, 0.1), (False, True))]
    out += [(16, 2, 5, 1028, 0.0, True), (16, 2, 6, 1028, 0.1, False), (32, 2, 5, 64, 0.0, True), (32, 2, 5, 192, 0.1, False)]
    return out


def make_case(case):
    r, b, c, n, slope, affine = case
    g = torch.Generator().manual_seed(1000 * r + 10 * c + n + int(affine))
    coords = torch.rand(b, 3, n, generator=g) * (r - 1)
    coords[:, :, :n // 8] = torch.round(coords[:, :, :n // 8])
    grid = torch.randn(b, c, r ** 3, generator=g)
    pre = torch.randn(b, c, n, generator=g)
    pre[:, :, 1::7] = 0.0                       # exact zeros (v == shift: either side of 0)
    pre[0, 0, 2] = -0.0                         # ... and one negative zero
    pre[:, :, 3::5] = -pre[:, :, 3::5].abs()    # negative values
    chan = lambda scale, shift: torch.randn(c, generator=g) * scale + shift
    grid_bn = (chan(0.2, 1.0), chan(0.3, 0.0), chan(0.2, 0.0), torch.rand(c, generator=g) + 0.5)
    gamma, beta = (chan(0.2, 1.0), chan(0.3, 0.0)) if affine else (None, None)
    mean, rstd = chan(0.2, 0.0), torch.rand(c, generator=g) + 0.5
    mean[0] = 0.0
    if beta is not None:
        beta[0] = 0.0                           # channel 0: shift == 0, so the zeros of `pre` reach the v > 0 test as +-0
    dev = lambda t: t.to(DEV) if t is not None else None
    return (r, slope, dev(coords), dev(grid), tuple(dev(t) for t in grid_bn), dev(pre), dev(gamma), dev(beta), dev(mean), dev(rstd))


def fused_and_unfused(be, made):
    r, slope, coords, grid, (gg, gb, gm, gr), pre, gamma, beta, mean, rstd = made
    act = be.bnact_forward(pre, gamma, beta, None, None, False, 0.0, 1e-5, slope, stats=(mean, rstd))[0]
    want = be.trilinear_devoxelize_bnact_forward(r, True, coords, grid, gg, gb, gm, gr, 0.1, act)
    got = be.trilinear_devoxelize_bnact_forward(r, True, coords, grid, gg, gb, gm, gr, 0.1, pre, addend_bn=(gamma, beta, mean, rstd, slope))
    return got, want


def check_forward_cases(be):
    for case in forward_cases():
        got, want = fused_and_unfused(be, make_case(case))
        for name, a, b in zip(('outs', 'inds', 'wgts'), got, want):
            assert torch.equal(a, b), (case, name, (a.float() - b.float()).abs().max().item())
        assert not torch.isnan(got[0]).any()


def test_fused_gather_is_bit_identical_in_the_pipelined_and_small_grid_kernels(hip):
    check_forward_cases(hip)


def _child(tmp_path, body, env, *args):
    script = tmp_path / 'child.py'
    script.write_text('import os, sys\nsys.path[:0] = [sys.argv[1], os.path.join(sys.argv[1], "tests")]\n' + body)
    subprocess.run([sys.executable, str(script), ROOT, *map(str, args)], check=True, env=dict(os.environ, **env), timeout=300)


def test_fused_gather_is_bit_identical_in_the_generic_kernel(tmp_path):
    """PVCNN_GATHER_PIPE=0: every shape above through gather_lds_kernel (1024-thread padded slabs at R = 16 / 32)."""
    _child(tmp_path, 'from pvcnn_amd.modules.functional.backend import HipBackend\nimport test_gpu_point_branch as t\n'
                     't.check_forward_cases(HipBackend())\n', {'PVCNN_GATHER_PIPE': '0'})


def test_the_entry_refuses_what_it_does_not_serve(hip):
    made = make_case((8, 2, 5, 64, 0.1, True))
    r, slope, coords, grid, (gg, gb, gm, gr), pre, gamma, beta, mean, rstd = made
    with pytest.raises(RuntimeError):            # a transform without an addend
        hip.trilinear_devoxelize_bnact_forward(r, True, coords, grid, gg, gb, gm, gr, 0.1, None, addend_bn=(gamma, beta, mean, rstd, slope))
    with pytest.raises(RuntimeError):            # statistics of another width
        hip.trilinear_devoxelize_bnact_forward(r, True, coords, grid, gg, gb, gm, gr, 0.1, pre, addend_bn=(gamma, beta, mean[:4], rstd, slope))


# ---- offset views inside NaN-filled allocations ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('off', [0, 1, 2, 3])
def test_offset_views_in_poisoned_allocations(hip, off):
    """Every operand `off` elements behind a 16-byte boundary with the sentinel all around: same bits as on fresh allocations, the pads
    untouched, no NaN in the output (an addend element or a parameter read past its end would be one)."""
    for case in [(8, 2, 5, 64, 0.1, True), (8, 2, 7, 67, 0.0, True), (16, 2, 5, 1028, 0.1, True), (32, 2, 3, 192, 0.0, False)]:
        made = make_case(case)
        r, slope, coords, grid, (gg, gb, gm, gr), pre, gamma, beta, mean, rstd = made
        want = fused_and_unfused(hip, made)[1]
        held = []

        def put(t):
            if t is None:
                return None
            view, whole = embedded.embed(t, off)
            held.append((view, whole))
            return view
        e_coords, e_grid, e_pre = put(coords), put(grid), put(pre)
        e_bn = tuple(put(t) for t in (gg, gb, gm, gr))
        e_add = tuple(put(t) for t in (gamma, beta, mean, rstd))
        got = hip.trilinear_devoxelize_bnact_forward(r, True, e_coords, e_grid, *e_bn, 0.1, e_pre, addend_bn=(*e_add, slope))
        torch.cuda.synchronize()
        for name, a, b in zip(('outs', 'inds', 'wgts'), got, want):
            assert torch.equal(a, b), (case, off, name)
        assert not embedded.has_nan(got[0]) and not embedded.has_nan(got[2]), (case, off)
        for view, whole in held:
            assert embedded.intact(whole, view), (case, off)


# ---- module level: the path on against PVCNN_POINT_FUSED=0 ---------------------------------------------------------------------------------
MODULE_CASES = [(64, 64), (9, 64)]


def run_pvconv(cin, cout, count=None):
    """One training-mode PVConv forward + backward on seeded inputs -> dict of CPU tensors."""
    from pvcnn_amd.modules import PVConv
    torch.manual_seed(7 + cin)
    layer = PVConv(cin, cout, 3, resolution=8).to(DEV).train()
    with torch.no_grad():
        for m in layer.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.weight.uniform_(0.5, 1.5); m.bias.uniform_(-0.3, 0.3)
    g = torch.Generator().manual_seed(11)
    feats = torch.randn(2, cin, 256, generator=g).to(DEV).requires_grad_()
    coords = torch.rand(2, 3, 256, generator=g).to(DEV)
    gy = torch.randn(2, cout, 256, generator=g).to(DEV)
    out = {}
    for step in range(2):                        # (two steps: running statistics and num_batches_tracked move twice)
        layer.zero_grad(); feats.grad = None
        y, _ = layer((feats, coords))
        y.backward(gy)
    torch.cuda.synchronize()
    out['y'] = y.detach().cpu()
    out['grad features'] = feats.grad.cpu()
    for name, p in layer.named_parameters():
        out['grad ' + name] = p.grad.cpu()
    for name, b in layer.named_buffers():
        out['buffer ' + name] = b.detach().cpu()
    return out


def _spy(be):
    """Count the gathers that take a pre-BatchNorm addend."""
    seen, orig = [], be.trilinear_devoxelize_bnact_forward

    def wrapped(*a, **kw):
        seen.append('addend_bn' in kw)
        return orig(*a, **kw)
    be.trilinear_devoxelize_bnact_forward = wrapped
    return seen


def test_pvconv_with_the_path_on_equals_the_path_off(tmp_path):
    from pvcnn_amd.modules.functional import backend as seam
    be = seam._backend
    assert be.has_point_branch_fused, 'this process must run with the path on (PVCNN_POINT_FUSED unset)'
    seen = _spy(be)
    try:
        on = [run_pvconv(*c) for c in MODULE_CASES]
    finally:
        del be.trilinear_devoxelize_bnact_forward
    assert seen and all(seen), seen                      # every gather of these layers took the point branch pre-BatchNorm
    _child(tmp_path, 'import torch\nimport test_gpu_point_branch as t\nfrom pvcnn_amd.modules.functional import backend as seam\n'
                     'assert not seam._backend.has_point_branch_fused\nseen = t._spy(seam._backend)\n'
                     'out = [t.run_pvconv(*c) for c in t.MODULE_CASES]\nassert seen and not any(seen)\ntorch.save(out, sys.argv[2])\n',
           {'PVCNN_POINT_FUSED': '0'}, tmp_path / 'off.pt')
    off = torch.load(tmp_path / 'off.pt')
    for case, a, b in zip(MODULE_CASES, on, off):
        assert a.keys() == b.keys()
        for name in a:
            if name == 'y' or name.startswith('buffer '):
                assert torch.equal(a[name], b[name]), (case, name)
            else:
                err = (a[name].double() - b[name].double()).abs().max().item() / max(b[name].double().abs().max().item(), 1e-30)
                print(case, name, 'relative error', err, 'bitwise equal', torch.equal(a[name], b[name]))
                assert err <= BAR, (case, name, err)


def test_other_configurations_keep_the_separate_pass(hip):
    """eval mode, a hooked point branch, squeeze-and-excitation: the gather takes a finished addend, as before."""
    from pvcnn_amd.modules import PVConv
    from pvcnn_amd.modules.functional import backend as seam
    be = seam._backend
    torch.manual_seed(3)
    feats, coords = torch.randn(2, 16, 128, device=DEV), torch.rand(2, 3, 128, device=DEV)
    plain, hooked, se = (PVConv(16, 16, 3, resolution=8).to(DEV).train(), PVConv(16, 16, 3, resolution=8).to(DEV).train(),
                         PVConv(16, 16, 3, resolution=8, with_se=True).to(DEV).train())
    hooked.point_features.layers[1].register_forward_hook(lambda m, i, o: None)
    seen = _spy(be)
    try:
        plain((feats, coords))
        assert seen == [True]
        del seen[:]
        hooked((feats, coords)); se((feats, coords)); plain.eval()((feats, coords))
        with torch.no_grad():
            plain.train()((feats, coords))
        assert seen == [False, False, False, False], seen
    finally:
        del be.trilinear_devoxelize_bnact_forward


# ---- a captured step ----------------------------------------------------------------------------------------------------------------------
def test_graphed_step_equals_the_eager_step(hip):
    import torch.nn.functional as tf
    from pvcnn_amd import workload
    from pvcnn_amd.dp import GradBucketReducer
    from pvcnn_amd.graph import GraphedTrainStep
    from pvcnn_amd.modules.functional import backend as seam
    torch.manual_seed(0)
    model = workload.PVCNN(13, 6, width_multiplier=0.125).to(DEV).train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    x, y = workload.make_s3dis_batch(2, 1024, device=DEV, seed=3)
    twin = copy.deepcopy(model)
    build = lambda mod: (GradBucketReducer(mod), torch.optim.Adam(mod.parameters(), lr=1e-3, fused=True, capturable=True))
    red, opt = build(model)
    seen = _spy(seam._backend)

    def eager():
        red.zero_grad()
        loss = tf.cross_entropy(model(x), y)
        loss.backward()
        red.finish()
        opt.step()
        return loss
    try:
        want = [eager().item() for _ in range(4)]
        assert seen and all(seen)                        # the model's PVConvs are on the new path
        red2, opt2 = build(twin)
        step = GraphedTrainStep(twin, lambda: tf.cross_entropy(twin(x), y), opt2, red2, warmup=3)   # eager steps 0..2 happen in here
        got = step().item()
    finally:
        del seam._backend.trilinear_devoxelize_bnact_forward
    # the replay is the twin's step 3: the same kernels on the same numbers as the eager model's (test_gpu_graph.py's bound)
    assert abs(want[3] - got) <= 1e-4 * abs(want[3]), (want, got)
