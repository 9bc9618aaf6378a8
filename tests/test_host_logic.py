"""Host-side logic of the module layer that needs no GPU: layer dispatch, stride handling, batch sharding."""
import pytest
import torch
import torch.nn as nn


def test_batch_strided_gradient_views_are_recognised():
    from pvcnn_amd.modules.functional.backend import batch_strided_ok
    from pvcnn_amd.modules.functional.bnact import _rows
    wide = torch.randn(3, 40, 16)
    sl = wide[:, 8:24, :]                                   # what torch.cat's backward hands to a consumer
    assert not sl.is_contiguous() and batch_strided_ok(sl)
    v = _rows(sl, sl.shape)
    assert v.data_ptr() == sl.data_ptr() and v.stride(0) == 40 * 16, 'channel slices must be consumed in place'
    assert batch_strided_ok(torch.randn(2, 5, 7))
    assert not batch_strided_ok(wide.transpose(1, 2))       # rows not contiguous: needs a copy
    assert not batch_strided_ok(wide[:, :, ::2])
    assert not batch_strided_ok(torch.randn(2, 5, 7).double())
    t = _rows(wide.transpose(1, 2), (3, 16, 40))
    assert t.is_contiguous() and t.shape == (3, 16, 40)
    g5 = torch.randn(2, 6, 4, 4, 4)[:, 1:5]                 # 5-D slice: viewable as (B, C, S) without a copy
    v5 = _rows(g5, g5.shape)
    assert v5.shape == (2, 4, 64) and v5.data_ptr() == g5.data_ptr()


def test_pointwise_detection():
    from pvcnn_amd.modules.functional.bnact import _is_pointwise
    assert _is_pointwise(nn.Conv1d(8, 4, 1))
    assert _is_pointwise(nn.Conv2d(8, 4, 1))
    assert _is_pointwise(nn.Conv2d(8, 4, (1, 1), bias=False))
    assert not _is_pointwise(nn.Conv1d(8, 4, 3, padding=1))
    assert not _is_pointwise(nn.Conv1d(8, 4, 1, stride=2))
    assert not _is_pointwise(nn.Conv1d(8, 8, 1, groups=2))
    assert not _is_pointwise(nn.Conv3d(8, 4, 1))
    assert not _is_pointwise(nn.Linear(8, 4))


def test_run_layers_on_cpu_is_the_plain_sequential():
    """CPU tensors never reach a native kernel: run_layers must be nn.Sequential.forward (same bits, same buffers)."""
    from pvcnn_amd.modules.functional.bnact import fusable_tail, run_layers
    torch.manual_seed(0)
    seq = nn.Sequential(nn.Conv1d(6, 8, 1), nn.BatchNorm1d(8), nn.ReLU(True), nn.Conv1d(8, 5, 1), nn.BatchNorm1d(5), nn.ReLU(True)).train()
    ref = nn.Sequential(*list(seq))                                            # same module objects
    x = torch.randn(4, 6, 32)
    state = {k: v.clone() for k, v in seq.state_dict().items()}
    a = run_layers(seq, x)
    seq.load_state_dict(state)
    b = ref(x)
    assert torch.equal(a, b)
    seq.load_state_dict(state)
    y, part = run_layers(seq, x, stop=4, tail_stats=True)
    assert part is None and y.shape == (4, 5, 32)
    assert fusable_tail(seq, x) is None                       # the fused tail is a GPU-only path


def test_voxelization_cpu_formula_matches_the_reference_expression():
    from pvcnn_amd.modules import Voxelization
    torch.manual_seed(1)
    coords = torch.randn(2, 3, 50)
    for normalize, eps in [(True, 0.0), (True, 1e-3), (False, 0.0)]:
        v = Voxelization(8, normalize=normalize, eps=eps)
        got = v.normalized_coords(coords)
        c = coords - coords.mean(2, keepdim=True)
        want = c / (c.norm(dim=1, keepdim=True).max(dim=2, keepdim=True).values * 2.0 + eps) + 0.5 if normalize else (c + 1) / 2.0
        assert torch.equal(got, torch.clamp(want * 8, 0, 7))


def test_shard_batch():
    from pvcnn_amd.dp import shard_batch
    assert [shard_batch(16, 4, r) for r in range(4)] == [slice(0, 4), slice(4, 8), slice(8, 12), slice(12, 16)]
    with pytest.raises(ValueError):
        shard_batch(10, 4, 0)


def test_coordinate_memo_survives_a_weakref_callback_inside_its_own_critical_section():
    """The memo's weak-reference callback takes the same lock as memo(): a garbage collection that frees a keyed tensor
    while memo() holds the lock must not deadlock (it did with a non-reentrant lock: a hang in training)."""
    import gc
    import threading
    import torch
    from pvcnn_amd.modules.functional import _cache

    done = threading.Event()

    def work():
        for i in range(25):
            t = torch.zeros(3)
            _cache.memo(t, 'k', lambda: i)
            cyc = [t]
            cyc.append(cyc)                     # the tensor dies only through the cycle collector ...
            del t, cyc

            def make():
                gc.collect()                    # ... which runs here, inside memo() of another tensor
                return 1
            u = torch.zeros(3)
            with _cache._lock:                  # the callback fires while this thread holds the lock
                gc.collect()
            assert _cache.memo(u, 'k', make) == 1
        done.set()

    th = threading.Thread(target=work, daemon=True)
    th.start()
    th.join(30)
    assert done.is_set(), 'memo() deadlocked against its own weak-reference callback'


# ---- the f16x2 scale tables ("amax buffers") travel from the BatchNorm pass that writes a tensor to the convolution that reads it ----
class _AmaxStandIn:
    """The native calls of BatchNormAct / VoxelConv3d evaluated with torch on the CPU: what is under test is the WIRING -- the
    BatchNorm apply passes (forward and backward) emit the amax buffer of what they write, the tag rides on the tensor object,
    and the neighbouring convolution picks it up instead of measuring the tensor again."""
    has_conv3d_split = True
    conv_math = 'f16x2'
    CONV_NSPLIT = {'f16x2': 2}
    BNACT_AMAX_MAX_SEG = 256
    PW_AMAX_SEG = 256

    def __init__(self):
        self.calls, self.emitted = [], []

    @staticmethod
    def _table(x3, seg):
        import torch
        b, c, n = x3.shape
        nseg = (n + seg - 1) // seg
        pad = torch.zeros(b, c, nseg * seg)
        pad[:, :, :n] = x3.abs()
        rows = pad.view(b, c, nseg, seg).amax(dim=(1, 3)).reshape(-1)
        return torch.cat([rows.max().reshape(1), rows]).view(torch.int32)

    def conv_amax(self, x, want_global=True):
        self.calls.append('conv_amax')
        return self._table(x.reshape(x.shape[0], x.shape[1], -1), x.shape[2])

    def bnact_forward(self, x3, w, b, rm, rv, training, momentum, eps, slope, stats=None, amax_seg=0, y_amax=None):
        import torch
        mean = x3.mean(dim=(0, 2))
        var = x3.var(dim=(0, 2), unbiased=False)
        rstd = torch.rsqrt(var + eps)
        z = (x3 - mean.view(1, -1, 1)) * (rstd * w).view(1, -1, 1) + b.view(1, -1, 1)
        y = torch.where(z > 0, z, z * slope)
        if amax_seg:
            self.emitted.append(self._table(y, amax_seg))
            return y, mean, rstd, self.emitted[-1]
        return y, mean, rstd

    def bnact_backward(self, x3, g3, w, b, mean, rstd, slope, training, amax_seg=0):
        import torch
        with torch.enable_grad():
            xr = x3.detach().clone().requires_grad_()
            wr, br = w.detach().clone().requires_grad_(), b.detach().clone().requires_grad_()
            m = xr.mean(dim=(0, 2), keepdim=True)
            v = xr.var(dim=(0, 2), unbiased=False, keepdim=True)
            eps = (1.0 / rstd.view(1, -1, 1) ** 2 - v.detach())
            z = (xr - m) * torch.rsqrt(v + eps) * wr.view(1, -1, 1) + br.view(1, -1, 1)
            torch.where(z > 0, z, z * slope).backward(g3)
        out = (xr.grad, wr.grad, br.grad)
        if amax_seg:
            self.emitted.append(self._table(xr.grad, amax_seg))
            return out + (self.emitted[-1],)
        return out

    def conv3d_forward_split(self, x, weight, bias, nsplit, want_stats=False, amax=None):
        import torch
        assert nsplit == 2 and amax is not None and torch.equal(amax, self._table(x.reshape(x.shape[0], x.shape[1], -1), x.shape[2]))
        self.calls.append(('fwd', amax))
        return torch.nn.functional.conv3d(x, weight, bias, padding=1)

    def conv3d_backward_data_split(self, grad_y, weight, nsplit, amax=None):
        import torch
        assert torch.equal(amax, self._table(grad_y.reshape(grad_y.shape[0], grad_y.shape[1], -1), grad_y.shape[2]))
        self.calls.append(('bwd_data', amax))
        b, _, r = grad_y.shape[:3]
        return torch.nn.grad.conv3d_input((b, weight.shape[1], r, r, r), weight, grad_y, padding=1)

    def conv3d_backward_weight_f16_serves(self, x):
        return True

    def conv3d_backward_weight_f16(self, x, grad_y, x_amax, gy_amax, with_bias=False):
        import torch
        self.calls.append(('wgrad', x_amax, gy_amax))
        gw = torch.nn.grad.conv3d_weight(x, (grad_y.shape[1], x.shape[1], 3, 3, 3), grad_y, padding=1)
        return (gw, grad_y.sum(dim=(0, 2, 3, 4))) if with_bias else gw


def test_amax_buffers_travel_from_the_batchnorm_passes_to_the_convolutions(monkeypatch):
    """Conv3d -> BatchNorm3d + LeakyReLU -> Conv3d -> BatchNorm3d + LeakyReLU (PVConv.voxel_layers, modules/pvconv.py:20-27) on the
    autograd nodes of the GPU path with a torch stand-in for the kernels: same output and gradients as the plain modules; the
    second convolution's forward and both convolutions' backward products take the table their BatchNorm neighbour emitted (the
    very same tensor object), and only the first convolution's input is measured by a pass of its own."""
    import torch
    import torch.nn as nn
    from pvcnn_amd.modules.functional import backend as seam, bnact as bnact_mod
    from pvcnn_amd.modules.functional.bnact import BatchNormAct
    from pvcnn_amd.modules.functional import _cache
    from pvcnn_amd.modules.functional.conv3d import voxel_conv3d
    torch.manual_seed(5)
    fake = _AmaxStandIn()
    monkeypatch.setattr(seam, '_backend', fake)
    monkeypatch.setattr(bnact_mod, '_amax_seg_for', lambda shape, is_cuda: int(shape[2]) if len(shape) == 5 else 0)
    r = 4
    convs = [nn.Conv3d(3, 6, 3, padding=1), nn.Conv3d(6, 5, 3, padding=1)]
    bns = [nn.BatchNorm3d(6, eps=1e-4), nn.BatchNorm3d(5, eps=1e-4)]
    with torch.no_grad():
        for bn in bns:
            bn.weight.uniform_(0.5, 1.5); bn.bias.uniform_(-0.5, 0.5)
    x = torch.randn(2, 3, r, r, r)
    x1 = x.clone().requires_grad_()
    ref = x1
    for conv, bn in zip(convs, bns):
        ref = nn.functional.leaky_relu(bn(conv(ref)), 0.1)
    wgt = torch.randn_like(ref)
    (ref * wgt).sum().backward()
    want = [x1.grad] + [p.grad.clone() for m in convs + bns for p in m.parameters()]
    for m in convs + bns:
        for p in m.parameters():
            p.grad = None

    def bn_act(t, bn):          # batch_norm_act() without its is_cuda gate
        seg = t.shape[2]
        y, amax = BatchNormAct.apply(t, bn.weight, bn.bias, None, None, True, 0.1, bn.eps, 0.1, None, None, seg)
        return _cache.tag_amax(y, seg, amax)
    x2 = x.clone().requires_grad_()
    h = x2
    for conv, bn in zip(convs, bns):
        h = bn_act(voxel_conv3d(h, conv.weight, conv.bias, False, 2), bn)
    assert torch.allclose(h, ref, atol=1e-5)
    (h * wgt).sum().backward()
    got = [x2.grad] + [p.grad for m in convs + bns for p in m.parameters()]
    for a, b in zip(got, want):     # (a bias in front of a train-mode BatchNorm has a zero true gradient: pure round-off, ~1e-5)
        assert a is not None and torch.allclose(a, b, rtol=1e-4, atol=1e-4), (a - b).abs().max()
    assert fake.calls.count('conv_amax') == 1                             # only the network input was measured by a separate pass
    emitted = {id(t) for t in fake.emitted}
    assert len(fake.emitted) == 4                                         # two forward applies, two backward applies
    fwd = [c for c in fake.calls if isinstance(c, tuple) and c[0] == 'fwd']
    assert id(fwd[0][1]) not in emitted and id(fwd[1][1]) in emitted      # conv 2 consumed BatchNorm 1's table
    for c in fake.calls:
        if isinstance(c, tuple) and c[0] == 'bwd_data':
            assert id(c[1]) in emitted                                    # gradients arrive tagged by the BatchNorm backward
        if isinstance(c, tuple) and c[0] == 'wgrad':
            assert id(c[2]) in emitted


def test_amax_tag_dies_with_an_in_place_update_and_is_keyed_by_segment_length():
    import torch
    from pvcnn_amd.modules.functional import _cache
    t = torch.randn(8)
    tag = torch.tensor([7, 7], dtype=torch.int32)
    _cache.tag_amax(t, 16, tag)
    assert _cache.amax_of(t, 16) is tag
    assert _cache.amax_of(t, 32) is None                               # another segmentation: not this table
    assert _cache.amax_of(t.view(8), 16) is None                       # another tensor object: not tagged
    t.mul_(2.0)                                                        # modified in place: the tag no longer describes it
    assert _cache.amax_of(t, 16) is None


def test_trace_steady_delimits_steps_by_the_optimizer_not_by_the_gradient_packing(tmp_path):
    """tools/trace_steady.py: the fused-Adam launches end a step; the multi_tensor_apply COPY kernels of the gradient packing
    (pvcnn_amd/dp.py) must not -- counting them as optimizer phases halved every per-step figure once."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    adam = ('void at::native::(anonymous namespace)::multi_tensor_apply_kernel<at::native::(anonymous namespace)::'
            'FusedOptimizerTensorListMetadata<4>, at::native::(anonymous namespace)::FusedAdamMathFunctor<float, 4>, float*>(...)')
    pack = ('void at::native::(anonymous namespace)::multi_tensor_apply_kernel<at::native::(anonymous namespace)::'
            'TensorListMetadata<2>, at::native::(anonymous namespace)::CopyFunctor<float, float, 2, 1, 1>>(...)')
    rows, t = ['Kernel_Name,Start_Timestamp,End_Timestamp'], 0
    for step in range(6):
        for name, dur in (('pvcnn::conv', 300), (pack, 10), ('pvcnn::bn', 50), (pack, 10), (adam, 70), (adam, 70)):
            rows.append(f'"{name}",{t},{t + dur * 1000}')
            t += dur * 1000 + 1000
    trace = tmp_path / 'kernel_trace.csv'
    trace.write_text('\n'.join(rows) + '\n')
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'trace_steady.py'), str(trace), '4', '10', '1'],
                         capture_output=True, text=True, check=True).stdout
    first = out.splitlines()[0]
    assert 'last 4 steps: 24 kernel launches (6/step)' in first, first
    assert 'kernel time 0.510 ms/step' in first, first


def test_bench_byte_formulas_reproduce_the_survey_totals():
    """bench.py's algorithmic bytes (what roofline.achieved is computed from) are SURVEY 8(d)'s formulas: devoxelize forward of the
    R = 32 stage 156.0 MB, backward 155.2 MB, and the eight voxelize + devoxelize calls of a cfg2 step forward + backward 844 MB."""
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location('bench_for_test', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    b, n, s32, s16 = 16, 4096, 32 ** 3, 16 ** 3
    assert bench.bytes_devox_fwd(b, 64, n, s32) == 155_975_680
    assert bench.bytes_devox_bwd(b, 64, n, s32) == 155_189_248
    assert bench.bytes_devox_fwd(b, 64, n, s32, training=False) == 155_975_680 - 64 * b * n
    total = bench.bytes_vox_fwd(b, 9, n, s32) + bench.bytes_vox_bwd(b, 9, n, s32)
    total += sum(bench.bytes_vox_fwd(b, c, n, s16) + bench.bytes_vox_bwd(b, c, n, s16) for c in (64, 64, 64))
    total += bench.bytes_devox_fwd(b, 64, n, s32) + bench.bytes_devox_bwd(b, 64, n, s32)
    total += sum(bench.bytes_devox_fwd(b, c, n, s16) + bench.bytes_devox_bwd(b, c, n, s16) for c in (64, 64, 128))
    assert round(total / 1e6) == 844
    # the traffic table: the committed PMC passes, doubled FETCH_SIZE (gfx950), per launch
    # (round 5: cited only while the table was collected on the kernel sources that are checked out -- a stale table must say so)
    import json
    from pvcnn_amd._lib import sources_digest
    table = json.load(open(os.path.join(os.path.dirname(bench.__file__), 'profiles', 'pmc_traffic.json')))
    t = bench.pmc_traffic('trilinear_devoxelize_fwd', [16, 64, 4096, 32])
    if table.get('sources_digest') == sources_digest():
        assert t['traffic'] is not None and 1.0 <= t['traffic'] / (bench.bytes_devox_fwd(b, 64, n, s32) + 4 * b * 64 * n) <= 1.1
        assert bench.pmc_traffic('no_such_op', [1, 2, 3, 4]) == {'traffic': None}
    else:
        assert t['traffic'] is None and 'not cited' in t['traffic_note']


# ---- PVConv's tail with squeeze-and-excitation as one autograd node: the algebra, checked on the CPU ------------------------------
class _SETailStandIn:
    """The native calls of BatchNormActSEDevoxelize evaluated with torch (float64 friendly) + the CPU oracle's devoxelization."""

    def __init__(self, oracle):
        self.o = oracle

    @staticmethod
    def _z(x3, g, b, mean, rstd):
        xhat = (x3 - mean.view(1, -1, 1)) * rstd.view(1, -1, 1)
        gam = g if g is not None else torch.ones_like(mean)
        bet = b if b is not None else torch.zeros_like(mean)
        return xhat, xhat * gam.view(1, -1, 1) + bet.view(1, -1, 1)

    def bn_stats(self, x3, rm, rv, momentum, eps):
        mean = x3.mean(dim=(0, 2))
        var = x3.var(dim=(0, 2), unbiased=False)
        return mean, torch.rsqrt(var + eps)

    def bnact_partial_sums(self, x3, gy, g, b, mean, rstd, slope):
        xhat, z = self._z(x3, g, b, mean, rstd)
        d = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope)) * (gy if gy is not None else 1.0)
        return d.sum(dim=2), (d * xhat).sum(dim=2)

    def bnact_backward_apply(self, x3, gy, g, b, mean, rstd, sum_gamma, sum_beta, slope, training, bc_mul=None, bc_add=None, amax_seg=256):
        xhat, z = self._z(x3, g, b, mean, rstd)
        gin = gy * (bc_mul.unsqueeze(-1) if bc_mul is not None else 1.0) + (bc_add.unsqueeze(-1) if bc_add is not None else 0.0)
        gp = gin * torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
        scale = ((g if g is not None else torch.ones_like(mean)) * rstd).view(1, -1, 1)
        inv = 1.0 / (x3.shape[0] * x3.shape[2])
        if training:
            gx = scale * (gp - (sum_beta * inv).view(1, -1, 1) - xhat * (sum_gamma * inv).view(1, -1, 1))
        else:
            gx = scale * gp
        return gx, None

    def trilinear_devoxelize_bnact_forward(self, r, is_training, coords, x3, g, b, mean, rstd, slope, addend=None, se_scale=None):
        _, z = self._z(x3, g, b, mean, rstd)
        a = torch.where(z > 0, z, z * slope)
        if se_scale is not None:
            a = a * se_scale.unsqueeze(-1)
        out, inds, wgts = self.o.trilinear_devoxelize_forward(r, True, coords.float().contiguous(), a.float().contiguous())
        out = out.to(x3.dtype)
        if addend is not None:
            out = out + addend
        return [out, inds, wgts]

    def trilinear_devoxelize_backward(self, grad, inds, wgts, r):
        return self.o.trilinear_devoxelize_backward(grad.float().contiguous(), inds, wgts, r).to(grad.dtype)


def test_se_tail_node_matches_the_modules_it_replaces(oracle, monkeypatch):
    """BatchNormActSEDevoxelize (BatchNorm3d + LeakyReLU + SE3d + trilinear_devoxelize + point-branch sum as one node whose backward
    derives every BatchNorm / excitation sum from TWO reduction passes) == the reference's module chain, output and every gradient."""
    import torch.nn as nn
    from pvcnn_amd.modules import SE3d
    from pvcnn_amd.modules import functional as PF
    from pvcnn_amd.modules.functional import backend as seam, bnact as bnact_mod
    from pvcnn_amd.modules.functional.bnact import batch_norm_act_se_devoxelize
    torch.manual_seed(9)
    nb, nc, r, n = 2, 16, 6, 50
    bn, act, se = nn.BatchNorm3d(nc, eps=1e-4), nn.LeakyReLU(0.1), SE3d(nc)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5); bn.bias.uniform_(-0.5, 0.5)
    grid = torch.randn(nb, nc, r, r, r)
    coords = torch.rand(nb, 3, n) * (r - 1)
    addend = torch.randn(nb, nc, n)
    wgt = torch.randn(nb, nc, n)

    # the module chain (with the oracle's devoxelization through the package's own autograd function)
    monkeypatch.setattr(seam, '_backend', oracle)
    g1, a1 = grid.clone().requires_grad_(), addend.clone().requires_grad_()
    out1 = PF.trilinear_devoxelize(se(act(bn(g1))), coords, r, True) + a1
    (out1 * wgt).sum().backward()
    want = [g1.grad, a1.grad, bn.weight.grad, bn.bias.grad, se.fc[0].weight.grad, se.fc[2].weight.grad]
    want = [t.clone() for t in want]
    for p in list(bn.parameters()) + list(se.parameters()):
        p.grad = None

    monkeypatch.setattr(seam, '_backend', _SETailStandIn(oracle))
    monkeypatch.setattr(bnact_mod, '_amax_seg_for', lambda shape, is_cuda: 0)
    bn2 = nn.BatchNorm3d(nc, eps=1e-4)
    bn2.load_state_dict({k: v for k, v in bn.state_dict().items() if 'running' not in k and 'num_batches' not in k}, strict=False)
    g2, a2 = grid.clone().requires_grad_(), addend.clone().requires_grad_()
    out2 = batch_norm_act_se_devoxelize(g2, coords, bn2, 0.1, se, r, True, stats_part=None, addend=a2)
    assert torch.allclose(out2, out1, atol=2e-5), (out2 - out1).abs().max()
    (out2 * wgt).sum().backward()
    got = [g2.grad, a2.grad, bn2.weight.grad, bn2.bias.grad, se.fc[0].weight.grad, se.fc[2].weight.grad]
    for name, a, b in zip(('grid', 'addend', 'bn.weight', 'bn.bias', 'fc1', 'fc2'), got, want):
        assert a is not None and torch.allclose(a, b, rtol=2e-4, atol=2e-5), (name, (a - b).abs().max().item(), b.abs().max().item())


# ---- which kernels a 1x1 convolution takes: the two size bars of functional/pwconv.py ------------------------------------------------
class _PwRouteStandIn:
    """torch stand-ins for the 1x1 kernels that record which of them a layer took."""
    has_pwconv_split = True
    pw_math = 'f16x2'
    PW_NSPLIT = {'f16x2': 2, 'bf16x3': 3, 'fp32': 0}
    PW_AMAX_SEG = 256
    pw_split_min_macs = 1 << 12
    pw_wgrad_f16_min_macs = 1 << 16

    def __init__(self):
        self.calls = []

    def pw_amax(self, x3, want_global=True):
        self.calls.append('pw_amax')
        return x3.abs().amax().reshape(1).view(torch.int32)

    def pwconv_forward(self, x3, w2, b):
        self.calls.append('forward_fp32')
        return torch.einsum('oc,bcn->bon', w2, x3) + (b.view(1, -1, 1) if b is not None else 0)

    def pwconv_forward_split(self, x3, w2, b, nsplit, amax=None):
        self.calls.append(f'forward_split{nsplit}')
        return torch.einsum('oc,bcn->bon', w2, x3) + (b.view(1, -1, 1) if b is not None else 0)

    def pwconv_backward_data(self, g3, w2):
        self.calls.append('bwd_data_fp32')
        return torch.einsum('oc,bon->bcn', w2, g3)

    def pwconv_backward_data_split(self, g3, w2, nsplit, amax=None):
        self.calls.append(f'bwd_data_split{nsplit}')
        return torch.einsum('oc,bon->bcn', w2, g3)

    def pwconv_backward_weight_f16_serves(self, x3):
        return x3.shape[2] % 4 == 0

    def pwconv_backward_weight_f16(self, x3, g3, x_amax, g_amax, with_bias=False):
        self.calls.append('wgrad_f16')
        gw = torch.einsum('bon,bcn->oc', g3, x3)
        return (gw, g3.sum(dim=(0, 2))) if with_bias else gw

    def pwconv_backward_weight(self, x3, g3, with_bias=False):
        self.calls.append('wgrad_fp32')
        gw = torch.einsum('bon,bcn->oc', g3, x3)
        return (gw, g3.sum(dim=(0, 2))) if with_bias else gw


def test_pointwise_conv_routes_by_the_two_size_bars(monkeypatch):
    """functional/pwconv.py: forward / backward-data take the split (f16x2) kernels from `pw_split_min_macs` multiply-adds up, the
    backward-weight its f16x2 kernel only from `pw_wgrad_f16_min_macs` up (it writes 128 x 128 partial tiles per partition: a loss
    on small weight matrices) -- and the results are the plain convolution's either way."""
    from pvcnn_amd.modules.functional import backend as seam
    from pvcnn_amd.modules.functional.pwconv import pointwise_conv, pw_nsplit
    fake = _PwRouteStandIn()
    monkeypatch.setattr(seam, '_backend', fake)
    torch.manual_seed(3)
    for (b, ci, co, n), want in (((1, 4, 4, 64), ['forward_fp32', 'bwd_data_fp32', 'wgrad_fp32']),                    # 1 Ki MACs
                                 ((2, 8, 8, 64), ['pw_amax', 'forward_split2', 'pw_amax', 'bwd_data_split2', 'wgrad_fp32']),   # 8 Ki
                                 ((2, 32, 32, 64), ['pw_amax', 'forward_split2', 'pw_amax', 'bwd_data_split2', 'wgrad_f16'])):  # 128 Ki
        x = torch.randn(b, ci, n, requires_grad=True)
        w = torch.randn(co, ci, 1, requires_grad=True)
        bias = torch.randn(co, requires_grad=True)
        assert pw_nsplit(x, w.view(co, ci)) == (2 if b * ci * co * n >= fake.pw_split_min_macs else 0)
        fake.calls.clear()
        y = pointwise_conv(x, w, bias)
        gy = torch.randn_like(y)
        y.backward(gy)
        assert fake.calls == want, (fake.calls, want)
        x2, w2, b2 = x.detach().clone().requires_grad_(), w.detach().clone().requires_grad_(), bias.detach().clone().requires_grad_()
        torch.nn.functional.conv1d(x2, w2, b2).backward(gy)
        assert torch.allclose(x.grad, x2.grad, atol=1e-5) and torch.allclose(w.grad, w2.grad, atol=1e-4) and torch.allclose(bias.grad, b2.grad, atol=1e-4)


@pytest.mark.parametrize('mode,nsplit', [('f16x2', 2), ('bf16x3', 3), ('fp32', 0), ('tf32', 0), (None, 0)])
def test_pw_nsplit_and_the_routes_follow_every_mode_string(monkeypatch, mode, nsplit):
    """functional/pwconv.py pw_nsplit per `pw_math`: f16x2 -> 2, bf16x3 -> 3, fp32 -> 0; a string the table does not hold -- and a
    backend without the attribute -- falls back to the fp32 kernels (`PW_NSPLIT.get(..., 0)`); below `pw_split_min_macs` it is 0 in
    every mode.  pointwise_conv then takes that family, and only f16x2 measures amax buffers or takes the f16x2 backward-weight."""
    from pvcnn_amd.modules.functional import backend as seam
    from pvcnn_amd.modules.functional.pwconv import pointwise_conv, pw_nsplit
    fake = _PwRouteStandIn()
    if mode is None:
        monkeypatch.delattr(_PwRouteStandIn, 'pw_math')
    else:
        fake.pw_math = mode
    monkeypatch.setattr(seam, '_backend', fake)
    assert nsplit == seam.HipBackend.PW_NSPLIT.get(mode if mode is not None else 'fp32', 0) == fake.PW_NSPLIT.get(mode, 0)
    torch.manual_seed(4)
    below, at = (1, 4, 4, 64), (2, 8, 8, 32)                      # 1 Ki multiply-adds; 4 Ki = the stand-in's bar exactly (`macs < bar`)
    assert below[0] * below[1] * below[2] * below[3] < fake.pw_split_min_macs == at[0] * at[1] * at[2] * at[3]
    split = {2: ['pw_amax', 'forward_split2', 'pw_amax', 'bwd_data_split2', 'wgrad_fp32'],       # (4 Ki < the 64 Ki backward-weight bar)
             3: ['forward_split3', 'bwd_data_split3', 'wgrad_fp32'], 0: ['forward_fp32', 'bwd_data_fp32', 'wgrad_fp32']}
    for (b, ci, co, n), want_nsplit in ((below, 0), (at, nsplit)):
        x = torch.randn(b, ci, n, requires_grad=True)
        w = torch.randn(co, ci, 1, requires_grad=True)
        assert pw_nsplit(x, w.view(co, ci)) == want_nsplit
        fake.calls.clear()
        pointwise_conv(x, w, None).sum().backward()
        assert fake.calls == split[want_nsplit], (mode, fake.calls)
    big = (2, 32, 32, 64)                                         # above both bars: the f16x2 backward-weight kernel in f16x2 mode alone
    x, w = torch.randn(*big[:2], big[3], requires_grad=True), torch.randn(big[2], big[1], 1, requires_grad=True)
    fake.calls.clear()
    pointwise_conv(x, w, None).sum().backward()
    assert fake.calls[-1] == ('wgrad_f16' if nsplit == 2 else 'wgrad_fp32'), (mode, fake.calls)


@pytest.mark.parametrize('mode,nsplit', [('f16x2', 2), ('bf16x3', 3), ('fp32', 0), ('tf32', 0), (None, 0)])
def test_conv_nsplit_and_the_amax_hand_over_follow_every_mode_string(monkeypatch, mode, nsplit):
    """functional/conv3d.py conv_nsplit per `conv_math` (same table, same fallback: `CONV_NSPLIT.get(..., 0)`; 0 without the split
    kernels), and functional/bnact.py _amax_seg_for: a BatchNorm pass emits an amax table only for an f16x2 consumer of ITS kind."""
    from pvcnn_amd.modules.functional import backend as seam
    from pvcnn_amd.modules.functional.bnact import _amax_seg_for
    from pvcnn_amd.modules.functional.conv3d import conv_nsplit

    class Fake:
        has_conv3d_split = has_pwconv_split = True
        CONV_NSPLIT = {'f16x2': 2, 'bf16x3': 3, 'fp32': 0}
        PW_AMAX_SEG, BNACT_AMAX_MAX_SEG = 256, 256
        pw_math = 'f16x2'
    fake = Fake()
    if mode is not None:
        fake.conv_math = mode
    monkeypatch.setattr(seam, '_backend', fake)
    assert nsplit == seam.HipBackend.CONV_NSPLIT.get(mode if mode is not None else 'fp32', 0) == conv_nsplit()
    grid, points = (2, 8, 12, 12, 12), (2, 8, 300)
    assert _amax_seg_for(grid, True) == (12 if mode == 'f16x2' else 0)          # the Conv3d's z row, for an f16x2 Conv3d only
    assert _amax_seg_for(points, True) == 256                                   # ... whatever the Conv3d's mode: the 1x1's own
    assert _amax_seg_for(grid, False) == 0 and _amax_seg_for(points, False) == 0
    fake.pw_math, fake.conv_math = (mode or 'fp32'), 'f16x2'                    # and the reverse pair
    assert _amax_seg_for(points, True) == (256 if mode == 'f16x2' else 0) and _amax_seg_for(grid, True) == 12
    fake.has_conv3d_split = False
    assert conv_nsplit() == 0


def test_classifier_head_and_pooling_fall_back_to_the_modules_on_cpu():
    """workload._classify (fused Dropout, last Conv1d on the package's GEMM) and functional.pooling.neighbor_max (csrc/pool.hip) are
    GPU paths: on CPU tensors they ARE nn.Sequential.forward / torch.max, bit for bit, in train and eval mode."""
    import torch
    import torch.nn as nn
    from pvcnn_amd import workload
    from pvcnn_amd.modules.functional.pooling import neighbor_max
    torch.manual_seed(0)
    layers, _ = workload._head(24, [16, 0.3, 8, 0.3, 5], 1, pointwise=True, classify=True)
    head = nn.Sequential(*layers)
    x = torch.randn(2, 24, 50)
    head.eval()
    assert torch.equal(workload._classify(head, x), head(x))
    head.train()
    torch.manual_seed(1); a = workload._classify(head, x)
    head2 = nn.Sequential(*layers)            # same modules: running statistics moved once more, the outputs of the same draw agree
    torch.manual_seed(1); b = head2(x)
    assert torch.equal(a, b)
    calls = []
    head[0].register_forward_hook(lambda m, i, o: calls.append(1))      # a hooked module: the Sequential's own __call__ path
    workload._classify(head, x)
    assert calls
    y = torch.relu(torch.randn(2, 3, 7, 32))
    ya, yb = y.clone().requires_grad_(), y.clone().requires_grad_()
    neighbor_max(ya).sum().backward(); yb.max(dim=-1).values.sum().backward()
    assert torch.equal(neighbor_max(y), y.max(dim=-1).values) and torch.equal(ya.grad, yb.grad)


def test_weight_bank_serves_an_armed_pair_once_and_never_a_changed_weight():
    """backend._WeightBank.take (host logic of the batched weight-image refresh; the launches are GPU tests): a pair is served once per
    arming, only while the parameter's version counter and address are what they were at the refresh; anything else is noted as
    wanted (for the next table rebuild) and answered with None -- the caller then splits the weight itself."""
    import weakref
    import torch
    from pvcnn_amd.modules.functional.backend import _WeightBank
    bank = _WeightBank(be=None)
    w = torch.nn.Parameter(torch.randn(8, 4, 1))
    w2 = w.view(8, 4)
    key = ('pw', w.data_ptr(), (8, 4), 2)                                              # (kind, address, (Co, Ci), nsplit: 2 = f16x2, 1 = plain bf16)
    assert bank.take('pw', w2) is None and key in bank.wanted and bank.dirty          # first sighting: noted
    wf, wb = torch.zeros(1), torch.zeros(1)
    bank.entries[key] = {'param': weakref.ref(w), 'wf': wf, 'wb': wb, 'armed': True, 'version': w._version, 'epoch': bank.epoch}
    bank.dirty = False
    got = bank.take('pw', w2)
    assert got is not None and got[0] is wf and got[1] is wb
    assert bank.take('pw', w2) is None and not bank.dirty                              # served once per arming
    # a raw-pointer write of the parameters (FlatAdam's kernel: no version counter moves) is announced by an epoch bump:
    # a pair that was armed before it and not consumed is never served afterwards
    bank.entries[key]['armed'] = True
    bank.epoch += 1                                                                     # = HipBackend.weight_bank_invalidate()
    assert bank.take('pw', w2) is None and not bank.entries[key]['armed']
    bank.entries[key]['epoch'] = bank.epoch
    bank.entries[key]['armed'] = True
    with torch.no_grad():
        w.mul_(2.0)                                                                     # in-place change since the refresh
    assert bank.take('pw', w2) is None and not bank.entries[key]['armed']
    assert bank.take('conv', w2) is None and ('conv', w.data_ptr(), (8, 4), 2) in bank.wanted    # the kind is part of the key
    assert bank.take('pw', w2, 1) is None and ('pw', w.data_ptr(), (8, 4), 1) in bank.wanted      # ... and so is the arithmetic (bf16 pairs)
    for i in range(5000):                                                               # temporaries do not pile up
        bank.take('pw', torch.empty(2, 2))
    assert len(bank.wanted) <= 4096


def test_gradient_slots_are_handed_out_once_per_step_and_only_for_a_first_gradient():
    """functional/_gradslots.py (the backward kernels write parameter gradients straight into the reducer's flat buckets): the rules of
    claim(), and that autograd installs the returned alias as `p.grad` without a copy -- `_Bucket.pack` has nothing left to gather."""
    import torch.nn as nn
    from pvcnn_amd.dp import GradBucketReducer
    from pvcnn_amd.modules.functional import _gradslots

    class Lin(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, w, b):
            ctx.save_for_backward(x, w)
            ctx.b = b
            return x @ w.t() + b

        @staticmethod
        def backward(ctx, g):
            x, w = ctx.saved_tensors
            gw, gb = _gradslots.claim(w), _gradslots.claim(ctx.b)
            if gw is None:                                   # (the rules said no: a tensor of its own, as before)
                return g @ w, g.t() @ x, g.sum(0)
            torch.mm(g.t(), x, out=gw)
            gb.copy_(g.sum(0))
            return g @ w, gw, gb

    torch.manual_seed(0)
    m = nn.Linear(4, 3)
    ref = nn.Linear(4, 3)
    ref.load_state_dict(m.state_dict())
    red = GradBucketReducer(m)
    x = torch.randn(5, 4)
    copied = []
    orig = torch._foreach_copy_
    torch._foreach_copy_ = lambda d, s: (copied.append(len(d)), orig(d, s))[1]
    try:
        red.zero_grad()
        Lin.apply(x, m.weight, m.bias).square().sum().backward()
        red.finish()
        assert copied == []                                  # both gradients were written in place and taken over as they were
        ref(x).square().sum().backward()
        assert torch.allclose(m.weight.grad, ref.weight.grad) and torch.allclose(m.bias.grad, ref.bias.grad)
        view = next(v for p, v in zip(red.buckets[0].params, red.buckets[0].views) if p is m.weight)
        assert m.weight.grad.data_ptr() == view.data_ptr()
        # a second backward WITHOUT zero_grad accumulates: p.grad exists, so no slot -- autograd adds the node's own tensor
        Lin.apply(x, m.weight, m.bias).square().sum().backward()
        red.finish()
        assert torch.allclose(m.weight.grad, 2 * ref.weight.grad)
        # a parameter used twice in one graph: the slot goes to the first use only, the sum is still right
        red.zero_grad()
        (Lin.apply(x, m.weight, m.bias) + Lin.apply(2 * x, m.weight, m.bias)).square().sum().backward()
        red.finish()
        ref.zero_grad()
        (ref(x) + ref(2 * x)).square().sum().backward()
        assert torch.allclose(m.weight.grad, ref.weight.grad, rtol=1e-5, atol=1e-6)
    finally:
        torch._foreach_copy_ = orig
    red.zero_grad()
    with torch.no_grad():
        a = _gradslots.claim(m.weight)
        assert a is not None and a is not view and a.data_ptr() == view.data_ptr() and a.shape == m.weight.shape
        assert _gradslots.claim(m.weight) is None            # once per step
        assert _gradslots.claim(m.weight.view(12)) is None   # (still the same slot)
    red.zero_grad()
    assert _gradslots.claim(m.weight) is None                # grad mode on (create_graph): the node's result must be differentiable
    with torch.no_grad():
        assert _gradslots.claim(torch.zeros(3, 4)) is None   # not a registered parameter
        assert _gradslots.claim(m.weight.view(12)).shape == (12,)     # a contiguous view of the whole parameter gets the slot, shaped like it
    red.remove()
    with torch.no_grad():
        assert _gradslots.claim(m.bias) is None              # the reducer is gone


def test_the_per_tensor_judge_fails_a_dense_error_and_passes_a_sparse_flip():
    """tests/test_gpu_train_parity.judge_per_tensor (the whole-network bar since round 5), on synthetic gradients: a 10 % error of ONE
    whole tensor fails although another tensor of the network is far worse in the oracle stack (the round-4 bar, one number per
    network set by the worst tensor, let it pass); one flipped element passes as a counted flip site; a small dense excess passes only
    in FRONT of a flip site (its shadow) and never behind one or without one; a forward-only quantity (a running statistic) never gets
    an allowance."""
    import test_gpu_train_parity as tp
    g = torch.Generator().manual_seed(0)
    truth = {'<input>': torch.randn(4, 9, 64, generator=g).double(), 'a.weight': torch.randn(32, 16, generator=g).double(),
             'b.weight': torch.randn(64, 32, generator=g).double(), 'c.weight': torch.randn(64, 32, generator=g).double(),
             'd.weight': torch.randn(8, 8, generator=g).double(), 'e.weight': torch.randn(8, 8, generator=g).double(),
             'f.weight': torch.randn(8, 8, generator=g).double(), 'g.weight': torch.randn(8, 8, generator=g).double(),
             'buffer bn.running_mean': torch.randn(32, generator=g).double()}
    noise = lambda t, rel: t + rel * t.abs().max() * torch.randn(t.shape, generator=g).double().clamp(-1, 1)
    cpu = {k: noise(v, 1e-6) for k, v in truth.items()}
    cpu['c.weight'] = noise(truth['c.weight'], 5e-2)                   # the network's ill-conditioned tensor: the oracle stack is 5e-2 off
    hip = {k: noise(v, 1e-6) for k, v in truth.items()}
    judge = lambda label, h, cap=1e-2: tp.judge_per_tensor(label, ((0.0, h), (0.0, cpu), (0.0, truth)), flip_cap=cap)
    ok = judge('synthetic: all within', hip)
    assert all(r['hip'] <= r['bar'] for r in ok)

    dense = dict(hip)
    dense['a.weight'] = truth['a.weight'] * 1.1                        # a wrong scale on one tensor
    worst_cpu = max(r['cpu'] for r in ok)
    assert (dense['a.weight'] - truth['a.weight']).abs().max() / truth['a.weight'].abs().max() < 4 * worst_cpu   # the old bar passes it
    with pytest.raises(AssertionError, match='a.weight'):
        judge('synthetic: dense 10 %', dense)

    flip = dict(hip)
    flip['b.weight'] = hip['b.weight'].clone()
    flip['b.weight'][1, 2] += 5e-3 * truth['b.weight'].abs().max()    # one element: a flipped decision in layer b
    rows = judge('synthetic: one flip', flip)
    assert [r['name'] for r in rows if r['hip'] > r['bar']] == ['b.weight']
    with pytest.raises(AssertionError, match='b.weight'):              # ... but not beyond the cap
        judge('synthetic: one flip, tight cap', flip, 1e-3)

    shadow = dict(flip)
    shadow['a.weight'] = noise(truth['a.weight'], 5e-4)                # IN FRONT of the site (forward order): its shadow, admitted
    rows = judge('synthetic: a flip and its shadow', shadow)
    assert sorted(r['name'] for r in rows if r['hip'] > r['bar']) == ['a.weight', 'b.weight']
    behind = dict(flip)
    behind['d.weight'] = noise(truth['d.weight'], 5e-4)                # BEHIND the site: no flip can explain it
    with pytest.raises(AssertionError, match='d.weight'):
        judge('synthetic: dense excess behind the site', behind)
    alone = dict(hip)
    alone['a.weight'] = noise(truth['a.weight'], 5e-4)                 # no site at all
    with pytest.raises(AssertionError, match='a.weight'):
        judge('synthetic: dense excess without a site', alone)

    stat = dict(hip)
    stat['buffer bn.running_mean'] = hip['buffer bn.running_mean'].clone()
    stat['buffer bn.running_mean'][5] += 1e-3 * truth['buffer bn.running_mean'].abs().max()
    with pytest.raises(AssertionError, match='running_mean'):
        judge('synthetic: a running statistic off', stat)

    # round 6: what the network RETURNS is a forward-only row too -- one point's logits off by 1e-3 of the largest fails whatever the
    # gradients do; _grads puts the rows in front of `<input>`
    class _Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(3))
    leaf = torch.ones(2, 3, requires_grad=True)
    out = (leaf * _Net().w).sum()
    out.backward()
    assert list(tp._grads(_Net(), leaf, leaf.detach() * 2))[:2] == ['<logits>', '<input>']
    assert list(tp._grads(_Net(), leaf, {'mask_logits': leaf.detach(), 'n': torch.zeros(2, dtype=torch.long)}))[0] == '<output mask_logits>'
    with_out = lambda d, o: {'<logits>': o, **d}
    logits = torch.randn(2, 13, 64, generator=g).double()
    cpu['<logits>'] = noise(logits, 1e-7)
    truth['<logits>'] = logits
    rows = judge('synthetic: logits within 1e-5', with_out(hip, noise(logits, 1e-6)))
    assert [r['forward_only'] for r in rows if r['name'] == '<logits>'] == [True]
    off = noise(logits, 1e-7)
    off[1, 3, 7] += 1e-3 * logits.abs().max()
    with pytest.raises(AssertionError, match='<logits>'):
        judge('synthetic: one point of the logits off', with_out(hip, off))


def test_the_sampling_chain_accepts_only_the_tensor_it_expects():
    """pvcnn_amd.workload._SamplingChain (PVCNN++'s sampling ahead): identity + in-place version, and a refusal breaks the chain for good."""
    import torch
    from pvcnn_amd.workload import _SamplingChain
    a = torch.zeros(2, 3, 8)
    chain = _SamplingChain(a)
    assert chain.accepts(a) and not chain.broken
    b = torch.zeros(2, 3, 4)
    chain.expect(b)
    assert chain.accepts(b)
    assert not chain.accepts(a) and chain.broken               # another tensor
    assert not chain.accepts(b)                                # ... and broken stays broken
    chain = _SamplingChain(a)
    a.add_(1.0)
    assert not chain.accepts(a) and chain.broken               # the same tensor, modified in place
    chain = _SamplingChain(a)
    del a
    assert not chain.accepts(torch.zeros(2, 3, 8))             # the expected tensor is gone


def test_the_roofline_launch_is_priced_on_the_slower_trustworthy_timing():
    """bench.py price_launch_us: max(burst, in-graph) with a trace of the running sources, max(burst, in-step pairs) without one --
    never the optimistic figure alone."""
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location('bench_for_pricing', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    us, label = bench.price_launch_us(31.1, 35.3, 36.4)
    assert us == 36.4 and 'in-graph' in label
    us, label = bench.price_launch_us(38.0, 35.3, 36.4)              # a burst slower than the trace prices the line
    assert us == 38.0 and label == 'live HIP events of this run'
    us, label = bench.price_launch_us(31.1, 62.3, 36.4)              # host-paced pairs never beat a matching trace
    assert us == 36.4
    us, label = bench.price_launch_us(12.2, 34.7, None)              # no trace of the running sources: the in-step upper bound
    assert us == 34.7 and 'no trace' in label
    us, label = bench.price_launch_us(40.0, 34.7, None)
    assert us == 40.0 and label == 'live HIP events of this run'
    assert bench.price_launch_us(31.1, 35.3, 0.0)[0] == 35.3         # (in_graph_us() reports a stale trace as None / nothing)


def test_bench_full_is_an_option_and_the_variants_run_with_it(monkeypatch):
    """A plain bench.py run measures the headline only; `--full` adds the rest.  The variants copy eager_value from their own line,
    so their processes run with --full (and without variants or CPU baseline of their own)."""
    import importlib.util
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--help'], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and '--full' in out.stdout
    spec = importlib.util.spec_from_file_location('bench_for_variants', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    seen = []

    def fake_run(cmd, **kw):
        seen.append(cmd)
        return subprocess.CompletedProcess(cmd, 0, stdout=json.dumps({'metric': 'm', 'value': 1.0, 'eager_value': 0.5}) + '\n', stderr='')
    monkeypatch.setattr(subprocess, 'run', fake_run)
    v = bench.run_variant('cfg2', ['--reference-composition'])
    assert v['eager_value'] == 0.5
    assert {'--full', '--no-variants', '--no-cpu-baseline', '--reference-composition'} <= set(seen[0])


def test_trace_overlap_reports_what_ran_next_to_a_kernel(tmp_path):
    """tools/trace_overlap.py (the evidence of profiles/ab/r05i): per launch of the named kernel its duration, whether anything else
    was on the chip, and the time each other kernel shared with it."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    rows = ['Kernel_Name,Start_Timestamp,End_Timestamp']
    t = 0
    for step in range(3):
        base = step * 5_000_000
        rows.append(f'"void pvcnn::fps_kernel<512, 16, true>(float const*)",{base},{base + 900_000}')          # 900 us chain
        rows.append(f'"void pvcnn::conv3d_igemm(float const*)",{base + 100_000},{base + 400_000}')               # 300 us inside it
        rows.append(f'"pvcnn::bn_finalize_kernel(int)",{base + 800_000},{base + 1_000_000}')                      # 100 us of its 200 inside
        rows.append(f'"pvcnn::later_kernel(int)",{base + 2_000_000},{base + 2_100_000}')                          # not next to it
    rows.append(f'"void pvcnn::fps_kernel<512, 16, true>(float const*)",{20_000_000},{20_880_000}')               # one launch alone
    trace = tmp_path / 'kernel_trace.csv'
    trace.write_text('\n'.join(rows) + '\n')
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'trace_overlap.py'), str(trace), 'fps_kernel<512', '10'],
                         capture_output=True, text=True, check=True).stdout
    head = out.splitlines()[0]
    assert '4 launches' in head and '1 ran with nothing else on the chip' in head, head
    assert 'median 900.0 us (min 880.0, max 900.0)' in head, head
    body = '\n'.join(out.splitlines()[1:])
    assert '225.0 us per launch next to  void pvcnn::conv3d_igemm' in body, body           # 3 x 300 us over 4 launches
    assert '75.0 us per launch next to  pvcnn::bn_finalize_kernel' in body, body            # 3 x 100 us over 4 launches
    assert 'later_kernel' not in body
