"""Pin the CPU oracle against the REFERENCE'S OWN KERNELS executed on the CPU.

oracle/_ref/libpvcnn_ref_cpu.so is built by oracle/build_ref.py from the reference's .cu files where
they lie (/root/reference/modules/functional/src/**), through a CUDA-execution-model shim
(oracle/ref_shim/cuda_on_cpu.h: one fiber per CUDA thread, real __syncthreads(), real launch
shapes from the reference's own optimal_num_threads / optimal_block_config).  This is the
reference itself, not a restatement: if the oracle agrees with it, the HIP path's bit-exact
agreement with the oracle (tests/test_gpu_parity.py) is agreement with the reference.

What is compared how:
  * everything deterministic in the reference (indices, counts, weights, gathers, interpolation,
    ball_query, FPS incl. its launch-shape-dependent tie rule, voxelize backward) : bit-exact;
  * atomicAdd accumulations (voxelize fwd, devoxelize bwd, grouping/gather bwd, 3-NN bwd): the
    shim runs threads in ascending threadIdx order, a legal CUDA schedule.  The reference launches
    optimal_num_threads(n) = 2^floor(log2 n) <= 512 threads (cuda_utils.cuh:13-18); when n is a power
    of two <= 512 every thread owns exactly one point and that schedule IS point order, so the
    comparison is bit-exact; otherwise the schedule visits points as (i mod threads, i) and the
    comparison is to 1e-5 -- which also shows the reference's result is only defined up to
    summation order.
Where oracle/_ref was not built (no reference tree at build time) the reference side is its recorded outputs for exactly
these calls (tests/golden/ref_kernels.pt.xz, written by tests/golden/gen_golden.py from the built reference; each stored as
its bitwise difference from the oracle's output on the call plus a digest that makes the rebuilt value exact): the oracle is
then checked against what the reference computed on the same inputs.
"""
import os

import pytest
import torch

from conftest import grid_coords, synth_cloud

from oracle import ref_backend

RECORDED = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_kernels.pt.xz')
RECORD_TO = os.environ.get('PVCNN_RECORD_REF')        # set by tests/golden/gen_golden.py: record the live reference's outputs there
_recording = {}


def _reference(variant, oracle):
    if RECORD_TO:
        return ref_backend.RecordedRefBackend(_recording, oracle, variant, live=ref_backend.RefCpuBackend(variant))
    if ref_backend.available(variant):
        return ref_backend.RefCpuBackend(variant)
    return ref_backend.RecordedRefBackend(ref_backend.load_recording(RECORDED), oracle, variant)


@pytest.fixture(scope='module')
def ref(oracle):
    yield _reference('fma', oracle)
    if RECORD_TO:
        ref_backend.save_recording(_recording, RECORD_TO)


@pytest.fixture(scope='module')
def ref_nofma(oracle):
    yield _reference('nofma', oracle)
    if RECORD_TO:
        ref_backend.save_recording(_recording, RECORD_TO)


def _vox(gen, b, c, n, r):
    feat = torch.randn(b, c, n, generator=gen)
    vox = torch.randint(0, r, (b, 3, n), generator=gen, dtype=torch.int32)
    vox[:, :, : n // 4] = vox[:, :, n // 4: 2 * (n // 4)]       # guaranteed multi-point voxels
    return feat, vox.contiguous()


@pytest.mark.parametrize('b,c,n,r', [(2, 5, 256, 8), (1, 3, 32, 5), (2, 4, 512, 12)])
def test_avg_voxelize_bit_exact_small(oracle, ref, gen, b, c, n, r):
    feat, vox = _vox(gen, b, c, n, r)
    o, rf = oracle.avg_voxelize_forward(feat, vox, r), ref.avg_voxelize_forward(feat, vox, r)
    for a, e in zip(o, rf):
        assert torch.equal(a, e)
    gy = torch.randn(b, c, r ** 3, generator=gen)
    assert torch.equal(oracle.avg_voxelize_backward(gy, o[1], o[2]), ref.avg_voxelize_backward(gy, rf[1], rf[2]))


def test_avg_voxelize_large_n_order_only(oracle, ref, gen):
    b, c, n, r = 2, 6, 3000, 10      # threads own points i, i+512, ...: a different (legal) atomic order
    feat, vox = _vox(gen, b, c, n, r)
    o, rf = oracle.avg_voxelize_forward(feat, vox, r), ref.avg_voxelize_forward(feat, vox, r)
    assert torch.equal(o[1], rf[1]) and torch.equal(o[2], rf[2])
    assert torch.allclose(o[0], rf[0], atol=1e-5, rtol=1e-5)
    truth = oracle.avg_voxelize_forward_f64(feat, o[1], o[2])
    assert (o[0].double() - truth).abs().max() < 1e-5 and (rf[0].double() - truth).abs().max() < 1e-5


@pytest.mark.parametrize('b,c,n,r', [(2, 5, 500, 8), (1, 3, 37, 5), (2, 4, 3000, 12), (1, 2, 700, 32)])
@pytest.mark.parametrize('training', [True, False])
def test_trilinear_devox_fwd_bit_exact(oracle, ref, gen, b, c, n, r, training):
    feat = torch.randn(b, c, r ** 3, generator=gen)
    co = grid_coords(gen, b, n, r)
    o, rf = oracle.trilinear_devoxelize_forward(r, training, co, feat), ref.trilinear_devoxelize_forward(r, training, co, feat)
    for a, e in zip(o, rf):
        assert torch.equal(a, e)


@pytest.mark.parametrize('b,c,n,r,exact', [(2, 5, 512, 8, True), (1, 3, 32, 5, True), (2, 4, 3000, 12, False), (1, 3, 500, 6, False)])
def test_trilinear_devox_bwd(oracle, ref, gen, b, c, n, r, exact):
    co = grid_coords(gen, b, n, r)
    _, inds, wgts = oracle.trilinear_devoxelize_forward(r, True, co, torch.zeros(b, 1, r ** 3))
    gy = torch.randn(b, c, n, generator=gen)
    o, rf = oracle.trilinear_devoxelize_backward(gy, inds, wgts, r), ref.trilinear_devoxelize_backward(gy, inds, wgts, r)
    if exact:
        assert torch.equal(o, rf)
    else:
        assert torch.allclose(o, rf, atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize('b,n,m,radius,u', [(2, 2000, 300, 0.2, 32), (1, 700, 77, 0.3, 5), (2, 64, 16, 0.8, 32), (1, 130, 9, 10.0, 70)])
def test_ball_query_bit_exact(oracle, ref, gen, b, n, m, radius, u):
    pts = synth_cloud(gen, b, n, 's3dis')
    ctr = pts[:, :, torch.randperm(n, generator=gen)[:m]].contiguous()
    assert torch.equal(oracle.ball_query(ctr, pts, radius, u), ref.ball_query(ctr, pts, radius, u))


@pytest.mark.parametrize('b,c,n,m,u,exact', [(2, 4, 300, 32, 8, True), (1, 3, 2000, 600, 16, False)])
def test_grouping_gather(oracle, ref, gen, b, c, n, m, u, exact):
    f = torch.randn(b, c, n, generator=gen)
    idx = torch.randint(0, n, (b, m, u), generator=gen, dtype=torch.int32)
    assert torch.equal(oracle.grouping_forward(f, idx), ref.grouping_forward(f, idx))
    g = torch.randn(b, c, m, u, generator=gen)
    o, rf = oracle.grouping_backward(g, idx, n), ref.grouping_backward(g, idx, n)
    # one (channel, centre) pair per thread when c*m <= blockDim (optimal_block_config): exact; else tolerance
    assert torch.equal(o, rf) if exact else torch.allclose(o, rf, atol=1e-5, rtol=1e-5)
    gi = torch.randint(0, n, (b, m), generator=gen, dtype=torch.int32)
    assert torch.equal(oracle.gather_features_forward(f, gi), ref.gather_features_forward(f, gi))
    gg = torch.randn(b, c, m, generator=gen)
    o, rf = oracle.gather_features_backward(gg, gi, n), ref.gather_features_backward(gg, gi, n)
    assert torch.equal(o, rf) if exact else torch.allclose(o, rf, atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize('b,n,m', [(2, 2000, 128), (1, 700, 60), (2, 64, 16), (1, 17, 17), (1, 3500, 40)])
def test_fps_bit_exact(oracle, ref, gen, b, n, m):
    pts = synth_cloud(gen, b, n, 's3dis')      # 5 % exact duplicates -> ties at distance 0
    assert torch.equal(oracle.furthest_point_sampling(pts, m), ref.furthest_point_sampling(pts, m))


def test_fps_tie_rule_is_the_references(oracle, ref):
    # integer lattice with N > 512: the winner among equidistant points is decided by the reference's
    # 512-slot strided scan + left-biased tree, which the oracle restates as min (k mod 512, k)
    g = torch.arange(9, dtype=torch.float32)
    pts = torch.stack(torch.meshgrid(g, g, g, indexing='ij')).reshape(1, 3, -1).contiguous()   # N = 729
    assert torch.equal(oracle.furthest_point_sampling(pts, 60), ref.furthest_point_sampling(pts, 60))


@pytest.mark.parametrize('b,c,m,n,exact', [(2, 4, 40, 64, True), (1, 2, 2, 32, True), (1, 3, 1, 16, True), (2, 5, 200, 2500, False)])
def test_three_nn_interpolate(oracle, ref, gen, b, c, m, n, exact):
    pts = synth_cloud(gen, b, n, 's3dis')
    ctr = pts[:, :, torch.randperm(n, generator=gen)[:m]].contiguous()
    feats = torch.randn(b, c, m, generator=gen)
    o, rf = (oracle.three_nearest_neighbors_interpolate_forward(pts, ctr, feats),
             ref.three_nearest_neighbors_interpolate_forward(pts, ctr, feats))
    for a, e in zip(o, rf):
        assert torch.equal(a, e)
    g = torch.randn(b, c, n, generator=gen)
    ob, rb = (oracle.three_nearest_neighbors_interpolate_backward(g, o[1], o[2], m),
              ref.three_nearest_neighbors_interpolate_backward(g, rf[1], rf[2], m))
    assert torch.equal(ob, rb) if exact else torch.allclose(ob, rb, atol=1e-5, rtol=1e-5)


def test_contraction_sensitivity_is_reported(oracle, ref, ref_nofma, gen):
    """How much hangs on nvcc's fma contraction (which the oracle pins with fmaf)?  The same reference
    source built WITHOUT contraction differs from the contracted build only in the last bits of the
    interpolation sums; index / weight outputs have no mul+add to contract and are identical."""
    b, c, n, r = 2, 4, 600, 8
    feat = torch.randn(b, c, r ** 3, generator=gen)
    co = grid_coords(gen, b, n, r)
    a = ref.trilinear_devoxelize_forward(r, True, co, feat)
    z = ref_nofma.trilinear_devoxelize_forward(r, True, co, feat)
    assert torch.equal(a[1], z[1]) and torch.equal(a[2], z[2])
    assert (a[0] - z[0]).abs().max() < 1e-5 and not torch.equal(a[0], z[0])
    assert torch.equal(oracle.trilinear_devoxelize_forward(r, True, co, feat)[0], a[0])   # oracle == contracted build
    pts = synth_cloud(gen, 1, 500, 's3dis')
    ctr = pts[:, :, :40].contiguous()
    assert torch.equal(ref.ball_query(ctr, pts, 0.2, 16), ref_nofma.ball_query(ctr, pts, 0.2, 16))


def test_contraction_exposure_of_the_index_ops_is_bounded(ref, ref_nofma):
    """ASSUMPTION, stated as such: oracle/_ref is the reference source AS CONTRACTED BY GCC
    (-ffp-contract=fast).  Whether nvcc's NVVM fuses the same products cannot be checked here (no nvcc).  What can be
    bounded is the exposure: the same source built with and without contraction brackets nvcc's choice (any other
    association of fused / unfused products lies between), so the index-producing ops -- ball_query (d^2 < r^2),
    furthest point sampling (arg-max of squared distances) and 3-NN (three smallest squared distances) -- are swept
    over both builds on S3DIS-like clouds at the PVCNN++ level sizes and the number of differing indices is REPORTED.
    The test fails only if the two builds stop agreeing on essentially everything (which would mean index parity hangs
    on the compiler): a d^2 within one ulp of r^2, or two candidates within one ulp of each other, is the only way a
    contraction choice can flip an index."""
    g = torch.Generator().manual_seed(20240924)
    total = {'ball_query': [0, 0], 'fps': [0, 0], 'three_nn': [0, 0]}
    for (n, m, radius) in [(8192, 1024, 0.1), (1024, 256, 0.2), (256, 64, 0.4), (64, 16, 0.8)]:      # cfg3 levels
        pts = synth_cloud(g, 2, n, 's3dis')
        f_a, f_z = ref.furthest_point_sampling(pts, m), ref_nofma.furthest_point_sampling(pts, m)
        total['fps'][0] += (f_a != f_z).sum().item(); total['fps'][1] += f_a.numel()
        ctr = torch.gather(pts, 2, f_a.long().unsqueeze(1).expand(-1, 3, -1)).contiguous()
        b_a, b_z = ref.ball_query(ctr, pts, radius, 32), ref_nofma.ball_query(ctr, pts, radius, 32)
        total['ball_query'][0] += (b_a != b_z).sum().item(); total['ball_query'][1] += b_a.numel()
        feats = torch.randn(2, 4, m, generator=g)
        t_a = ref.three_nearest_neighbors_interpolate_forward(pts, ctr, feats)
        t_z = ref_nofma.three_nearest_neighbors_interpolate_forward(pts, ctr, feats)
        total['three_nn'][0] += (t_a[1] != t_z[1]).sum().item(); total['three_nn'][1] += t_a[1].numel()
    for op, (diff, count) in total.items():
        print(f'[contraction exposure] {op}: {diff} of {count} indices differ between the fma and the no-fma build of the reference source')
        assert diff <= max(2, count // 10000), (op, diff, count)
