"""Evaluation on the device (csrc/evaluate.hip, pvcnn_amd.evaluate, pvcnn_amd.meters) against tests/golden/eval_votes.pt -- the
reference's own eval loops and meters -- and against restatements of the reference inside this file.  Reads nothing outside the
repository."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, SEED

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'eval_votes.pt')


@pytest.fixture(scope='module')
def golden():
    return torch.load(GOLDEN, weights_only=False)


def _votes_for_s3dis_case(case):
    from pvcnn_amd.evaluate import SceneVotes
    votes = SceneVotes(case['confidences'].numel(), DEV)
    mapping = case['mapping'].to(DEV)
    for call in case['calls']:
        lo = call['min_window_index']
        votes.add(call['conf'].to(DEV), call['pred'].to(DEV, torch.int32), call['shuffled'].to(DEV), mapping[lo:])
    return votes


def test_tile_is_bit_exact():
    from pvcnn_amd.evaluate import s3dis_shuffled_indices, shapenet_shuffled_indices
    from pvcnn_amd.modules.functional.backend import _backend as be
    rng = np.random.RandomState(3)
    w, maxpts, c, npts = 3, 50, 9, 16
    data = rng.randn(w, maxpts, c).astype(np.float32)
    snp = np.array([50, 31, 7])
    extra = math.ceil(maxpts / npts)
    idx = s3dis_shuffled_indices(snp, 0, w, extra * npts, rng)
    got = be.eval_tile(torch.from_numpy(data).to(DEV), torch.from_numpy(idx).to(DEV), npts, c, (maxpts * c, c, 1), maxpts).cpu().numpy()
    want = np.stack([data[r][idx[r]] for r in range(w)]).reshape(w * extra, npts, c).transpose(0, 2, 1)
    assert got.tobytes() == np.ascontiguousarray(want).tobytes()
    # channels-first point set of ShapeNet: point_set[:, shuffled].reshape(-1, E, np).transpose(1, 0, 2)
    pset = rng.randn(22, 70).astype(np.float32)
    sidx = shapenet_shuffled_indices(70, 3 * 32, rng)
    got = be.eval_tile(torch.from_numpy(pset).to(DEV), torch.from_numpy(sidx).to(DEV).view(1, -1), 32, 22, (0, 1, 70), 70).cpu().numpy()
    want = pset[:, sidx].reshape(-1, 3, 32).transpose(1, 0, 2)
    assert got.tobytes() == np.ascontiguousarray(want).tobytes()


def _check_confidence(x, c0, c1, conf, pred):
    p = F.softmax(x, 1)[:, c0:c1]
    wc, wp = p.max(1)
    assert torch.allclose(conf, wc, rtol=1e-6, atol=0)
    top2 = p.topk(2, dim=1).values if c1 - c0 > 1 else None
    if top2 is not None:
        distinct = (top2[:, 0] - top2[:, 1]) > 1e-6 * top2[:, 0]
        assert torch.equal(pred.long()[distinct], (wp + c0)[distinct])
    assert ((pred >= c0) & (pred < c1)).all()


def test_vote_confidence_matches_torch_softmax_max():
    from pvcnn_amd.evaluate import vote_confidence
    g = torch.Generator().manual_seed(SEED)
    x = (torch.randn(4, 13, 300, generator=g) * 4).to(DEV)
    conf, pred = vote_confidence(x)
    _check_confidence(x, 0, 13, conf, pred)
    conf, pred = vote_confidence(x, (3, 9))
    _check_confidence(x, 3, 9, conf, pred)
    table = torch.tensor([[0, 4], [4, 6], [6, 13], [2, 3]], dtype=torch.int32, device=DEV)
    conf, pred = vote_confidence(x, table)
    for b, (s, e) in enumerate(table.tolist()):
        _check_confidence(x[b:b + 1], s, e, conf[b:b + 1], pred[b:b + 1])
    # exactly tied logits: the lowest class wins
    t = torch.zeros(2, 5, 64, device=DEV)
    t[:, 1] = 2.0
    t[:, 3] = 2.0
    conf, pred = vote_confidence(t)
    assert (pred == 1).all()
    conf, pred = vote_confidence(t, (2, 5))
    assert (pred == 3).all()


def test_merge_and_stats_equal_the_reference(golden):
    from pvcnn_amd.evaluate import s3dis_scene_stats
    for case in golden['s3dis']:
        votes = _votes_for_s3dis_case(case)
        assert torch.equal(votes.predictions().cpu(), case['predictions'])
        assert votes.confidences().cpu().numpy().tobytes() == case['confidences'].numpy().tobytes()
        again = _votes_for_s3dis_case(case)                                        # repeat-run identical
        assert torch.equal(again.predictions(), votes.predictions()) and torch.equal(again.confidences(), votes.confidences())
        assert not votes._keys.any()                                               # the workspace is left zero
        stats = np.zeros((3, case['num_classes'], 2))
        s3dis_scene_stats(stats, case['ground_truth'].numpy(), votes, 1)
        assert np.array_equal(stats, case['stats'].numpy())


def test_shape_merge_and_stats_equal_the_reference(golden):
    from pvcnn_amd.evaluate import ShapeVotes, shapenet_shape_stats
    for case in golden['shapenet']:
        votes = ShapeVotes(case['confidences'].numel(), DEV, case['start_class'], case['end_class'])
        for call in case['calls']:
            votes.add(call['conf'].to(DEV), call['pred'].to(DEV, torch.int32), call['shuffled'].to(DEV))
        assert torch.equal(votes.predictions().cpu(), case['predictions'])
        assert votes.confidences().cpu().numpy().tobytes() == case['confidences'].numpy().tobytes()
        stats = np.zeros((4, 2))
        shapenet_shape_stats(stats, case['ground_truth'].numpy(), votes, 2, case['start_class'], case['end_class'])
        assert np.array_equal(stats, case['stats'].numpy())


def test_seg_counts_keep_the_unvoted_quirk():
    from pvcnn_amd.modules.functional.backend import _backend as be
    gt = torch.tensor([0, 1, 2, 2, 1], dtype=torch.int64, device=DEV)
    pd = torch.tensor([0, -1, 2, -1, 2], dtype=torch.int64, device=DEV)
    assert be.seg_counts(gt, pd, 3).tolist() == [[1, 2, 2], [1, 0, 4], [1, 0, 1]]           # -1 -> a positive of class C-1
    assert be.seg_counts(gt, pd, 3, wrap_negative=False).tolist() == [[1, 2, 2], [1, 0, 2], [1, 0, 1]]


def test_meters_equal_the_reference(golden):
    from pvcnn_amd.meters import MeterS3DIS, MeterShapeNet
    g = golden['meter_s3dis']
    for metric, want in g['results'].items():
        m = MeterS3DIS(metric, g['num_classes'])
        for batch in g['batches']:
            m.update(batch['outputs'].to(DEV), batch['targets'].to(DEV))
        assert m.counts() == g['counts']
        assert m.compute() == want, metric
    m = MeterShapeNet()
    for batch in golden['meter_shapenet']['batches']:
        m.update(batch['outputs'].to(DEV), batch['targets'].to(DEV))
    assert m.compute() == golden['meter_shapenet']['result']
    m.reset()
    batch = golden['meter_shapenet']['batches'][0]
    m.update(batch['outputs'].to(DEV), batch['targets'].to(DEV))
    assert len(m.rows()) == batch['outputs'].shape[0]


def _capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    return graph


def test_update_and_add_capture_into_a_graph(golden):
    from pvcnn_amd.meters import MeterS3DIS, MeterShapeNet
    g = golden['meter_s3dis']
    x, t = g['batches'][0]['outputs'].to(DEV), g['batches'][0]['targets'].to(DEV)
    eager, captured = MeterS3DIS('iou', g['num_classes']), MeterS3DIS('iou', g['num_classes'])
    captured.update(x, t)                                           # allocates the device counts
    captured.reset()
    graph = _capture(lambda: captured.update(x, t))
    captured.reset()
    for _ in range(3):
        graph.replay()
        eager.update(x, t)
    assert captured.counts() == eager.counts() and captured.compute() == eager.compute()

    b = golden['meter_shapenet']['batches'][0]
    xs, ts = b['outputs'].to(DEV), b['targets'].to(DEV)
    eager, captured = MeterShapeNet(), MeterShapeNet()
    captured.reserve(3 * xs.shape[0], DEV)
    graph = _capture(lambda: captured.update(xs, ts))
    captured.reset()
    for _ in range(3):
        graph.replay()
        eager.update(xs, ts)
    assert captured.rows() == eager.rows() and captured.compute() == eager.compute()

    case = golden['s3dis'][0]
    from pvcnn_amd.evaluate import SceneVotes
    votes = SceneVotes(case['confidences'].numel(), DEV)
    mapping = case['mapping'].to(DEV)
    calls = [(c['conf'].to(DEV), c['pred'].to(DEV, torch.int32), c['shuffled'].to(DEV), mapping[c['min_window_index']:])
             for c in case['calls']]
    graph = _capture(lambda: [votes.add(*c) for c in calls])
    graph.replay()
    graph.replay()                                                  # the same votes again: nothing is strictly greater
    assert torch.equal(votes.predictions().cpu(), case['predictions'])
    assert votes.confidences().cpu().numpy().tobytes() == case['confidences'].numpy().tobytes()


def test_s3dis_file_votes_end_to_end():
    """s3dis_file_votes with a small eval-mode PVCNN against a numpy restatement of the reference loop (eval.py:139-180, 184-213) fed
    by the same model's torch-softmax outputs."""
    from pvcnn_amd.evaluate import SceneVotes, s3dis_file_votes, s3dis_scene_stats
    from pvcnn_amd.workload import PVCNN
    torch.manual_seed(SEED)
    model = PVCNN(num_classes=13, extra_feature_channels=6, width_multiplier=0.125).to(DEV).eval()
    rng = np.random.RandomState(SEED)
    w, maxpts, c, npts, bsz, scene_points, num_votes = 5, 700, 9, 512, 2, 2000, 1
    scene_data = rng.rand(w, maxpts, c).astype(np.float32) * np.array([1.5, 1.5, 3.0] + [1.0] * 6, dtype=np.float32)
    scene_num_points = rng.randint(300, maxpts + 1, size=w).astype(np.int64)
    mapping = rng.randint(0, scene_points - 100, size=(w, maxpts)).astype(np.int64)
    gt = rng.randint(0, 13, size=scene_points).astype(np.int64)

    votes = SceneVotes(scene_points, DEV)
    s3dis_file_votes(model, scene_data, scene_num_points, mapping, votes, num_points=npts, num_votes=num_votes, batch_size=bsz,
                     rng=np.random.RandomState(11))
    stats = np.zeros((3, 13, 1))
    s3dis_scene_stats(stats, gt, votes, 0)

    # the reference's loop, restated (numba loops as numpy/python), same RNG stream
    r = np.random.RandomState(11)
    conf = np.zeros(scene_points, dtype=np.float32)
    pred = np.full(scene_points, -1, dtype=np.int64)
    extra = num_votes * math.ceil(maxpts / npts)
    V = extra * npts
    for lo in range(0, w, bsz):
        hi = min(lo + bsz, w)
        bs = hi - lo
        window_data = scene_data[np.arange(lo, hi)].reshape(bs, -1, c)
        inputs = np.zeros((bs, V, c), dtype=np.float32)
        shuffled = np.zeros((bs, V), dtype=np.int64)
        for k in range(bs):
            n = scene_num_points[k + lo]
            idx = np.tile(np.arange(n), math.ceil(V / n))[:V]
            r.shuffle(idx)
            shuffled[k] = idx
            inputs[k] = window_data[k][idx]
        x = torch.from_numpy(inputs.reshape((bs * extra, npts, -1)).transpose(0, 2, 1)).float().to(DEV)
        with torch.no_grad():
            bc, bp = F.softmax(model(x), dim=1).max(dim=1)
        bc, bp = bc.view(bs, V).cpu().numpy(), bp.view(bs, V).cpu().numpy()
        for b in range(bs):
            for p in range(V):
                t = mapping[lo + b][shuffled[b, p]]
                if bc[b, p] > conf[t]:
                    conf[t] = bc[b, p]
                    pred[t] = bp[b, p]
    want = np.zeros((3, 13, 1))
    for p in range(scene_points):
        want[0, gt[p], 0] += 1
        want[1, pred[p], 0] += 1
        if gt[p] == pred[p]:
            want[2, gt[p], 0] += 1
    assert (pred == -1).any()
    assert np.array_equal(votes.predictions().cpu().numpy(), pred)
    np.testing.assert_allclose(votes.confidences().cpu().numpy(), conf, rtol=1e-6, atol=0)
    assert np.array_equal(stats, want)
