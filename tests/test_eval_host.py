"""Host side of the device evaluation (pvcnn_amd.evaluate, pvcnn_amd.meters): the final arithmetic of the meters from integer counts,
and the index builder of s3dis_file_votes, against tests/golden/eval_votes.pt (written by gen_eval_golden.py from the reference's own
eval loops and meters).  Where the reference tree is mounted, random cases against the imported reference meters as well."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'eval_votes.pt')
REF = '/root/reference'


@pytest.fixture(scope='module')
def golden():
    return torch.load(GOLDEN, weights_only=False)


def shapenet_rows(table, outputs, targets, max_parts):
    """Per-cloud rows [(s, e), (intersection, union) ...] restated on the CPU from the reference meter's definitions."""
    rows = []
    for b in range(outputs.size(0)):
        s, e = table[int(targets[b, 0])]
        pred = torch.argmax(outputs[b, s:e, :], dim=0) + s
        row = [(s, e)]
        for i in range(s, e):
            it, ip = targets[b] == i, pred == i
            row.append((int((it & ip).sum()), int((it | ip).sum())))
        rows.append(row + [(0, 0)] * (max_parts + 1 - len(row)))
    return rows


def s3dis_counts(outputs, targets, c):
    pred = outputs.argmax(1)
    seen = [int((targets == i).sum()) for i in range(c)]
    pos = [int((pred == i).sum()) for i in range(c)]
    cor = [int(((targets == i) & (pred == i)).sum()) for i in range(c)]
    return seen, pos, cor, targets.numel(), int((targets == pred).sum())


def test_golden_loads(golden):
    assert {'s3dis', 'shapenet', 'meter_s3dis', 'meter_shapenet', 'shuffle'} <= set(golden)
    assert os.path.getsize(GOLDEN) < 1 << 20
    for case in golden['s3dis']:
        assert case['predictions'].dtype == torch.int64 and (case['predictions'] == -1).any()     # the unvoted-point quirk is covered


def test_s3dis_meter_arithmetic_is_the_references(golden):
    from pvcnn_amd.meters import s3dis_meter_value
    g = golden['meter_s3dis']
    c = g['num_classes']
    counts = [0] * (3 * c + 2)
    for batch in g['batches']:
        seen, pos, cor, numel, correct = s3dis_counts(batch['outputs'], batch['targets'], c)
        for i in range(c):
            counts[i] += seen[i]; counts[c + i] += pos[i]; counts[2 * c + i] += cor[i]
        counts[3 * c] += numel; counts[3 * c + 1] += correct
    assert counts == g['counts']
    for metric, want in g['results'].items():
        got = s3dis_meter_value(metric, c, counts)
        assert type(got) is float and got == want, (metric, got, want)


def test_shapenet_meter_arithmetic_is_the_references(golden):
    from pvcnn_amd.meters import MeterShapeNet, shapenet_meter_value
    m = MeterShapeNet()
    rows = []
    for batch in golden['meter_shapenet']['batches']:
        rows += shapenet_rows(m.part_class_to_shape_part_classes, batch['outputs'], batch['targets'], m.max_parts)
    assert any(u == 0 for row in rows for (_, u) in row[1:1 + row[0][1] - row[0][0]])      # union 0 -> IoU 1 is exercised
    assert shapenet_meter_value(rows) == golden['meter_shapenet']['result']


def test_shapenet_stats_arithmetic_is_the_references(golden):
    from pvcnn_amd.evaluate import shapenet_iou
    for case in golden['shapenet']:
        gt, pd, s, e = case['ground_truth'], case['predictions'], case['start_class'], case['end_class']
        counts = [[int((gt == i).sum()) for i in range(e)], [int((pd == i).sum()) for i in range(e)],
                  [int(((gt == i) & (pd == i)).sum()) for i in range(e)]]
        assert shapenet_iou(counts, s, e) == case['stats'][2, 0].item()


def test_index_builder_consumes_the_rng_like_the_reference(golden):
    from pvcnn_amd.evaluate import s3dis_shuffled_indices
    g = golden['shuffle']
    rng = np.random.RandomState(g['seed'])
    got = s3dis_shuffled_indices(g['scene_num_points'].numpy(), 0, len(g['scene_num_points']), g['V'], rng)
    assert got.dtype == np.int64 and np.array_equal(got, g['indices'].numpy())
    assert rng.random_sample() == g['next_draw']
    # batched the way s3dis_file_votes' caller would see it: the same arrays, window by window
    rng = np.random.RandomState(g['seed'])
    parts = [s3dis_shuffled_indices(g['scene_num_points'].numpy(), lo, min(lo + 3, 4), g['V'], rng) for lo in (0, 3)]
    assert np.array_equal(np.concatenate(parts), g['indices'].numpy())


@pytest.fixture(scope='module')
def ref_meters():
    if not os.path.isdir(os.path.join(REF, 'meters')):
        pytest.skip('reference tree not mounted')
    saved = {k: v for k, v in sys.modules.items() if k == 'meters' or k.startswith('meters.')}
    for k in saved:
        del sys.modules[k]
    sys.path.insert(0, REF)
    try:
        yield importlib.import_module('meters.s3dis').MeterS3DIS, importlib.import_module('meters.shapenet').MeterShapeNet
    finally:
        sys.path.remove(REF)
        for k in [k for k in sys.modules if k == 'meters' or k.startswith('meters.')]:
            del sys.modules[k]
        sys.modules.update(saved)


@pytest.mark.parametrize('seed', range(4))
def test_random_cases_against_the_reference_meters(ref_meters, seed):
    from pvcnn_amd.meters import MeterShapeNet, s3dis_meter_value, shapenet_meter_value
    RefS3DIS, RefShapeNet = ref_meters
    g = torch.Generator().manual_seed(seed)
    c = 13
    refs = {m: RefS3DIS(metric=m, num_classes=c) for m in ('overall', 'class', 'iou')}
    counts = [0] * (3 * c + 2)
    for _ in range(3):
        x = torch.randint(-2, 3, (2, c, 77), generator=g).float()
        t = torch.randint(0, c - 2, (2, 77), generator=g)
        for m in refs.values():
            m.update(x, t)
        seen, pos, cor, numel, correct = s3dis_counts(x, t, c)
        for i in range(c):
            counts[i] += seen[i]; counts[c + i] += pos[i]; counts[2 * c + i] += cor[i]
        counts[3 * c] += numel; counts[3 * c + 1] += correct
    for metric, m in refs.items():
        assert s3dis_meter_value(metric, c, counts) == m.compute()
    ref, ours = RefShapeNet(), MeterShapeNet()
    assert ours.part_class_to_shape_part_classes == ref.part_class_to_shape_part_classes
    rows = []
    for _ in range(2):
        t = torch.stack([torch.randint(*ours.part_class_to_shape_part_classes[int(k)], (40,), generator=g)
                         for k in torch.randint(0, 50, (3,), generator=g)])
        x = torch.randint(-2, 3, (3, 50, 40), generator=g).float()
        ref.update(x, t)
        rows += shapenet_rows(ours.part_class_to_shape_part_classes, x, t, ours.max_parts)
    assert shapenet_meter_value(rows) == ref.compute()
