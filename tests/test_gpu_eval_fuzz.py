"""The evaluation kernels (csrc/evaluate.hip) at real sizes against the plain references of tests/eval_truth.py: every grid-stride
loop strides at least twice (grids are capped at 8192, or 1024 for the histograms, workgroups of 256 threads), many workgroups flush
into one table, and every contract clause written in the kernels' comments has a case that fails without its guard.  Integer
outputs and merged confidences (copies of inputs) are bit-exact.  Seeded; reads nothing outside the repository.

Every case that feeds an out-of-range index, row or id hands the kernel a VIEW into a larger allocation filled with a sentinel: a
missing guard shows as a wrong value or a changed sentinel, never as an access outside the allocation."""
import numpy as np
import pytest
import torch

import eval_truth as T
import fuzz_cases as F

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
THREADS, GRID_CAP, HIST_GRID_CAP = 256, 8192, 1024
PAD = 64
LEVELS = np.array([0.0, -0.0, -0.25, np.nan, 1e-40, np.inf, 0.125, 0.25, 0.5, 0.75, 1.0, 0.5, 0.25], dtype=np.float32)


def _be():
    from pvcnn_amd.modules.functional.backend import _backend
    return _backend


def _padded(shape, dtype, sentinel, pad=PAD):
    """-> (view of `shape`, the whole allocation): the view sits `pad` elements inside a sentinel-filled buffer."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * pad,), sentinel, dtype=dtype, device=DEV)
    return whole[pad:pad + n].view(shape), whole


def _pads_intact(whole, sentinel, pad=PAD):
    edge = torch.cat([whole[:pad], whole[-pad:]])
    return bool((edge == sentinel).all())


class _Votes:
    """SceneVotes whose three state arrays are views inside sentinel-padded allocations."""

    def __init__(self, num_points):
        from pvcnn_amd.evaluate import SceneVotes
        self.votes = SceneVotes(num_points, DEV)
        self.votes._conf, self.conf_all = _padded((num_points,), torch.float32, -7.0)
        self.votes._pred, self.pred_all = _padded((num_points,), torch.int64, -77)
        self.votes._keys, self.keys_all = _padded((num_points,), torch.int64, 0)
        self.votes._conf.zero_()
        self.votes._pred.fill_(-1)
        self.conf = np.zeros(num_points, dtype=np.float32)
        self.pred = np.full(num_points, -1, dtype=np.int64)

    def add(self, conf, pred, shuffled, mapping=None, mapping_dev=None):
        self.votes.add(torch.from_numpy(conf).to(DEV), torch.from_numpy(pred).to(DEV), torch.from_numpy(shuffled).to(DEV), mapping_dev)
        T.merge_vectorised(self.conf, self.pred, conf, pred, shuffled, mapping)
        assert not self.keys_all.any()                                                   # the workspace (and its pads) is all zero
        assert _pads_intact(self.conf_all, -7.0) and _pads_intact(self.pred_all, -77)

    def check(self):
        assert self.votes.confidences().cpu().numpy().tobytes() == self.conf.tobytes()
        assert np.array_equal(self.votes.predictions().cpu().numpy(), self.pred)


def _vote_call(rng, b, v, hi, bad=1e-4):
    """One call's (conf, pred, shuffled): confidences from a handful of levels (0, -0.0, negative, NaN, a positive subnormal, +inf
    among them), indices in [0, hi) with a share of -1, hi and hi + 5."""
    conf = LEVELS[rng.integers(0, len(LEVELS), size=(b, v))]
    pred = rng.integers(0, 13, size=(b, v), dtype=np.int32)
    shuffled = rng.integers(0, hi, size=(b, v), dtype=np.int64)
    flat = shuffled.reshape(-1)
    where = rng.choice(flat.size, size=max(int(flat.size * bad), 3), replace=False)
    flat[where] = np.array([-1, hi, hi + 5], dtype=np.int64)[np.arange(where.size) % 3]
    return conf, pred, shuffled


BIG_B, BIG_V = 8, 786561                    # B * V = 6,292,488 >= 3 * 8192 * 256 = 6,291,456, and not a multiple of 256
POINTS = 1000003


def test_vote_sizes_cross_the_grid_cap():
    assert BIG_B * BIG_V >= 3 * GRID_CAP * THREADS and (BIG_B * BIG_V) % THREADS != 0


@pytest.mark.parametrize('with_mapping', [False, True])
def test_vote_merge_at_scale(with_mapping):
    """6.3 M votes in one call (every thread of the capped grid strides three times, the last stride ragged) onto ~1e6 points, then
    two smaller calls; confidences from 13 levels, so ties between distant votes decide most points (the 0xFFFFFFFF - g order word
    at g up to 6.3e6); dropped: conf 0, -0.0, negative, NaN; shuffled index -1 / M / M + 5; mapping target -1 / P / P + 7.  The
    guards read in the kernel: vote_target() tests idx against [0, map_stride) BEFORE mapping[] and t against [0, P) BEFORE keys[t];
    `!(c > 0.0f)` drops NaN."""
    def run():
        st = _Votes(POINTS)
        r = np.random.default_rng(17 + with_mapping)
        mapping = mapping_dev = None
        m = POINTS
        if with_mapping:
            m = 300007
            reserved = POINTS - 1                                                        # no vote targets it: the pads name it
            mapping = r.integers(0, POINTS - 1000, size=(BIG_B, m), dtype=np.int64)      # the last 1000 points are never voted
            flat = mapping.reshape(-1)
            where = r.choice(flat.size, size=600, replace=False)
            flat[where] = np.array([-1, POINTS, POINTS + 7], dtype=np.int64)[np.arange(600) % 3]
            whole = torch.full((BIG_B + 2, m), reserved, dtype=torch.int64, device=DEV)  # a missing index guard votes for `reserved`
            whole[1:BIG_B + 1] = torch.from_numpy(mapping).to(DEV)
            mapping_dev = whole[1:BIG_B + 1]
        for b, v in ((BIG_B, BIG_V), (3, 100001), (1, 255)):
            conf, pred, shuffled = _vote_call(r, b, v, m)
            st.add(conf, pred, shuffled, None if mapping is None else mapping[:b], None if mapping_dev is None else mapping_dev[:b])
        st.check()
        return st
    first = run()
    assert (first.pred == -1).any() and (first.pred >= 0).sum() > 800000
    if with_mapping:
        assert first.pred[-1] == -1 and first.conf[-1] == 0
    second = run()                                                                       # two runs are bit-identical
    assert torch.equal(first.votes.confidences().view(torch.int32), second.votes.confidences().view(torch.int32))
    assert torch.equal(first.votes.predictions(), second.votes.predictions())


def test_vote_merge_every_vote_on_one_target_and_a_repeated_call():
    """The 64-bit atomicMax under full contention: 6.3 M votes on ONE point (the first vote of the largest confidence wins, wherever
    it is), and a second call repeating the first changes nothing (strictly greater only)."""
    rng = np.random.default_rng(23)
    st = _Votes(1000)
    conf = LEVELS[rng.integers(0, len(LEVELS) - 1, size=(BIG_B, BIG_V))]
    conf[conf == np.inf] = 0.875                                                         # the maximum (1.0) is held by many votes
    pred = rng.integers(0, 13, size=(BIG_B, BIG_V), dtype=np.int32)
    shuffled = np.full((BIG_B, BIG_V), 421, dtype=np.int64)
    st.add(conf, pred, shuffled)
    st.check()
    first_one = int(np.flatnonzero(conf.reshape(-1) == 1.0)[0])
    assert st.pred[421] == pred.reshape(-1)[first_one] and st.conf[421] == 1.0 and (np.delete(st.pred, 421) == -1).all()
    before = (st.votes.confidences().clone(), st.votes.predictions().clone())
    pred2 = ((pred + 1) % 13).astype(np.int32)                                           # the same confidences, other classes
    st.add(conf, pred2, shuffled)
    st.check()
    assert torch.equal(before[0], st.votes.confidences()) and torch.equal(before[1], st.votes.predictions())
    # spread targets, the call repeated verbatim
    st = _Votes(50021)
    call = _vote_call(rng, 4, 300001, 50021)
    st.add(*call)
    before = (st.votes.confidences().clone(), st.votes.predictions().clone())
    st.add(*call)
    st.check()
    assert torch.equal(before[0].view(torch.int32), st.votes.confidences().view(torch.int32))
    assert torch.equal(before[1], st.votes.predictions())


@pytest.mark.parametrize('c', [1, 13, 50, 4096])
@pytest.mark.parametrize('wrap', [True, False])
def test_seg_counts_at_scale(c, wrap):
    """P = 800,003 > 3 * 1024 * 256: every thread of the 1024-workgroup grid strides three times and 1024 LDS histograms flush into
    one table.  Values in [0, C), [-C, 0), below -C and >= C in both wrap modes (class_slot() maps anything else to -1 and no
    counter is touched); accumulation into a non-zero table."""
    p = 800003
    assert p > 3 * HIST_GRID_CAP * THREADS
    rng = np.random.default_rng(31 + c)
    gt = rng.integers(-2 * c - 3, 2 * c + 3, size=p, dtype=np.int64)
    pd = np.where(rng.random(p) < 0.5, gt, rng.integers(-2 * c - 3, 2 * c + 3, size=p, dtype=np.int64))
    pd[::97] = -1                                                                        # the unvoted-point quirk
    counts, whole = _padded((3, c), torch.int64, -5)
    start = rng.integers(0, 1000, size=(3, c), dtype=np.int64)
    counts.copy_(torch.from_numpy(start))
    got = _be().seg_counts(torch.from_numpy(gt).to(DEV), torch.from_numpy(pd).to(DEV), c, counts=counts, wrap_negative=wrap)
    want = start + T.seg_counts_truth(gt, pd, c, wrap)
    assert np.array_equal(got.cpu().numpy(), want) and _pads_intact(whole, -5)
    assert want[1].sum() - start[1].sum() < p                                            # some values were counted nowhere


def _capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    return graph


def _meter_logits(rng, b, c, n):
    """A handful of values (many exact ties in a column) with a share of NaN."""
    x = (rng.integers(-3, 4, size=(b, c, n)) * 0.5).astype(np.float32)
    x[rng.random((b, c, n)) < 0.01] = np.nan
    return x


def test_seg_meter_s3dis_at_scale_and_graph_replay():
    """B * N = 540,024 > 2 * 1024 * 256: tied logits, NaN logits (a NaN wins the argmax), targets outside [0, C) (seen nowhere:
    `t >= 0 && t < C` guards the LDS histogram); numel (added by workgroup 0 only) and correct; a replayed graph adds exactly once
    per replay."""
    from pvcnn_amd.meters import MeterS3DIS
    b, c, n = 8, 13, 67503
    assert b * n > 2 * HIST_GRID_CAP * THREADS
    rng = np.random.default_rng(41)
    x = _meter_logits(rng, b, c, n)
    t = rng.integers(-3, c + 3, size=(b, n), dtype=np.int64)
    want = T.meter_s3dis_truth(x, t, c)
    assert want[3 * c] == b * n and 0 < want[3 * c + 1] < b * n and want[:c].sum() < b * n
    xd, td = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)
    m = MeterS3DIS('iou', c)
    m.update(xd, td)
    assert m.counts() == want.tolist()
    m.update(xd, td)
    assert m.counts() == (2 * want).tolist()
    m.reset()
    graph = _capture(lambda: m.update(xd, td))
    m.reset()
    for k in range(1, 4):
        graph.replay()
        assert m.counts() == (k * want).tolist()


@pytest.mark.parametrize('n', [1, 255, 256, 257, 2048, 5000])
def test_seg_meter_shapenet_rows(n):
    """One workgroup per cloud striding over N by 256.  Labels outside the table (the range table is a view between sentinel rows of a
    valid-looking (0, 2): `label >= 0 && label < nranges` is tested before ranges[] is read), table rows with s >= e, e > C and
    e - s > max_parts (all become (0, 0)), targets outside [s, e), NaN logits, a non-zero cursor, and a capacity that the last rows
    of the batch fall beyond (`r >= capacity` returns before the store: the rows behind the view keep their sentinel)."""
    c, max_parts, b = 50, 6, 23
    rng = np.random.default_rng(50 + n)
    table = [(0, 4), (4, 6), (6, 6), (9, 8), (44, 51), (10, 17), (10, 16), (47, 50), (-1, 3), (30, 36)]
    bad = {2, 3, 4, 5, 8}
    ranges_all = torch.tensor([(0, 2)] * 4 + table + [(0, 2)] * 4, dtype=torch.int32, device=DEV)
    ranges = ranges_all[4:4 + len(table)]
    x = _meter_logits(rng, b, c, n)
    labels = np.array([i % len(table) for i in range(b)], dtype=np.int64)
    labels[[11, 17, 21]] = [-1, len(table), len(table) + 3]                              # outside the table
    t = np.zeros((b, n), dtype=np.int64)
    for i in range(b):
        s, e = table[labels[i]] if 0 <= labels[i] < len(table) else (0, 4)
        t[i] = rng.integers(min(s, e) - 2, max(s, e) + 2, size=n)                        # some targets outside [s, e)
        t[i, 0] = labels[i]
    cursor_start, capacity = 5, 5 + b - 4                                                # the last 4 clouds fall beyond the capacity
    rows_all = torch.full((capacity + b, max_parts + 1, 2), -9, dtype=torch.int32, device=DEV)
    rows = rows_all[:capacity]
    cursor = torch.tensor([cursor_start], dtype=torch.int64, device=DEV)
    _be().seg_meter_update(torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV), part_ranges=ranges, max_parts=max_parts, rows=rows,
                           row_cursor=cursor)
    want = T.meter_shapenet_rows_truth(x, t, table, max_parts)
    for i in range(b):
        ok = 0 <= labels[i] < len(table) and labels[i] not in bad
        assert (tuple(want[i, 0]) != (0, 0)) == ok
    got = rows_all.cpu().numpy()
    assert (got[:cursor_start] == -9).all() and (got[capacity:] == -9).all()
    assert np.array_equal(got[cursor_start:capacity], want[:capacity - cursor_start])
    assert cursor.item() == cursor_start


def _check_confidence(x, lo, hi, conf, pred, label):
    """conf within the derived bound of the fp64 softmax; pred equal to the fp64 argmax wherever the top-two gap exceeds it.
    -> (worst ratio to the bound, excluded share)."""
    c = x.shape[1]
    truth = T.vote_confidence_truth(x, lo, hi)
    tol = T.confidence_rel_bound(c, truth['dist']) * truth['conf'] + T.FLT_MIN
    err = np.abs(conf.astype(np.float64) - truth['conf'])
    ratio = float((err / tol).max())
    excluded = T.confidence_excluded(truth, c)
    share = float(excluded.mean())
    print(f'vote_confidence {label}: worst |error| / bound {ratio:.3f}, excluded share {share:.4%}')
    assert np.isfinite(conf).all() and ratio <= 1.0
    assert share <= 0.01
    assert np.array_equal(pred[~excluded], truth['pred'][~excluded])
    empty = truth['pred'] < 0
    assert (pred[empty] == -1).all() and (conf[empty] == 0).all()
    inside = ~empty
    los = np.broadcast_to(np.maximum(np.asarray(lo), 0).reshape(-1, 1), pred.shape)
    his = np.broadcast_to(np.minimum(np.asarray(hi), c).reshape(-1, 1), pred.shape)
    assert ((pred >= los) & (pred < his))[inside].all()
    return ratio, share


def test_vote_confidence_at_scale():
    """B * N = 4,194,365 > 2 * 8192 * 256 with C = 13: logits N(0, 4^2), a block of +-80 with -inf entries; all classes, the fixed
    range (3, 9) and a per-cloud table with an empty row, a reversed row and over-wide rows (clamped to [0, C]; an empty range gives
    conf 0, pred -1).  The tolerance is derived (eval_truth.confidence_rel_bound), not measured.
    Measured on an MI355X: worst |error| / bound 0.258 (all classes), 0.402 (range (3, 9)), 0.399 (table); excluded share 0.0001 %,
    0.0034 %, 0.0222 %."""
    from pvcnn_amd.evaluate import vote_confidence
    b, c, n = 5, 13, 838873
    assert b * n > 2 * GRID_CAP * THREADS
    x = F.confidence_logits(61, b, c, n)
    xd = torch.from_numpy(x).to(DEV)
    conf, pred = vote_confidence(xd)
    _check_confidence(x, 0, c, conf.cpu().numpy(), pred.cpu().numpy(), 'C=13 all classes')
    conf, pred = vote_confidence(xd, (3, 9))
    _check_confidence(x, 3, 9, conf.cpu().numpy(), pred.cpu().numpy(), 'C=13 range (3, 9)')
    table = np.array([[0, 4], [7, 7], [9, 2], [-5, 40], [11, 99]], dtype=np.int32)
    conf, pred = vote_confidence(xd, torch.from_numpy(table).to(DEV))
    _check_confidence(x, table[:, 0], table[:, 1], conf.cpu().numpy(), pred.cpu().numpy(), 'C=13 per-cloud table')
    assert (pred[1] == -1).all() and (pred[2] == -1).all() and (conf[1] == 0).all()


@pytest.mark.parametrize('c,ranges', F.CONFIDENCE_SMALL_CASES)
def test_vote_confidence_small_class_counts(c, ranges):
    from pvcnn_amd.evaluate import vote_confidence
    b, n = 4, 20000
    x = F.confidence_logits(11 + c, b, c, n)
    xd = torch.from_numpy(x).to(DEV)
    for lo, hi in ranges:
        conf, pred = vote_confidence(xd, (lo, hi))
        _check_confidence(x, lo, hi, conf.cpu().numpy(), pred.cpu().numpy(), f'C={c} range ({lo}, {hi})')


def test_vote_confidence_exact_ties_go_to_the_lowest_class():
    from pvcnn_amd.evaluate import vote_confidence
    n = 2 * GRID_CAP * THREADS // 2 + 77
    t = torch.zeros(2, 7, n, device=DEV)
    t[:, 2] = t[:, 5] = t[:, 6] = 3.0
    conf, pred = vote_confidence(t)
    assert (pred == 2).all() and (conf == conf[0, 0]).all()
    conf, pred = vote_confidence(t, (3, 7))
    assert (pred == 5).all()
    conf, pred = vote_confidence(t, torch.tensor([[0, 2], [6, 9]], dtype=torch.int32, device=DEV))
    assert (pred[0] == 0).all() and (pred[1] == 6).all()


@pytest.mark.parametrize('num_points', [1, 255, 256, 257, 4096])
@pytest.mark.parametrize('layout', ['points_major', 'channels_first'])
def test_eval_tile_many_rows_and_bad_indices(num_points, layout):
    """B * E * C in the tens of thousands (the % C, / E row decode of every row), both stride layouts, result bytes equal to the numpy
    gather; indices -1, src_points and src_points + 5 give a quiet NaN and every other element is untouched.  The source is a view
    inside a sentinel-filled allocation: `idx >= 0 && idx < src_points` is tested before src[] is read, so neither the sentinel nor a
    neighbouring cloud's value can appear."""
    rng = np.random.default_rng(70 + num_points)
    c = 9
    e = {1: 600, 255: 12, 256: 12, 257: 12, 4096: 2}[num_points]
    b = {1: 5, 255: 180, 256: 180, 257: 180, 4096: 700}[num_points] if layout == 'points_major' else 1
    if layout == 'channels_first':
        e = {1: 3000, 255: 1200, 256: 1200, 257: 1200, 4096: 1200}[num_points]
    assert b * e * c >= 10000
    v = e * num_points
    src_points = 777
    if layout == 'points_major':
        src, whole = _padded((b, src_points, c), torch.float32, 12345.0)
        strides = (src_points * c, c, 1)
    else:
        src, whole = _padded((c, src_points), torch.float32, 12345.0)
        strides = (0, 1, src_points)
    data = rng.standard_normal(tuple(src.shape)).astype(np.float32)
    src.copy_(torch.from_numpy(data))
    idx = rng.integers(0, src_points, size=(b, v), dtype=np.int64)
    flat = idx.reshape(-1)
    where = rng.choice(flat.size, size=max(flat.size // 500, 3), replace=False)
    flat[where] = np.array([-1, src_points, src_points + 5], dtype=np.int64)[np.arange(where.size) % 3]
    got = _be().eval_tile(src, torch.from_numpy(idx).to(DEV), num_points, c, strides, src_points).cpu().numpy()
    ok = (idx >= 0) & (idx < src_points)
    safe = np.where(ok, idx, 0)
    if layout == 'points_major':
        gathered = np.stack([data[r][safe[r]] for r in range(b)])                        # (b, v, c)
        gathered[~ok] = np.nan
        want = gathered.reshape(b * e, num_points, c).transpose(0, 2, 1)
    else:
        gathered = data[:, safe[0]]                                                      # (c, v)
        gathered[:, ~ok[0]] = np.nan
        want = gathered.reshape(c, e, num_points).transpose(1, 0, 2)
    want = np.ascontiguousarray(want)
    assert got.shape == want.shape
    bad = np.isnan(want)
    assert bad.sum() == c * where.size and np.isnan(got[bad]).all()
    assert got[~bad].tobytes() == want[~bad].tobytes()
    assert _pads_intact(whole, 12345.0) and not (got == 12345.0).any()
