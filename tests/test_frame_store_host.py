"""The host side of the KITTI frame store (pvcnn_amd.frames.random_shift_box2d, tests/frame_store_truth.py): the numpy definition against
closed forms and against pvcnn_amd.data.angle_to_bin_id.  No GPU, no native call."""
import numpy as np
import pytest

from conftest import SEED
import frame_store_truth as fst

P = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_random_shift_box2d_equals_the_truth_bit_for_bit():
    from pvcnn_amd import frames
    rng = np.random.RandomState(SEED)
    lo = rng.rand(257, 2) * [1100, 300]
    boxes = np.concatenate([lo, lo + rng.rand(257, 2) * [140, 70] + 1], axis=1)
    draws = rng.random_sample((257, 4))
    for ratio in (0.1, 0.25, 0.037):
        got = frames.random_shift_box2d(boxes, draws, ratio)
        want = np.stack([fst.random_shift_box2d(b, u, ratio) for b, u in zip(boxes, draws)])
        assert got.shape == (257, 4) and got.dtype == np.float64 and np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(frames.random_shift_box2d(boxes, draws)), bits(frames.random_shift_box2d(boxes, draws, 0.1)))
    assert np.array_equal(bits(frames.random_shift_box2d(boxes, draws, 0.0)), bits(boxes))     # off: the boxes as they are
    with pytest.raises(ValueError):
        frames.random_shift_box2d(boxes, draws[:5])


def test_random_shift_box2d_closed_forms():
    from pvcnn_amd import frames
    box = np.array([[100.0, 40.0, 180.0, 104.0]])                       # w = 80, h = 64: every product below is exact
    same = frames.random_shift_box2d(box, [[0.5, 0.5, 0.5, 0.5]], 0.25)
    assert np.array_equal(same, box)                                    # u = 0.5 everywhere: the same centre and size
    left = frames.random_shift_box2d(box, [[0.0, 0.5, 0.5, 0.5]], 0.25)
    assert np.array_equal(left, box - [[20.0, 0.0, 20.0, 0.0]])         # u0 = 0: shifted by -w r
    low = frames.random_shift_box2d(box, [[0.5, 0.5, 0.0, 0.5]], 0.25)
    assert np.array_equal(low, [[100.0, 48.0, 180.0, 96.0]])            # u2 = 0: h (1 - r) about the same centre
    wide = frames.random_shift_box2d(box, [[0.5, 1.0, 0.5, 1.0]], 0.25)
    assert np.array_equal(wide, [[90.0, 56.0, 190.0, 120.0]])           # u1 = 1: +h r; u3 = 1: w (1 + r)
    row = fst.params_row(P, box[0], [0.5, 0.5, 0.5, 0.5], 0.25)
    assert row.shape == (fst.PARAMS,) and np.array_equal(row[4:8], box[0])
    assert row[8] == np.pi / 2.0 + frames.frustum_angle(type('C', (), {'P': P}), box)[0] and row[9] == np.cos(row[8]) and row[11] == 0


def test_the_bins_of_the_truth_are_those_of_the_dataset():
    from pvcnn_amd.data import angle_to_bin_id
    rng = np.random.RandomState(SEED + 1)
    angles = np.concatenate([rng.uniform(-20, 20, size=2000), [0.0, -0.0, np.pi, -np.pi, 2 * np.pi, -2 * np.pi, 4 * np.pi, -1e-300, 7.5, -7.5],
                             np.arange(-24, 25) * (2 * np.pi / 12), np.arange(-24, 25) * (2 * np.pi / 12) + np.pi / 12])
    assert (angles < 0).any() and (angles > 2 * np.pi).any()
    for bins in (12, 1, 7):
        for a in angles:
            want_bin, want_res = angle_to_bin_id(np.float64(a), bins)
            got_bin, got_res = fst.angle_to_bin(a, bins)
            assert got_bin == want_bin and np.array_equal(bits(got_res), bits(want_res)), (a, bins)
            assert 0 <= got_bin <= bins
    assert fst.floor_mod(-1.0, 3.0) == 2.0 and fst.floor_mod(7.0, 3.0) == 1.0 and fst.floor_mod(-6.0, 3.0) == 0.0


def test_the_three_branches_of_the_acceptance_rule():
    rows = np.array([[0.0, 1.0, 10.0, 0.5], [3.0, 1.0, 10.0, 0.5]], dtype=np.float32)        # point 0 inside the 3-D box, point 1 outside
    uv = np.array([[104.0, 60.0], [170.0, 60.0]])
    box, box_3d = np.array([100.0, 47.0, 180.0, 73.0]), np.array([1.6, 1.0, 1.0, 0.0, 1.5, 10.0, 0.0])       # 26 px high
    sel, pos = fst.select((rows, uv), box, box_3d)
    assert sel.tolist() == [True, True] and pos.tolist() == [True, False] and fst.admitted((rows, uv), box, box_3d)

    def used(u):
        return fst.box_used((rows, uv), P, box, box_3d, fst.params_row(P, box, u))

    keep = used([0.5, 0.5, 0.5, 0.5])
    assert keep[0] == 1 and keep[5] == 'accepted' and np.allclose(keep[1], box, rtol=0, atol=1e-12)
    low = used([0.5, 0.5, 0.0, 0.5])                                   # 26 (1 - 0.1) = 23.4 px
    assert low[0] == 0 and low[5] == 'low' and np.array_equal(low[1], box) and low[2] == fst.rotation_angle(P, box)
    lost = used([0.999, 0.5, 0.5, 0.5])                                # shifted right by almost 8 px: point 0 (4 px in) is out, point 1 is not
    assert lost[0] == 0 and lost[5] == 'lost' and np.array_equal(lost[1], box)
    assert fst.select((rows, uv), fst.params_row(P, box, [0.999, 0.5, 0.5, 0.5])[4:8], box_3d)[0].tolist() == [False, True]
    off = fst.box_used((rows, uv), P, box, box_3d, None, shift_ratio=0)
    assert off[0] == 0 and off[5] == 'off'
    assert fst.accepted([0, 0, 10, 25], 1) and not fst.accepted([0, 0, 10, 24.999], 1) and not fst.accepted([0, 0, 10, 25], 0)
    # a fallen-back sample is the unperturbed one: the same bits as with the perturbation off
    item = dict(box=box, box_3d=box_3d, one_hot=[1, 0, 0], size_residual=np.zeros(3, np.float32), size_template_id=0, class_id=0)
    a = fst.sample((rows, uv), P, item, fst.params_row(P, box, [0.5, 0.5, 0.0, 0.5]), [0, 1, 1], 0.9, -0.3, frustum_rotate=True,
                   random_flip=True, random_shift=True)
    b = fst.sample((rows, uv), P, item, None, [0, 1, 1], 0.9, -0.3, frustum_rotate=True, random_flip=True, random_shift=True, shift_ratio=0)
    assert a['used'] == 0 and all(np.array_equal(a[k], b[k]) for k in a) and a['mask_logits'].tolist() == [1, 0, 0]
