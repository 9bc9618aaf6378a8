"""The device draw stream on the CPU: tests/draws_truth.py (numpy integers) against the published Philox vectors, against the constants
of csrc/philox.h, and against the integer draws stored in tests/golden/device_draws.pt -- so the recording the GPU test compares with is
itself checked here, and a slip in the stream's statement (a counter word, a truncation of the seed) cannot pass unseen."""
import os
import re

import numpy as np
import torch

from conftest import ROOT
import draws_truth as dt
import test_gpu_device_draws as cases

HEADER = os.path.join(ROOT, 'pvcnn_amd', 'csrc', 'philox.h')


def hexes(words):
    return ' '.join(f'{int(w):08x}' for w in words)


def test_philox_known_answers():
    """The Random123 vectors of philox4x32_10 (kat_vectors)."""
    ones = 0xFFFFFFFF
    assert hexes(dt.philox4x32_10((0, 0, 0, 0), (0, 0))) == '6627e8d5 e169c58d bc57ac4c 9b00dbd8'
    assert hexes(dt.philox4x32_10((ones,) * 4, (ones, ones))) == '408f276d 41c83b0e a20bc7c6 6d5451fd'
    assert hexes(dt.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        'd16cfe09 94fdcceb 5001e420 24126ea1'
    many = dt.philox4x32_10((np.arange(5), 7, 9, 1), (3, 4))                       # arrays broadcast, element by element
    assert many.shape == (5, 4) and all(np.array_equal(many[i], dt.philox4x32_10((i, 7, 9, 1), (3, 4))) for i in range(5))


def test_key_and_stream_from_a_seed():
    seed = (0x0123456789ABCDEF, (5 << 32) | 7)
    assert dt.draw_stream(seed) == ((0x89ABCDEF, 0x01234567), 7)                   # low half first; seed[1] truncated
    assert dt.draw_stream((-1, -2)) == ((0xFFFFFFFF, 0xFFFFFFFF), 0xFFFFFFFE)      # int64 words are taken as their 64 bits
    assert np.array_equal(dt.draw_words(seed, 3, 2, 1), dt.philox4x32_10((3, 2, 7, 1), (0x89ABCDEF, 0x01234567)))
    assert not np.array_equal(dt.draw_words(seed, 3, 2, 1), dt.draw_words((seed[0], 5 << 32), 3, 2, 1))


def test_pick_sort_words_and_flip_bit():
    seed = cases.SEED_WORDS['s3dis']
    p = np.arange(64)
    x = dt.draw_words(seed, p, 1, 0)[:, 0].astype(object)
    for n in (1, 40, 8192):
        pick = dt.draw_index(seed, p, 1, n)
        assert pick.tolist() == [(int(w) * n) >> 32 for w in x] and pick.min() >= 0 and pick.max() < n
    w = dt.sort_words(seed, 1, 70)
    assert [int(v) for v in w] == [(int(k) << 32) | i for i, k in enumerate(dt.draw_words(seed, np.arange(70), 1, 0)[:, 0].astype(object))]
    chosen = dt.select_distinct(seed, 1, 70, 64)
    assert len(set(chosen.tolist())) == 64 and chosen.tolist() == sorted(range(70), key=lambda i: int(w[i]))[:64]
    flips = dt.flip_bit(seed, np.arange(256))
    assert flips.tolist() == [int(v) >> 31 for v in dt.draw_words(seed, 0, np.arange(256), 2)[:, 0]] and 64 < flips.sum() < 192


def test_word_to_number_conversions():
    r = np.array([0, 1, 255, 256, 0x80000000, 0xFFFFFF00, 0xFFFFFFFF], dtype=np.uint32)
    assert dt.unit_f32(r).dtype == np.float32 and dt.unit_f32(r).tolist() == [0.0, 0.0, 0.0, 2.0 ** -24, 0.5, 1 - 2.0 ** -24, 1 - 2.0 ** -24]
    assert dt.open_f64(r).tolist() == [(int(v) + 0.5) / 2.0 ** 32 for v in r] and 0 < dt.open_f64(r).min() and dt.open_f64(r).max() < 1
    assert dt.unit_f64(r).tolist() == [int(v) / 2.0 ** 32 for v in r] and dt.unit_f64(r).min() == 0 and dt.unit_f64(r).max() < 1


def test_the_counter_words_of_the_header():
    """csrc/philox.h's table is the numpy restatement's, and the words one seed can reach are distinct."""
    text = open(HEADER).read()
    table = {name: int(value) for name, value in re.findall(r'constexpr uint32_t kDraw(\w+) = (\d+)u;', text)}
    assert table == {'Pick': 0, 'Jitter': 1, 'FlipShift': 2, 'Box': 3, 'AugCloud': 16, 'AugJitter': 20, 'AugKeep': 21}
    assert [table[k] for k in ('Pick', 'Jitter', 'FlipShift', 'Box', 'AugCloud', 'AugJitter', 'AugKeep')] == list(dt.COUNTERS.values())
    assembly = [table[k] for k in ('Pick', 'Jitter', 'FlipShift', 'Box')]
    augment = list(range(table['AugCloud'], table['AugCloud'] + dt.AUG_CLOUD_WORDS)) + [table['AugJitter'], table['AugKeep']]
    assert len(set(assembly + augment)) == len(assembly) + len(augment) == 10
    assert 'static_assert(kDrawPick' in text


# ---- the recording -------------------------------------------------------------------------------------------------------------------
def golden():
    return torch.load(cases.GOLDEN)


def test_recorded_s3dis_picks_are_the_streams():
    """Channel 0 of the indexed store names the row: with replacement below N points, the sorted selection from N on."""
    g, seed, n_out = golden(), cases.SEED_WORDS['s3dis'], cases.S3DIS_POINTS
    for name in ('s3dis9.0', 's3dis6.0'):
        picks = g[name][:, 0, :].numpy()
        assert g[name].shape[1] == int(name[5]) and np.array_equal(picks, np.round(picks))
        for b, n in enumerate(cases.S3DIS_COUNTS):
            want = dt.select_distinct(seed, b, n, n_out) if n >= n_out else dt.draw_index(seed, np.arange(n_out), b, n)
            assert picks[b].astype(np.int64).tolist() == want.tolist(), (name, b, n)


def test_recorded_frustum_picks_and_flips_are_the_streams():
    """Channel 3 (reflectance) names the row; a flipped sample is the one whose x is the negated stored x."""
    g, seed = golden(), cases.SEED_WORDS['frustum']
    _, clouds = cases.frustum_clouds()
    p = np.arange(cases.FRUSTUM_POINTS)
    flips = dt.flip_bit(seed, np.arange(len(clouds)))
    assert 0 < flips.sum() < len(clouds)                                           # both states are in the recording
    for name in ('frustum.0.features', 'frustum_rgb.0.features'):
        f = g[name].numpy()
        for b, cloud in enumerate(clouds):
            want = dt.draw_index(seed, p, b, len(cloud))
            assert f[b, 3].astype(np.int64).tolist() == want.tolist(), (name, b)
            x = cloud[want, 0]
            assert np.array_equal(f[b, 0], -x if name == 'frustum.0.features' and flips[b] else x), (name, b)


def test_recorded_frame_store_draws_are_the_streams():
    import frame_store_truth as fst
    import test_gpu_frame_store as ts
    g, seed = golden(), cases.SEED_WORDS['frame_store']
    b = np.arange(cases.FRAME_STORE_BATCH)
    rows, used = g['frame_store.draws.params'].numpy(), g['frame_store.draws.used'].numpy()
    assert np.array_equal(rows[:, :4], dt.unit_f64(dt.draw_words(seed, 0, b, dt.COUNTERS['box'])))
    assert np.array_equal(g['frame_store.draws.flip'].numpy(), dt.flip_bit(seed, b).astype(np.float64))
    item = 0
    for f in cases.FRAME_STORE_FRAMES:
        scan, boxes, boxes_3d, _ = ts.frame(*f)
        points = fst.frame_points(scan, ts.P, ts.R0, ts.V2C, ts.SIZE)
        for box, box_3d in zip(boxes, boxes_3d):
            use, box_used = fst.box_used(points, ts.P, box, box_3d, rows[item])[:2]
            k = int(fst.select(points, box_used, box_3d)[0].sum())
            assert use == used[item] and k > 0
            want = dt.draw_index(seed, np.arange(cases.FRAME_STORE_POINTS), item, k)
            assert g['frame_store.draws.choices'][item].tolist() == want.tolist(), item
            item += 1
    assert item == cases.FRAME_STORE_BATCH


def test_recorded_mask_selections_are_the_streams():
    g, seed = golden(), cases.SEED_WORDS['mask_select']
    branches = set()
    for name, mask in cases.masks().items():
        m = cases.MASK_CASES[name][1]
        for b in range(mask.shape[0]):
            cand = np.nonzero(mask[b].numpy())[0]
            branches.add(len(cand) >= m)
            assert g[f'mask_select.{name}'][b].tolist() == cand[dt.mask_select(seed, b, len(cand), m)].tolist(), (name, b)
    assert branches == {True, False}
