"""`train.py --evaluate` on the device: the per-file loops of evaluate/s3dis/eval.py and evaluate/shapenet/eval.py.

Reference (evaluate/s3dis/eval.py:133-216, evaluate/shapenet/eval.py:124-200): per batch of windows it tiles and shuffles the points on
the host, runs F.softmax(model(x), 1).max(1), copies both results back with .cpu() and merges the votes and counts the statistics in
numba loops.  Here the shuffled index arrays are still drawn on the host -- with the same RNG calls in the same order, so a seeded run
feeds the model exactly what the reference feeds it -- and uploaded once per file; everything after is on the device
(csrc/evaluate.hip): pvcnn_eval_tile -> model(x) under no_grad -> pvcnn_vote_confidence -> pvcnn_vote_merge, and pvcnn_seg_counts for
the statistics.  The merge reproduces the reference's sequential "strictly greater, first wins" update exactly.

Data loading (h5py, np.loadtxt) stays with the caller; see INTEGRATION.md for the reference's loop with these calls swapped in.
"""
import math

import numpy as np
import torch

from .modules.functional import backend as _be

__all__ = ['SceneVotes', 'ShapeVotes', 'vote_confidence', 's3dis_shuffled_indices', 'shapenet_shuffled_indices', 's3dis_file_votes',
           's3dis_scene_stats', 'shapenet_shape_votes', 'shapenet_shape_stats']


def vote_confidence(logits, class_range=None):
    """-> (conf, pred int32) = F.softmax(logits, 1)[:, c0:c1].max(1) with pred += c0; ties go to the lowest class."""
    return _be._backend.vote_confidence(logits.float().contiguous(), class_range)


class SceneVotes:
    """Per-point vote state of one scene (or shape) on the device: confidences start at 0, predictions at -1, as in the reference."""

    def __init__(self, num_points, device):
        self.num_points = int(num_points)
        self.device = torch.device(device)
        self._conf = torch.zeros((self.num_points,), dtype=torch.float32, device=self.device)
        self._pred = torch.full((self.num_points,), -1, dtype=torch.int64, device=self.device)
        self._keys = torch.zeros((self.num_points,), dtype=torch.int64, device=self.device)   # merge workspace: zero between calls

    def add(self, conf, pred, shuffled, mapping=None):
        """update_scene_predictions / update_shape_predictions: conf, pred (B, V) (or anything of B*V elements, viewed as shuffled's
        shape); vote (b, p) targets mapping[b, shuffled[b, p]], or shuffled[b, p] without a mapping."""
        shuffled = shuffled if shuffled.dim() == 2 else shuffled.view(1, -1)
        _be._backend.vote_merge(conf.reshape(shuffled.shape), pred.reshape(shuffled.shape), shuffled, self._conf, self._pred, self._keys,
                                mapping)

    def predictions(self):
        return self._pred

    def confidences(self):
        return self._conf


class ShapeVotes(SceneVotes):
    """SceneVotes of one ShapeNet shape: votes are the softmax maxima inside the shape's part classes [start_class, end_class)."""

    def __init__(self, num_points, device, start_class, end_class):
        super().__init__(num_points, device)
        self.start_class, self.end_class = int(start_class), int(end_class)

    def add_logits(self, logits, shuffled):
        conf, pred = vote_confidence(logits, (self.start_class, self.end_class))
        self.add(conf, pred, shuffled)


def s3dis_shuffled_indices(scene_num_points, min_window_index, max_window_index, total_num_voted_points, rng=np.random):
    """The reference's "repeat, shuffle" index arrays (eval.py:160-167) for windows [min, max): (windows, V) int64, drawing from `rng`
    exactly as the reference draws from np.random (one shuffle per window, in window order)."""
    out = np.zeros((max_window_index - min_window_index, total_num_voted_points), dtype=np.int64)
    for relative_window_index in range(max_window_index - min_window_index):
        num_points_in_window = scene_num_points[relative_window_index + min_window_index]
        num_repeats = math.ceil(total_num_voted_points / num_points_in_window)
        shuffled_point_indices = np.tile(np.arange(num_points_in_window), num_repeats)
        shuffled_point_indices = shuffled_point_indices[:total_num_voted_points]
        rng.shuffle(shuffled_point_indices)
        out[relative_window_index] = shuffled_point_indices
    return out


def shapenet_shuffled_indices(total_num_points_in_shape, total_num_voted_points, rng=np.random):
    """evaluate/shapenet/eval.py:165-168: (V,) int64."""
    num_repeats = math.ceil(total_num_voted_points / total_num_points_in_shape)
    shuffled_point_indices = np.tile(np.arange(total_num_points_in_shape), num_repeats)
    shuffled_point_indices = shuffled_point_indices[:total_num_voted_points]
    rng.shuffle(shuffled_point_indices)
    return shuffled_point_indices


def _upload(a, dtype, device):
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=dtype).contiguous()
    np_dtype = {torch.float32: np.float32, torch.int64: np.int64}[dtype]
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np_dtype)).to(device)


def s3dis_file_votes(model, scene_data, scene_num_points, window_to_scene_mapping, votes, num_points=4096, num_votes=1, batch_size=10,
                     rng=np.random):
    """The per-file loop of evaluate/s3dis/eval.py:139-180 on the device.  scene_data (W, max_points, C) float32 (h5 'data'),
    scene_num_points (W,) ('data_num'), window_to_scene_mapping (W, max_points) int64 ('indices_split_to_full'); votes: the scene's
    SceneVotes.  The model sees (batch_size * E, C, num_points) inputs, as in the reference."""
    be, device = _be._backend, votes.device
    num_windows, max_num_points_per_window, num_channels = scene_data.shape
    extra_batch_size = num_votes * math.ceil(max_num_points_per_window / num_points)
    total_num_voted_points = extra_batch_size * num_points
    scene_num_points = np.asarray(scene_num_points.cpu() if isinstance(scene_num_points, torch.Tensor) else scene_num_points)
    shuffled = s3dis_shuffled_indices(scene_num_points, 0, num_windows, total_num_voted_points, rng)
    data = _upload(scene_data, torch.float32, device)
    mapping = _upload(window_to_scene_mapping, torch.int64, device)
    shuffled = torch.from_numpy(shuffled).to(device)
    for min_window_index in range(0, num_windows, batch_size):
        max_window_index = min(min_window_index + batch_size, num_windows)
        batch = shuffled[min_window_index:max_window_index]
        inputs = be.eval_tile(data[min_window_index:max_window_index], batch, num_points, num_channels,
                              (max_num_points_per_window * num_channels, num_channels, 1), max_num_points_per_window)
        with torch.no_grad():
            conf, pred = vote_confidence(model(inputs))
        votes.add(conf, pred, batch, mapping[min_window_index:max_window_index])


def s3dis_scene_stats(stats, ground_truth, predictions, scene_index):
    """update_stats of evaluate/s3dis/eval.py:205-213: stats (3, C, S) float64 numpy array, column scene_index += [seen; positive;
    correct] of (ground_truth, predictions), including the reference's quirk: an unvoted point (prediction -1) counts as a positive of
    class C-1.  Counted on the device (exact integers), one device-to-host copy."""
    if isinstance(predictions, SceneVotes):
        predictions = predictions.predictions()
    gt = _upload(np.asarray(ground_truth).reshape(-1) if not isinstance(ground_truth, torch.Tensor) else ground_truth.reshape(-1),
                 torch.int64, predictions.device)
    counts = _be._backend.seg_counts(gt, predictions.reshape(-1).contiguous(), stats.shape[1], wrap_negative=True)
    stats[:, :, scene_index] += counts.cpu().numpy()


def shapenet_shape_votes(model, point_set, votes, num_points=2048, num_votes=1, rng=np.random):
    """The per-shape vote of evaluate/shapenet/eval.py:162-183 on the device.  point_set (C, P) float32 (coordinates, normals,
    one-hot shape id, as the reference builds it); votes: the shape's ShapeVotes (it holds the part-class range).
    -> the shuffled index array (V,) the reference would have drawn."""
    be, device = _be._backend, votes.device
    num_channels, total_num_points_in_shape = point_set.shape
    extra_batch_size = num_votes * math.ceil(total_num_points_in_shape / num_points)
    total_num_voted_points = extra_batch_size * num_points
    idx = shapenet_shuffled_indices(total_num_points_in_shape, total_num_voted_points, rng)
    src = _upload(point_set, torch.float32, device)
    shuffled = torch.from_numpy(idx).to(device).view(1, -1)
    inputs = be.eval_tile(src, shuffled, num_points, num_channels, (0, 1, total_num_points_in_shape), total_num_points_in_shape)
    with torch.no_grad():
        logits = model(inputs)
    votes.add_logits(logits, shuffled)
    return idx


def shapenet_iou(counts, start_class, end_class):
    """The IoU of update_stats (evaluate/shapenet/eval.py:189-200) from (3, >= end_class) integer counts, in the reference's order."""
    seen, positive, correct = counts
    iou = 0.0
    for i in range(start_class, end_class):
        union = seen[i] + positive[i] - correct[i]
        if union == 0:
            iou += 1
        else:
            iou += correct[i] / union
    iou /= (end_class - start_class)
    return iou


def shapenet_shape_stats(stats, ground_truth, predictions, shape_id, start_class, end_class):
    """update_stats of evaluate/shapenet/eval.py:189-200: stats (num_shapes, 2) float64, row shape_id += (IoU, 1)."""
    if isinstance(predictions, SceneVotes):
        predictions = predictions.predictions()
    gt = _upload(np.asarray(ground_truth).reshape(-1) if not isinstance(ground_truth, torch.Tensor) else ground_truth.reshape(-1),
                 torch.int64, predictions.device)
    counts = _be._backend.seg_counts(gt, predictions.reshape(-1).contiguous(), end_class, wrap_negative=False).tolist()
    stats[shape_id][0] += shapenet_iou(counts, start_class, end_class)
    stats[shape_id][1] += 1
