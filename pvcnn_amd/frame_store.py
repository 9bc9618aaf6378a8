"""Frustum-KITTI training batches straight from the frames, with a fresh perturbation of every sample's 2-D box (csrc/frame_store.hip).

The original preparation (frustum-pointnets' `extract_frustum_data`, `perturb_box2d=True`, which the reference's
datasets/kitti/frustum.py points to for its pickles) never trains on a ground-truth 2-D box as it is: it draws five shifted and rescaled
copies of every box, once, offline, and keeps those that are still 25 px high and still hold a point of the object.  A perturbed box
selects other points of the sweep, so the draw cannot be made on a packed frustum (`DeviceFrustumKitti`).  `DeviceKittiFrames` keeps
the in-image points of every frame in device memory instead -- about 20 k points, 640 KB, per KITTI frame -- and cuts every sample out
of its frame when the batch is assembled: a new draw for every sample of every epoch, inside a captured step.

    store = DeviceKittiFrames(frames, 1024, size_templates=..., class_name_to_size_template_id=..., random_flip=True,
                              random_shift=True, frustum_rotate=True)          # frames: (scan, calib, image_size, boxes_2d, boxes_3d, names)
    loader = DeviceLoader(store, 32, drop_last=True)
    x, y = loader.static_batch()
    step = GraphedTrainStep(model, lambda: (loader.feed(), criterion(model(x), y))[1], ...)

An item is one object of a whitelisted class whose own box passes the original's rule (at least `min_box_height` high, one point inside
the 3-D box); a sample whose perturbed box fails the rule falls back to the item's own box, so there is no retry and no data-dependent
launch.  The batch has `DeviceFrustumKitti`'s ground-truth structure.  The definition is include/pvcnn_hip.h's ("KITTI frame store");
tests/frame_store_truth.py restates it in numpy.

Two sources of randomness, as in `data`: parity mode (`choices`, `params`, `flip`, `shift` from the caller: no trigonometric function
runs on the device, the batch equals the numpy truth bit for bit) and device mode (a Philox stream keyed by `seed`; the rows the kernel
used are left in `draws(batch_size)`, and `draws_out=` records every draw so that the batch can be reproduced in parity mode).

Host synchronisation: one device-to-host copy per frame when the store is built (the counts that decide which objects are admitted),
none on the batch path; all of them go through `_read`, which counts them (`copies_made()`).  There is no CPU implementation.
"""
import numpy as np
import torch

from . import frames as _frames
from .data import DeviceFrustumKitti

__all__ = ['DeviceKittiFrames', 'copies_made', 'PARAMS', 'MAX_FRAME_POINTS']

PARAMS = 12                          # PVCNN_FRAME_STORE_PARAMS
ITEM_COLUMNS = 24                    # PVCNN_FRAME_STORE_ITEM_COLUMNS
MAX_FRAME_POINTS = 1 << 17           # PVCNN_FRAME_STORE_MAX_POINTS: the in-image points of one frame (sizes the launch's LDS)
_copies = 0


def copies_made():
    """Device-to-host copies this module has made so far (every one goes through `_read`)."""
    return _copies


def _read(t):
    """The one place this module reads device memory on the host."""
    global _copies
    _copies += 1
    return t.cpu().numpy()


class DeviceKittiFrames(DeviceFrustumKitti):
    """The in-image points of KITTI frames and one item per admitted object; `assemble` / `DeviceLoader.feed()` write
    `DeviceFrustumKitti`'s ground-truth batch.  A subclass of `DeviceFrustumKitti` for what the two share -- the batch structure, the
    argument handling, `DeviceLoader`'s refusal of `augment=` -- not for its packed store: the constructors of the parent do not apply.

    frames: one tuple (scan (N, 4) fp32, Calibration, image_size (width, height), boxes_2d (M, 4), boxes_3d (M, 7) h w l x y z ry,
    class names (M)) or a list of them; more can be added with `add_frame`.  Objects of other classes than `classes` are left out.
    shift_ratio = 0 turns the perturbation off (the stored boxes, no draw consumed)."""

    def __init__(self, frames=None, num_points=1024, classes=('Car', 'Pedestrian', 'Cyclist'), num_heading_angle_bins=12,
                 class_name_to_size_template_id=None, size_templates=None, random_flip=False, random_shift=False, frustum_rotate=False,
                 shift_ratio=0.1, min_box_height=25, clip_distance=2.0, max_frame_points=MAX_FRAME_POINTS):
        if int(num_points) < 1:
            raise ValueError('num_points must be positive')
        if class_name_to_size_template_id is None or size_templates is None:
            raise ValueError('class_name_to_size_template_id and size_templates are required')
        if not 0.0 <= float(shift_ratio) < 1.0:
            raise ValueError('shift_ratio must lie in [0, 1)')
        if not 1 <= int(max_frame_points) <= MAX_FRAME_POINTS:
            raise ValueError(f'max_frame_points must lie in [1, {MAX_FRAME_POINTS}]')
        self.rgb_detection = False
        self.num_points, self.classes = int(num_points), tuple(classes)
        self.num_classes = len(self.classes)
        self.num_heading_angle_bins = int(num_heading_angle_bins)
        self.random_flip, self.random_shift, self.frustum_rotate = bool(random_flip), bool(random_shift), bool(frustum_rotate)
        self.shift_ratio, self.min_box_height, self.clip_distance = float(shift_ratio), float(min_box_height), float(clip_distance)
        self.max_frame_points = int(max_frame_points)
        self._template_ids, self._templates = dict(class_name_to_size_template_id), size_templates
        self.device = None
        self._chunks, self._counts = [], []                  # per stored frame: (rows, uv) on the device; its in-image points
        self._f64, self._f32, self._i64 = [], [], []          # per item: the rows of the tables
        self._ready, self._scratch = False, {}
        self._tables = ['rows', 'uv', 'frame_offsets', 'item_f64', 'item_f32', 'item_i64']
        self.rows = self.uv = self.frame_offsets = self.item_f64 = self.item_f32 = self.item_i64 = self.labels = None
        if frames is not None:
            for frame in ([frames] if isinstance(frames, tuple) else list(frames)):
                self.add_frame(*frame)
            self._finalise()

    @classmethod
    def _not_this_store(cls, *args, **kwargs):
        raise TypeError('DeviceKittiFrames is built from frames (its constructor, `add_frame`); packed frustums go to DeviceFrustumKitti')
    from_frustums = from_rgb_detection = from_dataset = _not_this_store

    # -- construction --
    def add_frame(self, scan, calib, image_size, boxes_2d, boxes_3d, classes):
        """One frame -> the number of objects admitted.  One device-to-host copy: the counts of the frame's boxes and of its in-image
        points.  A frame with more than `max_frame_points` in-image points is refused, and nothing of it is stored; a frame that
        admits no object leaves no points behind."""
        x = _frames._device_scan(scan)
        dev = x.device
        if self.device is not None and dev != self.device:
            raise ValueError(f'the store lives on {self.device}, the scan on {dev}')
        boxes = np.asarray(boxes_2d, dtype=np.float64).reshape(-1, 4)
        b3 = np.asarray(boxes_3d, dtype=np.float64).reshape(-1, 7)
        classes = list(classes)
        if not (len(classes) == boxes.shape[0] == b3.shape[0]):
            raise ValueError('one class name and one 3-D box (h, w, l, x, y, z, ry) per 2-D box expected')
        class_id = {c: i for i, c in enumerate(self.classes)}
        want = [i for i, c in enumerate(classes) if c in class_id]
        if not want:
            return 0
        rows, uv, in_image = _frames._project(x, calib, image_size, self.clip_distance, None)
        table = torch.from_numpy(_frames.box_table(calib, boxes[want], None, None, b3[want])).to(dev)
        counts = _frames._count(rows, uv, in_image, table, True)[3]
        host = _read(torch.cat([counts.reshape(-1).to(torch.int64), in_image.sum(dtype=torch.int64).reshape(1)])).astype(np.int64)
        n_in, n = int(host[-1]), host[:-1].reshape(-1, 2)
        if n_in > self.max_frame_points:
            raise ValueError(f'a frame with {n_in} in-image points: at most {self.max_frame_points} are held per frame '
                             f'(the cap sizes the batch kernel\'s LDS; {MAX_FRAME_POINTS} at the most)')
        keep = ((boxes[want, 3] - boxes[want, 1]) >= self.min_box_height) & (n[:, 1] > 0)
        if not keep.any():
            return 0
        # the in-image points in ascending point index (a stable sort of the flags: no host round trip for the count, it is known)
        first = torch.argsort(in_image, descending=True, stable=True)[:n_in]
        frame = len(self._counts)
        k = self.num_classes
        P = calib.P
        for j in np.nonzero(keep)[0]:
            i = want[j]
            name, box, (h, w, l, tx, ty, tz, ry) = classes[i], boxes[i], b3[i]
            corners = _frames.box_corners(b3[i])[0]
            rotation = np.pi / 2.0 + _frames.frustum_angle(calib, box)[0]
            f64 = np.zeros(ITEM_COLUMNS, dtype=np.float64)
            f64[0:3] = P[0, 0], P[0, 2], P[0, 3]
            f64[3:7] = box
            f64[7:16] = h, w, l, tx, ty, tz, np.cos(ry), np.sin(ry), ry
            f64[16:19] = (corners[0, :] + corners[6, :]) / 2.0
            f64[19:22] = rotation, np.cos(rotation), np.sin(rotation)
            f32 = np.zeros(k + 3, dtype=np.float32)
            f32[class_id[name]] = 1
            f32[k:k + 3] = (np.array([l, w, h]) - np.asarray(self._templates[name])).astype(np.float32)
            self._f64.append(f64)
            self._f32.append(f32)
            self._i64.append(np.array([frame, self._template_ids[name], class_id[name]], dtype=np.int64))
        self._chunks.append((rows[first], uv[first]))
        self._counts.append(n_in)
        self.device, self._ready = dev, False
        return int(keep.sum())

    def _finalise(self):
        """Pack what has been added: the frames' points one after another, the item tables uploaded."""
        if self._ready:
            return
        if not self._f64:
            raise ValueError('a store with no admitted object: no box of a whitelisted class is at least min_box_height high and holds '
                             'a point of its 3-D box')
        dev = self.device
        if len(self._chunks) > 1:                            # (the merged tensors stay the one chunk that later frames are added to)
            self._chunks = [(torch.cat([c[0] for c in self._chunks]).contiguous(), torch.cat([c[1] for c in self._chunks]).contiguous())]
        self.rows, self.uv = self._chunks[0]
        offsets = np.zeros(len(self._counts) + 1, dtype=np.int64)
        np.cumsum(self._counts, out=offsets[1:])
        self.frame_offsets = torch.from_numpy(offsets).to(dev)
        self.item_f64 = torch.from_numpy(np.stack(self._f64)).to(dev)
        self.item_f32 = torch.from_numpy(np.stack(self._f32)).to(dev)
        self.item_i64 = torch.from_numpy(np.stack(self._i64)).to(dev)
        self.largest_frame = int(max(self._counts))
        self._ready = True

    # -- what DeviceLoader needs --
    def __len__(self):
        return len(self._f64)

    @property
    def num_frames(self):
        return len(self._counts)

    @property
    def out_channels(self):
        return 4

    @property
    def nbytes(self):
        self._finalise()
        return super().nbytes

    def to(self, device):
        raise RuntimeError('DeviceKittiFrames lives where its frames were projected -- there is no CPU implementation')

    def item(self, i):
        """(rows (n, 4) fp32, uv (n, 2) fp64) of the frame of item i: its in-image points, as stored."""
        self._finalise()
        f = int(np.stack(self._i64)[i, 0])
        a, b = int(sum(self._counts[:f])), int(sum(self._counts[:f + 1]))
        return self.rows[a:b], self.uv[a:b]

    def assemble_reference(self, *args, **kwargs):
        raise NotImplementedError('the definition of this assembly is include/pvcnn_hip.h ("KITTI frame store"), restated in numpy by '
                                  'tests/frame_store_truth.py')

    def empty_draws(self, batch_size):
        """Uninitialised tensors for `draws_out=`: every draw of one batch -- params (B, 12) fp64, used (B) int32, choices (B, N)
        int32, flip (B) and shift (B) fp64 -- which, handed back as `params`, `choices`, `flip`, `shift`, reproduce the batch."""
        b, d = int(batch_size), self.device
        return {'params': torch.empty((b, PARAMS), dtype=torch.float64, device=d), 'used': torch.empty((b,), dtype=torch.int32, device=d),
                'choices': torch.empty((b, self.num_points), dtype=torch.int32, device=d),
                'flip': torch.empty((b,), dtype=torch.float64, device=d), 'shift': torch.empty((b,), dtype=torch.float64, device=d)}

    def draws(self, batch_size):
        """(params (B, 12) fp64, used (B) int32) of the latest `assemble` of this batch size without `draws_out`: the box rows the
        kernel used (the four uniforms, the perturbed box, its rotation angle, cos and sin) and 1 where the perturbed box was accepted,
        0 where the sample fell back to the item's own box.  The tensors are allocated once per batch size; a replayed graph rewrites
        them."""
        b = int(batch_size)
        if b not in self._scratch:
            self._scratch[b] = (torch.zeros((b, PARAMS), dtype=torch.float64, device=self.device),
                                torch.zeros((b,), dtype=torch.int32, device=self.device))
        return self._scratch[b]

    def assemble(self, indices=None, out=None, *, choices=None, jitter=None, flip=None, shift=None, seed=None, order=None, cursor=None,
                 batch_size=None, params=None, draws_out=None):
        """One launch.  As `DeviceFrustumKitti.assemble`, plus `params` (B, 12) fp64, the parity rows of the box perturbation (needed
        with `choices` unless shift_ratio is 0), and `draws_out` (an `empty_draws` dict) to record every draw."""
        self._finalise()
        _, order, cursor, b, out, choices = self._begin(indices, out, order, cursor, batch_size, choices)
        params = self._draw(params, (b, PARAMS), torch.float64, 'params')
        flip, shift = self._draw(flip, (b,), torch.float64, 'flip'), self._draw(shift, (b,), torch.float64, 'shift')
        self._parity(choices, params=(params, self.shift_ratio != 0.0), flip=(flip, self.random_flip), shift=(shift, self.random_shift))
        seed = None if choices is not None else self._seed(seed)
        if draws_out is None:
            params_out, used = self.draws(b)
            record = (None, None, None)
        else:
            want = self.empty_draws(0)
            for name, like in want.items():
                t = draws_out[name]
                if tuple(t.shape) != (b,) + tuple(like.shape[1:]) or t.dtype != like.dtype or t.device != self.device or not t.is_contiguous():
                    raise ValueError(f'draws_out[{name}]: contiguous {like.dtype} tensor of shape {(b,) + tuple(like.shape[1:])} expected')
            params_out, used = draws_out['params'], draws_out['used']
            record = (draws_out['choices'], draws_out['flip'], draws_out['shift'])
        x, y = out
        _frames._call('frame_store_batch', self.rows, self.rows, self.uv, self.frame_offsets, self.num_frames, self.rows.shape[0],
                      self.largest_frame, self.item_f64, self.item_f32, self.item_i64, len(self), self.num_classes,
                      self.num_heading_angle_bins, int(self.frustum_rotate), int(self.random_flip), int(self.random_shift),
                      self.shift_ratio, self.min_box_height, order, order.numel(), cursor, b, self.num_points, params, choices, flip,
                      shift, seed, x['features'], x['one_hot_vectors'], y['mask_logits'], y['center'], y['heading_bin_id'],
                      y['heading_residual'], y['size_template_id'], y['size_residual'], y['class_id'], params_out, used, *record)
        return out
