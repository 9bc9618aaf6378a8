"""Device-resident datasets: a whole split in device memory, training batches assembled by one kernel (csrc/batch.hip).

Reference: datasets/s3dis.py, datasets/shapenet.py, datasets/kitti/frustum.py -- `Dataset.__getitem__` once per cloud on the host,
then default_collate, pin, copy.  Here a split is packed once (only the valid rows of every item, an int64 offset table, fp32 rows,
labels in the narrowest integer type) and a batch is one launch that writes what one iteration of the reference's `DataLoader` yields,
straight into the tensors it is given -- the static inputs of a captured step, for instance.

Everything about an item that does not depend on a random draw is computed ONCE, on the host, with numpy, in the reference's own
arithmetic, when the store is built (ShapeNet's normalisation; Frustum-KITTI's rotation, centre, size residual, `dist` of the shift and
the heading bin of both flip states).  Per step the kernel draws or takes the choices, gathers, and applies the draw-dependent part.

Two sources of randomness, as `logits_mask` has them:
  * parity mode: the caller hands the draws (`choices` (B, N) int32; ShapeNet `jitter` (B, 3, N) fp64; Frustum `flip` (B) and `shift`
    (B) fp64).  The batch is then bit-identical to the reference's for numpy's draws;
  * device mode (default): a Philox stream keyed by two int64 words drawn from torch's device generator -- no host round trip, fresh
    numbers on every graph replay, `torch.manual_seed` governs it.  Same distributions, other numbers than numpy's.

`assemble_reference` is the torch formulation of each assembly (parity mode only, any device): the definition the kernels are tested
against.  The product path (`assemble`, `DeviceLoader.feed`) needs device tensors and the native library: there is no CPU fallback.
"""

import numpy as np
import torch

from . import augment as _augment
from .modules.functional import backend as _seam

__all__ = ['DeviceS3DIS', 'DeviceShapeNet', 'DeviceFrustumKitti', 'DeviceLoader']


def _numpy(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _default_device(device):
    if device is not None:
        return torch.device(device)
    return torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')


def _narrowest(labels):
    """labels (any integer array) in the narrowest of uint8 / int16 / int32 / int64 that holds them."""
    labels = np.asarray(labels)
    if labels.size == 0:
        return labels.astype(np.uint8)
    return labels.astype(_narrowest_name(int(labels.min()), int(labels.max())))


def _narrowest_name(lo, hi):
    """Name (numpy's and torch's) of the narrowest of uint8 / int16 / int32 / int64 that holds [lo, hi]."""
    for name in ('uint8', 'int16', 'int32'):
        if np.iinfo(name).min <= lo and hi <= np.iinfo(name).max:
            return name
    return 'int64'


class _Store:
    """Packed, ragged, row-major: item i owns rows offsets[i] .. offsets[i + 1] of `rows` (R, C) fp32 and `labels` (R)."""
    channels = 0

    def _pack(self, row_list, label_list, device):
        self.device = _default_device(device)
        counts = [int(r.shape[0]) for r in row_list]
        if not counts:
            raise ValueError('an empty split cannot be stored')
        if min(counts) < 1:
            raise ValueError('every item needs at least one point (numpy cannot choose from an empty item either)')
        offsets = np.zeros(len(counts) + 1, dtype=np.int64)
        np.cumsum(counts, out=offsets[1:])
        self.max_n = max(counts)
        self.offsets = torch.from_numpy(offsets).to(self.device)
        rows = np.concatenate([np.ascontiguousarray(r, dtype=np.float32).reshape(-1, self.channels) for r in row_list])
        self.rows = torch.from_numpy(rows).to(self.device)
        self.labels = None
        if label_list is not None:
            self.labels = torch.from_numpy(_narrowest(np.concatenate([np.asarray(l).reshape(-1) for l in label_list]))).to(self.device)
        self._tables = ['rows', 'labels', 'offsets']

    def __len__(self):
        return self.offsets.numel() - 1

    @property
    def nbytes(self):
        """Bytes of device memory the split takes: R * C * 4 (rows) + R * label width + (W + 1) * 8 (offsets) + the per-item tables."""
        return sum(t.numel() * t.element_size() for t in (getattr(self, k) for k in self._tables) if t is not None)

    def to(self, device):
        """A copy of the store on another device (the torch formulation runs anywhere; `assemble` needs the GPU)."""
        import copy
        other = copy.copy(self)
        other.device = torch.device(device)
        for k in self._tables:
            t = getattr(self, k)
            setattr(other, k, None if t is None else t.to(other.device))
        return other

    def item(self, i):
        """(rows (n, C) fp32, labels (n) or None) of item i, as stored."""
        a, b = int(self.offsets[i]), int(self.offsets[i + 1])
        return self.rows[a:b], None if self.labels is None else self.labels[a:b]

    # -- shared argument handling --
    def _label_bytes(self):
        return 1 if self.labels is None else self.labels.element_size()

    def _indices(self, indices, order, cursor, batch_size):
        if indices is not None:
            order = torch.as_tensor(indices, dtype=torch.int64).to(self.device).reshape(-1).contiguous()
            return order, None, order.numel()
        if order is None or batch_size is None:
            raise ValueError('without `indices`, `order` (int64 device tensor) and `batch_size` are required (DeviceLoader passes them)')
        if order.dtype != torch.int64 or (cursor is not None and (cursor.dtype != torch.int64 or cursor.numel() != 1)):
            raise ValueError('`order` must be an int64 tensor and `cursor` one int64 word')
        return order, cursor, int(batch_size)

    def _reference_items(self, indices):
        idx = torch.as_tensor(indices, dtype=torch.int64).to(self.device).reshape(-1)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= len(self)):
            raise IndexError('item index out of range')
        return idx

    def _reference_rows(self, idx, choices):
        """Global row of every (sample, point): offsets[item] + clamp(choice, 0, n - 1)."""
        if choices is None:
            raise ValueError('the torch formulation is parity mode only: `choices` (B, N) is required')
        choices = torch.as_tensor(choices).to(self.device).long()
        if tuple(choices.shape) != (idx.numel(), self.num_points):
            raise ValueError(f'choices of shape {(idx.numel(), self.num_points)} expected, got {tuple(choices.shape)}')
        start, n = self.offsets[idx], self.offsets[idx + 1] - self.offsets[idx]
        return start[:, None] + torch.minimum(choices.clamp(min=0), (n - 1)[:, None])

    def _draw(self, t, shape, dtype, name):
        if t is None:
            return None
        t = torch.as_tensor(t).to(device=self.device, dtype=dtype).contiguous()
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f'{name} of shape {tuple(shape)} expected, got {tuple(t.shape)}')
        return t

    def _seed(self, seed):
        return _seam.fresh_seed(self.device) if seed is None else _seam.check_seed(seed, self.rows.device)

    def _begin(self, indices, out, order, cursor, batch_size, choices):
        """The shared opening of every `assemble` -> (backend, order, cursor, B, out (checked, or allocated), choices (B, N) int32)."""
        be = self._backend()
        order, cursor, b = self._indices(indices, order, cursor, batch_size)
        if out is None:
            out = self.empty_batch(b)
        else:
            self._check_out(out, self._describe(b))
        return be, order, cursor, b, out, self._draw(choices, (b, self.num_points), torch.int32, 'choices')

    @staticmethod
    def _parity(choices, **draws):
        """The rule of parity mode: with `choices` every needed draw is present, without it none is.  draws: name -> (tensor, needed)."""
        names = ' / '.join(f'`{k}`' for k in draws)
        if choices is None and any(t is not None for t, _ in draws.values()):
            raise ValueError(f'{names} draws without `choices`: parity mode takes every draw from the caller')
        if choices is not None and any(needed and t is None for t, needed in draws.values()):
            raise ValueError(f'parity mode takes every draw from the caller: {names} fp64 are missing')

    def _backend(self):
        be = _seam._backend
        if self.device.type != 'cuda' or not getattr(be, 'has_batch_assembly', False):
            raise RuntimeError('batch assembly needs a CUDA (HIP) store and the native library -- there is no CPU implementation; '
                               '`assemble_reference` is the torch formulation')
        return be

    def _check_out(self, out, like):
        """`out` must have the structure, shapes, dtypes and device of `like` (a freshly described batch)."""
        flat_o, flat_l = _flatten(out), _flatten(like)
        if [k for k, _ in flat_o] != [k for k, _ in flat_l]:
            raise ValueError(f'out= must have the structure {[k for k, _ in flat_l]}')
        for (k, o), (_, (shape, dtype)) in zip(flat_o, flat_l):
            if tuple(o.shape) != tuple(shape) or o.dtype != dtype or o.device != self.device or not o.is_contiguous():
                raise ValueError(f'out[{k}]: contiguous {dtype} tensor of shape {tuple(shape)} on {self.device} expected')

    def empty_batch(self, batch_size):
        """Uninitialised tensors with the structure of one batch (what `out=` takes; the static inputs of a captured step)."""
        return _build(self._describe(int(batch_size)), lambda sd: torch.empty(sd[0], dtype=sd[1], device=self.device))


def _flatten(batch):
    out = []
    for i, part in enumerate(batch):
        if isinstance(part, dict):
            out += [(f'{i}.{k}', v) for k, v in part.items()]
        else:
            out.append((str(i), part))
    return out


def _build(desc, make):
    return tuple({k: make(v) for k, v in part.items()} if isinstance(part, dict) else make(part) for part in desc)


# ------------------------------------------------------------------------------------------------------------------- S3DIS
class DeviceS3DIS(_Store):
    """The windows of an S3DIS split (datasets/s3dis.py).  data (W, P, 9) any float dtype, label_seg (W, P), data_num (W,): only the
    first data_num[w] rows of window w are kept.  One batch = (features (B, 9 or 6, N) fp32, targets (B, N) int64)."""
    channels = 9

    def __init__(self, data, label_seg, data_num, num_points, with_normalized_coords=True, device=None):
        data, label_seg, data_num = _numpy(data), _numpy(label_seg), _numpy(data_num).reshape(-1)
        if data.ndim != 3 or data.shape[2] != 9:
            raise ValueError(f'data (W, P, 9) expected, got {data.shape}')
        if label_seg.shape != data.shape[:2] or data_num.shape[0] != data.shape[0]:
            raise ValueError('label_seg (W, P) and data_num (W,) must match data (W, P, 9)')
        if int(num_points) < 1:
            raise ValueError('num_points must be positive')
        if data_num.size and (data_num.min() < 1 or data_num.max() > data.shape[1]):
            raise ValueError('data_num must lie in [1, P]')
        self.num_points, self.with_normalized_coords = int(num_points), bool(with_normalized_coords)
        # the reference: np.array(scene_data[i]).astype(np.float32), np.array(scene_label[i]).astype(np.int64)
        self._pack([data[w, :int(data_num[w])].astype(np.float32) for w in range(data.shape[0])],
                   [label_seg[w, :int(data_num[w])].astype(np.int64) for w in range(data.shape[0])], device)

    @classmethod
    def from_dataset(cls, ds, device=None):
        """From the reference's `_S3DISDataset`: reads the h5 files of ds.scene_list in index order."""
        import h5py                                 # not an import-time dependency
        data, label, num = [], [], []
        for files in ds.scene_list.values():
            for name in files:
                with h5py.File(name, 'r') as h5f:
                    data.append(np.array(h5f['data'])); label.append(np.array(h5f['label_seg'])); num.append(np.array(h5f['data_num']))
        return cls(np.concatenate(data), np.concatenate(label), np.concatenate(num), ds.num_points,
                   with_normalized_coords=ds.with_normalized_coords, device=device)

    @classmethod
    def from_rooms(cls, windows, num_points, with_normalized_coords=True):
        """From `rooms.prepare_room` results (one `RoomWindows` or a list of them, every one with labels, on one device): the packed
        tables are concatenated on the device, in list order -- no numpy round trip.  The store equals the one the constructor builds
        from the same windows' padded h5 arrays."""
        windows = [windows] if hasattr(windows, 'rows') else list(windows)
        if not windows:
            raise ValueError('an empty split cannot be stored')
        if any(w.labels is None for w in windows):
            raise ValueError('every room needs labels (prepare_room(xyzrgb, labels))')
        if int(num_points) < 1:
            raise ValueError('num_points must be positive')
        device = windows[0].rows.device
        if device.type != 'cuda' or any(w.rows.device != device for w in windows):
            raise RuntimeError('from_rooms needs the windows of every room on one CUDA (HIP) device -- there is no CPU implementation')
        self = cls.__new__(cls)
        self.num_points, self.with_normalized_coords, self.device = int(num_points), bool(with_normalized_coords), device
        counts = torch.cat([w.offsets[1:] - w.offsets[:-1] for w in windows])
        self.offsets = torch.cat([torch.zeros((1,), dtype=torch.int64, device=device), torch.cumsum(counts, 0)])
        self.rows = torch.cat([w.rows for w in windows]).contiguous()
        labels = torch.cat([w.labels for w in windows])
        self.max_n, lo, hi = (int(v) for v in torch.stack([counts.max(), labels.min(), labels.max()]).tolist())
        self.labels = labels.to(getattr(torch, _narrowest_name(lo, hi))).contiguous()
        self._tables = ['rows', 'labels', 'offsets']
        return self

    @property
    def out_channels(self):
        return 9 if self.with_normalized_coords else 6

    def _describe(self, b):
        return (((b, self.out_channels, self.num_points), torch.float32), ((b, self.num_points), torch.int64))

    def assemble_reference(self, indices, *, choices=None, jitter=None, flip=None, shift=None):
        rows = self._reference_rows(self._reference_items(indices), choices)
        features = self.rows[rows].permute(0, 2, 1)[:, :self.out_channels].contiguous()
        return features, self.labels[rows].to(torch.int64)

    def assemble(self, indices=None, out=None, *, choices=None, jitter=None, flip=None, shift=None, seed=None, order=None, cursor=None,
                 batch_size=None):
        be, order, cursor, b, out, choices = self._begin(indices, out, order, cursor, batch_size, choices)
        if choices is None and self.max_n >= self.num_points and self.max_n > 8192:
            raise RuntimeError(f'sampling {self.num_points} of up to {self.max_n} points without replacement: the selection is '
                               'resident in LDS and holds at most 8192 points per window')
        be.batch_launch('batch_s3dis', self.rows, self.rows, self.labels, self._label_bytes(), self.offsets, len(self), self.max_n,
                        order, order.numel(), cursor, b, self.num_points, self.out_channels, choices,
                        None if choices is not None else self._seed(seed), out[0], out[1])
        return out


# ---------------------------------------------------------------------------------------------------------------- ShapeNet
class DeviceShapeNet(_Store):
    """A ShapeNet-part split (datasets/shapenet.py).  clouds: a list of (n_i, 7) arrays as np.loadtxt returns them (xyz, normal,
    part label); shape_ids: one per cloud.  One batch = (features (B, 3 [+3] [+16], N) fp32, targets (B, N) int64)."""
    channels = 6
    num_shapes = 16

    def __init__(self, clouds, shape_ids, num_points, with_normal=True, with_one_hot_shape_id=True, normalize=True, jitter=True,
                 device=None):
        shape_ids = self._configure(len(clouds), shape_ids, num_points, with_normal, with_one_hot_shape_id, normalize, jitter)
        rows, labels = [], []
        for cloud in clouds:
            cloud = _numpy(cloud)
            if cloud.ndim != 2 or cloud.shape[1] != 7:
                raise ValueError(f'clouds of shape (n, 7) expected, got {cloud.shape}')
            data = cloud.astype(np.float32)
            coords = data[:, :3]
            if self.normalize:
                coords = self.normalize_point_cloud(coords)
            rows.append(np.concatenate([coords, data[:, 3:6]], axis=1))
            labels.append(data[:, -1].astype(np.int64))
        self._pack_shapes(rows, labels, shape_ids, device)

    def _configure(self, num_clouds, shape_ids, num_points, with_normal, with_one_hot_shape_id, normalize, jitter):
        """The checks and the flags every way of building the store shares -> shape_ids (W,) int64 numpy."""
        shape_ids = np.asarray(shape_ids, dtype=np.int64).reshape(-1)
        if num_clouds != shape_ids.shape[0]:
            raise ValueError('one shape id per cloud expected')
        if shape_ids.size and (shape_ids.min() < 0 or shape_ids.max() >= self.num_shapes):
            raise ValueError(f'shape ids must lie in [0, {self.num_shapes})')
        if int(num_points) < 1:
            raise ValueError('num_points must be positive')
        self.num_points = int(num_points)
        self.with_normal, self.with_one_hot_shape_id = bool(with_normal), bool(with_one_hot_shape_id)
        self.normalize, self.jitter = bool(normalize), bool(jitter)
        return shape_ids

    def _pack_shapes(self, rows, labels, shape_ids, device):
        self._pack(rows, labels, device)
        self.shape_ids = torch.from_numpy(shape_ids.astype(np.int32)).to(self.device)
        self._tables = self._tables + ['shape_ids']

    @classmethod
    def from_clouds(cls, clouds, labels, shape_ids, num_points, *, k=16, orient='outward', with_normal=True,
                    with_one_hot_shape_id=True, normalize=True, jitter=True, device=None):
        """From raw clouds WITHOUT normals: clouds[i] (n_i, 3) xyz, labels[i] (n_i,) part labels, one shape id per cloud.  The
        coordinates are normalised on the host exactly as the constructor normalises them; the normals of the whole split are then
        computed on the packed rows by ONE k_nearest launch and ONE shape_normals launch (pvcnn_amd.shapes: PCA over the k nearest
        points, oriented by `orient`; 'outward' adds the centroid launch) and written into the store's normal columns.  The store is the
        one the constructor builds from the (n_i, 7) arrays [xyz, those normals, label]: `assemble`, `DeviceLoader` and `Augment` work
        on it unchanged.  with_normal=False stores zero normals (nothing reads them) and launches nothing.  A store on the CPU takes
        the torch formulation of the same definitions."""
        from . import shapes as _shapes
        if len(labels) != len(clouds):
            raise ValueError('one label array per cloud expected')
        self = cls.__new__(cls)
        shape_ids = self._configure(len(clouds), shape_ids, num_points, with_normal, with_one_hot_shape_id, normalize, jitter)
        k = _shapes._check_k(k)
        rows, label_list = [], []
        for cloud, label in zip(clouds, labels):
            cloud, label = _numpy(cloud), _numpy(label).reshape(-1)
            if cloud.ndim != 2 or cloud.shape[1] != 3:
                raise ValueError(f'clouds of shape (n, 3) expected, got {cloud.shape}')
            if label.shape[0] != cloud.shape[0]:
                raise ValueError(f'{cloud.shape[0]} labels expected, got {label.shape[0]}')
            data = np.zeros((cloud.shape[0], 7), dtype=np.float32)          # the constructor's array: same layout, same arithmetic
            data[:, :3] = cloud
            coords = data[:, :3]
            if self.normalize:
                coords = self.normalize_point_cloud(coords)
            rows.append(np.concatenate([coords, data[:, 3:6]], axis=1))
            label_list.append(label.astype(np.float32).astype(np.int64))    # (labels reach the constructor through the fp32 array)
        self._pack_shapes(rows, label_list, shape_ids, device)
        if self.with_normal:
            host = self.offsets.cpu().numpy() if self.offsets.is_cuda else self.offsets.numpy()
            _shapes._check_sizes(host, _shapes.MAX_CLOUD_POINTS)
            normals, _ = _shapes._normals_packed(self.rows, self.offsets, host, k, orient)
            self.rows[:, 3:6] = normals
        return self

    @staticmethod
    def normalize_point_cloud(points):
        """shapenet.py:86-90, in numpy and fp32 like the reference (which caches the result per item as well)."""
        centroid = np.mean(points, axis=0)
        points = points - centroid
        return points / np.max(np.linalg.norm(points, axis=1))

    @classmethod
    def from_dataset(cls, ds, device=None):
        """From the reference's `_ShapeNetDataset`: loads every text file of ds.file_paths."""
        return cls([np.loadtxt(path) for path, _ in ds.file_paths], [sid for _, sid in ds.file_paths], ds.num_points,
                   with_normal=ds.with_normal, with_one_hot_shape_id=ds.with_one_hot_shape_id, normalize=ds.normalize,
                   jitter=ds.jitter, device=device)

    @property
    def out_channels(self):
        return 3 + (3 if self.with_normal else 0) + (self.num_shapes if self.with_one_hot_shape_id else 0)

    def _describe(self, b):
        return (((b, self.out_channels, self.num_points), torch.float32), ((b, self.num_points), torch.int64))

    def assemble_reference(self, indices, *, choices=None, jitter=None, flip=None, shift=None):
        idx = self._reference_items(indices)
        rows = self._reference_rows(idx, choices)
        picked = self.rows[rows].permute(0, 2, 1)                               # (B, 6, N)
        coords = picked[:, :3]
        if self.jitter:
            if jitter is None:
                raise ValueError('the torch formulation needs the `jitter` draws (B, 3, N) fp64 of a jittering split')
            z = self._draw(jitter, (idx.numel(), 3, self.num_points), torch.float64, 'jitter')
            coords = (0.01 * z).clamp(-0.05, 0.05).to(torch.float32) + coords
        parts = [coords]
        if self.with_normal:
            parts.append(picked[:, 3:6])
        if self.with_one_hot_shape_id:
            hot = torch.zeros((idx.numel(), self.num_shapes, self.num_points), dtype=torch.float32, device=self.device)
            hot[torch.arange(idx.numel(), device=self.device), self.shape_ids[idx].long()] = 1.0
            parts.append(hot)
        return torch.cat(parts, dim=1).contiguous(), self.labels[rows].to(torch.int64)

    def assemble(self, indices=None, out=None, *, choices=None, jitter=None, flip=None, shift=None, seed=None, order=None, cursor=None,
                 batch_size=None):
        be, order, cursor, b, out, choices = self._begin(indices, out, order, cursor, batch_size, choices)
        jitter = self._draw(jitter, (b, 3, self.num_points), torch.float64, 'jitter')
        self._parity(choices, jitter=(jitter, self.jitter))
        be.batch_launch('batch_shapenet', self.rows, self.rows, self.labels, self._label_bytes(), self.offsets, len(self),
                        self.shape_ids, order, order.numel(), cursor, b, self.num_points, int(self.with_normal),
                        self.num_shapes if self.with_one_hot_shape_id else 0, int(self.jitter), choices, jitter,
                        None if choices is not None else self._seed(seed), out[0], out[1])
        return out


# ----------------------------------------------------------------------------------------------------------- Frustum-KITTI
def rotate_points_along_y(features, rotation_angle):
    """kitti/frustum.py:150-164 in the reference's arithmetic (fp64 cosine / sine, a BLAS product, written back in the array's type)."""
    v_cos = np.cos(rotation_angle)
    v_sin = np.sin(rotation_angle)
    features[:, [0, 2]] = np.dot(features[:, [0, 2]], [[v_cos, v_sin], [-v_sin, v_cos]])
    return features


def angle_to_bin_id(angle, num_angle_bins):
    """kitti/frustum.py:167-183: (bin id, residual) with bin_id * (2 pi / N) + residual = angle."""
    angle = angle % (2 * np.pi)
    angle_per_bin = 2 * np.pi / float(num_angle_bins)
    shifted_angle = (angle + angle_per_bin / 2) % (2 * np.pi)
    bin_id = int(shifted_angle / angle_per_bin)
    return bin_id, shifted_angle - (bin_id * angle_per_bin + angle_per_bin / 2)


class DeviceFrustumKitti(_Store):
    """A Frustum-KITTI split (datasets/kitti/frustum.py) from the arrays of its pickle.  One batch = (inputs dict, targets dict) as the
    reference's DataLoader collates them.  Point clouds are held in fp32 (the prepared KITTI pickles store fp32; a cloud of another
    type is cast when the store is built, where the reference would carry it through flip and shift and cast last).
    `size_templates`: class name -> (3,) template (kitti_attributes.class_name_to_size_template)."""
    channels = 4

    def __init__(self, point_clouds, mask_logits, boxes_3d, heading_angles, sizes, class_names, frustum_rotation_angles, num_points,
                 classes=('Car', 'Pedestrian', 'Cyclist'), num_heading_angle_bins=12, class_name_to_size_template_id=None,
                 size_templates=None, random_flip=False, random_shift=False, frustum_rotate=False, device=None, _rgb_probs=None):
        self.rgb_detection = _rgb_probs is not None
        w = len(point_clouds)
        lists = [class_names, frustum_rotation_angles] + ([_rgb_probs] if self.rgb_detection else
                                                          [mask_logits, boxes_3d, heading_angles, sizes])
        if any(len(x) != w for x in lists):
            raise ValueError('every per-item list must have one entry per point cloud')
        if int(num_points) < 1:
            raise ValueError('num_points must be positive')
        self.num_points, self.classes = int(num_points), tuple(classes)
        self.num_classes = k = len(self.classes)
        self.num_heading_angle_bins = int(num_heading_angle_bins)
        self.random_flip, self.random_shift = bool(random_flip), bool(random_shift)
        self.frustum_rotate = bool(frustum_rotate)
        class_id = {c: i for i, c in enumerate(self.classes)}
        if any(c not in class_id for c in class_names):
            raise ValueError(f'class names must be among {self.classes}')
        if not self.rgb_detection:
            if class_name_to_size_template_id is None or size_templates is None:
                raise ValueError('class_name_to_size_template_id and size_templates are required with ground truth')
        rows, labels = [], []
        tables = self._new_item_tables(w)
        for i in range(w):
            rotation_angle = self._fill_item(tables, i, class_names[i], frustum_rotation_angles[i], class_id,
                                             None if self.rgb_detection else (boxes_3d[i], heading_angles[i], sizes[i]),
                                             _rgb_probs[i] if self.rgb_detection else None, class_name_to_size_template_id, size_templates)
            cloud = np.asarray(point_clouds[i])
            if cloud.ndim != 2 or cloud.shape[1] != 4:
                raise ValueError(f'point clouds of shape (n, 4) expected, got {cloud.shape}')
            cloud = cloud.astype(np.float32) if cloud.dtype != np.float32 else cloud
            if self.frustum_rotate:
                cloud = rotate_points_along_y(np.copy(cloud), rotation_angle)
            rows.append(cloud)
            if not self.rgb_detection:
                labels.append(np.asarray(mask_logits[i]).astype(np.int64))
        self._pack(rows, None if self.rgb_detection else labels, device)
        self._upload_item_tables(tables)

    def _new_item_tables(self, w):
        k = self.num_classes
        return (np.zeros((w, 1 if self.rgb_detection else 4), dtype=np.float64),
                np.zeros((w, k + (1 if self.rgb_detection else 5)), dtype=np.float32), np.zeros((w, 4), dtype=np.int64))

    def _fill_item(self, tables, i, name, frustum_rotation_angle, class_id, truth, prob, class_name_to_size_template_id, size_templates):
        """Row i of the per-item tables: everything about an item that no draw decides, in the reference's arithmetic.  truth:
        (corners (8, 3), heading angle, size) or None (the detection form, with `prob`).  -> the item's rotation angle."""
        f64, f32, i64 = tables
        k = self.num_classes
        rotation_angle = np.pi / 2.0 + frustum_rotation_angle
        f32[i, class_id[name]] = 1
        if truth is None:
            f32[i, k] = np.asarray(rotation_angle).astype(np.float32)
            f64[i, 0] = prob
            return rotation_angle
        box_3d, heading_angle, size = truth
        center = (box_3d[0, :] + box_3d[6, :]) / 2.0
        if self.frustum_rotate:
            center = rotate_points_along_y(np.expand_dims(center, 0), rotation_angle).squeeze()
            heading_angle = heading_angle - rotation_angle
        f64[i, :3] = center
        f64[i, 3] = np.sqrt(np.sum(center[0] ** 2 + center[1] ** 2))
        for fl, angle in enumerate((heading_angle, np.pi - heading_angle)):
            i64[i, fl], residual = angle_to_bin_id(angle, self.num_heading_angle_bins)
            f32[i, k + fl] = np.array(residual, dtype=np.float32)
        f32[i, k + 2:k + 5] = (np.asarray(size) - np.asarray(size_templates[name])).astype(np.float32)
        i64[i, 2], i64[i, 3] = class_name_to_size_template_id[name], class_id[name]
        return rotation_angle

    def _upload_item_tables(self, tables):
        f64, f32, i64 = tables
        self.item_f64, self.item_f32 = torch.from_numpy(f64).to(self.device), torch.from_numpy(f32).to(self.device)
        self.item_i64 = None if self.rgb_detection else torch.from_numpy(i64).to(self.device)
        self._tables = self._tables + ['item_f64', 'item_f32', 'item_i64']

    @classmethod
    def from_frustums(cls, frames, num_points, classes=('Car', 'Pedestrian', 'Cyclist'), num_heading_angle_bins=12,
                      class_name_to_size_template_id=None, size_templates=None, random_flip=False, random_shift=False,
                      frustum_rotate=False):
        """From `frames.extract_frustums` results (one `FrameFrustums` or a list, all with or all without ground truth, on one
        device): rows, labels and offsets are concatenated on the device in list order -- the points never visit the host -- and the
        per-item tables come from the frames' small host arrays through the constructor's own code.  With frustum_rotate the packed
        rows are rotated by one launch (csrc/frames.hip) in the elementwise fp64 form x' = x c + z (-s), z' = x s + z c, rounded once:
        within one fp32 ulp of the constructor's BLAS product.  Serves the ground-truth form and the rgb-detection form."""
        frames = [frames] if hasattr(frames, 'rows') else list(frames)
        frames = [f for f in frames if len(f)]
        if not frames:
            raise ValueError('an empty split cannot be stored')
        truth = frames[0].labels is not None
        if any((f.labels is not None) != truth for f in frames):
            raise ValueError('frames with and without ground truth cannot share a store')
        if int(num_points) < 1:
            raise ValueError('num_points must be positive')
        device = frames[0].rows.device
        if device.type != 'cuda' or any(f.rows.device != device for f in frames):
            raise RuntimeError('from_frustums needs the frustums of every frame on one CUDA (HIP) device -- there is no CPU implementation')
        self = cls.__new__(cls)
        self.rgb_detection = not truth
        self.num_points, self.classes, self.device = int(num_points), tuple(classes), device
        self.num_classes = len(self.classes)
        self.num_heading_angle_bins = int(num_heading_angle_bins)
        self.random_flip, self.random_shift = bool(random_flip), bool(random_shift)
        self.frustum_rotate = bool(frustum_rotate)
        class_id = {c: i for i, c in enumerate(self.classes)}
        names = [n for f in frames for n in f.class_names]
        if any(c not in class_id for c in names):
            raise ValueError(f'class names must be among {self.classes}')
        if truth and (class_name_to_size_template_id is None or size_templates is None):
            raise ValueError('class_name_to_size_template_id and size_templates are required with ground truth')
        w = len(names)
        tables = self._new_item_tables(w)
        cos_sin = np.zeros((w, 2), dtype=np.float64)
        i = 0
        for f in frames:
            for j in range(len(f)):
                rotation_angle = self._fill_item(tables, i, f.class_names[j], f.frustum_angles[j], class_id,
                                                 (f.boxes_3d[j], f.heading_angles[j], f.sizes[j]) if truth else None,
                                                 None if truth else f.scores[j], class_name_to_size_template_id, size_templates)
                cos_sin[i] = np.cos(rotation_angle), np.sin(rotation_angle)
                i += 1
        counts = np.concatenate([np.asarray(f.counts, dtype=np.int64) for f in frames])
        offsets = np.zeros(w + 1, dtype=np.int64)
        np.cumsum(counts, out=offsets[1:])
        self.max_n = int(counts.max())
        self.offsets = torch.from_numpy(offsets).to(device)
        self.rows = torch.cat([f.rows for f in frames]).contiguous()
        self.labels = torch.cat([f.labels for f in frames]).contiguous() if truth else None
        if self.rows.shape[0] != int(offsets[-1]):
            raise ValueError('the frames\' counts do not add up to their rows')
        if self.frustum_rotate:
            _seam._device_call('frame_rotate_rows', self.rows, self.rows, self.rows.shape[0], self.offsets, w, torch.from_numpy(cos_sin).to(device))
        self._tables = ['rows', 'labels', 'offsets']
        self._upload_item_tables(tables)
        return self

    @classmethod
    def from_rgb_detection(cls, point_clouds, class_names, frustum_rotation_angles, probs, num_points,
                           classes=('Car', 'Pedestrian', 'Cyclist'), frustum_rotate=False, device=None):
        """The detection form (no ground truth): targets are {'rotation_angle', 'rgb_score'}."""
        return cls(point_clouds, None, None, None, None, class_names, frustum_rotation_angles, num_points, classes=classes,
                   frustum_rotate=frustum_rotate, device=device, _rgb_probs=list(probs))

    @classmethod
    def from_dataset(cls, ds, size_templates=None, device=None):
        """From the reference's `_FrustumKittiDataset` (reads ds.data.*).  size_templates: kitti_attributes.class_name_to_size_template."""
        d = ds.data
        if ds.from_rgb_detection:
            return cls.from_rgb_detection(d.point_clouds, d.class_names, d.frustum_rotation_angles, d.probs, ds.num_points,
                                          classes=ds.classes, frustum_rotate=ds.frustum_rotate, device=device)
        return cls(d.point_clouds, d.mask_logits, d.boxes_3d, d.heading_angles, d.sizes, d.class_names, d.frustum_rotation_angles,
                   ds.num_points, classes=ds.classes, num_heading_angle_bins=ds.num_heading_angle_bins,
                   class_name_to_size_template_id=ds.class_name_to_size_template_id, size_templates=size_templates,
                   random_flip=ds.random_flip, random_shift=ds.random_shift, frustum_rotate=ds.frustum_rotate, device=device)

    def _describe(self, b):
        n, k, f, i = self.num_points, self.num_classes, torch.float32, torch.int64
        inputs = {'features': ((b, 4, n), f), 'one_hot_vectors': ((b, k), f)}
        if self.rgb_detection:
            return inputs, {'rotation_angle': ((b,), f), 'rgb_score': ((b,), torch.float64)}
        return inputs, {'mask_logits': ((b, n), i), 'center': ((b, 3), f), 'heading_bin_id': ((b,), i), 'heading_residual': ((b,), f),
                        'size_template_id': ((b,), i), 'size_residual': ((b, 3), f), 'class_id': ((b,), i)}

    def assemble_reference(self, indices, *, choices=None, jitter=None, flip=None, shift=None):
        idx = self._reference_items(indices)
        b, k = idx.numel(), self.num_classes
        rows = self._reference_rows(idx, choices)
        features = self.rows[rows].permute(0, 2, 1).contiguous()               # (B, 4, N)
        f32 = self.item_f32[idx]
        inputs = {'features': features, 'one_hot_vectors': f32[:, :k].contiguous()}
        if self.rgb_detection:
            return inputs, {'rotation_angle': f32[:, k].contiguous(), 'rgb_score': self.item_f64[idx, 0].contiguous()}
        f64, i64 = self.item_f64[idx], self.item_i64[idx]
        center = f64[:, :3].clone()
        flipped = torch.zeros(b, dtype=torch.bool, device=self.device)
        if self.random_flip:
            if flip is None:
                raise ValueError('the torch formulation needs the `flip` draws (B) fp64 of a flipping split')
            flipped = self._draw(flip, (b,), torch.float64, 'flip') > 0.5
            features[:, 0] = torch.where(flipped[:, None], -features[:, 0], features[:, 0])
            center[:, 0] = torch.where(flipped, -center[:, 0], center[:, 0])
        if self.random_shift:
            if shift is None:
                raise ValueError('the torch formulation needs the `shift` draws (B) fp64 of a shifting split')
            dist = f64[:, 3]
            # the reference's expression as written: np.clip(randn() * dist * 0.05, dist * 0.8, dist * 1.2)
            s = torch.clamp(self._draw(shift, (b,), torch.float64, 'shift') * dist * 0.05, min=dist * 0.8, max=dist * 1.2)
            features[:, 2] = (features[:, 2].to(torch.float64) + s[:, None]).to(torch.float32)
            center[:, 2] = center[:, 2] + s
        fl = flipped.long()[:, None]
        return inputs, {'mask_logits': self.labels[rows].to(torch.int64), 'center': center.to(torch.float32),
                        'heading_bin_id': i64[:, :2].gather(1, fl)[:, 0], 'heading_residual': f32[:, k:k + 2].gather(1, fl)[:, 0],
                        'size_template_id': i64[:, 2].contiguous(), 'size_residual': f32[:, k + 2:k + 5].contiguous(),
                        'class_id': i64[:, 3].contiguous()}

    def assemble(self, indices=None, out=None, *, choices=None, jitter=None, flip=None, shift=None, seed=None, order=None, cursor=None,
                 batch_size=None):
        be, order, cursor, b, out, choices = self._begin(indices, out, order, cursor, batch_size, choices)
        seed = None if choices is not None else self._seed(seed)
        x, y = out
        if self.rgb_detection:
            be.batch_launch('batch_frustum_rgb', self.rows, self.rows, self.offsets, len(self), self.item_f64, self.item_f32,
                            self.num_classes, order, order.numel(), cursor, b, self.num_points, choices, seed, x['features'],
                            x['one_hot_vectors'], y['rotation_angle'], y['rgb_score'])
            return out
        flip, shift = self._draw(flip, (b,), torch.float64, 'flip'), self._draw(shift, (b,), torch.float64, 'shift')
        self._parity(choices, flip=(flip, self.random_flip), shift=(shift, self.random_shift))
        be.batch_launch('batch_frustum', self.rows, self.rows, self.labels, self._label_bytes(), self.offsets, len(self), self.item_f64,
                        self.item_f32, self.item_i64, self.num_classes, int(self.random_flip), int(self.random_shift), order,
                        order.numel(), cursor, b, self.num_points, choices, flip, shift, seed, x['features'], x['one_hot_vectors'],
                        y['mask_logits'], y['center'], y['heading_bin_id'], y['heading_residual'], y['size_template_id'],
                        y['size_residual'], y['class_id'])
        return out


# ------------------------------------------------------------------------------------------------------------------ loader
class DeviceLoader:
    """`DataLoader(dataset, batch_size, shuffle, drop_last)` over a device store: iterable, `len()` as DataLoader's, yields device
    batches.  The epoch's permutation (`order`, a device torch.randperm) and the position in it (`cursor`, one int64 word) live in
    device memory, so a captured `feed()` walks the epoch on replay:

        loader = DeviceLoader(store, 16, drop_last=True)
        x, y = loader.static_batch()                       # the static inputs of the step
        step = GraphedTrainStep(model, lambda: (loader.feed(), criterion(model(x), y))[1], ...)
        for epoch in ...:
            loader.new_epoch()
            for _ in range(len(loader)): step()

    `rank` / `world_size` keep every world_size-th item of the permutation (a data-parallel rank's share).

    `augment` (an `augment.Augment`; S3DIS and ShapeNet stores): every batch is assembled into a private staging batch and augmented
    from there into the batch handed out -- features and targets, two more launches per `feed()`, captured with the step and keyed
    by the same seed words as the assembly.  Without it nothing changes: the same launches, the same tensors, the same bits."""

    def __init__(self, store, batch_size, shuffle=True, drop_last=False, generator=None, rank=0, world_size=1, augment=None):
        if int(batch_size) < 1:
            raise ValueError('batch_size must be positive')
        if not 0 <= int(rank) < int(world_size):
            raise ValueError('rank must lie in [0, world_size)')
        if augment is not None:
            if isinstance(store, DeviceFrustumKitti):
                raise ValueError('a Frustum-KITTI store cannot be augmented: its targets hold box geometry (centre, heading, size) that '
                                 'a generic transform of the points would silently invalidate; the dataset has its own flip and shift')
            augment.check_channels(store.out_channels)
        self.augment, self._staging, self._augment_params = augment, None, None
        self.store, self.batch_size, self.shuffle, self.drop_last = store, int(batch_size), bool(shuffle), bool(drop_last)
        self.generator, self.rank, self.world_size = generator, int(rank), int(world_size)
        self.num_items = len(range(self.rank, len(store), self.world_size))
        dev = store.device
        self.order = torch.arange(self.rank, len(store), self.world_size, dtype=torch.int64, device=dev)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=dev)
        self.seed = torch.zeros(2, dtype=torch.int64, device=dev)
        self._static = None
        if self.shuffle:
            self.new_epoch()

    def __len__(self):
        return self.num_items // self.batch_size if self.drop_last else -(-self.num_items // self.batch_size)

    def batch_sizes(self):
        """The size of every batch of an epoch (the last one is ragged unless drop_last)."""
        return [min(self.batch_size, self.num_items - i * self.batch_size) for i in range(len(self))]

    def new_epoch(self):
        """Reshuffle into the same `order` tensor and zero the cursor (no host synchronisation with a device generator)."""
        if self.shuffle:
            gdev = self.generator.device if self.generator is not None else self.order.device
            perm = torch.randperm(len(self.store), generator=self.generator, device=gdev)
            self.order.copy_(perm[self.rank::self.world_size])
        self.cursor.zero_()

    def static_batch(self):
        """Allocate (once) and return the static tensors `feed()` writes into."""
        if self._static is None:
            self._static = self.store.empty_batch(self.batch_size)
        return self._static

    def feed(self, *, choices=None, jitter=None, flip=None, shift=None, seed=None):
        """One assembly of the next `batch_size` items of the epoch into the static batch; advances the cursor on the device.  Inside
        a graph capture (the `loss_fn` of GraphedTrainStep) it is captured with the step; that needs drop_last=True -- the ragged last
        batch of drop_last=False goes through `__iter__` and the step's eager path."""
        out = self.static_batch()
        if seed is None and (choices is None or self.augment is not None):
            seed = _seam.fresh_seed(self.seed.device, out=self.seed)
        into = out
        if self.augment is not None:
            if self._staging is None:
                self._staging = self.store.empty_batch(self.batch_size)
                self._augment_params = torch.empty((self.batch_size, _augment.PARAMS), dtype=torch.float64, device=self.store.device)
            into = self._staging
        self.store.assemble(None, into, choices=choices, jitter=jitter, flip=flip, shift=shift, seed=seed, order=self.order,
                            cursor=self.cursor, batch_size=self.batch_size)
        if self.augment is not None:
            self.augment.augment(into[0], into[1], out=out[0], out_targets=out[1], seed=seed, params_out=self._augment_params)
        self.cursor.add_(self.batch_size)
        return out

    def __iter__(self):
        self.new_epoch()
        for size in self.batch_sizes():
            batch = self.store.assemble(None, None, order=self.order, cursor=self.cursor, batch_size=size)
            if self.augment is not None:
                batch = self.augment.augment(batch[0], batch[1])
            self.cursor.add_(size)
            yield batch
