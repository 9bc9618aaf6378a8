"""ShapeNet shapes on the device: a raw xyz cloud -> surface normals -> the model's input -> per-point part labels (csrc/shapes.hip).

Reference: every ShapeNet configuration has `with_normal = True` (configs/shapenet/__init__.py), so the networks read xyz, a surface
normal and a one-hot shape id per point -- and only the benchmark's pre-computed text files carry those normals (datasets/shapenet.py
reads columns 3..5).  A scanned object of one's own has xyz only.  Here the normals are computed:

    k_nearest        the k nearest points of every point inside its own cloud: exact, exhaustive, ties broken by position
    estimate_normals the eigenvector of the smallest eigenvalue of the neighbours' covariance (PCA), oriented outward from the
                     cloud's centroid or towards a viewpoint
    prepare_shape    xyz -> the (n, 6) rows [normalised coordinates, normal] a ShapeNet model is fed from
    segment_shape    xyz + shape id -> per-point part labels (the per-shape vote of evaluate/shapenet/eval.py)

and `data.DeviceShapeNet.from_clouds` builds a training store from xyz clouds.  The definitions are in include/pvcnn_hip.h ("Shapes on
the device") and restated in numpy by tests/shapes_truth.py.  All of them work on packed ragged clouds: rows (R, >= 3) fp32 with xyz in
the first three columns and `offsets` (W + 1,), cloud w owning rows offsets[w] .. offsets[w + 1] -- the layout of `data._Store`; a
whole split is two launches.

Device tensors (and numpy arrays, uploaded once when a GPU is present) take the kernels.  CPU tensors take a torch formulation of the
same definitions: the neighbour table is the same bit for bit (separate tensor operations round as the kernel's separate instructions
do), the normals agree within the solver's accuracy.  The search is exhaustive, O(n^2) per cloud: `max_cloud_points` bounds n -- a
stated limit, not a kernel's.
"""
import numpy as np
import torch

from . import meters as _meters
from .data import DeviceShapeNet, _default_device
from .evaluate import ShapeVotes, shapenet_shape_votes
from .modules.functional import backend as _seam

__all__ = ['k_nearest', 'estimate_normals', 'prepare_shape', 'segment_shape', 'shape_part_classes', 'MAX_K', 'MAX_CLOUD_POINTS']

MAX_K = 64                     # PVCNN_K_NEAREST_MAX_K: lane l of a wave holds the l-th nearest
MAX_CLOUD_POINTS = 131072      # default bound of one cloud's points (131072^2 = 1.7e10 distances)
_MODES = {None: 0, 'outward': 1, 'viewpoint': 2}
_CHUNK = 1 << 22               # distances per step of the torch formulation


def _rows(points):
    """(R, >= 3) fp32 rows on the device they live on; numpy is uploaded once (to the GPU when there is one)."""
    if isinstance(points, torch.Tensor):
        x = points
    else:
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(points), dtype=np.float32)).to(_default_device(None))
    if x.dim() != 2 or x.shape[1] < 3:
        raise ValueError(f'points (n, >= 3) expected, got {tuple(x.shape)}')
    if x.dtype != torch.float32:
        x = x.to(torch.float32)
    if x.shape[0] > 1 and (x.stride(1) != 1 or x.stride(0) < x.shape[1]):
        x = x.contiguous()
    return x


def _offsets(offsets, r, device):
    """-> (offsets (W + 1,) int64 on `device`, the same on the host as a numpy array), checked: 0 = o[0] < o[1] < ... < o[W] = R."""
    if offsets is None:
        host = np.array([0, r], dtype=np.int64)
    elif isinstance(offsets, torch.Tensor):
        host = offsets.detach().cpu().numpy().astype(np.int64).reshape(-1)
    else:
        host = np.asarray(offsets, dtype=np.int64).reshape(-1)
    if host.size < 2 or host[0] != 0 or host[-1] != r or (np.diff(host) < 1).any():
        raise ValueError('offsets (W + 1,) expected: 0 first, the number of rows last, at least one point per cloud')
    if isinstance(offsets, torch.Tensor) and offsets.device == device and offsets.dtype == torch.int64 and offsets.is_contiguous():
        return offsets.reshape(-1), host
    return torch.from_numpy(host).to(device), host


def _check_k(k):
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f'k in [1, {MAX_K}] expected, got {k}')
    return k


def _check_sizes(host, max_cloud_points):
    largest = int(np.diff(host).max())
    if largest > int(max_cloud_points):
        raise ValueError(f'a cloud of {largest} points exceeds max_cloud_points = {int(max_cloud_points)} (the search is exhaustive: '
                         f'{largest}^2 distances); raise the keyword if that is meant')


# ---------------------------------------------------------------------------------------------- the torch formulation (any device)
def _k_nearest_torch(rows, host, k):
    """The definition with tensor operations, one rounding each: d = ((dx dx) + (dy dy)) + (dz dz), a stable sort by d."""
    out = torch.full((rows.shape[0], k), -1, dtype=torch.int32, device=rows.device)
    for a, b in zip(host[:-1].tolist(), host[1:].tolist()):
        x = rows[a:b, :3]
        n, kk = b - a, min(k, b - a)
        step = max(1, _CHUNK // n)
        for q0 in range(0, n, step):
            q = x[q0:q0 + step]
            dx, dy, dz = (x[None, :, c] - q[:, None, c] for c in range(3))
            d = (dx * dx + dy * dy) + dz * dz
            out[a + q0:a + q0 + q.shape[0], :kk] = torch.sort(d, dim=1, stable=True).indices[:, :kk].to(torch.int32)
    return out


def _centroids_torch(rows, host):
    return torch.stack([rows[a:b, :3].to(torch.float64).sum(0) / float(b - a) for a, b in zip(host[:-1].tolist(), host[1:].tolist())]
                       ).to(torch.float32)


def _normals_torch(rows, host, knn, ref, mode):
    """fp64 covariance of the neighbours, torch.linalg.eigh, the unit vector rounded once, then the sign."""
    r, k = knn.shape
    normals = torch.zeros((r, 3), dtype=torch.float32, device=rows.device)
    curvature = torch.zeros((r,), dtype=torch.float32, device=rows.device)
    for w, (a, b) in enumerate(zip(host[:-1].tolist(), host[1:].tolist())):
        c = min(k, b - a)
        if c < 3:
            continue
        x = rows[a:b, :3].to(torch.float64)
        p = x[knn[a:b, :c].long()]                                   # (n, c, 3)
        q = p - p.sum(1, keepdim=True) / c
        cov = torch.einsum('nki,nkj->nij', q, q)
        tr = cov.diagonal(dim1=1, dim2=2).sum(1)
        ok = tr > 0
        lam, vec = torch.linalg.eigh(cov / torch.where(ok, tr, torch.ones_like(tr))[:, None, None])
        v = vec[:, :, 0]
        v = (v / v.norm(dim=1, keepdim=True)).to(torch.float32)
        if mode:
            dot = (v.to(torch.float64) * (x - ref[w].to(torch.float64))).sum(1)
            v = torch.where(((-dot if mode == 2 else dot) < 0)[:, None], -v, v)
        normals[a:b] = torch.where(ok[:, None], v, torch.zeros_like(v))
        curvature[a:b] = torch.where(ok, lam[:, 0].clamp(min=0), torch.zeros_like(tr)).to(torch.float32)
    return normals, curvature


# ------------------------------------------------------------------------------------------------------------ packed entry points
def _knn_packed(rows, offsets, host, k):
    if rows.is_cuda:
        return _seam._backend.k_nearest(rows, offsets, k)
    return _k_nearest_torch(rows, host, k)


def _normals_packed(rows, offsets, host, k, orient, viewpoint=None, want_curvature=False):
    """(normals (R, 3), curvature (R,) or None) of packed rows: one k_nearest launch and one shape_normals launch on the device (and the
    centroid launch of 'outward')."""
    if orient not in _MODES:
        raise ValueError("orient: 'outward', 'viewpoint' or None expected")
    mode, w = _MODES[orient], host.size - 1
    ref = None
    if mode == 2:
        if viewpoint is None:
            raise ValueError("orient='viewpoint' needs `viewpoint`: one point (3,), or one per cloud (W, 3)")
        v = viewpoint if isinstance(viewpoint, torch.Tensor) else torch.from_numpy(np.asarray(viewpoint, dtype=np.float32))
        v = v.to(device=rows.device, dtype=torch.float32)
        if v.numel() == 3:
            v = v.reshape(1, 3).expand(w, 3)
        if tuple(v.shape) != (w, 3):
            raise ValueError(f'viewpoint (3,) or ({w}, 3) expected, got {tuple(v.shape)}')
        ref = v.contiguous()
    elif viewpoint is not None:
        raise ValueError("`viewpoint` is only read with orient='viewpoint'")
    knn = _knn_packed(rows, offsets, host, k)
    if rows.is_cuda:
        if mode == 1:
            ref = _seam._backend.cloud_centroids(rows, offsets)
        return _seam._backend.shape_normals(rows, offsets, knn, ref, mode, want_curvature)
    if mode == 1:
        ref = _centroids_torch(rows, host)
    normals, curvature = _normals_torch(rows, host, knn, ref, mode)
    return normals, (curvature if want_curvature else None)


def k_nearest(points, k, offsets=None):
    """points (R, >= 3): xyz in the first three columns (a numpy array is uploaded once); offsets (W + 1,) or None (one cloud).
    -> (R, k) int32 on the points' device: for every point the min(k, n) points of its own cloud nearest to it -- itself included, at
    distance 0 --, ascending in (squared fp32 distance, position), as positions inside the cloud; -1 beyond a cloud of fewer than k."""
    k = _check_k(k)
    rows = _rows(points)
    offsets, host = _offsets(offsets, rows.shape[0], rows.device)
    return _knn_packed(rows, offsets, host, k)


def estimate_normals(points, k=16, offsets=None, orient='outward', viewpoint=None, return_curvature=False, *,
                     max_cloud_points=MAX_CLOUD_POINTS):
    """PCA normals of packed clouds -> (R, 3) fp32 [, curvature (R,) fp32 = smallest eigenvalue / trace].

    Per point: the covariance of its min(k, n) nearest points (itself included), the unit eigenvector of the smallest eigenvalue; a
    point with fewer than three neighbours or with coincident ones gets (0, 0, 0).  orient: 'outward' -- away from the cloud's
    centroid (the fp64 mean, rounded once); 'viewpoint' -- towards `viewpoint`, (3,) or one per cloud (W, 3); None -- the sign is
    left as the solver found it.  ValueError for k outside [1, 64] and for a cloud of more than max_cloud_points points."""
    k = _check_k(k)
    rows = _rows(points)
    offsets, host = _offsets(offsets, rows.shape[0], rows.device)
    _check_sizes(host, max_cloud_points)
    normals, curvature = _normals_packed(rows, offsets, host, k, orient, viewpoint, return_curvature)
    return (normals, curvature) if return_curvature else normals


# ------------------------------------------------------------------------------------------------------------------- one shape
def _coords(xyz, normalize):
    """(n, 3) fp32 coordinates on the device.  numpy: normalised on the host by the reference's own fp32 arithmetic
    (`DeviceShapeNet.normalize_point_cloud`), then uploaded; a tensor: normalised where it lives, in fp64, rounded once."""
    if isinstance(xyz, torch.Tensor):
        if xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.shape[0] < 1:
            raise ValueError(f'xyz (n, 3) with n >= 1 expected, got {tuple(xyz.shape)}')
        if not normalize:
            return xyz.to(torch.float32).contiguous()
        x = xyz.to(torch.float64)
        x = x - x.mean(dim=0)
        return (x / x.norm(dim=1).max()).to(torch.float32).contiguous()
    x = np.asarray(xyz)
    if x.ndim != 2 or x.shape[1] != 3 or x.shape[0] < 1:
        raise ValueError(f'xyz (n, 3) with n >= 1 expected, got {x.shape}')
    x = x.astype(np.float32)
    if normalize:
        x = DeviceShapeNet.normalize_point_cloud(x)
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(_default_device(None))


def prepare_shape(xyz, *, k=16, normalize=True, orient='outward', viewpoint=None):
    """xyz (n, 3) -> (n, 6) fp32 rows on the device: [coordinates (centred and scaled into the unit ball when `normalize`), normal].
    The normals are those of the NORMALISED coordinates (`estimate_normals`; a viewpoint is given in that frame)."""
    coords = _coords(xyz, normalize)
    return torch.cat([coords, estimate_normals(coords, k=k, orient=orient, viewpoint=viewpoint)], dim=1)


def shape_part_classes(shape_id, shape_name_to_part_classes=None):
    """(start_class, end_class) of shape `shape_id`: the shape_id-th entry of meters.MeterShapeNet's table."""
    table = _meters.default_shape_name_to_part_classes if shape_name_to_part_classes is None else shape_name_to_part_classes
    parts = list(table.values())[int(shape_id)]
    return int(parts[0]), int(parts[-1]) + 1


def segment_shape(model, xyz, shape_id, *, normals=None, num_points=2048, num_votes=1, with_one_hot_shape_id=True, num_shapes=16,
                  part_classes=None, rng=np.random, **prepare_options):
    """A raw shape -> per-point part labels: `prepare_shape` (skipped when `normals` (n, 3) are given; `normalize` still applies), the
    (C, n) point set of evaluate/shapenet/eval.py (coordinates, normals, one-hot shape id), a `ShapeVotes` over the shape's part
    classes -- `part_classes` = (start, end), default the shape_id-th range of meters.MeterShapeNet's table -- and
    `evaluate.shapenet_shape_votes`.  -> (predictions (n,) int64 on the device, the ShapeVotes).  rng: what the index shuffle draws from."""
    shape_id = int(shape_id)
    if not 0 <= shape_id < int(num_shapes):
        raise ValueError(f'shape_id in [0, {int(num_shapes)}) expected')
    if normals is None:
        rows = prepare_shape(xyz, **prepare_options)
    else:
        extra = set(prepare_options) - {'normalize'}
        if extra:
            raise TypeError(f'with `normals` given nothing is estimated: {sorted(extra)} have no meaning')
        coords = _coords(xyz, prepare_options.get('normalize', True))
        nrm = normals if isinstance(normals, torch.Tensor) else torch.from_numpy(np.asarray(normals, dtype=np.float32))
        nrm = nrm.to(device=coords.device, dtype=torch.float32)
        if tuple(nrm.shape) != tuple(coords.shape):
            raise ValueError(f'normals of shape {tuple(coords.shape)} expected, got {tuple(nrm.shape)}')
        rows = torch.cat([coords, nrm], dim=1)
    n, device = rows.shape[0], rows.device
    parts = [rows.t()]
    if with_one_hot_shape_id:
        hot = torch.zeros((int(num_shapes), n), dtype=torch.float32, device=device)
        hot[shape_id] = 1.0
        parts.append(hot)
    point_set = torch.cat(parts, dim=0).contiguous()
    start_class, end_class = part_classes if part_classes is not None else shape_part_classes(shape_id)
    votes = ShapeVotes(n, device, start_class, end_class)
    shapenet_shape_votes(model, point_set, votes, num_points=num_points, num_votes=num_votes, rng=rng)
    return votes.predictions(), votes
