"""The native seam: `_backend` with the reference's 12 entry points, served by libpvcnn_hip.so.

Reference: modules/functional/backend.py:6-25 JIT-builds a pybind module `_pvcnn_backend`
(src/bindings.cpp:10-37) with nvcc; every function rejects non-CUDA tensors (utils.hpp:7).
Here the same object shape is implemented over the C ABI in include/pvcnn_hip.h:

  * same names, argument order and return shapes / dtypes as the pybind functions;
  * same input contract: device tensor, contiguous, float32 / int32 -- violations raise
    RuntimeError like TORCH_CHECK does (plus shape checks the reference lacks);
  * outputs are allocated here with torch.empty (the library writes every element) on the
    inputs' device and work is enqueued on torch's current stream -- no host sync;
  * a failed launch raises (the reference prints and exit(-1)s, cuda_utils.cuh:28-37);
  * there is no CPU path: a CPU tensor or a missing library is an error, never a fallback.
"""
import ctypes
import os

import torch

from ... import _lib
from . import _cache
from ._align import aligned as _aligned
from ._product import CONV, PW

__all__ = ['_backend']


def _dev(t, name):
    if not t.is_cuda:
        raise RuntimeError(f'{name} must be a CUDA (HIP) tensor -- the PVConv hot path has no CPU implementation')


def _f32(t, name):
    _dev(t, name)
    if not t.is_contiguous():
        raise RuntimeError(f'{name} must be a contiguous tensor')
    if t.dtype != torch.float32:
        raise RuntimeError(f'{name} must be a float tensor')


def _f32_rows(t, name):
    """float32 (B, C, S) tensor whose C*S rows of a sample are contiguous; samples may be further apart (a channel
    slice of a wider tensor, e.g. a gradient coming out of torch.cat's backward).  -> batch stride in elements."""
    _dev(t, name)
    if t.dtype != torch.float32:
        raise RuntimeError(f'{name} must be a float tensor')
    b, c, n = t.shape
    ok = (n == 1 or t.stride(2) == 1) and (c == 1 or t.stride(1) == n) and (b == 1 or t.stride(0) >= c * n)
    if not ok:
        raise RuntimeError(f'{name} must be contiguous within each sample')
    return t.stride(0) if b > 1 else c * n


def batch_strided_ok(t):
    """True when _f32_rows would accept t (callers use it to skip a .contiguous() copy)."""
    if t.dim() != 3 or t.dtype != torch.float32:
        return False
    b, c, n = t.shape
    return (n == 1 or t.stride(2) == 1) and (c == 1 or t.stride(1) == n) and (b == 1 or t.stride(0) >= c * n)


def _i32(t, name):
    _dev(t, name)
    if not t.is_contiguous():
        raise RuntimeError(f'{name} must be a contiguous tensor')
    if t.dtype != torch.int32:
        raise RuntimeError(f'{name} must be an int tensor')


def _shape(cond, msg):
    if not cond:
        raise RuntimeError(msg)


def _arg(cond, msg):
    """_shape for the entry points whose messages their own tests trip (tests/test_gpu_shapes.py), not the recorded call logs."""
    if not cond:
        raise RuntimeError(msg)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else ctypes.c_void_p(None)


_DUMMIES = {}


def _dummies(dev):
    """The 1-element (inds, wgts) the devoxelize forward returns when it does not emit them (trilinear_devox.cpp:45-53): one zeroed
    pair per device, made once -- a training step asks for them once per PVConv layer behind the first of a resolution (two fill
    launches each)."""
    key = (dev.type, dev.index)
    if key not in _DUMMIES:
        _DUMMIES[key] = (torch.zeros((1,), dtype=torch.int32, device=dev), torch.zeros((1,), dtype=torch.float32, device=dev))
    return _DUMMIES[key]


class _Launch:
    """Device guard + current stream of the tensor's device for one native call."""

    def __init__(self, ref):
        self.device = ref.device
        self.guard = torch.cuda.device(self.device)

    def __enter__(self):
        self.guard.__enter__()
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def __exit__(self, *exc):
        return self.guard.__exit__(*exc)


def _run(fn, label, ref, *args):
    """One native call on `ref`'s device and torch's current stream: a tensor among `args` goes as its device pointer (_p: an empty
    one as NULL), None as NULL, everything else as it is; the stream goes last; a non-zero return code raises, naming `label`."""
    conv = [_p(a) if a is None or isinstance(a, torch.Tensor) else a for a in args]
    with _Launch(ref) as s:
        _lib.check(fn(*conv, s), label)


def _device_call(name, ref, *args, lib=None, error=ValueError):
    """One pvcnn_<name> call (of `lib`, default the loaded library) on `ref`'s device and torch's current stream (`_run`): tensors
    (contiguous, on that device, else `error`) as device pointers, None as NULL, floats as doubles, everything else as an int."""
    for a in args:
        if isinstance(a, torch.Tensor) and (a.device != ref.device or not a.is_contiguous()):
            raise error(f'{name}: contiguous tensors on one device expected')
    _run(getattr(lib or _lib.load(), 'pvcnn_' + name), name, ref, *(a if a is None or isinstance(a, (torch.Tensor, float)) else int(a) for a in args))


def fresh_seed(device, generator=None, out=None):
    """The two int64 words that key a device draw stream (include/pvcnn_hip.h, "Device draws"), from torch's generator of `device`
    (or from `generator`, on its own device): no host synchronisation, `torch.manual_seed` governs them.  `out`: two device words
    redrawn in place -- inside a captured step, fresh words on every replay."""
    if out is not None:
        return out.random_(0, 2 ** 62)
    gdev = generator.device if generator is not None else device
    return torch.randint(0, 2 ** 62, (2,), dtype=torch.int64, device=gdev, generator=generator).to(device)


def check_seed(seed, device=None):
    """-> seed, or ValueError unless it is two (or more) contiguous int64 words on `device` (default: on any GPU)."""
    if not isinstance(seed, torch.Tensor) or seed.dtype != torch.int64 or seed.numel() < 2 or not seed.is_contiguous() \
            or (seed.device != device if device is not None else not seed.is_cuda):
        raise ValueError('seed = two int64 words on the device')
    return seed


def _mean_rstd(c, device):
    """The uninitialised (mean, rstd) pair of a BatchNorm over c channels."""
    return torch.empty((c,), dtype=torch.float32, device=device), torch.empty((c,), dtype=torch.float32, device=device)


class HipBackend:
    name = 'hip-gfx950'

    def __init__(self):
        self._lib = None

    @property
    def lib(self):
        if self._lib is None:
            self._lib = _lib.load()
        return self._lib

    @staticmethod
    def _scratch(nbytes, device):
        """Caller-owned scratch for the deterministic scatters (torch's caching allocator makes this cheap)."""
        return torch.empty((max(int(nbytes), 16),), dtype=torch.uint8, device=device)

    # ---- "last workgroup done" tickets (include/pvcnn_hip.h, ABI v11): zeroed words a reduction's launch leaves zeroed, so that its
    # finalize step is the tail of the launch instead of a ~5 us launch of its own.  MEASURED AND NOT THE DEFAULT (round 5,
    # profiles/ab/r05d_fold_without_fences.md): the published atomics + tickets of ~100 k workgroups per step cost what the 26 launches
    # cost (PVCNN 6.636 vs 6.605 ms, Frustum-PVCNN 6.19 vs 6.07 ms); with fences, twice the step.  PVCNN_FOLD_FINALIZE=1 (read once per
    # process) switches it on; the tests pin both paths against each other.  One persistent pool per device (a captured graph keeps the
    # addresses); slices are handed out round robin PER (device, stream) -- launches on one stream never overlap, launches on two
    # streams (a side stream, a parallel branch of a captured step) draw from pools of their own (a word shared by two
    # concurrent launches would fool the "last workgroup" decision)
    fold_finalize = os.environ.get('PVCNN_FOLD_FINALIZE', '0') == '1'
    _TICKET_POOL = 1 << 16

    def _tickets(self, n, device):
        """-> a zeroed int32 view of n words (every kernel that takes tickets leaves them zeroed), or None when folding is off."""
        if not self.fold_finalize or n > self._TICKET_POOL:
            return None
        pools = self.__dict__.setdefault('_ticket_pools', {})
        key = (device.type, device.index, int(torch.cuda.current_stream(device).cuda_stream) if device.type == 'cuda' else 0)
        ent = pools.get(key)
        if ent is None:
            ent = pools[key] = [torch.zeros((self._TICKET_POOL,), dtype=torch.int32, device=device), 0]
        if ent[1] + n > self._TICKET_POOL:
            ent[1] = 0
        view = ent[0][ent[1]:ent[1] + n]
        ent[1] += (int(n) + 15) & ~15
        return view

    # ---- sampling.cpp:6-41 ------------------------------------------------------------------
    def gather_features_forward(self, features, indices):
        _f32(features, 'features'); _i32(indices, 'indices')
        _shape(features.dim() == 3 and indices.dim() == 2 and indices.shape[0] == features.shape[0],
               'gather: features (B,C,N), indices (B,M) expected')
        b, c, n = features.shape
        m = indices.shape[1]
        out = torch.empty((b, c, m), dtype=torch.float32, device=features.device)
        _run(self.lib.pvcnn_gather_fwd, 'gather_features_forward', features, features, indices, b, c, n, m, out)
        return out

    def gather_features_backward(self, grad_y, indices, n):
        _f32(grad_y, 'grad_y'); _i32(indices, 'indices')
        _shape(grad_y.dim() == 3 and indices.dim() == 2 and indices.shape == (grad_y.shape[0], grad_y.shape[2]),
               'gather backward: grad_y (B,C,M), indices (B,M) expected')
        b, c, m = grad_y.shape
        grad_x = torch.empty((b, c, int(n)), dtype=torch.float32, device=grad_y.device)
        ws = self._scratch(self.lib.pvcnn_gather_bwd_workspace_bytes(b, c, int(n), m), grad_y.device)
        _run(self.lib.pvcnn_gather_bwd, 'gather_features_backward', grad_y, grad_y, indices, b, c, int(n), m, grad_x, ws, ws.numel())
        return grad_x

    # ---- sampling.cpp:43-58 -----------------------------------------------------------------
    def furthest_point_sampling(self, coords, num_samples):
        _f32(coords, 'coords')
        _shape(coords.dim() == 3 and coords.shape[1] == 3, 'furthest_point_sampling: coords (B,3,N) expected')
        b, _, n = coords.shape
        m = int(num_samples)
        indices = torch.empty((b, m), dtype=torch.int32, device=coords.device)
        distances = None
        if n > 16384:   # PVCNN_FPS_MAX_RESIDENT_POINTS: larger clouds need the global scratch
            distances = torch.empty((b, n), dtype=torch.float32, device=coords.device)
        _run(self.lib.pvcnn_fps, 'furthest_point_sampling', coords, coords, b, n, m, distances, indices)
        return indices

    # ---- the index selection of logits_mask (modules/functional/sampling.py:69-82) on the device ----------------
    has_mask_select = True

    def mask_select(self, mask, num_samples, choices=None, seed=None):
        """mask (B,N) bool -> selected (B,M) int32 foreground point ids (see include/pvcnn_hip.h).  choices (B,M) int32:
        parity mode (the caller's draws); else seed: int64 device tensor (key, stream id) for the Philox stream."""
        _dev(mask, 'mask')
        _shape(mask.dim() == 2 and mask.dtype in (torch.bool, torch.uint8) and mask.is_contiguous(), 'mask_select: mask (B,N) bool expected')
        b, n = mask.shape
        m = int(num_samples)
        if choices is not None:
            _i32(choices, 'choices')
            _shape(tuple(choices.shape) == (b, m), 'mask_select: choices (B,M) expected')
        else:
            _dev(seed, 'seed')
            _shape(seed.dtype == torch.int64 and seed.numel() >= 2 and seed.is_contiguous(), 'mask_select: seed = 2 x int64 on the device')
        selected = torch.empty((b, m), dtype=torch.int32, device=mask.device)
        _run(self.lib.pvcnn_mask_select, 'mask_select', mask, mask.view(torch.uint8), b, n, m, choices, seed if choices is None else None,
             selected, None)
        return selected

    # ---- batches assembled on the device (csrc/batch.hip; pvcnn_amd/data.py checks shapes and owns the tensors) ----------------
    has_batch_assembly = True

    def batch_launch(self, entry, ref, *args):
        """One pvcnn_batch_* launch on `ref`'s device and torch's current stream (`_device_call`); a tensor off the GPU is refused."""
        for a in (*args, ref):
            if isinstance(a, torch.Tensor):
                _dev(a, entry)
        _device_call(entry, ref, *args, lib=self.lib, error=RuntimeError)

    # ---- augmentation of an assembled batch (csrc/augment.hip; pvcnn_amd/augment.py checks shapes and owns the tensors) ----------
    has_augment = True

    def augment_draw(self, params, seed, axis, scalars):
        """params (B, 24) fp64 <- the per-cloud draws; `scalars`: the ten ranges of pvcnn_augment_draw in the header's order."""
        _run(self.lib.pvcnn_augment_draw, 'augment_draw', params, params.shape[0], int(axis), *(float(v) for v in scalars), seed, params)

    def augment_apply(self, src, targets_src, layout, params, jitter_sigma, jitter_clip, jitter_on, drop_on, jitter, keep, seed, dst,
                      targets_dst, jitter_out, keep_out):
        """One pvcnn_augment_apply launch.  src / dst (B, C, N) fp32 may be batch-strided views, and so may the targets (B, N) int64,
        whose rows the caller has checked to be contiguous; `layout`: [(role, first plane), ...] with the header's role numbers (it
        goes as a small host array)."""
        b, c, n = src.shape
        stride_x = _f32_rows(src, 'src'), _f32_rows(dst, 'dst')
        stride_t = (n, n)
        if targets_src is not None:
            _dev(targets_src, 'targets'); _dev(targets_dst, 'out_targets')
            stride_t = tuple(t.stride(0) if b > 1 else n for t in (targets_src, targets_dst))
        flat = (ctypes.c_int32 * max(2 * len(layout), 1))(*[v for pair in layout for v in pair])
        _run(self.lib.pvcnn_augment_apply, 'augment_apply', src, src, stride_x[0], targets_src, stride_t[0], b, c, n, flat, len(layout),
             params, float(jitter_sigma), float(jitter_clip), int(jitter_on), int(drop_on), jitter, keep, seed, dst, stride_x[1],
             targets_dst, stride_t[1], jitter_out, keep_out)

    # ---- ball_query.cpp:6-30 ----------------------------------------------------------------
    def ball_query(self, centers_coords, points_coords, radius, num_neighbors):
        _f32(centers_coords, 'centers_coords'); _f32(points_coords, 'points_coords')
        _shape(centers_coords.dim() == 3 and points_coords.dim() == 3 and centers_coords.shape[1] == 3
               and points_coords.shape[1] == 3 and centers_coords.shape[0] == points_coords.shape[0],
               'ball_query: centers (B,3,M), points (B,3,N) expected')
        b, _, m = centers_coords.shape
        n = points_coords.shape[2]
        u = int(num_neighbors)
        out = torch.empty((b, m, u), dtype=torch.int32, device=centers_coords.device)
        _run(self.lib.pvcnn_ball_query, 'ball_query', centers_coords, centers_coords, points_coords, b, n, m, float(radius), u, out)
        return out

    # ---- grouping.cpp:6-44 ------------------------------------------------------------------
    def grouping_forward(self, features, indices):
        _f32(features, 'features'); _i32(indices, 'indices')
        _shape(features.dim() == 3 and indices.dim() == 3 and indices.shape[0] == features.shape[0],
               'grouping: features (B,C,N), indices (B,M,U) expected')
        b, c, n = features.shape
        _, m, u = indices.shape
        out = torch.empty((b, c, m, u), dtype=torch.float32, device=features.device)
        _run(self.lib.pvcnn_grouping_fwd, 'grouping_forward', features, features, indices, b, c, n, m, u, out)
        return out

    def grouping_backward(self, grad_y, indices, n):
        _f32(grad_y, 'grad_y'); _i32(indices, 'indices')
        _shape(grad_y.dim() == 4 and indices.dim() == 3 and tuple(indices.shape) == (grad_y.shape[0], grad_y.shape[2], grad_y.shape[3]),
               'grouping backward: grad_y (B,C,M,U), indices (B,M,U) expected')
        b, c, m, u = grad_y.shape
        grad_x = torch.empty((b, c, int(n)), dtype=torch.float32, device=grad_y.device)
        ws = self._scratch(self.lib.pvcnn_grouping_bwd_workspace_bytes(b, c, int(n), m, u), grad_y.device)
        _run(self.lib.pvcnn_grouping_bwd, 'grouping_backward', grad_y, grad_y, indices, b, c, int(n), m, u, grad_x, ws, ws.numel())
        return grad_x

    # ---- neighbor_interpolate.cpp:6-65 ------------------------------------------------------
    def three_nearest_neighbors_interpolate_forward(self, points_coords, centers_coords, centers_features):
        _f32(points_coords, 'points_coords'); _f32(centers_coords, 'centers_coords'); _f32(centers_features, 'centers_features')
        _shape(points_coords.dim() == 3 and centers_coords.dim() == 3 and centers_features.dim() == 3
               and points_coords.shape[1] == 3 and centers_coords.shape[1] == 3
               and centers_coords.shape[2] == centers_features.shape[2]
               and points_coords.shape[0] == centers_coords.shape[0] == centers_features.shape[0],
               '3-NN interpolate: points (B,3,N), centers (B,3,M), features (B,C,M) expected')
        b, c, m = centers_features.shape
        n = points_coords.shape[2]
        dev = points_coords.device
        indices = torch.empty((b, 3, n), dtype=torch.int32, device=dev)
        weights = torch.empty((b, 3, n), dtype=torch.float32, device=dev)
        out = torch.empty((b, c, n), dtype=torch.float32, device=dev)
        _run(self.lib.pvcnn_three_nn_interp_fwd, 'three_nearest_neighbors_interpolate_forward', points_coords,
             points_coords, centers_coords, centers_features, b, c, m, n, indices, weights, out)
        return [out, indices, weights]

    def three_nearest_neighbors_interpolate_backward(self, grad_y, indices, weights, m):
        _f32(grad_y, 'grad_y'); _i32(indices, 'indices'); _f32(weights, 'weights')
        _shape(grad_y.dim() == 3 and tuple(indices.shape) == (grad_y.shape[0], 3, grad_y.shape[2])
               and indices.shape == weights.shape,
               '3-NN interpolate backward: grad_y (B,C,N), indices/weights (B,3,N) expected')
        b, c, n = grad_y.shape
        grad_x = torch.empty((b, c, int(m)), dtype=torch.float32, device=grad_y.device)
        ws = self._scratch(self.lib.pvcnn_three_nn_interp_bwd_workspace_bytes(b, c, n, int(m)), grad_y.device)
        _run(self.lib.pvcnn_three_nn_interp_bwd, 'three_nearest_neighbors_interpolate_backward', grad_y,
             grad_y, indices, weights, b, c, n, int(m), grad_x, ws, ws.numel())
        return grad_x

    # the two scatter entries of the 12-callable seam keep their plan on the tensor they were called with (False: the one-shot C entries,
    # which rebuild the counting sort per call -- kept reachable for the tests that pin them)
    seam_plan_memo = True

    # ---- trilinear_devox.cpp:18-91 (argument order: r, is_training, coords, features) ----------
    def trilinear_devoxelize_forward(self, r, is_training, coords, features):
        _f32(features, 'features'); _f32(coords, 'coords')
        r = int(r)
        _shape(features.dim() == 3 and coords.dim() == 3 and coords.shape[1] == 3
               and coords.shape[0] == features.shape[0] and features.shape[2] == r * r * r,
               'trilinear_devoxelize: coords (B,3,N), features (B,C,R^3) expected')
        b, c = features.shape[:2]
        n = coords.shape[2]
        dev = features.device
        outs = torch.empty((b, c, n), dtype=torch.float32, device=dev)
        if is_training:
            inds = torch.empty((b, 8, n), dtype=torch.int32, device=dev)
            wgts = torch.empty((b, 8, n), dtype=torch.float32, device=dev)
        else:   # 1-element dummies, like trilinear_devox.cpp:45-53
            inds, wgts = _dummies(dev)
        _run(self.lib.pvcnn_trilinear_devox_fwd, 'trilinear_devoxelize_forward', features, coords, features, b, c, n, r,
             int(bool(is_training)), inds if is_training else None, wgts if is_training else None, outs)
        return [outs, inds, wgts]

    def trilinear_devoxelize_backward(self, grad_y, indices, weights, r):
        gy_bstride = _f32_rows(grad_y, 'grad_y'); _f32(weights, 'weights'); _i32(indices, 'indices')
        _shape(grad_y.dim() == 3 and tuple(indices.shape) == (grad_y.shape[0], 8, grad_y.shape[2])
               and indices.shape == weights.shape,
               'trilinear_devoxelize backward: grad_y (B,C,N), indices/weights (B,8,N) expected')
        b, c, n = grad_y.shape
        r = int(r)
        # PLAN REUSE BEHIND THE REFERENCE'S OWN CALL (functional/devoxelization.py:30-39 passes the saved (inds, wgts) here on every
        # backward): the counting sort depends on (inds, wgts, R) only, so it is memoised on the `indices` tensor OBJECT (identity +
        # in-place version + storage view: _cache.memo; dies with the tensor) together with the identity / version of `weights` -- a
        # second call with the same saved tensors runs the apply alone.  No new API: section B users of INTEGRATION.md get it as is.
        if self.seam_plan_memo and self.lib.pvcnn_trilinear_devox_bwd_plan_bytes(b, n, r):
            key = ('seam devox bwd plan', r, id(weights), weights._version, weights.data_ptr())
            plan = _cache.memo(indices, key, lambda: self.trilinear_devoxelize_backward_plan(indices, weights, r))
            if plan is not None:
                return self.trilinear_devoxelize_backward_apply(grad_y, plan, r)
        grad_x = torch.empty((b, c, r * r * r), dtype=torch.float32, device=grad_y.device)
        ws = self._scratch(self.lib.pvcnn_trilinear_devox_bwd_workspace_bytes(b, c, n, r), grad_y.device)
        _run(self.lib.pvcnn_trilinear_devox_bwd_strided, 'trilinear_devoxelize_backward', grad_y,
             grad_y, gy_bstride, indices, weights, b, c, n, r, grad_x, ws, ws.numel())
        return grad_x

    # ---- modules/voxelization.py:16-25 ---------------------------------------------------------
    has_voxel_coords = True

    def voxel_coords(self, coords, resolution, normalize, eps):
        """coords (B,3,N) -> (norm_coords float (B,3,N) in [0,R-1], vox_coords int32 (B,3,N)) in one launch."""
        _f32(coords, 'coords')
        _shape(coords.dim() == 3 and coords.shape[1] == 3, 'voxel_coords: coords (B,3,N) expected')
        b, _, n = coords.shape
        norm = torch.empty_like(coords)
        vox = torch.empty((b, 3, n), dtype=torch.int32, device=coords.device)
        _run(self.lib.pvcnn_voxel_coords, 'voxel_coords', coords, coords, b, n, int(resolution), int(bool(normalize)), float(eps), norm, vox)
        return norm, vox

    def voxel_coords_tail(self, coords, mean, radius, resolution, eps):
        """The fused elementwise tail of Voxelization.forward: coords (B,3,N) (rows contiguous within a cloud; may be a
        channel slice of a wider tensor), mean (B,3,1) and radius (B,1,1) | None from the reference's own torch
        reductions -> (norm_coords, vox_coords), bit-identical to modules/voxelization.py:16-25 on this device."""
        cstride = _f32_rows(coords, 'coords')
        _shape(coords.dim() == 3 and coords.shape[1] == 3, 'voxel_coords: coords (B,3,N) expected')
        b, _, n = coords.shape
        _f32(mean, 'mean')
        _shape(mean.numel() == b * 3, 'voxel_coords: mean (B,3) expected')
        if radius is not None:
            _f32(radius, 'radius')
            _shape(radius.numel() == b, 'voxel_coords: radius (B) expected')
        norm = torch.empty((b, 3, n), dtype=torch.float32, device=coords.device)
        vox = torch.empty((b, 3, n), dtype=torch.int32, device=coords.device)
        _run(self.lib.pvcnn_voxel_coords_tail, 'voxel_coords_tail', coords, coords, cstride, mean, radius, b, n, int(resolution), float(eps),
             norm, vox)
        return norm, vox

    # ---- vox.cpp:17-76 ----------------------------------------------------------------------
    def avg_voxelize_forward(self, features, coords, resolution):
        _f32(features, 'features'); _i32(coords, 'coords')
        _shape(features.dim() == 3 and coords.dim() == 3 and coords.shape[1] == 3
               and coords.shape[0] == features.shape[0] and coords.shape[2] == features.shape[2],
               'avg_voxelize: features (B,C,N), coords (B,3,N) expected')
        b, c, n = features.shape
        r = int(resolution)
        s3 = r * r * r
        dev = features.device
        # plan reuse behind the reference's own call (functional/voxelization.py:10-24): memoised on the int32 `coords` tensor object
        # (identity + in-place version: a coords tensor written in place misses); the plan's ind / cnt are handed out as they are
        # (read-only by the reference's convention: saved for backward) and re-checked by their own version counters on every hit
        if self.seam_plan_memo and self.lib.pvcnn_avg_voxelize_plan_bytes(b, n, r):
            key = ('seam voxelize plan', r)
            hit = _cache.memo(coords, key, lambda: self._stamped_voxel_plan(coords, r))
            if hit is not None and (hit[0].ind._version, hit[0].cnt._version) != hit[1]:     # a caller wrote into ind / cnt: rebuild
                _cache.forget(coords, key)
                hit = _cache.memo(coords, key, lambda: self._stamped_voxel_plan(coords, r))
            if hit is not None:
                return [self.avg_voxelize_apply(features, hit[0]), hit[0].ind, hit[0].cnt]
        out = torch.empty((b, c, s3), dtype=torch.float32, device=dev)
        ind = torch.empty((b, n), dtype=torch.int32, device=dev)
        cnt = torch.empty((b, s3), dtype=torch.int32, device=dev)
        ws = self._scratch(self.lib.pvcnn_avg_voxelize_fwd_workspace_bytes(b, c, n, r), dev)
        _run(self.lib.pvcnn_avg_voxelize_fwd, 'avg_voxelize_forward', features, features, coords, b, c, n, r, out, ind, cnt, ws, ws.numel())
        return [out, ind, cnt]

    def _stamped_voxel_plan(self, coords, r):
        vp = self.avg_voxelize_plan(coords, r)
        return None if vp is None else (vp, (vp.ind._version, vp.cnt._version))

    def avg_voxelize_backward(self, grad_y, indices, cnt):
        _f32(grad_y, 'grad_y'); _i32(indices, 'indices'); _i32(cnt, 'cnt')
        _shape(grad_y.dim() == 3 and indices.dim() == 2 and tuple(cnt.shape) == (grad_y.shape[0], grad_y.shape[2])
               and indices.shape[0] == grad_y.shape[0],
               'avg_voxelize backward: grad_y (B,C,S), indices (B,N), cnt (B,S) expected')
        b, c, s3 = grad_y.shape
        n = indices.shape[1]
        grad_x = torch.empty((b, c, n), dtype=torch.float32, device=grad_y.device)
        _run(self.lib.pvcnn_avg_voxelize_bwd, 'avg_voxelize_backward', grad_y, grad_y, indices, cnt, b, c, n, s3, grad_x)
        return grad_x

    # ---- scatter plans (include/pvcnn_hip.h "scatter plans"): one counting sort per (coords, R), applied by every layer ----
    has_scatter_plans = True

    class VoxelPlan:
        """avg_voxelize's plan for one (voxel coordinates, R): ind (B,N), cnt (B,R^3) and the opaque sort plan."""
        __slots__ = ('ind', 'cnt', 'plan', 'r', 'n', 'b')

    def _voxel_plan(self, b, n, r, nbytes, dev):
        """An empty VoxelPlan for (B, N, R) whose opaque plan takes nbytes."""
        vp = self.VoxelPlan()
        vp.r, vp.n, vp.b = r, n, b
        vp.ind = torch.empty((b, n), dtype=torch.int32, device=dev)
        vp.cnt = torch.empty((b, r * r * r), dtype=torch.int32, device=dev)
        vp.plan = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        return vp

    def avg_voxelize_plan(self, coords, resolution):
        """coords (B,3,N) int32 -> VoxelPlan, or None when the grid is too large for a plan (one-shot path then)."""
        _i32(coords, 'coords')
        _shape(coords.dim() == 3 and coords.shape[1] == 3, 'avg_voxelize: coords (B,3,N) expected')
        b, _, n = coords.shape
        r = int(resolution)
        nbytes = self.lib.pvcnn_avg_voxelize_plan_bytes(b, n, r)
        if nbytes == 0:
            return None
        vp = self._voxel_plan(b, n, r, nbytes, coords.device)
        scratch = self._scratch(self.lib.pvcnn_avg_voxelize_plan_scratch_bytes(b, n, r), coords.device)
        _run(self.lib.pvcnn_avg_voxelize_plan, 'avg_voxelize_plan', coords, coords, b, n, r, vp.ind, vp.cnt, vp.plan, vp.plan.numel(),
             scratch, scratch.numel())
        return vp

    # ---- the z rows of a grid that hold a point: what avg_voxelize's backward reads of the grid's gradient (include/pvcnn_hip.h,
    # NEEDED ROWS); conv3d_igemm_split(..., rows=) leaves out the output tiles without such a row ----
    has_conv_bwd_rows = True

    def voxel_need_rows(self, cnt, resolution):
        """cnt (B, R^3) int32, a VoxelPlan's counts -> int32 (B * R * R,): 1 where the z row (b, x, y) holds a point, else 0."""
        _i32(cnt, 'cnt')
        r = int(resolution)
        if not (cnt.dim() == 2 and cnt.shape[1] == r * r * r and cnt.is_contiguous()):
            raise ValueError('voxel_need_rows: cnt (B,R^3), contiguous, expected')
        rows = torch.empty((cnt.shape[0] * r * r,), dtype=torch.int32, device=cnt.device)
        _run(self.lib.pvcnn_voxel_need_rows, 'voxel_need_rows', cnt, cnt, cnt.shape[0], r, rows)
        return rows

    # PVCNN_PAIR_PLANS=0 (read once per process): the two plans of a PVConv geometry from their own chains (A/B; the pair is the default)
    has_pvconv_plans = os.environ.get('PVCNN_PAIR_PLANS', '1') != '0'

    def pvconv_plans(self, vox_coords, norm_coords, resolution):
        """(vox_coords int32 (B,3,N), norm_coords float (B,3,N), R) -> (VoxelPlan, devoxelize-backward plan tensor): what
        avg_voxelize_plan(vox_coords, R) and trilinear_devoxelize_backward_plan(inds, wgts, R) of the taps at norm_coords build, from ONE
        chain of three launches (csrc/csr.h: launch_csr_prep_pair).  None when the grid is too large for a plan."""
        _i32(vox_coords, 'vox_coords'); _f32(norm_coords, 'norm_coords')
        _shape(vox_coords.dim() == 3 and vox_coords.shape[1] == 3 and tuple(norm_coords.shape) == tuple(vox_coords.shape),
               'pvconv_plans: vox_coords / norm_coords (B,3,N) expected')
        b, _, n = vox_coords.shape
        r = int(resolution)
        vbytes, dbytes = self.lib.pvcnn_avg_voxelize_plan_bytes(b, n, r), self.lib.pvcnn_trilinear_devox_bwd_plan_bytes(b, n, r)
        if vbytes == 0 or dbytes == 0 or n == 0:
            return None
        dev = vox_coords.device
        vp = self._voxel_plan(b, n, r, vbytes, dev)
        dplan = torch.empty((dbytes,), dtype=torch.uint8, device=dev)
        scratch = self._scratch(self.lib.pvcnn_pvconv_plans_scratch_bytes(b, n, r), dev)
        _run(self.lib.pvcnn_pvconv_plans, 'pvconv_plans', vox_coords, vox_coords, norm_coords, b, n, r, vp.ind, vp.cnt, vp.plan, vp.plan.numel(),
             dplan, dplan.numel(), scratch, scratch.numel())
        return vp, dplan

    def avg_voxelize_apply(self, features, vp):
        """features (B,C,N) -> out (B,C,R^3) with the plan of avg_voxelize_plan (same B, N, R)."""
        _f32(features, 'features')
        _shape(features.dim() == 3 and features.shape[0] == vp.b and features.shape[2] == vp.n, 'avg_voxelize: features do not match the plan')
        b, c, n = features.shape
        out = torch.empty((b, c, vp.r ** 3), dtype=torch.float32, device=features.device)
        _run(self.lib.pvcnn_avg_voxelize_apply, 'avg_voxelize_apply', features, features, vp.plan, vp.plan.numel(), b, c, n, vp.r, out)
        return out

    def trilinear_devoxelize_backward_plan(self, indices, weights, r):
        """(inds, wgts) (B,8,N) -> opaque plan tensor of the backward scatter, or None when R is too large for one."""
        _i32(indices, 'indices'); _f32(weights, 'weights')
        _shape(indices.dim() == 3 and indices.shape[1] == 8 and indices.shape == weights.shape, 'inds / wgts (B,8,N) expected')
        b, _, n = indices.shape
        r = int(r)
        nbytes = self.lib.pvcnn_trilinear_devox_bwd_plan_bytes(b, n, r)
        if nbytes == 0:
            return None
        plan = torch.empty((nbytes,), dtype=torch.uint8, device=indices.device)
        scratch = self._scratch(self.lib.pvcnn_trilinear_devox_bwd_plan_scratch_bytes(b, n, r), indices.device)
        _run(self.lib.pvcnn_trilinear_devox_bwd_plan, 'trilinear_devoxelize_backward_plan', indices, indices, weights, b, n, r,
             plan, plan.numel(), scratch, scratch.numel())
        return plan

    def trilinear_devoxelize_backward_apply(self, grad_y, plan, r):
        gy_bstride = _f32_rows(grad_y, 'grad_y')
        b, c, n = grad_y.shape
        r = int(r)
        grad_x = torch.empty((b, c, r * r * r), dtype=torch.float32, device=grad_y.device)
        _run(self.lib.pvcnn_trilinear_devox_bwd_apply, 'trilinear_devoxelize_backward_apply', grad_y, grad_y, gy_bstride, plan, plan.numel(),
             b, c, n, r, grad_x)
        return grad_x

    # ---- voxel_layers Conv3d (k=3, stride 1, pad 1): modules/pvconv.py:20-27 (cuDNN in the reference) ----
    has_conv3d = True

    def _conv_wt(self, weight, for_bwd_data):
        co, ci = weight.shape[0], weight.shape[1]
        wt = torch.empty((ci * 27 * co,), dtype=torch.float32, device=weight.device)
        _run(self.lib.pvcnn_conv3d_weight_transform, 'conv3d_weight_transform', weight, weight, co, ci, int(for_bwd_data), wt)
        return wt

    def conv3d_forward(self, x, weight, bias, want_stats=False):
        _f32(x, 'x'); _f32(weight, 'weight')
        _shape(x.dim() == 5 and weight.dim() == 5 and tuple(weight.shape[2:]) == (3, 3, 3) and weight.shape[1] == x.shape[1]
               and x.shape[2] == x.shape[3] == x.shape[4], 'conv3d: x (B,Ci,R,R,R), weight (Co,Ci,3,3,3) expected')
        if bias is not None:
            _f32(bias, 'bias')
        b, ci, r = x.shape[0], x.shape[1], x.shape[2]
        co = weight.shape[0]
        wt = self._conv_wt(weight, False)
        y = torch.empty((b, co, r, r, r), dtype=torch.float32, device=x.device)
        if want_stats:   # per-workgroup (sum, sum of squares) partials for the BatchNorm that follows
            part = torch.empty((co, self.lib.pvcnn_conv3d_fwd_stats_parts(b, co, r), 2), dtype=torch.float32, device=x.device)
            _run(self.lib.pvcnn_conv3d_fwd_stats, 'conv3d_forward', x, x, wt, bias, b, ci, co, r, y, part)
            return y, part
        _run(self.lib.pvcnn_conv3d_fwd, 'conv3d_forward', x, x, wt, bias, b, ci, co, r, y)
        return y

    def conv3d_backward_data(self, grad_y, weight):
        _f32(grad_y, 'grad_y'); _f32(weight, 'weight')
        b, co, r = grad_y.shape[0], grad_y.shape[1], grad_y.shape[2]
        ci = weight.shape[1]
        wt = self._conv_wt(weight, True)
        gx = torch.empty((b, ci, r, r, r), dtype=torch.float32, device=grad_y.device)
        # a convolution with Ci and Co exchanged on the flipped weights
        _run(self.lib.pvcnn_conv3d_fwd, 'conv3d_backward_data', grad_y, grad_y, wt, None, b, co, ci, r, gx)
        return gx

    # the backward-weight / BatchNorm-backward entries take `out_w` / `out_b`: where to write the two parameter gradients (contiguous
    # fp32 tensors of the right shape, e.g. the parameter's slot in a flat gradient bucket: functional/_gradslots.py) instead of fresh ones
    has_grad_out = True

    @staticmethod
    def _grad_out(dst, shape, device):
        if dst is None:
            return torch.empty(shape, dtype=torch.float32, device=device)
        _shape(tuple(dst.shape) == tuple(shape) and dst.dtype == torch.float32 and dst.is_contiguous() and dst.device == device,
               'gradient destination: contiguous float32 tensor of the gradient\'s shape expected')
        return dst

    def conv3d_backward_weight(self, x, grad_y, with_bias=False, out_w=None, out_b=None):
        """-> grad_weight, or (grad_weight, grad_bias) when with_bias (the bias sum rides on the same pass)."""
        _f32(x, 'x'); _f32(grad_y, 'grad_y')
        return self._backward_weight(CONV, x, grad_y, with_bias, out_w, out_b)

    # ---- the same convolution on the bf16 matrix cores (csrc/conv3d_bf16.hip): nsplit = 3 "bf16x3" (fp32-class accuracy, up to
    # 2.7x the fp32-MFMA rate) or nsplit = 1 (plain bf16 operands: the autocast / BASELINE configs[4] path) ----
    has_conv3d_split = True
    # default arithmetic of the voxel convolutions' forward / backward-data products:
    #   'f16x2'  : power-of-two scaled fp16 hi + lo split of both fp32 operands, 3 partial products, fp32 accumulate (<= 1e-5 vs fp64)
    #   'bf16x3' : exact three-way bf16 split of both fp32 operands, 6 partial products, fp32 accumulate (<= 1e-5 vs fp64)
    #   'fp32'   : v_mfma_f32_32x32x2_f32, one rounding per product (conv3d.hip)
    conv_math = os.environ.get('PVCNN_CONV_MATH', 'f16x2')
    CONV_NSPLIT = {'f16x2': 2, 'bf16x3': 3, 'fp32': 0}

    def absmax_bits(self, x):
        """One uint32 on the device: the bit pattern of max |x| (a 1-word amax buffer: the scalar scale of the f16x2 kernels)."""
        _f32(x, 'x')
        x = _aligned(x)                      # (the kernel takes whole quads from a 16-byte boundary and refuses any other pointer)
        out = torch.empty((1,), dtype=torch.int32, device=x.device)
        _run(self.lib.pvcnn_absmax_bits, 'absmax_bits', x, x, x.numel(), out)
        return out

    # "amax buffers" (include/pvcnn_hip.h): [0] = bits of max |x| over the tensor, [1 + t] = bits of the maximum over all channels of
    # position segment t.  The f16x2 forward / backward-data kernels scale each workgroup's tile of x by the maxima of the segments it
    # touches (an outlier costs precision only inside its own tile); the backward-weight kernels scale by the global maximum, which
    # they take from the table, too (ABI v12) -- so a buffer made with want_global=False has NO word [0] and costs no launch for it.
    PW_AMAX_SEG = 256          # the 1x1 GEMM's point tile
    _TABLE_ONLY = ctypes.c_void_p(1)      # PVCNN_TABLE_ONLY (include/pvcnn_hip.h)
    amax_global = os.environ.get('PVCNN_AMAX_GLOBAL', '0') == '1'      # A/B switch: every amax buffer with its word [0] (ABI v11 behaviour: 11 more launches per PVCNN step)

    def absmax_tiles(self, x, seg, want_global=True):
        """x (B, C, L) -> int32 (1 + B * ceil(L / seg),): the amax buffer of x with segments of `seg` positions (one read of x).
        want_global=False: the table only, word [0] is left unwritten (for consumers that are handed the segment length)."""
        _f32(x, 'x')
        _shape(x.dim() == 3, 'absmax_tiles: x (B,C,L) expected')
        b, c, n = x.shape
        seg = int(seg)
        out = torch.empty((self.lib.pvcnn_absmax_tiles_count(b, n, seg),), dtype=torch.int32, device=x.device)
        ticket = self._tickets(1, x.device)
        want_global = want_global or self.amax_global
        _run(self.lib.pvcnn_absmax_tiles, 'absmax_tiles', x, x, b, c, n, seg, out, ticket if want_global else self._TABLE_ONLY)
        return out

    def conv_amax(self, x, want_global=True):
        """amax buffer of a voxel grid x (B,C,R,R,R) in the layout the Conv3d kernels take: one maximum per z row."""
        return self.absmax_tiles(x.view(x.shape[0], x.shape[1], -1), x.shape[2], want_global)

    def pw_amax(self, x, want_global=True):
        """amax buffer of point features x (B,C,N) in the layout the 1x1 GEMM takes: one maximum per 256-point tile."""
        return self.absmax_tiles(x, self.PW_AMAX_SEG, want_global)

    @staticmethod
    def _amax_seg(amax, tiles, seg):
        """0 when `amax` is a 1-word buffer (scalar scale), `seg` when it carries the `tiles`-entry table; anything else is an error."""
        if amax.numel() == 1:
            return 0
        _shape(amax.numel() == 1 + tiles, f'amax buffer has {amax.numel()} words, expected 1 or {1 + tiles}')
        return seg

    # ---- what the Conv3d and the 1x1 convolution share: `p` is the kind's descriptor, CONV or PW (functional/_product.py).  x and
    # grad_y are (B, C, L ...) with L = the grid resolution R or the number of points N ----
    def _amax_for(self, p, x, amax=None):
        """-> (amax buffer of x: the given one, else measured here with its word [0]; the segment length the kernels are told)."""
        if amax is None:
            amax = getattr(self, p.amax)(x)
        seg = p.amax_seg(self, x.shape[2])
        return amax, self._amax_seg(amax, p.amax_tiles(x.shape[0], x.shape[2], seg), seg)

    def _weight_split(self, p, weight, for_bwd_data, nsplit):
        co, ci = weight.shape[0], weight.shape[1]
        nbytes = p.entry(self.lib, 'weight_split_bytes')(co, ci, int(for_bwd_data), int(nsplit))
        wts = torch.empty((nbytes,), dtype=torch.uint8, device=weight.device)
        _run(p.entry(self.lib, 'weight_split'), f'{p.c}_weight_split', weight, weight, co, ci, int(for_bwd_data), int(nsplit), wts)
        return wts

    def _weight_images(self, p, weight, nsplit):
        co, ci = weight.shape[0], weight.shape[1]
        if int(nsplit) != 2:
            hit = self._bank().take(p.kind, weight, 1) if int(nsplit) == 1 else None      # plain bf16 (autocast): batched as well
            if hit is not None:
                return hit
            return self._weight_split(p, weight, False, nsplit), self._weight_split(p, weight, True, nsplit)
        hit = self._bank().take(p.kind, weight)
        if hit is not None:
            return hit
        wf, wb = (torch.empty((p.entry(self.lib, 'weight_split_bytes')(co, ci, for_bwd_data, 2),), dtype=torch.uint8, device=weight.device)
                  for for_bwd_data in (0, 1))
        _run(p.entry(self.lib, 'weight_split_pair'), f'{p.c}_weight_split_pair', weight, weight, co, ci, wf, wb)
        return wf, wb

    def _product_split(self, p, x, wts, bias, co, nsplit, want_stats=False, amax=None):
        """The split kernel's launch alone: x (B, Ci, L ...) and a pre-split weight image -> y (B, co, L ...) [, stats partials]."""
        b, ci, l = x.shape[0], x.shape[1], x.shape[2]
        y = torch.empty(p.out_shape(b, co, l), dtype=torch.float32, device=x.device)
        part = None
        if want_stats:
            parts = p.entry(self.lib, 'fwd_split_stats_parts')(*p.stats_parts(b, co, l, int(nsplit)))
            part = torch.empty((co, parts, 2), dtype=torch.float32, device=x.device)
        seg = 0
        if int(nsplit) == 2:
            amax, seg = self._amax_for(p, x, amax)
        _run(p.entry(self.lib, 'fwd_split'), f'{p.c}_forward_split', x, x, wts, bias, b, ci, co, l, int(nsplit), amax, seg, y, part)
        return (y, part) if want_stats else y

    def _backward_weight(self, p, x, grad_y, with_bias, out_w, out_b, f16_amax=None):
        """grad_weight [, grad_bias] on the fp32-MFMA kernel, or, with f16_amax = (x_amax, gy_amax) (each an amax buffer or None: one
        global maximum, measured here), on the f16x2 one.  A buffer with a table is passed with its segment length: the kernel then
        takes the global maximum from the table (a table-only buffer has no word [0])."""
        b, ci, l = x.shape[0], x.shape[1], x.shape[2]
        co = grad_y.shape[1]
        name, label, scales = 'bwd_weight', f'{p.c}_backward_weight', ()
        if f16_amax is not None:
            name, label = name + '_f16', label + '_f16'
            given = [(t, amax if amax is not None else self.absmax_bits(t)) for t, amax in zip((x, grad_y), f16_amax)]
            for t, amax in given:
                scales += (amax, self._amax_for(p, t, amax)[1])
        gw = self._grad_out(out_w, p.wgrad_shape(co, ci), x.device)
        gb = self._grad_out(out_b, (co,), x.device) if with_bias else None
        ws = self._scratch(p.entry(self.lib, name + '_workspace_bytes')(b, ci, co, l), x.device)
        _run(p.entry(self.lib, name), label, x, x, grad_y, *scales, b, ci, co, l, gw, gb, ws, ws.numel())
        return (gw, gb) if with_bias else gw

    def _conv_wsplit(self, weight, for_bwd_data, nsplit):
        return self._weight_split(CONV, weight, for_bwd_data, nsplit)

    # ---- the f16x2 weight images of a whole model, refreshed by one launch per kind and step ---------------------------------
    has_weight_bank = True

    def weight_bank_register(self, model):
        """Make the Conv3d / 1x1-convolution weights of `model` eligible for the batched refresh (weight_bank_refresh)."""
        self._bank().register(model)

    def weight_bank_refresh(self):
        """Recompute, in ONE launch per kind, both f16x2 images of every registered weight a forward pass has asked for before, and arm
        them: the next conv_weight_images / pw_weight_images call for such a weight takes its pair from the bank instead of launching.
        Call right before the forward pass of a training step (after the optimizer step that changed the weights).  A weight that is
        not armed -- not registered, first sighting, a second forward pass without a refresh, changed in place since (version
        counter) -- is split by its own launch as before: never stale."""
        self._bank().refresh()

    def weight_bank_invalidate(self):
        """Every armed image pair is stale from now on: call after the parameters were written behind torch's back (raw device pointers
        -- pvcnn_amd.optim.FlatAdam; in-place torch updates are caught by the tensors' version counters already)."""
        bank = getattr(self, '_weight_bank', None)
        if bank is not None:
            bank.epoch += 1

    def _bank(self):
        if getattr(self, '_weight_bank', None) is None:
            self._weight_bank = _WeightBank(self)
        return self._weight_bank

    def conv_weight_images(self, weight, nsplit):
        """(forward image, backward-data image) of a Conv3d weight; f16x2: both from ONE launch (a training step needs both and the
        weights do not change between its forward and its backward)."""
        return self._weight_images(CONV, weight, nsplit)

    def pw_weight_images(self, weight, nsplit):
        """(forward image, backward-data image) of a 1x1 convolution weight (Co, Ci); f16x2: one launch."""
        return self._weight_images(PW, weight, nsplit)

    def conv3d_forward_split(self, x, weight, bias, nsplit, want_stats=False, amax=None):
        _f32(x, 'x'); _f32(weight, 'weight')
        _shape(x.dim() == 5 and weight.dim() == 5 and tuple(weight.shape[2:]) == (3, 3, 3) and weight.shape[1] == x.shape[1]
               and x.shape[2] == x.shape[3] == x.shape[4], 'conv3d: x (B,Ci,R,R,R), weight (Co,Ci,3,3,3) expected')
        if bias is not None:
            _f32(bias, 'bias')
        return self._product_split(CONV, x, self._weight_split(CONV, weight, False, nsplit), bias, weight.shape[0], nsplit, want_stats, amax)

    def conv3d_igemm_split(self, x, wts, bias, co, nsplit, want_stats=False, amax=None, rows=None):
        """The implicit-GEMM launch alone (pre-split weight image `wts`; f16x2: `amax` = conv_amax(x), or a 1-word absmax_bits(x)
        for the single-scale mode): x (B,Ci,R,R,R) -> y (B,co,R,R,R) [, stats partials].  rows = voxel_need_rows(...) (bias None, no
        statistics): only the z rows it marks are read of y -- a tile of y without one comes as zeros (pvcnn_conv3d_fwd_split_rows)."""
        if rows is not None:
            _f32(x, 'x'); _i32(rows, 'rows')
            b, ci, r = x.shape[0], x.shape[1], x.shape[2]
            _shape(x.dim() == 5 and x.shape[2] == x.shape[3] == x.shape[4] and bias is None and not want_stats
                   and rows.numel() == b * r * r and rows.is_contiguous() and rows.device == x.device,
                   'conv3d_igemm_split: rows goes with a cube grid, no bias and no statistics and has B * R * R words')
            y = torch.empty(CONV.out_shape(b, co, r), dtype=torch.float32, device=x.device)
            seg = 0
            if int(nsplit) == 2:
                amax, seg = self._amax_for(CONV, x, amax)
            _run(self.lib.pvcnn_conv3d_fwd_split_rows, 'conv3d_forward_split_rows', x, x, wts, b, ci, co, r, int(nsplit), amax, seg, y, rows)
            return y
        return self._product_split(CONV, x, wts, bias, co, nsplit, want_stats, amax)

    def conv3d_backward_data_split(self, grad_y, weight, nsplit, amax=None):
        _f32(grad_y, 'grad_y'); _f32(weight, 'weight')
        # a convolution with Ci and Co exchanged on the flipped weights
        return self._product_split(CONV, grad_y, self._weight_split(CONV, weight, True, nsplit), None, weight.shape[1], nsplit, False, amax)

    # ---- backward-weight in f16x2 (csrc/conv3d_wgrad_f16.hip): R = 8, 12, 16 and 32; other grids stay on the fp32-MFMA kernel ----
    def conv3d_backward_weight_f16_serves(self, x):
        return x.dim() == 5 and x.shape[2] in (8, 12, 16, 32)

    def conv3d_backward_weight_f16(self, x, grad_y, x_amax=None, gy_amax=None, with_bias=False, out_w=None, out_b=None):
        """grad_w (Co,Ci,3,3,3) [, grad_bias]: x (B,Ci,R,R,R), grad_y (B,Co,R,R,R); *_amax = amax buffers of the two tensors.  The
        kernel scales by each tensor's global maximum: the one word of a 1-word buffer, else the maximum over the table (ABI v12:
        word [0] of a table-only buffer is uninitialised and never read)."""
        _f32(x, 'x'); _f32(grad_y, 'grad_y')
        _shape(self.conv3d_backward_weight_f16_serves(x) and tuple(grad_y.shape) == CONV.out_shape(x.shape[0], grad_y.shape[1], x.shape[2]),
               'conv3d_backward_weight_f16: R must be 8, 12, 16 or 32')
        return self._backward_weight(CONV, x, grad_y, with_bias, out_w, out_b, (x_amax, gy_amax))

    # ---- SharedMLP 1x1 convolutions as channel-major MFMA GEMMs (csrc/pointwise.hip) --------------------
    has_pwconv = True

    def pwconv_forward(self, x, weight, bias, want_stats=False):
        """x (B,Ci,N), weight (Co,Ci), bias (Co) or None -> y (B,Co,N)."""
        _f32(x, 'x'); _f32(weight, 'weight')
        _shape(x.dim() == 3 and weight.dim() == 2 and weight.shape[1] == x.shape[1], 'pwconv: x (B,Ci,N), weight (Co,Ci) expected')
        if bias is not None:
            _f32(bias, 'bias')
        b, ci, n = x.shape
        co = weight.shape[0]
        k32 = (ci + 31) // 32 * 32                 # wt rows: K rounded up to the kernel's 32-channel chunk (zero tail)
        wt = torch.empty((k32, co), dtype=torch.float32, device=x.device)
        y = torch.empty((b, co, n), dtype=torch.float32, device=x.device)
        part = None
        if want_stats:
            part = torch.empty((co, self.lib.pvcnn_pwconv_fwd_stats_parts(b, n), 2), dtype=torch.float32, device=x.device)
        _run(self.lib.pvcnn_pwconv_transpose, 'pwconv_transpose', x, weight, co, ci, wt)
        if want_stats:
            _run(self.lib.pvcnn_pwconv_fwd_stats, 'pwconv_forward', x, x, wt, k32, bias, b, ci, co, n, y, part)
        else:
            _run(self.lib.pvcnn_pwconv_fwd, 'pwconv_forward', x, x, wt, k32, bias, b, ci, co, n, y)
        return (y, part) if want_stats else y

    def pwconv_backward_data(self, grad_y, weight):
        """grad_y (B,Co,N), weight (Co,Ci) -> grad_x (B,Ci,N): the forward GEMM with K = Co on the weight as stored."""
        _f32(grad_y, 'grad_y'); _f32(weight, 'weight')
        b, co, n = grad_y.shape
        ci = weight.shape[1]
        gx = torch.empty((b, ci, n), dtype=torch.float32, device=grad_y.device)
        _run(self.lib.pvcnn_pwconv_fwd, 'pwconv_backward_data', grad_y, grad_y, weight, co, None, b, co, ci, n, gx)
        return gx

    # ---- the same GEMMs on the bf16 matrix cores (csrc/pointwise_bf16.hip), nsplit = 3 (bf16x3) or 1 (bf16) ----
    has_pwconv_split = True
    # arithmetic of the SharedMLP forward / backward-data products: 'fp32' (pointwise.hip), 'f16x2' or 'bf16x3' (pointwise_bf16.hip)
    pw_math = os.environ.get('PVCNN_PW_MATH', 'f16x2')
    PW_NSPLIT = {'f16x2': 2, 'bf16x3': 3, 'fp32': 0}
    # K * M * B * N below which the split forward / backward-data path is not worth its extra launches (weight images, an amax pass
    # when the producer left no table).  Round 3, after the straight-line / pipelined kernels: a sweep of the threshold from 2^32
    # (round 2) down to "always" on one box -- PVCNN 2121 -> 2157, PVCNN++ 429 -> 484, ShapeNet 1418 -> 1497 clouds/s, Frustum
    # 3763 -> 4095 frustums/s, flat below 2^24 (profiles/ab/r03w_*).  Backward-weight has its own bar: the f16x2 kernel writes
    # 128 x 128 partial tiles per partition of the points, a loss on small weight matrices (64 x 64: 0.17 vs 0.05 ms).
    pw_split_min_macs = 1 << 24
    pw_wgrad_f16_min_macs = 1 << 32

    def _pw_wsplit(self, weight, for_bwd_data, nsplit):
        return self._weight_split(PW, weight, for_bwd_data, nsplit)

    def pwconv_gemm_split(self, x, wts, bias, m, nsplit, want_stats=False, amax=None):
        """The GEMM launch alone: x (B,K,N), pre-split weight image (f16x2: amax = pw_amax(x), or a 1-word absmax_bits(x) for the
        single-scale mode) -> y (B,m,N) [, stats partials]."""
        return self._product_split(PW, x, wts, bias, m, nsplit, want_stats, amax)

    def pwconv_forward_split(self, x, weight, bias, nsplit, want_stats=False, amax=None):
        _f32(x, 'x'); _f32(weight, 'weight')
        _shape(x.dim() == 3 and weight.dim() == 2 and weight.shape[1] == x.shape[1], 'pwconv: x (B,Ci,N), weight (Co,Ci) expected')
        if bias is not None:
            _f32(bias, 'bias')
        return self._product_split(PW, x, self._weight_split(PW, weight, False, nsplit), bias, weight.shape[0], nsplit, want_stats, amax)

    def pwconv_backward_data_split(self, grad_y, weight, nsplit, amax=None):
        _f32(grad_y, 'grad_y'); _f32(weight, 'weight')
        return self._product_split(PW, grad_y, self._weight_split(PW, weight, True, nsplit), None, weight.shape[1], nsplit, False, amax)

    # ---- the activation tail (include/pvcnn_hip.h: the *_act entry points): y = LeakyReLU(product + bias, act_slope) written once,
    # and y's amax buffer emitted by the same epilogues -- what an eval-mode [conv, BatchNorm, activation] triple is once the
    # BatchNorm sits in the weights (functional/_fold.py).  Counterparts of conv3d_igemm_split / pwconv_gemm_split / conv3d_forward /
    # pwconv_forward on PREPARED weights (nothing is split or transposed here); each -> (y, y's amax buffer | None).
    has_product_act = True

    def _amax_table(self, p, b, l, device, emit):
        """-> (y's zeroed table-only amax buffer -- the epilogues combine into it with atomicMax --, its segment length) or (None, 0)."""
        if not emit:
            return None, 0
        seg = p.amax_seg(self, l)
        return torch.zeros((1 + p.amax_tiles(b, l, seg),), dtype=torch.int32, device=device), seg

    def _product_split_act(self, p, x, wts, bias, co, nsplit, act_slope, amax=None, emit_amax=True):
        b, ci, l = x.shape[0], x.shape[1], x.shape[2]
        y = torch.empty(p.out_shape(b, co, l), dtype=torch.float32, device=x.device)
        seg = 0
        if int(nsplit) == 2:
            amax, seg = self._amax_for(p, x, amax)
        table, yseg = self._amax_table(p, b, l, x.device, emit_amax)
        _run(p.entry(self.lib, 'fwd_split_act'), f'{p.c}_forward_split_act', x, x, wts, bias, b, ci, co, l, int(nsplit), amax, seg, y, None,
             float(act_slope), table, yseg)
        return y, table

    def conv3d_igemm_split_act(self, x, wts, bias, co, nsplit, act_slope, amax=None, emit_amax=True):
        """conv3d_igemm_split + the activation tail: -> (y (B,co,R,R,R), y's amax buffer with one maximum per z row | None)."""
        return self._product_split_act(CONV, x, wts, bias, co, nsplit, act_slope, amax, emit_amax)

    def pwconv_gemm_split_act(self, x, wts, bias, m, nsplit, act_slope, amax=None, emit_amax=True):
        """pwconv_gemm_split + the activation tail: -> (y (B,m,N), y's amax buffer with one maximum per 256 points | None)."""
        return self._product_split_act(PW, x, wts, bias, m, nsplit, act_slope, amax, emit_amax)

    def conv3d_forward_act(self, x, wt, bias, co, act_slope, emit_amax=True):
        """The fp32-MFMA Conv3d on a transformed weight (`_conv_wt`) + the activation tail."""
        b, ci, r = x.shape[0], x.shape[1], x.shape[2]
        y = torch.empty((b, co, r, r, r), dtype=torch.float32, device=x.device)
        table, yseg = self._amax_table(CONV, b, r, x.device, emit_amax)
        _run(self.lib.pvcnn_conv3d_fwd_act, 'conv3d_forward_act', x, x, wt, bias, b, ci, co, r, y, float(act_slope), table, yseg)
        return y, table

    def pwconv_weight_transposed(self, weight):
        """(Co,Ci) -> the (K32,Co) layout pvcnn_pwconv_fwd takes (K rounded up to the 32-channel chunk, zero tail)."""
        co, ci = weight.shape
        wt = torch.empty(((ci + 31) // 32 * 32, co), dtype=torch.float32, device=weight.device)
        _run(self.lib.pvcnn_pwconv_transpose, 'pwconv_transpose', weight, weight, co, ci, wt)
        return wt

    def pwconv_forward_act(self, x, wt, bias, co, act_slope, emit_amax=True):
        """The fp32-MFMA 1x1 GEMM on a transposed weight (`pwconv_weight_transposed`) + the activation tail."""
        b, ci, n = x.shape
        y = torch.empty((b, co, n), dtype=torch.float32, device=x.device)
        table, yseg = self._amax_table(PW, b, n, x.device, emit_amax)
        _run(self.lib.pvcnn_pwconv_fwd_act, 'pwconv_forward_act', x, x, wt, wt.shape[0], bias, b, ci, co, n, y, float(act_slope), table, yseg)
        return y, table

    def pwconv_backward_weight(self, x, grad_y, with_bias=False, out_w=None, out_b=None):
        """-> grad_weight (Co,Ci), or (grad_weight, grad_bias) when with_bias."""
        _f32(x, 'x'); _f32(grad_y, 'grad_y')
        return self._backward_weight(PW, x, grad_y, with_bias, out_w, out_b)

    def pwconv_backward_weight_f16_serves(self, x):
        return x.dim() == 3 and x.shape[2] % 4 == 0

    def pwconv_backward_weight_f16(self, x, grad_y, x_amax=None, gy_amax=None, with_bias=False, out_w=None, out_b=None):
        """f16x2 on the fp16 matrix cores (csrc/pointwise_wgrad_f16.hip): -> grad_weight (Co,Ci) [, grad_bias]."""
        _f32(x, 'x'); _f32(grad_y, 'grad_y')
        _shape(self.pwconv_backward_weight_f16_serves(x) and tuple(grad_y.shape) == PW.out_shape(x.shape[0], grad_y.shape[1], x.shape[2]),
               'pwconv_backward_weight_f16: N must be a multiple of 4')
        return self._backward_weight(PW, x, grad_y, with_bias, out_w, out_b, (x_amax, gy_amax))

    # ---- BatchNorm + ReLU/LeakyReLU in two passes each way (csrc/bnact.hip) ---------------------------
    has_bnact = True

    BNACT_AMAX_MAX_SEG = 256   # the apply passes emit amax buffers for segments up to this long

    has_bnact_dropout = True

    def dropout_keep_mask(self, seed, p, numel):
        """keep(e), e = 0 .. numel - 1, of the dropout fused into bnact_forward / bnact_backward (drop=(seed, p)) -> bool tensor (tests)."""
        keep = torch.empty((int(numel),), dtype=torch.uint8, device=seed.device)
        _run(self.lib.pvcnn_dropout_keep_mask, 'dropout_keep_mask', seed, seed, float(p), int(numel), keep)
        return keep.bool()

    def bnact_forward(self, x, gamma, beta, running_mean, running_var, training, momentum, eps, slope, stats=None, amax_seg=0,
                      y_amax=None, drop=None):
        """x (B,C,S) -> (y, mean, rstd).  Training: batch statistics (running stats updated in place);
        eval: running statistics.  stats = (mean, rstd) already known (from a convolution epilogue +
        bn_finalize): only the normalise + activate pass runs.
        amax_seg > 0: -> (y, mean, rstd, y_amax), y's amax buffer with segments of amax_seg positions emitted by the apply pass.
        y_amax given: the buffer bn_finalize(..., zero_word=y_amax) already armed (all of it is zero: the pass then needs no
        reduction launch behind it).
        drop = (seed: one int64 on the device, p): the nn.Dropout(p) behind the pair, applied by the same pass (needs amax_seg > 0)."""
        _f32(x, 'x')
        b, c, s3 = x.shape
        dev = x.device
        y = torch.empty_like(x)
        if stats is not None:
            mean, rstd = stats
            training = False                    # the kernel entry's "statistics are given" mode
        elif training:
            mean, rstd = _mean_rstd(c, dev)
        else:
            mean = running_mean.clone()          # saved for backward: must not alias the live buffer
            rstd = torch.rsqrt(running_var + eps)
        ws = self._scratch(self.lib.pvcnn_bnact_workspace_bytes(b, c, s3), dev)
        amax_seg = int(amax_seg)
        armed = y_amax is not None
        if amax_seg > 0 and not armed:
            y_amax = self.amax_buffer(b, s3, amax_seg, dev)
        _run(self.lib.pvcnn_bnact_fwd, 'bnact_forward', x, x, gamma, beta, running_mean if training else None,
             running_var if training else None, b, c, s3, float(eps), float(momentum), float(slope), int(bool(training)), mean, rstd, y,
             y_amax if amax_seg > 0 else None, amax_seg, int(armed), ws, ws.numel(), drop[0] if drop else None,
             float(drop[1]) if drop else 0.0)
        return (y, mean, rstd, y_amax) if amax_seg > 0 else (y, mean, rstd)

    has_bnact_rowmax = True

    def amax_and_row_keys(self, b, c, n, seg, device):
        """One uninitialised int32 buffer holding the amax buffer of a (b, c, n) tensor AND its b * c 64-bit row keys (8-byte aligned)
        -> (whole buffer: hand it to bn_finalize(zero_word=...), amax view, keys view)."""
        words = self.lib.pvcnn_absmax_tiles_count(int(b), int(n), int(seg))
        off = (words + 1) // 2 * 2
        whole = torch.empty((off + 2 * int(b) * int(c),), dtype=torch.int32, device=device)
        return whole, whole[:words], whole[off:]

    def bnact_apply_rowmax(self, x, gamma, beta, mean, rstd, slope, amax_seg, y_amax, row_keys, out=None):
        """The apply pass of bnact_forward on known statistics, also emitting the row maxima of y: x (B,C,S) -> (y, winners (B,C) int64,
        values (B,C)) == (y, *y.max(dim=-1)[::-1]).  y_amax / row_keys: the views of amax_and_row_keys, ZEROED (bn_finalize)."""
        _f32(x, 'x')
        x = _aligned(x)                      # (as absmax_bits: 16-byte loads only)
        b, c, s3 = x.shape
        _shape(s3 % 256 == 0 and amax_seg % 4 == 0 and 0 < amax_seg <= 256 and 256 % amax_seg == 0,
               'bnact_apply_rowmax: S % 256 == 0 and an amax_seg that is a multiple of 4 and divides 256 expected')
        # out: where y goes -- a (B, C, S) view whose rows are contiguous inside a sample and whose samples may be further apart: the
        # channel slice of the classifier's concatenation that this tensor will be (the concatenation then copies nothing for it)
        if out is None:
            y = torch.empty_like(x)
        else:
            y = out
            _dev(y, 'out')
            _shape(tuple(y.shape) == tuple(x.shape) and y.dtype == torch.float32 and y.stride(2) == 1 and y.stride(1) == s3
                   and y.stride(0) >= c * s3 and y.stride(0) % 4 == 0 and y.data_ptr() % 16 == 0,
                   'bnact_apply_rowmax: out must be a (B, C, S) float32 view with contiguous, 16-byte aligned rows')
        ybs = int(y.stride(0)) if b > 1 else c * s3
        winners = torch.empty((b, c), dtype=torch.int64, device=x.device)
        values = torch.empty((b, c), dtype=torch.float32, device=x.device)
        _run(self.lib.pvcnn_bnact_apply_rowmax, 'bnact_apply_rowmax', x, x, gamma, beta, mean, rstd, b, c, s3, float(slope), y, ybs, y_amax,
             int(amax_seg), row_keys)
        _run(self.lib.pvcnn_row_keys_decode, 'row_keys_decode', x, row_keys, y, b * c, s3, winners, values, c, ybs)
        return y, winners, values

    has_devox_bnact = True

    def amax_buffer(self, b, n, seg, device):
        """Uninitialised amax buffer for a (b, C, n) tensor with segments of `seg` positions."""
        return torch.empty((self.lib.pvcnn_absmax_tiles_count(int(b), int(n), int(seg)),), dtype=torch.int32, device=device)

    def bn_finalize(self, part, count, running_mean, running_var, momentum, eps, shift=None, zero_word=None, counter=None):
        """(C, nparts, 2) partial sums of (y - shift) from a convolution epilogue (shift = that convolution's bias, or None)
        -> (mean, rstd) of y; running stats updated in place.  zero_word: an amax buffer this launch zeroes (arming it for the
        apply pass that follows, which fills it by atomic maxima: bnact_forward(..., y_amax=zero_word)).  counter: the module's int64 num_batches_tracked,
        incremented by the same launch."""
        c, nparts = part.shape[0], part.shape[1]
        mean, rstd = _mean_rstd(c, part.device)
        _run(self.lib.pvcnn_bn_finalize, 'bn_finalize', part, part, c, nparts, float(count), float(eps), float(momentum), shift,
             running_mean, running_var, mean, rstd, zero_word, zero_word.numel() if zero_word is not None else 0, counter)
        return mean, rstd

    def bn_stats(self, x, running_mean, running_var, momentum, eps):
        """Training-mode statistics of x (B,C,S): -> (mean, rstd); running stats updated in place (may be None)."""
        _f32(x, 'x')
        b, c, s3 = x.shape
        mean, rstd = _mean_rstd(c, x.device)
        ws = self._scratch(self.lib.pvcnn_bnact_workspace_bytes(b, c, s3), x.device)
        _run(self.lib.pvcnn_bn_stats, 'bn_stats', x, x, running_mean, running_var, b, c, s3, float(eps), float(momentum), mean, rstd,
             ws, ws.numel())
        return mean, rstd

    # PVCNN_POINT_FUSED=0 (read once per process): PVConv's point branch through its own BatchNorm + ReLU pass (A/B; fused is the default)
    has_point_branch_fused = os.environ.get('PVCNN_POINT_FUSED', '1') != '0'

    def trilinear_devoxelize_bnact_forward(self, r, is_training, coords, features, gamma, beta, mean, rstd, slope, addend=None,
                                           se_scale=None, addend_bn=None):
        """trilinear_devoxelize_forward of leaky_relu(bn(features)) [* se_scale (B,C): SE3d's excitation] without materialising that
        tensor: features (B,C,R^3) is the PRE-BatchNorm grid, mean / rstd (C) its statistics.
        addend_bn = (gamma | None, beta | None, mean, rstd, slope): the addend is PRE-BatchNorm too (PVConv's point branch behind its
        1x1 convolution); its BatchNorm + ReLU | LeakyReLU(slope) is applied where the gather's store adds it (no se_scale then)."""
        _f32(features, 'features'); _f32(coords, 'coords')
        r = int(r)
        _shape(features.dim() == 3 and coords.dim() == 3 and coords.shape[1] == 3
               and coords.shape[0] == features.shape[0] and features.shape[2] == r * r * r,
               'trilinear_devoxelize: coords (B,3,N), features (B,C,R^3) expected')
        b, c = features.shape[:2]
        n = coords.shape[2]
        dev = features.device
        if addend is not None:
            _f32(addend, 'addend')
            _shape(tuple(addend.shape) == (b, c, n), 'trilinear_devoxelize: addend (B,C,N) expected')
        if se_scale is not None:
            _f32(se_scale, 'se_scale')
            _shape(tuple(se_scale.shape) == (b, c), 'trilinear_devoxelize: se_scale (B,C) expected')
        outs = torch.empty((b, c, n), dtype=torch.float32, device=dev)
        if is_training:
            inds = torch.empty((b, 8, n), dtype=torch.int32, device=dev)
            wgts = torch.empty((b, 8, n), dtype=torch.float32, device=dev)
        else:
            inds, wgts = _dummies(dev)
        if addend_bn is not None:
            if addend is None or se_scale is not None or len(addend_bn) != 5:
                raise RuntimeError('trilinear_devoxelize: addend_bn = (gamma, beta, mean, rstd, slope) goes with an addend and without se_scale')
            a_gamma, a_beta, a_mean, a_rstd, a_slope = addend_bn
            for name, t, optional in (('gamma', a_gamma, True), ('beta', a_beta, True), ('mean', a_mean, False), ('rstd', a_rstd, False)):
                if t is None and optional:
                    continue
                _f32(t, 'addend_bn ' + name)
                if tuple(t.shape) != (c,) or not t.is_contiguous():
                    raise RuntimeError(f'trilinear_devoxelize: addend_bn {name} (C,) contiguous expected')
            _run(self.lib.pvcnn_trilinear_devox_bnact_addbn_fwd, 'trilinear_devoxelize_bnact_forward', features, coords, features, gamma,
                 beta, mean, rstd, float(slope), b, c, n, r, int(bool(is_training)), inds if is_training else None,
                 wgts if is_training else None, addend, a_gamma, a_beta, a_mean, a_rstd, float(a_slope), outs)
            return [outs, inds, wgts]
        _run(self.lib.pvcnn_trilinear_devox_bnact_fwd, 'trilinear_devoxelize_bnact_forward', features, coords, features, gamma, beta,
             mean, rstd, float(slope), b, c, n, r, int(bool(is_training)), inds if is_training else None,
             wgts if is_training else None, addend, se_scale, outs)
        return [outs, inds, wgts]

    # ---- torch.cat(features, dim=1) of the classifier input + the amax buffer of its output in one pass (csrc/bnact.hip) ----
    has_concat_points = True

    def concat_points(self, tensors, want_amax=True, out=None, in_place=None, want_global=True):
        """tensors: (B, C_i, N) float32, each with contiguous rows inside a cloud (a channel slice is fine) or broadcast over the points
        (stride 0 along N, contiguous (B, C_i)) -> (out (B, sum C_i, N), its amax buffer with 256-point segments | None).
        out: the (B, sum C_i, N) buffer to fill; in_place = {i: amax buffer of tensors[i]}: those sources ALREADY ARE their channel slice
        of `out` (the pass that produced them wrote them there: bnact_apply_rowmax(..., out=)): nothing is copied for them.
        want_global=False: the amax buffer's table only, no word [0] (see absmax_tiles)."""
        _shape(0 < len(tensors) <= 8, 'concat_points: 1..8 sources')
        b, n = tensors[0].shape[0], tensors[0].shape[2]
        ptrs, bstr, chans, pstr = [], [], [], []
        for i, t in enumerate(tensors):
            _dev(t, 'source')
            _shape(t.dim() == 3 and t.dtype == torch.float32 and t.shape[0] == b and t.shape[2] == n, 'concat_points: (B, C_i, N) float sources expected')
            c = t.shape[1]
            if n > 1 and t.stride(2) == 0:
                _shape(t.stride(1) == 1 or c == 1, 'concat_points: a broadcast source must be contiguous over (B, C)')
                pstr.append(0); bstr.append(t.stride(0) if b > 1 else c)
            else:
                _shape((n == 1 or t.stride(2) == 1) and (c == 1 or t.stride(1) == n), 'concat_points: rows must be contiguous inside a cloud')
                # (a single cloud: torch leaves stride(0) of a size-1 dimension arbitrary, so it is stated -- except for a source that
                #  already IS its channel slice of `out`, whose cloud stride is the buffer's and is checked as such by the library)
                pstr.append(1); bstr.append(t.stride(0) if (b > 1 or (in_place and i in in_place)) else c * n)
            ptrs.append(t.data_ptr()); chans.append(c)
        k = len(tensors)
        if out is None:
            out = torch.empty((b, sum(chans), n), dtype=torch.float32, device=tensors[0].device)
        else:
            _f32(out, 'out')
            _shape(tuple(out.shape) == (b, sum(chans), n), 'concat_points: out (B, sum C_i, N) expected')
        pre = [None] * k
        for i, table in (in_place or {}).items():
            _shape(want_amax and table is not None and table.dtype == torch.int32 and table.is_cuda, 'concat_points: an in-place source comes with its amax buffer')
            pre[i] = table.data_ptr()
        amax = self.amax_buffer(b, n, self.PW_AMAX_SEG, out.device) if want_amax else None
        ticket = self._tickets(1, out.device) if want_amax else None
        _run(self.lib.pvcnn_concat_points, 'concat_points', out, (ctypes.c_void_p * k)(*ptrs), (ctypes.c_long * k)(*bstr),
             (ctypes.c_int * k)(*chans), (ctypes.c_int * k)(*pstr), (ctypes.c_void_p * k)(*pre) if in_place else None, k, b, n, out, amax,
             ticket if want_global or self.amax_global or not want_amax else self._TABLE_ONLY)
        return out, amax

    # ---- the two halves of bnact_backward on their own (PVConv's SE tail puts the excitation's backward between them) ----
    has_bnact_split_bwd = True

    # ---- Linear + BatchNorm1d + ReLU on a handful of rows (models/utils.py:11-12: the cloud-descriptor heads), csrc/dense.hip ----
    has_dense_bn_relu = True

    def dense_bn_relu_supported(self, rows, cin, cout):
        return bool(self.lib.pvcnn_dense_bn_relu_supported(int(rows), int(cin), int(cout)))

    def dense_bn_relu_forward(self, x, weight, bias, gamma, beta, running_mean, running_var, counter, eps, momentum):
        """x (rows, Cin) -> (y (rows, Cout), z, mean, rstd): y = relu(batch_norm(x W^T + bias)) with batch statistics in ONE launch;
        running statistics / num_batches_tracked updated in place (None: not tracked)."""
        _f32(x, 'x'); _f32(weight, 'weight')
        _shape(x.dim() == 2 and weight.dim() == 2 and weight.shape[1] == x.shape[1], 'dense_bn_relu: x (rows, Cin), weight (Cout, Cin) expected')
        rows, cin = x.shape
        cout = weight.shape[0]
        dev = x.device
        z = torch.empty((rows, cout), dtype=torch.float32, device=dev)
        y = torch.empty((rows, cout), dtype=torch.float32, device=dev)
        mean, rstd = _mean_rstd(cout, dev)
        _run(self.lib.pvcnn_dense_bn_relu_fwd, 'dense_bn_relu_forward', x, x, weight, bias, gamma, beta, running_mean, running_var, counter,
             rows, cin, cout, float(eps), float(momentum), z, y, mean, rstd)
        return y, z, mean, rstd

    def dense_bn_relu_backward(self, x, grad_y, z, mean, rstd, gamma, beta, out_w=None, out_b=None, out_gamma=None, out_beta=None):
        """-> (grad_z (rows, Cout), grad_weight (Cout, Cin), grad_bias, grad_gamma, grad_beta) in ONE launch (grad_x = grad_z @ weight is
        the caller's GEMM).  out_*: where to write the parameter gradients (slots of a flat gradient bucket), else fresh tensors."""
        _f32(x, 'x'); _f32(grad_y, 'grad_y')
        rows, cin = x.shape
        cout = z.shape[1]
        dev = x.device
        gz = torch.empty((rows, cout), dtype=torch.float32, device=dev)
        gw = self._grad_out(out_w, (cout, cin), dev)
        gb = self._grad_out(out_b, (cout,), dev)
        gg = self._grad_out(out_gamma, (cout,), dev)
        gbeta = self._grad_out(out_beta, (cout,), dev)
        _run(self.lib.pvcnn_dense_bn_relu_bwd, 'dense_bn_relu_backward', x, x, grad_y, z, mean, rstd, gamma, beta, rows, cin, cout,
             gz, gw, gb, gg, gbeta)
        return gz, gw, gb, gg, gbeta

    # ---- max over the neighbours of a centre (modules/pointnet.py:85) ------------------------------------------------
    has_neighbor_max = True

    def neighbor_max_supported(self, k):
        return bool(self.lib.pvcnn_neighbor_max_supported(int(k)))

    def neighbor_max_forward(self, x):
        """x (..., K) contiguous -> (max over K (...), winners (...) uint8)."""
        _f32(x, 'x')
        k = x.shape[-1]
        rows = x.numel() // k
        out = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device)
        winners = torch.empty(x.shape[:-1], dtype=torch.uint8, device=x.device)
        _run(self.lib.pvcnn_neighbor_max_fwd, 'neighbor_max_forward', x, x, rows, k, out, winners)
        return out, winners

    def neighbor_max_backward(self, grad_out, winners, k):
        """-> grad_x (..., K): grad_out at the winner, zeros elsewhere (one write pass)."""
        _f32(grad_out, 'grad_out')
        _shape(grad_out.shape == winners.shape and winners.dtype == torch.uint8 and winners.is_contiguous(), 'neighbor_max: winners (...) uint8 expected')
        gx = torch.empty(tuple(grad_out.shape) + (int(k),), dtype=torch.float32, device=grad_out.device)
        _run(self.lib.pvcnn_neighbor_max_bwd, 'neighbor_max_backward', grad_out, grad_out, winners, grad_out.numel(), int(k), gx)
        return gx

    def row_argmax(self, x, with_values=False):
        """x (..., K) contiguous, K % 4 == 0 -> winners (...) int64 [, values (...)]: `x.max(dim=-1)` for long rows, one read."""
        _f32(x, 'x')
        k = x.shape[-1]
        _shape(k % 4 == 0 and k > 0, 'row_argmax: the last dimension must be a multiple of 4')
        winners = torch.empty(x.shape[:-1], dtype=torch.int64, device=x.device)
        values = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device) if with_values else None
        _run(self.lib.pvcnn_row_argmax, 'row_argmax', x, x, x.numel() // k, k, winners, values)
        return (winners, values) if with_values else winners

    has_frustum_loss = True

    def frustum_box_loss(self, center, center_reg, heading_scores, size_scores, hrn, srn, hr, sr, heading_bin_id, size_template_id,
                         heading_residual, size_residual, center_t, templates, bin_centers, bin_width, w_heading, w_size, w_corners):
        """csrc/frustum.hip: the box part of FrustumPointNetLoss (modules/frustum.py:43-124) and its gradient in one launch ->
        (loss, 0-dim; grads, flat: the gradients with respect to the first eight arguments, concatenated in that order)."""
        outs = (center, center_reg, heading_scores, size_scores, hrn, srn, hr, sr)
        for t in outs + (heading_residual, size_residual, center_t, templates, bin_centers):
            _f32(t, 'frustum_box_loss input')
        b, nh, ns = center.shape[0], heading_scores.shape[1], size_scores.shape[1]
        _shape(tuple(center.shape) == (b, 3) and tuple(center_reg.shape) == (b, 3) and tuple(center_t.shape) == (b, 3)
               and tuple(heading_scores.shape) == (b, nh) and tuple(hrn.shape) == (b, nh) and tuple(hr.shape) == (b, nh)
               and tuple(size_scores.shape) == (b, ns) and tuple(srn.shape) == (b, ns, 3) and tuple(sr.shape) == (b, ns, 3)
               and tuple(heading_residual.shape) == (b,) and tuple(size_residual.shape) == (b, 3) and tuple(templates.shape) == (ns, 3)
               and tuple(bin_centers.shape) == (nh,) and tuple(heading_bin_id.shape) == (b,) and tuple(size_template_id.shape) == (b,)
               and heading_bin_id.dtype == torch.int64 and size_template_id.dtype == torch.int64
               and heading_bin_id.is_contiguous() and size_template_id.is_contiguous(), 'frustum_box_loss: shapes of modules/frustum.py:57-75 expected')
        loss = torch.empty((), dtype=torch.float32, device=center.device)
        grads = torch.empty((self.lib.pvcnn_frustum_box_loss_grad_floats(b, nh, ns),), dtype=torch.float32, device=center.device)
        _run(self.lib.pvcnn_frustum_box_loss, 'frustum_box_loss', center, *outs, heading_bin_id, size_template_id, heading_residual,
             size_residual, center_t, templates, bin_centers, b, nh, ns, float(bin_width), float(w_heading), float(w_size),
             float(w_corners), loss, grads)
        return loss, grads

    has_se_excite = True

    def se_excite_forward(self, part, gamma, beta, w1, w2, s3):
        """part (C,B,slices,2) from bnact_partial_sums_raw(grad_y=None) -> (a_sum (B,C), ax_sum (B,C), squeezed (B,C), hidden (B,H),
        excite (B,C)): the slice sums + SE3d's two Linear layers + ReLU + Sigmoid on the squeeze, one launch."""
        c, b, slices, _ = part.shape
        h = w1.shape[0]
        _shape(tuple(w1.shape) == (h, c) and tuple(w2.shape) == (c, h) and c <= 2048 and h <= 256, 'se_excite: W1 (H,C), W2 (C,H), C <= 2048, H <= 256')
        dev = part.device
        a_sum, ax_sum, squeezed, excite = (torch.empty((b, c), dtype=torch.float32, device=dev) for _ in range(4))
        hidden = torch.empty((b, h), dtype=torch.float32, device=dev)
        _run(self.lib.pvcnn_se_excite_fwd, 'se_excite_fwd', part, part, slices, gamma, beta, w1, w2, b, c, h, 1.0 / float(s3),
             a_sum, ax_sum, squeezed, hidden, excite)
        return a_sum, ax_sum, squeezed, hidden, excite

    def se_excite_backward(self, part, a_sum, ax_sum, gamma, beta, squeezed, hidden, excite, w1, w2, s3):
        """part (C,B,slices,2) from bnact_partial_sums_raw(grad_y) -> (g_w1 (H,C), g_w2 (C,H), g_mean (B,C), sum_beta (C), sum_gamma (C)),
        two launches."""
        c, b, slices, _ = part.shape
        h = w1.shape[0]
        dev = part.device
        g_w1 = torch.empty((h, c), dtype=torch.float32, device=dev)
        g_w2 = torch.empty((c, h), dtype=torch.float32, device=dev)
        g_mean = torch.empty((b, c), dtype=torch.float32, device=dev)
        sum_beta = torch.empty((c,), dtype=torch.float32, device=dev)
        sum_gamma = torch.empty((c,), dtype=torch.float32, device=dev)
        ws = torch.empty((b * (3 * c + h),), dtype=torch.float32, device=dev)
        _run(self.lib.pvcnn_se_excite_bwd, 'se_excite_bwd', part, part, slices, a_sum, ax_sum, gamma, beta, squeezed, hidden, excite, w1, w2,
             b, c, h, 1.0 / float(s3), g_w1, g_w2, g_mean, sum_beta, sum_gamma, ws)
        return g_w1, g_w2, g_mean, sum_beta, sum_gamma

    def bnact_partial_sums_raw(self, x, grad_y, gamma, beta, mean, rstd, slope):
        """-> part (C,B,slices,2): per slice of positions the sums of g' and g' * xhat, g' = grad_y * act'(z) (grad_y None: == 1)."""
        _f32(x, 'x')
        b, c, s3 = x.shape
        gy_bstride = _f32_rows(grad_y, 'grad_y') if grad_y is not None else c * s3
        slices = self.lib.pvcnn_bnact_slices(s3)
        part = torch.empty((c, b, slices, 2), dtype=torch.float32, device=x.device)
        _run(self.lib.pvcnn_bnact_partial_sums, 'bnact_partial_sums', x, x, grad_y, gy_bstride, gamma, beta, mean, rstd, b, c, s3,
             float(slope), part)
        return part

    def bnact_partial_sums(self, x, grad_y, gamma, beta, mean, rstd, slope):
        """-> (P, Q) (B,C) each: sums over the positions of g' and g' * xhat, g' = grad_y * act'(z) (grad_y None: == 1)."""
        sums = self.bnact_partial_sums_raw(x, grad_y, gamma, beta, mean, rstd, slope).sum(dim=2)   # (C, B, 2)
        return sums[..., 0].t().contiguous(), sums[..., 1].t().contiguous()

    def bnact_backward_apply(self, x, grad_y, gamma, beta, mean, rstd, sum_gamma, sum_beta, slope, training, bc_mul=None, bc_add=None,
                             amax_seg=256):
        """grad_x of BatchNorm + activation with the two per-channel sums GIVEN and g' = (grad_y * bc_mul[b][c] + bc_add[b][c]) * act'(z);
        -> (grad_x, its amax buffer with segments of amax_seg positions)."""
        _f32(x, 'x')
        gy_bstride = _f32_rows(grad_y, 'grad_y')
        b, c, s3 = x.shape
        for t, name in ((bc_mul, 'bc_mul'), (bc_add, 'bc_add')):
            if t is not None:
                _f32(t, name)
                _shape(tuple(t.shape) == (b, c), f'{name} (B,C) expected')
        gx = torch.empty_like(x)
        amax = self.amax_buffer(b, s3, amax_seg, x.device)
        _run(self.lib.pvcnn_bnact_bwd_apply, 'bnact_backward_apply', x, x, grad_y, gy_bstride, gamma, beta, mean, rstd, sum_gamma, sum_beta,
             bc_mul, bc_add, b, c, s3, float(slope), int(bool(training)), gx, amax, int(amax_seg))
        return gx, amax

    def bnact_backward(self, x, grad_y, gamma, beta, mean, rstd, slope, training, amax_seg=0, drop=None, out_w=None, out_b=None):
        """-> (grad_x, grad_gamma, grad_beta [, grad_x's amax buffer with segments of amax_seg positions, emitted by the apply pass]).
        drop = (seed, p) of the forward call: grad_y is then the gradient of the DROPPED output (needs amax_seg > 0)."""
        _f32(x, 'x')
        gy_bstride = _f32_rows(grad_y, 'grad_y')
        b, c, s3 = x.shape
        dev = x.device
        gx = torch.empty_like(x)
        gg = self._grad_out(out_w, (c,), dev)
        gb = self._grad_out(out_b, (c,), dev)
        ws = self._scratch(self.lib.pvcnn_bnact_workspace_bytes(b, c, s3), dev)
        amax_seg = int(amax_seg)
        gx_amax = self.amax_buffer(b, s3, amax_seg, dev) if amax_seg > 0 else None
        tickets = self._tickets(c, dev)                   # one word per channel: the reduce pass finalises its own sums
        _run(self.lib.pvcnn_bnact_bwd_strided, 'bnact_backward', x, x, grad_y, gy_bstride, gamma, beta, mean, rstd, b, c, s3, float(slope),
             int(bool(training)), gx, gg, gb, gx_amax, amax_seg, ws, ws.numel(), drop[0] if drop else None,
             float(drop[1]) if drop else 0.0, tickets)
        return (gx, gg, gb, gx_amax) if amax_seg > 0 else (gx, gg, gb)

    # ---- evaluation (csrc/evaluate.hip, ABI v13): evaluate/{s3dis,shapenet}/eval.py and meters/{s3dis,shapenet}.py on the device --------
    def eval_tile(self, src, shuffled, num_points, channels, strides, src_points):
        """-> (B*E, channels, num_points) float32, the model input of the reference's repeat / shuffle / tile.  src: a contiguous float32
        device tensor; strides = (batch, point, channel) element strides into it; src_points: points per batch item (shuffled indices
        must lie in [0, src_points)); shuffled (B, V) int64, V % num_points == 0."""
        _f32(src, 'src'); _dev(shuffled, 'shuffled')
        _shape(shuffled.dtype == torch.int64 and shuffled.dim() == 2 and shuffled.is_contiguous(), 'eval_tile: shuffled (B,V) int64 expected')
        b, v = shuffled.shape
        np_, c, (bs, ps, cs) = int(num_points), int(channels), (int(x) for x in strides)
        _shape(np_ > 0 and v % np_ == 0 and c > 0, 'eval_tile: V must be a multiple of num_points')
        _shape(min(bs, ps, cs) >= 0 and (b == 0 or (b - 1) * bs + (int(src_points) - 1) * ps + (c - 1) * cs < src.numel()),
               'eval_tile: strides reach beyond src')
        out = torch.empty((b * (v // np_), c, np_), dtype=torch.float32, device=src.device)
        _run(self.lib.pvcnn_eval_tile, 'eval_tile', src, src, bs, ps, cs, int(src_points), shuffled, b, v, np_, c, out)
        return out

    def vote_confidence(self, logits, class_range=None):
        """logits (B, C, N) -> (conf (B, N) float32, pred (B, N) int32) = F.softmax(logits, 1)[:, c0:c1].max(1), pred + c0.
        class_range: None (all classes), (c0, c1), or a (B, 2) int32 device tensor of per-cloud ranges."""
        _f32(logits, 'logits')
        _shape(logits.dim() == 3, 'vote_confidence: logits (B,C,N) expected')
        b, c, n = logits.shape
        table = None
        if class_range is None:
            c0, c1 = 0, c
        elif isinstance(class_range, torch.Tensor):
            _i32(class_range, 'class_range')
            _shape(tuple(class_range.shape) == (b, 2), 'vote_confidence: class_range table (B,2) expected')
            table, c0, c1 = class_range, 0, 0
        else:
            c0, c1 = int(class_range[0]), int(class_range[1])
            _shape(0 <= c0 < c1 <= c, 'vote_confidence: class range must satisfy 0 <= c0 < c1 <= C')
        conf = torch.empty((b, n), dtype=torch.float32, device=logits.device)
        pred = torch.empty((b, n), dtype=torch.int32, device=logits.device)
        _run(self.lib.pvcnn_vote_confidence, 'vote_confidence', logits, logits, b, c, n, c0, c1, table, conf, pred)
        return conf, pred

    def vote_merge(self, conf, pred, shuffled, scene_conf, scene_pred, keys, mapping=None):
        """update_scene_predictions in place on (scene_conf (P) float32, scene_pred (P) int64).  keys: the (P) int64 workspace, zero
        before the first call (every call leaves it zero).  mapping: None, or contiguous (rows >= B, M) int64: vote (b, p) targets
        mapping[b, shuffled[b, p]]."""
        _f32(conf, 'conf'); _i32(pred, 'pred'); _f32(scene_conf, 'scene_conf')
        for t, name in ((shuffled, 'shuffled'), (scene_pred, 'scene_pred'), (keys, 'keys')):
            _dev(t, name)
            _shape(t.dtype == torch.int64 and t.is_contiguous(), f'vote_merge: {name} must be a contiguous int64 tensor')
        _shape(conf.dim() == 2 and conf.shape == pred.shape == shuffled.shape, 'vote_merge: conf, pred, shuffled (B,V) expected')
        b, v = conf.shape
        p = scene_conf.numel()
        _shape(scene_pred.numel() == p and keys.numel() == p, 'vote_merge: scene_pred (P) and a (P) key workspace expected')
        map_stride = 0
        if mapping is not None:
            _dev(mapping, 'mapping')
            _shape(mapping.dtype == torch.int64 and mapping.is_contiguous() and mapping.dim() == 2 and mapping.shape[0] >= b,
                   'vote_merge: mapping (>= B, M) contiguous int64 expected')
            map_stride = mapping.shape[1]
        _run(self.lib.pvcnn_vote_merge, 'vote_merge', conf, conf, pred, shuffled, mapping, map_stride, b, v, p, scene_conf, scene_pred,
             keys, keys.numel() * 8)

    def seg_counts(self, gt, pred, num_classes, counts=None, wrap_negative=True):
        """counts (3, C) int64 += [seen; positive; correct] of (gt, pred) (int64, P each); a new zeroed buffer when counts is None."""
        for t, name in ((gt, 'gt'), (pred, 'pred')):
            _dev(t, name)
            _shape(t.dtype == torch.int64 and t.is_contiguous(), f'seg_counts: {name} must be a contiguous int64 tensor')
        _shape(gt.numel() == pred.numel(), 'seg_counts: gt and pred must have the same number of points')
        c = int(num_classes)
        if counts is None:
            counts = torch.zeros((3, c), dtype=torch.int64, device=gt.device)
        _shape(counts.dtype == torch.int64 and counts.is_contiguous() and counts.numel() == 3 * c, 'seg_counts: counts (3,C) int64')
        _run(self.lib.pvcnn_seg_counts, 'seg_counts', gt, gt, pred, gt.numel(), c, int(bool(wrap_negative)), counts)
        return counts

    def seg_meter_update(self, logits, targets, counts=None, part_ranges=None, max_parts=0, rows=None, row_cursor=None):
        """S3DIS mode (part_ranges None): counts (3C + 2) int64 += this batch.  ShapeNet mode: rows (capacity, max_parts + 1, 2) int32,
        cloud b written at row *row_cursor + b (see include/pvcnn_hip.h)."""
        _f32(logits, 'logits'); _dev(targets, 'targets')
        _shape(logits.dim() == 3 and targets.dtype == torch.int64 and targets.is_contiguous()
               and tuple(targets.shape) == (logits.shape[0], logits.shape[2]), 'seg_meter_update: logits (B,C,N), targets (B,N) int64')
        b, c, n = logits.shape
        if part_ranges is None:
            _shape(counts is not None and counts.dtype == torch.int64 and counts.is_contiguous() and counts.numel() == 3 * c + 2,
                   'seg_meter_update: counts (3C+2) int64 expected')
            tail = (None, 0, 0, counts, None, None, 0)
        else:
            _i32(part_ranges, 'part_ranges')
            _shape(part_ranges.dim() == 2 and part_ranges.shape[1] == 2, 'seg_meter_update: part_ranges (K,2) int32 expected')
            _i32(rows, 'rows')
            _shape(rows.dim() == 3 and rows.shape[1:] == (int(max_parts) + 1, 2), 'seg_meter_update: rows (capacity, max_parts+1, 2)')
            if row_cursor is not None:
                _dev(row_cursor, 'row_cursor')
                _shape(row_cursor.dtype == torch.int64 and row_cursor.numel() == 1, 'seg_meter_update: row_cursor: one int64')
            tail = (part_ranges, part_ranges.shape[0], int(max_parts), None, rows, row_cursor, rows.shape[0])
        _run(self.lib.pvcnn_seg_meter_update, 'seg_meter_update', logits, logits, targets, b, c, n, *tail)

    # ---- oriented boxes (csrc/boxes.hip, ABI v14): meters/kitti and the KITTI AP overlaps on the device ------------------------------
    @staticmethod
    def _box_heads(center, heading_scores, heading_residuals, size_scores, size_residuals):
        for t, name in ((center, 'center'), (heading_scores, 'heading_scores'), (heading_residuals, 'heading_residuals'),
                        (size_scores, 'size_scores'), (size_residuals, 'size_residuals')):
            _f32(t, name)
        b, nh = heading_scores.shape
        ns = size_scores.shape[1]
        _shape(tuple(center.shape) == (b, 3) and tuple(heading_residuals.shape) == (b, nh) and tuple(size_scores.shape) == (b, ns)
               and tuple(size_residuals.shape) == (b, ns, 3), 'box heads: center (B,3), heading (B,NH) x2, size (B,NS), (B,NS,3)')
        return b, nh, ns

    @staticmethod
    def _box_tables(bin_centers, size_templates, nh, ns):
        _f32(bin_centers, 'heading_angle_bin_centers'); _f32(size_templates, 'size_templates')
        _shape(bin_centers.numel() == nh and size_templates.numel() == 3 * ns,
               'box tables: NH heading bin centers and (NS, 3) size templates expected')

    def frustum_meter_update(self, outputs, targets, bin_centers, size_templates, class_ids, thresholds, sums, counts):
        """MeterFrustumKitti.update of the box metrics: sums (2) float64 += [iou_2d, iou_3d], counts (3 + 2K) int64 += [boxes, -,
        iou_3d >= 0.7, correct K | seen K].  outputs / targets: (center, heading_scores, heading_residuals, size_scores, size_residuals)
        float32 and (center, heading_bin_id int64, heading_residual, size_template_id int64, size_residual, class_id int64)."""
        b, nh, ns = self._box_heads(*outputs)
        self._box_tables(bin_centers, size_templates, nh, ns)
        center_t, hid_t, hres_t, sid_t, sres_t, cls_t = targets
        for t, name in ((center_t, 'center'), (hres_t, 'heading_residual'), (sres_t, 'size_residual')):
            _f32(t, name)
        for t, name in ((hid_t, 'heading_bin_id'), (sid_t, 'size_template_id'), (cls_t, 'class_id'), (class_ids, 'class_ids'),
                        (counts, 'counts')):
            _dev(t, name)
            _shape(t.dtype == torch.int64 and t.is_contiguous(), f'frustum_meter_update: {name} must be a contiguous int64 tensor')
        _dev(thresholds, 'thresholds'); _dev(sums, 'sums')
        k = class_ids.numel()
        _shape(tuple(center_t.shape) == (b, 3) and hid_t.numel() == b and hres_t.numel() == b and sid_t.numel() == b
               and tuple(sres_t.shape) == (b, 3) and cls_t.numel() == b, 'frustum_meter_update: targets of B boxes expected')
        _shape(thresholds.dtype == torch.float64 and thresholds.numel() == k and sums.dtype == torch.float64 and sums.numel() == 2
               and counts.numel() == 3 + 2 * k, 'frustum_meter_update: thresholds (K) / sums (2) float64, counts (3 + 2K) int64')
        _run(self.lib.pvcnn_frustum_meter_update, 'frustum_meter_update', outputs[0], *outputs, *targets, b, nh, ns, bin_centers,
             size_templates, class_ids, thresholds, k, None, None, 0, 0, sums, counts)

    def frustum_meter_accuracy(self, mask_logits, mask_targets, counts):
        """MeterFrustumKitti.update, metric 'accuracy': counts[0] += B*N, counts[1] += #(argmax(mask_logits, 1) == target)."""
        _f32(mask_logits, 'mask_logits'); _dev(mask_targets, 'mask_targets'); _dev(counts, 'counts')
        _shape(mask_logits.dim() == 3 and mask_targets.dtype == torch.int64 and mask_targets.is_contiguous()
               and tuple(mask_targets.shape) == (mask_logits.shape[0], mask_logits.shape[2]),
               'frustum_meter_accuracy: mask_logits (B,C,N) float32, targets (B,N) int64')
        _shape(counts.dtype == torch.int64 and counts.is_contiguous() and counts.numel() >= 2, 'frustum_meter_accuracy: counts int64')
        b, c, n = mask_logits.shape
        _run(self.lib.pvcnn_frustum_meter_update, 'frustum_meter_accuracy', mask_logits, *([None] * 11), b, 0, 0, None, None, None, None, 0,
             mask_logits, mask_targets, c, n, None, counts)

    def box_iou_3d(self, corners_1, corners_t):
        """(B, 3, 8) float32 corner sets -> (iou_3d, iou_2d), (B) float64 each (get_box_iou_3d per pair)."""
        _f32(corners_1, 'corners_1'); _f32(corners_t, 'corners_t')
        _shape(corners_1.dim() == 3 and tuple(corners_1.shape[1:]) == (3, 8) and corners_1.shape == corners_t.shape,
               'box_iou_3d: two (B,3,8) corner tensors expected')
        b = corners_1.shape[0]
        iou_3d = torch.empty((b,), dtype=torch.float64, device=corners_1.device)
        iou_2d = torch.empty_like(iou_3d)
        _run(self.lib.pvcnn_box_iou_3d, 'box_iou_3d', corners_1, corners_1, corners_t, b, iou_3d, iou_2d)
        return iou_3d, iou_2d

    def rotate_iou(self, boxes, query_boxes, criterion=-1, boxes_3d=None, query_boxes_3d=None, z_axis=1, z_center=1.0):
        """(N, K) float32 overlaps of rboxes (N, 5) and (K, 5) float32 (x, y, dx, dy, angle).  With boxes_3d / query_boxes_3d
        ((N, 7) / (K, 7) float64, whose BEV columns the rboxes are): d3_box_overlap instead of the BEV overlap."""
        _f32(boxes, 'boxes'); _f32(query_boxes, 'query_boxes')
        _shape(boxes.dim() == 2 and boxes.shape[1] == 5 and query_boxes.dim() == 2 and query_boxes.shape[1] == 5,
               'rotate_iou: boxes (N,5) and query_boxes (K,5) expected')
        n, k = boxes.shape[0], query_boxes.shape[0]
        out = torch.zeros((n, k), dtype=torch.float32, device=boxes.device)
        if boxes_3d is None:
            _run(self.lib.pvcnn_rotate_iou, 'rotate_iou', boxes, boxes, n, query_boxes, k, int(criterion), out)
            return out
        for t, name, rows in ((boxes_3d, 'boxes_3d', n), (query_boxes_3d, 'query_boxes_3d', k)):
            _dev(t, name)
            _shape(t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == (rows, 7),
                   f'box3d_overlap: {name} ({rows},7) contiguous float64 expected')
        _run(self.lib.pvcnn_box3d_overlap, 'box3d_overlap', boxes, boxes, boxes_3d, n, query_boxes, query_boxes_3d, k, int(criterion),
             int(z_axis), float(z_center), out)
        return out

    def frustum_predictions(self, heads, bin_centers, size_templates, rotation_angle, rgb_score, table, step):
        """Rows step .. step+B-1 of table (rows, 8) float64 = update_predictions of the decoded boxes.  heads: (center,
        heading_scores, heading_residuals, size_scores, size_residuals) float32; rotation_angle, rgb_score (B) float64."""
        b, nh, ns = self._box_heads(*heads)
        self._box_tables(bin_centers, size_templates, nh, ns)
        for t, name in ((rotation_angle, 'rotation_angle'), (rgb_score, 'rgb_score'), (table, 'predictions')):
            _dev(t, name)
            _shape(t.dtype == torch.float64 and t.is_contiguous(), f'frustum_predictions: {name} must be a contiguous float64 tensor')
        _shape(rotation_angle.numel() == b and rgb_score.numel() == b and table.dim() == 2 and table.shape[1] == 8,
               'frustum_predictions: rotation_angle, rgb_score (B), table (rows, 8) expected')
        _shape(0 <= int(step) and int(step) + b <= table.shape[0], 'frustum_predictions: the batch does not fit in the table')
        _run(self.lib.pvcnn_frustum_predictions, 'frustum_predictions', heads[0], *heads, b, nh, ns, bin_centers, size_templates,
             rotation_angle, rgb_score, table, table.shape[0], int(step))

    # ---- the KITTI AP evaluation (csrc/kitti_ap.hip; include/pvcnn_hip.h "the KITTI AP evaluation") ----
    @staticmethod
    def _ap_typed(t, name, dtype, numel=None):
        _dev(t, name)
        _shape(t.dtype == dtype and t.is_contiguous() and (numel is None or t.numel() == numel),
               f'kitti_ap: {name} must be a contiguous {dtype} tensor' + ('' if numel is None else f' of {numel} elements'))

    def image_box_overlap(self, boxes, query_boxes, criterion=-1):
        """(N, K) float64 overlaps of (N, 4) and (K, 4) float64 boxes: the reference's image_box_overlap, bit for bit."""
        n, k = boxes.shape[0], query_boxes.shape[0]
        self._ap_typed(boxes, 'boxes', torch.float64, 4 * n); self._ap_typed(query_boxes, 'query_boxes', torch.float64, 4 * k)
        out = torch.zeros((n, k), dtype=torch.float64, device=boxes.device)
        _run(self.lib.pvcnn_image_box_overlap, 'image_box_overlap', boxes, boxes, n, query_boxes, k, int(criterion), out)
        return out

    def kitti_ap_overlaps(self, p, metric, z_axis=1, z_center=1.0):
        """The per-image overlaps[det, gt] blocks of a packed evaluation `p` (kitti._Packed), flat at p.pair_off: float64 for metric 0
        (2-D boxes), float32 for 1 (BEV) and 2 (3-D)."""
        dev = p.gt_off.device
        if metric == 0:
            out = torch.zeros((p.pairs,), dtype=torch.float64, device=dev)
            _run(self.lib.pvcnn_kitti_ap_bbox_overlaps, 'kitti_ap_bbox_overlaps', p.gt_off, p.dt_bbox, p.gt_bbox, p.dt_off, p.gt_off,
                 p.pair_off, p.images, p.pairs, out)
            return out
        _shape(metric in (1, 2), 'unknown metric')
        bev_dt, bev_gt, full_dt, full_gt = p.boxes_3d(z_axis)
        out = torch.zeros((p.pairs,), dtype=torch.float32, device=dev)
        full = (None, None) if metric == 1 else (full_dt, full_gt)
        _run(self.lib.pvcnn_kitti_ap_box_overlaps, 'kitti_ap_box_overlaps', p.gt_off, bev_dt, full[0], bev_gt, full[1], p.dt_off, p.gt_off,
             p.pair_off, p.images, p.pairs, -1, int(z_axis), float(z_center), out)
        return out

    def kitti_ap_clean(self, p, classes, difficulties):
        """clean_data for every (class, difficulty): (ignored_gt (M, L, G) int8, ignored_det (M, L, D) int8, dc_index int32,
        num_valid_gt (M, L) int64).  classes / difficulties: int32 device tensors."""
        dev = p.gt_off.device
        m, l = classes.numel(), difficulties.numel()
        self._ap_typed(classes, 'classes', torch.int32); self._ap_typed(difficulties, 'difficulties', torch.int32)
        ignored_gt = torch.zeros((m, l, p.G), dtype=torch.int8, device=dev)
        ignored_det = torch.zeros((m, l, p.D), dtype=torch.int8, device=dev)
        dc_index = torch.zeros((p.dontcares,), dtype=torch.int32, device=dev)
        dc_out = self._ap_some(dc_index)
        num_valid_gt = torch.zeros((m, l), dtype=torch.int64, device=dev)
        _run(self.lib.pvcnn_kitti_ap_clean, 'kitti_ap_clean', p.gt_off, p.gt_name, p.gt_bbox, p.gt_occluded, p.gt_truncated, p.G, p.dt_name,
             p.dt_bbox, p.D, p.gt_off, p.dc_off, p.images, classes, m, difficulties, l, ignored_gt, ignored_det, dc_out, num_valid_gt)
        return ignored_gt, ignored_det, dc_index, num_valid_gt

    @staticmethod
    def _ap_some(t):
        """t, or one zero where t is empty: the library refuses a null pointer wherever the sizes alone do not rule a read out."""
        return t if t.numel() > 0 else torch.zeros((1,), dtype=t.dtype, device=t.device)

    def _ap_args(self, p, overlaps, clean, min_overlaps):
        ignored_gt, ignored_det, dc_index, _ = clean
        m, l = ignored_gt.shape[:2]
        k = min_overlaps.shape[0]
        self._ap_typed(overlaps, 'overlaps', torch.float64, p.pairs)
        self._ap_typed(min_overlaps, 'min_overlaps', torch.float64, k * m)
        self._ap_typed(ignored_gt, 'ignored_gt', torch.int8, m * l * p.G); self._ap_typed(ignored_det, 'ignored_det', torch.int8, m * l * p.D)
        self._ap_typed(dc_index, 'dc_index', torch.int32, p.dontcares)
        overlaps, dc_index = self._ap_some(overlaps), self._ap_some(dc_index)
        return (overlaps, p.gt_off, p.dt_off, p.dc_off, p.pair_off, p.images, p.G, p.D, p.max_gt, p.max_dt, ignored_gt, ignored_det,
                p.dt_score, p.dt_alpha, p.gt_alpha, p.dt_bbox, p.gt_bbox, dc_index, min_overlaps, m, l, k), (m, l, k)

    def kitti_ap_match(self, p, overlaps, clean, min_overlaps):
        """Matching pass 1 for every (image, class, difficulty, min_overlap row): tp_scores (M, L, K, G) float64, a true positive's
        score in the slot of its ground truth and -inf elsewhere.  overlaps: float64, flat at p.pair_off; min_overlaps (K, M)."""
        args, cells = self._ap_args(p, overlaps, clean, min_overlaps)
        tp_scores = torch.full(cells + (p.G,), float('-inf'), dtype=torch.float64, device=overlaps.device)
        _run(self.lib.pvcnn_kitti_ap_match, 'kitti_ap_match', p.gt_off, *args, tp_scores)
        return tp_scores

    def kitti_ap_thresholds(self, tp_scores, num_valid_gt):
        """get_thresholds per cell: (thresholds (M, L, K, 41) float64, counts (M, L, K) int32), left on the device."""
        m, l, k, g = tp_scores.shape
        self._ap_typed(tp_scores, 'tp_scores', torch.float64); self._ap_typed(num_valid_gt, 'num_valid_gt', torch.int64, m * l)
        ordered = torch.sort(tp_scores, dim=-1, descending=True).values.contiguous()
        thresholds = torch.zeros((m, l, k, 41), dtype=torch.float64, device=tp_scores.device)
        counts = torch.zeros((m, l, k), dtype=torch.int32, device=tp_scores.device)
        _run(self.lib.pvcnn_kitti_ap_thresholds, 'kitti_ap_thresholds', tp_scores, ordered, g, num_valid_gt, m * l * k, k, thresholds, counts)
        return thresholds, counts

    def kitti_ap_stats(self, p, overlaps, clean, min_overlaps, thresholds, counts, metric, compute_aos):
        """Matching pass 2 at every threshold slot, summed over the images: pr (M, L, K, 41, 4) float64 = [tp, fp, fn, similarity]."""
        args, cells = self._ap_args(p, overlaps, clean, min_overlaps)
        n = cells[0] * cells[1] * cells[2]
        self._ap_typed(thresholds, 'thresholds', torch.float64, n * 41); self._ap_typed(counts, 'counts', torch.int32, n)
        pr = torch.zeros(cells + (41, 4), dtype=torch.float64, device=overlaps.device)
        nbytes = self.lib.pvcnn_kitti_ap_workspace_bytes(p.images, n)
        workspace = torch.empty((max(nbytes, 8) // 8,), dtype=torch.float64, device=overlaps.device)
        _run(self.lib.pvcnn_kitti_ap_stats, 'kitti_ap_stats', p.gt_off, *args, thresholds, counts, int(metric), int(bool(compute_aos)), pr,
             workspace, nbytes)
        return pr

    # ---- shapes on the device (csrc/shapes.hip; include/pvcnn_hip.h "Shapes on the device"; pvcnn_amd/shapes.py owns the policy) ----
    has_shapes = True
    K_NEAREST_MAX_K = 64

    @staticmethod
    def _packed(rows, offsets, who):
        """rows (R, ld >= 3) fp32 with unit column stride (a column slice of a wider store is fine), offsets (W + 1,) int64
        -> (R, ld, W)."""
        _dev(rows, 'rows'); _dev(offsets, 'offsets')
        _arg(rows.dim() == 2 and rows.dtype == torch.float32 and rows.shape[1] >= 3 and (rows.shape[0] <= 1 or rows.stride(0) >= rows.shape[1])
               and rows.stride(1) == 1, f'{who}: rows (R, >= 3) float32 with contiguous columns expected')
        _arg(offsets.dim() == 1 and offsets.dtype == torch.int64 and offsets.numel() >= 1 and offsets.is_contiguous()
               and offsets.device == rows.device, f'{who}: offsets (W + 1,) int64 on the rows\' device expected')
        return rows.shape[0], (rows.stride(0) if rows.shape[0] > 1 else rows.shape[1]), offsets.numel() - 1

    @staticmethod
    def _shapes_out(out, shape, dtype, device, who):
        if out is None:
            return torch.empty(shape, dtype=dtype, device=device)
        _arg(tuple(out.shape) == tuple(shape) and out.dtype == dtype and out.device == device and out.is_contiguous(),
               f'{who}: out= must be a contiguous {dtype} tensor of shape {tuple(shape)} on {device}')
        return out

    def k_nearest(self, rows, offsets, k, out=None):
        """-> (R, k) int32: per row the min(k, n_w) nearest rows of its own cloud, ascending in (distance, position), as positions inside
        the cloud; -1 beyond n_w.  One launch, nothing read back: capturable (give `out=` for a static buffer)."""
        r, ld, w = self._packed(rows, offsets, 'k_nearest')
        k = int(k)
        _arg(1 <= k <= self.K_NEAREST_MAX_K, f'k_nearest: k in [1, {self.K_NEAREST_MAX_K}] expected')
        out = self._shapes_out(out, (r, k), torch.int32, rows.device, 'k_nearest')
        _run(self.lib.pvcnn_k_nearest, 'k_nearest', rows, rows, r, ld, offsets, w, k, out)
        return out

    def shape_normals(self, rows, offsets, knn, ref=None, mode=0, want_curvature=False, out=None, out_curvature=None):
        """-> (normals (R, 3) fp32, curvature (R,) fp32 or None) from the neighbour table knn (R, k) int32; ref (W, 3) fp32 and
        mode 1 (outward from ref) / 2 (towards ref), or mode 0: sign as the solver leaves it.  One launch."""
        r, ld, w = self._packed(rows, offsets, 'shape_normals')
        _i32(knn, 'knn')
        _arg(knn.dim() == 2 and knn.shape[0] == r and 1 <= knn.shape[1] <= self.K_NEAREST_MAX_K and knn.device == rows.device,
               'shape_normals: knn (R, k) int32 with k in [1, 64] expected')
        mode = int(mode)
        _arg(mode in (0, 1, 2), 'shape_normals: mode 0, 1 or 2 expected')
        if mode:
            _arg(ref is not None, 'shape_normals: an oriented mode needs ref (W, 3)')
            _f32(ref, 'ref')
            _arg(tuple(ref.shape) == (w, 3) and ref.device == rows.device, 'shape_normals: ref (W, 3) float32 expected')
        normals = self._shapes_out(out, (r, 3), torch.float32, rows.device, 'shape_normals')
        curvature = None
        if want_curvature or out_curvature is not None:
            curvature = self._shapes_out(out_curvature, (r,), torch.float32, rows.device, 'shape_normals')
        _run(self.lib.pvcnn_shape_normals, 'shape_normals', rows, rows, r, ld, offsets, w, knn, knn.shape[1], ref if mode else None, mode,
             normals, curvature)
        return normals, curvature

    def cloud_centroids(self, rows, offsets, out=None):
        """-> (W, 3) fp32: the fp64 mean of every cloud's xyz, rounded once.  One launch."""
        r, ld, w = self._packed(rows, offsets, 'cloud_centroids')
        out = self._shapes_out(out, (w, 3), torch.float32, rows.device, 'cloud_centroids')
        _run(self.lib.pvcnn_cloud_centroids, 'cloud_centroids', rows, rows, r, ld, offsets, w, out)
        return out

    # ---- sparse voxels (csrc/sparse.hip; include/pvcnn_hip.h "Sparse voxels"; functional/sparse.py owns the autograd nodes) ----
    has_sparse = True
    SPARSE_ROW_TILE = 64
    SPARSE_MAX_R = 128

    def sparse_supported(self, b, r):
        """True when a (b, r^3) grid has a map: r <= 128 and b r^3 < 2^31 (the size query's answer)."""
        return self.lib.pvcnn_sparse_map_workspace_bytes(int(b), int(r)) > 0

    def sparse_skip(self, on=None):
        """The debug switch of the tap skip (on by default): set it (True / False) or only ask (None); -> the previous state."""
        return bool(self.lib.pvcnn_sparse_debug_skip(-1 if on is None else int(bool(on))))

    def sparse_map(self, cnt, resolution, cap, out=None):
        """cnt (B, R^3) int32 -> (voxel (cap,), index (B R^3,), offsets (B + 1,), nbr (cap, 27), overflow (1,)), all int32; four
        launches, nothing read back.  `out=`: the five tensors, preallocated (static buffers of a captured step)."""
        _i32(cnt, 'cnt')
        r, cap = int(resolution), int(cap)
        _arg(cnt.dim() == 2 and cnt.shape[1] == r ** 3, 'sparse_map: cnt (B, R^3) int32 expected')
        b = cnt.shape[0]
        nbytes = self.lib.pvcnn_sparse_map_workspace_bytes(b, r)
        _arg(nbytes > 0 and self.lib.pvcnn_sparse_map_bytes(b, r, cap) > 0,
             'sparse_map: R <= 128, B R^3 < 2^31 and 1 <= cap < 2^31 / 27 expected')
        dev = cnt.device
        shapes = ((cap,), (b * r ** 3,), (b + 1,), (cap, 27), (1,))
        if out is None:
            out = tuple(torch.empty(s, dtype=torch.int32, device=dev) for s in shapes)
        else:
            _arg(len(out) == 5, 'sparse_map: out= (voxel, index, offsets, nbr, overflow) expected')
            out = tuple(self._shapes_out(o, s, torch.int32, dev, 'sparse_map') for o, s in zip(out, shapes))
        workspace = self._scratch(nbytes, dev)
        _run(self.lib.pvcnn_sparse_map, 'sparse_map', cnt, cnt, b, r, cap, *out, workspace, workspace.numel())
        return out

    @staticmethod
    def _sparse_count(count, ref, who):
        _i32(count, 'count')
        _arg(count.numel() == 1 and count.device == ref.device, f'{who}: count = one int32 word on the device expected')

    def sparse_gather(self, grid, voxel, count, out=None):
        """grid (B, C, R^3) fp32 -> rows (cap, C) fp32, zeros at the rows >= count.  One launch."""
        _f32(grid, 'grid'); _i32(voxel, 'voxel'); self._sparse_count(count, grid, 'sparse_gather')
        _arg(grid.dim() == 3 and voxel.dim() == 1 and voxel.device == grid.device, 'sparse_gather: grid (B, C, R^3), voxel (cap,) expected')
        b, c, r3 = grid.shape
        r = round(r3 ** (1.0 / 3.0))
        _arg(r ** 3 == r3, 'sparse_gather: a cubic grid expected')
        cap = voxel.shape[0]
        rows = self._shapes_out(out, (cap, c), torch.float32, grid.device, 'sparse_gather')
        _run(self.lib.pvcnn_sparse_gather, 'sparse_gather', grid, grid, voxel, count, b, c, r, cap, rows)
        return rows

    def sparse_scatter(self, rows, index, count, batch, resolution, out=None):
        """rows (cap, C) fp32 -> grid (B, C, R^3) fp32, zero at every voxel without a row; every word is written.  One launch."""
        _f32(rows, 'rows'); _i32(index, 'index'); self._sparse_count(count, rows, 'sparse_scatter')
        b, r = int(batch), int(resolution)
        _arg(rows.dim() == 2 and index.dim() == 1 and index.shape[0] == b * r ** 3 and index.device == rows.device,
             'sparse_scatter: rows (cap, C), index (B R^3,) expected')
        cap, c = rows.shape
        grid = self._shapes_out(out, (b, c, r ** 3), torch.float32, rows.device, 'sparse_scatter')
        _run(self.lib.pvcnn_sparse_scatter, 'sparse_scatter', rows, rows, index, count, b, c, r, cap, grid)
        return grid

    def sparse_conv3d_weight_image(self, weight, for_bwd_data=False):
        """weight (Co, Ci, 3, 3, 3) -> the image the convolution kernel reads: (27, Ci, Co), or for backward-data (27, Co, Ci) with
        the taps reversed.  One launch."""
        _f32(weight, 'weight')
        _arg(weight.dim() == 5 and tuple(weight.shape[2:]) == (3, 3, 3), 'sparse_conv3d: weight (Co, Ci, 3, 3, 3) expected')
        co, ci = weight.shape[:2]
        wt = torch.empty((27, co, ci) if for_bwd_data else (27, ci, co), dtype=torch.float32, device=weight.device)
        _run(self.lib.pvcnn_sparse_conv3d_weight_transform, 'sparse_conv3d_weight_transform', weight, weight, co, ci, int(bool(for_bwd_data)), wt)
        return wt

    def sparse_conv3d_forward(self, rows, wt, bias, nbr, count, out=None):
        """rows (cap, Ci), wt (27, Ci, Co) (sparse_conv3d_weight_image), bias (Co,) or None -> (cap, Co); zeros at the rows >= count.
        Backward-data is the same call on grad_y and the backward image, without a bias.  One launch."""
        _f32(rows, 'rows'); _f32(wt, 'wt'); _i32(nbr, 'nbr'); self._sparse_count(count, rows, 'sparse_conv3d')
        _arg(rows.dim() == 2 and wt.dim() == 3 and wt.shape[0] == 27 and wt.shape[1] == rows.shape[1] and wt.device == rows.device,
             'sparse_conv3d: rows (cap, Ci) and a weight image (27, Ci, Co) expected')
        cap, ci = rows.shape
        co = wt.shape[2]
        _arg(tuple(nbr.shape) == (cap, 27) and nbr.device == rows.device, 'sparse_conv3d: nbr (cap, 27) int32 expected')
        if bias is not None:
            _f32(bias, 'bias')
            _arg(tuple(bias.shape) == (co,) and bias.device == rows.device, 'sparse_conv3d: bias (Co,) expected')
        y = self._shapes_out(out, (cap, co), torch.float32, rows.device, 'sparse_conv3d')
        _run(self.lib.pvcnn_sparse_conv3d_fwd, 'sparse_conv3d_fwd', rows, rows, wt, bias, nbr, count, cap, ci, co, y)
        return y

    def sparse_conv3d_backward_weight(self, rows, grad_y, nbr, count, want_weight=True, want_bias=True, out=None, out_bias=None):
        """-> (grad_w (Co, Ci, 3, 3, 3) or None, grad_bias (Co,) or None): partial sums per chunk of rows, added in a fixed order by a
        second launch (no float atomics)."""
        _f32(rows, 'rows'); _f32(grad_y, 'grad_y'); _i32(nbr, 'nbr'); self._sparse_count(count, rows, 'sparse_conv3d_bwd_weight')
        _arg(rows.dim() == 2 and grad_y.dim() == 2 and grad_y.shape[0] == rows.shape[0] and grad_y.device == rows.device,
             'sparse_conv3d_bwd_weight: rows (cap, Ci), grad_y (cap, Co) expected')
        cap, ci = rows.shape
        co = grad_y.shape[1]
        _arg(tuple(nbr.shape) == (cap, 27) and nbr.device == rows.device, 'sparse_conv3d_bwd_weight: nbr (cap, 27) int32 expected')
        gw = self._shapes_out(out, (co, ci, 3, 3, 3), torch.float32, rows.device, 'sparse_conv3d_bwd_weight') if want_weight else None
        gb = self._shapes_out(out_bias, (co,), torch.float32, rows.device, 'sparse_conv3d_bwd_weight') if want_bias else None
        if gw is None and gb is None:
            return None, None
        nbytes = self.lib.pvcnn_sparse_conv3d_bwd_weight_workspace_bytes(cap, ci, co)
        _arg(nbytes > 0, 'sparse_conv3d_bwd_weight: sizes out of range')
        workspace = self._scratch(nbytes, rows.device)
        _run(self.lib.pvcnn_sparse_conv3d_bwd_weight, 'sparse_conv3d_bwd_weight', rows, rows, grad_y, nbr, count, cap, ci, co, gw, gb,
             workspace, workspace.numel())
        return gw, gb


class _WeightBank:
    """Persistent f16x2 image pairs of registered weights (HipBackend.weight_bank_*).  An entry is keyed by (kind, data pointer,
    (Co, Ci)); `wanted` = the keys a forward pass asked for (take() misses note them), so a refresh computes what is used and nothing
    else; the device tables are rebuilt when that set changes (the warm-up steps), not in steady state."""

    _PRODUCTS = {CONV.kind: CONV, PW.kind: PW}
    # lib.pvcnn_<conv3d|pwconv>_weight_split_pair_<entry|batch><suffix>: the f16x2 pairs (nsplit 2), the plain-bf16 pairs of autocast (1)
    _PAIR_SUFFIX = {2: '', 1: '_bf16'}

    def __init__(self, be):
        import weakref
        self.be, self._weakref = be, weakref
        self.params = []            # weakrefs of registered parameters
        self.seen = set()           # id()s of registered parameters
        self.wanted = set()
        self.entries = {}           # key -> dict(param=weakref, wf, wb, armed, version)
        self.tables = {}            # kind -> (device table, n, total rows, keys)
        self.dirty = True
        self.epoch = 0              # bumped by weight_bank_invalidate(): pairs armed in an earlier epoch are never served
        self.pinned = []            # buffers a stream capture saw (a replayed graph reads and writes them by raw pointer): never freed

    @staticmethod
    def _kind_of(p):
        if p.dim() == 5 and tuple(p.shape[2:]) == (3, 3, 3):
            return 'conv'
        if p.dim() in (3, 4) and all(k == 1 for k in p.shape[2:]):
            return 'pw'
        return None

    def register(self, model):
        import torch.nn as nn
        for m in model.modules():
            if isinstance(m, (nn.Conv1d, nn.Conv2d, nn.Conv3d)) and m.weight is not None and self._kind_of(m.weight) and id(m.weight) not in self.seen:
                self.seen.add(id(m.weight))
                self.params.append(self._weakref.ref(m.weight))
                self.dirty = True

    def take(self, kind, w, nsplit=2):
        key = (kind, w.data_ptr(), (int(w.shape[0]), int(w.shape[1])), int(nsplit))
        e = self.entries.get(key)
        if e is not None and e['armed']:
            e['armed'] = False
            p = e['param']()
            if p is not None and p._version == e['version'] and p.data_ptr() == key[1] and e['epoch'] == self.epoch:
                if e['wf'].is_cuda and torch.cuda.is_current_stream_capturing():
                    self._pin(e)
                return e['wf'], e['wb']
        if key not in self.wanted:
            if len(self.wanted) >= 4096:                # (keys of temporaries -- a weight that is copied to be made contiguous has a new
                self.wanted.clear()                     # address per call -- must not pile up; registered weights are re-noted at once)
            self.wanted.add(key)
            self.dirty = True
        return None

    def _pin(self, e):
        if not e.get('pinned'):
            e['pinned'] = True
            self.pinned.append((e['wf'], e['wb']))

    def _rebuild(self):
        lib = self.be.lib
        # (kind, nsplit): nsplit 2 = the f16x2 pairs, 1 = the plain-bf16 pairs of the autocast mode
        live, by_kind = {}, {(kind, nsplit): [] for nsplit in self._PAIR_SUFFIX for kind in self._PRODUCTS}
        for ref in self.params:
            p = ref()
            if p is None or not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                continue
            kind = self._kind_of(p)
            for nsplit in (2, 1):
                key = (kind, p.data_ptr(), (int(p.shape[0]), int(p.shape[1])), nsplit)
                if key not in self.wanted:
                    continue
                e = self.entries.get(key)
                if e is None or e['param']() is not p:
                    co, ci = key[2]
                    nbytes = self._PRODUCTS[kind].entry(lib, 'weight_split_bytes')
                    e = {'param': ref, 'armed': False, 'version': -1, 'epoch': -1,
                         'wf': torch.empty((nbytes(co, ci, 0, nsplit),), dtype=torch.uint8, device=p.device),
                         'wb': torch.empty((nbytes(co, ci, 1, nsplit),), dtype=torch.uint8, device=p.device)}
                live[key] = e
                by_kind[(kind, nsplit)].append((key, p, e))
        self.entries, self.tables = live, {}
        for (kind, nsplit), items in by_kind.items():
            if not items:
                continue
            fill = self._PRODUCTS[kind].entry(lib, 'weight_split_pair_entry' + self._PAIR_SUFFIX[nsplit])
            host = torch.zeros((len(items), 10), dtype=torch.int64)
            rows = 0
            for i, (key, p, e) in enumerate(items):
                n = fill(_p(p), key[2][0], key[2][1], _p(e['wf']), _p(e['wb']), ctypes.c_void_p(host[i].data_ptr()))
                if n < 0:
                    raise RuntimeError('weight bank: bad entry')
                host[i, 9] = rows
                rows += n
            dev = items[0][1].device
            self.tables[(kind, nsplit)] = (host.to(dev), len(items), rows, [k for k, _, _ in items], dev)
        self.dirty = False

    def refresh(self):
        if self.dirty:
            if torch.cuda.is_current_stream_capturing():        # no allocation / host-to-device copy inside a capture: this step's layers
                for e in self.entries.values():                 # split their own weights (take() finds nothing armed)
                    e['armed'] = False
                return
            self._rebuild()
        capturing = torch.cuda.is_current_stream_capturing()
        lib = self.be.lib
        for (kind, nsplit), (table, n, rows, keys, dev) in self.tables.items():
            launch = self._PRODUCTS[kind].entry(lib, 'weight_split_pair_batch' + self._PAIR_SUFFIX[nsplit])
            _run(launch, 'weight_split_pair_batch', table, table, n, rows)
            if capturing:                               # the captured launch walks this table and writes every entry's buffers on replay
                self.pinned.append(table)
            for key in keys:
                e = self.entries[key]
                if capturing:
                    self._pin(e)
                p = e['param']()
                if p is not None and p.data_ptr() == key[1]:
                    e['armed'], e['version'], e['epoch'] = True, p._version, self.epoch
                else:                                   # the parameter moved or died: rebuild before the next refresh
                    e['armed'] = False
                    self.dirty = True


_backend = HipBackend()
