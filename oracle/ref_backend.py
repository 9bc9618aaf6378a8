"""The reference's own kernels on the CPU (oracle/_ref, built by build_ref.py) behind the same
12-function `_backend` shape.  TEST INFRASTRUCTURE: used to pin oracle/pvcnn_oracle.c
(tests/test_oracle_vs_ref.py) and optionally as the "reference" CPU baseline.

Host-side allocation mirrors the reference's *.cpp files (torch::zeros / torch::full(1e38))."""
import ctypes
import hashlib
import io
import lzma
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path(variant='fma'):
    return os.path.join(_HERE, '_ref', 'libpvcnn_ref_cpu.so' if variant == 'fma' else f'libpvcnn_ref_cpu_{variant}.so')


def available(variant='fma'):
    return os.path.exists(lib_path(variant))


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


class RefCpuBackend:
    name = 'reference-kernels-on-cpu'

    def __init__(self, variant='fma'):
        self.lib = ctypes.CDLL(lib_path(variant))
        self.lib.ref_ball_query.argtypes = [ctypes.c_int] * 3 + [ctypes.c_float, ctypes.c_int] + [ctypes.c_void_p] * 3
        for name, nint in [('ref_avg_voxelize', 4), ('ref_avg_voxelize_grad', 4), ('ref_trilinear_devoxelize', 5),
                           ('ref_trilinear_devoxelize_grad', 4), ('ref_grouping', 5), ('ref_grouping_grad', 5),
                           ('ref_gather_features', 4), ('ref_gather_features_grad', 4), ('ref_furthest_point_sampling', 3),
                           ('ref_three_nn_interpolate', 4), ('ref_three_nn_interpolate_grad', 4)]:
            fn = getattr(self.lib, name)
            nptr = {'ref_avg_voxelize': 5, 'ref_avg_voxelize_grad': 4, 'ref_trilinear_devoxelize': 5,
                    'ref_trilinear_devoxelize_grad': 4, 'ref_grouping': 3, 'ref_grouping_grad': 3, 'ref_gather_features': 3,
                    'ref_gather_features_grad': 3, 'ref_furthest_point_sampling': 3, 'ref_three_nn_interpolate': 6,
                    'ref_three_nn_interpolate_grad': 4}[name]
            fn.argtypes = [ctypes.c_int] * nint + [ctypes.c_void_p] * nptr
            fn.restype = None
        self.lib.ref_ball_query.restype = None

    def gather_features_forward(self, features, indices):
        b, c, n = features.shape; m = indices.shape[1]
        out = torch.zeros(b, c, m)
        self.lib.ref_gather_features(b, c, n, m, _p(features), _p(indices), _p(out))
        return out

    def gather_features_backward(self, grad_y, indices, n):
        b, c, m = grad_y.shape
        gx = torch.zeros(b, c, n)
        self.lib.ref_gather_features_grad(b, c, n, m, _p(grad_y), _p(indices), _p(gx))
        return gx

    def furthest_point_sampling(self, coords, num_samples):
        b, _, n = coords.shape
        indices = torch.zeros(b, num_samples, dtype=torch.int32)
        distances = torch.full((b, n), 1e38)
        self.lib.ref_furthest_point_sampling(b, n, num_samples, _p(coords), _p(distances), _p(indices))
        return indices

    def ball_query(self, centers_coords, points_coords, radius, num_neighbors):
        b, _, m = centers_coords.shape; n = points_coords.shape[2]
        out = torch.zeros(b, m, num_neighbors, dtype=torch.int32)
        r = ctypes.c_float(radius).value
        self.lib.ref_ball_query(b, n, m, ctypes.c_float(r * r).value, num_neighbors, _p(centers_coords), _p(points_coords), _p(out))
        return out

    def grouping_forward(self, features, indices):
        b, c, n = features.shape; _, m, u = indices.shape
        out = torch.zeros(b, c, m, u)
        self.lib.ref_grouping(b, c, n, m, u, _p(features), _p(indices), _p(out))
        return out

    def grouping_backward(self, grad_y, indices, n):
        b, c = grad_y.shape[:2]; _, m, u = indices.shape
        gx = torch.zeros(b, c, n)
        self.lib.ref_grouping_grad(b, c, n, m, u, _p(grad_y), _p(indices), _p(gx))
        return gx

    def three_nearest_neighbors_interpolate_forward(self, points_coords, centers_coords, centers_features):
        b, c, m = centers_features.shape; n = points_coords.shape[2]
        indices = torch.zeros(b, 3, n, dtype=torch.int32); weights = torch.zeros(b, 3, n); out = torch.zeros(b, c, n)
        self.lib.ref_three_nn_interpolate(b, c, m, n, _p(points_coords), _p(centers_coords), _p(centers_features),
                                          _p(indices), _p(weights), _p(out))
        return [out, indices, weights]

    def three_nearest_neighbors_interpolate_backward(self, grad_y, indices, weights, m):
        b, c, n = grad_y.shape
        gx = torch.zeros(b, c, m)
        self.lib.ref_three_nn_interpolate_grad(b, c, n, m, _p(grad_y), _p(indices), _p(weights), _p(gx))
        return gx

    def trilinear_devoxelize_forward(self, r, is_training, coords, features):
        b, c = features.shape[:2]; n = coords.shape[2]
        outs = torch.zeros(b, c, n)
        if is_training:
            inds = torch.zeros(b, 8, n, dtype=torch.int32); wgts = torch.zeros(b, 8, n)
        else:
            inds = torch.zeros(1, dtype=torch.int32); wgts = torch.zeros(1)
        self.lib.ref_trilinear_devoxelize(b, c, n, int(r), int(bool(is_training)), _p(coords), _p(features), _p(inds), _p(wgts), _p(outs))
        return [outs, inds, wgts]

    def trilinear_devoxelize_backward(self, grad_y, indices, weights, r):
        b, c, n = grad_y.shape
        gx = torch.zeros(b, c, r * r * r)
        self.lib.ref_trilinear_devoxelize_grad(b, c, n, r * r * r, _p(indices), _p(weights), _p(grad_y), _p(gx))
        return gx

    def avg_voxelize_forward(self, features, coords, resolution):
        b, c, n = features.shape; r = int(resolution); s = r ** 3
        ind = torch.zeros(b, n, dtype=torch.int32); out = torch.zeros(b, c, s); cnt = torch.zeros(b, s, dtype=torch.int32)
        self.lib.ref_avg_voxelize(b, c, n, r, _p(coords), _p(features), _p(ind), _p(cnt), _p(out))
        return [out, ind, cnt]

    def avg_voxelize_backward(self, grad_y, indices, cnt):
        b, c, s = grad_y.shape; n = indices.shape[1]
        gx = torch.zeros(b, c, n)
        self.lib.ref_avg_voxelize_grad(b, c, n, s, _p(indices), _p(cnt), _p(grad_y), _p(gx))
        return gx


def _digest(h, tensors):
    for t in tensors:
        t = t.detach().cpu().contiguous()
        h.update(f'|{t.dtype}{tuple(t.shape)}|'.encode())
        h.update(t.numpy().tobytes())
    return h


def call_key(variant, op, args):
    """Digest of one backend call: the build variant, the function, and every argument (tensors by dtype, shape and bytes)."""
    h = hashlib.sha256(f'{variant}:{op}'.encode())
    for a in args:
        if isinstance(a, torch.Tensor):
            _digest(h, [a])
        else:
            h.update(f'|{a!r}|'.encode())
    return h.hexdigest()[:32]


def _bits(t):
    return t.contiguous().view(torch.int32)          # every output is float32 or int32


def _encode(ref, pred):
    """A reference output stored against the predictor's output for the same call: per tensor the XOR of the two bit patterns
    (all zeros where they agree -- nothing after compression) or, where shapes differ, the tensor itself; plus a digest of the
    reference output, which is what makes the stored form exact."""
    one = isinstance(ref, torch.Tensor)
    ref, pred = ([ref], [pred]) if one else (list(ref), list(pred))
    parts = []
    for r, p in zip(ref, pred):
        same_form = p is not None and r.shape == p.shape and r.dtype == p.dtype and r.element_size() == 4
        parts.append({'xor': _bits(r) ^ _bits(p)} if same_form else {'full': r.clone()})
    return {'one': one, 'parts': parts, 'sha': _digest(hashlib.sha256(), ref).hexdigest()}


def _decode(entry, pred):
    pred = [pred] if entry['one'] else list(pred)
    out = [part['full'].clone() if 'full' in part else (_bits(p) ^ part['xor']).view(p.dtype) for part, p in zip(entry['parts'], pred)]
    if _digest(hashlib.sha256(), out).hexdigest() != entry['sha']:
        raise AssertionError('the predictor\'s output for this call changed since the recording, so the recorded reference output cannot '
                             'be rebuilt from it: re-record with tests/golden/gen_golden.py where oracle/_ref can be built')
    return out[0] if entry['one'] else out


def save_recording(table, path):
    """A RecordedRefBackend table as an xz-compressed torch.save file."""
    buf = io.BytesIO()
    torch.save(table, buf)
    with open(path, 'wb') as f:
        f.write(lzma.compress(buf.getvalue(), preset=9 | lzma.PRESET_EXTREME))


def load_recording(path):
    with open(path, 'rb') as f:
        return torch.load(io.BytesIO(lzma.decompress(f.read())), weights_only=True)


class RecordedRefBackend:
    """The reference's kernels as RECORDED from RefCpuBackend, so that tests pinned to the reference run where oracle/_ref cannot be
    built.  Each recorded call (looked up by call_key) is stored against `predictor`'s output for the same inputs -- the CPU oracle,
    which agrees with the reference bit for bit on most calls -- and rebuilt from it exactly: the stored digest of the reference output
    must match, else the call fails.  A call whose inputs were never recorded is an error.  With `live` given, calls go to that
    backend and are added to `table`."""
    name = 'reference-kernels-recorded'

    def __init__(self, table, predictor, variant='fma', live=None):
        self.table, self.predictor, self.variant, self.live = table, predictor, variant, live

    def __getattr__(self, op):
        if op.startswith('_'):
            raise AttributeError(op)

        def call(*args):
            key = call_key(self.variant, op, args)
            pred = getattr(self.predictor, op)(*args)
            if self.live is not None:
                out = getattr(self.live, op)(*args)
                self.table[key] = _encode(out, pred)
                return out
            if key not in self.table:
                raise LookupError(f'{op} ({self.variant}): no recorded reference output for these inputs '
                                  '(tests/golden/gen_golden.py records them from oracle/_ref)')
            return _decode(self.table[key], pred)
        return call
