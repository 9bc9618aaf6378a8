"""Augmentation of an assembled training batch on the device (csrc/augment.hip): a rotation about the up axis, a small rotation
perturbation, axis flips, random scale and translation, clipped Gaussian jitter and PointNet++'s random point dropout.

Not in the reference: its datasets draw what `data.py` draws (ShapeNet's jitter, Frustum-KITTI's flip and shift).  A host
`Dataset.__getitem__` was where a user put these transforms; a batch assembled by `DeviceLoader.feed()` inside a captured step never
visits the host, so they run here: two launches (the per-cloud draws; one read and one write of the batch), capturable, no allocation
between them when `out=` is given.

    y = s * (Rp x) + t + jitter        planes (c, c + 1, c + 2) of a 'position' triple
    y = Rp x                            planes of a 'direction' triple (normals)
    Rp = Rx(a) Ry(b) Rz(c) R_axis(theta) diag(+-1)

with theta ~ U(-rotate_max, rotate_max), a, b, c = clip(perturb_sigma z, +-perturb_clip), axis k flipped with probability flip_prob[k],
s ~ U(scale), t ~ U(-translate, translate)^3, jitter = clip(jitter_sigma z, +-jitter_clip) per point and axis, and -- dropout -- every
point n > 0 whose uniform is <= ratio = u * dropout_max replaced by point 0 in ALL channels and in its target (PointNet++'s
`pc[drop_idx] = pc[0]`: the batch keeps its shape, a dropped point duplicates point 0 together with its label).  Every other channel
is copied.  Each element is computed in fp64 from the fp32 input, in the order written, and rounded once.

Two sources of randomness, as `data.py` has them: parity mode (the caller hands `params`, `jitter`, `keep`: the result is a function
of the arguments, bit-identical to `augment_reference`) and device mode (a Philox stream keyed by two int64 words in device memory:
no host round trip, fresh numbers on every graph replay, `torch.manual_seed` governs it).

`augment_reference` is the torch formulation (parity mode only, any device): the definition the kernel is tested against.  The
product path needs device tensors and the native library: there is no CPU fallback.
"""
import math

import numpy as np
import torch

from .modules.functional import backend as _seam

__all__ = ['Augment', 'compose_reference', 'PARAMS', 'POSITION', 'DIRECTION']

PARAMS = 24                       # doubles per cloud: Rp (9), s, t (3), ratio, theta a b c, the three flip uniforms, three zeros
POSITION, DIRECTION = 1, 2        # the role numbers of include/pvcnn_hip.h
_ROLES = {'position': POSITION, 'direction': DIRECTION}
_MAX_TRIPLES = 4


def _rotation(axis, angle):
    """The right-handed rotation about axis 0 (x), 1 (y) or 2 (z) by `angle` (any shape) -> (..., 3, 3)."""
    c, s = np.cos(angle), np.sin(angle)
    one, zero = np.ones_like(c), np.zeros_like(c)
    rows = {0: [[one, zero, zero], [zero, c, -s], [zero, s, c]],
            1: [[c, zero, s], [zero, one, zero], [-s, zero, c]],
            2: [[c, -s, zero], [s, c, zero], [zero, zero, one]]}[axis]
    return np.stack([np.stack(r, axis=-1) for r in rows], axis=-2)


def compose_reference(raw, rotate_axis=2, flip_prob=(0.0, 0.0, 0.0)):
    """Rp (..., 3, 3) from the raw draws of params rows `raw` (..., 24) -- columns 14..17 the angles theta, a, b, c, columns 18..20 the
    flip uniforms (axis k is flipped when u_k < flip_prob[k]) -- in numpy fp64: Rx(a) Ry(b) Rz(c) R_axis(theta) diag(+-1)."""
    raw = np.asarray(raw.detach().cpu() if isinstance(raw, torch.Tensor) else raw, dtype=np.float64)
    theta, a, b, c = (raw[..., k] for k in range(14, 18))
    sign = np.where(raw[..., 18:21] < np.asarray(flip_prob, dtype=np.float64), -1.0, 1.0)
    m = _rotation(0, a) @ _rotation(1, b) @ _rotation(2, c) @ _rotation(int(rotate_axis), theta)
    return m * sign[..., None, :]


class Augment:
    """The transforms of one training set-up; every range defaults to "off" (the identity of its stage, exactly).

    layout: [('position' | 'direction', first_channel), ...], at most four triples: which channel planes are coordinates and which
    are directions (normals).  rotate_axis: 0, 1, 2 = x, y, z.  A positive sigma needs a positive clip (math.inf: no clip)."""

    def __init__(self, layout=(('position', 0),), rotate_axis=2, rotate_max=0.0, perturb_sigma=0.0, perturb_clip=0.0,
                 flip_prob=(0.0, 0.0, 0.0), scale=(1.0, 1.0), translate=0.0, jitter_sigma=0.0, jitter_clip=0.0, dropout_max=0.0):
        triples = []
        for entry in layout:
            role, first = entry
            if role not in _ROLES:
                raise ValueError(f"layout roles are 'position' and 'direction', got {role!r}")
            if int(first) != first or int(first) < 0:
                raise ValueError('a triple starts at a non-negative channel')
            triples.append((_ROLES[role], int(first)))
        if len(triples) > _MAX_TRIPLES:
            raise ValueError(f'a layout holds at most {_MAX_TRIPLES} triples')
        starts = sorted(first for _, first in triples)
        if any(b < a + 3 for a, b in zip(starts, starts[1:])):
            raise ValueError('the triples of a layout overlap')
        self.layout = tuple(triples)
        if rotate_axis not in (0, 1, 2):
            raise ValueError('rotate_axis must be 0, 1 or 2')
        self.rotate_axis = int(rotate_axis)
        flip_prob, scale = tuple(float(p) for p in flip_prob), tuple(float(s) for s in scale)
        if len(flip_prob) != 3 or not all(0.0 <= p <= 1.0 for p in flip_prob):
            raise ValueError('flip_prob: three probabilities expected')
        if len(scale) != 2 or not (math.isfinite(scale[0]) and math.isfinite(scale[1])) or scale[0] > scale[1]:
            raise ValueError('scale = (low, high) with low <= high expected')
        self.flip_prob, self.scale = flip_prob, scale
        for name, value in (('rotate_max', rotate_max), ('perturb_sigma', perturb_sigma), ('translate', translate),
                            ('jitter_sigma', jitter_sigma)):
            if not (math.isfinite(value) and value >= 0.0):
                raise ValueError(f'{name} must be finite and not negative')
        for name, sigma, clip in (('perturb', perturb_sigma, perturb_clip), ('jitter', jitter_sigma, jitter_clip)):
            if not clip >= 0.0 or (sigma > 0.0 and not clip > 0.0):
                raise ValueError(f'{name}_clip must be positive where {name}_sigma is (clip 0 would clip every draw to 0; '
                                 'math.inf: no clip)')
        if not 0.0 <= dropout_max <= 1.0:
            raise ValueError('dropout_max must lie in [0, 1]')
        self.rotate_max, self.perturb_sigma, self.perturb_clip = float(rotate_max), float(perturb_sigma), float(perturb_clip)
        self.translate, self.jitter_sigma, self.jitter_clip = float(translate), float(jitter_sigma), float(jitter_clip)
        self.dropout_max = float(dropout_max)

    @classmethod
    def s3dis(cls, **ranges):
        """S3DIS batches (B, 9 or 6, N): coordinates in channels 0..2; colours and normalised room coordinates (3..8) untouched."""
        return cls(layout=[('position', 0)], **ranges)

    @classmethod
    def shapenet(cls, with_normal=True, **ranges):
        """ShapeNet batches: coordinates in channels 0..2, normals (with_normal) in 3..5, the one-hot planes untouched."""
        return cls(layout=[('position', 0)] + ([('direction', 3)] if with_normal else []), **ranges)

    # -- what is on --
    @property
    def jitter_on(self):
        return self.jitter_sigma > 0.0

    @property
    def dropout_on(self):
        return self.dropout_max > 0.0

    def compose_reference(self, raw):
        """`compose_reference` with this object's axis and flip probabilities."""
        return compose_reference(raw, self.rotate_axis, self.flip_prob)

    # -- shared argument handling --
    def check_channels(self, channels):
        """ValueError unless every triple of the layout lies inside `channels` planes."""
        for _, first in self.layout:
            if first + 3 > channels:
                raise ValueError(f'the layout has a triple at channels {first}..{first + 2}, the batch has {channels}')

    def _check_batch(self, x, targets):
        if x.dim() != 3 or x.dtype != torch.float32:
            raise ValueError(f'x (B, C, N) fp32 expected, got {tuple(x.shape)} {x.dtype}')
        self.check_channels(x.shape[1])
        if targets is not None and (tuple(targets.shape) != (x.shape[0], x.shape[2]) or targets.dtype != torch.int64):
            raise ValueError(f'targets (B, N) int64 expected, got {tuple(targets.shape)} {targets.dtype}')

    def _draws(self, x, params, jitter, keep):
        """The parity draws on x's device in the kernel's types; ValueError for a wrong shape or a stage without its draws."""
        b, _, n = x.shape
        out = []
        for t, shape, dtype, name, needed in ((params, (b, PARAMS), torch.float64, 'params', True),
                                              (jitter, (b, 3, n), torch.float32, 'jitter', self.jitter_on),
                                              (keep, (b, n), torch.float32, 'keep', self.dropout_on)):
            if t is None or not needed:
                if needed:
                    raise ValueError(f'parity mode takes every draw from the caller: `{name}` {shape} is missing')
                out.append(None)
                continue
            t = torch.as_tensor(t)
            if tuple(t.shape) != shape:
                raise ValueError(f'{name} of shape {shape} expected, got {tuple(t.shape)}')
            out.append(t.to(device=x.device, dtype=dtype).contiguous())
        return out

    # -- the torch formulation --
    def augment_reference(self, x, targets, params, jitter=None, keep=None):
        """(features, targets) in parity mode on x's device, by torch: fp64 arithmetic in the stated order, one rounding to fp32."""
        self._check_batch(x, targets)
        params, jitter, keep = self._draws(x, params, jitter, keep)
        col = lambda k: params[:, k, None]                                   # (B, 1) against the (B, N) planes
        out = x.clone()
        for role, first in self.layout:
            x0, x1, x2 = (x[:, first + k].to(torch.float64) for k in range(3))
            for k in range(3):
                v = (col(3 * k) * x0 + col(3 * k + 1) * x1) + col(3 * k + 2) * x2
                if role == POSITION:
                    v = col(9) * v + col(10 + k)
                    if self.jitter_on:
                        v = v + (self.jitter_sigma * jitter[:, k].to(torch.float64)).clamp(-self.jitter_clip, self.jitter_clip)
                out[:, first + k] = v.to(torch.float32)
        if self.dropout_on:
            dropped = keep.to(torch.float64) <= col(13)
            dropped[:, 0] = False
            out = torch.where(dropped[:, None, :], out[:, :, :1], out)
            if targets is not None:
                targets = torch.where(dropped, targets[:, :1], targets)
        return out, (None if targets is None else targets.clone())

    # -- the product path --
    def _backend(self, x):
        be = _seam._backend
        if not x.is_cuda or not getattr(be, 'has_augment', False):
            raise RuntimeError('augment needs CUDA (HIP) tensors and the native library -- there is no CPU implementation; '
                               '`augment_reference` is the torch formulation')
        return be

    def draw(self, batch_size, seed, out=None):
        """params (B, 24) fp64 on seed's device from the Philox stream of `seed` (two int64 words on the device): one launch."""
        _seam.check_seed(seed)
        if out is None:
            out = torch.empty((int(batch_size), PARAMS), dtype=torch.float64, device=seed.device)
        elif tuple(out.shape) != (int(batch_size), PARAMS) or out.dtype != torch.float64 or not out.is_contiguous() or out.device != seed.device:
            raise ValueError(f'params buffer: contiguous fp64 ({int(batch_size)}, {PARAMS}) on {seed.device} expected')
        self._backend(seed).augment_draw(out, seed, self.rotate_axis,
                                         (self.rotate_max, self.perturb_sigma, self.perturb_clip, *self.flip_prob, *self.scale,
                                          self.translate, self.dropout_max))
        return out

    def augment(self, x, targets=None, *, out=None, out_targets=None, seed=None, params=None, jitter=None, keep=None,
                return_draws=False, params_out=None):
        """x (B, C, N) fp32 [, targets (B, N) int64] on the device -> the augmented batch, out of place (`out`, `out_targets`: where to
        write; allocated when missing).  The tensors may be batch-strided views (a channel slice keeps its samples contiguous).  `out`
        may be `x` itself unless dropout is on.

        Parity mode: `params` (B, 24) fp64, with `jitter` (B, 3, N) and `keep` (B, N) fp32 where those stages are on -- one launch.
        Device mode (default): two launches keyed by `seed` (two int64 words on the device; drawn from torch's device generator when
        None: no host synchronisation); `params_out`: a (B, 24) fp64 buffer for the per-cloud draws instead of a fresh one.
        Returns `out`, or `(out, out_targets)` with targets; with return_draws=True that and {'params', 'jitter', 'keep'}: the draws
        in use (None for a stage that is off), which reproduce the call in parity mode."""
        be = self._backend(x)
        self._check_batch(x, targets)
        b, c, n = x.shape
        if params is None and (jitter is not None or keep is not None):
            raise ValueError('`jitter` / `keep` draws without `params`: parity mode takes every draw from the caller')
        if out is None:
            out = torch.empty((b, c, n), dtype=torch.float32, device=x.device)
        elif tuple(out.shape) != (b, c, n) or out.dtype != torch.float32 or out.device != x.device:
            raise ValueError(f'out: fp32 {(b, c, n)} on {x.device} expected')
        if targets is None:
            if out_targets is not None:
                raise ValueError('out_targets without targets')
        elif out_targets is None:
            out_targets = torch.empty((b, n), dtype=torch.int64, device=x.device)
        elif tuple(out_targets.shape) != (b, n) or out_targets.dtype != torch.int64 or out_targets.device != x.device:
            raise ValueError(f'out_targets: int64 {(b, n)} on {x.device} expected')
        for t in (targets, out_targets):
            if t is not None and not ((n == 1 or t.stride(1) == 1) and (b == 1 or t.stride(0) >= n)):
                raise ValueError('targets: the N labels of a sample must be contiguous, samples at least N apart')
        if self.dropout_on and (out.data_ptr() == x.data_ptr() or (targets is not None and out_targets.data_ptr() == targets.data_ptr())):
            raise ValueError('with dropout on, the batch cannot be augmented in place: a dropped point reads point 0')
        if params is not None:
            params, jitter, keep = self._draws(x, params, jitter, keep)
            seed = None
        else:
            if seed is None:
                seed = _seam.fresh_seed(x.device)
            params = self.draw(b, seed, params_out)
        jitter_out = keep_out = None
        if return_draws:
            jitter_out = torch.empty((b, 3, n), dtype=torch.float32, device=x.device) if self.jitter_on else None
            keep_out = torch.empty((b, n), dtype=torch.float32, device=x.device) if self.dropout_on else None
        be.augment_apply(x, targets, self.layout, params, self.jitter_sigma, self.jitter_clip, self.jitter_on, self.dropout_on, jitter, keep,
                         seed, out, out_targets, jitter_out, keep_out)
        result = out if targets is None else (out, out_targets)
        if return_draws:
            return result, {'params': params, 'jitter': jitter_out, 'keep': keep_out}
        return result
