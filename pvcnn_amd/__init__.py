"""pvcnn_amd -- MI355X (gfx950) native PVConv hot path behind the reference's operator API.

Layout (only what the hot path needs):
  csrc/      hand-written HIP kernels + the C ABI (include/pvcnn_hip.h) -> libpvcnn_hip.so
  _lib.py    ctypes binding of that C ABI (fails loudly when the library is missing)
  modules/   host-side mirror of the reference's `modules` package (same names, ctor/forward
             signatures, state_dict keys); `modules.functional.backend._backend` is the seam
  dp.py      one-process-per-GPU data-parallel gradient all-reduce (RCCL) harness
  workload.py  synthetic (B,C,N,R) inputs + the PVCNN/PVCNN++ network builders used by bench.py

`install_dropin()` registers `pvcnn_amd.modules` under the top-level name `modules`, so the
reference's unchanged `models/` (`from modules import PVConv, ...`) run on this backend.
"""
import importlib
import sys

__version__ = '0.1.0'

_DROPIN_SUBMODULES = (
    'ball_query', 'frustum', 'loss', 'pointnet', 'pvconv', 'se', 'shared_mlp', 'voxelization',
    'functional', 'functional.backend', 'functional.ball_query', 'functional.devoxelization',
    'functional.grouping', 'functional.interpolatation', 'functional.loss', 'functional.sampling',
    'functional.voxelization',
)


def install_dropin(name='modules'):
    """Alias pvcnn_amd.modules (and every sub-module the reference imports by path) as `name`."""
    impl = importlib.import_module('pvcnn_amd.modules')
    sys.modules[name] = impl
    for sub in _DROPIN_SUBMODULES:
        sys.modules[f'{name}.{sub}'] = importlib.import_module(f'pvcnn_amd.modules.{sub}')
    return impl


_ADOPTED = {}          # (original class, donor forward) -> the derived class, registered in this module under an importable name


def _adopted_class(cls, forward, extra=None):
    """`cls` with `forward` replaced, created ONCE per (class, forward) and registered as an attribute of this module under its own
    `__qualname__`, so that `pickle` / `torch.save(model)` / mp-spawn find it again by name (a class created inside a
    function call cannot be pickled)."""
    key = (cls, forward, tuple(sorted((extra or {}).items())))
    if key not in _ADOPTED:
        name = '_Adopted_' + ''.join(c if c.isalnum() else '_' for c in f'{cls.__module__}.{cls.__qualname__}')
        if any(k[0] is cls for k in _ADOPTED):                      # the same class with another donor: a name of its own
            name += f'_{len(_ADOPTED)}'
        body = {'forward': forward, '__module__': __name__, '__qualname__': name, '_adopted_from': cls}
        body.update(extra or {})
        derived = type(cls.__name__, (cls,), body)                  # keeps the class NAME (repr, logs); pickle goes by __qualname__
        setattr(sys.modules[__name__], name, derived)
        _ADOPTED[key] = derived
    return _ADOPTED[key]


def _classify_forward(self, x):
    import torch
    from . import workload
    if not torch.is_tensor(x):             # a stack fed with (features, coords) tuples (box_estimation/pointnet.py:37): the modules as they are
        return torch.nn.Sequential.forward(self, x)
    return workload._classify(self, x)


def adopt(model):
    """Opt-in, ONE line in the caller's script -- `model = pvcnn_amd.adopt(model)` after building a reference network on top of
    `install_dropin()` -- for what a swapped `modules` package cannot reach: the torch glue the reference's `models/` put BETWEEN the
    operators (models/s3dis/pvcnn.py:34-46: `.max()` over the points, `.repeat()`, `torch.cat`; models/utils.py:15-46: `nn.Dropout` and
    a bare `nn.Conv1d` inside the classifier's `nn.Sequential`).  The instance keeps its parameters, buffers, sub-module names and
    state_dict; only `forward` changes, to `pvcnn_amd.workload`'s composition of the same operators:
      * a point-wise head [SharedMLP, Dropout, ..., Conv1d] runs module by module on this package's kernels (Dropout on the BatchNorm
        passes, the last Conv1d on the 1x1 GEMM): any `nn.Sequential` of that shape inside `model`;
      * a network with the attribute structure of the reference's S3DIS PVCNN / ShapeNet PVCNN / S3DIS PVCNN++ takes the matching
        workload forward (max-pool winners out of the BatchNorm pass, one concatenation kernel that also emits the scale table);
      * (round 6) a Frustum network (`inst_seg_net` / `center_reg_net` / `box_est_net`, models/kitti/frustum/frustum_net.py:14-76): its
        segmentation net takes workload's forward (the last stage into its slice of the concatenation, row maxima out of the BatchNorm
        pass), its two regression nets the dense-head kernel behind their global max.
    Anything it does not recognise is left as it is; CPU tensors, eval mode and hooked modules fall back to the modules themselves
    inside those forwards.  `bench.py` reports both compositions (`value` and `reference_composition_value`).
    The swapped classes are registered in this module by name: an adopted model pickles (`torch.save(model)`) in a process that has
    imported `pvcnn_amd` and adopted a model of the same class first (the derived class is created by `adopt`, not at import time);
    `state_dict()` checkpoints are unaffected."""
    import torch.nn as nn
    from . import workload
    from .modules import SharedMLP

    def is_head(seq):
        kids = list(seq)
        return (len(kids) >= 2 and isinstance(kids[0], SharedMLP) and isinstance(kids[-1], (nn.Conv1d, SharedMLP))
                and all(isinstance(k, (SharedMLP, nn.Dropout, nn.Conv1d)) for k in kids))

    def take(module, donor_forward, extra=None):
        if type(module).forward is not donor_forward:
            module.__class__ = _adopted_class(type(module), donor_forward, extra)

    for m in model.modules():
        if type(m) is nn.Sequential and is_head(m):
            m.__class__ = _adopted_class(nn.Sequential, _classify_forward)
    has = lambda obj, *names: all(hasattr(obj, a) for a in names)
    if has(model, 'inst_seg_net', 'center_reg_net', 'box_est_net'):
        seg, ctr, box = model.inst_seg_net, model.center_reg_net, model.box_est_net
        if has(seg, 'point_features', 'cloud_features', 'classifier', 'in_channels'):
            take(seg, workload._FrustumSegmentation.forward)
        if has(ctr, 'features', 'regression'):
            take(ctr, workload._CloudRegressor.forward, {'_head_attr': 'regression', '_coords_tuple': False})
        if has(box, 'features', 'classifier'):
            take(box, workload._CloudRegressor.forward, {'_head_attr': 'classifier', '_coords_tuple': True})
        return model
    donor = None
    if has(model, 'sa_layers', 'fp_layers', 'classifier'):
        donor = workload.PVCNN2
    elif has(model, 'point_features', 'classifier', 'num_shapes', 'in_channels') and isinstance(model.point_features, nn.ModuleList):
        donor = workload.PVCNNShapeNet
    elif has(model, 'point_features', 'cloud_features', 'classifier') and isinstance(model.point_features, nn.ModuleList):
        donor = workload.PVCNN
    if donor is not None:
        take(model, donor.forward)
    return model


def fold_batchnorm(model):
    """Opt-in, ONE line -- `model = pvcnn_amd.fold_batchnorm(model)` before handing a trained network to `evaluate.*`,
    `rooms.segment_room` or the Frustum evaluation: puts `model` in eval() and folds every BatchNorm that directly follows a SharedMLP
    1x1 convolution or a PVConv Conv3d (and is followed by a ReLU / LeakyReLU) into that convolution's weights.  Under
    `torch.no_grad()` / `inference_mode` such a triple then runs as ONE product whose epilogue applies the activation and emits the
    scale table of what it writes: no stand-alone BatchNorm pass, no re-read of the tensor (functional/_fold.py, functional/bnact.py:
    run_layers).  The folded weights are snapshots attached to the convolutions as plain attributes: parameters, buffers and
    `state_dict()` are untouched, checkpoints save and load as before.  A snapshot is never stale -- after any change to the six
    tensors it was formed from (in place, by `load_state_dict`, by FlatAdam), `.train()`, or with gradients enabled, the modules run as
    they always did; call `fold_batchnorm` again after changing the weights.  Returns `model`."""
    import torch.nn as nn
    from .modules.functional import _fold
    from .modules.functional.bnact import _is_pointwise, _slope
    model.eval()
    for seq in model.modules():
        if not isinstance(seq, nn.Sequential):
            continue
        kids = list(seq)
        for conv, bn, act in zip(kids, kids[1:], kids[2:]):
            if ((_is_pointwise(conv) or hasattr(conv, 'forward_with_stats')) and isinstance(bn, nn.modules.batchnorm._BatchNorm)
                    and bn.running_mean is not None and bn.running_var is not None and bn.num_features == conv.out_channels
                    and _slope(act) is not None):
                _fold.attach(conv, bn)
    return model


def unfold_batchnorm(model):
    """Remove the snapshots of `fold_batchnorm`: the model is the one it was before (its mode stays as it is).  Returns `model`."""
    from .modules.functional import _fold
    for m in model.modules():
        _fold.detach(m)
    return model
