"""What HipBackend sends to the C library outside the Conv3d / 1x1 products, and what the three BatchNorm autograd nodes ask of a
backend, pinned call by call on the CPU against tests/golden/backend_calls.json (recorded by tests/golden/gen_backend_calls_golden.py,
which imports the cases and the stand-ins below).  The harness -- proxy library, pointer roles, tables -- is test_product_host.py's.

  * lib   -- every public HipBackend method that reaches the library and is not in product_calls.json already, at tiny shapes over
             its optional arguments and mode flags, with a call that trips each of its shape messages.  No method is left out: none
             steers host control flow by what a kernel wrote (the proxy runs no kernel, outputs stay uninitialised).
  * node  -- BatchNormAct / BatchNormActDevoxelize / BatchNormActSEDevoxelize on a recording stand-in that computes with torch (and
             the CPU oracle's devoxelization): the call log of every case equals the golden, outputs, gradients, running statistics
             and num_batches_tracked equal the plain modules'.
  * the launch helper itself: what it converts, where the stream goes, how a library error surfaces."""
import contextlib
import ctypes
import inspect
import itertools
import os
import types
import weakref

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import ROOT
import test_product_host as host

GOLDEN_PATH = os.path.join(ROOT, 'tests', 'golden', 'backend_calls.json')
F32, F64, I8, U8, I32, I64 = torch.float32, torch.float64, torch.int8, torch.uint8, torch.int32, torch.int64
CPU = torch.device('cpu')


def z(*shape, dtype=F32):
    return torch.zeros(*shape, dtype=dtype)


# ---- the lib log: the cases -------------------------------------------------------------------------------------------------------
def _annos(*images):
    def one(names):
        n = len(names)
        return {'name': np.array(names), 'bbox': np.zeros((n, 4)), 'alpha': np.zeros(n), 'occluded': np.zeros(n), 'truncated': np.zeros(n),
                'score': np.zeros(n), 'location': np.zeros((n, 3)), 'dimensions': np.ones((n, 3)), 'rotation_y': np.zeros(n)}
    return [one(names) for names in images]


def _packed(gt, dt):
    from pvcnn_amd.kitti import _Packed
    p = _Packed(_annos(*gt), _annos(*dt), device=CPU)
    p.boxes_3d(1), p.boxes_3d(2)
    return p


def _voxel_plan(b, n, r):
    from pvcnn_amd.modules.functional.backend import HipBackend
    vp = HipBackend.VoxelPlan()
    vp.b, vp.n, vp.r, vp.ind, vp.cnt, vp.plan = b, n, r, z(b, n, dtype=I32), z(b, r ** 3, dtype=I32), z(64, dtype=U8)
    return vp


def _bank_refresh(be, kind, nsplit, shape):
    """_WeightBank.refresh on a bank holding one entry (a CPU weight never registers itself: _rebuild wants device tensors), then what
    take() serves -> (armed before the take, what the take returned, armed after)."""
    w, table = z(*shape), z(1, 10, dtype=I64)
    bank = be._bank()
    key = (kind, w.data_ptr(), (shape[0], shape[1]), nsplit)
    entry = {'param': weakref.ref(w), 'armed': False, 'version': -1, 'epoch': -1, 'wf': z(32, dtype=U8), 'wb': z(48, dtype=U8)}
    bank.entries, bank.tables, bank.dirty = {key: entry}, {(kind, nsplit): (table, 1, 7, [key], CPU)}, False
    host_rec = be.lib._rec
    host_rec.named.update({table.data_ptr(): 'table'})
    host_rec.held += [w, table]
    be.weight_bank_refresh()
    armed = entry['armed']
    pair = bank.take(kind, w, nsplit)
    return armed, pair, entry['armed']


def lib_cases():
    """(settings of the backend object, method name or callable, keyword arguments ('*': further positional ones)) of every pinned call."""
    out, tf = [], (False, True)

    def add(method, good, *bad, **settings):
        for kw in (good, *({**good, **b} for b in bad)):
            out.append((settings, method, kw))

    def vary(method, base, axes, **settings):
        for values in itertools.product(*axes.values()):
            out.append((settings, method, {**base, **dict(zip(axes, values))}))

    b, c, n, m, u, r = 2, 6, 5, 4, 2, 2
    pts, ctr, ivox, feat, grid = z(b, 3, n), z(b, 3, m), z(b, 3, n, dtype=I32), z(b, c, n), z(b, c, r ** 3)
    # sampling, ball query, grouping, 3-NN
    add('gather_features_forward', {'features': feat, 'indices': z(b, m, dtype=I32)}, {'indices': z(3, m, dtype=I32)})
    add('gather_features_backward', {'grad_y': z(b, c, m), 'indices': z(b, m, dtype=I32), 'n': n}, {'indices': z(b, n, dtype=I32)})
    add('furthest_point_sampling', {'coords': pts, 'num_samples': m}, {'coords': z(1, 3, 16385)}, {'coords': z(b, 2, n)})
    mask = z(b, n, dtype=torch.bool)
    add('mask_select', {'mask': mask, 'num_samples': m, 'choices': z(b, m, dtype=I32)}, {'choices': None, 'seed': z(2, dtype=I64)},
        {'choices': z(b, 3, dtype=I32), 'seed': z(2, dtype=I64)}, {'mask': z(b, n)}, {'choices': None, 'seed': z(2, dtype=I32)})
    add('batch_launch', {'entry': 'batch_s3dis', 'ref': pts, '*': (pts, None, 3, z(4, dtype=I64), True, None)},
        {'*': (pts, z(4, 4).t())})
    add('ball_query', {'centers_coords': ctr, 'points_coords': pts, 'radius': 0.5, 'num_neighbors': u}, {'centers_coords': z(b, 2, m)})
    add('grouping_forward', {'features': feat, 'indices': z(b, m, u, dtype=I32)}, {'indices': z(3, m, u, dtype=I32)})
    add('grouping_backward', {'grad_y': z(b, c, m, u), 'indices': z(b, m, u, dtype=I32), 'n': n}, {'indices': z(b, m, 3, dtype=I32)})
    add('three_nearest_neighbors_interpolate_forward', {'points_coords': pts, 'centers_coords': ctr, 'centers_features': z(b, c, m)},
        {'centers_features': z(b, c, n)})
    add('three_nearest_neighbors_interpolate_backward', {'grad_y': feat, 'indices': z(b, 3, n, dtype=I32), 'weights': z(b, 3, n), 'm': m},
        {'weights': z(b, 3, m)})
    # voxelize and devoxelize: one-shot, plan and apply, with and without the memo behind the seam's own calls
    vary('trilinear_devoxelize_forward', {'r': r, 'coords': pts, 'features': grid}, {'is_training': tf})
    add('trilinear_devoxelize_forward', {'r': r, 'is_training': True, 'coords': pts, 'features': z(b, c, 7)})
    inds, wgts, sliced = z(b, 8, n, dtype=I32), z(b, 8, n), z(b, c + 2, n)[:, :c]
    for memo in tf:
        devox_bwd = {'grad_y': feat, 'indices': inds, 'weights': wgts, 'r': r}
        add('trilinear_devoxelize_backward', devox_bwd, devox_bwd, {'grad_y': sliced}, {'indices': z(b, 8, m, dtype=I32)}, seam_plan_memo=memo)
        vox_fwd = {'features': feat, 'coords': ivox, 'resolution': r}
        add('avg_voxelize_forward', vox_fwd, vox_fwd, {'coords': z(b, 3, m, dtype=I32)}, seam_plan_memo=memo)
    vary('voxel_coords', {'coords': pts, 'resolution': r, 'eps': 0.0}, {'normalize': tf})
    add('voxel_coords', {'coords': z(b, 2, n), 'resolution': r, 'normalize': True, 'eps': 0.0})
    add('voxel_coords_tail', {'coords': pts, 'mean': z(b, 3, 1), 'radius': z(b, 1, 1), 'resolution': r, 'eps': 1e-6}, {'radius': None},
        {'coords': z(b, 5, n)[:, 1:4]}, {'coords': z(b, 3, n + 3)[:, :, :n]}, {'coords': z(b, 2, n)}, {'mean': z(b, 2, 1)}, {'radius': z(3, 1, 1)})
    add('avg_voxelize_backward', {'grad_y': grid, 'indices': z(b, n, dtype=I32), 'cnt': z(b, r ** 3, dtype=I32)}, {'cnt': z(b, 7, dtype=I32)})
    add('avg_voxelize_plan', {'coords': ivox, 'resolution': r}, {'resolution': 1024}, {'coords': z(b, 2, n, dtype=I32)})
    add('pvconv_plans', {'vox_coords': ivox, 'norm_coords': pts, 'resolution': r}, {'resolution': 1024},
        {'vox_coords': z(b, 3, 0, dtype=I32), 'norm_coords': z(b, 3, 0)}, {'norm_coords': z(b, 3, m)})
    add('avg_voxelize_apply', {'features': feat, 'vp': _voxel_plan(b, n, r)}, {'features': z(b, c, m)})
    add('trilinear_devoxelize_backward_plan', {'indices': inds, 'weights': wgts, 'r': r}, {'r': 1024}, {'weights': z(b, 8, m)})
    add('trilinear_devoxelize_backward_apply', {'grad_y': feat, 'plan': z(64, dtype=U8), 'r': r}, {'grad_y': sliced})
    # amax buffers
    add('absmax_bits', {'x': feat})
    for amax_global in tf:
        vary('absmax_tiles', {'x': feat, 'seg': 4}, {'want_global': tf}, amax_global=amax_global)
    add('absmax_tiles', {'x': z(b, n), 'seg': 4})
    add('amax_buffer', {'b': b, 'n': n, 'seg': 4, 'device': CPU})
    add('amax_and_row_keys', {'b': b, 'c': 4, 'n': 256, 'seg': 64, 'device': CPU})
    # the BatchNorm family
    c, s = 4, 8
    x, gy, gam, bet, mean, rstd = z(b, c, s), z(b, c, s), z(c), z(c), z(c), z(c)
    rm, rv, seed = z(c), z(c), z(1, dtype=I64)
    add('dropout_keep_mask', {'seed': seed, 'p': 0.5, 'numel': 7})
    fwd = {'x': x, 'running_mean': rm, 'running_var': rv, 'momentum': 0.1, 'eps': 1e-5, 'slope': 0.1}
    for affine, amax_seg in itertools.product(tf, (0, 4)):
        vary('bnact_forward', {**fwd, 'gamma': gam if affine else None, 'beta': bet if affine else None, 'amax_seg': amax_seg},
             {'training': tf, 'stats': (None, (mean, rstd)), 'y_amax': (None, z(5, dtype=I32)), 'drop': (None, (seed, 0.5))})
    add('bnact_forward', {**fwd, 'gamma': gam, 'beta': bet, 'training': True, 'running_mean': None, 'running_var': None})
    whole = z(6 + 2 * b * c, dtype=I32)
    wide, wide_out = z(b, c, 256), z(b, c + 2, 256)
    rowmax = {'x': wide, 'gamma': gam, 'beta': bet, 'mean': mean, 'rstd': rstd, 'slope': 0.1, 'amax_seg': 64, 'y_amax': whole[:5],
              'row_keys': whole[6:]}
    add('bnact_apply_rowmax', rowmax, {'gamma': None, 'beta': None, 'out': wide_out[:, :c]}, {'x': wide[:1], 'out': wide_out[:1, :c]},
        {'x': x}, {'amax_seg': 48}, {'out': wide_out[:, 1:c + 1].transpose(1, 2).contiguous().transpose(1, 2)}, {'out': z(b, c, 128)})
    part = z(c, 3, 2)
    vary('bn_finalize', {'part': part, 'count': b * s, 'momentum': 0.1, 'eps': 1e-5},
         {'running_mean': (rm, None), 'running_var': (rv, None), 'shift': (None, z(c)), 'zero_word': (None, z(5, dtype=I32)),
          'counter': (None, z(1, dtype=I64))})
    vary('bn_stats', {'x': x, 'momentum': 0.1, 'eps': 1e-5}, {'running_mean': (rm, None), 'running_var': (rv, None)})
    devox = {'r': r, 'coords': pts, 'features': z(b, c, r ** 3), 'mean': mean, 'rstd': rstd, 'slope': 0.1}
    for affine in tf:
        vary('trilinear_devoxelize_bnact_forward', {**devox, 'gamma': gam if affine else None, 'beta': bet if affine else None},
             {'is_training': tf, 'addend': (None, z(b, c, n)), 'se_scale': (None, z(b, c))})
    add('trilinear_devoxelize_bnact_forward', {**devox, 'is_training': True, 'gamma': gam, 'beta': bet, 'features': z(b, c, 7)},
        {'features': devox['features'], 'addend': z(b, c, m)}, {'features': devox['features'], 'se_scale': z(b, 3)})
    sums = {'x': x, 'gamma': gam, 'beta': bet, 'mean': mean, 'rstd': rstd, 'slope': 0.1}
    for method in ('bnact_partial_sums_raw', 'bnact_partial_sums'):
        add(method, {**sums, 'grad_y': gy}, {'grad_y': None}, {'grad_y': z(b, c + 1, s)[:, :c], 'gamma': None, 'beta': None})
    apply_ = {**sums, 'grad_y': gy, 'sum_gamma': z(c), 'sum_beta': z(c)}
    vary('bnact_backward_apply', apply_, {'training': tf, 'bc_mul': (None, z(b, c)), 'bc_add': (None, z(b, c))})
    add('bnact_backward_apply', {**apply_, 'training': True, 'gamma': None, 'beta': None, 'sum_gamma': None, 'sum_beta': None, 'amax_seg': 4},
        {'bc_mul': z(b, 3)}, {'bc_add': z(b, 3)})
    for affine in tf:
        vary('bnact_backward', {**sums, 'grad_y': gy, 'gamma': gam if affine else None, 'beta': bet if affine else None},
             {'training': tf, 'amax_seg': (0, 4), 'drop': (None, (seed, 0.5)), 'out_w': (None, z(c)), 'out_b': (None, z(c))})
    add('bnact_backward', {**sums, 'grad_y': z(b, c + 1, s)[:, :c], 'training': True, 'out_w': z(c + 1)})
    hidden, separt = 2, z(c, b, 3, 2)
    se = {'part': separt, 'gamma': gam, 'beta': bet, 'w1': z(hidden, c), 'w2': z(c, hidden), 's3': s}
    add('se_excite_forward', se, {'gamma': None, 'beta': None}, {'w2': z(c, 3)})
    add('se_excite_backward', {**se, 'a_sum': z(b, c), 'ax_sum': z(b, c), 'squeezed': z(b, c), 'hidden': z(b, hidden), 'excite': z(b, c)},
        {'gamma': None, 'beta': None})
    # concatenation, dense head, pooling
    bc, sl = z(b, 2, 1).expand(b, 2, n), z(b, 5, n)[:, 1:3]
    table = types.SimpleNamespace(dtype=I32, is_cuda=True, data_ptr=z(3, dtype=I32).data_ptr)      # (an amax buffer "on the device")
    for amax_global in tf:
        vary('concat_points', {'tensors': [z(b, 3, n), bc, sl]}, {'want_amax': tf, 'want_global': tf, 'out': (None, z(b, 7, n))}, amax_global=amax_global)
    add('concat_points', {'tensors': [sl, z(b, 3, n)], 'in_place': {0: table}}, {'want_global': False}, {'tensors': [z(1, 2, n), z(1, 5, n)[:, 1:3]]},
        {'tensors': [z(1, 5, n)[:, 1:3]], 'in_place': {0: table}}, {'tensors': []}, {'tensors': [z(b, 3, n), z(b, 3, m)]},
        {'tensors': [z(b, 4)[:, ::2].unsqueeze(-1).expand(b, 2, n)]}, {'tensors': [z(b, n, 3).transpose(1, 2)]}, {'out': z(b, 4, n)},
        {'want_amax': False}, {'in_place': {0: None}})
    add('dense_bn_relu_supported', {'rows': 4, 'cin': 3, 'cout': 5})
    dense = {'x': z(4, 3), 'weight': z(5, 3), 'bias': z(5), 'gamma': z(5), 'beta': z(5), 'running_mean': z(5), 'running_var': z(5),
             'counter': z(1, dtype=I64), 'eps': 1e-5, 'momentum': 0.1}
    add('dense_bn_relu_forward', dense, {k: None for k in ('bias', 'gamma', 'beta', 'running_mean', 'running_var', 'counter')}, {'weight': z(5, 2)})
    dense_bwd = {'x': z(4, 3), 'grad_y': z(4, 5), 'z': z(4, 5), 'mean': z(5), 'rstd': z(5), 'gamma': z(5), 'beta': z(5)}
    add('dense_bn_relu_backward', dense_bwd, {'gamma': None, 'beta': None, 'out_w': z(5, 3), 'out_b': z(5), 'out_gamma': z(5), 'out_beta': z(5)},
        {'out_gamma': z(4)})
    add('neighbor_max_supported', {'k': 2})
    add('neighbor_max_forward', {'x': z(b, 3, m, u)})
    add('neighbor_max_backward', {'grad_out': z(b, 3, m), 'winners': z(b, 3, m, dtype=U8), 'k': u}, {'winners': z(b, 3, m, dtype=I32)})
    add('row_argmax', {'x': z(b, 3, 8)}, {'with_values': True}, {'x': z(b, 3, 5)})
    # the Frustum loss and the evaluation kernels
    nh, ns = 3, 2
    loss = {'center': z(b, 3), 'center_reg': z(b, 3), 'heading_scores': z(b, nh), 'size_scores': z(b, ns), 'hrn': z(b, nh), 'srn': z(b, ns, 3),
            'hr': z(b, nh), 'sr': z(b, ns, 3), 'heading_bin_id': z(b, dtype=I64), 'size_template_id': z(b, dtype=I64),
            'heading_residual': z(b), 'size_residual': z(b, 3), 'center_t': z(b, 3), 'templates': z(ns, 3), 'bin_centers': z(nh),
            'bin_width': 0.5, 'w_heading': 1.0, 'w_size': 2.0, 'w_corners': 3.0}
    add('frustum_box_loss', loss, {'center_t': z(b, 2)})
    tile = {'src': z(b, 10, 3), 'shuffled': z(b, 8, dtype=I64), 'num_points': 4, 'channels': 3, 'strides': (30, 3, 1), 'src_points': 10}
    add('eval_tile', tile, {'shuffled': z(b, 8, dtype=I32)}, {'num_points': 3}, {'strides': (100, 3, 1)})
    logits = z(b, 4, n)
    add('vote_confidence', {'logits': logits}, {'class_range': (1, 3)}, {'class_range': z(b, 2, dtype=I32)}, {'logits': z(b, n)},
        {'class_range': z(3, 2, dtype=I32)}, {'class_range': (3, 1)})
    vote = {'conf': z(b, n), 'pred': z(b, n, dtype=I32), 'shuffled': z(b, n, dtype=I64), 'scene_conf': z(7), 'scene_pred': z(7, dtype=I64),
            'keys': z(7, dtype=I64)}
    add('vote_merge', vote, {'mapping': z(b, 6, dtype=I64)}, {'shuffled': z(b, n, dtype=I32)}, {'scene_pred': z(7, dtype=I32)},
        {'keys': z(7, dtype=I32)}, {'pred': z(b, m, dtype=I32)}, {'keys': z(6, dtype=I64)}, {'mapping': z(1, 6, dtype=I64)})
    counts = {'gt': z(9, dtype=I64), 'pred': z(9, dtype=I64), 'num_classes': 3}
    add('seg_counts', counts, {'counts': z(3, 3, dtype=I64), 'wrap_negative': False}, {'gt': z(9, dtype=I32)}, {'pred': z(9, dtype=I32)},
        {'pred': z(8, dtype=I64)}, {'counts': z(3, 2, dtype=I64)})
    meter = {'logits': logits, 'targets': z(b, n, dtype=I64)}
    parts = {**meter, 'part_ranges': z(3, 2, dtype=I32), 'max_parts': 2, 'rows': z(6, 3, 2, dtype=I32)}
    add('seg_meter_update', {**meter, 'counts': z(14, dtype=I64)}, {'targets': z(b, m, dtype=I64)}, {'counts': None})
    add('seg_meter_update', parts, {'row_cursor': z(1, dtype=I64)}, {'part_ranges': z(3, 3, dtype=I32)}, {'rows': z(6, 2, 2, dtype=I32)},
        {'row_cursor': z(2, dtype=I64)})
    heads = (z(b, 3), z(b, nh), z(b, nh), z(b, ns), z(b, ns, 3))
    targets = (z(b, 3), z(b, dtype=I64), z(b), z(b, dtype=I64), z(b, 3), z(b, dtype=I64))
    fm = {'outputs': heads, 'targets': targets, 'bin_centers': z(nh), 'size_templates': z(ns, 3), 'class_ids': z(2, dtype=I64),
          'thresholds': z(2, dtype=F64), 'sums': z(2, dtype=F64), 'counts': z(7, dtype=I64)}
    swap = lambda seq, i, v: tuple(v if j == i else t for j, t in enumerate(seq))
    add('frustum_meter_update', fm, {'outputs': swap(heads, 2, z(b, 2))}, {'bin_centers': z(2)},
        *({'targets': swap(targets, i, z(b, dtype=I32))} for i in (1, 3, 5)), {'class_ids': z(2, dtype=I32)}, {'counts': z(7, dtype=I32)},
        {'targets': swap(targets, 0, z(b, 2))}, {'thresholds': z(2)})
    add('frustum_meter_accuracy', {'mask_logits': z(b, 2, n), 'mask_targets': z(b, n, dtype=I64), 'counts': z(7, dtype=I64)},
        {'mask_targets': z(b, m, dtype=I64)}, {'counts': z(7, dtype=I32)})
    add('box_iou_3d', {'corners_1': z(b, 3, 8), 'corners_t': z(b, 3, 8)}, {'corners_t': z(b, 3, 7)})
    iou = {'boxes': z(3, 5), 'query_boxes': z(2, 5)}
    add('rotate_iou', iou, {'criterion': 1, 'boxes_3d': z(3, 7, dtype=F64), 'query_boxes_3d': z(2, 7, dtype=F64), 'z_axis': 2, 'z_center': 0.5},
        {'boxes': z(3, 4)}, {'boxes_3d': z(3, 6, dtype=F64), 'query_boxes_3d': z(2, 7, dtype=F64)},
        {'boxes_3d': z(3, 7, dtype=F64), 'query_boxes_3d': z(2, 7)})
    pred = {'heads': heads, 'bin_centers': z(nh), 'size_templates': z(ns, 3), 'rotation_angle': z(b, dtype=F64), 'rgb_score': z(b, dtype=F64),
            'table': z(4, 8, dtype=F64), 'step': 1}
    add('frustum_predictions', pred, {'rotation_angle': z(b)}, {'rgb_score': z(b)}, {'table': z(4, 8)}, {'table': z(4, 7, dtype=F64)}, {'step': 3})
    # the KITTI AP evaluation
    add('image_box_overlap', {'boxes': z(3, 4, dtype=F64), 'query_boxes': z(2, 4, dtype=F64)}, {'criterion': 0}, {'boxes': z(3, 4)})
    for p in (_packed((['Car', 'DontCare'], ['Pedestrian']), (['Car'], ['Car', 'Cyclist'])), _packed((['Car'],), (['Car', 'Car'],))):
        ml, k = (2, 3), 2
        vary('kitti_ap_overlaps', {'p': p}, {'metric': (0, 1, 2, 3)})
        add('kitti_ap_overlaps', {'p': p, 'metric': 2, 'z_axis': 2, 'z_center': 0.5})
        add('kitti_ap_clean', {'p': p, 'classes': z(ml[0], dtype=I32), 'difficulties': z(ml[1], dtype=I32)}, {'classes': z(ml[0], dtype=I64)})
        clean = (z(*ml, p.G, dtype=I8), z(*ml, p.D, dtype=I8), z(p.dontcares, dtype=I32), z(*ml, dtype=I64))
        ap = {'p': p, 'overlaps': z(p.pairs, dtype=F64), 'clean': clean, 'min_overlaps': z(k, ml[0], dtype=F64)}
        add('kitti_ap_match', ap, {'overlaps': z(p.pairs)}, {'min_overlaps': z(k, 3, dtype=F64)})
        add('kitti_ap_thresholds', {'tp_scores': z(*ml, k, p.G, dtype=F64), 'num_valid_gt': clean[3]}, {'num_valid_gt': z(5, dtype=I64)})
        stats = {**ap, 'thresholds': z(*ml, k, 41, dtype=F64), 'counts': z(*ml, k, dtype=I32)}
        vary('kitti_ap_stats', stats, {'metric': (0, 2), 'compute_aos': tf})
        add('kitti_ap_stats', {**stats, 'metric': 0, 'compute_aos': True, 'counts': z(*ml, k, dtype=I64)})
    # the weight bank's batched refresh
    add(_bank_refresh, {'kind': 'conv', 'nsplit': 2, 'shape': (6, 3, 3, 3, 3)}, {'kind': 'pw', 'nsplit': 1, 'shape': (6, 3, 1)})
    return out


# ---- the lib log: recording -------------------------------------------------------------------------------------------------------
def _names(prefix, v, into):
    """Every tensor reachable from an argument, by the name a reader would give it."""
    if isinstance(v, torch.Tensor):
        into[prefix] = v
    elif isinstance(v, (list, tuple)):
        for i, t in enumerate(v):
            _names(f'{prefix}[{i}]', t, into)
    elif isinstance(v, dict):
        for k, t in v.items():
            _names(f'{prefix}[{k}]', t, into)
    elif hasattr(v, '_boxes_3d'):               # kitti._Packed: its arrays and the box views it hands out
        for k, t in vars(v).items():
            _names(f'{prefix}.{k}', t, into)
    elif hasattr(v, '__slots__'):               # a VoxelPlan
        for k in v.__slots__:
            _names(f'{prefix}.{k}', getattr(v, k), into)
    return into


def _outcome(res):
    if isinstance(res, torch.Tensor):
        return [list(res.shape), str(res.dtype)]
    if isinstance(res, (tuple, list)):
        return [_outcome(t) for t in res]
    if hasattr(res, '__slots__'):
        return {k: _outcome(getattr(res, k)) for k in res.__slots__}
    return res


def lib_log():
    methods, launches, outcomes, cases = host.Table(), host.Table(), host.Table(), []
    with host.proxied_backend() as (be, rec):
        for settings, method, kwargs in lib_cases():
            be.seam_plan_memo, be.amax_global, be.fold_finalize = True, False, False
            for name, value in settings.items():
                setattr(be, name, value)
            named = {}
            for name, v in kwargs.items():
                _names(name, v, named)
            rec.begin(named)
            try:
                if not isinstance(method, str):
                    outcome = _outcome(method(be, **kwargs))
                elif '*' in kwargs:               # batch_launch(entry, ref, *args)
                    outcome = _outcome(getattr(be, method)(kwargs['entry'], kwargs['ref'], *kwargs['*']))
                else:
                    outcome = _outcome(getattr(be, method)(**kwargs))
            except RuntimeError as e:
                outcome = 'RuntimeError: ' + str(e)
            label = method if isinstance(method, str) else method.__name__
            cases.append([methods.index([label, settings]), [launches.index(call) for call in rec.calls], outcomes.index(outcome)])
    return {'methods': methods.rows, 'launches': launches.rows, 'outcomes': outcomes.rows, 'cases': cases}


# ---- the node log: a recording stand-in for the BatchNorm family ------------------------------------------------------------------
def _desc(v):
    if isinstance(v, torch.Tensor):
        return list(v.shape)
    if isinstance(v, (tuple, list)):
        return [_desc(t) for t in v]
    return v if v is None or isinstance(v, (bool, int, float)) else str(v)


def recorded(fn):
    """Note the call (name, positional arguments, keywords by name) on `self.log`, then run the torch implementation."""
    names = list(inspect.signature(fn).parameters)[1:]

    def wrapper(self, *args, **kwargs):
        self.log.append([fn.__name__, [_desc(v) for v in args], {n: _desc(v) for n, v in kwargs.items()}])
        assert len(args) <= len(names) and set(kwargs) <= set(names)
        return fn(self, *args, **kwargs)
    wrapper.__name__, wrapper.__wrapped__ = fn.__name__, fn
    return wrapper


def _act(t, slope):
    return torch.where(t > 0, t, t * slope)


def _dact(t, slope):
    return torch.where(t > 0, torch.ones_like(t), torch.full_like(t, slope))


def _xhat_z(x3, g, b, mean, rstd):
    xhat = (x3 - mean.view(1, -1, 1)) * rstd.view(1, -1, 1)
    gam = g if g is not None else torch.ones_like(mean)
    bet = b if b is not None else torch.zeros_like(mean)
    return xhat, xhat * gam.view(1, -1, 1) + bet.view(1, -1, 1), gam


def _track(rm, rv, mean, var, count, momentum):
    if rm is not None:
        rm.mul_(1 - momentum).add_(momentum * mean)
        rv.mul_(1 - momentum).add_(momentum * var * count / (count - 1))


class RecordingBNBackend:
    """torch stand-ins for what the three BatchNorm nodes ask of a backend, recording every call."""
    BNACT_AMAX_MAX_SEG = PW_AMAX_SEG = 256
    has_bnact = has_bnact_rowmax = has_bnact_dropout = has_devox_bnact = has_bnact_split_bwd = True
    SLICES = 2

    def __init__(self, oracle, has_se_excite):
        self.log, self.o, self.has_se_excite, self.keep = [], oracle, has_se_excite, None

    def _keep(self, drop, like):
        seed, p = drop
        g = torch.Generator().manual_seed(int(seed) & 0x7fffffff)
        self.keep = (torch.rand(like.numel(), generator=g) >= p).view_as(like).to(like.dtype) / (1.0 - p)
        return self.keep

    @staticmethod
    def _words(b, n, seg):
        return 1 + b * ((n + seg - 1) // seg)

    @recorded
    def amax_buffer(self, b, n, seg, device):
        return torch.zeros(self._words(b, n, seg), dtype=I32)

    @recorded
    def amax_and_row_keys(self, b, c, n, seg, device):
        words = self._words(b, n, seg)
        off = (words + 1) // 2 * 2
        whole = torch.ones(off + 2 * b * c, dtype=I32)          # (bn_finalize zeroes it)
        return whole, whole[:words], whole[off:]

    @recorded
    def bn_finalize(self, part, count, running_mean, running_var, momentum, eps, shift=None, zero_word=None, counter=None):
        sums = part.double().sum(dim=1) / count
        var = (sums[:, 1] - sums[:, 0] ** 2).float()
        mean = sums[:, 0].float() + (shift if shift is not None else 0.0)
        _track(running_mean, running_var, mean, var, count, momentum)
        if zero_word is not None:
            zero_word.zero_()
        if counter is not None:
            counter.add_(1)
        return mean, torch.rsqrt(var + eps)

    @recorded
    def bn_stats(self, x, running_mean, running_var, momentum, eps):
        mean, var = x.mean(dim=(0, 2)), x.var(dim=(0, 2), unbiased=False)
        _track(running_mean, running_var, mean, var, x.shape[0] * x.shape[2], momentum)
        return mean, torch.rsqrt(var + eps)

    @recorded
    def bnact_forward(self, x, gamma, beta, running_mean, running_var, training, momentum, eps, slope, stats=None, amax_seg=0, y_amax=None,
                      drop=None):
        if stats is not None:
            mean, rstd = stats
        elif training:
            mean, rstd = RecordingBNBackend.bn_stats.__wrapped__(self, x, running_mean, running_var, momentum, eps)
        else:
            mean, rstd = running_mean.clone(), torch.rsqrt(running_var + eps)
        y = _act(_xhat_z(x, gamma, beta, mean, rstd)[1], slope)
        if drop:
            y = y * self._keep(drop, y)
        if amax_seg:
            assert y_amax is None or not y_amax.any()
            return y, mean, rstd, y_amax if y_amax is not None else torch.zeros(self._words(x.shape[0], x.shape[2], amax_seg), dtype=I32)
        return y, mean, rstd

    @recorded
    def bnact_apply_rowmax(self, x, gamma, beta, mean, rstd, slope, amax_seg, y_amax, row_keys, out=None):
        assert not y_amax.any() and not row_keys.any()
        y = _act(_xhat_z(x, gamma, beta, mean, rstd)[1], slope)
        values, winners = y.max(dim=-1)
        return y, winners, values

    def _reduce(self, x, grad_y, gamma, beta, mean, rstd, slope):
        xhat, zz, _ = _xhat_z(x, gamma, beta, mean, rstd)
        d = _dact(zz, slope) * (grad_y if grad_y is not None else 1.0)
        return d, d * xhat

    @recorded
    def bnact_partial_sums(self, x, grad_y, gamma, beta, mean, rstd, slope):
        d, dx = self._reduce(x, grad_y, gamma, beta, mean, rstd, slope)
        return d.sum(dim=2), dx.sum(dim=2)

    @recorded
    def bnact_partial_sums_raw(self, x, grad_y, gamma, beta, mean, rstd, slope):
        b, c, s = x.shape
        halves = [t.reshape(b, c, self.SLICES, s // self.SLICES).sum(dim=3) for t in self._reduce(x, grad_y, gamma, beta, mean, rstd, slope)]
        return torch.stack(halves, dim=-1).permute(1, 0, 2, 3).contiguous()          # (C, B, slices, 2)

    @staticmethod
    def _pair(part):
        sums = part.sum(dim=2)
        return sums[..., 0].t(), sums[..., 1].t()

    @recorded
    def se_excite_forward(self, part, gamma, beta, w1, w2, s3):
        a_sum, ax_sum = self._pair(part)
        gam = gamma if gamma is not None else 1.0
        bet = beta if beta is not None else 0.0
        squeezed = (gam * ax_sum + bet * a_sum) / s3
        hidden = torch.relu(squeezed @ w1.t())
        return a_sum, ax_sum, squeezed, hidden, torch.sigmoid(hidden @ w2.t())

    @recorded
    def se_excite_backward(self, part, a_sum, ax_sum, gamma, beta, squeezed, hidden, excite, w1, w2, s3):
        p_sum, q_sum = self._pair(part)
        gam = gamma if gamma is not None else 1.0
        bet = beta if beta is not None else 0.0
        g_pre2 = (gam * q_sum + bet * p_sum) * excite * (1.0 - excite)
        g_pre1 = (g_pre2 @ w2) * (hidden > 0)
        g_mean = (g_pre1 @ w1) / s3
        return (g_pre1.t() @ squeezed, g_pre2.t() @ hidden, g_mean, (excite * p_sum + g_mean * a_sum).sum(dim=0),
                (excite * q_sum + g_mean * ax_sum).sum(dim=0))

    def _grad_x(self, x, g_in, gamma, beta, mean, rstd, sum_gamma, sum_beta, slope, training):
        xhat, zz, gam = _xhat_z(x, gamma, beta, mean, rstd)
        gp = g_in * _dact(zz, slope)
        if sum_gamma is None:
            sum_gamma, sum_beta = (gp * xhat).sum(dim=(0, 2)), gp.sum(dim=(0, 2))
        inv = 1.0 / (x.shape[0] * x.shape[2])
        if training:
            gp = gp - (sum_beta * inv).view(1, -1, 1) - xhat * (sum_gamma * inv).view(1, -1, 1)
        return (gam * rstd).view(1, -1, 1) * gp, sum_gamma, sum_beta

    @recorded
    def bnact_backward_apply(self, x, grad_y, gamma, beta, mean, rstd, sum_gamma, sum_beta, slope, training, bc_mul=None, bc_add=None,
                             amax_seg=256):
        g_in = grad_y * (bc_mul.unsqueeze(-1) if bc_mul is not None else 1.0) + (bc_add.unsqueeze(-1) if bc_add is not None else 0.0)
        gx = self._grad_x(x, g_in, gamma, beta, mean, rstd, sum_gamma, sum_beta, slope, training)[0]
        return gx, torch.zeros(self._words(x.shape[0], x.shape[2], amax_seg), dtype=I32)

    @recorded
    def bnact_backward(self, x, grad_y, gamma, beta, mean, rstd, slope, training, amax_seg=0, drop=None, out_w=None, out_b=None):
        g_in = grad_y * self.keep if drop else grad_y
        out = self._grad_x(x, g_in, gamma, beta, mean, rstd, None, None, slope, training)
        return out + (torch.zeros(self._words(x.shape[0], x.shape[2], amax_seg), dtype=I32),) if amax_seg else out

    @recorded
    def trilinear_devoxelize_bnact_forward(self, r, is_training, coords, features, gamma, beta, mean, rstd, slope, addend=None, se_scale=None):
        a = _act(_xhat_z(features, gamma, beta, mean, rstd)[1], slope)
        if se_scale is not None:
            a = a * se_scale.unsqueeze(-1)
        out, inds, wgts = self.o.trilinear_devoxelize_forward(r, is_training, coords, a.contiguous())
        return [out + addend if addend is not None else out, inds, wgts]

    @recorded
    def trilinear_devoxelize_backward(self, grad_y, indices, weights, r):
        return self.o.trilinear_devoxelize_backward(grad_y.contiguous(), indices, weights, r)


# ---- the node log: the cases ------------------------------------------------------------------------------------------------------
NODES = ('bnact', 'devox', 'se_devox')
B, C, R, N, WIDE, SLOPE, EPS, DROP_P = 2, 4, 4, 8, 256, 0.1, 1e-4, 0.25


def node_cases():
    """The product of the axes, least important innermost, without what the wrappers cannot be asked or reject: an addend on the plain
    node, dropout on the two devoxelize nodes (neither has the parameter) and dropout without amax segments (an assertion)."""
    tf = (False, True)
    for case in itertools.product(NODES, tf, tf, tf, tf, tf, tf, tf, tf, tf, tf):
        node, training, part, seg, row_max, drop, affine, momentum, counter, addend, fused_se = case
        if (drop and (node != 'bnact' or not seg)) or (addend and node == 'bnact'):
            continue
        yield case


class _DeviceCounter(torch.Tensor):
    """A num_batches_tracked that says it lives on the device: what _bn_mode asks before it hands the counter to bn_finalize."""
    is_cuda = True


_DATA = {}


def _data():
    if not _DATA:
        g = torch.Generator().manual_seed(1588147245)
        rnd = lambda *s: torch.randn(*s, generator=g)
        _DATA.update(points=rnd(B, C, N), wide=rnd(B, C, WIDE), grid=rnd(B, C, R, R, R), coords=torch.rand(B, 3, N, generator=g) * (R - 1),
                     addend=rnd(B, C, N), gy=rnd(B, C, N), gy_wide=rnd(B, C, WIDE), gamma=torch.rand(C, generator=g) + 0.5, beta=rnd(C) * 0.5,
                     shift=rnd(C) * 0.3, rm=rnd(C) * 0.1, rv=torch.rand(C, generator=g) + 0.5, fc1=rnd(2, C) * 0.5, fc2=rnd(C, 2) * 0.5)
    return _DATA


def _module(cls, affine, momentum, training, d):
    bn = cls(C, eps=EPS, momentum=0.1 if momentum else None, affine=affine)
    with torch.no_grad():
        if affine:
            bn.weight.copy_(d['gamma']); bn.bias.copy_(d['beta'])
        bn.running_mean.copy_(d['rm']); bn.running_var.copy_(d['rv'])
    return bn.train(training)


def _stats_part(x, shift):
    """What a convolution epilogue leaves: (C, 2, 2) sums of (x - shift) and its square over the two halves of the positions."""
    x3 = x.reshape(B, C, -1) - shift.view(1, -1, 1)
    halves = x3.reshape(B, C, 2, -1).permute(1, 2, 0, 3).reshape(C, 2, -1)
    return torch.stack([halves.sum(dim=2), halves.square().sum(dim=2)], dim=-1)


def run_bn_case(case, oracle):
    """One forward (+ backward where the output is differentiable) of a node on the stand-in and of the plain modules
    -> (call log, [(name, got, want)])."""
    from pvcnn_amd.modules import SE3d
    from pvcnn_amd.modules import functional as PF
    from pvcnn_amd.modules.functional import bnact
    node, training, part, seg, row_max, drop, affine, momentum, counter, addend, fused_se = case
    d = _data()
    plain = node == 'bnact'
    wide = plain and row_max
    x0 = (d['wide'] if wide else d['points']) if plain else d['grid']
    gy = d['gy_wide'] if wide else d['gy']
    cls = nn.BatchNorm1d if plain else nn.BatchNorm3d
    bn, ref = _module(cls, affine, momentum, training, d), _module(cls, affine, momentum, training, d)
    if counter:
        bn.num_batches_tracked = torch.Tensor._make_subclass(_DeviceCounter, bn.num_batches_tracked)
    se = SE3d(C, reduction=2)
    with torch.no_grad():
        se.fc[0].weight.copy_(d['fc1']); se.fc[2].weight.copy_(d['fc2'])
    fake = RecordingBNBackend(oracle, fused_se)
    x, xr = x0.clone().requires_grad_(), x0.clone().requires_grad_()
    add, addr = (d['addend'].clone().requires_grad_(), d['addend'].clone().requires_grad_()) if addend else (None, None)
    stats = (_stats_part(x0, d['shift']), d['shift']) if part else None
    amax_seg = (64 if wide else 4) if seg else 0
    saved, bnact._amax_seg_for = bnact._amax_seg_for, lambda shape, is_cuda: amax_seg
    try:
        with host.seam(fake), (bnact.emit_row_max(bn) if row_max else contextlib.nullcontext()):
            if plain:
                y = bnact.batch_norm_act(x, bn, SLOPE, stats_part=stats, drop_p=DROP_P if drop else 0.0)
            elif node == 'devox':
                y = bnact.batch_norm_act_devoxelize(x, d['coords'], bn, SLOPE, R, training, stats_part=stats, addend=add)
            else:
                y = bnact.batch_norm_act_se_devoxelize(x, d['coords'], bn, SLOPE, se, R, training, stats_part=stats, addend=add)
            if plain or training:                   # (the devoxelization is not differentiable in eval mode, like the reference's)
                y.backward(gy)
    finally:
        bnact._amax_seg_for = saved
    got_se = [se.fc[0].weight.grad, se.fc[2].weight.grad]
    se.zero_grad()
    with host.seam(oracle):
        yr = nn.functional.leaky_relu(ref(xr), SLOPE)
        if plain and fake.keep is not None:
            yr = yr * fake.keep
        if node == 'se_devox':
            yr = se(yr)
        if not plain:
            yr = PF.trilinear_devoxelize(yr, d['coords'], R, training)
            yr = yr + addr if addend else yr
        if plain or training:
            yr.backward(gy)
    pairs = [('y', y.detach(), yr.detach()), ('grad x', x.grad, xr.grad), ('running_mean', bn.running_mean, ref.running_mean),
             ('running_var', bn.running_var, ref.running_var),
             ('num_batches_tracked', bn.num_batches_tracked.as_subclass(torch.Tensor), ref.num_batches_tracked)]
    if affine:
        pairs += [('grad gamma', bn.weight.grad, ref.weight.grad), ('grad beta', bn.bias.grad, ref.bias.grad)]
    if addend:
        pairs.append(('grad addend', add.grad, addr.grad))
    if node == 'se_devox':
        pairs += [('grad fc1', got_se[0], se.fc[0].weight.grad), ('grad fc2', got_se[1], se.fc[2].weight.grad)]
    if hasattr(y, '_pvcnn_row_max'):
        values, winners = y.detach().max(dim=-1)
        pairs += [('row-max winners', y._pvcnn_row_max[0], winners), ('row-max values', y._pvcnn_row_max[1], values)]
    return fake.log, pairs


def node_log(oracle):
    entries, logs, cases, results = host.Table(), host.Table(), [], []
    threads = torch.get_num_threads()
    torch.set_num_threads(1)            # (tensors this small: waking the thread pool costs a hundred times the arithmetic)
    try:
        for case in node_cases():
            log, pairs = run_bn_case(case, oracle)
            cases.append(logs.index([entries.index(e) for e in log]))
            results.append((case, pairs))
    finally:
        torch.set_num_threads(threads)
    return {'entries': entries.rows, 'logs': logs.rows, 'cases': host.run_lengths(cases)}, results


def the_oracle():
    from oracle import oracle_backend
    oracle_backend.build()
    return oracle_backend.OracleBackend()


def record():
    return {**{'node ' + k: v for k, v in node_log(the_oracle())[0].items()}, **{'lib ' + k: v for k, v in lib_log().items()}}


# ---- the tests --------------------------------------------------------------------------------------------------------------------
def _golden(section):
    import json
    with open(GOLDEN_PATH) as fh:
        return {k[len(section) + 1:]: v for k, v in json.load(fh).items() if k.startswith(section + ' ')}


def test_the_backend_sends_the_library_what_the_golden_records():
    import ast
    from pvcnn_amd.modules.functional import backend as mod
    got, want = host._lib_logs(lib_log()), host._lib_logs(_golden('lib'))
    assert len(got) == len(want) == len(lib_cases())
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (i, a, b)
    # every shape message of the methods pinned here is tripped by some case (those of the Conv3d / 1x1 methods: product_calls.json)
    texts = [log[-1] for log in got if isinstance(log[-1], str)]
    product = ('conv3d_', 'pwconv_', '_amax_seg', '_grad_out')
    cls = next(n for n in ast.parse(inspect.getsource(mod)).body if isinstance(n, ast.ClassDef) and n.name == 'HipBackend')
    for fn in (n for n in cls.body if isinstance(n, ast.FunctionDef) and not n.name.startswith(product)):
        for call in (n for n in ast.walk(fn) if isinstance(n, ast.Call) and getattr(n.func, 'id', '') == '_shape'):
            msg = call.args[1]
            pieces = [v.value for v in (msg.values if isinstance(msg, ast.JoinedStr) else [msg]) if isinstance(v, ast.Constant)]
            if isinstance(msg, ast.BinOp):          # _ap_typed: an f-string plus an optional tail
                pieces = [v.value for v in msg.left.values if isinstance(v, ast.Constant)]
            assert pieces and any(all(piece in t for piece in pieces) for t in texts), (fn.name, pieces)
    assert any('gradient destination' in t for t in texts)


def test_the_batchnorm_nodes_ask_the_backend_for_what_the_golden_records_and_compute_the_plain_modules(oracle):
    section, results = node_log(oracle)
    got, want = host._node_logs(section), host._node_logs(_golden('node'))
    cases = list(node_cases())
    assert len(got) == len(want) == len(cases) == 384 + 512 + 512
    for i, (case, a, b) in enumerate(zip(cases, got, want)):
        assert a == b, (i, case, a, b)
    for case, pairs in results:
        for name, a, b in pairs:
            if b is None:
                assert a is None, (case, name)
            else:
                assert a is not None and torch.allclose(a.to(b.dtype), b, rtol=1e-4, atol=1e-4), (case, name, a, b)


def test_the_launch_helper_converts_its_arguments_appends_the_stream_and_raises_with_the_label(monkeypatch):
    from pvcnn_amd import _lib
    from pvcnn_amd.modules.functional import backend as mod
    x, empty, table = torch.zeros(3), torch.zeros(0), (ctypes.c_int * 2)(4, 5)
    with host.proxied_backend() as (be, rec):
        rec.begin({'x': x, 'empty': empty})
        mod._run(be.lib.pvcnn_some_entry, 'some label', x, x, empty, None, 7, 0.5, be._TABLE_ONLY, table)
        assert rec.calls == [['pvcnn_some_entry', ['argument x', 'NULL', 'NULL', 7, 0.5, 'PVCNN_TABLE_ONLY', [4, 5], 'NULL'], 'some label']]
    # as the entry sees them: tensors and None as pointers, the rest as the very objects, the stream last
    seen, stream = [], ctypes.c_void_p(0x5157)

    class Launch(host._NullLaunch):
        def __enter__(self):
            return stream
    monkeypatch.setattr(mod, '_Launch', Launch)
    sentinel, number = mod.HipBackend._TABLE_ONLY, 7.25
    mod._run(lambda *args: seen.append(args) or 0, 'label', x, x, empty, None, number, sentinel, table)
    (args,) = seen
    assert [type(a) for a in args[:3]] == [ctypes.c_void_p] * 3 and [a.value for a in args[:3]] == [x.data_ptr(), None, None]
    assert args[3] is number and args[4] is sentinel and args[5] is table and args[6] is stream and len(args) == 7
    # a host-side argument check of the real library (B = 0: rejected before any HIP call) surfaces with the label and its message
    out = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(_lib.PvcnnHipError) as err:
        mod._run(_lib.load().pvcnn_absmax_tiles, 'the label of this call', x, x, 0, 1, 3, 4, out, None)
    message = _lib.load().pvcnn_last_error_string().decode()
    assert message and str(err.value).startswith('the label of this call failed (code ') and str(err.value).endswith(message)
