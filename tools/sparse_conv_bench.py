"""The submanifold sparse 3x3x3 convolution (csrc/sparse.hip) against the dense Conv3d launches on the same data.

    python tools/sparse_conv_bench.py [--launches 50] [--rounds 3] [--batch 16] [--points 4096]

The method of tools/infer_bench.py: one process, every launch warmed up first, then `--rounds` rounds in which the variants ALTERNATE;
a round is `--launches` launches between two device events.  The occupancy is that of pvcnn_amd.workload's synthetic cfg2 input
(make_s3dis_batch, normalised coordinates as PVConv voxelizes them): 64 -> 64 channels at R = 32 and, for contrast, 128 -> 128 at
R = 16.  Compared, for forward, backward-data and backward-weight (+ bias):
  sparse  the rows of the active voxels (the weight image launch of forward / backward-data included, as the autograd node runs it)
  fp32    the dense fp32-MFMA launches (hip.conv3d_forward and its two backwards): the same arithmetic, on the zero-filled grid
  f16x2   the default dense launches, for information only
Also printed: the row count, the share of (tile, tap) products the skip leaves out, the time of the map, gather and scatter launches,
and whether every sparse forward round beats every dense fp32 round by more than the dense rounds' own spread.  One JSON line per
shape."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pvcnn_amd                                                        # noqa: E402,F401
import pvcnn_amd.modules.functional as F                                # noqa: E402
from pvcnn_amd import workload                                          # noqa: E402
from pvcnn_amd.modules import Voxelization                              # noqa: E402
from pvcnn_amd.modules.functional import backend as seam                # noqa: E402

SHAPES = [dict(resolution=32, channels=64), dict(resolution=16, channels=128)]


def timed(fn, launches):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(launches):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / launches * 1e3                    # microseconds per launch


def measure(variants, launches, rounds):
    """variants: name -> callable (or None) -> name -> [us per launch of every round]; the variants alternate inside a round."""
    live = {k: v for k, v in variants.items() if v is not None}
    for fn in live.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in live}
    for _ in range(rounds):
        for k, fn in live.items():
            out[k].append(round(timed(fn, launches), 2))
    return out


def optional(fn):
    """fn if it runs on this shape, else None (the f16x2 launches are information, not the subject)."""
    try:
        fn()
        torch.cuda.synchronize()
        return fn
    except Exception as e:                                              # noqa: BLE001
        print(f'# skipped: {e}', file=sys.stderr)
        return None


def bench_shape(coords, resolution, channels, launches, rounds):
    hip = seam._backend
    b, r, c = coords.shape[0], resolution, channels
    vox = Voxelization(r)
    _, vox_coords = vox.grid_coordinates(coords)
    cnt = hip.avg_voxelize_plan(vox_coords.contiguous(), r).cnt
    m = F.sparse_map(cnt, r, num_points=coords.shape[2])
    count = int(m.count)
    tiles = (m.nbr.view(m.cap // 64, 64, 27) >= 0).any(1)[:(count + 63) // 64]
    torch.manual_seed(1588147245)
    x = torch.randn((m.cap, c), device='cuda')
    gy = torch.randn((m.cap, c), device='cuda')
    w, bias = 0.1 * torch.randn((c, c, 3, 3, 3), device='cuda'), 0.1 * torch.randn((c,), device='cuda')
    xd, gyd = F.sparse_scatter(x, m).contiguous(), F.sparse_scatter(gy, m).contiguous()       # the same data, zero-filled
    res = {'resolution': r, 'batch': b, 'channels': c, 'voxels': b * r ** 3, 'cap': m.cap, 'rows': count,
           'occupancy': round(count / (b * r ** 3), 4), 'tile_tap_products_skipped': round(1.0 - tiles.float().mean().item(), 4),
           'launches_per_round': launches, 'rounds': rounds}
    res['forward_us'] = measure({
        'sparse': lambda: hip.sparse_conv3d_forward(x, hip.sparse_conv3d_weight_image(w), bias, m.nbr, m.count),
        'fp32': lambda: hip.conv3d_forward(xd, w, bias),
        'f16x2': optional(lambda: hip.conv3d_forward_split(xd, w, bias, 2))}, launches, rounds)
    res['backward_data_us'] = measure({
        'sparse': lambda: hip.sparse_conv3d_forward(gy, hip.sparse_conv3d_weight_image(w, True), None, m.nbr, m.count),
        'fp32': lambda: hip.conv3d_backward_data(gyd, w),
        'f16x2': optional(lambda: hip.conv3d_backward_data_split(gyd, w, 2))}, launches, rounds)
    res['backward_weight_us'] = measure({
        'sparse': lambda: hip.sparse_conv3d_backward_weight(x, gy, m.nbr, m.count),
        'fp32': lambda: hip.conv3d_backward_weight(xd, gyd, with_bias=True),
        'f16x2': optional(lambda: hip.conv3d_backward_weight_f16(xd, gyd, with_bias=True))}, launches, rounds)
    res['plumbing_us'] = measure({
        'map': lambda: hip.sparse_map(cnt, r, m.cap),
        'gather': lambda: hip.sparse_gather(xd.view(b, c, -1), m.voxel, m.count),
        'scatter': lambda: hip.sparse_scatter(x, m.index, m.count, b, r)}, launches, rounds)
    s, d = res['forward_us']['sparse'], res['forward_us']['fp32']
    res['dense_fp32_forward_spread_us'] = round(max(d) - min(d), 2)
    res['sparse_forward_faster_beyond_dense_spread'] = bool(min(d) - max(s) > max(d) - min(d))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--points', type=int, default=4096)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    feats, _ = workload.make_s3dis_batch(args.batch, args.points)
    coords = feats[:, :3, :].cuda().contiguous()
    for shape in SHAPES:
        print(json.dumps(bench_shape(coords, shape['resolution'], shape['channels'], args.launches, args.rounds)), flush=True)


if __name__ == '__main__':
    main()
