#!/usr/bin/env python3
"""Generate tests/golden/routes.json: the host-only launch queries of libpvcnn_hip.so over a sweep of problem sizes, recorded from the
commit BEFORE the launch plans of csrc/route.h existed (ABI 16) -- what tests/test_route_host.py holds the plans to.

Recorded, each as a flat list in itertools.product order of the axes named next to it (the axes themselves are in the file):
  conv_stats_parts  pvcnn_conv3d_fwd_split_stats_parts(B, Co, R, nsplit)            over  B x C x R x nsplit
  conv_route        pvcnn_conv3d_fwd_split_route(B, Ci, Co, R, nsplit)              over  B x C x C x R x nsplit
  conv_wgrad_bytes  pvcnn_conv3d_bwd_weight_f16_workspace_bytes(B, Ci, Co, R)       over  B x C x C x R
  pw_stats_parts    pvcnn_pwconv_fwd_split_stats_parts(B, N)                        over  B x N
  pw_wgrad_bytes    pvcnn_pwconv_bwd_weight_f16_workspace_bytes(B, K, M, N)         over  B x C x C x N
The queries are pure functions of their integer arguments: no GPU is needed.  Run with the kernel switches (PVCNN_CONV_WIDE, ...) unset.

Run:  python tests/golden/gen_routes_golden.py [root of a built tree of that commit]     (rewrites routes.json)
"""
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

AXES = {
    'B': [1, 2, 3, 5, 8, 16, 20, 40],
    'C': [3, 9, 10, 13, 16, 20, 32, 48, 64, 96, 128, 256],
    'R': [4, 6, 8, 12, 16, 20, 32, 33],
    'nsplit': [1, 2, 3],
    'N': [1, 255, 256, 1024, 2048, 4096, 4100],
}


def sweep(fn, *axes):
    return [int(fn(*args)) for args in itertools.product(*(AXES[a] for a in axes))]


def main():
    root = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(HERE))
    sys.path.insert(0, root)
    from pvcnn_amd import _lib
    lib = _lib.load()
    out = {
        'abi_version': lib.pvcnn_version(),
        'axes': AXES,
        'conv_stats_parts': sweep(lib.pvcnn_conv3d_fwd_split_stats_parts, 'B', 'C', 'R', 'nsplit'),
        'conv_route': sweep(lib.pvcnn_conv3d_fwd_split_route, 'B', 'C', 'C', 'R', 'nsplit'),
        'conv_wgrad_bytes': sweep(lib.pvcnn_conv3d_bwd_weight_f16_workspace_bytes, 'B', 'C', 'C', 'R'),
        'pw_stats_parts': sweep(lib.pvcnn_pwconv_fwd_split_stats_parts, 'B', 'N'),
        'pw_wgrad_bytes': sweep(lib.pvcnn_pwconv_bwd_weight_f16_workspace_bytes, 'B', 'C', 'C', 'N'),
    }
    with open(os.path.join(HERE, 'routes.json'), 'w') as f:
        json.dump(out, f, separators=(',', ':'))
        f.write('\n')
    print({k: (len(v) if isinstance(v, list) else v) for k, v in out.items() if k != 'axes'})


if __name__ == '__main__':
    main()
