#!/usr/bin/env python3
"""Generate tests/golden/device_draws.pt: the complete outputs of device mode of every data kernel, for fixed seed words.

Producer: `record()` of tests/test_gpu_device_draws.py on the library built from commit 88ce5cd ("Frustum-KITTI batches from the
frames: a fresh 2-D box per sample"), the parent of the commit that moved the draw stream into csrc/philox.h -- on an MI355X, once.
The file pins what a seed means; it is regenerated only by a change that is meant to alter the stream, never to make a test pass.
tests/test_device_draws_host.py checks the recorded integer draws against the numpy stream (tests/draws_truth.py) without a GPU.
Run:  python tests/golden/gen_device_draws_golden.py [output path]     (needs the GPU and the built library)
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    from pvcnn_amd.modules.functional.backend import HipBackend
    import test_gpu_device_draws as cases
    path = sys.argv[1] if len(sys.argv) > 1 else cases.GOLDEN
    out = cases.record(HipBackend())
    again = cases.record(HipBackend())
    from test_gpu_frames import same
    assert sorted(out) == sorted(again) and all(same(out[k], again[k]) for k in out), 'two recordings differ'
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save(out, path)
    print(f'{path}: {len(out)} tensors, {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
