"""Record tests/golden/weight_images.json: per case of tests/test_gpu_weight_images.py the size of the split-weight image and one
SHA-256 over the whole buffer (that module holds the cases and the closed-form weights; this script only writes the file).  Needs an
MI355X and a built libpvcnn_hip.so.

    python tests/golden/gen_weight_images_golden.py            # rewrite the golden from the checked-out code
    python tests/golden/gen_weight_images_golden.py --check    # exit 1 unless the file on disk is reproduced byte for byte

The file was recorded from the commit before csrc/weight_image.h (the per-kind writers of conv3d_bf16.hip and pointwise_bf16.hip) and
is reproduced byte for byte by this tree."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.dirname(HERE), REPO]      # tests/ (conftest, the test module) and the repository

import test_gpu_weight_images as t      # noqa: E402

if __name__ == '__main__':
    from pvcnn_amd.modules.functional.backend import HipBackend
    text = t.dumps(t.record(HipBackend()))
    if '--check' in sys.argv[1:]:
        same = open(t.GOLDEN_PATH).read() == text
        print('reproduced byte for byte' if same else 'DIFFERS from the file on disk')
        sys.exit(0 if same else 1)
    with open(t.GOLDEN_PATH, 'w') as fh:
        fh.write(text)
    print(f'{t.GOLDEN_PATH}: {len(text)} bytes, {len(t.CASES)} cases')
