"""Record tests/golden/product_calls.json: what the Conv3d / 1x1 autograd nodes ask of a backend and what HipBackend's methods for the
two kinds send to the C library (tests/test_product_host.py holds the stand-ins and the cases; this script only writes the file).

    python tests/golden/gen_product_calls_golden.py            # rewrite the golden from the checked-out code
    python tests/golden/gen_product_calls_golden.py --check    # exit 1 unless the file on disk is reproduced byte for byte

Needs the built libpvcnn_hip.so (its host-only size queries are answered by the real library), no GPU."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]      # tests/ (conftest, the test module) and the repository

import test_product_host as t      # noqa: E402

if __name__ == '__main__':
    text = t.dumps(t.record())
    if '--check' in sys.argv[1:]:
        same = open(t.GOLDEN_PATH).read() == text
        print('reproduced byte for byte' if same else 'DIFFERS from the file on disk')
        sys.exit(0 if same else 1)
    with open(t.GOLDEN_PATH, 'w') as fh:
        fh.write(text)
    print(f'{t.GOLDEN_PATH}: {len(text)} bytes')
