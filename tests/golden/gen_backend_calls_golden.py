"""Record tests/golden/backend_calls.json: what HipBackend sends to the C library outside the Conv3d / 1x1 products and what the three
BatchNorm autograd nodes ask of a backend (tests/test_backend_calls_host.py holds the cases and the stand-ins; this script only writes
the file).

    python tests/golden/gen_backend_calls_golden.py            # rewrite the golden from the checked-out code
    python tests/golden/gen_backend_calls_golden.py --check    # exit 1 unless the file on disk is reproduced byte for byte

PVCNN_AMD_ROOT=<another checkout, built>: record with that checkout's `pvcnn_amd` package (the file was recorded that way, from the
commit before the launch helper), the cases and the stand-ins still being this tree's.

Needs the built libpvcnn_hip.so (its host-only size queries are answered by the real library) and the CPU oracle, no GPU."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.dirname(HERE), REPO]      # tests/ (conftest, the test modules) and the repository
if os.environ.get('PVCNN_AMD_ROOT'):
    import importlib.util
    spec = importlib.util.spec_from_file_location('pvcnn_amd', os.path.join(os.environ['PVCNN_AMD_ROOT'], 'pvcnn_amd', '__init__.py'),
                                                  submodule_search_locations=[os.path.join(os.environ['PVCNN_AMD_ROOT'], 'pvcnn_amd')])
    sys.modules['pvcnn_amd'] = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sys.modules['pvcnn_amd'])

import test_backend_calls_host as t      # noqa: E402

if __name__ == '__main__':
    text = t.host.dumps(t.record())
    if '--check' in sys.argv[1:]:
        same = open(t.GOLDEN_PATH).read() == text
        print('reproduced byte for byte' if same else 'DIFFERS from the file on disk')
        sys.exit(0 if same else 1)
    with open(t.GOLDEN_PATH, 'w') as fh:
        fh.write(text)
    print(f'{t.GOLDEN_PATH}: {len(text)} bytes')
