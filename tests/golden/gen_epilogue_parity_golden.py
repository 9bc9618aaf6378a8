"""Record tests/golden/epilogue_parity.json: one SHA-256 per case of tests/test_gpu_epilogue_parity.py over the bytes of what the
tile-per-workgroup Conv3d / 1x1 kernels return (that module holds the cases and the closed-form inputs; this script only writes the
file).  Needs an MI355X and a built libpvcnn_hip.so.

    python tests/golden/gen_epilogue_parity_golden.py            # rewrite the golden from the checked-out code
    python tests/golden/gen_epilogue_parity_golden.py --check    # exit 1 unless the file on disk is reproduced byte for byte

PVCNN_AMD_ROOT=<another checkout, built>: record with that checkout's `pvcnn_amd` package and library (the file was recorded that way,
from the commit before the shared epilogue, and reproduced byte for byte by this tree), the cases still being this tree's."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.dirname(HERE), REPO]      # tests/ (conftest, the test module) and the repository
if os.environ.get('PVCNN_AMD_ROOT'):
    import importlib.util
    spec = importlib.util.spec_from_file_location('pvcnn_amd', os.path.join(os.environ['PVCNN_AMD_ROOT'], 'pvcnn_amd', '__init__.py'),
                                                  submodule_search_locations=[os.path.join(os.environ['PVCNN_AMD_ROOT'], 'pvcnn_amd')])
    sys.modules['pvcnn_amd'] = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sys.modules['pvcnn_amd'])

import test_gpu_epilogue_parity as t      # noqa: E402

if __name__ == '__main__':
    from pvcnn_amd.modules.functional.backend import HipBackend
    be = HipBackend()
    for case in t.CASES:                   # the recording is of the launches the cases are listed for
        if 'ns' in case:
            assert t.route_of(be.lib, case) == t.expected_route(case), case['id']
    text = t.dumps(t.record(be))
    if '--check' in sys.argv[1:]:
        same = open(t.GOLDEN_PATH).read() == text
        print('reproduced byte for byte' if same else 'DIFFERS from the file on disk')
        sys.exit(0 if same else 1)
    with open(t.GOLDEN_PATH, 'w') as fh:
        fh.write(text)
    print(f'{t.GOLDEN_PATH}: {len(text)} bytes, {len(t.CASES)} cases')
