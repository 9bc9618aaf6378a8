"""The tile-per-workgroup GEMM kernels share ONE epilogue (csrc/gemm_epilogue.h: unscale, BatchNorm partial sums of y - bias, bias,
masked store) and ONE product ladder (csrc/split16.h: split_products).  Their results are pinned BIT FOR BIT to what the kernels
computed when each carried its own copy of that text: tests/golden/epilogue_parity.json holds one SHA-256 per case over the bytes of
every tensor the call returns (y, and the statistics partials where asked), recorded by tests/golden/gen_epilogue_parity_golden.py
from the commit before the shared epilogue.

Inputs are closed-form integer arithmetic (a 32-bit hash of the element index, mapped to multiples of 2^-20 in [-2, 2)): no library
random numbers, so the file does not depend on a torch version.  The cases are small (B <= 2, <= 96 channels -- 1x1: <= 160 --, R <= 32,
N <= 600) and reach, by the launch plans of csrc/route.h -- asserted through pvcnn_conv3d_fwd_split_route / pvcnn_pwconv_fwd_split_route
for every case, on the CPU as well --, every instantiation those sizes can reach:
  Conv3d split   conv3d_igemm_bf16_kernel at tz = 8 / 16 / 32, vector and scalar staging, nsplit 1, 2, 3; its 32-row form (Co <= 32 at
                 16 < R <= 32, f16x2); conv3d_igemm_f16_pipe_kernel (f16x2, the (2, 4, 16) tile, Ci % 16 == 0);
  1x1 split      pw_gemm_bf16_kernel with 64- and 128-row tiles, vector and scalar loads, nsplit 1, 2, 3; pw_gemm_f16_pipe_kernel
                 (128 rows, vector loads, nsplit 1 and 2);
  fp32           conv3d_forward (conv3d_igemm_kernel: three tiles, vector and scalar staging) and pwconv_forward;
each with a row count that is no multiple of the tile (Co = 70, 33, 20), a reduction depth that is no multiple of 16 (Ci = 5), a grid
or point count that is no multiple of the tile (R = 4, 6, 10, 12, 20; N = 300, 301, 599), with and without bias, with and without
statistics.  (The wider tiles of the same kernels need B * tiles >= 256: the cross-kernel tests of test_gpu_conv3d.py,
test_gpu_conv_wide.py and test_gpu_pwconv.py run them.)  One R = 32 f16x2 case through the persistent wide kernel, whose epilogue is
its own, is the control."""
import hashlib
import json
import os

import pytest
import torch

from conftest import ROOT

GOLDEN_PATH = os.path.join(ROOT, 'tests', 'golden', 'epilogue_parity.json')


def _conv(ns, tile, kernel, rows=64):
    """Two cases per instantiation: ragged everything with bias and statistics; another ragged shape with neither."""
    return lambda *shapes: [dict(op='conv', ns=ns, tile=tile, kernel=kernel, rows=rows, shape=s[:4], bias=s[4], stats=s[5]) for s in shapes]


def _cases():
    out = []
    for ns in (1, 2, 3):
        ig = lambda tile: _conv(ns, tile, 'igemm')
        out += ig((1, 8, 8))((2, 5, 70, 4, True, True), (1, 16, 33, 8, False, False))              # vector staging (R % 4 == 0)
        out += ig((1, 8, 8))((2, 5, 70, 6, True, True), (1, 16, 33, 6, False, False))              # scalar staging
        out += ig((4, 4, 16))((1, 5, 70, 10, True, True), (2, 16, 33, 10, False, False))           # scalar staging, 8 < R
        out += ig((2, 4, 16))((1, 5, 70, 12, True, True), (1, 5, 33, 16, False, False))            # (f16x2: Ci % 16 != 0 keeps it here)
        out += ig((2, 4, 32))((1, 5, 70, 20, True, True), (1, 5, 33, 32, False, False))
    out += _conv(2, (2, 4, 16), 'pipe')((2, 16, 70, 12, True, True), (1, 48, 33, 16, False, False), (1, 16, 64, 16, True, False))
    out += _conv(2, (2, 4, 32), 'co32', 32)((1, 5, 20, 20, True, True), (1, 16, 32, 32, False, False), (1, 5, 20, 32, False, True))
    out += _conv(2, (4, 4, 32), 'wide')((1, 32, 64, 32, True, True))                                # the control
    for ns in (1, 2, 3):
        pw = lambda rows, *shapes: [dict(op='pw', ns=ns, rows=rows, shape=s[:4], bias=s[4], stats=s[5]) for s in shapes]
        out += pw(64, (2, 5, 33, 300, True, True), (1, 16, 64, 256, False, False))                  # N % 4 == 0: vector loads
        out += pw(64, (1, 5, 33, 301, True, True), (2, 32, 64, 599, False, False))
        out += pw(128, (2, 5, 70, 300, True, True), (1, 48, 160, 512, False, False))                # nsplit 1, 2: the pipe kernel
        out += pw(128, (1, 5, 70, 301, True, True), (2, 16, 129, 599, False, False))
    for s in ((1, 5, 70, 20, True, True), (1, 6, 36, 32, False, False), (1, 5, 70, 12, True, True), (2, 6, 36, 16, False, False),
              (2, 5, 70, 6, True, True), (1, 6, 36, 8, False, False)):
        out.append(dict(op='conv_fp32', shape=s[:4], bias=s[4], stats=s[5]))
    for s in ((2, 5, 33, 300, True, True), (1, 32, 64, 256, False, False), (1, 5, 70, 301, True, True), (1, 64, 128, 512, True, True),
              (1, 64, 160, 512, False, False)):
        out.append(dict(op='pw_fp32', shape=s[:4], bias=s[4], stats=s[5]))
    for c in out:
        c['id'] = '-'.join([c['op'] + (f"{c['ns']}" if 'ns' in c else '')] + [str(v) for v in c['shape']] +
                           ['bias' if c['bias'] else 'nobias', 'stats' if c['stats'] else 'nostats'])
    assert len({c['id'] for c in out}) == len(out)
    return out


CASES = _cases()


def field(shape, salt):
    """Element i of tensor `salt` = (the low 22 bits of hash32(i, salt) - 2^21) / 2^20: exact in fp32 and the same on every machine;
    22 significant bits, so the lo / second / third pieces of the split arithmetics are not zero."""
    n = 1
    for d in shape:
        n *= d
    h = (torch.arange(n, dtype=torch.int64) * 2654435761 + (salt * 97 + 12345)) & 0xffffffff
    h = h ^ (h >> 15)
    h = (h * 40503) & 0xffffffff
    h = h ^ (h >> 13)
    return (((h & 0x3fffff) - 0x200000).to(torch.float32) / 1048576.0).reshape(shape)


def route_of(lib, case):
    b, ci, co, l = case['shape']
    if case['op'] == 'conv':
        return lib.pvcnn_conv3d_fwd_split_route(b, ci, co, l, case['ns'])
    return lib.pvcnn_pwconv_fwd_split_route(b, ci, co, l, case['ns'])


def expected_route(case):
    if case['op'] == 'conv':
        tx, ty, tz = case['tile']
        return (tx * ty * tz) << 8 | case['rows']
    return case['rows']


def run_case(be, case):
    """-> the tensors the call returns, on the CPU."""
    b, ci, co, l = case['shape']
    conv = case['op'].startswith('conv')
    x = field((b, ci, l, l, l) if conv else (b, ci, l), 1).cuda()
    w = (field((co, ci, 3, 3, 3) if conv else (co, ci), 2) / 32.0).cuda()
    bias = field((co,), 3).cuda() if case['bias'] else None
    if case['op'] == 'conv':
        out = be.conv3d_forward_split(x, w, bias, case['ns'], want_stats=case['stats'])
    elif case['op'] == 'pw':
        out = be.pwconv_forward_split(x, w, bias, case['ns'], want_stats=case['stats'])
    elif case['op'] == 'conv_fp32':
        out = be.conv3d_forward(x, w, bias, want_stats=case['stats'])
    else:
        out = be.pwconv_forward(x, w, bias, want_stats=case['stats'])
    return [t.cpu().contiguous() for t in (out if isinstance(out, tuple) else (out,))]


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.numpy().tobytes())
    return h.hexdigest()


def record(be):
    return {case['id']: digest(run_case(be, case)) for case in CASES}


def dumps(table):
    return json.dumps(table, indent=1, sort_keys=True) + '\n'


def test_the_cases_take_the_launches_they_are_listed_for():
    """On the CPU (the route queries are host code): every split case takes the tile it is listed under, and the list still holds every
    (kernel, arithmetic, tile, staging) combination of the docstring."""
    from pvcnn_amd import _lib
    lib = _lib.load()
    reached = set()
    for case in CASES:
        if 'ns' not in case:
            continue
        assert route_of(lib, case) == expected_route(case), (case['id'], route_of(lib, case))
        b, ci, co, l = case['shape']
        if case['op'] == 'conv':
            vec = l % 4 == 0
            assert case['kernel'] != 'pipe' or (ci % 16 == 0 and vec), case['id']
            assert case['kernel'] != 'igemm' or case['ns'] != 2 or case['tile'] != (2, 4, 16) or not vec or ci % 16 != 0, case['id']
            assert case['kernel'] != 'igemm' or case['ns'] != 2 or case['tile'][2] != 32 or co > 32, case['id']
            reached.add((case['kernel'], case['ns'], case['tile'], vec))
        else:
            reached.add(('pw', case['ns'], case['rows'], l % 4 == 0))
    want = {('igemm', ns, tile, vec) for ns in (1, 2, 3)
            for tile, vec in (((1, 8, 8), True), ((1, 8, 8), False), ((4, 4, 16), False), ((2, 4, 16), True), ((2, 4, 32), True))}
    want |= {('pipe', 2, (2, 4, 16), True), ('co32', 2, (2, 4, 32), True), ('wide', 2, (4, 4, 32), True)}
    want |= {('pw', ns, rows, vec) for ns in (1, 2, 3) for rows in (64, 128) for vec in (True, False)}
    assert reached == want
    for key in {k for k in reached}:
        group = [c for c in CASES if 'ns' in c and
                 ((c['op'] == 'conv' and (c['kernel'], c['ns'], c['tile'], c['shape'][3] % 4 == 0) == key) or
                  (c['op'] == 'pw' and ('pw', c['ns'], c['rows'], c['shape'][3] % 4 == 0) == key))]
        if key[0] == 'wide':
            continue
        assert {c['bias'] for c in group} == {True, False} and {c['stats'] for c in group} == {True, False}, key


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN_PATH) as fh:
        table = json.load(fh)
    assert sorted(table) == sorted(c['id'] for c in CASES)
    return table


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=[c['id'] for c in CASES])
def test_bit_identical_to_the_kernels_with_their_own_epilogues(hip, golden, case):
    if 'ns' in case:
        assert route_of(hip.lib, case) == expected_route(case), case['id']
    out = run_case(hip, case)
    assert len(out) == (2 if case['stats'] else 1)
    assert digest(out) == golden[case['id']], case['id']
