"""The split-weight images (csrc/weight_image.h: the pre-split, pre-swizzled weights the f16x2, bf16 and bf16x3 products read) are
pinned BYTE FOR BYTE to what the per-kind writers of conv3d_bf16.hip and pointwise_bf16.hip wrote before the format was stated once:
tests/golden/weight_images.json holds, per case, the size pvcnn_*_weight_split_bytes returns and one SHA-256 over the WHOLE buffer
(every byte is written: the padding rows and chunks, and the shifts of the padded rows behind an f16x2 image), recorded by
tests/golden/gen_weight_images_golden.py from the commit before the header.

Inputs are the closed-form field of test_gpu_epilogue_parity.py; weight row r is scaled by 2^((r mod 7) - 3) and row 3 is all zeros, so
the per-row shifts of the f16x2 images differ (and one is the shift of a zero row).  Shapes (Co, Ci): ragged rows and chunks, one exact
tile, and for the 1x1 images both row tiles (64 and 128), with different tiles for the two directions ((64, 160), (160, 64), (130, 70)).
Cases: nsplit 1, 2, 3 x forward and backward-data through pvcnn_*_weight_split; the f16x2 pair entry and a registered bank refresh
(f16x2 and plain bf16) must write the same bytes as the single launches."""
import json
import os

import pytest
import torch

from conftest import ROOT
from test_gpu_epilogue_parity import digest, field

GOLDEN_PATH = os.path.join(ROOT, 'tests', 'golden', 'weight_images.json')
SHAPES = {'conv': ((70, 33), (20, 5), (64, 16)), 'pw': ((33, 5), (70, 33), (64, 160), (160, 64), (130, 70))}
ZERO_ROW = 3


def _cases():
    return [dict(kind=kind, co=co, ci=ci, ns=ns, bwd=bwd, id=f"{kind}-{co}x{ci}-ns{ns}-{'bwd' if bwd else 'fwd'}")
            for kind, shapes in SHAPES.items() for co, ci in shapes for ns in (1, 2, 3) for bwd in (0, 1)]


CASES = _cases()
PAIRS = [(kind, co, ci) for kind, shapes in SHAPES.items() for co, ci in shapes]
case_id = lambda kind, co, ci, ns, bwd: f"{kind}-{co}x{ci}-ns{ns}-{'bwd' if bwd else 'fwd'}"


def weight(kind, co, ci):
    """(Co, Ci, 3, 3, 3) or (Co, Ci) fp32 on the CPU: exact in fp32 (a 22-bit field times a power of two), the same on every machine."""
    taps = 27 if kind == 'conv' else 1
    w = field((co, ci, taps), 7 + co * 1000 + ci)
    w = w * torch.exp2(((torch.arange(co) % 7) - 3).to(torch.float32)).view(co, 1, 1)
    w[ZERO_ROW] = 0.0
    return w.reshape((co, ci, 3, 3, 3) if kind == 'conv' else (co, ci)).contiguous()


def bytes_of(lib, case):
    entry = lib.pvcnn_conv3d_weight_split_bytes if case['kind'] == 'conv' else lib.pvcnn_pwconv_weight_split_bytes
    return int(entry(case['co'], case['ci'], case['bwd'], case['ns']))


def split(be, case):
    w = weight(case['kind'], case['co'], case['ci']).cuda()
    fn = be._conv_wsplit if case['kind'] == 'conv' else be._pw_wsplit
    return fn(w, bool(case['bwd']), case['ns']).cpu()


def record(be):
    out = {}
    for case in CASES:
        img = split(be, case)
        assert img.numel() == bytes_of(be.lib, case), case['id']
        out[case['id']] = {'bytes': img.numel(), 'sha256': digest([img])}
    return out


def dumps(table):
    return json.dumps(table, indent=1, sort_keys=True) + '\n'


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN_PATH) as fh:
        table = json.load(fh)
    assert sorted(table) == sorted(c['id'] for c in CASES)
    return table


def test_the_sizes_are_the_recorded_ones(golden):
    """On the CPU (the size queries are host code): image + shift table of every case."""
    from pvcnn_amd import _lib
    lib = _lib.load()
    for case in CASES:
        assert bytes_of(lib, case) == golden[case['id']]['bytes'], case['id']
    for entry in (lib.pvcnn_conv3d_weight_split_bytes, lib.pvcnn_pwconv_weight_split_bytes):
        assert entry(0, 5, 0, 2) == 0 and entry(5, 0, 1, 2) == 0 and entry(5, 5, 0, 0) == 0 and entry(5, 5, 0, 4) == 0


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=[c['id'] for c in CASES])
def test_single_launch_images_are_the_recorded_bytes(hip, golden, case):
    img = split(hip, case)
    assert img.numel() == golden[case['id']]['bytes']
    assert digest([img]) == golden[case['id']]['sha256'], case['id']


@pytest.mark.gpu
@pytest.mark.parametrize('kind,co,ci', PAIRS, ids=[f'{k}-{co}x{ci}' for k, co, ci in PAIRS])
def test_the_pair_entry_writes_the_two_single_images(hip, golden, kind, co, ci):
    w = weight(kind, co, ci).cuda()
    pair = (hip.conv_weight_images if kind == 'conv' else hip.pw_weight_images)(w, 2)
    for bwd, img in enumerate(pair):
        want = golden[case_id(kind, co, ci, 2, bwd)]
        assert img.numel() == want['bytes'] and digest([img.cpu()]) == want['sha256'], (kind, co, ci, bwd)


@pytest.mark.gpu
@pytest.mark.parametrize('nsplit', [1, 2])
def test_a_bank_refresh_writes_the_single_images(hip, golden, nsplit):
    """Every shape registered in one model: one batched launch per kind writes all of them (entries of different tiles side by side)."""
    import torch.nn as nn
    net = nn.Sequential(*[nn.Conv3d(ci, co, 3, padding=1) if kind == 'conv' else nn.Conv1d(ci, co, 1) for kind, co, ci in PAIRS]).cuda()
    with torch.no_grad():
        for layer, (kind, co, ci) in zip(net, PAIRS):
            layer.weight.copy_(weight(kind, co, ci).view_as(layer.weight))
    hip.weight_bank_register(net)
    views = [layer.weight if kind == 'conv' else layer.weight.view(co, ci) for layer, (kind, co, ci) in zip(net, PAIRS)]
    images = lambda: [(hip.conv_weight_images if kind == 'conv' else hip.pw_weight_images)(w, nsplit) for w, (kind, _, _) in zip(views, PAIRS)]
    images()                                                       # first sighting: noted as wanted
    hip.weight_bank_refresh()
    bank = hip._bank()
    for pair, w, (kind, co, ci) in zip(images(), views, PAIRS):
        assert bank.entries[(kind, w.data_ptr(), (co, ci), nsplit)]['wf'] is pair[0]        # served from the bank
        for bwd, img in enumerate(pair):
            want = golden[case_id(kind, co, ci, nsplit, bwd)]
            assert img.numel() == want['bytes'] and digest([img.cpu()]) == want['sha256'], (kind, co, ci, bwd)
