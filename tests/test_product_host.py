"""The host logic shared by the voxel Conv3d and the SharedMLP 1x1 convolution, pinned call by call on the CPU.

Two logs are compared with tests/golden/product_calls.json (recorded by tests/golden/gen_product_calls_golden.py, which imports the
stand-ins below, so the two cannot disagree):

  * node  -- what the autograd nodes VoxelConv3d / PointwiseConv ask of a backend: a recording stand-in computes with
             torch.nn.functional and notes every call (name, tensor shapes, keyword names, where each amax buffer came from), over the
             full product of arithmetic mode, bias, want_stats, which inputs want a gradient, the backend's optional surface, the two
             backward-weight bars and amax tags on the input and on the incoming gradient;
  * lib   -- what HipBackend's Conv3d / 1x1 methods send to the C library: a proxy `lib` answers the host-only size and route queries
             from the real library and records every launch (entry, integers, the role of each pointer) without running a kernel.

The golden is kept small by storing every distinct value once: `Table` turns a call entry, a log or a launch record into its index in
a table of the file, and the node cases -- generated with the axes that matter least innermost -- are run-length coded
("cases": [index into "logs", how many consecutive cases])."""
import contextlib
import ctypes
import inspect
import itertools
import json
import os

import torch
import torch.nn.functional as F

from conftest import ROOT

GOLDEN_PATH = os.path.join(ROOT, 'tests', 'golden', 'product_calls.json')
AMAX_NAMES = ('amax', 'x_amax', 'gy_amax')


class Table:
    """Distinct JSON values in order of first appearance; index(v) -> position of v."""

    def __init__(self):
        self.rows, self._at = [], {}

    def index(self, v):
        key = json.dumps(v)
        if key not in self._at:
            self._at[key] = len(self.rows)
            self.rows.append(json.loads(key))
        return self._at[key]


def run_lengths(values):
    runs = []
    for v in values:
        if runs and runs[-1][0] == v:
            runs[-1][1] += 1
        else:
            runs.append([v, 1])
    return runs


def _desc(v):
    if isinstance(v, torch.Tensor):
        return list(v.shape)
    return v if v is None or isinstance(v, (bool, int)) else repr(v)


def recorded(fn, name=None):
    """Note the call (name, positional arguments, keywords by name) on `self.log`, then run the torch implementation."""
    names, name = list(inspect.signature(fn).parameters)[1:], name or fn.__name__

    def wrapper(self, *args, **kwargs):
        def show(name, v):
            return self.amax_origin(v) if name in AMAX_NAMES else _desc(v)
        self.log.append([name, [show(n, v) for n, v in zip(names, args)], {n: show(n, v) for n, v in kwargs.items()}])
        return fn(self, *args, **kwargs)
    wrapper.__name__, wrapper.__wrapped__ = name, fn
    return wrapper


class RecordingBackend:
    """torch stand-ins for the Conv3d / 1x1 kernels that record how the autograd nodes call them."""
    has_conv3d_split = has_pwconv_split = True
    conv_math = pw_math = 'f16x2'
    CONV_NSPLIT = PW_NSPLIT = {'f16x2': 2, 'bf16x3': 3, 'fp32': 0}
    PW_AMAX_SEG = 256

    def __init__(self, has_grad_out=False, serves=True, pw_wgrad_f16_min_macs=0, pw_split_min_macs=0):
        self.log, self.own, self.tags, self.bwd_images = [], {}, {}, set()
        self.has_grad_out, self.serves = has_grad_out, serves
        self.pw_wgrad_f16_min_macs, self.pw_split_min_macs = pw_wgrad_f16_min_macs, pw_split_min_macs

    def amax_origin(self, amax):
        if amax is None:
            return None
        if id(amax) in self.tags:
            return 'tag'
        return ['own', self.own[id(amax)]] if id(amax) in self.own else 'unknown'

    def _measure(self, want_global):
        buf = torch.zeros(1, dtype=torch.int32)
        self.own[id(buf)] = bool(want_global)
        self.keep = getattr(self, 'keep', []) + [buf]
        return buf

    @recorded
    def conv_amax(self, x, want_global=True):
        return self._measure(want_global)

    # ---- the products themselves: 5-D tensors are the Conv3d's, 3-D ones the 1x1's ----
    @staticmethod
    def _fwd(x, w, bias):
        if x.dim() == 5:
            return F.conv3d(x, w, bias, padding=1)
        return torch.einsum('oc,bcn->bon', w, x) + (bias.view(1, -1, 1) if bias is not None else 0)

    @staticmethod
    def _bwd_data(g, w):
        return F.conv_transpose3d(g, w, padding=1) if g.dim() == 5 else torch.einsum('oc,bon->bcn', w, g)

    def _bwd_weight(self, x, g, with_bias, out_w, out_b):
        if x.dim() == 5:
            gw = torch.nn.grad.conv3d_weight(x, (g.shape[1], x.shape[1], 3, 3, 3), g, padding=1)
            gb = g.sum(dim=(0, 2, 3, 4))
        else:
            gw, gb = torch.einsum('bon,bcn->oc', g, x), g.sum(dim=(0, 2))
        assert self.has_grad_out or (out_w is None and out_b is None)
        gw = gw if out_w is None else out_w.copy_(gw)
        gb = gb if out_b is None else out_b.copy_(gb)
        return (gw, gb) if with_bias else gw

    def _stats(self, y, want_stats):
        return (y, torch.zeros(y.shape[1], 1, 2)) if want_stats else y

    def _split(self, x, wts, bias, co, want_stats):
        y = self._bwd_data(x, wts) if id(wts) in self.bwd_images else self._fwd(x, wts, bias)
        assert y.shape[1] == co
        return self._stats(y, want_stats)

    @recorded
    def conv3d_forward(self, x, weight, bias, want_stats=False):
        return self._stats(self._fwd(x, weight, bias), want_stats)

    @recorded
    def conv3d_forward_split(self, x, weight, bias, nsplit, want_stats=False, amax=None):
        return self._stats(self._fwd(x, weight, bias), want_stats)

    @recorded
    def conv3d_igemm_split(self, x, wts, bias, co, nsplit, want_stats=False, amax=None):
        return self._split(x, wts, bias, co, want_stats)

    @recorded
    def conv3d_backward_data(self, grad_y, weight):
        return self._bwd_data(grad_y, weight)

    @recorded
    def conv3d_backward_data_split(self, grad_y, weight, nsplit, amax=None):
        return self._bwd_data(grad_y, weight)

    @recorded
    def conv3d_backward_weight_f16_serves(self, x):
        return self.serves

    @recorded
    def conv3d_backward_weight(self, x, grad_y, with_bias=False, out_w=None, out_b=None):
        return self._bwd_weight(x, grad_y, with_bias, out_w, out_b)

    @recorded
    def conv3d_backward_weight_f16(self, x, grad_y, x_amax=None, gy_amax=None, with_bias=False, out_w=None, out_b=None):
        return self._bwd_weight(x, grad_y, with_bias, out_w, out_b)


class RecordingBackendWithImages(RecordingBackend):
    """... with the optional weight-image surface: the backward-data image is told from the forward one by identity."""

    def _images(self, weight):
        wf, wb = weight.detach().clone(), weight.detach().clone()
        self.bwd_images.add(id(wb))
        self.keep = getattr(self, 'keep', []) + [wb]
        return wf, wb

    @recorded
    def conv_weight_images(self, weight, nsplit):
        return self._images(weight)


# the 1x1's methods are the Conv3d's under their own names: the stand-in's arithmetic goes by the tensors' dimensions
for _conv, _pw in (('conv_amax', 'pw_amax'), ('conv_weight_images', 'pw_weight_images'), ('conv3d_igemm_split', 'pwconv_gemm_split'),
                   *((f'conv3d_{n}', f'pwconv_{n}') for n in ('forward', 'forward_split', 'backward_data', 'backward_data_split',
                                                              'backward_weight', 'backward_weight_f16', 'backward_weight_f16_serves'))):
    _owner = RecordingBackendWithImages if 'images' in _pw else RecordingBackend
    setattr(_owner, _pw, recorded(getattr(_owner, _conv).__wrapped__, _pw))


# ---- the node log -----------------------------------------------------------------------------------------------------------------
KINDS = (('conv', (2, 3, 4, 4, 4), (6, 3, 3, 3, 3)), ('pw3', (2, 8, 64), (12, 8, 1)), ('pw4', (2, 8, 16, 4), (12, 8, 1, 1)))
GRADS = ((True, True, True), (False, True, True), (True, False, False), (False, False, True))     # (x, weight, bias) want a gradient
# split=None: pw_nsplit decides against pw_split_min_macs, set to the case's own multiply-add count (the split path: `macs < bar` is
# false) or to one more (fp32) -- a miscounted GEMM takes the other path
AUTO_LOW, AUTO_HIGH = 'auto, bar at the MAC count', 'auto, bar one above'
PW_MACS = 2 * 8 * 12 * 64                   # B * Ci * Co * N of both 1x1 cases


def node_cases():
    for kind, xs, ws in KINDS:
        modes = (0, 1, 2, 3) if kind == 'conv' else (0, 1, 2, 3, AUTO_LOW, AUTO_HIGH)
        for mode, tag_x, grads, grad_out, want_stats, images, has_bias, serves, tag_g, wgrad_bar in itertools.product(
                modes, (True, False), GRADS, (True, False), (False, True), (True, False), (True, False), (True, False), (True, False),
                (0, 1 << 62)):
            yield kind, xs, ws, mode, has_bias, want_stats, grads, images, grad_out, wgrad_bar, serves, tag_x, tag_g


@contextlib.contextmanager
def seam(fake):
    from pvcnn_amd.modules.functional import backend
    saved, backend._backend = backend._backend, fake
    try:
        yield
    finally:
        backend._backend = saved


_DATA = {}


def _data(kind, xs, ws):
    """Inputs of a kind and the plain-autograd truth (output and all gradients, with and without bias), made once."""
    if kind not in _DATA:
        g = torch.Generator().manual_seed(1588147245 + len(_DATA))
        x, w, b = torch.randn(xs, generator=g), torch.randn(ws, generator=g) * 0.3, torch.randn(ws[0], generator=g)
        conv = {5: lambda *a: F.conv3d(*a, padding=1), 3: F.conv1d, 4: F.conv2d}[len(xs)]
        gy = torch.randn(conv(x, w, b).shape, generator=g)
        truth = {}
        for has_bias in (True, False):
            leaves = [t.clone().requires_grad_() for t in ((x, w, b) if has_bias else (x, w))]
            y = conv(*leaves)
            y.backward(gy)
            truth[has_bias] = (y.detach(), [t.grad for t in leaves] + [None] * (not has_bias))
        _DATA[kind] = (x, w, b, gy, truth)
    return _DATA[kind]


def run_node_case(case):
    """One forward + backward of a node on the recording stand-in -> (its call log, output, gradients, truth)."""
    from pvcnn_amd.modules.functional import _cache, _gradslots
    from pvcnn_amd.modules.functional.conv3d import voxel_conv3d
    from pvcnn_amd.modules.functional.pwconv import pointwise_conv
    kind, xs, ws, mode, has_bias, want_stats, grads, images, grad_out, wgrad_bar, serves, tag_x, tag_g = case
    x0, w0, b0, gy, truth = _data(kind, xs, ws)
    auto = isinstance(mode, str)
    fake = (RecordingBackendWithImages if images else RecordingBackend)(
        has_grad_out=grad_out, serves=serves, pw_wgrad_f16_min_macs=wgrad_bar, pw_split_min_macs=(PW_MACS + 1 if mode == AUTO_HIGH else PW_MACS if auto else 0))
    x, w = x0.clone().requires_grad_(grads[0]), w0.clone().requires_grad_(grads[1])
    b = b0.clone().requires_grad_(grads[2]) if has_bias else None
    seg = xs[2] if kind == 'conv' else fake.PW_AMAX_SEG
    tags = [torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)]
    fake.tags = {id(t): True for t in tags}
    # the parameters' slots in a flat gradient bucket: handed to a backend that has_grad_out as out_w / out_b
    slots = [_gradslots.register(p, torch.zeros_like(p)) for p in (w, b) if p is not None and p.requires_grad]
    held = []
    try:
        with seam(fake):
            if tag_x:
                _cache.tag_amax(x, seg, tags[0])
            out = voxel_conv3d(x, w, b, want_stats, mode) if kind == 'conv' else pointwise_conv(x, w, b, want_stats, None if auto else mode)
            y = out[0] if want_stats else out
            if y.requires_grad:
                if tag_g:
                    y.register_hook(lambda g: held.append(_cache.tag_amax(g, seg, tags[1])) or held[-1])
                y.backward(gy.clone())          # (a tensor of its own: a tag must not outlive the case)
    finally:
        _gradslots.unregister(slots)
    return fake.log, y.detach(), [x.grad, w.grad, b.grad if has_bias else None], truth[has_bias]


def node_log():
    entries, logs, cases, results = Table(), Table(), [], []
    for case in node_cases():
        log, y, got, want = run_node_case(case)
        cases.append(logs.index([entries.index(e) for e in log]))
        results.append((case, y, got, want))
    return {'entries': entries.rows, 'logs': logs.rows, 'cases': run_lengths(cases)}, results


# ---- the wrapper log --------------------------------------------------------------------------------------------------------------
HOST_ONLY = ('_bytes', '_stats_parts', '_count', '_route', '_slices', '_supported', '_grad_floats')       # + *_pair_entry*: fills a host table


class ProxyLib:
    """Forwards the host-only queries to the real library; records every other entry's arguments and returns 0."""

    def __init__(self, real, recorder):
        self._real, self._rec = real, recorder

    def __getattr__(self, name):
        if name.endswith(HOST_ONLY) or '_pair_entry' in name:
            return getattr(self._real, name)
        return lambda *args: self._rec.launch(name, args)


class LibRecorder:
    """The role of every pointer a launch receives: NULL, the PVCNN_TABLE_ONLY sentinel, an argument of the public method, or the
    k-th buffer (in order of first use) the method allocated itself."""

    def __init__(self):
        self.allocated, self.reset = {}, None
        self.begin({})

    def begin(self, named):
        self.calls, self.fresh = [], {}
        self.named = {t.data_ptr(): name for name, t in named.items() if isinstance(t, torch.Tensor) and t.numel()}
        self.held = list(named.values())

    def noting(self, make):
        """torch.empty / zeros / full / empty_like as backend.py calls it, with every buffer it makes noted as one of the method's own."""
        def made(*args, **kwargs):
            t = make(*args, **kwargs)
            if t.numel():
                self.allocated[t.data_ptr()] = (t, t.numel(), str(t.dtype))       # (kept alive: an address is never handed out twice)
            return t
        return made

    def empty(self, *args, **kwargs):
        return self.noting(self._torch_empty)(*args, **kwargs)

    def role(self, a):
        if isinstance(a, ctypes.Array):         # a host table of pointers (each by its role) or of integers
            return [self.role(ctypes.c_void_p(v)) if a._type_ is ctypes.c_void_p else v for v in a]
        if not isinstance(a, ctypes.c_void_p):
            return a if a is None or isinstance(a, (bool, int, float)) else repr(a)
        if a.value is None:
            return 'NULL'
        if a.value == 1:
            return 'PVCNN_TABLE_ONLY'
        if a.value in self.named:
            return 'argument ' + self.named[a.value]
        if a.value in self.allocated:
            _, numel, dtype = self.allocated[a.value]
            k = self.fresh.setdefault(a.value, len(self.fresh))
            return f'fresh buffer #{k} of {numel} elements of {dtype}'
        return 'unknown pointer'

    def launch(self, name, args):
        self.calls.append([name, ['NULL' if a is None else self.role(a) for a in args]])
        return 0

    def check(self, rc, what):
        self.calls[-1].append(what)
        assert rc == 0


class _NullLaunch:
    def __init__(self, ref):
        pass

    def __enter__(self):
        return ctypes.c_void_p(None)

    def __exit__(self, *exc):
        return False


class _Shim:
    """A module as backend.py sees it, with some names replaced (nothing outside that module is touched)."""

    def __init__(self, module, **replaced):
        self._module = module
        self.__dict__.update(replaced)

    def __getattr__(self, name):
        return getattr(self._module, name)


@contextlib.contextmanager
def proxied_backend():
    """A HipBackend whose `lib` is the proxy, with CPU tensors let through and a null stream -> (backend, recorder).  The module's
    own names `torch` and `_lib` are shims whose `empty` (`zeros`, `full`, `empty_like`) / `check` report to the recorder; no stream
    is ever being captured."""
    from pvcnn_amd import _lib
    from pvcnn_amd.modules.functional import backend as mod
    rec = LibRecorder()
    be = mod.HipBackend()
    be._lib = ProxyLib(_lib.load(), rec)
    rec._torch_empty = torch.empty
    saved = (mod._dev, mod._Launch, mod._lib, mod.torch)
    shim = _Shim(torch, empty=rec.empty, cuda=_Shim(torch.cuda, is_current_stream_capturing=lambda: False),
                 **{name: rec.noting(getattr(torch, name)) for name in ('zeros', 'full', 'empty_like')})
    mod._dev, mod._Launch, mod._lib, mod.torch = (lambda t, name: None), _NullLaunch, _Shim(_lib, check=rec.check), shim
    try:
        yield be, rec
    finally:
        mod._dev, mod._Launch, mod._lib, mod.torch = saved


def lib_calls():
    """(shape label, amax_global, method name, arguments by name, keyword arguments) of every wrapper call that is pinned."""
    f = lambda *s: torch.zeros(*s)
    tf = (False, True)
    conv = dict(amax='conv_amax', fwd='conv3d_forward', bwd_data='conv3d_backward_data', wgrad='conv3d_backward_weight', wsplit='_conv_wsplit',
                images='conv_weight_images', fwd_split='conv3d_forward_split', split='conv3d_igemm_split', co='co')
    pw = dict(amax='pw_amax', fwd='pwconv_forward', bwd_data='pwconv_backward_data', wgrad='pwconv_backward_weight', wsplit='_pw_wsplit',
              images='pw_weight_images', fwd_split='pwconv_forward_split', split='pwconv_gemm_split', co='m')
    shapes = [(conv, (b, ci, co, r), (b, ci, r, r, r), (co, ci, 3, 3, 3), (b, co, r, r, r), b * r * r) for b, ci, co, r in ((1, 3, 5, 4), (2, 16, 32, 8))]
    shapes += [(pw, (b, k, m, n), (b, k, n), (m, k), (b, m, n), b * ((n + 255) // 256)) for b, k, m, n in ((2, 8, 12, 20), (2, 8, 12, 257))]
    for names, dims, xs, ws, gs, tiles in shapes:
        tag = f"{names['amax'].split('_')[0]} {dims}"
        x, w, g, bias = f(*xs), f(*ws), f(*gs), f(ws[0])
        amaxes = [None] + [torch.zeros(n, dtype=torch.int32) for n in (1, 1 + tiles, 3 + tiles)]     # none, one word, the table, a wrong length
        for ag, wg in itertools.product(tf, tf):
            yield tag, ag, names['amax'], {'x': x}, {'want_global': wg}
            if names is conv:
                yield tag, ag, 'absmax_tiles', {'x': x.view(xs[0], xs[1], -1), 'seg': xs[2]}, {'want_global': wg}
        yield tag, False, 'absmax_bits', {'x': x}, {}
        for hb, ws_ in itertools.product(tf, tf):
            yield tag, False, names['fwd'], {'x': x, 'weight': w, 'bias': bias if hb else None}, {'want_stats': ws_}
        yield tag, False, names['bwd_data'], {'grad_y': g, 'weight': w}, {}
        yield tag, False, names['wgrad'] + '_f16_serves', {'x': x}, {}
        for wb, given in itertools.product(tf, tf):
            out = {'out_w': f(*ws), 'out_b': f(ws[0]) if wb else None} if given else {}
            yield tag, False, names['wgrad'], {'x': x, 'grad_y': g}, {'with_bias': wb, **out}
            for xa, ga in itertools.product(amaxes, amaxes):
                yield tag, False, names['wgrad'] + '_f16', {'x': x, 'grad_y': g, 'x_amax': xa, 'gy_amax': ga}, {'with_bias': wb, **out}
        wts = torch.zeros(64, dtype=torch.uint8)
        for ns in (1, 2, 3):
            for bd in tf:
                yield tag, False, names['wsplit'], {'weight': w, 'for_bwd_data': bd, 'nsplit': ns}, {}
            yield tag, False, names['images'], {'weight': w, 'nsplit': ns}, {}
            for am, ag in itertools.product(amaxes, tf):
                for hb, ws_ in itertools.product(tf, tf):
                    b_ = bias if hb else None
                    yield tag, ag, names['fwd_split'], {'x': x, 'weight': w, 'bias': b_, 'nsplit': ns}, {'want_stats': ws_, 'amax': am}
                    yield tag, ag, names['split'], {'x': x, 'wts': wts, 'bias': b_, names['co']: dims[2], 'nsplit': ns}, {'want_stats': ws_, 'amax': am}
                yield tag, ag, names['bwd_data'] + '_split', {'grad_y': g, 'weight': w, 'nsplit': ns}, {'amax': am}


def _result_shape(res):
    if isinstance(res, torch.Tensor):
        return list(res.shape)
    return [_result_shape(r) for r in res] if isinstance(res, (tuple, list)) else res


def lib_log():
    methods, launches, outcomes, cases = Table(), Table(), Table(), []       # (the arguments of a case are lib_calls()'s: not stored)
    with proxied_backend() as (be, rec):
        for tag, amax_global, method, args, kwargs in lib_calls():
            be.amax_global = amax_global
            rec.begin({**args, **kwargs})
            try:
                outcome = _result_shape(getattr(be, method)(*args.values(), **kwargs))
            except RuntimeError as e:
                outcome = 'RuntimeError: ' + str(e)
            cases.append([methods.index([tag, method]), [launches.index(c) for c in rec.calls], outcomes.index(outcome)])
    return {'methods': methods.rows, 'launches': launches.rows, 'outcomes': outcomes.rows, 'cases': cases}


def record():
    return {**{'node ' + k: v for k, v in node_log()[0].items()}, **{'lib ' + k: v for k, v in lib_log().items()}}


def dumps(golden):
    """One line per table of the file."""
    tables = [f'"{name}":' + json.dumps(rows, separators=(',', ':')) for name, rows in sorted(golden.items())]
    return '{\n' + ',\n'.join(tables) + '\n}\n'


# ---- the tests --------------------------------------------------------------------------------------------------------------------
def _golden(section):
    with open(GOLDEN_PATH) as fh:
        return {k[len(section) + 1:]: v for k, v in json.load(fh).items() if k.startswith(section + ' ')}


def _node_logs(section):
    """The call log of every node case, written out."""
    logs = [[section['entries'][e] for e in log] for log in section['logs']]
    return [logs[i] for i, n in section['cases'] for _ in range(n)]


def _lib_logs(section):
    return [[section['methods'][m], [section['launches'][i] for i in ls], section['outcomes'][o]] for m, ls, o in section['cases']]


def test_the_nodes_ask_the_backend_for_what_the_golden_records_and_compute_the_plain_convolution():
    section, results = node_log()
    got, want = _node_logs(section), _node_logs(_golden('node'))
    assert len(got) == len(want) == (4 + 6 + 6) * 1024         # the full product of the axes of node_cases()
    for i, (case, a, b) in enumerate(zip(node_cases(), got, want)):
        assert a == b, (i, case[0], case[3:], a, b)
    for case, y, grads, (want_y, want_grads) in results:
        assert torch.allclose(y, want_y, rtol=1e-4, atol=1e-4), (case[0], case[3:])
        for name, wanted, a, b in zip('xwb', case[6], grads, want_grads):
            if wanted and b is not None:
                assert a is not None and torch.allclose(a, b, rtol=1e-4, atol=1e-4), (case[0], case[3:], name)
            else:
                assert a is None, (case[0], case[3:], name)


def test_the_wrappers_send_the_library_what_the_golden_records():
    got, want = _lib_logs(lib_log()), _lib_logs(_golden('lib'))
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (i, a, b)
    texts = [log[-1] for log in got if isinstance(log[-1], str)]
    assert any('amax buffer has' in t for t in texts) and any('pwconv_backward_weight_f16: N must be a multiple of 4' in t for t in texts)
