"""Adam on the flat buckets of the data-parallel step (csrc/optim.hip).

Reference: train.py:96-119 calls `optimizer.step()` of torch.optim.Adam on the model's ~100 parameter tensors, train.py:121-122
`scheduler.step()` of a torch.optim.lr_scheduler on that optimizer, and train.py:186-199 / 249-255 save and restore
`optimizer.state_dict()`.  Here the parameters are laid out like the gradient buckets of `pvcnn_amd.dp.GradBucketReducer`
(flatten_parameters) and one elementwise kernel updates a whole bucket: same arithmetic as torch.optim.Adam, fp32, step counter AND
hyper-parameters on the device, so the update is graph-capturable (pvcnn_amd/graph.py) and costs ~10 us instead of 2 x 72 us for
PVCNN's 9.8 MiB.

FlatAdam IS a torch.optim.Optimizer: `param_groups` / `state` / `state_dict()` / `load_state_dict()` have torch.optim.Adam's layout
(per-parameter `step`, `exp_avg`, `exp_avg_sq`, under amsgrad `max_exp_avg_sq` -- here views of the flat buffers), so a checkpoint
written by either loads into the other, and a `torch.optim.lr_scheduler` drives it unchanged: the scheduler writes
`param_groups[k]['lr']` on the host, and the next `step()` -- or, for a captured step, `GraphedTrainStep.__call__` through
`sync_hyperparameters()` -- copies the hyper-parameters of every group into the device block the kernel reads.

Beyond the reference's one-group Adam (all optional; a FlatAdam built without them runs exactly the one-group kernel, launch for launch):
  * `param_groups`: torch's list of dicts -- a no-decay group for BatchNorm and biases, a smaller rate for a loaded backbone.  The
    groups must partition the reducer's parameters (`check_param_groups`).  The update stays ONE launch per bucket: the kernel gets
    a run table per bucket (`group_runs`: (end offset, group id), adjacent parameters of a group merged) and a (G, 5) hyper block.
  * `decoupled_weight_decay=True`: torch.optim.AdamW's update; `amsgrad=True`: a fourth flat buffer `max_exp_avg_sq`.  Both hold
    for the whole optimizer, as the kernel is chosen per launch.
  * `max_grad_norm`: torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm) in front of the update, without its pass over ~100
    tensors and without a place in the loop (a captured step has none): one sum-of-squares launch per bucket, one finalize, and the
    update multiplies the gradient by the coefficient in registers.  `p.grad` is NOT rewritten: after `step()` it still holds the
    unclipped gradient.  `opt.grad_norm` (a 0-d device tensor) is the norm before clipping, for logging without a sync.
  * `skip_nonfinite=True`: when the sum of squares is not finite (an overflowing bf16 step) the update kernels write nothing --
    parameters, moments and the step counter stay as they were -- and `opt.skipped_steps` (a 0-d device tensor) counts it.  The
    norm pass runs for this alone, too.
  Multi-rank: the norm is taken after `reducer.finish()`, on averaged gradients that are identical on every rank, so every rank
  clips and skips alike without another collective.

GPU only (there is no CPU implementation of the kernels); use torch.optim.Adam for CPU runs.  `check_param_groups` and `group_runs`
are pure host functions and work on CPU tensors.
"""
import math

import torch

from . import _lib
from .modules.functional.backend import _run

__all__ = ['FlatAdam', 'check_param_groups', 'group_runs']

_HYPER_KEYS = ('lr', 'betas', 'eps', 'weight_decay')
MAX_RUNS, MAX_GROUPS = 4096, 256                       # csrc/optim.hip: what the run table's LDS copy holds


def _describe(p, where=None):
    return (f'parameter {where} ' if where is not None else 'a tensor ') + f'of shape {tuple(p.shape)}'


def check_param_groups(params, param_groups, amsgrad=False, decoupled_weight_decay=False):
    """-> {parameter: group id} when `param_groups` (torch's list of dicts with 'params') holds every tensor of `params` exactly once
    and nothing else; ValueError naming what is missing, duplicated or foreign otherwise, and for a group that sets `amsgrad`,
    `decoupled_weight_decay` or `maximize` differently from the optimizer (one kernel variant per launch).  Host only."""
    index = {p: i for i, p in enumerate(params)}
    group_of, problems = {}, []
    if not param_groups:
        raise ValueError('FlatAdam: param_groups is empty')
    for gid, group in enumerate(param_groups):
        if not isinstance(group, dict) or 'params' not in group:
            raise ValueError(f"FlatAdam: param_groups[{gid}] is not a dict with 'params'")
        for key, mine in (('amsgrad', amsgrad), ('decoupled_weight_decay', decoupled_weight_decay), ('maximize', False)):
            if key in group and bool(group[key]) != bool(mine):
                raise ValueError(f'FlatAdam: param_groups[{gid}] sets {key}={group[key]!r}, the optimizer {key}={bool(mine)!r}: '
                                 f'{key} holds for the whole optimizer, not per group')
        members = group['params']
        for p in ([members] if isinstance(members, torch.Tensor) else members):
            if p not in index:
                problems.append(f'foreign: {_describe(p)} in group {gid} is not a parameter of the reducer')
            elif p in group_of:
                problems.append(f'duplicated: {_describe(p, index[p])} is in groups {group_of[p]} and {gid}')
            else:
                group_of[p] = gid
    problems += [f'missing: {_describe(p, i)} is in no group' for i, p in enumerate(params) if p not in group_of]
    if problems:
        raise ValueError('FlatAdam: param_groups must hold every parameter of the reducer exactly once -- ' + '; '.join(problems))
    return group_of


def group_runs(bucket_params, group_of):
    """The run table of one bucket: [(end offset, group id)] over the bucket's parameters laid back to back and unpadded
    (dp._Bucket), adjacent parameters of the same group merged; ends strictly increasing, the last one = the bucket's size."""
    runs, off = [], 0
    for p in bucket_params:
        if p.numel() == 0:
            continue
        off += p.numel()
        gid = group_of[p]
        if runs and runs[-1][1] == gid:
            runs[-1] = (off, gid)
        else:
            runs.append((off, gid))
    return runs


class FlatAdam(torch.optim.Optimizer):
    """opt = FlatAdam(reducer, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, *, param_groups=None,
                      decoupled_weight_decay=False, amsgrad=False, max_grad_norm=None, skip_nonfinite=False)
    per step, after reducer.finish(): opt.step().

    The gradients are read from the reducer's flat buckets (where `finish()` leaves them: `p.grad` are views of those buffers) and
    never written: with `max_grad_norm` the clip coefficient is applied in the update's registers, `p.grad` stays unclipped.
    Without `param_groups` there is one group (the reference trains with one: train.py:163); lr / betas / eps / weight_decay are
    the defaults of groups that do not set their own."""

    def __init__(self, reducer, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, *, param_groups=None,
                 decoupled_weight_decay=False, amsgrad=False, max_grad_norm=None, skip_nonfinite=False):
        self.amsgrad, self.decoupled_weight_decay = bool(amsgrad), bool(decoupled_weight_decay)
        self.skip_nonfinite = bool(skip_nonfinite)
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f'FlatAdam: max_grad_norm must be positive, got {max_grad_norm!r}')
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        groups, group_of = None, None
        if param_groups is not None:                             # validated on the host, before any device memory is touched
            groups = [dict(g, params=[g['params']] if isinstance(g['params'], torch.Tensor) else list(g['params']))
                      if isinstance(g, dict) and 'params' in g else g for g in param_groups]
            group_of = check_param_groups(reducer.params, groups, self.amsgrad, self.decoupled_weight_decay)
            if len(groups) > MAX_GROUPS:
                raise ValueError(f'FlatAdam: at most {MAX_GROUPS} parameter groups')
        if not reducer.buckets or not all(b.flat.is_cuda and b.flat.dtype == torch.float32 for b in reducer.buckets):
            raise ValueError('FlatAdam needs float32 parameters on a GPU (use torch.optim.Adam elsewhere)')
        reducer.flatten_parameters()
        self.reducer = reducer
        defaults = dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps), weight_decay=float(weight_decay),
                        capturable=True, amsgrad=self.amsgrad, decoupled_weight_decay=self.decoupled_weight_decay)
        # one group: model.parameters() order, torch.optim.Adam(model.parameters())'s
        super().__init__(list(reducer.params) if groups is None else groups, defaults)
        self._built = True
        # the reference's optimizer, untouched: one group and no option -> the one-group kernel, launch for launch
        self._norm_pass = self.max_grad_norm is not None or self.skip_nonfinite
        self._plain = groups is None and not (self.amsgrad or self.decoupled_weight_decay or self._norm_pass)
        dev = reducer.buckets[0].flat.device
        self.exp_avg = [torch.zeros_like(b.flat) for b in reducer.buckets]
        self.exp_avg_sq = [torch.zeros_like(b.flat) for b in reducer.buckets]
        self.max_exp_avg_sq = [torch.zeros_like(b.flat) for b in reducer.buckets] if self.amsgrad else None
        self.step_count = torch.zeros((1,), dtype=torch.float32, device=dev)
        # what the kernel reads: lr, beta1, beta2, eps, weight_decay -- (5,) for the one-group kernel, (G, 5) for the grouped one
        self.hyper = torch.zeros((5,) if self._plain else (len(self.param_groups), 5), dtype=torch.float32, device=dev)
        self._hyper_host = None
        self.run_tables, self.status, self.partials, self.grad_norm, self.skipped_steps = None, None, None, None, None
        if not self._plain:
            if group_of is None:
                group_of = {p: 0 for p in reducer.params}
            tables = [group_runs(b.params, group_of) for b in reducer.buckets]
            if max(len(t) for t in tables) > MAX_RUNS:
                raise ValueError(f'FlatAdam: a bucket alternates between groups {max(len(t) for t in tables)} times (at most {MAX_RUNS})')
            self.run_tables = [torch.tensor(t, dtype=torch.int32).reshape(-1, 2).to(dev) for t in tables]
        if self._norm_pass:
            # the status block of include/pvcnn_hip.h: norm, coef, skip, skipped | max_norm, skip_nonfinite | 2 reserved
            self._max_norm_host = math.inf if self.max_grad_norm is None else self.max_grad_norm
            self.status = torch.tensor([0.0, 1.0, 0.0, 0.0, self._max_norm_host, float(self.skip_nonfinite), 0.0, 0.0],
                                       dtype=torch.float32).to(dev)
            self.grad_norm, self.skipped_steps = self.status[0], self.status[3]
            # a FIXED grid per bucket (a function of its size alone): the order of every addition, hence the norm's bits, is fixed
            parts = [min(1024, max(1, -(-b.flat.numel() // 2048))) for b in reducer.buckets]
            self.partials = torch.zeros((sum(parts),), dtype=torch.float32, device=dev)
            self._partials = list(self.partials.split(parts))
        # torch.optim.Adam's per-parameter state, as views: `step` is the one device counter, the moments are slices of the flat buffers
        for i, b in enumerate(reducer.buckets):
            off = 0
            for p in b.params:
                n = p.numel()
                self.state[p] = {'step': self.step_count.view(()), 'exp_avg': self.exp_avg[i][off:off + n].view_as(p),
                                 'exp_avg_sq': self.exp_avg_sq[i][off:off + n].view_as(p)}
                if self.amsgrad:
                    self.state[p]['max_exp_avg_sq'] = self.max_exp_avg_sq[i][off:off + n].view_as(p)
                off += n
        self._lib = _lib.load()
        self.sync_hyperparameters()

    def add_param_group(self, param_group):
        if getattr(self, '_built', False):
            raise NotImplementedError('FlatAdam updates the parameter groups its reducer laid out at construction (run tables per bucket); '
                                      'pass param_groups= to the constructor, or build a second reducer / optimizer pair')
        super().add_param_group(param_group)

    def _group_hyper(self):
        rows = tuple((float(g['lr']), float(g['betas'][0]), float(g['betas'][1]), float(g['eps']), float(g['weight_decay']))
                     for g in self.param_groups)
        return rows[0] if self._plain else rows

    def sync_hyperparameters(self):
        """Copy every group's lr / betas / eps / weight_decay -- the whole (G, 5) block -- and `max_grad_norm` into device memory when
        any of them changed on the host (a scheduler stepped, a checkpoint was loaded, `opt.max_grad_norm = ...`).  One small
        host-to-device copy each, only then; never call it while a graph is being captured (step() skips it there -- the captured
        kernels read whatever the blocks hold at replay time)."""
        now = self._group_hyper()
        if now != self._hyper_host:
            self.hyper.copy_(torch.tensor(now, dtype=torch.float32), non_blocking=False)
            self._hyper_host = now
        if self._norm_pass:
            mx = math.inf if self.max_grad_norm is None else float(self.max_grad_norm)
            if mx != self._max_norm_host:
                self.status[4:5].copy_(torch.tensor([mx], dtype=torch.float32), non_blocking=False)
                self._max_norm_host = mx

    def _check_aliasing(self):
        for b in self.reducer.buckets:
            lo = b.pflat.data_ptr()
            hi = lo + b.pflat.numel() * 4
            for p in b.params:
                if not (lo <= p.data_ptr() < hi):
                    raise RuntimeError('FlatAdam: a parameter no longer lives in its flat bucket (model.to() / .half() / .float() after the '
                                       'optimizer was built re-allocates parameters): build the reducer and the optimizer last')

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._plain and len(self.param_groups) != 1:
            raise RuntimeError('FlatAdam updates one parameter group')
        buckets = self.reducer.buckets
        last = len(buckets) - 1
        with torch.cuda.device(self.step_count.device):
            if not torch.cuda.is_current_stream_capturing():
                self._check_aliasing()
                self.sync_hyperparameters()
            if self._plain:
                for i, b in enumerate(buckets):
                    _run(self._lib.pvcnn_adam_step, 'adam_step', self.step_count, b.pflat, b.flat, self.exp_avg[i], self.exp_avg_sq[i],
                         b.flat.numel(), self.step_count, self.hyper, int(i == last))
            else:
                if self._norm_pass:                                # the global norm of ALL buckets first: coefficient and skip flag
                    for b, part in zip(buckets, self._partials):
                        _run(self._lib.pvcnn_grad_sqsum, 'grad_sqsum', self.step_count, b.flat, b.flat.numel(), part, part.numel())
                    _run(self._lib.pvcnn_grad_norm_finalize, 'grad_norm_finalize', self.step_count, self.partials,
                         self.partials.numel(), self.status)
                for i, b in enumerate(buckets):
                    _run(self._lib.pvcnn_adam_step_grouped, 'adam_step_grouped', self.step_count, b.pflat, b.flat, self.exp_avg[i],
                         self.exp_avg_sq[i], self.max_exp_avg_sq[i] if self.amsgrad else None, b.flat.numel(), self.step_count,
                         self.hyper, len(self.param_groups), self.run_tables[i], self.run_tables[i].shape[0], self.status,
                         int(self.decoupled_weight_decay), int(i == last))
        # the kernel writes the parameters through raw pointers: torch's version counters do not move, so tell the holders of
        # derived data (the f16x2 weight images of backend.weight_bank_*) that every parameter changed
        from .modules.functional._autograd import native
        invalidate = getattr(native(), 'weight_bank_invalidate', None)
        if invalidate is not None:
            invalidate()
        return loss

    def zero_grad(self, set_to_none=True):
        self.reducer.zero_grad()

    # ---- checkpoints: torch.optim.Adam's layout (train.py:186-199 saves optimizer.state_dict(), 249-255 restores it) ----
    _STATE_KEYS = ('exp_avg', 'exp_avg_sq')

    def _moment_keys(self):
        return self._STATE_KEYS + (('max_exp_avg_sq',) if self.amsgrad else ())

    def state_dict(self):
        """{'state': {i: {'step', 'exp_avg', 'exp_avg_sq'[, 'max_exp_avg_sq']}}, 'param_groups': [{..., 'params': [ids]}, ...]} -- what
        torch.optim.Adam(the same groups, capturable=True).state_dict() holds for the same model: the ids run over the groups in
        order (tensors are copies)."""
        state, groups, i = {}, [], 0
        for g in self.param_groups:
            ids = []
            for p in g['params']:
                state[i] = {'step': self.step_count.detach().clone().view(()),
                            **{k: self.state[p][k].detach().clone() for k in self._moment_keys()}}
                ids.append(i)
                i += 1
            group = {k: v for k, v in g.items() if k != 'params'}
            group['params'] = ids
            groups.append(group)
        return {'state': state, 'param_groups': groups}

    def load_state_dict(self, state_dict):
        """Accepts the state_dict of a torch.optim.Adam / AdamW built with the same groups for the same model (any `capturable` /
        `fused` flavour: `step` may be a float or a tensor) -- and therefore FlatAdam's own.  The moments are copied INTO the flat
        buffers (the kernel's addresses never change: a captured graph stays valid); a parameter without saved state (never stepped)
        keeps zero moments.  Everything is validated BEFORE any state is touched."""
        groups = state_dict['param_groups']
        for g in groups:
            if g.get('maximize'):
                raise ValueError('FlatAdam does not implement maximize')
            if bool(g.get('amsgrad', False)) != self.amsgrad:
                raise ValueError(f'the checkpoint has amsgrad={bool(g.get("amsgrad", False))}, this FlatAdam amsgrad={self.amsgrad}')
            if 'decoupled_weight_decay' in g and bool(g['decoupled_weight_decay']) != self.decoupled_weight_decay:
                raise ValueError(f'the checkpoint has decoupled_weight_decay={bool(g["decoupled_weight_decay"])}, this FlatAdam '
                                 f'decoupled_weight_decay={self.decoupled_weight_decay}')
        if len(self.param_groups) == 1:
            # ONE set of hyper-parameters here: a checkpoint with several param groups -- e.g. a no-decay group for BatchNorm / biases --
            # loads only if they all agree (it used to load silently with groups[0]'s values)
            for g in groups:
                for key in _HYPER_KEYS:
                    a, b = g.get(key), groups[0].get(key)
                    if (tuple(a) if key == 'betas' and a is not None else a) != (tuple(b) if key == 'betas' and b is not None else b):
                        raise ValueError(f'FlatAdam keeps one set of hyper-parameters; the checkpoint\'s {len(groups)} param groups differ in {key!r}: '
                                         f'{[gg.get(key) for gg in groups]} (build it with param_groups= to load them)')
            sources = [groups[0]]
        else:
            mine, theirs = [len(g['params']) for g in self.param_groups], [len(g['params']) for g in groups]
            if mine != theirs:
                raise ValueError(f'the checkpoint has {len(theirs)} param groups of sizes {theirs}, this FlatAdam {len(mine)} of sizes {mine}')
            sources = groups
        ids = [i for g in groups for i in g['params']]
        params = [p for g in self.param_groups for p in g['params']]
        if len(ids) != len(params):
            raise ValueError(f'optimizer state for {len(ids)} parameters, this model has {len(params)}')
        for i, p in zip(ids, params):
            st = state_dict['state'].get(i)
            if st is None:
                continue
            for key in self._moment_keys():
                if key not in st:
                    raise ValueError(f'optimizer state {i} has no {key!r}')
                if tuple(st[key].shape) != tuple(p.shape):
                    raise ValueError(f'optimizer state {i}: {key} of shape {tuple(st[key].shape)} vs parameter {tuple(p.shape)}')
        found = {float(st['step']) for st in (state_dict['state'].get(i) for i in ids) if st is not None}
        if len(found) > 1:
            raise ValueError(f'FlatAdam keeps ONE step counter; the checkpoint has parameters at steps {sorted(found)}')
        for i, p in zip(ids, params):
            st = state_dict['state'].get(i)
            mine = self.state[p]
            for key in self._moment_keys():
                if st is None:
                    mine[key].zero_()
                else:
                    mine[key].copy_(st[key])
        self.step_count.fill_(found.pop() if found else 0.0)
        for g, target in zip(sources, self.param_groups):
            for key in _HYPER_KEYS + ('initial_lr',):
                if key in g:
                    target[key] = tuple(g[key]) if key == 'betas' else g[key]
        self.sync_hyperparameters()
