"""FlatAdam's parameter groups on the host (pvcnn_amd/optim.py: check_param_groups, group_runs): the partition check and the run
tables the grouped kernel of csrc/optim.hip indexes, on CPU tensors -- no GPU, no kernel."""
import pytest
import torch
import torch.nn as nn

from pvcnn_amd.dp import GradBucketReducer
from pvcnn_amd.optim import FlatAdam, check_param_groups, group_runs


def _toy():
    torch.manual_seed(0)
    return nn.Sequential(nn.Conv1d(7, 33, 1), nn.BatchNorm1d(33), nn.ReLU(), nn.Conv1d(33, 5, 1), nn.Conv3d(3, 4, 3))


def _decay_split(net):
    params = list(net.parameters())
    return [p for p in params if p.dim() > 1], [p for p in params if p.dim() <= 1]


def test_run_tables_map_every_element_to_its_parameters_group():
    net = _toy()
    assert [p.numel() for p in net.parameters()] == [231, 33, 33, 33, 165, 5, 324, 4]
    red = GradBucketReducer(net, bucket_mb=0.001)
    assert len(red.buckets) > 2
    decay, rest = _decay_split(net)
    group_of = check_param_groups(red.params, [{'params': decay}, {'params': rest, 'weight_decay': 0.0}])
    assert all(group_of[p] == 0 for p in decay) and all(group_of[p] == 1 for p in rest)
    merged = False
    for b in red.buckets:
        runs = group_runs(b.params, group_of)
        size = sum(p.numel() for p in b.params)
        ends = [e for e, _ in runs]
        assert ends == sorted(set(ends)) and ends[0] > 0, runs                   # strictly increasing
        assert ends[-1] == size, (runs, size)
        assert all(a[1] != c[1] for a, c in zip(runs, runs[1:])), runs           # adjacent parameters of one group are ONE run
        merged |= len(runs) < len(b.params)
        brute = [group_of[p] for p in b.params for _ in range(p.numel())]        # element by element
        table, lo = [], 0
        for end, gid in runs:
            table += [gid] * (end - lo)
            lo = end
        assert table == brute
    assert merged                                                                # (the two BatchNorm vectors share a bucket and a run)


def test_partition_check_names_missing_duplicated_and_foreign_parameters():
    net = _toy()
    red = GradBucketReducer(net, bucket_mb=0.001)
    decay, rest = _decay_split(net)
    with pytest.raises(ValueError, match=r'missing: parameter 7 of shape \(4,\)'):
        check_param_groups(red.params, [{'params': decay}, {'params': rest[:-1]}])
    with pytest.raises(ValueError, match=r'duplicated: parameter 0 of shape \(33, 7, 1\) is in groups 0 and 1'):
        check_param_groups(red.params, [{'params': decay}, {'params': rest + decay[:1]}])
    with pytest.raises(ValueError, match=r'foreign: a tensor of shape \(3,\) in group 1'):
        check_param_groups(red.params, [{'params': decay}, {'params': rest + [torch.zeros(3)]}])
    with pytest.raises(ValueError, match='amsgrad'):
        check_param_groups(red.params, [{'params': decay}, {'params': rest, 'amsgrad': True}])
    with pytest.raises(ValueError, match='decoupled_weight_decay'):
        check_param_groups(red.params, [{'params': decay, 'decoupled_weight_decay': False}, {'params': rest}], decoupled_weight_decay=True)
    with pytest.raises(ValueError, match='maximize'):
        check_param_groups(red.params, [{'params': decay, 'maximize': True}, {'params': rest}])
    # a group that repeats the optimizer's own setting is fine
    check_param_groups(red.params, [{'params': decay, 'amsgrad': True}, {'params': rest}], amsgrad=True)


def test_the_constructor_checks_the_groups_before_it_asks_for_a_gpu():
    """A wrong partition is reported as such -- before any device memory is touched, hence on a CPU model too, where a correct one
    ends at 'needs float32 parameters on a GPU'."""
    net = _toy()
    red = GradBucketReducer(net, bucket_mb=0.001)
    decay, rest = _decay_split(net)
    with pytest.raises(ValueError, match='missing'):
        FlatAdam(red, param_groups=[{'params': decay}])
    with pytest.raises(ValueError, match='on a GPU'):
        FlatAdam(red, param_groups=[{'params': decay}, {'params': rest, 'weight_decay': 0.0}])
    with pytest.raises(ValueError, match='max_grad_norm'):
        FlatAdam(red, max_grad_norm=0.0)
