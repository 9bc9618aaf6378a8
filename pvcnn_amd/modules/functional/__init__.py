"""`modules.functional` of the reference (modules/functional/__init__.py:1-7): same ten names, plus the fused criteria
(cross_entropy, cross_entropy_is_fused: csrc/xent.hip; dml_pair_loss, dml_pair_loss_is_fused, kl_loss_is_fused: csrc/dml.hip;
lovasz_softmax, lovasz_softmax_is_fused, lovasz_softmax_parts: csrc/lovasz.hip) and the sparse voxel
operators (SparseMap, sparse_map, sparse_gather, sparse_scatter, sparse_conv3d, sparse_conv3d_reference, sparse_default_cap:
csrc/sparse.hip)."""
from .ball_query import ball_query
from .devoxelization import trilinear_devoxelize
from .grouping import grouping
from .interpolatation import nearest_neighbor_interpolate
from .loss import (kl_loss, kl_loss_is_fused, huber_loss, cross_entropy, cross_entropy_is_fused, dml_pair_loss,
                   dml_pair_loss_is_fused, lovasz_softmax, lovasz_softmax_is_fused, lovasz_softmax_parts)
from .sampling import gather, furthest_point_sample, logits_mask
from .sparse import (SparseMap, sparse_conv3d, sparse_conv3d_reference, sparse_default_cap, sparse_gather, sparse_map,
                     sparse_scatter)
from .voxelization import avg_voxelize

__all__ = ['ball_query', 'trilinear_devoxelize', 'grouping', 'nearest_neighbor_interpolate', 'kl_loss',
           'huber_loss', 'gather', 'furthest_point_sample', 'logits_mask', 'avg_voxelize', 'cross_entropy',
           'cross_entropy_is_fused', 'kl_loss_is_fused', 'dml_pair_loss', 'dml_pair_loss_is_fused',
           'lovasz_softmax', 'lovasz_softmax_is_fused', 'lovasz_softmax_parts', 'SparseMap', 'sparse_map', 'sparse_gather',
           'sparse_scatter', 'sparse_conv3d', 'sparse_conv3d_reference', 'sparse_default_cap']
