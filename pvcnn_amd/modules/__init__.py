"""Host-side mirror of the reference's `modules` package (modules/__init__.py:1-8): the same
ten public classes with the same constructor / forward signatures and sub-module names
(state_dict keys), implemented over the gfx950 native backend; CrossEntropyLoss (nn.CrossEntropyLoss on the fused criterion),
DMLPairLoss (the criterion pair of a deep-mutual-learning step), LovaszSoftmax (the IoU surrogate per cloud) and CrossEntropyLovasz
(the two added) are this package's own, and so is SparseConv3d (the submanifold sparse convolution on the active voxels)."""
from .ball_query import BallQuery
from .frustum import FrustumPointNetLoss
from .loss import CrossEntropyLoss, CrossEntropyLovasz, DMLPairLoss, KLLoss, LovaszSoftmax
from .pointnet import PointNetAModule, PointNetSAModule, PointNetFPModule
from .pvconv import PVConv
from .se import SE3d
from .shared_mlp import SharedMLP
from .sparse import SparseConv3d
from .voxelization import Voxelization

__all__ = ['BallQuery', 'CrossEntropyLoss', 'CrossEntropyLovasz', 'DMLPairLoss', 'FrustumPointNetLoss', 'KLLoss', 'LovaszSoftmax',
           'PointNetAModule', 'PointNetSAModule', 'PointNetFPModule', 'PVConv', 'SE3d', 'SharedMLP', 'SparseConv3d', 'Voxelization']
