"""PointNet++ set-abstraction ops and modules on the device: the counterpart of the reference's ``pointnet2_ops`` package
(``from pointnet2_ops import pointnet2_utils, pointnet2_modules``).  Importing it needs torch but no GPU."""
from . import pointnet2_models, pointnet2_modules, pointnet2_train, pointnet2_utils, resampled_dataset  # noqa: F401
from .pointnet2_models import PointNet2ClassificationMSG, PointNet2ClassificationSSG, PointNet2SemSegMSG, PointNet2SemSegSSG  # noqa: F401
from .pointnet2_utils import furthest_point_sample_np  # noqa: F401
