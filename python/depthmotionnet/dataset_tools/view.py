"""Drop-in module path of the reference's python/depthmotionnet/dataset_tools/view.py: the View namedtuple (R t K image depth
depth_metric).  Reading and writing views from HDF5 groups is not provided."""
from demon_amd.view_tools import View  # noqa: F401

__all__ = ["View"]
