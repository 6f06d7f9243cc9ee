"""Drop-in module path of the reference's python/depthmotionnet/dataset_tools/view_tools.py: compute_visible_points_mask,
compute_depth_ratios and check_depth_consistency with the reference's signatures, computed on the GPU (demon_amd/view_tools.py), plus
the batched forms view_pair_counts / consistent_pairs.  adjust_intrinsics, resize_view and the viewers are not provided."""
from demon_amd.view_tools import (View, check_depth_consistency, compute_depth_ratios, compute_visible_points_mask,  # noqa: F401
                                  consistent_pairs, view_pair_counts)

__all__ = ["View", "compute_visible_points_mask", "compute_depth_ratios", "check_depth_consistency", "view_pair_counts", "consistent_pairs"]
