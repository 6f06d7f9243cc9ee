"""The reference's view tools (python/depthmotionnet/dataset_tools/view_tools.py, view_tools_cython.pyx) on the GPU.

compute_visible_points_mask, compute_depth_ratios and check_depth_consistency have the reference's signatures, assertions and return
types; the per-pixel loop runs in demon_amd/csrc/viewgeom.hip and returns the reference's masks and ratios bit for bit.
view_pair_counts / consistent_pairs are the batched form the mining loop of dataset_tools/sun3d_utils.py:186-212 wants: the depth maps
of a sequence are uploaded once, many ordered pairs are tested per launch, and only four integer counts per pair come back.

One deviation: the reference reads the second depth map with bounds checks off, and a projection that rounds to row H2 reads past the
array.  Here such a lookup is "no ratio" (NaN).

The module-level functions run on ONE ops-only context per process, created on first use on device 0 (DemonContext.ops_only(0)), and kept until
release() or the end of the process; it holds a stream and no device buffers between calls.  To use another device or to control the lifetime, call DemonContext.view_pair / view_pairs on a context of your own."""
from collections import namedtuple

import numpy as np

__all__ = ["View", "compute_visible_points_mask", "compute_depth_ratios", "check_depth_consistency", "view_pair_counts", "consistent_pairs"]

View = namedtuple("View", ["R", "t", "K", "image", "depth", "depth_metric"])   # dataset_tools/view.py:25

_ctx = None


def _context():
    """one ops-only context per process, created on first use (device 0)"""
    global _ctx
    if _ctx is None:
        from .engine import DemonContext
        _ctx = DemonContext.ops_only(0)
    return _ctx


def release():
    """closes the process-wide context (the next call creates a new one)"""
    global _ctx
    if _ctx is not None:
        _ctx.close()
        _ctx = None


def projection_matrix(view2):
    """P2 exactly as view_tools_cython.pyx:81-84 and :95-98 write it: R and t stored into a float32 [3,4] array, then K.dot, then
    astype(float32)"""
    P2 = np.empty((3, 4), dtype=np.float32)
    P2[:, 0:3] = view2.R
    P2[:, 3:4] = view2.t.reshape((3, 1))
    P2 = view2.K.dot(P2)
    return P2.astype(np.float32)


def _camera1(view1):
    """view_tools_cython.pyx:95-97"""
    return view1.K.astype(np.float32), view1.R.astype(np.float32), view1.t.astype(np.float32)


def _depth32(depth, name):
    depth = np.asarray(depth)
    if depth.dtype != np.float32 or depth.ndim != 2:      # the compiled routine takes np.ndarray[np.float32_t, ndim=2] and nothing else
        raise ValueError("%s must be a 2-d float32 array, not %s %s" % (name, depth.dtype, depth.shape))
    return depth


def ratio_thresholds(depth_ratio_threshold):
    """view_tools.py:82-83; the comparison of :90 is one of a float32 array with a Python float, i.e. with the threshold rounded to
    float32"""
    lo = min(depth_ratio_threshold, 1 / depth_ratio_threshold)
    hi = max(depth_ratio_threshold, 1 / depth_ratio_threshold)
    return np.float32(lo), np.float32(hi)


def counts_consistent(counts, pixels, min_valid_threshold=0.5, min_depth_consistent=0.7):
    """the two tests of view_tools.py:87-92 on the integer counts of one ordered pair (counts[2] finite ratios, counts[3] of them
    within the thresholds, `pixels` = dr.size); no finite ratio means not consistent"""
    n_ratio, n_cons = int(counts[2]), int(counts[3])
    if n_ratio / pixels < min_valid_threshold:
        return False
    if n_ratio == 0 or n_cons / n_ratio < min_depth_consistent:
        return False
    return True


def compute_visible_points_mask(view1, view2, borderx=0, bordery=0):
    """Computes a mask of the pixels in view1 that are visible in view2

    view1, view2: View namedtuples; borderx, bordery: int borders in which points are considered invalid.
    Returns a uint8 mask of valid points (view_tools.py:23-42, view_tools_cython.pyx:62-102)."""
    assert view1.depth_metric == 'camera_z', "Depth metric must be 'camera_z'"
    if view2.depth is None:
        width2, height2 = view1.depth.shape[1], view1.depth.shape[0]
    else:
        width2, height2 = view2.depth.shape[1], view2.depth.shape[0]
    K1, R1, t1 = _camera1(view1)
    mask, _, _ = _context().view_pair(_depth32(view1.depth, "view1.depth"), None, K1, R1, t1, projection_matrix(view2), width2=width2, height2=height2,
                                      borderx=int(borderx), bordery=int(bordery), want_mask=True, want_ratios=False)
    return mask


def compute_depth_ratios(view1, view2):
    """Projects each point defined in view1 to view2 and computes the ratio of the depth value of the projected point and the
    stored depth value in view2 (view_tools.py:45-59, view_tools_cython.pyx:164-191).

    Returns the scale value for view2 relative to view1: float32 [h,w], NaN where there is none."""
    assert view1.depth_metric == 'camera_z', "Depth metric must be 'camera_z'"
    assert view2.depth_metric == 'camera_z', "Depth metric must be 'camera_z'"
    K1, R1, t1 = _camera1(view1)
    _, ratios, _ = _context().view_pair(_depth32(view1.depth, "view1.depth"), _depth32(view2.depth, "view2.depth"), K1, R1, t1, projection_matrix(view2),
                                        want_mask=False, want_ratios=True)
    return ratios


def check_depth_consistency(view, rest_of_the_views, depth_ratio_threshold=0.9, min_valid_threshold=0.5, min_depth_consistent=0.7):
    """Checks if the depth of view is consistent with the rest_of_the_views (view_tools.py:62-94)

    depth_ratio_threshold: the allowed minimum depth ratio; min_valid_threshold: ratio of pixels that should have consistent depth
    values with the rest_of_the_views; min_depth_consistent: ratio of depth consistent pixels with respect to the number of valid
    depth ratios.  Returns True if the depth is consistent.  Only the four counts of each pair leave the GPU."""
    lo, hi = ratio_thresholds(depth_ratio_threshold)
    rest = list(rest_of_the_views)
    counts = None
    if len(rest) > 1 and all(v.depth is not None and np.shape(v.depth) == np.shape(view.depth) for v in rest):
        # maps of one size: one upload and two launches for all of them instead of one trip per view
        depth, pairs, K1, R1, t1, P2 = _pair_arrays([view] + rest, [(0, j + 1) for j in range(len(rest))], check_metric=False)
        counts, _, _ = _context().view_pairs(depth, pairs, K1, R1, t1, P2, ratio_lo=lo, ratio_hi=hi)
    else:
        K1, R1, t1 = _camera1(view)
    for j, v in enumerate(rest):
        assert view.depth_metric == 'camera_z', "Depth metric must be 'camera_z'"
        assert v.depth_metric == 'camera_z', "Depth metric must be 'camera_z'"
        if counts is not None:
            c = counts[j]
        else:
            _, _, c = _context().view_pair(_depth32(view.depth, "view.depth"), _depth32(v.depth, "depth"), K1, R1, t1, projection_matrix(v),
                                           ratio_lo=lo, ratio_hi=hi, want_mask=False, want_ratios=False)
        if not counts_consistent(c, view.depth.size, min_valid_threshold, min_depth_consistent):
            return False
    return True


def _pair_arrays(views, pairs, check_metric=True):
    """the per-pair float32 inputs of demon_op_view_pairs, built view by view with the reference's casts"""
    pairs = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    for v in views if check_metric else ():
        assert v.depth_metric == 'camera_z', "Depth metric must be 'camera_z'"
    shape = views[0].depth.shape
    if any(_depth32(v.depth, "depth").shape != shape for v in views):
        raise ValueError("the views of a set must have depth maps of one size")
    if pairs.size and (pairs.min() < 0 or pairs.max() >= len(views)):
        raise ValueError("a pair names a view outside the set")
    cams = [_camera1(v) for v in views]
    P2s = [projection_matrix(v) for v in views]
    K1 = np.stack([cams[i][0] for i in pairs[:, 0]]).reshape(-1, 9) if pairs.size else np.zeros((0, 9), np.float32)
    R1 = np.stack([cams[i][1] for i in pairs[:, 0]]).reshape(-1, 9) if pairs.size else np.zeros((0, 9), np.float32)
    t1 = np.stack([cams[i][2].reshape(3) for i in pairs[:, 0]]) if pairs.size else np.zeros((0, 3), np.float32)
    P2 = np.stack([P2s[j] for j in pairs[:, 1]]).reshape(-1, 12) if pairs.size else np.zeros((0, 12), np.float32)
    depth = np.stack([v.depth for v in views])
    return depth, pairs, K1, R1, t1, P2


def view_pair_counts(views, pairs, depth_ratio_threshold=0.9, borderx=0, bordery=0, with_mask=False, with_ratios=False):
    """views: list of View with depth maps of one size; pairs: [n,2] indices (view 1, view 2) into it.
    Returns int32 [n,4] per ordered pair: pixels of view 1 with valid depth | visible in view 2 (compute_visible_points_mask) |
    finite depth ratios (compute_depth_ratios) | finite ratios strictly between min and max of (threshold, 1 / threshold).
    with_mask / with_ratios: returns (counts, mask [n,h,w] uint8 or None, ratios [n,h,w] float32 or None) instead."""
    depth, pairs, K1, R1, t1, P2 = _pair_arrays(views, pairs)
    lo, hi = ratio_thresholds(depth_ratio_threshold)
    if pairs.shape[0] == 0:
        counts, mask, ratios = np.zeros((0, 4), np.int32), None, None
    else:
        counts, mask, ratios = _context().view_pairs(depth, pairs, K1, R1, t1, P2, borderx=int(borderx), bordery=int(bordery), ratio_lo=lo, ratio_hi=hi,
                                                     want_mask=with_mask, want_ratios=with_ratios)
    return (counts, mask, ratios) if with_mask or with_ratios else counts


def consistent_pairs(views, pairs, depth_ratio_threshold=0.9, min_valid_threshold=0.5, min_depth_consistent=0.7):
    """check_depth_consistency(views[i], [views[j]], ...) for every ordered pair (i, j) of `pairs`, in one call: bool [n]"""
    counts = view_pair_counts(views, pairs, depth_ratio_threshold)
    pixels = views[0].depth.size if len(views) else 1
    return np.array([counts_consistent(c, pixels, min_valid_threshold, min_depth_consistent) for c in counts], dtype=bool)
