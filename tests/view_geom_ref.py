"""float32 numpy restatement of the reference's view tools (python/depthmotionnet/dataset_tools/view_tools_cython.pyx:9-58
`_compute_visible_points_mask`, :108-159 `_compute_depth_ratios`) and of the counts check_depth_consistency (view_tools.py:82-94)
decides on.  Every operation is ONE float32 rounding, evaluated left to right as the compiled loop does on baseline x86-64 (no FMA):

    X = (d * (px - cx)) / fx - t0 ...        q = (RT0 * X + RT1 * Y) + RT2 * Z        p = ((P0 * q0 + P1 * q1) + P2 * q2) + P3 * 1

The lookup rounds half to even (Python's round) and clamps to [0, W2] / [0, H2] -- not W2 - 1 / H2 - 1: the reference reads the
contiguous map with bounds checks off, so x2 == W2 is the first pixel of the next row, and a flat index at or past H2 * W2 is outside
the map, which here gives "no ratio" (what the reference returns when the memory behind the map holds NaN).

`mutant` switches ONE deliberate deviation on; tests/test_view_geom_cpu.py shows that the golden cases reject each of them."""
import numpy as np

F = np.float32
NAN_BITS = 0x7FC00000
MUTANTS = ("roundf", "clamp_minus_one", "no_wrap", "fma_projection", "border_ge", "double_thresholds", "reciprocal_fx")


def projection_matrix(K2, R2, t2):
    """P2 as view_tools_cython.pyx:81-84 / :180-183 builds it, before the astype(float32) of :98 / :191"""
    P2 = np.empty((3, 4), dtype=np.float32)
    P2[:, 0:3] = R2
    P2[:, 3:4] = np.asarray(t2).reshape((3, 1))
    return np.asarray(K2).dot(P2)


def thresholds(depth_ratio_threshold):
    """view_tools.py:82-83, as Python floats.  view_geometry rounds them to float32, which is what numpy's comparison of a float32
    array with a Python float does (view_tools.py:90)"""
    lo = min(depth_ratio_threshold, 1 / depth_ratio_threshold)
    hi = max(depth_ratio_threshold, 1 / depth_ratio_threshold)
    return lo, hi


def _fma(a, b, c):
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(F)


def view_geometry(depth1, depth2, K1, R1, t1, P2, width2=None, height2=None, borderx=0, bordery=0, lo=0.0, hi=np.inf, mutant=None):
    """depth1 [h,w]; depth2 [H2,W2] or None (then width2 / height2 size the mask and there are no ratios); K1, R1 [3,3], t1 [3],
    P2 [3,4].  Returns (mask uint8 [h,w], ratios float32 [h,w] with NaN 0x7fc00000 where there is none,
    counts int32 [4] = valid1, visible, finite ratios, finite ratios with lo < ratio < hi)."""
    assert mutant is None or mutant in MUTANTS
    d = np.ascontiguousarray(depth1, dtype=F)
    h, w = d.shape
    K1, R1, t1, P2 = (np.asarray(a).astype(F) for a in (K1, R1, t1, P2))
    if depth2 is not None:
        depth2 = np.ascontiguousarray(depth2, dtype=F)
        H2, W2 = depth2.shape
        width2, height2 = (W2, H2) if width2 is None else (width2, height2)
    RT = R1.transpose()
    with np.errstate(all="ignore"):
        valid = np.isfinite(d) & (d > 0)
        px = (np.arange(w, dtype=F) + F(0.5))[None, :]
        py = (np.arange(h, dtype=F) + F(0.5))[:, None]
        if mutant == "reciprocal_fx":
            X = (d * (px - K1[0, 2])) * (F(1) / K1[0, 0])
            Y = (d * (py - K1[1, 2])) * (F(1) / K1[1, 1])
        else:
            X = (d * (px - K1[0, 2])) / K1[0, 0]
            Y = (d * (py - K1[1, 2])) / K1[1, 1]
        X = X - t1[0]
        Y = Y - t1[1]
        Z = d - t1[2]
        q = [(RT[i, 0] * X + RT[i, 1] * Y) + RT[i, 2] * Z for i in range(3)]
        if mutant == "fma_projection":
            p = [_fma(q[2], P2[i, 2], _fma(q[1], P2[i, 1], P2[i, 0] * q[0])) + P2[i, 3] * F(1) for i in range(3)]
        else:
            p = [((P2[i, 0] * q[0] + P2[i, 1] * q[1]) + P2[i, 2] * q[2]) + P2[i, 3] * F(1) for i in range(3)]
        front = valid & (p[2] > 0)
        u = p[0] / p[2]
        v = p[1] / p[2]
        bx0, by0, bx1, by1 = F(borderx), F(bordery), F(int(width2) - int(borderx)), F(int(height2) - int(bordery))
        if mutant == "border_ge":
            mask = front & (u >= bx0) & (v >= by0) & (u <= bx1) & (v <= by1)
        else:
            mask = front & (u > bx0) & (v > by0) & (u < bx1) & (v < by1)
        ratios = np.full((h, w), np.nan, dtype=F)
        assert ratios.view(np.uint32)[0, 0] == NAN_BITS
        if depth2 is not None:
            inside = front & (u > 0) & (v > 0) & (u < F(W2)) & (v < F(H2))
            us, vs = np.where(inside, u, F(0)), np.where(inside, v, F(0))
            rnd = (lambda a: np.floor(a + F(0.5))) if mutant == "roundf" else np.rint    # (a >= 0 here; a + 0.5 is exact below 2^22)
            x2, y2 = rnd(us).astype(np.int64), rnd(vs).astype(np.int64)
            if mutant == "clamp_minus_one":
                x2, y2 = np.clip(x2, 0, W2 - 1), np.clip(y2, 0, H2 - 1)
            else:
                x2, y2 = np.clip(x2, 0, W2), np.clip(y2, 0, H2)
            idx = y2 * W2 + x2
            readable = inside & (idx < H2 * W2)
            if mutant == "no_wrap":
                readable &= x2 < W2
            d2 = depth2.reshape(-1)[np.where(readable, idx, 0)]
            hit = readable & np.isfinite(d2) & (d2 > 0)
            ratios[hit] = (p[2] / d2)[hit]
        fin = np.isfinite(ratios)
        if mutant == "double_thresholds":
            cons = fin & (ratios.astype(np.float64) > float(lo)) & (ratios.astype(np.float64) < float(hi))
        else:
            cons = fin & (ratios > F(lo)) & (ratios < F(hi))
    counts = np.array([valid.sum(), mask.sum(), fin.sum(), cons.sum()], np.int32)
    return mask.astype(np.uint8), ratios, counts


def consistent(counts, pixels, min_valid_threshold=0.5, min_depth_consistent=0.7):
    """the two tests of view_tools.py:87-92 on one pair's counts; no finite ratio is not consistent"""
    n_ratio, n_cons = int(counts[2]), int(counts[3])
    if n_ratio / pixels < min_valid_threshold:
        return False
    if n_ratio == 0 or n_cons / n_ratio < min_depth_consistent:
        return False
    return True
