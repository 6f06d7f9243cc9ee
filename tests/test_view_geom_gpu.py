"""The view tools on the GPU (demon_amd/csrc/viewgeom.hip) against what the reference's compiled routines returned
(tests/golden/view_geometry.npz; tests/test_view_geom_cpu.py holds the numpy restatement to the same file).

There is no tolerance in this file: masks are compared byte for byte, ratios as bit patterns, counts as integers.  Every output buffer
is pre-filled with 0xCD bytes, so a pixel the kernel does not write shows.  The kernel's chunk is 1024 pixels (256 lanes x 4 pixels):
5x7 is less than a wave, 16x24 less than a chunk, 33x65 three chunks with a ragged tail and planes that are not 16-byte aligned from the
second pair on, 17x130 rows longer than a wave's span, 48x64 exactly three chunks."""
import ctypes
import hashlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import view_geom_ref as ref  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "view_geometry.npz")
FILL = 0xCD


def _case_names():
    with np.load(GOLDEN) as z:
        return [str(c) for c in z["cases"]]


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def ops_ctx():
    from demon_amd import DemonContext
    ctx = DemonContext.ops_only(0)
    yield ctx
    ctx.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def _u8p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


def _filled(shape, dtype):
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = FILL
    return a


def _views(g, name):
    from demon_amd.view_tools import View
    get = lambda k: g[name + "." + k]   # noqa: E731
    v1 = View(R=get("R1"), t=get("t1"), K=get("K1"), image=None, depth=get("depth1"), depth_metric="camera_z")
    v2 = View(R=get("R2"), t=get("t2"), K=get("K2"), image=None, depth=get("depth2"), depth_metric="camera_z")
    return v1, v2


def _f32c(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ---- demon_op_view_pair: every golden case, straight through the C entry ---------------------------------------------------------------
@pytest.mark.parametrize("name", _case_names())
def test_view_pair_entry_equals_the_reference(ops_ctx, golden, name):
    from demon_amd import view_tools
    g = golden
    v1, v2 = _views(g, name)
    h, w = v1.depth.shape
    H2, W2 = v2.depth.shape
    bx, by = (int(v) for v in g[name + ".border"])
    lo, hi = view_tools.ratio_thresholds(float(g[name + ".threshold"]))
    K1, R1, t1, P2 = _f32c(v1.K), _f32c(v1.R), _f32c(v1.t), view_tools.projection_matrix(v2)
    d1, d2 = _f32c(v1.depth), _f32c(v2.depth)
    for want_mask, want_ratios in ((True, True), (True, False), (False, True), (False, False)):
        mask, ratios, counts = _filled((h, w), np.uint8), _filled((h, w), np.float32), _filled(4, np.int32)
        rc = ops_ctx.lib.demon_op_view_pair(ops_ctx.h, _ip(counts), _u8p(mask) if want_mask else None, _fp(ratios) if want_ratios else None, _fp(d1), _fp(d2),
                                            _fp(K1), _fp(R1), _fp(t1), _fp(P2), h, w, H2, W2, bx, by, float(lo), float(hi))
        assert rc == 0, ops_ctx.lib.demon_last_error(ops_ctx.h).decode()
        assert np.array_equal(counts, g[name + ".counts"]), (name, counts, g[name + ".counts"])
        if want_mask:
            assert np.array_equal(mask, g[name + ".mask"]), name
        else:
            assert (mask == FILL).all()
        if want_ratios:
            assert np.array_equal(_bits(ratios), _bits(g[name + ".ratios"])), name
        else:
            assert (ratios.view(np.uint8) == FILL).all()


@pytest.mark.parametrize("name", _case_names())
def test_python_functions_equal_the_reference(golden, name):
    from demon_amd import view_tools
    g = golden
    v1, v2 = _views(g, name)
    bx, by = (int(v) for v in g[name + ".border"])
    try:
        mask = view_tools.compute_visible_points_mask(v1, v2, bx, by)
        assert mask.dtype == np.uint8 and np.array_equal(mask, g[name + ".mask"])
        ratios = view_tools.compute_depth_ratios(v1, v2)
        assert ratios.dtype == np.float32 and np.array_equal(_bits(ratios), _bits(g[name + ".ratios"]))
    finally:
        view_tools.release()


def test_mask_without_a_second_depth_map(ops_ctx, golden):
    """view2.depth is None: width2 / height2 are view 1's (view_tools_cython.pyx:86-88); no ratios, ratio counts 0"""
    from demon_amd import view_tools
    g = golden
    name = "general_33x65"
    v1, v2 = _views(g, name)
    P2 = ref.projection_matrix(v2.K, v2.R, v2.t).astype(np.float32)
    h, w = v1.depth.shape
    want_m, _, want_c = ref.view_geometry(v1.depth, None, v1.K, v1.R, v1.t, P2, width2=w, height2=h, borderx=2, bordery=1)
    try:
        got = view_tools.compute_visible_points_mask(v1, v2._replace(depth=None), 2, 1)
    finally:
        view_tools.release()
    assert np.array_equal(got, want_m) and want_m.any() and not want_m.all()
    mask, ratios, counts = ops_ctx.view_pair(v1.depth, None, _f32c(v1.K), _f32c(v1.R), _f32c(v1.t), P2, width2=w, height2=h, borderx=2, bordery=1, want_ratios=False)
    assert ratios is None and np.array_equal(mask, want_m) and np.array_equal(counts, want_c) and counts[2] == 0 and counts[3] == 0
    # ratios without a second map: an error, nothing written
    out = _filled((h, w), np.float32)
    rc = ops_ctx.lib.demon_op_view_pair(ops_ctx.h, None, None, _fp(out), _fp(_f32c(v1.depth)), None, _fp(_f32c(v1.K)), _fp(_f32c(v1.R)), _fp(_f32c(v1.t)), _fp(P2),
                                        h, w, h, w, 0, 0, 0.0, 1.0)
    assert rc == -1 and ops_ctx.lib.demon_last_error(ops_ctx.h).decode() and (out.view(np.uint8) == FILL).all()


# ---- demon_op_view_pairs: the 20 ordered pairs of the 5-view set -------------------------------------------------------------------------
def _set_inputs(g):
    from demon_amd import view_tools
    views = [view_tools.View(R=g["set.R"][i], t=g["set.t"][i], K=g["set.K"], image=None, depth=g["set.depth"][i], depth_metric="camera_z") for i in range(5)]
    return views, view_tools._pair_arrays(views, g["set.pairs"])


@pytest.mark.parametrize("form", ["counts", "mask", "ratios", "full"])
def test_view_pairs_entry_on_the_set(ops_ctx, golden, form):
    from demon_amd import view_tools
    g = golden
    _, (depth, pairs, K1, R1, t1, P2) = _set_inputs(g)
    V, h, w = depth.shape
    n = pairs.shape[0]
    lo, hi = view_tools.ratio_thresholds(float(g["set.threshold"]))
    mask, ratios, counts = _filled((n, h, w), np.uint8), _filled((n, h, w), np.float32), _filled((n, 4), np.int32)
    rc = ops_ctx.lib.demon_op_view_pairs(ops_ctx.h, _ip(counts), _u8p(mask) if form in ("mask", "full") else None, _fp(ratios) if form in ("ratios", "full") else None,
                                         _fp(depth), _ip(pairs), _fp(K1), _fp(R1), _fp(t1), _fp(P2), V, n, h, w, 0, 0, float(lo), float(hi))
    assert rc == 0, ops_ctx.lib.demon_last_error(ops_ctx.h).decode()
    assert np.array_equal(counts, g["set.counts"])
    if form in ("mask", "full"):
        assert np.array_equal(mask, g["set.mask"])
    else:
        assert (mask == FILL).all()
    if form in ("ratios", "full"):
        assert np.array_equal(_bits(ratios[g["set.ratios_stored"]]), _bits(g["set.ratios"]))
        assert hashlib.sha1(ratios.tobytes()).hexdigest() == str(g["set.ratios_sha1"])
    else:
        assert (ratios.view(np.uint8) == FILL).all()


def test_pair_index_out_of_range_is_an_error(ops_ctx, golden):
    from demon_amd import view_tools
    g = golden
    _, (depth, pairs, K1, R1, t1, P2) = _set_inputs(g)
    V, h, w = depth.shape
    n = pairs.shape[0]
    for bad in ((7, 1, V), (12, 0, -1), (19, 1, 1 << 20)):
        p = pairs.copy()
        p[bad[0], bad[1]] = bad[2]
        mask, ratios, counts = _filled((n, h, w), np.uint8), _filled((n, h, w), np.float32), _filled((n, 4), np.int32)
        rc = ops_ctx.lib.demon_op_view_pairs(ops_ctx.h, _ip(counts), _u8p(mask), _fp(ratios), _fp(depth), _ip(p), _fp(K1), _fp(R1), _fp(t1), _fp(P2), V, n, h, w,
                                             0, 0, 0.0, 1.0)
        assert rc == -1 and "pair" in ops_ctx.lib.demon_last_error(ops_ctx.h).decode(), bad
        assert (mask == FILL).all() and (ratios.view(np.uint8) == FILL).all() and (counts.view(np.uint8) == FILL).all(), bad
    for kw in (dict(n=0), dict(h=0), dict(V=0)):
        a = dict(V=V, n=n, h=h)
        a.update(kw)
        rc = ops_ctx.lib.demon_op_view_pairs(ops_ctx.h, None, None, None, _fp(depth), _ip(pairs), _fp(K1), _fp(R1), _fp(t1), _fp(P2), a["V"], a["n"], a["h"], w,
                                             0, 0, 0.0, 1.0)
        assert rc == -1, kw
    # the context still works
    got = ops_ctx.view_pairs(depth, pairs, K1, R1, t1, P2, ratio_lo=view_tools.ratio_thresholds(0.9)[0], ratio_hi=view_tools.ratio_thresholds(0.9)[1])[0]
    assert np.array_equal(got, g["set.counts"])


def test_batched_python_forms_and_decisions(golden):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "python"))
    from depthmotionnet.dataset_tools import view_tools
    g = golden
    views, _ = _set_inputs(g)
    thr, mv, mc = float(g["set.threshold"]), float(g["set.min_valid_threshold"]), float(g["set.min_depth_consistent"])
    try:
        counts = view_tools.view_pair_counts(views, g["set.pairs"], thr)
        assert counts.dtype == np.int32 and np.array_equal(counts, g["set.counts"])
        counts, mask, ratios = view_tools.view_pair_counts(views, g["set.pairs"], thr, with_mask=True, with_ratios=True)
        assert np.array_equal(mask, g["set.mask"]) and hashlib.sha1(ratios.tobytes()).hexdigest() == str(g["set.ratios_sha1"])
        ok = view_tools.consistent_pairs(views, g["set.pairs"], thr, mv, mc)
        assert ok.dtype == bool and np.array_equal(ok, g["set.pair_consistent"])
        rest = [int(j) for j in g["set.rest"]]
        got = [view_tools.check_depth_consistency(views[i], [views[j] for j in rest if j != i], thr, mv, mc) for i in range(5)]
        assert got == [bool(v) for v in g["set.view_consistent"]]
        assert view_tools.view_pair_counts(views, np.zeros((0, 2), np.int32)).shape == (0, 4)
        with pytest.raises(ValueError):
            view_tools.view_pair_counts(views, [[0, 5]])
    finally:
        import demon_amd.view_tools
        demon_amd.view_tools.release()


def test_depthmask_of_the_evaluation_protocol(golden):
    """evaluation.invalidate_points_not_visible_in_second_image against the restatement fed the same R"""
    from demon_amd import evaluation, view_tools
    rng = np.random.default_rng(3)
    h, w = 48, 64
    inv = rng.uniform(0.2, 1.0, (1, h, w)).astype(np.float32)
    inv[0, ::7, ::5] = 0.0
    inv[0, 3, 3] = np.nan
    motion = np.array([0.02, -0.11, 0.03, -0.4, 0.05, 0.1])
    for intrinsics in (None, np.array([[0.8, 1.1, 0.45, 0.55]], np.float32)):
        depth = inv.copy()
        try:
            evaluation.invalidate_points_not_visible_in_second_image(depth, motion, intrinsics)
        finally:
            view_tools.release()
        k = (np.array([0.891, 1.188, 0.5, 0.5], np.float32) if intrinsics is None else intrinsics.squeeze()).astype(np.float64)
        K = np.array([k[0] * w, 0, k[2] * w, 0, k[1] * h, k[3] * h, 0, 0, 1]).reshape(3, 3)
        R = evaluation._rotmat(motion[:3])
        with np.errstate(divide="ignore"):
            abs_depth = 1 / inv[0]
        P2 = ref.projection_matrix(K, R, motion[3:]).astype(np.float32)
        want_mask, _, _ = ref.view_geometry(abs_depth, None, K, np.eye(3), np.zeros(3), P2, width2=w, height2=h)
        want = inv.copy()
        want[0][want_mask == 0] = np.nan
        assert np.array_equal(_bits(depth), _bits(want)) and want_mask.any() and not want_mask.all()


def test_one_host_buffer_for_both_views_of_a_single_pair(ops_ctx, golden):
    """demon_op_view_pair with depth1 and depth2 pointing at the same host buffer, view 2 being the larger reading of it (8x5 = 40
    floats, of which view 1 is the first 5x7 = 35): the second map is uploaded in its own size, not taken from view 1's upload"""
    from demon_amd import view_tools
    g = golden
    v1, v2 = _views(g, "general_5x7")
    (h, w), (H2, W2) = v1.depth.shape, v2.depth.shape
    assert H2 * W2 > h * w
    buf = _f32c(v2.depth).reshape(-1).copy()
    buf[:h * w] = _f32c(v1.depth).reshape(-1)
    d1, d2 = buf[:h * w].reshape(h, w), buf.reshape(H2, W2)
    lo, hi = view_tools.ratio_thresholds(0.9)
    K1, R1, t1, P2 = _f32c(v1.K), _f32c(v1.R), _f32c(v1.t), view_tools.projection_matrix(v2)
    want_m, want_r, want_c = ref.view_geometry(d1, d2, K1, R1, t1, P2, lo=lo, hi=hi)
    assert np.isfinite(want_r).any()
    mask, ratios, counts = _filled((h, w), np.uint8), _filled((h, w), np.float32), _filled(4, np.int32)
    rc = ops_ctx.lib.demon_op_view_pair(ops_ctx.h, _ip(counts), _u8p(mask), _fp(ratios), _fp(buf), _fp(buf), _fp(K1), _fp(R1), _fp(t1), _fp(P2), h, w, H2, W2,
                                        0, 0, float(lo), float(hi))
    assert rc == 0, ops_ctx.lib.demon_last_error(ops_ctx.h).decode()
    assert np.array_equal(mask, want_m) and np.array_equal(_bits(ratios), _bits(want_r)) and np.array_equal(counts, want_c)


def test_check_depth_consistency_on_one_view_and_on_maps_of_two_sizes(golden):
    """the two routes of check_depth_consistency that the set test does not take (there, four maps of one size go out as one call):
    a single other view, and other views whose maps differ in size, each through the single-pair entry.  The decisions are the
    restatement's, view by view, stopping at the first False like the reference's loop"""
    from demon_amd import view_tools
    g = golden
    views, _ = _set_inputs(g)
    thr, mv, mc = float(g["set.threshold"]), float(g["set.min_valid_threshold"]), float(g["set.min_depth_consistent"])
    lo, hi = view_tools.ratio_thresholds(thr)

    def want(v, rest):
        for o in rest:
            c = ref.view_geometry(v.depth, o.depth, v.K, v.R, v.t, ref.projection_matrix(o.K, o.R, o.t).astype(np.float32), lo=lo, hi=hi)[2]
            if not view_tools.counts_consistent(c, v.depth.size, mv, mc):
                return False
        return True

    cropped = [v._replace(depth=np.ascontiguousarray(v.depth[:-2, :-3])) for v in views]
    try:
        single = [view_tools.check_depth_consistency(views[i], [views[j]], thr, mv, mc) for i in range(5) for j in range(5) if i != j]
        assert single == [bool(v) for v in g["set.pair_consistent"]] and any(single) and not all(single)
        for i in range(5):
            rest = [cropped[j] if j % 2 else views[j] for j in range(5) if j != i]
            assert view_tools.check_depth_consistency(views[i], rest, thr, mv, mc) == want(views[i], rest), i
        assert view_tools.check_depth_consistency(views[0], [], thr, mv, mc) is True
    finally:
        view_tools.release()
