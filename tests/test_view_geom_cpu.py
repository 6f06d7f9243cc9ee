"""CPU side of the view tools (no GPU needed): the float32 numpy restatement (tests/view_geom_ref.py) against what the reference's
compiled routines returned (tests/golden/view_geometry.npz, tools/make_view_geometry_golden.py, and the older sculpture golden), the
host-side decisions of check_depth_consistency, mutants of the restatement that the golden cases must reject, the kernel-source hash,
and the ABI's new symbols.  Masks are compared byte for byte, ratios as bit patterns, counts as integers: there is no tolerance."""
import hashlib
import importlib.util
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import view_geom_ref as ref  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "view_geometry.npz")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def case_names():
    with np.load(GOLDEN) as z:
        return [str(c) for c in z["cases"]]


def run_case(g, name, mutant=None):
    get = lambda k: g[name + "." + k]   # noqa: E731
    P2 = ref.projection_matrix(get("K2"), get("R2"), get("t2")).astype(np.float32)
    lo, hi = ref.thresholds(float(get("threshold")))
    bx, by = (int(v) for v in get("border"))
    return ref.view_geometry(get("depth1"), get("depth2"), get("K1"), get("R1"), get("t1"), P2, borderx=bx, bordery=by, lo=lo, hi=hi, mutant=mutant)


def run_set(g, mutant=None):
    K, R, t, depth = g["set.K"], g["set.R"], g["set.t"], g["set.depth"]
    lo, hi = ref.thresholds(float(g["set.threshold"]))
    res = []
    for i, j in g["set.pairs"]:
        P2 = ref.projection_matrix(K, R[j], t[j]).astype(np.float32)
        res.append(ref.view_geometry(depth[i], depth[j], K, R[i], t[i], P2, lo=lo, hi=hi, mutant=mutant))
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.stack([r[2] for r in res])


def test_golden_file_is_small_and_covers_the_cases(golden):
    g = golden
    assert os.path.getsize(GOLDEN) < 200 * 1024
    names = case_names()
    assert {g[n + ".depth1"].shape for n in names} >= {(5, 7), (16, 24), (33, 65), (48, 64), (17, 130)}
    assert any(g[n + ".depth1"].shape != g[n + ".depth2"].shape for n in names) and any(g[n + ".depth1"].shape == g[n + ".depth2"].shape for n in names)
    assert {tuple(g[n + ".border"]) for n in names} == {(0, 0), (2, 1)}
    for which in ("depth1", "depth2"):
        d = np.concatenate([g[n + "." + which].ravel() for n in names if n.startswith("general")])
        assert np.isnan(d).any() and np.isposinf(d).any() and (d == 0).any() and (d == -1).any()
    tiny = g["denormal.depth1"]
    assert ((tiny > 0) & (tiny < np.finfo(np.float32).tiny)).any()
    assert g["set.depth"].shape == (5, 33, 65) and g["set.pairs"].shape == (20, 2) and len({tuple(p) for p in g["set.pairs"]}) == 20
    assert g["set.pair_consistent"].any() and not g["set.pair_consistent"].all()
    assert g["set.view_consistent"].any() and not g["set.view_consistent"].all()


@pytest.mark.parametrize("name", case_names())
def test_restatement_equals_the_reference_bit_for_bit(golden, name):
    mask, ratios, counts = run_case(golden, name)
    want_m, want_r = golden[name + ".mask"], golden[name + ".ratios"]
    assert mask.dtype == np.uint8 and mask.shape == want_m.shape and np.array_equal(mask, want_m)
    assert ratios.dtype == np.float32 and np.array_equal(_bits(ratios), _bits(want_r))
    assert counts.dtype == np.int32 and np.array_equal(counts, golden[name + ".counts"])
    nan = np.isnan(ratios)
    assert (_bits(ratios)[nan] == ref.NAN_BITS).all()          # a written ratio is never NaN


def test_restatement_equals_the_reference_on_the_set(golden):
    g = golden
    mask, ratios, counts = run_set(g)
    assert np.array_equal(mask, g["set.mask"]) and np.array_equal(counts, g["set.counts"])
    assert np.array_equal(_bits(ratios[g["set.ratios_stored"]]), _bits(g["set.ratios"]))
    assert hashlib.sha1(np.ascontiguousarray(ratios).tobytes()).hexdigest() == str(g["set.ratios_sha1"])


def test_restatement_equals_the_sculpture_golden():
    """the reference's outputs for its own example pair (tests/golden/make_golden.py), all 49 152 pixels"""
    with np.load(os.path.join(ROOT, "tests", "golden", "sculpture_geometry.npz")) as g:
        depth1, depth2, Rt1, Rt2, want_m, want_r = (g[k] for k in ("depth1", "depth2", "Rt1", "Rt2", "visible_mask", "depth_ratios"))
    H, W = depth1.shape
    intr = np.array([0.89115971, 1.18821287, 0.5, 0.5])
    K = np.array([[intr[0] * W, 0, intr[2] * W], [0, intr[1] * H, intr[3] * H], [0, 0, 1]], np.float64)
    P2 = ref.projection_matrix(K, Rt2[:, :3], Rt2[:, 3]).astype(np.float32)
    mask, ratios, counts = ref.view_geometry(depth1, depth2, K, Rt1[:, :3], Rt1[:, 3], P2)
    assert mask.size == 49152 and np.array_equal(mask, want_m) and np.array_equal(_bits(ratios), _bits(want_r))
    assert counts[1] == 38076 and counts[2] == 36354


def test_host_decisions_equal_the_recorded_ones(golden):
    from demon_amd import view_tools
    g = golden
    lo, hi = view_tools.ratio_thresholds(float(g["set.threshold"]))
    assert lo.dtype == np.float32 and (lo, hi) == tuple(np.float32(v) for v in ref.thresholds(float(g["set.threshold"])))
    mv, mc = float(g["set.min_valid_threshold"]), float(g["set.min_depth_consistent"])
    pixels = g["set.depth"][0].size
    got = np.array([view_tools.counts_consistent(c, pixels, mv, mc) for c in g["set.counts"]])
    assert np.array_equal(got, g["set.pair_consistent"])
    assert np.array_equal(got, np.array([ref.consistent(c, pixels, mv, mc) for c in g["set.counts"]]))
    rest = set(int(v) for v in g["set.rest"])
    views = [all(got[k] for k, (i, j) in enumerate(g["set.pairs"]) if i == v and j in rest) for v in range(5)]
    assert np.array_equal(views, g["set.view_consistent"])
    assert not view_tools.counts_consistent([10, 0, 0, 0], 10, 0.0, 0.0)      # no finite ratio: not consistent
    # P2 and the casts are the reference's: R and t go through float32 BEFORE K.dot
    v = view_tools.View(R=g["set.R"][1], t=g["set.t"][1], K=g["set.K"], image=None, depth=g["set.depth"][1], depth_metric="camera_z")
    P2 = view_tools.projection_matrix(v)
    assert P2.dtype == np.float32 and np.array_equal(P2, ref.projection_matrix(v.K, v.R, v.t).astype(np.float32))


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_golden_rejects_the_mutant(golden, mutant):
    """a restatement with ONE deviation (the kernel's likely mistakes) disagrees with the reference on at least one case"""
    g = golden
    rejected = []
    for name in case_names():
        mask, ratios, counts = run_case(g, name, mutant)
        if not (np.array_equal(mask, g[name + ".mask"]) and np.array_equal(_bits(ratios), _bits(g[name + ".ratios"])) and np.array_equal(counts, g[name + ".counts"])):
            rejected.append(name)
    mask, ratios, counts = run_set(g, mutant)
    if not (np.array_equal(mask, g["set.mask"]) and np.array_equal(counts, g["set.counts"])
            and hashlib.sha1(np.ascontiguousarray(ratios).tobytes()).hexdigest() == str(g["set.ratios_sha1"])):
        rejected.append("set")
    assert rejected, mutant
    if mutant == "roundf":
        assert "exact_half" in rejected
    if mutant == "double_thresholds":
        assert "threshold_edge" in rejected


def test_kernel_source_hash_is_the_recorded_one():
    """viewgeom.hip / viewgeom.h are built and linked but stay outside csrc_sha(): a changed hash would switch the output comparison of
    tests/test_dispatch_trace_gpu.py off without any test failing"""
    from demon_amd import build
    with np.load(os.path.join(ROOT, "tests", "golden", "dispatch_trace.npz"), allow_pickle=False) as z:
        meta = json.loads(bytes(z["meta"]).decode())
    assert build.csrc_sha() == meta["csrc_sha"]
    assert "viewgeom.hip" in build.EXTRA_SOURCES and "viewgeom.hip" not in build.SOURCES
    assert os.path.exists(os.path.join(ROOT, "demon_amd", "csrc", "viewgeom.h"))
    internal = open(os.path.join(ROOT, "demon_amd", "csrc", "internal.h")).read()
    assert "ViewArgs" not in internal and "viewgeom" not in internal


def test_abi_declares_and_binds_the_view_symbols():
    from demon_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "demon_hip.h")).read(), flags=re.S)
    for s in ("demon_op_view_pair", "demon_op_view_pairs"):
        m = re.search(r"\bint %s\(([^)]*)\)" % s, header)
        assert m, s
        assert s in _lib.SIGNATURES and len(_lib.SIGNATURES[s][1]) == len(m.group(1).split(",")), s
    assert len(_lib.SIGNATURES["demon_op_view_pair"][1]) == 18 and len(_lib.SIGNATURES["demon_op_view_pairs"][1]) == 18
    src = open(os.path.join(ROOT, "demon_amd", "csrc", "viewgeom.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "rintf" in src and "roundf" not in src and "__fdividef" not in src
    from demon_amd.engine import DemonContext
    assert callable(DemonContext.view_pair) and callable(DemonContext.view_pairs)


def test_drop_in_dataset_tools_modules():
    sys.path.insert(0, os.path.join(ROOT, "python"))
    import importlib
    vt = importlib.import_module("depthmotionnet.dataset_tools.view_tools")
    view = importlib.import_module("depthmotionnet.dataset_tools.view")
    assert view.View._fields == ("R", "t", "K", "image", "depth", "depth_metric") and vt.View is view.View
    for name in ("compute_visible_points_mask", "compute_depth_ratios", "check_depth_consistency", "view_pair_counts", "consistent_pairs"):
        assert callable(getattr(vt, name)), name
    from demon_amd import evaluation
    assert callable(evaluation.invalidate_points_not_visible_in_second_image)
    v = view.View(R=np.eye(3), t=np.zeros(3), K=np.eye(3), image=None, depth=np.ones((2, 2), np.float32), depth_metric="disparity")
    with pytest.raises(AssertionError):              # the reference's assertion, before any GPU call
        vt.compute_visible_points_mask(v, v)
    with pytest.raises(AssertionError):
        vt.compute_depth_ratios(v._replace(depth_metric="camera_z"), v)


def _compiled_reference():
    import glob
    so = glob.glob(os.path.join(ROOT, "oracle", "_ref", "view_tools_cython*.so"))
    if not so:
        return None
    spec = importlib.util.spec_from_file_location("view_tools_cython", so[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_restatement_equals_the_compiled_reference_on_fresh_inputs():
    mod = _compiled_reference()
    if mod is None:
        pytest.skip("oracle/_ref holds no compiled reference module")
    from demon_amd.view_tools import View
    rng = np.random.default_rng(7)
    bad = np.array([0.0, -1.0, np.nan, np.inf], np.float32)
    for h, w in ((5, 7), (16, 24), (33, 65), (17, 130)):
        for other in (False, True):
            h2, w2 = (h + 3, w - 2) if other else (h, w)
            depths = []
            for hh, ww in ((h, w), (h2, w2)):
                d = rng.uniform(1.0, 4.0, (hh, ww)).astype(np.float32)
                d.reshape(-1)[rng.permutation(d.size)[:max(4, d.size // 10)]] = bad[np.arange(max(4, d.size // 10)) % 4]
                depths.append(d)
            K1 = np.array([[0.89 * w, 0, 0.5 * w + 0.3], [0, 1.19 * h, 0.5 * h - 0.6], [0, 0, 1]])
            K2 = np.array([[0.89 * w2, 0, 0.5 * w2], [0, 1.19 * h2, 0.5 * h2], [0, 0, 1]])
            q1, _ = np.linalg.qr(np.eye(3) + 0.05 * rng.standard_normal((3, 3)))
            q2, _ = np.linalg.qr(np.eye(3) + 0.05 * rng.standard_normal((3, 3)))
            R1, R2 = q1 * np.sign(np.diag(q1)), q2 * np.sign(np.diag(q2))
            t1, t2 = rng.uniform(-0.1, 0.1, 3), rng.uniform(-0.1, 0.1, 3)
            pad = np.full((h2 + 2, w2), np.nan, np.float32)      # reads past the map are defined: NaN
            pad[:h2] = depths[1]
            v1 = View(R=R1, t=t1, K=K1, image=None, depth=depths[0], depth_metric="camera_z")
            v2 = View(R=R2, t=t2, K=K2, image=None, depth=pad[:h2], depth_metric="camera_z")
            bx, by = (2, 1) if other else (0, 0)
            want_m, want_r = np.asarray(mod.compute_visible_points_mask(v1, v2, bx, by)), np.asarray(mod.compute_depth_ratios(v1, v2))
            P2 = ref.projection_matrix(K2, R2, t2).astype(np.float32)
            mask, ratios, _ = ref.view_geometry(depths[0], depths[1], K1, R1, t1, P2, borderx=bx, bordery=by)
            assert np.array_equal(mask, want_m) and np.array_equal(_bits(ratios), _bits(want_r)), (h, w, other)
