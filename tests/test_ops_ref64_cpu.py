"""CPU proof that the float64 references of tests/ops_ref64.py can be trusted as a gate (no GPU):

  - the float32 C oracle (oracle/demon_oracle.c) lies within C_op 2^-24 bound_units of them at EVERY element of every input set the
    GPU suite runs, with 4 x its largest ratio <= C_op (the constants are measured here, not copied), NaN patterns equal;
  - from the references alone: >= 95 % of the finite elements of every input set are informative (bound <= 1e-3 of the value) and
    <= 2 % undecided;
  - every mutant of a reference -- the mistakes a kernel could make unnoticed by a tensor-wide sum -- is rejected at one or more
    informative elements of every input set on which it changes the result at all.
"""
import itertools

import numpy as np
import pytest

import ops_ref64 as R
from oracle import ops_ref

BOOLS = R.BOOLS


def _oracle_within(got, ref, C, floor, what, worst):
    worst.append(R.check(got, ref, C, what))
    info, und = R.shares(ref, C, floor)
    assert info >= 0.95, "%s: only %.1f %% of the elements are informative" % (what, 100 * info)
    assert und <= 0.02, "%s: %.1f %% of the elements are undecided" % (what, 100 * und)


def _changes(mut, ref):
    return not np.array_equal(mut.want.astype(np.float32), ref.want.astype(np.float32), equal_nan=True)


def _mutants(make, names, C, floor, what, seen):
    """make(mutant) -> Ref; every mutant that changes the result must fail the check at an informative element"""
    ref = make(None)
    for m in names:
        mut = make(m)
        if _changes(mut, ref):
            seen.add(m)
            assert R.rejected(mut, ref, C, floor), "%s: mutant %r passes the check" % (what, m)


def _constant(worst, C, name):
    ratio = max(worst)
    print("%s: largest oracle ratio %.3f over %d input sets, C = %g" % (name, ratio, len(worst), C))
    assert 4 * ratio <= C, "%s: 4 x %.3f > C = %g" % (name, ratio, C)
    assert 4 * ratio > C / 2 or C == 1, "%s: C = %g is not 4 x %.3f rounded up to a power of two" % (name, C, ratio)


def test_rodrigues_branches():
    K, rot, tr = R.cameras(3)
    Rm = R.rodrigues(rot)
    assert np.array_equal(Rm[0], np.eye(3))
    assert not np.array_equal(Rm[1], np.eye(3)) and np.abs(Rm[1] - np.eye(3)).max() < 3e-6      # just above the identity branch
    assert 1.5e-6 < np.linalg.norm(rot[1].astype(np.float64)) < 2.5e-6
    for i in range(3):
        assert np.abs(Rm[i] @ Rm[i].T - np.eye(3)).max() < 1e-14
        assert np.abs(Rm[i] - ops_ref.angleaxis_to_rotation(rot[i])).max() < 1e-6


def test_depth_to_flow_oracle_and_mutants():
    worst, seen = [], set()
    for shape, inv, norm, gate in itertools.product(R.GEOM_SHAPES, BOOLS, BOOLS, BOOLS):
        K, rot, tr = R.cameras(shape[0])
        d = R.depth_input(shape)
        what = "depth_to_flow %s inverse %d normalize %d gate %d" % (shape, inv, norm, gate)
        floor = 1.0 / shape[2] if norm else 1e-3
        ref = R.depth_to_flow(d, K, rot, tr, inv, norm, gate)
        got = ops_ref.depth_to_flow(d, K, rot, tr, inv, norm, gate)
        assert np.isnan(ref.want).any() != gate and np.isfinite(ref.want).any(), what
        _oracle_within(got, ref, R.C_DEPTH_TO_FLOW, floor, what, worst)
        _mutants(lambda m: R.depth_to_flow(d, K, rot, tr, inv, norm, gate, mutant=m), R.CAMERA_MUTANTS, R.C_DEPTH_TO_FLOW, floor, what, seen)
    assert seen == set(R.CAMERA_MUTANTS), seen
    _constant(worst, R.C_DEPTH_TO_FLOW, "depth_to_flow")


@pytest.mark.parametrize("method", [1, 0])
def test_flow_to_depth_oracle_and_mutants(method):
    worst, seen = [], set()
    C = R.C_FLOW_TO_DEPTH_0 if method == 0 else R.C_FLOW_TO_DEPTH_1
    for shape, inv, norm in itertools.product(R.DLT_SHAPES if method == 0 else R.GEOM_SHAPES, BOOLS, BOOLS):
        K, rot, tr = R.cameras(shape[0])
        f = R.flow_input(shape, norm)
        what = "flow_to_depth method %d %s inverse %d normalized %d" % (method, shape, inv, norm)
        ref = R.flow_to_depth(f, K, rot, tr, inv, norm, method)
        got = ops_ref.flow_to_depth(f, K, rot, tr, inv, norm, method)
        assert np.isnan(ref.want).sum() >= shape[0] and np.isfinite(ref.want).any(), what
        _oracle_within(got, ref, C, 1e-3, what, worst)
        # R against its transpose: with rotations of 0 and 2e-6 rad (the two-sample sets) the difference is below the rounding of the inputs
        names = [m for m in R.CAMERA_MUTANTS if m != "r_transposed" or shape[0] > 2]
        _mutants(lambda m: R.flow_to_depth(f, K, rot, tr, inv, norm, method, mutant=m), names, C, 1e-3, what, seen)
    assert seen == set(R.CAMERA_MUTANTS), seen
    _constant(worst, C, "flow_to_depth method %d" % method)


def test_warp2d_exact_oracle_and_mutants():
    seen = set()
    for (shape, norm), (border, bv) in itertools.product(R.WARP_EXACT_CASES, R.WARP_BORDERS):
        img, disp = R.warp_exact_input(shape, norm)
        what = "warp2d exact %s normalized %d %s %g" % (shape, norm, border, bv)
        ref = R.warp2d(img, disp, norm, border, bv)
        assert np.array_equal(ref.want, ref.want.astype(np.float32).astype(np.float64), equal_nan=True), what   # fp32 values: exact
        fin = np.isfinite(ref.want)
        assert np.array_equal(ref.want[fin] * 64, np.rint(ref.want[fin] * 64)), what                               # multiples of 1/64
        R.check_exact(ops_ref.warp2d(img, disp, norm, border, bv), ref.want, what)
        for m in ("trunc", "clamp_taps"):
            mut = R.warp2d(img, disp, norm, border, bv, mutant=m)
            if _changes(mut, ref):
                seen.add((m, border))
            assert _changes(mut, ref) == (m == "trunc" or border == "value"), (what, m)
    assert seen == {("trunc", "value"), ("trunc", "clamp"), ("clamp_taps", "value")}


def test_warp2d_exact_inputs_reach_the_edges():
    """the planted positions exist in every tier-1 input: sx in (-1, 0), exactly -1, in [W - 1, W), exactly W (y alike), both out"""
    for shape, norm in R.WARP_EXACT_CASES:
        n, c, h, w = shape
        img, disp = R.warp_exact_input(shape, norm)
        assert (img != 0).all() and np.abs(img).max() <= 8
        d = disp.astype(np.float64)
        with np.errstate(all="ignore"):
            sx = np.arange(w)[None, None, :] + d[:, 0] * (w if norm else 1)
            sy = np.arange(h)[None, :, None] + d[:, 1] * (h if norm else 1)
        for s, size in ((sx, w), (sy, h)):
            assert ((s > -1) & (s < 0)).any() and (s == -1).any() and ((s >= size - 1) & (s < size)).any() and (s == size).any()
        assert (((sx < 0) | (sx >= w)) & ((sy < 0) | (sy >= h))).any()
        assert ((d[:, 0] == 0) & (d[:, 1] == 0)).any() and np.isnan(d).any() and (d == np.inf).any() and (d == -np.inf).any()
        assert (d == 2e9).any() and (d == -2e9).any()


def test_warp2d_bound_oracle_and_mutants():
    worst, seen = [], set()
    img, disp = R.warp_bound_input()
    for border in ("value", "clamp"):
        what = "warp2d bound %s %s" % (R.WARP_BOUND_SHAPE, border)
        ref = R.warp2d(img, disp, True, border, 0.25)
        got = ops_ref.warp2d(img, disp, True, border, 0.25)
        _oracle_within(got, ref, R.C_WARP2D, 1e-3, what, worst)
        _mutants(lambda m: R.warp2d(img, disp, True, border, 0.25, mutant=m), ("trunc", "clamp_taps"), R.C_WARP2D, 1e-3, what, seen)
    assert seen == {"trunc", "clamp_taps"}
    _constant(worst, R.C_WARP2D, "warp2d")


SIG_MUTANTS = ("x_minus_1", "tile_x", "tile_y")


def test_scale_invariant_gradient_oracle_and_mutants():
    worst, applied = [], {}
    for shape, deltas in itertools.product(R.SIG_SHAPES, R.SIG_DELTAS):
        u, wts = R.sig_input(shape), R.sig_weights(len(deltas))
        what = "scale_invariant_gradient %s deltas %s" % (shape, deltas)
        ref = R.scale_invariant_gradient(u, deltas, wts, 0.01)
        got = ops_ref.scale_invariant_gradient(u, deltas, wts, 0.01)
        none = ref.bound == 0
        assert (ref.want[none] == 0).all()              # no neighbour: exactly 0 (the check demands it: bound 0)
        _oracle_within(got, ref, R.C_SIG, 1e-3, what, worst)
        seen = set()
        _mutants(lambda m: R.scale_invariant_gradient(u, deltas, wts, 0.01, mutant=m), SIG_MUTANTS, R.C_SIG, 1e-3, what, seen)
        applied[(shape, deltas)] = seen
    # the mutants bite where the kernel's structure says they must: a tile boundary in x needs W > 64, rows past a tile H > 4
    assert applied[((1, 2, 5, 65), (1,))] == set(SIG_MUTANTS)
    assert applied[((2, 1, 9, 130), (17,))] == set(SIG_MUTANTS) and applied[((2, 1, 9, 130), (32,))] == set(SIG_MUTANTS)
    assert applied[((1, 1, 4, 63), (16,))] == {"x_minus_1"} and applied[((1, 3, 1, 1), (1,))] == set()
    assert "tile_x" in applied[((2, 1, 9, 130), (1, -2, 3, -5, 8, -13, 21, 200))]
    _constant(worst, R.C_SIG, "scale_invariant_gradient")


@pytest.mark.parametrize("shape,deltas", [((2, 1, 9, 130), (1, 2, 4, 8, 16)), ((1, 1, 3, 64), (1,))])
def test_scale_invariant_gradient_eps0(shape, deltas):
    """eps = 0 and pairs of equal zeros: 0 / 0 = NaN, compared as a pattern"""
    u, wts = R.sig_input(shape, True), R.sig_weights(len(deltas))
    ref = R.scale_invariant_gradient(u, deltas, wts, 0.0)
    assert np.isnan(ref.want).any() and np.isfinite(ref.want).any()
    R.check(ops_ref.scale_invariant_gradient(u, deltas, wts, 0.0), ref, R.C_SIG, "sig eps 0 %s" % (shape,))


def test_depth_to_normals_oracle_and_mutants():
    worst, seen = [], set()
    names = ("no_half", "k0", "fx_by_h")
    for shape, inv in itertools.product(R.NORMALS_SHAPES, BOOLS):
        z, K = R.normals_input(shape)
        what = "depth_to_normals %s inverse %d" % (shape, inv)
        ref = R.depth_to_normals(z, K, inv)
        got = ops_ref.depth_to_normals(z, K, inv)
        assert np.isfinite(ref.want).any() == (shape[1] >= 3), what
        _oracle_within(got, ref, R.C_NORMALS, 1e-3, what, worst)
        _mutants(lambda m: R.depth_to_normals(z, K, inv, mutant=m), names, R.C_NORMALS, 1e-3, what, seen)
    assert seen == set(names), seen
    _constant(worst, R.C_NORMALS, "depth_to_normals")


def test_depth_to_normals_tie_is_undecided():
    """an exact tie of the forward and the backward depth step: both choices are accepted, a third is not"""
    z = np.array([[1.0, 1.0, 1.0, 1.0], [1.0, 1.25, 1.5, 1.75], [1.0, 1.5, 1.0, 1.0]], np.float32)[None, None]
    ref = R.depth_to_normals(z, R.K_DEMON, False)
    assert ref.alts and ref.alts[0][2][0, :, 1, 1].all()            # pixel (1, 1): |1.25 - 1| == |1.5 - 1.25| in x
    fwd, bwd = ref.want[0, :, 1, 1], ref.alts[0][0][0, :, 1, 1]
    assert np.abs(fwd - bwd).max() > 1e-3
    for pick, ok in ((fwd, True), (bwd, True), (0.5 * (fwd + bwd), False)):
        got = ref.want.copy()
        got[0, :, 1, 1] = pick
        assert R.compare(got, ref, R.C_NORMALS)[0].all() == ok


def test_median_oracle_and_mutant():
    seen = 0
    for shape, sprinkle in itertools.product(R.MEDIAN_SHAPES, BOOLS):
        x = R.median_input(shape, sprinkle)
        want = R.median3x3_downsample(x)
        R.check_exact(ops_ref.median3x3_downsample(x), want, "median %s" % (shape,))
        mut = R.median3x3_downsample(x, mutant="odd_centre")
        if shape[2] * shape[3] > 2:
            assert not np.array_equal(mut, want, equal_nan=True), shape
            seen += 1
    assert seen == 6


def test_elementwise_refs():
    rng = np.random.default_rng(7)
    x = rng.standard_normal(1025).astype(np.float32)
    x[1], x[2], x[3] = np.nan, np.inf, -np.inf
    for leak in (0.1, -0.3):
        R.check_exact(ops_ref.leaky_relu(x, leak), R.leaky_relu(x, leak), "leaky_relu")
    R.check_exact(ops_ref.replace_nonfinite(x, 2.5), R.replace_nonfinite(x, 2.5), "replace_nonfinite")


def test_check_rejects_what_a_sum_cannot_see():
    """one wrong element of 7020, far below any relative-L1 bar, fails; a NaN in place of a number and a number in place of a NaN too"""
    shape = (3, 9, 130)
    K, rot, tr = R.cameras(3)
    d = R.depth_input(shape)
    ref = R.depth_to_flow(d, K, rot, tr, True, True, False)
    good = ops_ref.depth_to_flow(d, K, rot, tr, True, True, False)
    i = tuple(np.argwhere(R.informative(ref, R.C_DEPTH_TO_FLOW, 1 / 130))[100])
    bad = good.copy()
    bad[i] *= np.float32(1.002)
    m = np.isfinite(good)
    assert np.abs(bad[m] - good[m]).sum() / np.abs(good[m]).sum() < 1e-5
    with pytest.raises(AssertionError):
        R.check(bad, ref, R.C_DEPTH_TO_FLOW)
    for v, j in ((np.nan, i), (0.0, tuple(np.argwhere(np.isnan(ref.want))[0]))):
        bad = good.copy()
        bad[j] = v
        with pytest.raises(AssertionError):
            R.check(bad, ref, R.C_DEPTH_TO_FLOW)
