"""The geometry and loss kernels of demon_amd/csrc/ops.hip held PER ELEMENT to the float64 references of tests/ops_ref64.py, through
the C ABI, at the smallest shapes that reach each edge: per-sample cameras (a zero rotation and one just above the identity branch
among them), H * W below, at and just above one 256-thread block, ragged 64 x 4 tiles, the staged and the un-staged path of the
scale-invariant gradient, warp taps on either side of every image border.  tests/test_ops_ref64_cpu.py proves on the CPU that the
bounds hold for the float32 oracle with a factor 4 to spare, that nearly every element is informative, and that the mutants fail."""
import itertools

import numpy as np
import pytest

import ops_ref64 as R

pytestmark = pytest.mark.gpu
BOOLS = R.BOOLS


def _held(got, ref, C, what):
    _, ratio = R.compare(got, ref, C)
    fin = ratio[np.isfinite(ratio)]
    print("%s: largest |got - want| / (2^-24 bound) = %.3f of C = %g" % (what, fin.max() if fin.size else 0.0, C))
    R.check(got, ref, C, what)


@pytest.mark.parametrize("shape", R.GEOM_SHAPES)
def test_depth_to_flow(gpu_ctx, shape):
    K, rot, tr = R.cameras(shape[0])
    d = R.depth_input(shape)
    for inv, norm, gate in itertools.product(BOOLS, BOOLS, BOOLS):
        got = gpu_ctx.depth_to_flow(d, K, rot, tr, inv, norm, gate)
        _held(got, R.depth_to_flow(d, K, rot, tr, inv, norm, gate), R.C_DEPTH_TO_FLOW, "depth_to_flow %s inverse %d normalize %d gate %d" % (shape, inv, norm, gate))


@pytest.mark.parametrize("method,shape", [(1, s) for s in R.GEOM_SHAPES] + [(0, s) for s in R.DLT_SHAPES])
def test_flow_to_depth(gpu_ctx, method, shape):
    K, rot, tr = R.cameras(shape[0])
    C = R.C_FLOW_TO_DEPTH_0 if method == 0 else R.C_FLOW_TO_DEPTH_1
    for inv, norm in itertools.product(BOOLS, BOOLS):
        f = R.flow_input(shape, norm)
        got = gpu_ctx.flow_to_depth(f, K, rot, tr, inv, norm, method)
        _held(got, R.flow_to_depth(f, K, rot, tr, inv, norm, method), C, "flow_to_depth method %d %s inverse %d normalized %d" % (method, shape, inv, norm))


@pytest.mark.parametrize("shape,normalized", R.WARP_EXACT_CASES)
def test_warp2d_exact(gpu_ctx, shape, normalized):
    """tier 1: integer image values, positions on the 1/8 grid: np.array_equal with the float64 result"""
    img, disp = R.warp_exact_input(shape, normalized)
    for border, bv in R.WARP_BORDERS:
        got = gpu_ctx.warp2d(img, disp, normalized, border, bv)
        R.check_exact(got, R.warp2d(img, disp, normalized, border, bv).want, "warp2d %s normalized %d %s %g" % (shape, normalized, border, bv))


@pytest.mark.parametrize("border", ["value", "clamp"])
def test_warp2d_bound(gpu_ctx, border):
    """tier 2: ragged shape, normalised displacements"""
    img, disp = R.warp_bound_input()
    got = gpu_ctx.warp2d(img, disp, True, border, 0.25)
    _held(got, R.warp2d(img, disp, True, border, 0.25), R.C_WARP2D, "warp2d %s %s" % (R.WARP_BOUND_SHAPE, border))


@pytest.mark.parametrize("shape", R.SIG_SHAPES)
def test_scale_invariant_gradient(gpu_ctx, shape):
    u = R.sig_input(shape)
    for deltas in R.SIG_DELTAS:
        wts = R.sig_weights(len(deltas))
        got = gpu_ctx.scale_invariant_gradient(u, deltas, wts, 0.01)
        _held(got, R.scale_invariant_gradient(u, deltas, wts, 0.01), R.C_SIG, "scale_invariant_gradient %s deltas %s" % (shape, deltas))


@pytest.mark.parametrize("shape,deltas", [((2, 1, 9, 130), (1, 2, 4, 8, 16)), ((1, 1, 3, 64), (1,))])
def test_scale_invariant_gradient_eps0(gpu_ctx, shape, deltas):
    """eps = 0 and pairs of equal zeros: 0 / 0 = NaN, the pattern is compared"""
    u, wts = R.sig_input(shape, True), R.sig_weights(len(deltas))
    ref = R.scale_invariant_gradient(u, deltas, wts, 0.0)
    assert np.isnan(ref.want).any()
    _held(gpu_ctx.scale_invariant_gradient(u, deltas, wts, 0.0), ref, R.C_SIG, "scale_invariant_gradient eps 0 %s" % (shape,))


def test_scale_invariant_gradient_refuses_nine_deltas(gpu_ctx):
    from demon_amd import DemonError
    u = R.sig_input((1, 1, 4, 63))
    with pytest.raises(DemonError):
        gpu_ctx.scale_invariant_gradient(u, list(range(1, 10)), R.sig_weights(9), 0.01)
    wts = R.sig_weights(8)                      # (and the context still works)
    _held(gpu_ctx.scale_invariant_gradient(u, list(range(1, 9)), wts, 0.01), R.scale_invariant_gradient(u, list(range(1, 9)), wts, 0.01), R.C_SIG, "8 deltas")


@pytest.mark.parametrize("shape", R.NORMALS_SHAPES)
def test_depth_to_normals(gpu_ctx, shape):
    z, K = R.normals_input(shape)
    for inv in BOOLS:
        got = gpu_ctx.depth_to_normals(z, K, inv)
        _held(got, R.depth_to_normals(z, K, inv), R.C_NORMALS, "depth_to_normals %s inverse %d" % (shape, inv))


@pytest.mark.parametrize("shape", R.MEDIAN_SHAPES)
def test_median3x3_downsample(gpu_ctx, shape):
    for sprinkle in BOOLS:
        x = R.median_input(shape, sprinkle)
        R.check_exact(gpu_ctx.median3x3_downsample(x), R.median3x3_downsample(x), "median3x3_downsample %s sprinkle %d" % (shape, sprinkle))


@pytest.mark.parametrize("shape", R.L2_SHAPES)
def test_pointwise_l2_loss(gpu_ctx, shape):
    inp, gt = R.l2_input(shape)
    for eps in (0.0, 1e-3):
        got, want = gpu_ctx.pointwise_l2_loss(inp, gt, eps), R.pointwise_l2_loss(inp, gt, eps)
        print("pointwise_l2_loss %s eps %g: got %r want %r" % (shape, eps, got, want))
        assert abs(got - want) <= 1e-5 * abs(want), (got, want)


def test_pointwise_l2_loss_all_nan_ground_truth(gpu_ctx):
    """every difference is replaced by 0: the loss is sqrt(eps)"""
    inp, _ = R.l2_input((1, 2, 1, 257))
    gt = np.full_like(inp, np.nan)
    for eps in (0.0, 1e-3):
        got, want = gpu_ctx.pointwise_l2_loss(inp, gt, eps), float(np.sqrt(np.float64(eps)))
        assert R.pointwise_l2_loss(inp, gt, eps) == want
        print("pointwise_l2_loss all NaN eps %g: got %r want %r" % (eps, got, want))
        assert abs(got - want) <= 1e-5 * abs(want), (got, want)


@pytest.mark.parametrize("count,leak", [(2, 0.1), (5, -0.3), (1025, 0.1)])
def test_elementwise(gpu_ctx, count, leak):
    rng = np.random.default_rng(109 + count)
    x = rng.standard_normal(count).astype(np.float32)
    if count > 3:
        x[1], x[2], x[3] = np.nan, np.inf, -np.inf
    R.check_exact(gpu_ctx.leaky_relu(x, leak), R.leaky_relu(x, leak), "leaky_relu %d" % count)
    R.check_exact(gpu_ctx.replace_nonfinite(x, 2.5), R.replace_nonfinite(x, 2.5), "replace_nonfinite %d" % count)
