"""Option precision = 1 (bf16 operands, fp32 accumulation; conv_bf16.hip) on the GPU.  Every test uses contexts of its own or
restores the option in `finally`: the shared gpu_ctx stays an fp32 context."""
import os

import numpy as np
import pytest
import torch

from conftest import make_inputs, rel_l1
import exact_ref as X
import test_bf16_cpu as E

pytestmark = pytest.mark.gpu

TILES = [(128, 128), (64, 128), (32, 128), (64, 64), (32, 64), (32, 32), (128, 32), (64, 32)]   # enum ConvTile


@pytest.fixture(scope="module")
def ops_bf16():
    from demon_amd import DemonContext
    ctx = DemonContext.ops_only(0)
    ctx.set_option("precision", 1)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def net_pair(synth_weights):
    """an fp32 and a bf16 context (batch 4) with the synthetic weights"""
    from demon_amd import DemonContext
    c32 = DemonContext(0, 4, 192, 256)
    c16 = DemonContext(0, 4, 192, 256, precision="bf16")
    c32.set_weights(synth_weights)
    c16.set_weights(synth_weights)
    yield c32, c16
    c32.close()
    c16.close()


def _run(ctx, kind, x, w, b, stride=(1, 1), lrelu=False, padding="caffe"):
    if kind == "deconv":
        return ctx.deconv4x4s2(x, w, b, lrelu=lrelu)
    if kind == "dense":
        return ctx.dense(x, w, b, lrelu=lrelu)
    return ctx.conv2d(x, w, b, stride, lrelu=lrelu, padding=padding)


def _ref64(kind, x, w, b, stride=(1, 1), padding="caffe"):
    """float64 result of the layer on the given operands, and sum |x||w| + |b| per output element"""
    def lin(x, w, b):
        xt, bt = torch.from_numpy(x.astype(np.float64)), torch.from_numpy(b.astype(np.float64))
        if kind == "dense":
            return torch.nn.functional.linear(xt, torch.from_numpy(w.T.astype(np.float64)), bt).numpy()
        wt = torch.from_numpy(np.ascontiguousarray(w.transpose(3, 2, 0, 1)).astype(np.float64))
        if kind == "deconv":
            return torch.nn.functional.conv_transpose2d(xt, wt, bt, stride=2, padding=1).numpy()
        kh, kw = w.shape[:2]
        if padding == "same":
            pads = []
            for n, k, s in ((x.shape[3], kw, stride[1]), (x.shape[2], kh, stride[0])):
                tot = max((-(-n // s) - 1) * s + k - n, 0)
                pads += [tot // 2, tot - tot // 2]
        else:
            pads = [kw // 2, kw // 2, kh // 2, kh // 2]
        return torch.nn.functional.conv2d(torch.nn.functional.pad(xt, pads), wt, bt, stride=stride).numpy()
    return lin(x, w, b), lin(np.abs(x), np.abs(w), np.abs(b))


# eligible shape classes of tests/test_variants_gpu.LAYERS: (kind, cin, cout, kh, kw, sh, sw, H, W[, padding])
SHAPES = [
    ("conv", 64, 64, 3, 1, 1, 1, 48, 64), ("conv", 64, 128, 5, 1, 2, 1, 48, 64), ("conv", 512, 512, 1, 3, 1, 1, 6, 8),
    ("conv", 32, 32, 1, 9, 1, 2, 12, 64), ("conv", 64, 64, 3, 3, 1, 1, 24, 32), ("conv", 32, 64, 3, 3, 2, 2, 24, 32),
    ("conv", 512, 24, 3, 3, 1, 1, 6, 8), ("conv", 16, 40, 3, 3, 1, 1, 7, 9), ("conv", 48, 32, 1, 5, 1, 2, 5, 23),
    ("conv", 30, 12, 3, 3, 2, 2, 24, 32), ("conv", 64, 16, 3, 3, 2, 2, 24, 32, "same"), ("conv", 32, 64, 1, 7, 1, 2, 12, 16, "same"),
    ("deconv", 512, 256, 0, 0, 0, 0, 6, 8), ("deconv", 128, 64, 0, 0, 0, 0, 17, 35), ("deconv", 16, 8, 0, 0, 0, 0, 3, 5),
    ("dense", 1024, 128, 0, 0, 0, 0, 1, 1), ("dense", 48, 200, 0, 0, 0, 0, 1, 1),
]


def _operands(shape, seed, n=3):
    kind, cin, cout, kh, kw, sh, sw, H, W = shape[:9]
    rng = np.random.default_rng(seed)
    if kind == "dense":
        x = rng.standard_normal((n, cin)).astype(np.float32)
        w = (rng.standard_normal((cin, cout)) / np.sqrt(cin)).astype(np.float32)
    else:
        x = rng.standard_normal((n, cin, H, W)).astype(np.float32)
        wshape = (4, 4, cout, cin) if kind == "deconv" else (kh, kw, cin, cout)
        w = (rng.standard_normal(wshape) / np.sqrt(np.prod(wshape) / cout)).astype(np.float32)
    b = rng.standard_normal((cout,)).astype(np.float32)
    return x, w, b


@pytest.mark.parametrize("shape", SHAPES)
def test_every_tile_and_split_is_exact_to_the_bf16_bound(ops_bf16, shape):
    """a bf16 x bf16 product is exact in fp32, so against float64 on the bf16-rounded operands only the fp32 additions err:
    |got - ref| <= (K + ksplit + 2) 2^-24 (sum |x||w| + |b|) for every element, tile and split-K.  On small non-zero integers
    (+-1, +-2 are bf16 values; tests/exact_ref.py) nothing rounds at all: every tile and split returns the integer result bit for bit"""
    kind, cin, cout, kh, kw, sh, sw = shape[:7]
    padding = shape[9] if len(shape) > 9 else "caffe"
    x, w, b = _operands(shape, 40)
    ref, mag = _ref64(kind, E.bf16_round(x), E.bf16_round(w), b, (sh, sw), padding)
    K = 4 * cin if kind == "deconv" else (cin if kind == "dense" else kh * kw * cin)
    ex = X.Layer(kind, cin, cout, kh, kw, (sh, sw), shape[7], shape[8], n=3, padding=padding)
    try:
        for t, (bm, bn) in enumerate(TILES):
            if -(-cout // 32) * 32 % bm:
                continue
            for ks in (1, 2, 3, 5):
                os.environ["DEMON_FORCE_PLAN"] = "17,%d,%d" % (t, ks)
                got = _run(ops_bf16, kind, x, w, b, (sh, sw), padding=padding)
                tag = ops_bf16.last_kernel()
                assert tag.startswith("conv_bf16<%dx%d>" % (bm, bn)), (t, ks, tag)
                bound = (K + ks + 2) * 2.0 ** -24 * mag
                bad = np.abs(got - ref) > bound
                assert not bad.any(), "tile %d ksplit %d (%s): %d elements off, worst %.3e over the bound" % (
                    t, ks, tag, bad.sum(), (np.abs(got - ref) / np.maximum(bound, 1e-300)).max())
                ex.saw_rel(tag, ks)
                ex.check(ops_bf16, ks, expect="conv_bf16<%dx%d>" % (bm, bn))
        ex.finish()
        # the heuristic plan (no hook) and the activation
        os.environ.pop("DEMON_FORCE_PLAN")
        got = _run(ops_bf16, kind, x, w, b, (sh, sw), lrelu=True, padding=padding)
        assert ops_bf16.last_kernel().startswith("conv_bf16<")
        want = np.where(ref >= 0, ref, 0.1 * ref)
        assert (np.abs(got - want) <= (K + 8) * 2.0 ** -24 * mag + 1e-7 * np.abs(want)).all()
    finally:
        os.environ.pop("DEMON_FORCE_PLAN", None)


def test_option_default_values_and_range(gpu_ctx):
    from demon_amd.engine import DemonError
    assert gpu_ctx.get_option("precision") == 0 and gpu_ctx.precision == "fp32"
    try:
        gpu_ctx.set_option("precision", 1)
        assert gpu_ctx.get_option("precision") == 1 and gpu_ctx.precision == "bf16"
        for bad in (2, -1):
            with pytest.raises(DemonError):
                gpu_ctx.set_option("precision", bad)
            assert gpu_ctx.get_option("precision") == 1
    finally:
        gpu_ctx.set_option("precision", 0)
    assert gpu_ctx.get_option("precision") == 0


def test_bf16_mode_really_rounds(ops_bf16):
    """operands with bits below bf16 precision: the emulated result, not the fp32 one"""
    from demon_amd import DemonContext
    x = np.full((2, 64), 1 + 2.0 ** -9, np.float32)
    w = np.full((64, 8), 1 + 2.0 ** -9, np.float32)
    b = np.zeros(8, np.float32)
    got = ops_bf16.dense(x, w, b)
    np.testing.assert_array_equal(got, np.full((2, 8), 64.0, np.float32))
    c32 = DemonContext.ops_only(0)
    try:
        assert np.all(c32.dense(x, w, b) > 64.1)
    finally:
        c32.close()
    xc = np.full((1, 16, 8, 8), 1 + 2.0 ** -9, np.float32)
    wc = np.full((1, 1, 16, 8), 1 + 2.0 ** -9, np.float32)
    np.testing.assert_array_equal(ops_bf16.conv2d(xc, wc, b), np.full((1, 8, 8, 8), 16.0, np.float32))


@pytest.mark.parametrize("shape", [("conv", 6, 32, 9, 1, 2, 1, 48, 64), ("conv", 24, 4, 3, 3, 1, 1, 48, 64), ("conv", 4, 32, 3, 3, 1, 1, 40, 72),
                                   ("conv", 64, 4, 3, 3, 1, 1, 24, 32), ("deconv", 4, 2, 0, 0, 0, 0, 6, 8), ("dense", 1024, 7, 0, 0, 0, 0, 1, 1),
                                   ("conv", 16, 7, 3, 3, 1, 1, 12, 16), ("conv", 15, 64, 3, 3, 1, 1, 12, 16)])
def test_excluded_shapes_are_untouched(ops_bf16, shape):
    """Cin < 16 or Cout < 8: the fp32 kernels, bit for bit, in both modes"""
    from demon_amd import DemonContext
    kind, cin, cout, kh, kw, sh, sw = shape[:7]
    x, w, b = _operands(shape, 41, n=2)
    c32 = DemonContext.ops_only(0)
    try:
        want = _run(c32, kind, x, w, b, (sh, sw), lrelu=True)
        tag32 = c32.last_kernel()
    finally:
        c32.close()
    got = _run(ops_bf16, kind, x, w, b, (sh, sw), lrelu=True)
    assert not ops_bf16.last_kernel().startswith("conv_bf16") and ops_bf16.last_kernel() == tag32
    np.testing.assert_array_equal(got, want)


def test_profile_runs_exactly_the_eligible_layers_on_conv_bf16(net_pair, synth_weights):
    c32, c16 = net_pair
    names = [k[:-len("/kernel")] for k in synth_weights if k.endswith("/kernel")]
    eligible = {n for n in names if E.bf16_eligible(n, np.shape(synth_weights[n + "/kernel"]))}
    for n in (1, 4):
        rec32 = c32.profile_full(n, 1, 1)
        rec16 = c16.profile_full(n, 1, 1)
        assert not any(r["kernel"].startswith("conv_bf16") for r in rec32)
        on16 = {r["name"] for r in rec16 if r["kernel"].startswith("conv_bf16")}
        ran = {r["name"] for r in rec16}
        assert on16 == eligible & ran, (sorted(on16 ^ (eligible & ran)))
        # every eligible layer of the sub-nets a full pass runs is in the record (pairs run as their two layers), motion_fc2 is not
        assert eligible - {x for x in eligible if x.endswith("motion_fc2")} <= ran | {x for x in eligible if x.endswith("motion_fc2")}
        for r in rec16:
            if r["name"] not in eligible:
                assert not r["kernel"].startswith("conv_bf16"), r


def _full(ctx, n, iterations, seed=0):
    pair, img2 = make_inputs(n, ctx.H, ctx.W, seed)
    return ctx.full(pair, img2, iterations=iterations), pair, img2


def _gate(got, emu, args, keys, what, perturb=0):
    """got against the bf16-emulating oracle emu(*args), per output tensor: rel L1 <= 1e-3 (the north-star gate), widened to five
    times the oracle's OWN spread where that is larger, and finiteness alone where that spread exceeds 5e-3.  The spread is how far the emulation moves when its input argument
    `perturb` is scaled by 1 + 2^-22 (two fp32 ulps, the size of a summation-order difference): with bf16 operands a rounding that
    flips at one element cascades through the following layers, so at these synthetic weights the small heads (flow5 / conf5,
    rotation) move by about 1e-2, and the normals of an iterative step with the closed-form flow_to_depth by about 0.5 -- no
    implementation can match the emulation closer than the emulation matches itself.  Returns {key: (rel L1, spread)}."""
    args2 = list(args)
    args2[perturb] = (np.asarray(args[perturb]) * np.float32(1 + 2.0 ** -22)).astype(np.float32)
    with E.emulate_bf16():
        want, want2 = emu(*args), emu(*args2)
    gaps = {}
    for k in keys:
        err, spread = rel_l1(got[k], want[k]), rel_l1(want2[k], want[k])
        gaps[k] = (err, spread)
        assert np.isfinite(got[k]).all(), (what, k)
        if spread > 5e-3:   # ill-conditioned at these weights: two ulps move the emulation itself by more than the difference could show
            continue
        assert err <= max(1e-3, 5 * spread), "%s %s: rel L1 %.3e against the bf16-emulating oracle (its own spread %.3e)" % (what, k, err, spread)
    return gaps


KEYS = ("predict_flow5", "predict_conf5", "predict_flow2", "predict_conf2", "predict_depth2", "predict_normal2", "predict_rotation",
        "predict_translation")


@pytest.mark.parametrize("n", [1, 4])
def test_whole_nets_against_the_bf16_emulating_oracle(net_pair, synth_weights, n):
    from oracle import net_ref
    c32, c16 = net_pair
    pair, img2 = make_inputs(n, 192, 256, 5)
    got = c16.full(pair, img2, iterations=3)
    ref = net_ref.DemonRef(synth_weights)
    boot = c16.bootstrap(pair, img2)
    _gate(boot, ref.bootstrap, (pair, img2), KEYS, "bootstrap")
    for method in (0, 1):
        c16.set_option("flow_to_depth_method", method)
        try:
            args = (pair, img2, boot["predict_depth2"], boot["predict_normal2"], boot["predict_rotation"], boot["predict_translation"])
            _gate(c16.iterative(*args), net_ref.DemonRef(synth_weights, method).iterative, args, KEYS, "iterative (method %d)" % method)
        finally:
            c16.set_option("flow_to_depth_method", 0)
    image1 = np.ascontiguousarray(pair[:, 0:3])
    _gate(c16.refine(image1, boot["predict_depth2"]), ref.refine, (image1, boot["predict_depth2"]), ("predict_depth0",), "refine")
    gaps = _gate(got, lambda p, i: ref.full(p, i, iterations=3), (pair, img2), KEYS + ("predict_depth0",), "full x3 (batch %d)" % n)
    plain = net_ref.DemonRef(synth_weights).full(pair, img2, iterations=3)
    print("\nbf16 mode, batch %d, full x3 -- rel L1 to the bf16-emulating oracle / its own spread / to the fp32 oracle:\n%s" % (
        n, "\n".join("  %-20s %.2e / %.2e / %.2e" % (k, gaps[k][0], gaps[k][1], rel_l1(got[k], plain[k])) for k in KEYS + ("predict_depth0",))))


def test_v2_and_640x480_against_the_bf16_emulating_oracle():
    from demon_amd import DemonContext, weights
    from oracle import net_ref
    w2 = weights.synthetic_weights(seed=1, version=2)
    ctx = DemonContext(0, 1, 192, 256, version=2, precision="bf16")
    try:
        ctx.set_weights(w2)
        pair, img2 = make_inputs(1, 192, 256, 6)
        got = ctx.full(pair, img2, iterations=1)
        _gate(got, lambda p, i: net_ref.DemonRefV2(w2).full(p, i, iterations=1), (pair, img2), KEYS + ("predict_depth0",), "v2 full")
    finally:
        ctx.close()
    w1 = weights.synthetic_weights(seed=1, height=480, width=640)
    ctx = DemonContext(0, 2, 480, 640, precision="bf16")
    try:
        ctx.set_weights(w1)
        pair, img2 = make_inputs(2, 480, 640, 7)
        got = ctx.full(pair, img2, iterations=1)
        _gate(got, lambda p, i: net_ref.DemonRef(w1).full(p, i, iterations=1), (pair, img2), KEYS + ("predict_depth0",), "640x480 full")
    finally:
        ctx.close()


def test_nan_cases_behave_as_in_fp32(net_pair, synth_weights):
    """tests/test_nets_gpu.py's NaN cases in bf16 mode, against the bf16-emulating oracle: the gate keeps the outputs finite, and a NaN
    in the fed depth2 propagates exactly where it does in the oracle (the operand conversion keeps NaN a NaN), sample 1 unaffected"""
    from oracle import net_ref
    _, c16 = net_pair
    pair, img2_2 = make_inputs(2, seed=6)
    depth2 = np.full((2, 1, 48, 64), 0.5, np.float32)
    depth2[0, 0, :10] = -1.0
    depth2[1, 0, 5, 5] = 0.0
    normal2 = np.zeros((2, 3, 48, 64), np.float32)
    rot = np.array([[0.0, 0.0, 0.0], [0.3, -0.2, 0.1]], np.float32)
    tr = np.array([[5.0, 0.0, 0.0], [0.1, 0.9, -0.2]], np.float32)
    args = (pair, img2_2, depth2, normal2, rot, tr)
    ref = net_ref.DemonRef(synth_weights)
    got = c16.iterative(*args)
    assert all(np.isfinite(got[k]).all() for k in KEYS)
    _gate(got, ref.iterative, args, KEYS, "gated iterative")
    pair, img2_2 = make_inputs(2, seed=16)
    depth2 = np.full((2, 1, 48, 64), 0.5, np.float32)
    depth2[0, 0, 5, 5] = np.nan
    rot = np.array([[0.02, -0.01, 0.03], [0.3, -0.2, 0.1]], np.float32)
    tr = np.array([[0.5, 0.1, 0.0], [0.1, 0.9, -0.2]], np.float32)
    args = (pair, img2_2, depth2, normal2, rot, tr)
    got = c16.iterative(*args)
    with E.emulate_bf16():
        want = ref.iterative(*args)
    for k in KEYS:
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
        assert np.isnan(want[k][0]).any(), k
        assert np.isfinite(got[k][1]).all(), k
    one = lambda a: a[1:2]   # sample 1 alone, against the emulation of sample 1 alone (pairs are independent)
    _gate({k: one(got[k]) for k in KEYS}, ref.iterative, tuple(one(a) for a in args), KEYS, "clean sample next to a NaN one")
    clean = depth2.copy()
    clean[0, 0, 5, 5] = 0.5
    alone = c16.iterative(pair, img2_2, clean, normal2, rot, tr)
    for k in KEYS:
        np.testing.assert_array_equal(alone[k][1], got[k][1])


def test_graph_cache_precision_switch_and_weight_changes(synth_weights):
    from demon_amd import DemonContext, weights
    pair, img2 = make_inputs(2, 192, 256, 10)
    a = DemonContext(0, 2, 192, 256)
    fresh = DemonContext(0, 2, 192, 256)
    try:
        a.set_weights(synth_weights)
        fresh.set_weights(synth_weights)
        want32 = fresh.full(pair, img2, iterations=1)
        r32 = a.full(pair, img2, iterations=1)
        a.set_precision("bf16")
        r16 = a.full(pair, img2, iterations=1)
        a.set_option("hipgraph", 0)
        r16_eager = a.full(pair, img2, iterations=1)
        a.set_option("hipgraph", 1)
        a.set_precision("fp32")
        r32b = a.full(pair, img2, iterations=1)
        for k in KEYS + ("predict_depth0",):
            np.testing.assert_array_equal(r32[k], want32[k], err_msg=k)
            np.testing.assert_array_equal(r32b[k], want32[k], err_msg=k)
            np.testing.assert_array_equal(r16_eager[k], r16[k], err_msg=k)
        assert any(not np.array_equal(r16[k], r32[k]) for k in KEYS)
        # new weights after a bf16 run are honoured (set_weights, then copy_weights_from)
        a.set_precision("bf16")
        w_other = weights.synthetic_weights(seed=2)
        a.set_weights(w_other)
        got = a.full(pair, img2, iterations=1)
        ref = DemonContext(0, 2, 192, 256, precision="bf16")
        try:
            ref.set_weights(w_other)
            want = ref.full(pair, img2, iterations=1)
            for k in KEYS:
                np.testing.assert_array_equal(got[k], want[k], err_msg=k)
            fresh.set_precision("bf16")
            fresh.full(pair, img2, iterations=1)    # bf16 weights of the old slab exist ...
            fresh.copy_weights_from(ref)            # ... and are stale now
            got2 = fresh.full(pair, img2, iterations=1)
            for k in KEYS:
                np.testing.assert_array_equal(got2[k], want[k], err_msg=k)
        finally:
            ref.close()
    finally:
        a.close()
        fresh.close()


def test_lanes_in_bf16_mode(synth_weights):
    from demon_amd import DemonContext
    from demon_amd.lanes import LaneGroup
    pair, img2 = make_inputs(4, 192, 256, 11)
    g = LaneGroup(synth_weights, lanes=2, batch=4, precision="bf16")
    try:
        single = DemonContext(0, 4, 192, 256, precision="bf16")   # the lanes' launch plan: the fp32 layers run the same kernels
        try:
            single.set_weights(synth_weights)
            single.set_plan(4, g.ctxs[0].get_plan(4))
            want = single.full(pair, img2, iterations=1)
        finally:
            single.close()
        assert all(c.precision == "bf16" for c in g.ctxs) and g.mapping_key().endswith("_bf16")
        for c in g.ctxs:   # round robin: every lane on its own
            got = c.full(pair, img2, iterations=1)
            for k in KEYS:
                np.testing.assert_array_equal(got[k], want[k], err_msg=k)
        for c in g.ctxs:
            c.upload_inputs(pair, img2)
        g.run_group(4, 1, iterations=1)
        g.ctxs[0].synchronize()
        outs = [c.download_outputs(4) for c in g.ctxs]
        for o in outs:
            for k in KEYS:
                np.testing.assert_array_equal(o[k], want[k], err_msg=k)
        # one lane back to fp32: the group graph must not be replayed stale
        g.ctxs[1].set_precision("fp32")
        g.run_group(4, 1, iterations=1)
        g.ctxs[0].synchronize()
        o1 = g.ctxs[1].download_outputs(4)
        assert any(not np.array_equal(o1[k], want[k]) for k in KEYS)
        np.testing.assert_array_equal(g.ctxs[0].download_outputs(4)["predict_depth2"], want["predict_depth2"])
    finally:
        g.close()


@pytest.mark.parametrize("shape", [("conv", 48, 32, 1, 5, 1, 2, 5, 23), ("deconv", 128, 64, 0, 0, 0, 0, 17, 35), ("conv", 16, 40, 3, 3, 1, 1, 7, 9)])
def test_poison_guard_every_tile(shape):
    """the bf16 layer ops under DEMON_POISON_GUARD=1 (every allocation between quiet-NaN canaries): every tile, ragged shapes --
    finite, equal to the unguarded run, no write outside a tensor (the op checks the guards itself and raises)"""
    from demon_amd import DemonContext
    kind, cin, cout, kh, kw, sh, sw = shape[:7]
    x, w, b = _operands(shape, 42, n=2)
    plain = DemonContext.ops_only(0)
    os.environ["DEMON_POISON_GUARD"] = "1"
    try:
        guarded = DemonContext.ops_only(0)
    finally:
        os.environ.pop("DEMON_POISON_GUARD", None)
    try:
        for c in (plain, guarded):
            c.set_option("precision", 1)
        for t, (bm, bn) in enumerate(TILES):
            if -(-cout // 32) * 32 % bm:
                continue
            for ks in (1, 3):
                os.environ["DEMON_FORCE_PLAN"] = "17,%d,%d" % (t, ks)
                want = _run(plain, kind, x, w, b, (sh, sw), lrelu=True)
                os.environ["DEMON_POISON_GUARD"] = "1"
                try:
                    got = _run(guarded, kind, x, w, b, (sh, sw), lrelu=True)
                finally:
                    os.environ.pop("DEMON_POISON_GUARD", None)
                assert guarded.last_kernel().startswith("conv_bf16<%dx%d>" % (bm, bn))
                assert np.isfinite(got).all(), (t, ks)
                np.testing.assert_array_equal(got, want)
    finally:
        os.environ.pop("DEMON_FORCE_PLAN", None)
        plain.close()
        guarded.close()
