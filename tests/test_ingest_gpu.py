"""uint8 image pairs prepared on the GPU (demon_amd/csrc/ingest.hip) against the CPU statement of the same rule
(demon_amd.preprocess.prepare_input_arrays, itself held to Pillow and to the reference function's arrays by tests/test_ingest_cpu.py).

There is no tolerance in this file: the resize is a gather through Pillow's NEAREST index tables and the value is one IEEE float32
division and one float32 subtraction, so every comparison is np.array_equal -- on the prepared inputs (op level) and on every
output of the networks run from them (resident path, lanes, pipeline)."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
GOLDEN = os.path.join(HERE, "golden", "sculpture_inputs.npz")


def _images(n, h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8), rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def ops_ctx():
    from demon_amd import DemonContext
    ctx = DemonContext.ops_only(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def net_ctx(synth_weights):
    from demon_amd import DemonContext
    guard = os.environ.pop("DEMON_POISON_GUARD", None)
    try:
        ctx = DemonContext(0, 2, 192, 256)
    finally:
        if guard is not None:
            os.environ["DEMON_POISON_GUARD"] = guard
    ctx.set_weights(synth_weights)
    yield ctx
    ctx.close()


def _same(got, want, what=""):
    assert set(got) == set(want)
    for k in want:
        assert np.isfinite(got[k]).all(), (what, k)
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s %s" % (what, k))


# ---- op level -------------------------------------------------------------------------------------------------------------------
# n, source h x w, context H x W: identity (dword loads) / rows where floor((x + 0.5) src / dst) is wrong (128 -> 192), three images
# (batch offsets) / both axes discriminating (64 -> 480, 256 -> 640), 256-lane workgroups / odd source rows that start at unaligned
# bytes, a source larger than the destination on one axis and smaller on the other / the smallest source
@pytest.mark.parametrize("n,sh,sw,H,W", [(1, 192, 256, 192, 256), (3, 128, 320, 192, 256), (2, 64, 256, 480, 640), (2, 33, 61, 32, 64),
                                         (1, 1, 1, 32, 32)])
def test_prepare_inputs_equals_the_cpu_rule(ops_ctx, n, sh, sw, H, W):
    from demon_amd.preprocess import prepare_input_arrays
    u1, u2 = _images(n, sh, sw, seed=sh + sw)
    want_pair, want_22 = prepare_input_arrays(u1, u2, H, W)
    pair, img22 = ops_ctx.prepare_inputs(u1, u2, H, W)
    assert pair.dtype == np.float32 and pair.shape == (n, 6, H, W) and img22.shape == (n, 3, H // 4, W // 4)
    np.testing.assert_array_equal(pair, want_pair)
    np.testing.assert_array_equal(img22, want_22)


def test_prepare_inputs_golden_big_pair(ops_ctx):
    """the 512 x 384 pair of the golden file: the arrays the REFERENCE function produced, by their committed sha256"""
    import hashlib
    from demon_amd.preprocess import prepare_input_arrays
    from make_golden_inputs import big_pair
    g = np.load(GOLDEN)
    u1, u2 = big_pair(g["image1_u8"])[None], big_pair(g["image2_u8"])[None]
    pair, img22 = ops_ctx.prepare_inputs(u1, u2, 192, 256)
    want_pair, want_22 = prepare_input_arrays(u1, u2)
    np.testing.assert_array_equal(pair, want_pair)
    np.testing.assert_array_equal(img22, want_22)
    np.testing.assert_array_equal(img22, g["big_image2_2_channels_first_nearest"])
    assert hashlib.sha256(pair.tobytes()).hexdigest() == str(g["sha256_big_image_pair_channels_first_nearest"])
    assert hashlib.sha256(img22.tobytes()).hexdigest() == str(g["sha256_big_image2_2_channels_first_nearest"])


@pytest.mark.parametrize("resize", [False, True])
def test_all_256_values_in_every_channel(ops_ctx, resize):
    """every byte value in every channel of both images, on the identity path and on the gather path: the 256 quotients are numpy's"""
    from demon_amd.preprocess import prepare_input_arrays
    h, w = (32, 64) if not resize else (16, 48)
    ramp = (np.arange(h * w) % 256).astype(np.uint8).reshape(h, w)
    u1 = np.stack([ramp, ramp[::-1], np.roll(ramp, 7, axis=1)], axis=-1)[None]
    u2 = np.ascontiguousarray(u1[:, :, ::-1])
    for u in (u1, u2):
        for c in range(3):
            assert len(np.unique(u[..., c])) == 256
    pair, img22 = ops_ctx.prepare_inputs(np.ascontiguousarray(u1), u2, 32, 64)
    want_pair, want_22 = prepare_input_arrays(u1, u2, 32, 64)
    for c in range(6):
        assert len(np.unique(pair[0, c])) == 256
    np.testing.assert_array_equal(pair, want_pair)
    np.testing.assert_array_equal(img22, want_22)
    table = np.arange(256).astype(np.float32) / 255 - 0.5
    assert set(np.unique(pair).tolist()) == set(table.tolist())


def test_prepare_inputs_refuses_bad_arguments(ops_ctx):
    from demon_amd.engine import DemonError
    u1, u2 = _images(1, 8, 8, 0)
    with pytest.raises(DemonError):
        ops_ctx.prepare_inputs(u1, u2, 48, 64)               # not a multiple of 32
    with pytest.raises(DemonError):
        ops_ctx.prepare_inputs(u1.astype(np.float32), u2, 32, 32)
    with pytest.raises(DemonError):
        ops_ctx.prepare_inputs(u1[:, :, ::2], u2[:, :, ::2], 32, 32)   # row strides
    null = ctypes.POINTER(ctypes.c_uint8)()
    out = np.empty((1, 6, 32, 32), np.float32)
    q = np.empty((1, 3, 8, 8), np.float32)
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))   # noqa: E731
    assert ops_ctx.lib.demon_op_prepare_inputs_u8(ops_ctx.h, fp(out), fp(q), null, null, 1, 8, 8, 32, 32) == -1
    u8 = u1.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    assert ops_ctx.lib.demon_op_prepare_inputs_u8(ops_ctx.h, fp(out), fp(q), u8, u8, 1, 0, 8, 32, 32) == -1
    assert ops_ctx.lib.demon_ingest_configure(ops_ctx.h, 8, 8) == -1   # network contexts only


# ---- resident path --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hipgraph", [1, 0])
@pytest.mark.parametrize("sh,sw", [(192, 256), (128, 320)])
def test_upload_images_runs_like_upload_inputs(net_ctx, hipgraph, sh, sw):
    """upload_images + run_full == upload_inputs(prepare_input_arrays) + run_full on the same context, every output, bit for bit"""
    from demon_amd.preprocess import prepare_input_arrays
    ctx, n = net_ctx, 2
    ctx.set_option("hipgraph", hipgraph)
    try:
        u1, u2 = _images(n, sh, sw, seed=11 + sh)
        assert ctx.upload_inputs(*prepare_input_arrays(u1, u2)) == n
        ctx.run_full(n, 2)
        want = ctx.download_outputs(n)
        ctx.upload_inputs(np.zeros((n, 6, 192, 256), np.float32), np.zeros((n, 3, 48, 64), np.float32))   # nothing of `want` stays resident
        assert ctx.upload_images(u1, u2) == n
        ctx.run_full(n, 2)
        got = ctx.download_outputs(n)
        _same(got, want, "%dx%d" % (sh, sw))
        # other pixels through the same (cached) graph: the outputs follow the new inputs
        v1, v2 = _images(n, sh, sw, seed=12 + sh)
        ctx.upload_images(v1, v2)
        ctx.run_full(n, 2)
        other = ctx.download_outputs(n)
        assert not np.array_equal(other["predict_depth0"], got["predict_depth0"])
        ctx.upload_inputs(*prepare_input_arrays(v1, v2))
        ctx.run_full(n, 2)
        _same(other, ctx.download_outputs(n), "second upload")
        # one image of a larger staging: n below max_batch
        ctx.upload_images(u1[:1], u2[:1])
        ctx.run_full(1, 2)
        one = ctx.download_outputs(1)
        ctx.upload_inputs(*prepare_input_arrays(u1[:1], u2[:1]))
        ctx.run_full(1, 2)
        _same(one, ctx.download_outputs(1), "n = 1")
    finally:
        ctx.set_option("hipgraph", 1)


def test_upload_images_errors(net_ctx, synth_weights):
    from demon_amd import DemonContext
    from demon_amd.engine import DemonError
    lib = net_ctx.lib
    u1, u2 = _images(2, 24, 40, 3)
    p1, p2 = (u.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) for u in (u1, u2))
    fresh = DemonContext(0, 2, 192, 256)
    try:
        fresh.set_weights(synth_weights)
        # unconfigured: the raw calls say NOT_READY (the Python method configures by itself)
        assert lib.demon_upload_images_u8_async(fresh.h, 2, p1, p2) == -3
        assert lib.demon_upload_images_u8(fresh.h, 2, p1, p2) == -3
        assert "demon_ingest_configure" in lib.demon_last_error(fresh.h).decode()
        assert lib.demon_ingest_configure(fresh.h, 0, 40) == -1
        fresh.configure_ingest(24, 40)
        assert lib.demon_upload_images_u8_async(fresh.h, 0, p1, p2) == -1
        assert lib.demon_upload_images_u8_async(fresh.h, 3, p1, p2) == -1      # > max_batch
        assert lib.demon_upload_images_u8(fresh.h, 2, None, p2) == -1
        assert lib.demon_upload_images_u8(fresh.h, 2, p1, p2) == 0
        # a change of size replaces staging and tables; going back works too
        w1, w2 = _images(2, 50, 30, 4)
        assert fresh.upload_images(w1, w2) == 2 and fresh._ingest_size == (50, 30)
        assert fresh.upload_images(u1, u2) == 2 and fresh._ingest_size == (24, 40)
        fresh.release_streams()
        with pytest.raises(DemonError, match="demon_acquire_streams"):
            fresh.upload_images(u1, u2)
        assert lib.demon_upload_images_u8_async(fresh.h, 2, p1, p2) == -3
        fresh.acquire_streams()
        assert fresh.upload_images(u1, u2) == 2
        with pytest.raises(DemonError):
            fresh.upload_images(u1.astype(np.int8), u2.astype(np.int8))
        with pytest.raises(DemonError):
            fresh.upload_images(u1, u2[:, :, :20])
    finally:
        fresh.close()


# ---- lanes and pipeline ------------------------------------------------------------------------------------------------------------
def test_lane_group_upload_images(synth_weights):
    from demon_amd.lanes import LaneGroup
    from demon_amd.preprocess import prepare_input_arrays
    n = 2
    group = LaneGroup(synth_weights, lanes=3, batch=n)
    try:
        batches = [_images(n, 128, 320, seed=70 + i) for i in range(3)]
        assert group.upload_images(batches) == [n] * 3
        group.run_resident(n, 3, iterations=1)
        group.synchronize()
        got = [c.download_outputs(n) for c in group.ctxs]
        group.upload_inputs([prepare_input_arrays(*b) for b in batches])
        group.run_resident(n, 3, iterations=1)
        group.synchronize()
        for i, c in enumerate(group.ctxs):
            _same(got[i], c.download_outputs(n), "lane %d" % i)
        assert not np.array_equal(got[0]["predict_depth0"], got[1]["predict_depth0"])
    finally:
        group.close()


def test_pipeline_u8_buffers(synth_weights):
    from demon_amd.engine import DemonError
    from demon_amd.pipeline import Pipeline
    from demon_amd.preprocess import prepare_input_arrays
    pipe = Pipeline(synth_weights, batch=4)
    try:
        u1, u2 = _images(8, 128, 320, seed=80)
        hb = pipe.buffers(8, source_size=(128, 320))
        fb = pipe.buffers(8)
        try:
            assert hb.image1_u8.shape == (8, 128, 320, 3) and hb.image1_u8.dtype == np.uint8 and not hasattr(hb, "image_pair")
            hb.image1_u8[:], hb.image2_u8[:] = u1, u2
            fb.image_pair[:], fb.image2_2[:] = prepare_input_arrays(u1, u2)
            want = {k: v.copy() for k, v in pipe.run_buffers(fb, iterations=2).items()}
            got = pipe.run_buffers(hb, iterations=2)
            _same(got, want, "u8 buffers")
            again = {k: v.copy() for k, v in pipe.run_buffers(hb, iterations=2).items()}
            _same(again, want, "u8 buffers, second run")
        finally:
            hb.release()
            fb.release()
        _same(pipe.run_images(u1, u2, iterations=2), want, "run_images")
        with pytest.raises(DemonError):
            pipe.run_images(u1[:3], u2[:3])
    finally:
        pipe.close()


# ---- poison guard --------------------------------------------------------------------------------------------------------------------
def test_ingest_between_poisoned_neighbours(synth_weights):
    """staging, tables and input buffers flush between NaN canaries; odd source rows at full max_batch: nothing written outside, and
    the prepared inputs (seen through the networks) are those of the plain context"""
    from demon_amd import DemonContext
    from demon_amd.preprocess import prepare_input_arrays
    n = 3
    u1, u2 = _images(n, 33, 61, seed=9)
    old = os.environ.get("DEMON_POISON_GUARD")
    os.environ["DEMON_POISON_GUARD"] = "1"
    try:
        ctx = DemonContext(0, n, 192, 256)
    finally:
        if old is None:
            os.environ.pop("DEMON_POISON_GUARD", None)
        else:
            os.environ["DEMON_POISON_GUARD"] = old
    try:
        ctx.set_weights(synth_weights)
        ctx.configure_ingest(40, 40)          # replaced by the next call: the freed staging leaves the guard list
        assert ctx.upload_images(u1, u2) == n
        bad, where = ctx.check_guards()
        assert bad == 0, where
        ctx.run_full(n, 1)
        got = ctx.download_outputs(n)
        bad, where = ctx.check_guards()
        assert bad == 0, where
        ctx.upload_inputs(*prepare_input_arrays(u1, u2))
        ctx.run_full(n, 1)
        _same(got, ctx.download_outputs(n), "guarded")
    finally:
        ctx.close()
