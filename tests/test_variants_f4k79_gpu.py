"""conv_wino4.hip kinds 2 and 3 (plan kind 16 on 7- / 9-tap stride-2 layers): four outputs per window, polyphase F(4,4) + F(4,3) -- 13
products instead of 28 -- and F(4,5) + F(4,4) -- 15 instead of 36 (tables: tests/test_wino_tables_f4k79.py).  Every workgroup shape
built for the kind, forced through DEMON_FORCE_PLAN, against PyTorch on the CPU and, per element, against the exact integer result
(tests/exact_ref.py's tier 2: c = 2 nnz + 1 = 23 / 27).  Also: the plan entries that were valid before these kinds existed launch
what they launched, and the tiles-per-workgroup field of a conv_row.hip plan entry (kind 13, ksplit) does not change a bit."""
import os
import re

import numpy as np
import pytest

from conftest import rel_l1
import exact_ref as X

pytestmark = pytest.mark.gpu

# The two tables and their tags, made known to exact_ref without editing it: the matrices enter its cache (through TABLES, which
# goes back to what it was -- tests/test_exact_ref.py holds TABLES against the layers of the older GPU tests), the tags its list.
NEW_TABLES = {"F4K7S2": ("kind_matrices4", 7, 2), "F4K9S2": ("kind_matrices4", 9, 2)}
for _name, _spec in NEW_TABLES.items():
    X.TABLES[_name] = _spec
    try:
        X.matrices(_name)
    finally:
        del X.TABLES[_name]
if not any(p == "wino4<t7," for p, _ in X.WINO_TAGS):
    X.WINO_TAGS = X.WINO_TAGS + (("wino4<t7,", "F4K7S2"), ("wino4<t9,", "F4K9S2"))

TABLE_OF = {7: "F4K7S2", 9: "F4K9S2"}
# operands of the exact check: +-1, +-2 for 7 taps; +-1 for 9 taps, whose |G| <= 16 and |BT| <= 21 would take sum |U||t| past what
# the bound below allows (asserted on the operands themselves in _exact_layer)
AMP = {7: 2, 9: 1}
HALF_STEP = {7: 1.0 / 240, 9: 1.0 / 720}   # half the smallest non-zero |AT| entry (1 / 120, 1 / 360)

# (cin, cout, kh, kw, sh, sw, H, W, padding).  A shape runs a layer only if its 16 WN positions per line block waste < 1.6 x, and a
# map narrower than a block must be a power of two wide, so:
#   along y (k x 1): position = pixel column -- 32 columns (one block) and 60 (two, the second ragged); 12, 12 and 18 output rows = 3, 3 and
#                    4 1/2 windows of 4 rows (the last one cut by Ho)
#   along x (1 x k): position = window of 4 outputs -- 32 outputs = 8 windows (narrower than a wave: 2 or 4 rows side by side in a
#                    block) and 244 outputs = 61 windows (a multiple of 4 and not of 8; two or four blocks, the last one ragged)
# Cin 20 / 22 / 18: no multiple of 4 (masked last K-step with one, two and four K groups per barrier), 24: of 4 and not of 16;
# Cout 24 / 36 / 40: no multiple of the 32- / 64-channel block
LAYERS = [(32, 64, 7, 1, 2, 1, 24, 32, "caffe"), (64, 64, 1, 7, 1, 2, 12, 64, "caffe"), (20, 24, 1, 7, 1, 2, 7, 488, "caffe"),
          (22, 36, 7, 1, 2, 1, 35, 60, "caffe"), (18, 40, 9, 1, 2, 1, 23, 60, "caffe"), (32, 32, 1, 9, 1, 2, 12, 64, "caffe"),
          (22, 40, 1, 9, 1, 2, 5, 488, "caffe"), (48, 64, 9, 1, 2, 1, 24, 32, "caffe"),
          # the v2 model's padding of a stride-2 conv: (taps - 2) / 2 on the left, one more on the right
          # (24 channels: masked with four K groups per barrier, i.e. shapes 6 and 7, and not with one or two; 32: never masked)
          (24, 64, 1, 7, 1, 2, 6, 64, "same"), (20, 48, 1, 9, 1, 2, 5, 488, "same"), (32, 64, 1, 9, 1, 2, 6, 64, "same"),
          # along y a map of 16 columns: two lines side by side in a block of 32 positions
          (32, 32, 7, 1, 2, 1, 24, 16, "caffe"), (32, 32, 9, 1, 2, 1, 24, 16, "caffe")]

# what conv_wino4.hip builds (w4_shape_built: no scratch in any instance), restated: shape -> (16-channel blocks per workgroup);
# (taps, axis) -> shapes.  Every layer above is sized so that the geometry admits each of them; Cout decides the channel block.
CHANNEL_BLOCKS = {6: 4, 7: 2, 8: 2, 14: 2, 15: 4}
BUILT = {(7, "y"): (8, 14, 15), (7, "x"): (6, 7, 8, 14, 15), (9, "y"): (14, 15), (9, "x"): (7, 14, 15)}


def _expected_shapes(layer):
    cin, cout, kh, kw = layer[:4]
    mpad = -(-cout // 32) * 32
    return [v for v in BUILT[(max(kh, kw), "y" if kw == 1 else "x")] if mpad % (16 * CHANNEL_BLOCKS[v]) == 0]


def _whole_launch():
    """kRowWholeLaunch of internal.h"""
    with open(os.path.join(X.ROOT, "demon_amd", "csrc", "internal.h")) as f:
        return int(re.search(r"kRowWholeLaunch\s*=\s*(\d+)", f.read()).group(1))


def _ref(x, w, b, stride, padding):
    import torch
    import torch.nn.functional as F
    kh, kw = w.shape[:2]
    pt, pb, _ = X._pads(x.shape[2], kh, stride[0], padding)
    pl, pr, _ = X._pads(x.shape[3], kw, stride[1], padding)
    y = F.conv2d(F.pad(torch.from_numpy(x), (pl, pr, pt, pb)), torch.from_numpy(np.ascontiguousarray(w.transpose(3, 2, 0, 1))), torch.from_numpy(b), stride=stride)
    return torch.where(y >= 0, y, 0.1 * y).numpy()


def _exact_layer(cin, cout, kh, kw, sh, sw, H, W, padding, n):
    """the layer's integer operands with the conditions that make its per-element check discriminate, asserted on those operands:
    sum |U||t| < 2^24 for every accumulator (wino_terms) and the largest bound below half the smallest step an integer error in one
    accumulator moves an output by"""
    taps = max(kh, kw)
    ex = X.Layer("conv", cin, cout, kh, kw, (sh, sw), H, W, n=n, padding=padding, amp=AMP[taps])
    t = ex.wino(TABLE_OF[taps])
    assert t["c"] == {7: 23, 9: 27}[taps]
    bound = float((t["c"] * X.U24 * (t["S"] + np.abs(ex.b).reshape(1, -1, 1, 1))).max())
    assert bound < HALF_STEP[taps], (taps, bound)
    return ex


@pytest.mark.parametrize("layer", LAYERS)
def test_four_outputs_per_window_7_and_9_taps(gpu_ctx, layer):
    """relative L1 against PyTorch below 1e-5 (numpy's figure for the integer-scaled tables at K = 64: 5.3e-7 / 6.7e-7,
    tools/wino_f4_error.py), run-to-run bit equality, lrelu(linear) == fused, and the exact integer result per element"""
    cin, cout, kh, kw, sh, sw, H, W, padding = layer
    taps = max(kh, kw)
    rng = np.random.default_rng(41)
    n = 3
    x = rng.standard_normal((n, cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((kh, kw, cin, cout)) / np.sqrt(kh * kw * cin)).astype(np.float32)
    b = rng.standard_normal((cout,)).astype(np.float32)
    want = _ref(x, w, b, (sh, sw), padding)
    ex = _exact_layer(cin, cout, kh, kw, sh, sw, H, W, padding, n)
    ran = []
    try:
        for v in range(16):
            os.environ["DEMON_FORCE_PLAN"] = "16,%d,1" % v
            got = gpu_ctx.conv2d(x, w, b, (sh, sw), lrelu=True, padding=padding)
            tag = gpu_ctx.last_kernel()
            if not tag.startswith("wino4<"):
                continue   # shape not built for this kind and axis, Cout not a multiple of its channel block, too much waste
            assert tag == "wino4<t%d,v%d>" % (taps, v), tag
            ran.append(v)
            assert got.shape == want.shape
            err = rel_l1(got, want)
            print("%s %s: rel L1 %.3e" % (layer, tag, err))
            assert err < 1e-5, "variant %d (%s): rel L1 %.3e" % (v, tag, err)
            np.testing.assert_array_equal(got, gpu_ctx.conv2d(x, w, b, (sh, sw), lrelu=True, padding=padding))
            lin = gpu_ctx.conv2d(x, w, b, (sh, sw), lrelu=False, padding=padding)
            assert gpu_ctx.last_kernel() == tag
            np.testing.assert_array_equal(np.where(lin >= 0, lin, np.float32(0.1) * lin), got)
            ex.saw_rel(tag, 1)
            ex.check(gpu_ctx, 1, expect="wino4<t%d," % taps)
        assert ran == _expected_shapes(layer), (layer, ran)   # a shape that is no longer built or admitted does not pass in silence
        assert ex.finish() == {"wino4<"}
    finally:
        os.environ.pop("DEMON_FORCE_PLAN", None)


def test_plan_entries_from_before_keep_their_kernels(gpu_ctx):
    """`13,0,1` is conv_row<32x128,t9> / <..,t7> with three tiles per workgroup, `16,v,1` on a 5-tap layer is wino4<t5,v>, and a
    kind-16 entry with a shape that a 7- / 9-tap kind does not build falls back as any entry that does not fit"""
    rng = np.random.default_rng(42)
    try:
        for taps in (9, 7):
            x = rng.standard_normal((3, 32, 6, 256)).astype(np.float32)
            w = (rng.standard_normal((1, taps, 32, 32)) / np.sqrt(taps * 32)).astype(np.float32)
            b = rng.standard_normal((32,)).astype(np.float32)
            os.environ["DEMON_FORCE_PLAN"] = "13,0,1"
            gpu_ctx.conv2d(x, w, b, (1, 2), lrelu=True)
            assert gpu_ctx.last_kernel() == "conv_row<32x128,t%d>" % taps
            os.environ["DEMON_FORCE_PLAN"] = "16,0,1"   # four lines per wave: 208 / 240 accumulators, not built
            gpu_ctx.conv2d(x, w, b, (1, 2), lrelu=True)
            assert not gpu_ctx.last_kernel().startswith("wino4<"), gpu_ctx.last_kernel()
        x = rng.standard_normal((3, 64, 48, 64)).astype(np.float32)
        w = (rng.standard_normal((5, 1, 64, 128)) / np.sqrt(5 * 64)).astype(np.float32)
        b = rng.standard_normal((128,)).astype(np.float32)
        for v in (4, 8):
            os.environ["DEMON_FORCE_PLAN"] = "16,%d,1" % v
            gpu_ctx.conv2d(x, w, b, (2, 1), lrelu=True)
            assert gpu_ctx.last_kernel() == "wino4<t5,v%d>" % v
        for v in (14, 15):   # the new shapes belong to the 7- / 9-tap kinds alone
            os.environ["DEMON_FORCE_PLAN"] = "16,%d,1" % v
            gpu_ctx.conv2d(x, w, b, (2, 1), lrelu=True)
            assert not gpu_ctx.last_kernel().startswith("wino4<"), gpu_ctx.last_kernel()
    finally:
        os.environ.pop("DEMON_FORCE_PLAN", None)


@pytest.mark.parametrize("taps", [9, 7])
def test_row_tiles_per_workgroup_is_bit_identical(gpu_ctx, taps):
    """conv_row.hip, ksplit field of a kind-13 plan entry = tiles a workgroup walks before it retires (0 / 1: three; kRowWholeLaunch:
    two workgroups per CU for the whole launch; a value outside {0, 1, 3, 6, 12, kRowWholeLaunch} means three, as every value did
    before the field had a meaning).  576 tiles: more than the 512 workgroups of a whole-launch grid, so every value walks."""
    rng = np.random.default_rng(43)
    x = rng.standard_normal((6, 32, 96, 256)).astype(np.float32)
    w = (rng.standard_normal((1, taps, 32, 32)) / np.sqrt(taps * 32)).astype(np.float32)
    b = rng.standard_normal((32,)).astype(np.float32)
    try:
        os.environ["DEMON_FORCE_PLAN"] = "13,0,1"
        ref = gpu_ctx.conv2d(x, w, b, (1, 2), lrelu=True)
        assert gpu_ctx.last_kernel() == "conv_row<32x128,t%d>" % taps
        assert np.isfinite(ref).all() and np.abs(ref).max() > 0
        for tpw in (0, 2, 3, 6, 12, _whole_launch()):
            os.environ["DEMON_FORCE_PLAN"] = "13,0,%d" % tpw
            got = gpu_ctx.conv2d(x, w, b, (1, 2), lrelu=True)
            assert gpu_ctx.last_kernel() == "conv_row<32x128,t%d>" % taps
            np.testing.assert_array_equal(got, ref, err_msg="tiles per workgroup %d" % tpw)
    finally:
        os.environ.pop("DEMON_FORCE_PLAN", None)
