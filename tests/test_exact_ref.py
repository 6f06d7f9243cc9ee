"""CPU checks of tests/exact_ref.py, the exact integer references the GPU tests hold the contraction kernels to:

  * exact() equals naive integer loops on tiny ragged shapes, for every kind and both paddings;
  * for every layer of the GPU tests' lists and every minimal-filtering table a kernel may run it on, the table restated in integers
    reproduces exact() (asserted inside wino_terms), every accumulator is exact in fp32 (sum |U||t| < 2^24), and for the tables
    whose output transform rounds: c <= 64 and the largest bound c 2^-24 (S + |b|) is below 1/48 -- half the smallest step (1/24) by
    which a wrong accumulator moves an output.  So the GPU checks can neither pass vacuously nor fail a correct kernel;
  * sensitivity: one output of a 192 x 256 layer that lost a tap, took a tap from the next row, or had one accumulator off by one
    is rejected by check_exact / check_rounded and accepted by the relative-L1 gate.  That is the gap these checks close."""
import numpy as np
import pytest

from conftest import rel_l1
import exact_ref as X


def _same(n, k, s):
    out = -(-n // s)
    tot = max((out - 1) * s + k - n, 0)
    return tot // 2, out


def _naive_conv(x, w, b, stride, padding):
    xi, wi = x.astype(np.int64), w.astype(np.int64)
    N, C, H, W = xi.shape
    kh, kw, _, O = wi.shape
    sh, sw = stride
    if padding == "same":
        (pt, Ho), (pl, Wo) = _same(H, kh, sh), _same(W, kw, sw)
    else:
        pt, pl, Ho, Wo = kh // 2, kw // 2, (H + 2 * (kh // 2) - kh) // sh + 1, (W + 2 * (kw // 2) - kw) // sw + 1
    out = np.zeros((N, O, Ho, Wo), np.int64) + b.astype(np.int64)[None, :, None, None]
    for y in range(Ho):
        for xo in range(Wo):
            for ky in range(kh):
                for kx in range(kw):
                    iy, ix = y * sh + ky - pt, xo * sw + kx - pl
                    if 0 <= iy < H and 0 <= ix < W:
                        out[:, :, y, xo] += xi[:, :, iy, ix] @ wi[ky, kx]
    return out


def _naive_deconv(x, w, b):
    """4x4 stride 2, padding 1: input pixel (y, x) adds x w[ky][kx] to output (2 y + ky - 1, 2 x + kx - 1)"""
    xi, wi = x.astype(np.int64), w.astype(np.int64)
    N, C, H, W = xi.shape
    O = wi.shape[2]
    out = np.zeros((N, O, 2 * H, 2 * W), np.int64) + b.astype(np.int64)[None, :, None, None]
    for y in range(H):
        for xx in range(W):
            for ky in range(4):
                for kx in range(4):
                    oy, ox = 2 * y + ky - 1, 2 * xx + kx - 1
                    if 0 <= oy < 2 * H and 0 <= ox < 2 * W:
                        out[:, :, oy, ox] += xi[:, :, y, xx] @ wi[ky, kx].T
    return out


@pytest.mark.parametrize("cfg", [(3, 5, 3, 3, 1, 1, 7, 9), (5, 4, 3, 1, 2, 1, 9, 5), (7, 3, 1, 5, 1, 2, 4, 11), (2, 3, 9, 1, 2, 1, 5, 3), (4, 2, 3, 3, 2, 2, 6, 8), (3, 2, 1, 7, 1, 2, 3, 10)])
@pytest.mark.parametrize("padding", ["caffe", "same"])
def test_exact_conv_equals_naive_integer_loops(cfg, padding):
    cin, cout, kh, kw, sh, sw, H, W = cfg
    x, w, b = X.int_operands("conv", (cin, cout, kh, kw, H, W), 5, 2)
    assert set(np.unique(np.abs(x))) <= {1, 2} and set(np.unique(np.abs(w))) <= {1, 2} and np.abs(b).max() <= 8
    want, mag = X.exact("conv", x, w, b, (sh, sw), padding)
    naive = _naive_conv(x, w, b, (sh, sw), padding)
    assert want.shape == naive.shape and np.array_equal(want, naive)
    assert np.array_equal(mag, _naive_conv(np.abs(x), np.abs(w), np.abs(b), (sh, sw), padding))


@pytest.mark.parametrize("cfg", [(5, 3, 3, 5), (4, 2, 6, 8), (7, 5, 1, 4)])
def test_exact_deconv_equals_naive_integer_loops(cfg):
    cin, cout, H, W = cfg
    x, w, b = X.int_operands("deconv", (cin, cout, 0, 0, H, W), 6, 2)
    want, mag = X.exact("deconv", x, w, b)
    assert np.array_equal(want, _naive_deconv(x, w, b)) and np.array_equal(mag, _naive_deconv(np.abs(x), np.abs(w), np.abs(b)))


@pytest.mark.parametrize("cfg", [(37, 5, 1), (128, 7, 4), (9, 33, 3)])
def test_exact_dense_equals_naive_integer_loops(cfg):
    cin, cout, n = cfg
    x, w, b = X.int_operands("dense", (cin, cout, 0, 0, 1, 1), 7, n)
    want, mag = X.exact("dense", x, w, b)
    naive = np.array([[sum(int(x[i, k]) * int(w[k, o]) for k in range(cin)) + int(b[o]) for o in range(cout)] for i in range(n)])
    assert np.array_equal(want, naive) and mag.max() <= 4 * cin + 8


def test_exact_refuses_what_is_not_exact():
    x, w, b = X.int_operands("dense", (16, 4, 0, 0, 1, 1), 1, 2)
    with pytest.raises(AssertionError):
        X.exact("dense", x + np.float32(0.5), w, b)
    with pytest.raises(AssertionError):
        X.exact("dense", x * np.float32(2 ** 12), w * np.float32(2 ** 12), b)   # sums past 2^24


def _gpu_layers():
    """(cin, cout, kh, kw, sh, sw, H, W, batch, padding) of every conv layer the GPU tests give an exact check, with the batch they run it at"""
    import test_bf16_gpu as B
    import test_layers_gpu as L
    import test_variants_gpu as V
    out = [l[1:] + (3, "caffe") for l in V.LAYERS if l[0] == "conv"]
    out += [l + (5, "caffe") for l in V.WINO1D_LAYERS]
    out += [(ci, co, 1, t, 1, 2, H, W, 3, "caffe") for ci, co, t, H, W in V.ROW_LAYERS]
    out += [(ci, co, 3, 3, 1, 1, H, W, 3, "caffe") for ci, co, H, W in V.WINO3_LAYERS + V.SMALL_LAYERS]
    out += [(ci, co, 3, 3, 2, 2, H, W, 3, "caffe") for ci, co, H, W in V.WINO3S2_LAYERS]
    out += [l + (3, "caffe") for l in V.WINO4_LAYERS]
    out += [l[:8] + (l[8], "caffe") for l in V.WINO4_FLAT_LAYERS]
    out += [(ci, co, kh, kw, 1, 1, H, W, V.WALK_BATCH, "caffe") for ci, co, kh, kw, H, W in V.WALK_LAYERS]
    out += [(ci, co, 9, 1, 2, 1, H, W, 3, "caffe") for ci, co, H, W in V.THIN_LAYERS]
    out += [l + (2, "caffe") for l in L.NET_CONVS if l[6] * l[7] < 96 * 128]
    out += [s[1:9] + (3, s[9] if len(s) > 9 else "caffe") for s in B.SHAPES if s[0] == "conv"]
    seen, uniq = set(), []
    for l in out:
        if l not in seen:
            seen.add(l)
            uniq.append(l)
    return uniq


def test_the_conditions_of_the_gpu_checks_hold_for_every_layer():
    """what makes the GPU assertions meaningful, on the very operands they use (same seed, same batch): the integer result exists
    below 2^24 for every layer; every table a kernel may run the layer on reproduces it with exact accumulators; c <= 64 and the
    largest tier-2 bound is below 1/48 -- also for the wino1d kernel's split-K at the factors the tests force (2, 3)"""
    import test_layers_gpu as L
    import test_variants_gpu as V
    worst = {}
    tables_met = set()
    for cin, cout, kh, kw, sh, sw, H, W in L.NET_CONVS:
        if H * W >= 96 * 128:   # (the large net shapes run under the heuristic plan only, which picks direct kernels: the integer result below 2^24 is all they need)
            X.Layer("conv", cin, cout, kh, kw, (sh, sw), H, W, n=2)
    for cin, cout, kh, kw, sh, sw, H, W, n, padding in _gpu_layers():
        lay = X.Layer("conv", cin, cout, kh, kw, (sh, sw), H, W, n=n, padding=padding)   # asserts integrality and sum |x||w| + |b| < 2^24
        for table in X.tables_for(kh, kw, sh, sw):
            t = lay.wino(table)   # asserts AT M == exact, M integral, sum |U||t| < 2^24
            tables_met.add(table)
            if X.tier1_table(table):
                continue
            absb = np.abs(lay.b).reshape(1, -1, 1, 1)
            cases = [(t["c"], t["S"])]
            if table in ("W2", "W3"):   # wino1d: the output transform per K slice
                cases += [(ks * 2 * t["nnz"] + ks, t["S_abs"]) for ks in (2, 3)]
            for c, S in cases:
                assert c <= 64, (table, c)
                bound = float((c * X.U24 * (S + absb)).max())
                assert bound < 1.0 / 48, (table, c, (cin, cout, kh, kw, sh, sw, H, W, n), bound)
                worst[(table, c)] = max(worst.get((table, c), 0.0), bound)
    assert tables_met == set(X.TABLES), tables_met
    for kind, shapes in (("deconv", [(ci, co, 0, 0, H, W, 3) for k, ci, co, _, _, _, _, H, W in V.LAYERS if k == "deconv"] + [(ci, co, 0, 0, H, W, 5) for ci, co, H, W in V.WINO_LAYERS]),
                         ("dense", [(ci, co, 0, 0, 1, 1, n) for n, ci, co in V.DENSE_LAYERS])):
        for s in shapes:
            x, w, b = X.int_operands(kind, s[:6], X.SEED, s[6])
            X.exact(kind, x, w, b)
    assert max(worst.values()) < 1.0 / 48 and len(worst) >= 9, worst


def test_counts_come_from_the_tables():
    """c = 2 nnz + 1 with nnz read off the generated AT; the smallest non-zero |AT| entry is the step an integer error makes"""
    want = {"W0": 3, "W1": 5, "W2": 7, "W3": 9, "F43": 5, "F4K5S2": 9, "F4K3S2": 5}
    for table, nnz in want.items():
        m = X.matrices(table)
        assert m["nnz"] == nnz and X.base_count(table) == 2 * nnz + 1 <= 64
        assert min(abs(v) for row in m["AT"] for v in row if v) >= 1 / 24
        assert X.tier1_table(table) == (table in ("W0", "W1"))
    for tag, tab in (("wino1d<t3x3,v2>", "W0"), ("wino1d<t9,v1>+splitk", "W3"), ("wino3rows<f4t3x3,v9>", "F43"), ("wino3rows<s2t3x3,v16>", "F4K3S2"),
                     ("wino4<t5,v3,flat>", "F4K5S2"), ("conv_row<32x128,t7>", "W2"), ("conv_mfma<128x32>+splitk", None), ("conv_small", None)):
        assert X.classify(tag)[1] == tab
    with pytest.raises(AssertionError):
        X.classify("conv_new_family<64x64>")
    for p in X.TIER1_PREFIXES + tuple(p for p, _ in X.WINO_TAGS):   # every family a plan can name (but the pair chains) has a tier
        X.classify(p + "64x64>")
    from test_plans_gpu import FAMILY
    for kind, prefixes in FAMILY.items():
        if kind not in (6, 7):
            assert all(any(q.startswith(p) for q in X.TIER1_PREFIXES + tuple(t for t, _ in X.WINO_TAGS)) for p in prefixes), prefixes


def _differing_tap(x, n, c, y, xx):
    """a column where the rows y and y + 1 of image n, channel c differ"""
    for dx in range(x.shape[3] - xx):
        if x[n, c, y, xx + dx] != x[n, c, y + 1, xx + dx]:
            return xx + dx
    raise AssertionError("rows are equal")


def test_one_wrong_element_is_seen_by_the_exact_checks_and_not_by_relative_l1():
    # tier 1: the first layer of the nets, 9 x 1 stride (2, 1) over the image pair at 192 x 256
    lay = X.Layer("conv", 6, 32, 9, 1, (2, 1), 192, 256, n=2)
    good = lay.want.astype(np.float32)
    X.check_exact(good, lay.want)
    n, co, y, xx, ky, c = 1, 17, 40, 255, 6, 3          # last pixel of a row, a tap inside the image
    iy = 2 * y + ky - 4
    dropped = good.copy()
    dropped[n, co, y, xx] -= lay.x[n, c, iy, xx] * lay.w[ky, 0, c, co]
    col = _differing_tap(lay.x, n, c, iy, 100)
    moved = good.copy()
    moved[n, co, y, col] += (lay.x[n, c, iy + 1, col] - lay.x[n, c, iy, col]) * lay.w[ky, 0, c, co]
    for bad in (dropped, moved):
        assert rel_l1(bad, lay.want) < 1e-5             # the aggregate gate accepts ...
        with pytest.raises(AssertionError, match="1 of"):
            X.check_exact(bad, lay.want)                # ... the per-element check names the element
    # tier 2: the 64 -> 16 conv of the refinement net's depth head at 192 x 256 on F(4,3) tiles
    lay = X.Layer("conv", 64, 16, 3, 3, (1, 1), 192, 256, n=2)
    t = lay.wino("F43")
    good = lay.want.astype(np.float32)
    assert X.check_rounded(good, lay.want, t["S"], t["c"], lay.b) == 0.0
    n, co, y, xx, ky, kx, c = 0, 5, 191, 252, 1, 2, 40
    dropped = good.copy()
    dropped[n, co, y, xx] -= lay.x[n, c, y + ky - 1, xx + kx - 1] * lay.w[ky, kx, c, co]
    col = _differing_tap(lay.x, n, c, y - 1, 8)
    moved = good.copy()      # tap (ky = 0, kx = 1) of output (y, col) read one row too low
    moved[n, co, y, col] += (lay.x[n, c, y, col] - lay.x[n, c, y - 1, col]) * lay.w[0, 1, c, co]
    shifted = good.copy()    # one accumulator of the tile off by one before the output transform: the smallest |AT| entry is 1/24
    shifted[n, co, y, xx] = np.float32(lay.want[n, co, y, xx] + 1.0 / 24)
    for bad in (dropped, moved, shifted):
        assert rel_l1(bad, lay.want) < 1e-5
        with pytest.raises(AssertionError, match="1 of"):
            X.check_rounded(bad, lay.want, t["S"], t["c"], lay.b)
        with pytest.raises(AssertionError):
            X.check_exact(bad, lay.want)
    # ... while the rounding the bound is there for passes: every output one fp32 rounding of (S + |b|) away
    mag = t["S"] + np.abs(lay.b).reshape(1, -1, 1, 1)
    ratio = X.check_rounded((lay.want + X.U24 * mag).astype(np.float32), lay.want, t["S"], t["c"], lay.b)
    assert 0 < ratio <= 2.0 / t["c"] + 1e-3
    assert float((t["c"] * X.U24 * mag).max()) < 1.0 / 48
