"""Exact integer references for the contraction kernels (conv, 4x4 stride-2 transposed conv, dense), checked PER ELEMENT.

The relative-L1 gate of the GPU tests is one sum over a whole tensor: one output that lost one tap moves it by ~1e-7 against a bar
of 1e-5.  Here the kernels are fed small NON-ZERO integers (x, w in {-2, -1, 1, 2}, b in -8 .. 8).  Every product and every partial
sum is then an integer far below 2^24, exactly representable in fp32, so any order of summation, any tile, any split-K, the fp32
MFMA and the bf16 MFMA with fp32 accumulation must return THE integer result, and because no operand is 0 a neighbour read in
place of padding is as visible as a dropped tap.

  tier 1  np.array_equal with the integer result: every direct family, every split-K, conv_bf16, wino_deconv (its transforms are
          sums and differences only) and the minimal-filtering tables whose output transform has denominators 1 and 2 only (half
          of an integer is exact).
  tier 2  the tables with denominators 3, 6, 12, 24 in the output transform (7 / 9 taps, every F(4,.) form): everything up to the
          accumulators M_e is exact, the output transform o_k = sum_e AT[k][e] M_e and the bias add round:
              |got - want| <= c 2^-24 (S + |b|),      S = sum_e |AT[k][e]| |M_e|
          c = 2 nnz + 1: one multiplication and one addition per non-zero entry of the table's fullest AT row (nnz), plus the bias
          add; the activation with lrelu = False is max(v, 1.0f * v), exact.  This count is also a rigorous bound: a term of the
          sum passes through at most nnz + 2 roundings (its coefficient's fp32 value, its product, nnz - 1 additions, the bias
          add), each of relative size 2^-24 on a partial sum of magnitude <= S + |b|, whether or not the compiler contracts
          multiply-adds.  Where the wino1d kernel runs split-K (conv_wino.hip, a.ksplit > 1) every slice applies the output
          transform to its own accumulators and conv_splitk_reduce adds the ks partial outputs and the bias:
              c = ks (2 nnz) + ks      (ks transforms, ks - 1 slice additions, the bias add)
          and S becomes the sum of the slices' S, which is bounded for ANY partition of the reduction by
              S_abs = sum_e |AT[k][e]| sum_(channel, kernel row) |U_e t_e|.
          conv_row, wino3rows and wino4 (plain, walking, flat) accumulate over channels and kernel rows into ONE set of
          accumulators and transform once (their epilogues): c = 2 nnz + 1 for them.
          An integer error in any M_e moves an output by at least 1/24 (the smallest non-zero |AT| entry); the CPU suite
          (tests/test_exact_ref.py) asserts c <= 64 and max bound < 1/48 for every layer the GPU tests run, so a tier-2 check can
          neither pass a wrong accumulator nor fail a correct kernel.

The matrices come from tools/gen_wino1d.py (integer G and BT, rational AT); tests/test_wino_tables.py proves the committed header is
what that generator writes, so they are the specification and not the code under test.
"""
import atexit
import importlib.util
import json
import os
from fractions import Fraction as Fr
from math import lcm

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO24 = float(2 ** 24)
U24 = 2.0 ** -24
SEED = 2024

# table -> (generator function, taps, stride); Wino1D<0..3>, Wino43, Wino4K5S2, Wino4K3S2 of wino1d_tables.h
TABLES = {"W0": ("kind_matrices", 3, 1), "W1": ("kind_matrices", 5, 2), "W2": ("kind_matrices", 7, 2), "W3": ("kind_matrices", 9, 2),
          "F43": ("kind_matrices4", 3, 1), "F4K5S2": ("kind_matrices4", 5, 2), "F4K3S2": ("kind_matrices4", 3, 2)}
_cache = {}


def _gen():
    if "gen" not in _cache:
        spec = importlib.util.spec_from_file_location("gen_wino1d", os.path.join(ROOT, "tools", "gen_wino1d.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _cache["gen"] = mod
    return _cache["gen"]


def matrices(table):
    """AT (rationals, OUT x NUV), G and BT (integer float64 arrays), WIN, OUT, taps, stride of a table; nnz of the fullest AT row,
    the common denominator of AT"""
    if table not in _cache:
        fn, taps, stride = TABLES[table]
        gen = _gen()
        AT, G, BT, win = getattr(gen, fn)(taps, stride)
        AT, G = gen.normalise(AT, G)
        assert all(v.denominator == 1 for row in G for v in row) and all(v.denominator == 1 for row in BT for v in row)
        den = 1
        for row in AT:
            for v in row:
                den = lcm(den, v.denominator)
        _cache[table] = dict(AT=AT, G=np.array([[float(v) for v in row] for row in G]), BT=np.array([[float(v) for v in row] for row in BT]),
                             win=win, out=len(AT), taps=taps, stride=stride, nnz=max(sum(1 for v in row if v) for row in AT), den=den,
                             ATi=np.array([[float(v * den) for v in row] for row in AT]), ATf=np.array([[float(v) for v in row] for row in AT]))
    return _cache[table]


def tier1_table(table):
    """denominators 1 and 2 only: the output transform of integers is exact"""
    return matrices(table)["den"] <= 2


def base_count(table):
    """c of one output transform plus the bias add"""
    return 2 * matrices(table)["nnz"] + 1


def tables_for(kh, kw, sh, sw):
    """the minimal-filtering tables a kernel of this project may run a conv layer of this geometry on"""
    if (kh, kw) == (3, 3):
        return ["W0", "F43"] if (sh, sw) == (1, 1) else (["F4K3S2"] if (sh, sw) == (2, 2) else [])
    if min(kh, kw) != 1:
        return []
    taps, s, so = max(kh, kw), (sh if kw == 1 else sw), (sw if kw == 1 else sh)
    if so != 1:
        return []
    return {(3, 1): ["W0", "F43"], (5, 2): ["W1", "F4K5S2"], (7, 2): ["W2"], (9, 2): ["W3"]}.get((taps, s), [])


# ---- operands and the integer result ---------------------------------------------------------------------------------------------
def int_operands(kind, shape, seed, n, amp=2):
    """x, w, b as float32 holding integers: x, w uniform in {-amp .. -1, 1 .. amp} (never 0), b in -8 .. 8.
    shape = (cin, cout, kh, kw, H, W); TF layouts: conv w [kh][kw][Cin][Cout], deconv w [4][4][Cout][Cin], dense x [n][Cin], w [Cin][Cout]"""
    cin, cout, kh, kw, H, W = shape
    rng = np.random.default_rng(seed)

    def nz(size):
        v = rng.integers(1, amp + 1, size=size)
        return (v * (2 * rng.integers(0, 2, size=size) - 1)).astype(np.float32)
    if kind == "dense":
        x, w = nz((n, cin)), nz((cin, cout))
    elif kind == "deconv":
        x, w = nz((n, cin, H, W)), nz((4, 4, cout, cin))
    else:
        x, w = nz((n, cin, H, W)), nz((kh, kw, cin, cout))
    b = rng.integers(-8, 9, size=(cout,)).astype(np.float32)
    assert (x != 0).all() and (w != 0).all()
    return x, w, b


def _pads(n, k, s, padding):
    """(zeros before, zeros after, outputs) along one axis"""
    if padding == "same":
        no = -(-n // s)
        tot = max((no - 1) * s + k - n, 0)
        return tot // 2, tot - tot // 2, no
    assert padding == "caffe", padding
    return k // 2, k // 2, (n + 2 * (k // 2) - k) // s + 1


def exact(kind, x, w, b, stride=(1, 1), padding="caffe"):
    """(want, mag): the layer's result in exact arithmetic (float64 on integers: asserted integral) and sum |x||w| + |b| per element,
    asserted < 2^24 -- the condition under which every fp32 summation order gives `want`"""
    import torch
    import torch.nn.functional as F

    def lin(x, w, b):
        xt, bt = torch.from_numpy(x.astype(np.float64)), torch.from_numpy(b.astype(np.float64))
        if kind == "dense":
            return (xt @ torch.from_numpy(w.astype(np.float64)) + bt).numpy()
        wt = torch.from_numpy(np.ascontiguousarray(w.transpose(3, 2, 0, 1)).astype(np.float64))
        if kind == "deconv":
            return F.conv_transpose2d(xt, wt, bt, stride=2, padding=1).numpy()
        assert kind == "conv", kind
        kh, kw = w.shape[:2]
        pt, pb, _ = _pads(x.shape[2], kh, stride[0], padding)
        pl, pr, _ = _pads(x.shape[3], kw, stride[1], padding)
        return F.conv2d(F.pad(xt, (pl, pr, pt, pb)), wt, bt, stride=stride).numpy()
    for a in (x, w, b):
        assert np.array_equal(a, np.rint(a)), "operands must be integers"
    want, mag = lin(x, w, b), lin(np.abs(x), np.abs(w), np.abs(b))
    assert np.array_equal(want, np.rint(want))
    assert mag.max() < TWO24, "sum |x||w| + |b| = %g: not exact in fp32" % mag.max()
    return want, mag


def wino_terms(table, x, w, b, stride=(1, 1), padding="caffe"):
    """The minimal-filtering algorithm of `table` restated on integers, as the kernels run it: windows of WIN inputs per OUT outputs
    along the filter axis (x for 1 x k and 3 x 3 layers, y for k x 1), t = BT d, U = G g, accumulators M_e = sum over input channels
    and kernel rows of U_e t_e, outputs AT M.  Input past the image is zero (also in the windows of a ragged last tile, whose unused
    outputs the kernels drop).  Returns a dict: S = sum_e |AT[k][e]| |M_e| and S_abs = sum_e |AT[k][e]| sum |U_e t_e| per output
    element, c (one transform + bias add), nnz, M [n][co][y][tile][e] (filter axis last; transposed layers: [n][co][x][tile][e]),
    transposed.  Asserts AT M + b == exact(...) in rationals (both sides times the common denominator, in integers), that M is
    integral and that sum |U||t| < 2^24 for every accumulator."""
    m = matrices(table)
    kh, kw = w.shape[:2]
    transposed = kw == 1 and kh > 1
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    sy, sx = stride
    if transposed:
        x64, w64, sy, sx = x64.transpose(0, 1, 3, 2), w64.transpose(1, 0, 2, 3), sx, sy
    R, taps = w64.shape[:2]
    assert taps == m["taps"] and sx == m["stride"], (table, w.shape, stride)
    N, C, H, W = x64.shape
    cout = w64.shape[3]
    pt, pb, Ho = _pads(H, R, sy, padding)
    pl, pr, Wo = _pads(W, taps, sx, padding)
    OUT, win, NUV = m["out"], m["win"], m["G"].shape[0]
    T = -(-Wo // OUT)
    need = (T - 1) * OUT * sx + win
    rows_need = (Ho - 1) * sy + R
    xp = np.pad(x64, ((0, 0), (0, 0), (pt, max(0, rows_need - pt - H)), (pl, max(0, need - pl - W))))
    idx = (np.arange(T) * OUT * sx)[:, None] + np.arange(win)[None, :]
    t = xp[..., idx] @ m["BT"].T                                   # [n][ci][row][tile][e]
    U = np.einsum("et,ktio->keio", m["G"], w64)                    # [ky][e][ci][co]
    M = np.zeros((N, cout, Ho, T, NUV))
    Mabs = np.zeros_like(M)
    for ky in range(R):
        ts = t[:, :, ky:ky + (Ho - 1) * sy + 1:sy]                 # rows y * sy + ky of the padded input
        for e in range(NUV):
            te = np.ascontiguousarray(ts[..., e])
            M[..., e] += np.einsum("io,niyj->noyj", U[ky, e], te, optimize=True)
            Mabs[..., e] += np.einsum("io,niyj->noyj", np.abs(U[ky, e]), np.abs(te), optimize=True)
    assert np.array_equal(M, np.rint(M))
    assert Mabs.max() < TWO24, "sum |U||t| = %g: the accumulators are not exact in fp32" % Mabs.max()

    def spread(A, V):   # [n][co][y][tile][e] x [k][e] -> [n][co][y][Wo]
        return np.einsum("noyje,ke->noyjk", V, A).reshape(N, cout, Ho, T * OUT)[..., :Wo]
    want, _ = exact("conv", x, w, b, stride, padding)
    wt = want.transpose(0, 1, 3, 2) if transposed else want
    assert wt.shape == (N, cout, Ho, Wo), (wt.shape, (N, cout, Ho, Wo))
    outL = spread(m["ATi"], M) + m["den"] * b.astype(np.float64)[None, :, None, None]
    assert np.array_equal(outL, m["den"] * wt), "%s: AT M differs from the direct sum" % table
    S, S_abs = spread(np.abs(m["ATf"]), np.abs(M)), spread(np.abs(m["ATf"]), Mabs)
    if transposed:
        S, S_abs = S.transpose(0, 1, 3, 2), S_abs.transpose(0, 1, 3, 2)
    return dict(S=S, S_abs=S_abs, c=base_count(table), nnz=m["nnz"], M=M, transposed=transposed, want=want, table=table)


# ---- the checks --------------------------------------------------------------------------------------------------------------------
def _worst(got, want, bad, excess):
    i = np.unravel_index(np.argmax(np.where(bad, excess, -np.inf)), got.shape)
    return "%d of %d elements off; worst at %s: got %r, want %r" % (int(bad.sum()), got.size, tuple(int(v) for v in i), float(got[i]), float(want[i]))


def check_exact(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    got64 = got.astype(np.float64)
    if np.array_equal(got64, want):
        return
    bad = ~(got64 == want)      # (a NaN counts)
    raise AssertionError("%s: not the exact integer result: %s" % (what, _worst(got64, want, bad, np.where(np.isfinite(got64), np.abs(got64 - want), np.inf))))


def check_rounded(got, want, S, c, b=None, what=""):
    """|got - want| <= c 2^-24 (S + |b|) per element (b per output channel); returns the largest |got - want| / bound"""
    assert got.shape == want.shape == S.shape, (what, got.shape, want.shape, S.shape)
    mag = S if b is None else S + np.abs(b.astype(np.float64)).reshape((1, -1) + (1,) * (S.ndim - 2))
    bound = c * U24 * mag
    got64 = got.astype(np.float64)
    err = np.abs(got64 - want)
    bad = ~(err <= bound)
    if bad.any():
        ratio = np.where(np.isfinite(err), err / np.maximum(bound, 1e-300), np.inf)
        raise AssertionError("%s: outside c 2^-24 (S + |b|), c = %d: %s (%.3g x the bound)" % (what, c, _worst(got64, want, bad, ratio), ratio[bad].max()))
    return float((err / np.maximum(bound, 1e-300)).max())


def lrelu32(v):
    """fp32 leaky ReLU of an fp32 array, as every epilogue computes it (v or 0.1f * v)"""
    v = np.asarray(v, np.float32)
    return np.where(v >= 0, v, np.float32(0.1) * v)


# ---- kernel tag -> tier ------------------------------------------------------------------------------------------------------------
TIER1_PREFIXES = ("conv_mfma<", "conv_patch<", "deconv4<", "conv_small", "conv_stream<", "conv_frag<", "dense_stream<", "conv_thin<", "wino_deconv<", "conv_bf16<")
WINO_TAGS = (("wino1d<t3x3,", "W0"), ("wino1d<t3,", "W0"), ("wino1d<t5,", "W1"), ("wino1d<t7,", "W2"), ("wino1d<t9,", "W3"),
             ("wino3rows<t3x3,", "W0"), ("wino3rows<f4t3x3,", "F43"), ("wino3rows<s2t3x3,", "F4K3S2"),
             ("wino4<t3,", "F43"), ("wino4<t5,", "F4K5S2"), ("conv_row<32x128,t7>", "W2"), ("conv_row<32x128,t9>", "W3"))


def classify(tag):
    """(family prefix, table or None); a tag that belongs to no tier is an error, so that a new family cannot enter unchecked"""
    for p in TIER1_PREFIXES:
        if tag.startswith(p):
            return p, None
    for p, table in WINO_TAGS:
        if tag.startswith(p):
            return tag[:tag.index("<") + 1], table
    raise AssertionError("kernel tag %r belongs to no tier of the exact checks" % tag)


# what the GPU tests observed: family -> {tier, c, largest |got - want| / bound, checks}; written as JSON at exit when DEMON_EXACT_REPORT names a file
REPORT = {}


def _note(family, tier, c, ratio):
    r = REPORT.setdefault(family, {"tier": tier, "c": [], "worst_ratio": 0.0, "checks": 0})
    r["tier"] = max(r["tier"], tier)
    if c and c not in r["c"]:
        r["c"] = sorted(r["c"] + [c])
    r["worst_ratio"] = max(r["worst_ratio"], ratio)
    r["checks"] += 1


@atexit.register
def _write_report():
    path = os.environ.get("DEMON_EXACT_REPORT")
    if path and REPORT:
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


class Layer:
    """One layer's integer operands and exact result (computed once), and the book-keeping of a GPU test: which (tag, split-K) got
    a relative-L1 check, which got an exact one."""

    def __init__(self, kind, cin, cout, kh=1, kw=1, stride=(1, 1), H=1, W=1, n=3, padding="caffe", seed=SEED, amp=2):
        self.kind, self.stride, self.padding = kind, tuple(stride), padding
        self.geom = (cin, cout, kh, kw, H, W)
        self.x, self.w, self.b = int_operands(kind, self.geom, seed, n, amp)
        self.want, self.mag = exact(kind, self.x, self.w, self.b, self.stride, padding)
        self.terms = {}
        self.rel_seen, self.exact_seen, self.act_seen = set(), set(), set()
        self.families = set()

    def wino(self, table):
        if table not in self.terms:
            self.terms[table] = wino_terms(table, self.x, self.w, self.b, self.stride, self.padding)
        return self.terms[table]

    def run(self, ctx, lrelu):
        if self.kind == "deconv":
            return ctx.deconv4x4s2(self.x, self.w, self.b, lrelu=lrelu)
        if self.kind == "dense":
            return ctx.dense(self.x, self.w, self.b, lrelu=lrelu)
        return ctx.conv2d(self.x, self.w, self.b, self.stride, lrelu=lrelu, padding=self.padding)

    def bound_terms(self, tag, ks):
        """(S, c) of the tier-2 check of a launch with this tag; ks = the split-K factor asked for (the library may clamp it: fewer
        slices, fewer operations -- c counts the ks asked for)"""
        _, table = classify(tag)
        t = self.wino(table)
        if tag.startswith("wino1d<") and "+splitk" in tag:
            assert ks > 1, (tag, ks)
            return t["S_abs"], ks * 2 * t["nnz"] + ks
        return t["S"], t["c"]

    def saw_rel(self, tag, ks=0):
        self.rel_seen.add((tag, ks))

    def check(self, ctx, ks=0, expect=None):
        """one launch with lrelu = False on the integer operands under whatever plan is forced, held to its tier by the tag
        last_kernel() reports; once per distinct tag also the activation: lrelu = True equals the fp32 leaky ReLU of that result
        bit for bit.  A (tag, split-K) pair already checked on this layer is not launched again (a forced plan that does not fit
        a layer falls back to the same kernel many times over).  Returns the tag."""
        got = self.run(ctx, False)
        tag = ctx.last_kernel()
        if expect is not None:
            assert tag.startswith(expect), (tag, expect)
        key = (tag, ks)
        if key in self.exact_seen:
            return tag
        family, table = classify(tag)
        what = "%s %s %s %s split %d (%s)" % (self.kind, self.geom, self.stride, self.padding, ks, tag)
        if table is None or tier1_table(table):
            if family == "wino_deconv<":
                assert 64 * self.geom[0] < TWO24   # tap sums |U| <= 4 * 2, differences of differences |t| <= 4 * 2, nine products per channel
            if table is not None:
                self.wino(table)                    # asserts sum |U||t| < 2^24 and that the table reproduces the direct sum
            check_exact(got, self.want, what)
            _note(family, 1, 0, 0.0)
        else:
            S, c = self.bound_terms(tag, ks)
            ratio = check_rounded(got, self.want, S, c, self.b, what)
            _note(family, 2, c, ratio)
        if tag not in self.act_seen:
            act = self.run(ctx, True)
            assert ctx.last_kernel() == tag, (ctx.last_kernel(), tag)
            if not np.array_equal(act, lrelu32(got)):
                bad = act != lrelu32(got)
                raise AssertionError("%s: lrelu = True is not the leaky ReLU of the lrelu = False result: %s" % (what, _worst(act, lrelu32(got), bad, bad.astype(np.float64))))
            self.act_seen.add(tag)
        self.exact_seen.add(key)
        self.families.add(family)
        return tag

    def finish(self):
        missing = self.rel_seen - self.exact_seen
        assert not missing, "relative-L1 checked but not exactly: %s" % sorted(missing)
        assert self.exact_seen, "no exact check ran"
        return self.families
