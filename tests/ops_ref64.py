"""Float64 references with PER ELEMENT error bounds for the geometry and loss ops of demon_amd/csrc/ops.hip.

tests/test_ops_gpu.py compares those kernels with oracle/demon_oracle.c -- float32 C in the kernels' own operation order -- through
one relative-L1 sum per tensor.  A wrong pixel column at a tile edge or a sample computed with another sample's camera moves such a
sum by far less than its bar, and a mistake the two share is invisible.  Here every op is restated in numpy float64 from its
formula (no loop of the C file; numpy.linalg.svd for the DLT) on the float32 inputs cast exactly, and returns a Ref:

    want    the float64 result; an element that must be NaN or inf holds that value and is compared as a pattern, exactly
    bound   bound_units: the same expression as the result with the absolute value of every term (a running error bound, the style of
            tier 2 in exact_ref.py).  The check on a finite element is  |got - want| <= C_op * 2^-24 * bound_units;  bound 0 = exact.
    alts    [(want, bound, mask)]: elements whose reference sits within the bound of a decision (the |flow| < 1 gate, the forward /
            backward choice of depth_to_normals) are undecided: under `mask` the other outcome is accepted as well.

C_op is 4 x the largest |oracle32 - ref64| / (2^-24 * bound_units) that the CPU float32 oracle reaches over the inputs of the GPU tests,
rounded up to a power of two (the factor 4: device sinf / cosf / sqrtf / division a few ulp from libm, other contraction choices).
tests/test_ops_ref64_cpu.py measures that ratio again and asserts 4 * ratio <= C_op, so a constant changes only with the oracle.

An element is INFORMATIVE when  C_op * 2^-24 * bound_units <= 1e-3 * max(|want|, floor),  floor = 1 / W for normalised flow and 1e-3
otherwise.  Every element is checked; the CPU suite asserts from the references alone that at least 95 % of the finite elements of
every input set are informative and at most 2 % undecided, and that every mutant below is rejected at an informative element.

The input generators are seeded and cached, so the CPU and the GPU suite see the same arrays (treat them as read-only).
"""
import functools
import itertools

import numpy as np

U24 = 2.0 ** -24
K_DEMON = np.array([0.89115971, 1.18821287, 0.5, 0.5], np.float32)

# C_op <- the measured oracle ratio it came from (largest over every input set of the GPU tests; test_ops_ref64_cpu.py re-measures)
C_DEPTH_TO_FLOW = 8       # 1.47  (4 x = 5.9)
C_FLOW_TO_DEPTH_1 = 2     # 0.45  (4 x = 1.8)   closed form
C_FLOW_TO_DEPTH_0 = 4     # 0.78  (4 x = 3.1)   DLT
C_SIG = 16                # 2.66  (4 x = 10.6)
C_WARP2D = 8              # 1.67  (4 x = 6.7)   tier 2 only; tier 1 is exact
C_NORMALS = 8             # 1.24  (4 x = 5.0)


class Ref:
    def __init__(self, want, bound, alts=()):
        self.want, self.bound, self.alts = want, bound, list(alts)

    def __iter__(self):              # want, bound = ref
        return iter((self.want, self.bound))


def _f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


# ---- the checks ------------------------------------------------------------------------------------------------------------------
def compare(got, ref, C):
    """(ok, ratio) per element: ok = within C 2^-24 bound of the reference (or, where undecided, of an alternative), non-finite
    reference values matched as patterns; ratio = |got - want| / (2^-24 bound), inf where a pattern or an exact element differs"""
    got = np.asarray(got).astype(np.float64)
    assert got.shape == ref.want.shape, (got.shape, ref.want.shape)

    def one(want, bound):
        fin = np.isfinite(want)
        with np.errstate(all="ignore"):
            err = np.abs(got - want)
            units = U24 * bound
            ratio = np.where(err == 0, 0.0, err / units)
            ok = (err <= C * units) & np.isfinite(got)
        same = (np.isnan(want) & np.isnan(got)) | (got == want)
        ratio = np.where(fin, np.where(np.isfinite(got), ratio, np.inf), np.where(same, 0.0, np.inf))
        return np.where(fin, ok, same), ratio
    ok, ratio = one(ref.want, ref.bound)
    for want, bound, mask in ref.alts:
        ok2, ratio2 = one(want, bound)
        ok = np.where(mask, ok | ok2, ok)
        ratio = np.where(mask, np.minimum(ratio, ratio2), ratio)
    return ok, ratio


def check(got, ref, C, what=""):
    """asserts every element; returns the largest ratio"""
    ok, ratio = compare(got, ref, C)
    if not ok.all():
        i = np.unravel_index(np.argmax(np.where(ok, -1.0, np.where(np.isnan(ratio), np.inf, ratio))), ok.shape)
        raise AssertionError("%s: %d of %d elements outside %g x 2^-24 x bound; worst at %s: got %r, want %r, bound units %r (%.3g x)" % (
            what, int((~ok).sum()), ok.size, C, tuple(int(v) for v in i), float(np.asarray(got)[i]), float(ref.want[i]), float(ref.bound[i]), float(ratio[i])))
    return float(ratio.max()) if ratio.size else 0.0


def check_exact(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got.astype(np.float64), want.astype(np.float64), equal_nan=True):
        bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, want %r" % (what, int(bad.sum()), bad.size, i, float(got[i]), float(want[i])))


def informative(ref, C, floor=1e-3):
    """mask of the finite elements whose bound is small against the value"""
    with np.errstate(all="ignore"):
        return np.isfinite(ref.want) & (C * U24 * ref.bound <= 1e-3 * np.maximum(np.abs(ref.want), floor))


def shares(ref, C, floor=1e-3):
    """(informative share of the finite elements, undecided share of all elements)"""
    fin = np.isfinite(ref.want)
    und = np.zeros(ref.want.shape, bool)
    for _, _, mask in ref.alts:
        und |= np.broadcast_to(mask, und.shape)
    return (float(informative(ref, C, floor).sum() / fin.sum()) if fin.any() else 1.0), float(und.mean()) if und.size else 0.0


def rejected(mutant_ref, ref, C, floor=1e-3):
    """a kernel that computed the mutant (rounded to fp32) fails the check at one or more informative elements"""
    ok, _ = compare(mutant_ref.want.astype(np.float32), ref, C)
    return bool((~ok & informative(ref, C, floor)).any())


# ---- cameras ---------------------------------------------------------------------------------------------------------------------
def rodrigues(rot):
    """[n,3] angle-axis -> [n,3,3] in float64; the identity branch (angle <= 1e-6) is decided on the float32 angle, as the op does"""
    a32 = np.asarray(rot, np.float32)
    angle32 = np.sqrt(a32[:, 0] * a32[:, 0] + a32[:, 1] * a32[:, 1] + a32[:, 2] * a32[:, 2])
    a = a32.astype(np.float64)
    R = np.tile(np.eye(3), (len(a), 1, 1))
    for i in np.nonzero(angle32 > np.float32(1e-6))[0]:
        angle = np.sqrt((a[i] * a[i]).sum())
        u = a[i] / angle
        cross = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
        R[i] = np.cos(angle) * np.eye(3) + (1 - np.cos(angle)) * np.outer(u, u) + np.sin(angle) * cross
    return R


class _Cam:
    """per-sample camera in pixels, every field shaped to broadcast against [n, h, w]"""

    def __init__(self, K, rot, tr, n, H, W, mutant=None):
        K = np.broadcast_to(_f64(K), (n, 4))
        if mutant == "k0":                       # sample 0's intrinsics for every sample
            K = np.broadcast_to(K[:1], (n, 4))
        s = (H, W) if mutant == "fx_by_h" else (W, H)   # fx scaled by H and fy by W
        self.fx, self.fy = (K[:, 0] * s[0])[:, None, None], (K[:, 1] * s[1])[:, None, None]
        self.cx, self.cy = (K[:, 2] * W)[:, None, None], (K[:, 3] * H)[:, None, None]
        half = 0.0 if mutant == "no_half" else 0.5      # pixel centre without the +0.5
        self.px = (np.arange(W) + half)[None, None, :]
        self.py = (np.arange(H) + half)[None, :, None]
        if rot is not None:
            R, t = rodrigues(rot), _f64(tr)
            if mutant == "rt0":                  # sample 0's rotation and translation for every sample
                R, t = np.broadcast_to(R[:1], R.shape), np.broadcast_to(t[:1], t.shape)
            if mutant == "r_transposed":
                R = R.transpose(0, 2, 1)
            self.R, self.t = R, t


CAMERA_MUTANTS = ("no_half", "k0", "rt0", "r_transposed", "fx_by_h")


# ---- depth_to_flow -----------------------------------------------------------------------------------------------------------------
def depth_to_flow(depth, K, rot, tr, inverse_depth=False, normalize_flow=False, gate=False, mutant=None):
    """P = z K^-1 p at the pixel centre, P2 = R P + t, flow = K P2 / P2.z - p (divided by (W, H) when normalised); NaN where the
    depth is not positive and finite after the optional 1 / d; gate: flow = |flow| < 1 ? flow : 0 (NaN -> 0).
    A2 = |R| |P| + |t|;  bound_x = fx (A2_x / |Z2|) (1 + A2_z / |Z2|) + |cx| + px,  bound_y alike."""
    d32 = np.asarray(depth, np.float32)
    n, _, H, W = d32.shape
    c = _Cam(K, rot, tr, n, H, W, mutant)
    with np.errstate(all="ignore"):
        dv = (np.float32(1) / d32 if inverse_depth else d32)[:, 0]          # validity is decided on the float32 value
        ok = (dv > 0) & np.isfinite(dv)
        d = np.where(ok, 1.0 / _f64(d32)[:, 0] if inverse_depth else _f64(d32)[:, 0], 1.0)
    P = np.stack([d * (c.px - c.cx) / c.fx, d * (c.py - c.cy) / c.fy, d], axis=1)
    P2 = np.einsum("nij,njhw->nihw", c.R, P) + c.t[:, :, None, None]
    A2 = np.einsum("nij,njhw->nihw", np.abs(c.R), np.abs(P)) + np.abs(c.t)[:, :, None, None]
    with np.errstate(all="ignore"):
        Z2 = np.abs(P2[:, 2])
        want = np.stack([c.fx * P2[:, 0] / P2[:, 2] + c.cx - c.px, c.fy * P2[:, 1] / P2[:, 2] + c.cy - c.py], axis=1)
        amp = 1 + A2[:, 2] / Z2
        bound = np.stack([c.fx * (A2[:, 0] / Z2) * amp + np.abs(c.cx) + c.px, c.fy * (A2[:, 1] / Z2) * amp + np.abs(c.cy) + c.py], axis=1)
    if normalize_flow:
        s = np.array([W, H], np.float64)[None, :, None, None]
        want, bound = want / s, bound / s
    ok2 = np.broadcast_to(ok[:, None], want.shape)
    want, bound = np.where(ok2, want, np.nan), np.where(ok2, bound, np.nan)
    if not gate:
        return Ref(want, bound)
    with np.errstate(all="ignore"):
        nrm = np.sqrt(want[:, 0] ** 2 + want[:, 1] ** 2)
        keep = nrm < 1                                                       # (NaN: False)
        und = ok & (np.abs(nrm - 1) <= C_DEPTH_TO_FLOW * U24 * (bound[:, 0] + bound[:, 1]))
    keep2, und2 = np.broadcast_to(keep[:, None], want.shape), np.broadcast_to(und[:, None], want.shape)
    return Ref(np.where(keep2, want, 0.0), np.where(keep2, bound, 0.0), [(np.where(keep2, 0.0, want), np.where(keep2, 0.0, bound), und2)])


# ---- flow_to_depth -----------------------------------------------------------------------------------------------------------------
def flow_to_depth(flow, K, rot, tr, inverse_depth=False, normalized_flow=False, method=0, mutant=None):
    """depth of the pixel along its camera-1 ray from (p1, p2 = p1 + flow), P1 = K [I | 0], P2 = K [R | t]; NaN flow gives NaN.
    method 1: least squares of the two reprojection equations, z = (ax bx + ay by) / (ax^2 + ay^2); every product and sum gets an
              absolute-value companion, bound_z = S_num / den + |z| S_den / den.
    method 0: DLT; the last right singular vector X of the 4 x 4 system A (numpy.linalg.svd), z = X[2] / X[3];
              bound_z = (||A||_F / (s3 - s4)) (1 + |z|) / |X[3]|: the null vector moved by a backward error of size u ||A||_F.
    inverse depth: 1 / z with bound_z / z^2."""
    f = _f64(flow)
    n, _, H, W = f.shape
    c = _Cam(K, rot, tr, n, H, W, mutant)
    nan = np.isnan(f).any(axis=1)
    u, v = np.where(nan, 0.0, f[:, 0]), np.where(nan, 0.0, f[:, 1])
    if normalized_flow:
        u, v = u * W, v * H
    R, aR, t, at = c.R[:, :, :, None, None], np.abs(c.R)[:, :, :, None, None], c.t[:, :, None, None], np.abs(c.t)[:, :, None, None]
    p2x, p2y = c.px + u, c.py + v
    with np.errstate(all="ignore"):
        if method == 1:
            rx, ry = (c.px - c.cx) / c.fx + 0 * u, (c.py - c.cy) / c.fy + 0 * u
            arx, ary = (c.px + np.abs(c.cx)) / c.fx + 0 * u, (c.py + np.abs(c.cy)) / c.fy + 0 * u
            q = [R[:, i, 0] * rx + R[:, i, 1] * ry + R[:, i, 2] for i in range(3)]
            aq = [aR[:, i, 0] * arx + aR[:, i, 1] * ary + aR[:, i, 2] for i in range(3)]
            pcx, pcy = p2x - c.cx, p2y - c.cy
            apcx, apcy = c.px + np.abs(u) + np.abs(c.cx), c.py + np.abs(v) + np.abs(c.cy)
            ax, bx = c.fx * q[0] - pcx * q[2], pcx * t[:, 2] - c.fx * t[:, 0]
            ay, by = c.fy * q[1] - pcy * q[2], pcy * t[:, 2] - c.fy * t[:, 1]
            aax, abx = c.fx * aq[0] + apcx * aq[2], apcx * at[:, 2] + c.fx * at[:, 0]
            aay, aby = c.fy * aq[1] + apcy * aq[2], apcy * at[:, 2] + c.fy * at[:, 1]
            den = ax * ax + ay * ay
            z = (ax * bx + ay * by) / den
            bound = (aax * abx + aay * aby) / den + np.abs(z) * (aax * aax + aay * aay) / den
        else:
            Rm, tm = c.R, c.t
            f4 = np.stack([c.fx[:, 0, 0], c.fy[:, 0, 0], c.cx[:, 0, 0], c.cy[:, 0, 0]], axis=1)
            P2 = np.empty((n, 3, 4))
            P2[:, 0, :3] = f4[:, 0:1] * Rm[:, 0] + f4[:, 2:3] * Rm[:, 2]
            P2[:, 1, :3] = f4[:, 1:2] * Rm[:, 1] + f4[:, 3:4] * Rm[:, 2]
            P2[:, 2, :3] = Rm[:, 2]
            P2[:, 0, 3] = f4[:, 0] * tm[:, 0] + f4[:, 2] * tm[:, 2]
            P2[:, 1, 3] = f4[:, 1] * tm[:, 1] + f4[:, 3] * tm[:, 2]
            P2[:, 2, 3] = tm[:, 2]
            A = np.zeros((n, H, W, 4, 4))
            A[..., 0, 0], A[..., 0, 2] = -c.fx, c.px - c.cx
            A[..., 1, 1], A[..., 1, 2] = -c.fy, c.py - c.cy
            A[..., 2, :] = p2x[..., None] * P2[:, None, None, 2, :] - P2[:, None, None, 0, :]
            A[..., 3, :] = p2y[..., None] * P2[:, None, None, 2, :] - P2[:, None, None, 1, :]
            _, s, Vh = np.linalg.svd(A)
            X = Vh[..., 3, :]
            z = X[..., 2] / X[..., 3]
            bound = np.sqrt((A * A).sum(axis=(-1, -2))) / (s[..., 2] - s[..., 3]) * (1 + np.abs(z)) / np.abs(X[..., 3])
        if inverse_depth:
            z, bound = 1.0 / z, bound / (z * z)
    return Ref(np.where(nan, np.nan, z)[:, None], np.where(nan, np.nan, bound)[:, None])


# ---- warp2d ------------------------------------------------------------------------------------------------------------------------
def warp2d(img, disp, normalized=False, border_mode="clamp", border_value=0.0, mutant=None):
    """out(x, y) = bilinear in(x + dx, y + dy) (displacement times (W, H) when normalised); a tap outside the image is the border value
    ('value') or the clamped pixel ('clamp'); a non-finite or huge (>= 1e9) position gives the border value / NaN.
    bound = sum_k w_k |v_k| + (|sx| + |sy|) (max_k v_k - min_k v_k): the weights' rounding, and the position's rounding times the
    largest slope (bilinear interpolation is continuous across a floor flip, so no element is excluded)."""
    im, d = _f64(img), _f64(disp)
    n, C, H, W = im.shape
    bv = float(np.float32(border_value))
    dx, dy = (d[:, 0] * W, d[:, 1] * H) if normalized else (d[:, 0], d[:, 1])
    with np.errstate(all="ignore"):
        sx, sy = np.arange(W)[None, None, :] + dx, np.arange(H)[None, :, None] + dy
        finite = np.isfinite(sx) & np.isfinite(sy) & (np.abs(sx) < 1e9) & (np.abs(sy) < 1e9)
    sx, sy = np.where(finite, sx, 0.0), np.where(finite, sy, 0.0)
    fl = np.trunc if mutant == "trunc" else np.floor              # truncation in place of floor
    x0, y0 = fl(sx), fl(sy)
    a, b = sx - x0, sy - y0
    value = border_mode == "value" and mutant != "clamp_taps"     # 'value' mode taps clamped into the image
    ni = np.arange(n)[:, None, None]
    want, mag, vs = 0.0, 0.0, []
    for ky, kx in itertools.product((0, 1), (0, 1)):
        xi, yi = x0 + kx, y0 + ky
        inside = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        vk = im[ni, :, np.clip(yi, 0, H - 1).astype(int), np.clip(xi, 0, W - 1).astype(int)].transpose(0, 3, 1, 2)
        if value:
            vk = np.where(inside[:, None], vk, bv)
        wk = ((a if kx else 1 - a) * (b if ky else 1 - b))[:, None]
        want, mag = want + wk * vk, mag + np.abs(wk) * np.abs(vk)
        vs.append(vk)
    bound = mag + (np.abs(sx) + np.abs(sy))[:, None] * (np.maximum.reduce(vs) - np.minimum.reduce(vs))
    fin = np.broadcast_to(finite[:, None], want.shape)
    return Ref(np.where(fin, want, bv if border_mode == "value" else np.nan), np.where(fin, bound, 0.0))


# ---- scale_invariant_gradient -----------------------------------------------------------------------------------------------------
def scale_invariant_gradient(x, deltas, weights, eps, mutant=None):
    """[N,C,H,W] -> [N*C,2,H,W]: gx = sum_k w_k (u(x + d_k, y) - u) / (|u(x + d_k, y)| + |u| + eps) over the neighbours that exist (a
    missing one contributes nothing, so with none the result is exactly 0), gy alike.  bound = sum_k |w_k| |un - u| / (|un| + |u| + eps)."""
    u = _f64(x)
    u = u.reshape((-1,) + u.shape[2:])
    _, H, W = u.shape
    eps = float(np.float32(eps))
    xs, ys = np.arange(W), np.arange(H)
    g, gb = np.zeros((2,) + u.shape), np.zeros((2,) + u.shape)
    au = np.abs(u)
    with np.errstate(all="ignore"):
        for dlt, wk in zip(np.asarray(deltas, np.int64), _f64(weights)):
            for axis in (0, 1):
                idx = (xs if axis == 0 else ys) + dlt
                valid = (idx >= 0) & (idx < (W if axis == 0 else H))
                src = idx - 1 if (mutant == "x_minus_1" and axis == 0) else idx          # neighbour taken from x + d - 1
                src = np.clip(src, 0, (W if axis == 0 else H) - 1)
                un = u[:, :, src] if axis == 0 else u[:, src, :]
                if mutant == "tile_x" and axis == 0:                                       # neighbours in another 64-column tile read as 0
                    un = np.where((idx // 64 != xs // 64)[None, None, :], 0.0, un)
                if mutant == "tile_y":                                                     # rows beyond the first 4-row tile read as 0
                    rows = np.broadcast_to(ys[None, :, None] if axis == 0 else idx[None, :, None], un.shape)
                    un = np.where(rows >= 4, 0.0, un)
                den = np.abs(un) + au + eps
                v = valid[None, None, :] if axis == 0 else valid[None, :, None]
                g[axis] += np.where(v, wk * (un - u) / den, 0.0)
                gb[axis] += np.where(v, np.abs(wk) * np.abs(un - u) / den, 0.0)
    want, bound = g.transpose(1, 0, 2, 3), gb.transpose(1, 0, 2, 3)
    return Ref(want, np.where(np.isfinite(want), bound, np.nan))


# ---- depth_to_normals ---------------------------------------------------------------------------------------------------------------
def depth_to_normals(depth, K, inverse_depth=False, mutant=None):
    """P(x, y) = z ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1); per axis the one-sided difference with the smaller |dz| (backward
    when |P0z - P1z| < |P2z - P0z|); n = normalize(diff_y x diff_x); NaN at the border and where the pixel's own or a 4-neighbour's depth
    is not positive and finite.  A difference P_a - P_b has the running bound |P_a| + |P_b|; a product of two of them the bound of each
    times the magnitude of the other plus its own rounding; A_c sums these over the cross product's terms.  Through n = c / |c|:
        bound_i = (A_c_i + |n_i| sum_j |n_j| A_c_j) / |c|
    (the second term is the norm's own error: for the dominant component this is the plain 2 A_c_i / |c|, for a small component next
    to a large one -- n_y on a wide, low map -- the doubled form misses what the large components' errors do to the norm; with it the
    oracle's ratio was 3.5 and one input in ten uninformative)."""
    d32 = np.asarray(depth, np.float32)
    n, _, H, W = d32.shape
    c = _Cam(K, None, None, n, H, W, mutant)
    with np.errstate(all="ignore"):
        dv = (np.float32(1) / d32 if inverse_depth else d32)[:, 0]
        good = (dv > 0) & np.isfinite(dv)
        z = np.where(good, 1.0 / _f64(d32)[:, 0] if inverse_depth else _f64(d32)[:, 0], 1.0)
    P = np.stack([z * (c.px - c.cx) / c.fx, z * (c.py - c.cy) / c.fy, z], axis=1)
    AP = np.abs(P)
    want, bound = np.full((n, 3, H, W), np.nan), np.full((n, 3, H, W), np.nan)
    if H < 3 or W < 3:
        return Ref(want, bound)
    ctr = (slice(None), slice(None), slice(1, -1), slice(1, -1))
    lf, rt = (slice(None), slice(None), slice(1, -1), slice(0, -2)), (slice(None), slice(None), slice(1, -1), slice(2, None))
    up, dn = (slice(None), slice(None), slice(0, -2), slice(1, -1)), (slice(None), slice(None), slice(2, None), slice(1, -1))
    g = good[:, None]
    ok = (g[ctr] & g[lf] & g[rt] & g[up] & g[dn])[:, 0]
    zb, zf = np.abs(P[ctr][:, 2] - P[lf][:, 2]), np.abs(P[rt][:, 2] - P[ctr][:, 2])
    yb, yf = np.abs(P[ctr][:, 2] - P[up][:, 2]), np.abs(P[dn][:, 2] - P[ctr][:, 2])
    bx, by = zb < zf, yb < yf
    tie = C_NORMALS * U24
    und_x = np.abs(zb - zf) <= tie * (2 * AP[ctr][:, 2] + AP[lf][:, 2] + AP[rt][:, 2])
    und_y = np.abs(yb - yf) <= tie * (2 * AP[ctr][:, 2] + AP[up][:, 2] + AP[dn][:, 2])

    def normals(bx, by):
        dx = np.where(bx[:, None], P[ctr] - P[lf], P[rt] - P[ctr])
        dy = np.where(by[:, None], P[ctr] - P[up], P[dn] - P[ctr])
        adx = np.where(bx[:, None], AP[ctr] + AP[lf], AP[rt] + AP[ctr])
        ady = np.where(by[:, None], AP[ctr] + AP[up], AP[dn] + AP[ctr])
        cr = np.stack([dy[:, 1] * dx[:, 2] - dy[:, 2] * dx[:, 1], dy[:, 2] * dx[:, 0] - dy[:, 0] * dx[:, 2], dy[:, 0] * dx[:, 1] - dy[:, 1] * dx[:, 0]], axis=1)
        mx, my = np.abs(dx), np.abs(dy)

        def run(i, j):   # running bound of dy_i dx_j: each factor's bound times the other's magnitude, and the product's own rounding
            return ady[:, i] * mx[:, j] + my[:, i] * adx[:, j] + my[:, i] * mx[:, j]
        acr = np.stack([run(1, 2) + run(2, 1), run(2, 0) + run(0, 2), run(0, 1) + run(1, 0)], axis=1)
        with np.errstate(all="ignore"):
            nrm = np.sqrt((cr * cr).sum(axis=1, keepdims=True))
            w = cr / nrm
            b = (acr + np.abs(w) * (np.abs(w) * acr).sum(axis=1, keepdims=True)) / nrm
        full_w, full_b = np.full((n, 3, H, W), np.nan), np.full((n, 3, H, W), np.nan)
        full_w[ctr], full_b[ctr] = np.where(ok[:, None], w, np.nan), np.where(ok[:, None], b, np.nan)
        return full_w, full_b
    want, bound = normals(bx, by)
    alts = []
    for fx_, fy_ in ((True, False), (False, True), (True, True)):
        mask = ok & (und_x if fx_ else True) & (und_y if fy_ else True)
        if mask.any():
            w, b = normals(bx ^ fx_, by ^ fy_)
            full = np.zeros((n, 3, H, W), bool)
            full[ctr] = mask[:, None]
            alts.append((w, b, full))
    return Ref(want, bound, alts)


# ---- exact ops ----------------------------------------------------------------------------------------------------------------------
def median3x3_downsample(x, mutant=None):
    """median of the 3 x 3 window centred at (2y, 2x), indices clamped; every NaN sorts behind +inf (numpy's sort order)"""
    x = np.asarray(x, np.float32)
    H, W = x.shape[2:]
    o = 1 if mutant == "odd_centre" else 0                                   # the median taken at (2y + 1, 2x + 1)
    ys, xs = 2 * np.arange((H + 1) // 2) + o, 2 * np.arange((W + 1) // 2) + o
    win = [x[:, :, np.clip(ys + dy, 0, H - 1)][:, :, :, np.clip(xs + dx, 0, W - 1)] for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    return np.sort(np.stack(win, axis=-1), axis=-1)[..., 4]


def leaky_relu(x, leak):
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        return np.where(x >= 0, x, (x.astype(np.float64) * float(np.float32(leak))).astype(np.float32))   # one fp32 rounding of the exact product


def replace_nonfinite(x, value):
    x = np.asarray(x, np.float32)
    return np.where(np.isfinite(x), x, np.float32(value))


def pointwise_l2_loss(inp, gt, eps):
    from oracle import ops_ref
    return ops_ref.pointwise_l2_loss(inp, gt, eps)


# ---- input generators (seeded, cached: both suites see the same arrays) ---------------------------------------------------------------
GEOM_SHAPES = ((3, 5, 7), (2, 16, 16), (2, 1, 257), (3, 9, 130))       # depth_to_flow, flow_to_depth method 1
DLT_SHAPES = ((3, 5, 7), (2, 16, 16), (2, 3, 86), (3, 9, 130))         # method 0 (no H = 1: its conditioning bound says nothing there)
BOOLS = (False, True)


CAMERA_SEED = 101      # (the first seed at which every input set of the geometry ops meets the 95 % condition)


@functools.lru_cache(maxsize=None)
def cameras(n, seed=None):
    """per-sample K = K_DEMON (1 + 0.2 rand), rotation and unit translation; sample 0's rotation is exactly zero (identity branch),
    sample 1's has |aa| ~ 2e-6 (just above it), so only a third sample turns by a general ~0.1 rad"""
    rng = np.random.default_rng((CAMERA_SEED if seed is None else seed) + n)
    K = (K_DEMON[None] * (1 + 0.2 * rng.random((n, 4)))).astype(np.float32)
    rot = (rng.standard_normal((n, 3)) * 0.1).astype(np.float32)
    tr = rng.standard_normal((n, 3))
    tr = (tr / np.linalg.norm(tr, axis=1, keepdims=True)).astype(np.float32)
    rot[0] = 0
    if n > 1:
        axis = rng.standard_normal(3)
        rot[1] = (2e-6 * axis / np.linalg.norm(axis)).astype(np.float32)
    return K, rot, tr


@functools.lru_cache(maxsize=None)
def depth_input(shape, seed=101):
    """(inverse) depth in 0.2 .. 1.2 with zeros, negatives, NaN and inf sprinkled in"""
    n, h, w = shape
    rng = np.random.default_rng(seed + h * w)
    d = (0.2 + rng.random((n, 1, h, w))).astype(np.float32)
    flat = d.reshape(-1)
    flat[3::17], flat[5::29], flat[7::31], flat[11::37] = 0, -1, np.nan, np.inf
    return d


@functools.lru_cache(maxsize=None)
def flow_input(shape, normalized, seed=102):
    """the oracle's depth_to_flow of a random inverse depth plus 0.002 (of the image size) noise, like a prediction; a few NaN pixels in
    every sample, and a few zero-flow pixels in the sample with a general rotation (with no rotation a zero flow makes the closed
    form 0 / 0: noise, not a result)"""
    from oracle import ops_ref
    n, h, w = shape
    rng = np.random.default_rng(seed + h * w)
    K, rot, tr = cameras(n)
    inv_depth = (0.2 + rng.random((n, 1, h, w))).astype(np.float32)
    flow = ops_ref.depth_to_flow(inv_depth, K, rot, tr, True, normalized)
    noise = rng.standard_normal(flow.shape) * 0.002
    if not normalized:
        noise *= np.array([w, h])[None, :, None, None]
    flow = (flow + noise).astype(np.float32)
    hw = h * w
    f = flow.reshape(n, 2, hw)
    for s in range(n):
        f[s, :, (5 + 3 * s) % hw] = np.nan
        f[s, 1, (hw - 2 - s) % hw] = np.nan
    if n > 2:
        f[2, :, 1 % hw] = 0
        f[2, :, hw // 2] = 0
        f[2, :, hw - 1] = 0
    return flow


WARP_EXACT_CASES = (((1, 1, 5, 7), False), ((2, 3, 16, 64), False), ((2, 5, 9, 130), False), ((2, 3, 16, 64), True))   # (shape, normalized)
WARP_BOUND_SHAPE = (2, 5, 9, 130)
WARP_BOUND_SIGMA = (0.03, 0.15)      # of the width / height: ~4 and ~1.4 pixels, so that x + dx rarely cancels a large x to a small sx
WARP_BORDERS = (("value", 7.0), ("clamp", 7.0), ("value", -2.0))


@functools.lru_cache(maxsize=None)
def warp_exact_input(shape, normalized, seed=103):
    """tier 1: non-zero integer image values in -8 .. 8 and sampling positions on the 1/8 grid, so that every weight is a multiple of
    1/64 and every product and sum is exact in fp32.  Planted positions: sx in (-1, 0), exactly -1, in [W - 1, W), exactly W, the same
    in y, both coordinates out at once, exactly zero displacement, NaN, +inf, -inf and +-2e9."""
    n, c, h, w = shape
    rng = np.random.default_rng(seed + h * w)
    img = (rng.integers(1, 9, size=shape) * (2 * rng.integers(0, 2, size=shape) - 1)).astype(np.float32)
    disp = rng.integers(-24, 25, size=(n, 2, h, w)).astype(np.float64) / 8           # pixels
    tx = [-0.5, -0.125, -0.875, -1.0, w - 1.0, w - 0.625, w - 0.125, float(w), w + 0.5, -1.25]
    ty = [-0.5, -0.125, -0.875, -1.0, h - 1.0, h - 0.625, h - 0.125, float(h), h + 0.5, -1.25]
    plant = [(t, None) for t in tx] + [(None, t) for t in ty] + [(-0.5, -0.5), (w - 0.5, h - 0.5), (-0.25, h - 0.75), (float(w), -1.0), (-3.0, h + 2.0)]
    special = [(0.0, 0.0), (np.nan, 0.0), (0.0, np.nan), (np.inf, 0.0), (0.0, -np.inf), (-np.inf, np.inf), (2e9, 0.0), (0.0, -2e9), (-2e9, 2e9)]
    hw = h * w
    step = max(1, hw // (len(plant) + len(special) + 1))
    d = disp.reshape(n, 2, hw)
    for s in range(n):
        for k, (sx, sy) in enumerate(plant):
            i = (k * step + s) % hw
            y, x = divmod(i, w)
            if sx is not None:
                d[s, 0, i] = sx - x
            if sy is not None:
                d[s, 1, i] = sy - y
        for k, (dx, dy) in enumerate(special):
            i = ((len(plant) + k) * step + s) % hw
            d[s, 0, i], d[s, 1, i] = dx, dy
    if normalized:
        assert w & (w - 1) == 0 and h & (h - 1) == 0
        with np.errstate(all="ignore"):
            disp = disp / np.array([w, h], np.float64)[None, :, None, None]
        big = np.isfinite(disp) & (np.abs(disp) > 1e6)
        disp[big] = np.sign(disp[big]) * 2e9                                             # (the huge displacements stay +-2e9)
    out = disp.astype(np.float32)
    fin = np.isfinite(out) & (np.abs(out) < 1e9)
    assert np.array_equal(out[fin].astype(np.float64), disp[fin])                       # every planted displacement is an fp32 value
    return img, out


@functools.lru_cache(maxsize=None)
def warp_bound_input(seed=104):
    """tier 2: ragged shape, normalised Gaussian displacements (many taps outside), NaN / inf / zero displacements planted"""
    n, c, h, w = WARP_BOUND_SHAPE
    rng = np.random.default_rng(seed)
    img = (0.5 + rng.random(WARP_BOUND_SHAPE)).astype(np.float32)
    disp = (rng.standard_normal((n, 2, h, w)) * np.array(WARP_BOUND_SIGMA)[None, :, None, None]).astype(np.float32)
    disp[0, 0, 0, 0] = np.nan
    disp[0, 1, h - 1, w - 1] = np.inf
    disp[1, 0, 3, 64] = -np.inf
    disp[:, :, h // 2, w // 2] = 0.0
    return img, disp


SIG_SHAPES = ((1, 2, 5, 65), (2, 1, 9, 130), (1, 1, 4, 63), (1, 3, 1, 1), (1, 1, 3, 64))
SIG_DELTAS = ((1,), (-1,), (16,), (17,), (32,), (1, 2, 4, 8, 16), (1, -3, 17), (1, -2, 3, -5, 8, -13, 21, 200))


def sig_weights(k):
    """neither all equal nor powers of two"""
    return (0.3 + 0.17 * np.arange(k)).astype(np.float32) * np.where(np.arange(k) % 3 == 2, -1, 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def sig_input(shape, zeros=False, seed=105):
    """non-zero values (a zero read in place of a neighbour shows); zeros=True plants runs of equal zeros for the eps = 0 case (0 / 0)"""
    n, c, h, w = shape
    rng = np.random.default_rng(seed + h * w)
    u = ((0.5 + rng.random(shape)) * (2 * rng.integers(0, 2, size=shape) - 1)).astype(np.float32)
    if zeros:
        u[..., 0, : min(w, 3)] = 0
        u[..., h - 1, w // 2: w // 2 + 2] = 0
        u[..., : min(h, 2), w - 1] = 0
    return u


NORMALS_SHAPES = ((3, 7, 9), (1, 3, 3), (1, 2, 5), (2, 6, 130))


@functools.lru_cache(maxsize=None)
def normals_input(shape, seed=107):
    """depths in 1 .. 2 with invalid ones sprinkled in, per-sample K (seed: the first at which every shape meets the 95 % condition)"""
    n, h, w = shape
    rng = np.random.default_rng(seed + h * w)
    z = (1.0 + rng.random((n, 1, h, w))).astype(np.float32)
    flat = z.reshape(-1)
    flat[13::23], flat[15::41], flat[17::53], flat[19::59] = 0, np.nan, -1, np.inf
    K = (K_DEMON[None] * (1 + 0.2 * rng.random((n, 4)))).astype(np.float32)
    return z, K


MEDIAN_SHAPES = ((1, 2, 9, 131), (1, 1, 8, 130), (1, 1, 1, 1), (1, 1, 2, 1), (2, 1, 1, 5))


@functools.lru_cache(maxsize=None)
def median_input(shape, sprinkle, seed=107):
    rng = np.random.default_rng(seed + shape[2] * shape[3])
    x = rng.standard_normal(shape).astype(np.float32)
    if sprinkle:
        flat = x.reshape(-1)
        flat[::7], flat[2::11], flat[4::13], flat[1::17], flat[3::5] = np.nan, np.inf, -np.inf, -0.0, np.nan
    return x


L2_SHAPES = ((1, 1, 3, 5), (1, 10, 16, 16), (1, 2, 1, 257))


@functools.lru_cache(maxsize=None)
def l2_input(shape, seed=108):
    rng = np.random.default_rng(seed + shape[2] * shape[3])
    inp, gt = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    gt.reshape(-1)[1::13] = np.nan
    inp.reshape(-1)[2::101] = np.inf
    return inp, gt
