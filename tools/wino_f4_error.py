#!/usr/bin/env python3
"""fp32 error of the integer-scaled four-outputs-per-window tables (tools/gen_wino1d.py) against a float64 direct sum, in numpy (no GPU):
t = BT d and U = G g in fp32, the reduction over K channels in fp32, the output transform in fp32 with the coefficients rounded to fp32 --
the arithmetic of conv_wino4.hip.  Relative L1 over random normal data, beside the direct fp32 sum's.

  python tools/wino_f4_error.py [--k 32 64] [--windows 4096]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_wino1d as gen  # noqa: E402

FORMS = [("F43", 3, 1), ("F4K5S2", 5, 2), ("F4K7S2", 7, 2), ("F4K9S2", 9, 2)]


def measure(taps, stride, K, windows, seed=0):
    """(relative L1 of the minimal-filtering form, of the direct fp32 sum)"""
    AT, G, BT, win = gen.kind_matrices4(taps, stride)
    AT, G = gen.normalise(AT, G)
    f32 = np.float32
    A, Gm, B = (np.array([[float(v) for v in row] for row in M], dtype=f32) for M in (AT, G, BT))
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((windows, K, win)).astype(f32)
    g = (rng.standard_normal((K, taps)) / np.sqrt(taps * K)).astype(f32)
    idx = stride * np.arange(4)[:, None] + np.arange(taps)[None, :]
    ref = np.einsum("wkot,kt->wo", d.astype(np.float64)[:, :, idx], g.astype(np.float64))
    direct = np.zeros((windows, 4), f32)
    for k in range(K):          # sequential fp32 accumulation, channel by channel and tap by tap
        for t in range(taps):
            direct += d[:, k, idx[:, t]] * g[k, t]
    t32 = np.zeros((windows, K, len(Gm)), f32)
    for n in range(win):
        t32 += d[:, :, n:n + 1] * B[None, None, :, n]
    U = np.zeros((K, len(Gm)), f32)
    for t in range(taps):
        U += g[:, t:t + 1] * Gm[None, :, t]
    M = np.zeros((windows, len(Gm)), f32)
    for k in range(K):
        M += t32[:, k] * U[k]
    o = np.zeros((windows, 4), f32)
    for e in range(len(Gm)):
        o += M[:, e:e + 1] * A[None, :, e]

    def rel(x):
        return float(np.abs(x.astype(np.float64) - ref).sum() / np.abs(ref).sum())
    return rel(o), rel(direct)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--windows", type=int, default=4096)
    args = ap.parse_args()
    for name, taps, stride in FORMS:
        for K in args.k:
            w, dsum = measure(taps, stride, K, args.windows)
            print("%-8s %d taps stride %d  K = %3d   minimal filtering %.2e   direct fp32 sum %.2e" % (name, taps, stride, K, w, dsum))


if __name__ == "__main__":
    main()
