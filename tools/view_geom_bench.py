"""What the view tools cost on the GPU (demon_amd/csrc/viewgeom.hip; demon_amd/view_tools.py) and on the host they replace.

  python tools/view_geom_bench.py [--out profiles/view_geometry.json]

At the sun3d depth size of 640x480, a set of 24 views of one plane with noise and invalid pixels:
(a) kernel: the two launches (view_pairs_kernel + view_counts_kernel) by hip events, median of 20 after 5 warm-up rounds
    (demon_bench_view_pairs), for 1, 32 and 512 ordered pairs, counts only and in full form (mask + ratios stored);
(b) host to host: view_pair_counts (packing the per-pair records, uploading the 24 maps, both launches, the counts back), best of 5;
(c) the same work on this host, one core, per pair: the float32 numpy restatement (tests/view_geom_ref.py) and, where oracle/_ref
    carries it, the reference's compiled loop (compute_depth_ratios, which is what check_depth_consistency runs per ordered pair)."""
import argparse
import glob
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from demon_amd import DemonContext, view_tools  # noqa: E402

H, W, V = 480, 640, 24


def make_views(seed=1):
    rng = np.random.default_rng(seed)
    K = np.array([[0.89115971 * W, 0, 0.5 * W], [0, 1.18821287 * H, 0.5 * H], [0, 0, 1]])
    normal = np.array([0.15, -0.1, 1.0]) / np.linalg.norm([0.15, -0.1, 1.0])
    px, py = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    rays = np.stack([(px - K[0, 2]) / K[0, 0], (py - K[1, 2]) / K[1, 1], np.ones_like(px)], -1)
    views = []
    for i in range(V):
        axis = rng.standard_normal(3)
        axis /= np.linalg.norm(axis)
        a = np.radians(rng.uniform(0, 6))
        Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx.dot(Kx)
        t = rng.uniform(-0.15, 0.15, 3)
        nr = R.dot(normal)
        d = ((2.5 + nr.dot(t)) / rays.dot(nr) * rng.uniform(0.97, 1.03, (H, W))).astype(np.float32)
        d[rng.random((H, W)) < 0.08] = 0.0
        views.append(view_tools.View(R=R, t=t, K=K, image=None, depth=d, depth_metric="camera_z"))
    return views


def ordered_pairs(n):
    allp = [(i, j) for i in range(V) for j in range(V) if i != j]
    return np.array(allp[:n], np.int32)


def kernel_times(ctx, views):
    out = {}
    lo, hi = view_tools.ratio_thresholds(0.9)
    for n in (1, 32, 512):
        depth, pairs, K1, R1, t1, P2 = view_tools._pair_arrays(views, ordered_pairs(n))
        for form, full in (("counts_only", False), ("full", True)):
            counts, _, _, ms = ctx.view_pairs(depth, pairs, K1, R1, t1, P2, ratio_lo=lo, ratio_hi=hi, want_mask=full, want_ratios=full, bench=(5, 20))
            km = statistics.median(ms)
            px = n * H * W
            moved = px * (4 + 4 + (5 if full else 0))     # depth 1 read, one gathered depth per pixel at most, mask + ratio written
            out["%s_n%d" % (form, n)] = {"pairs": n, "kernel_ms_median": round(km, 5), "kernel_ms_min": round(min(ms), 5), "kernel_ms_max": round(max(ms), 5),
                                         "launches": 2, "us_per_pair": round(1e3 * km / n, 3), "bytes_moved_at_most": moved,
                                         "gb_per_s_at_most": round(moved / km / 1e6, 1), "finite_ratio_fraction": round(float(counts[:, 2].sum()) / px, 4)}
            print(form, n, json.dumps(out["%s_n%d" % (form, n)]), flush=True)
    return out


def host_to_host(views):
    out = {}
    for n in (1, 32, 512):
        pairs = ordered_pairs(n)
        best = None
        for _ in range(5):
            t0 = time.perf_counter()
            view_tools.view_pair_counts(views, pairs)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        out["n%d" % n] = {"pairs": n, "ms": round(1e3 * best, 3), "ms_per_pair": round(1e3 * best / n, 4)}
    out["what"] = "view_pair_counts on 24 views of 640x480: records packed, 24 maps (29.5 MB) uploaded, two launches, counts back; best of 5"
    return out


def cpu_cost(views):
    import view_geom_ref as ref
    v1, v2 = views[0], views[1]
    P2 = view_tools.projection_matrix(v2)
    out = {}
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        ref.view_geometry(v1.depth, v2.depth, v1.K, v1.R, v1.t, P2, lo=0.9, hi=1 / 0.9)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    out["numpy_restatement_ms_per_pair"] = round(1e3 * best, 2)
    so = glob.glob(os.path.join(ROOT, "oracle", "_ref", "view_tools_cython*.so"))
    if so:
        spec = importlib.util.spec_from_file_location("view_tools_cython", so[0])
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        pad = np.full((H + 2, W), np.nan, np.float32)
        pad[:H] = v2.depth
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            mod.compute_depth_ratios(v1, v2._replace(depth=pad[:H]))
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        out["compiled_reference_ms_per_pair"] = round(1e3 * best, 2)
    else:
        out["compiled_reference_ms_per_pair"] = None
    out["what"] = "one ordered pair of 640x480 maps on this host, one core, best of 3"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_geometry.json"))
    args = ap.parse_args()
    views = make_views()
    rec = {"what": "view tools on the GPU (tools/view_geom_bench.py): measured on one MI355X, 24 views of 640x480"}
    ctx = DemonContext.ops_only(0)
    try:
        rec["a_kernel"] = kernel_times(ctx, views)
    finally:
        ctx.close()
    try:
        rec["b_host_to_host"] = host_to_host(views)
    finally:
        view_tools.release()
    print(json.dumps(rec["b_host_to_host"]), flush=True)
    rec["c_host_cost"] = cpu_cost(views)
    print(json.dumps(rec["c_host_cost"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
