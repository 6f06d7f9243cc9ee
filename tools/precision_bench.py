"""fp32 against bf16 (option precision, conv_bf16.hip) on the flagship workload: full passes (bootstrap + 3 iterations + refine) with
synthetic weights and inputs.

  python tools/precision_bench.py [--out profiles/bf16_vs_fp32.json] [--steps K]

Records pairs/s at 256 x 192, batch 1 / 8 / 32, one lane (DemonContext.time_full, hipGraph replays) and four lanes
(LaneGroup.run_resident, round robin, no calibration), and at 640 x 480, batch 64, one lane; then a per-layer table of
profile_full (batch 32, 256 x 192) in both modes.  bench.py stays the yardstick of the fp32 headline; this is the side-by-side."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

import demon_amd.lanes  # noqa: E402  (exports GPU_MAX_HW_QUEUES before the first HIP call)
from demon_amd import DemonContext, weights  # noqa: E402
from demon_amd.lanes import LaneGroup  # noqa: E402

ITER = 3


def one_lane(w, n, H, W, precision, steps):
    ctx = DemonContext(0, n, H, W, precision=precision)
    try:
        ctx.set_weights(w)
        ctx.load_tuned_plan(n)
        ctx.time_full(n, ITER, 2)   # capture + warm-up
        ms = min(ctx.time_full(n, ITER, steps) for _ in range(3))
        return {"pairs_per_s": round(n * steps / (ms / 1000.0), 1), "ms_per_pass": round(ms / steps, 4)}
    finally:
        ctx.close()


def four_lanes(w, n, precision, steps):
    g = LaneGroup(w, lanes=4, batch=n, precision=precision)
    try:
        g.run_resident(n, 4 * 2, ITER)
        g.ctxs[0].synchronize()
        for c in g.ctxs:
            c.synchronize()
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            g.run_resident(n, steps * 4, ITER)
            for c in g.ctxs:
                c.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return {"pairs_per_s": round(n * steps * 4 / best, 1), "lanes": 4}
    finally:
        g.close()


def layer_table(w, n, precision):
    ctx = DemonContext(0, n, 192, 256, precision=precision)
    try:
        ctx.set_weights(w)
        ctx.load_tuned_plan(n)
        rec = ctx.profile_full(n, ITER, 3)
    finally:
        ctx.close()
    return [{"name": r["name"], "kernel": r["kernel"], "ms": round(r["ms"] + r["reduce_ms"], 5), "gflop": round(r["flops"] / 1e9, 4)} for r in rec]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_vs_fp32.json"))
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    w = weights.synthetic_weights(seed=1)
    rec = {"what": "pairs/s of full passes (bootstrap + %d iterations + refine), synthetic weights and inputs; fp32 = option precision 0, "
                   "bf16 = option precision 1" % ITER, "runs": []}
    for (H, W, n, lanes) in ((192, 256, 1, 1), (192, 256, 8, 1), (192, 256, 32, 1), (192, 256, 1, 4), (192, 256, 8, 4), (192, 256, 32, 4),
                             (480, 640, 64, 1)):
        wt = w if (H, W) == (192, 256) else weights.synthetic_weights(seed=1, height=H, width=W)
        row = {"size": "%dx%d" % (W, H), "batch": n, "lanes": lanes}
        for p in ("fp32", "bf16"):
            steps = max(2, args.steps // (4 if n >= 32 else 1))
            row[p] = one_lane(wt, n, H, W, p, steps) if lanes == 1 else four_lanes(wt, n, p, steps)
        row["bf16_speedup"] = round(row["bf16"]["pairs_per_s"] / row["fp32"]["pairs_per_s"], 3)
        print(json.dumps(row), flush=True)
        rec["runs"].append(row)
    t32, t16 = layer_table(w, 32, "fp32"), layer_table(w, 32, "bf16")
    by16 = {}
    for r in t16:
        by16.setdefault(r["name"], []).append(r)
    layers = []
    for r in t32:
        o = by16.get(r["name"])
        o = o.pop(0) if o else None
        layers.append({"name": r["name"], "fp32_kernel": r["kernel"], "fp32_ms": r["ms"], "bf16_kernel": o["kernel"] if o else None,
                       "bf16_ms": o["ms"] if o else None, "gflop": r["gflop"]})
    extra16 = [r for rs in by16.values() for r in rs]   # steps only the bf16 pass has (pairs split into their two layers)
    rec["layers_batch32"] = {"fp32_total_ms": round(sum(r["ms"] for r in t32), 4), "bf16_total_ms": round(sum(r["ms"] for r in t16), 4),
                             "rows": layers, "bf16_only_rows": extra16}
    fam = {}
    for r in t32:
        f = fam.setdefault(r["kernel"].split("<")[0], [0.0, 0.0])
        f[0] += r["ms"]
    for r in t16:
        f = fam.setdefault(r["kernel"].split("<")[0], [0.0, 0.0])
        f[1] += r["ms"]
    rec["layers_batch32"]["by_family_ms"] = {k: {"fp32": round(v[0], 4), "bf16": round(v[1], 4)} for k, v in sorted(fam.items(), key=lambda kv: -kv[1][0])}
    print(json.dumps(rec["layers_batch32"]["by_family_ms"]), flush=True)
    print("per-layer totals (batch 32, ms): fp32 %.3f, bf16 %.3f" % (rec["layers_batch32"]["fp32_total_ms"], rec["layers_batch32"]["bf16_total_ms"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
