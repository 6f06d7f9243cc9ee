"""What preparing uint8 image pairs on the GPU costs and saves (demon_amd/csrc/ingest.hip; DemonContext.upload_images, Pipeline.buffers(B,
source_size=...)).

  python tools/ingest_bench.py [--out profiles/ingest_u8.json]

(a) kernel: the ingest launch at batch 32 by hip events, median of 20 after 5 warm-up launches -- identity (256 x 192 sources) and
    640 x 480 -> 256 x 192 -- beside a device-to-device hipMemcpyAsync of the bytes the kernel writes, timed in the same loop
    (demon_bench_ingest).  Bar: identity <= copy median + the spread (max - min) of the 20 copy timings.
(b) host to host: Pipeline.throughput pairs/s at batch 32, default lanes, 8 batches per pass, float buffers against uint8 buffers of the
    same pairs, legs alternating, three measurements each.  Bar: u8 median >= float median - (max - min of the float measurements).
(c) the host work removed: pairs/s of preprocess.prepare_input_arrays for 32 pairs on this host.
The resize case of (a), the 640 x 480 leg of (b) and (c) are recorded, not gated."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

import demon_amd.lanes  # noqa: E402,F401  (exports GPU_MAX_HW_QUEUES before the first HIP call)
from demon_amd import DemonContext, weights  # noqa: E402
from demon_amd.pipeline import Pipeline  # noqa: E402
from demon_amd.preprocess import prepare_input_arrays  # noqa: E402

N, H, W = 32, 192, 256


def images(n, h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8), rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def kernel_times(w):
    out = {}
    ctx = DemonContext(0, N, H, W)
    try:
        ctx.set_weights(w)
        out_bytes = 4 * N * (6 * H * W + 3 * (H // 4) * (W // 4))
        for name, (sh, sw) in (("identity_256x192", (192, 256)), ("resize_640x480", (480, 640))):
            ctx.upload_images(*images(N, sh, sw, seed=1))
            k, c = ctx.bench_ingest(N, warmup=5, iters=20)
            km, cm = statistics.median(k), statistics.median(c)
            in_bytes = 3 * N * (2 * H * W + (H // 4) * (W // 4))   # one source byte per output value (identity: the whole source once)
            out[name] = {"kernel_ms_median": round(km, 5), "kernel_ms_min": round(min(k), 5), "kernel_ms_max": round(max(k), 5),
                         "d2d_copy_ms_median": round(cm, 5), "d2d_copy_ms_min": round(min(c), 5), "d2d_copy_ms_max": round(max(c), 5),
                         "bytes_written": out_bytes, "bytes_gathered": in_bytes,
                         "kernel_gb_per_s": round((out_bytes + in_bytes) / km / 1e6, 1), "d2d_copy_gb_per_s": round(2 * out_bytes / cm / 1e6, 1)}
        r = out["identity_256x192"]
        r["bar"] = "kernel median <= copy median + (copy max - copy min)"
        r["bar_met"] = bool(r["kernel_ms_median"] <= r["d2d_copy_ms_median"] + (r["d2d_copy_ms_max"] - r["d2d_copy_ms_min"]))
    finally:
        ctx.close()
    return out


def host_to_host(w):
    pipe = Pipeline(w, batch=N)
    B = 8 * N
    legs = {}
    try:
        u1, u2 = images(B, H, W, seed=2)
        big1, big2 = images(B, 480, 640, seed=3)
        bufs = {"float": pipe.buffers(B), "u8_256x192": pipe.buffers(B, source_size=(H, W)), "u8_640x480": pipe.buffers(B, source_size=(480, 640))}
        try:
            bufs["float"].image_pair[:], bufs["float"].image2_2[:] = prepare_input_arrays(u1, u2)
            bufs["u8_256x192"].image1_u8[:], bufs["u8_256x192"].image2_u8[:] = u1, u2
            bufs["u8_640x480"].image1_u8[:], bufs["u8_640x480"].image2_u8[:] = big1, big2
            rates = {k: [] for k in bufs}
            for _ in range(3):
                for k, hb in bufs.items():
                    rates[k].append(pipe.throughput(hb, iterations=3, repeats=3)["pairs_per_s"])
            for k, v in rates.items():
                legs[k] = {"pairs_per_s": [round(x, 1) for x in v], "median": round(statistics.median(v), 1), "pinned": bool(bufs[k].pinned)}
        finally:
            for hb in bufs.values():
                hb.release()
    finally:
        pipe.close()
    spread = max(legs["float"]["pairs_per_s"]) - min(legs["float"]["pairs_per_s"])
    legs["lanes"] = 3
    legs["bar"] = "u8_256x192 median >= float median - (float max - float min)"
    legs["float_spread"] = round(spread, 1)
    legs["bar_met"] = bool(legs["u8_256x192"]["median"] >= legs["float"]["median"] - spread)
    return legs


def cpu_cost():
    out = {}
    for name, (sh, sw) in (("identity_256x192", (192, 256)), ("resize_640x480", (480, 640))):
        u1, u2 = images(N, sh, sw, seed=4)
        prepare_input_arrays(u1, u2)
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            prepare_input_arrays(u1, u2)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        out[name] = {"pairs_per_s": round(N / best, 1), "ms_per_32_pairs": round(1e3 * best, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_u8.json"))
    args = ap.parse_args()
    w = weights.synthetic_weights(seed=1)
    rec = {"what": "uint8 image pairs prepared on the GPU, batch %d at %dx%d (tools/ingest_bench.py)" % (N, W, H)}
    rec["a_kernel"] = kernel_times(w)
    print(json.dumps(rec["a_kernel"]), flush=True)
    rec["b_host_to_host"] = host_to_host(w)
    print(json.dumps(rec["b_host_to_host"]), flush=True)
    rec["c_cpu_prepare_input_arrays"] = cpu_cost()
    print(json.dumps(rec["c_cpu_prepare_input_arrays"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
