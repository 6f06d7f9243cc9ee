"""Records what libdemon_hip.so launches for a launch-plan entry, whether or not the entry fits the layer, and writes
tests/golden/dispatch_trace.npz (replayed by tests/test_dispatch_trace_gpu.py).

  python tools/record_dispatch_trace.py [--out tests/golden/dispatch_trace.npz]

Three sections, through the public Python API only (so the same script runs on any revision of the library):

  A  forced entries: DEMON_FORCE_PLAN="kind,tile,ks" on stand-alone layers at batch 3 -- every kind 0 .. 18 (the reserved numbers and the
     chain kinds included), tile 0, 1, the family's last variant and one past it, ks 0, 1, 3, 1002; per entry the kernel tag and the crc32
     of the output bytes
  B  bench tiles: bench_layer(tile=T, ksplit=K) over every encoded range; per entry the kernel tag or the error text
  C  tuned entries: set_plan(2, {layer: [kind, tile, ks]}) on named layers of one 192 x 256 network context; per entry the error text, or
     what get_plan returns, the kernel tag of the layer's step in profile_full and the crc32 of predict_depth0 of a one-iteration pass (run
     eagerly, option hipgraph = 0: the launches a graph would capture, without the capture); one entry installed for batch 2 runs batch 1

The trace is taken twice, in two fresh processes; the golden is written only when both agree on every text.  An entry whose checksum
differs between the two runs keeps its text and loses its checksum (the summary names it); entries of more than one kernel family
losing theirs is an error.  Metadata: commit, demon_amd.build.csrc_sha() and the hipcc version."""
import argparse
import json
import os
import subprocess
import sys
import zlib

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "dispatch_trace.npz")

# variants per plan kind: a hand copy of the *_COUNT / *_VARIANTS constants of csrc/internal.h, which must follow them -- when a family
# gains a variant and this table does not, the trace stays self-consistent but no longer probes "last" and "one past".  Numbers that are
# no kind get the im2col kernel's count: a forced entry of theirs runs as kind 0.
VARIANTS = {0: 8, 1: 9, 3: 1, 4: 18, 5: 22, 6: 22, 7: 18, 8: 7, 10: 13, 11: 2, 12: 1, 13: 1, 14: 1, 15: 20, 16: 16}
VARIANTS_SET_PLAN = {**VARIANTS, 3: 8}   # set_plan has always taken an im2col tile number for kind 3: it rejects from tile 8

# stand-alone layers (kind, cin, cout, kh, kw, sh, sw, H, W), shapes of tests/test_variants_gpu.py: the smallest at which each family
# applies or just fails to
LAYERS_A = {
    "row1x9s2": ("conv", 32, 32, 1, 9, 1, 2, 12, 64),
    "col3x1": ("conv", 64, 64, 3, 1, 1, 1, 48, 64),
    "c3x3": ("conv", 64, 64, 3, 3, 1, 1, 24, 32),
    "c3x3s2short": ("conv", 32, 64, 3, 3, 2, 2, 24, 32),
    "c3x3s2long": ("conv", 16, 64, 3, 3, 2, 2, 8, 64),
    "thin9x1s2": ("conv", 6, 32, 9, 1, 2, 1, 48, 64),
    "head24to4": ("conv", 24, 4, 3, 3, 1, 1, 6, 8),
    "plain5to3": ("conv", 5, 3, 3, 3, 1, 1, 9, 7),
    "up512to256": ("deconv", 512, 256, 0, 0, 0, 0, 6, 8),
    "up4to2": ("deconv", 4, 2, 0, 0, 0, 0, 6, 8),
    "up30to40": ("deconv", 30, 40, 0, 0, 0, 0, 9, 50),
    "dense8192": ("dense", 8192, 128, 0, 0, 0, 0, 1, 1),
}
BATCH_A = 3
KINDS_A = range(19)
KS_A = (0, 1, 3, 1002)

LAYERS_B = ("row1x9s2", "c3x3", "up512to256")
TILES_B = [-1] + list(range(8)) + list(range(100, 109)) + list(range(200, 218)) + list(range(300, 322)) + list(range(400, 413)) + [500]
KS_B = (0, 2)

NET = dict(max_batch=2, height=192, width=256, seed=1)
LAYERS_C = {
    "fused_y": "netFlow1/conv1y",                 # the k x 1 layer of a pair conv_pair.hip fuses
    "chain_y": "netFlow1/conv3_1y",               # the k x 1 layer of a chainable stride-1 pair ...
    "chain_x": "netFlow1/conv3_1x",               # ... and its 1 x k partner
    "level5_y": "netFlow1/conv5y",
    "upconv": "netFlow1/refine4/upconv",
    "fc1": "netDM1/motion_fc1",
    "head": "netFlow1/predict_flow2/conv2",       # Cout <= 4
    "refine3x3": "netRefine/conv1_1",
}
KINDS_C = range(18)
NEAREST = ("level5_y", [4, 10, 2])   # installed for batch 2, run at batch 1

SECTIONS = ["A-" + k for k in LAYERS_A] + ["B-" + k for k in LAYERS_B] + ["C-" + k for k in LAYERS_C] + ["C-nearest"]


def tiles_of(kind, variants=VARIANTS, second=True):
    """tile 0, (1,) the kind's last variant and one past it"""
    last = variants.get(kind, variants[0]) - 1
    return sorted({0, 1, last, last + 1} if second else {0, last, last + 1})


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def make_context():
    from demon_amd import DemonContext, weights
    ctx = DemonContext(0, NET["max_batch"], NET["height"], NET["width"])
    ctx.set_weights(weights.synthetic_weights(seed=NET["seed"], height=NET["height"], width=NET["width"]))
    ctx.set_option("hipgraph", 0)
    return ctx


def section_a(ctx, key):
    """[(entry, text, crc32)] of the forced entries on one stand-alone layer"""
    kind, cin, cout, kh, kw, sh, sw, H, W = LAYERS_A[key]
    rng = np.random.default_rng(30)
    b = rng.standard_normal((cout,)).astype(np.float32)
    if kind == "dense":
        x = rng.standard_normal((BATCH_A, cin)).astype(np.float32)
        w = (rng.standard_normal((cin, cout)) / np.sqrt(cin)).astype(np.float32)
        run = lambda: ctx.dense(x, w, b, lrelu=True)
    elif kind == "deconv":
        x = rng.standard_normal((BATCH_A, cin, H, W)).astype(np.float32)
        w = (rng.standard_normal((4, 4, cout, cin)) / np.sqrt(4 * cin)).astype(np.float32)
        run = lambda: ctx.deconv4x4s2(x, w, b, lrelu=True)
    else:
        x = rng.standard_normal((BATCH_A, cin, H, W)).astype(np.float32)
        w = (rng.standard_normal((kh, kw, cin, cout)) / np.sqrt(kh * kw * cin)).astype(np.float32)
        run = lambda: ctx.conv2d(x, w, b, (sh, sw), lrelu=True)
    out = []
    try:
        for k in KINDS_A:
            for t in tiles_of(k):
                for ks in KS_A:
                    os.environ["DEMON_FORCE_PLAN"] = "%d,%d,%d" % (k, t, ks)
                    got = run()
                    out.append(("A-%s/%d,%d,%d" % (key, k, t, ks), ctx.last_kernel(), crc(got)))
    finally:
        os.environ.pop("DEMON_FORCE_PLAN", None)
    return out


def section_b(ctx, key):
    from demon_amd.engine import DemonError
    kind, cin, cout, kh, kw, sh, sw, H, W = LAYERS_A[key]
    out = []
    for t in TILES_B:
        for ks in KS_B:
            try:
                ctx.bench_layer(kind, BATCH_A, cin, H, W, cout, max(kh, 1), max(kw, 1), max(sh, 1), max(sw, 1), tile=t, ksplit=ks, iters=1)
                text = ctx.last_kernel()
            except DemonError as e:
                text = "error: %s" % e
            out.append(("B-%s/%d,%d" % (key, t, ks), text, None))
    return out


def _net_inputs(n):
    rng = np.random.default_rng(0)
    pair = rng.random((n, 6, NET["height"], NET["width"]), dtype=np.float32) - np.float32(0.5)
    img2_2 = pair[:, 3:6].reshape(n, 3, NET["height"] // 4, 4, NET["width"] // 4, 4).mean(axis=(3, 5)).astype(np.float32)
    return pair, img2_2


def _step_tag(records, layer):
    """tag of the step that ran `layer`: its own step, or the step of its pair (named <k x 1 layer>+x) when that ran as one launch"""
    pair = (layer[:-1] + "y+x") if layer[-1:] in ("x", "y") else None
    for r in records:
        if r["name"] == layer:
            return "%s=%s" % (r["name"].rsplit("/", 1)[-1], r["kernel"])
    for r in records:
        if r["name"] == pair:
            return "%s=%s" % (r["name"].rsplit("/", 1)[-1], r["kernel"])
    return "no step"


def _run_entry(ctx, layer, entry, n):
    """set_plan(2, ...) then a pass at batch n; (text, crc32 or None)"""
    from demon_amd.engine import DemonError
    try:
        ctx.set_plan(2, {layer: entry})
    except DemonError as e:
        return "rejected: %s" % e, None
    try:
        stored = ctx.get_plan(2).get(layer)
        tag = _step_tag(ctx.profile_full(n, 1, 1), layer)
        pair, img2_2 = _net_inputs(n)
        depth0 = ctx.full(pair, img2_2, iterations=1)["predict_depth0"]
        return "stored %s %s" % (stored, tag), crc(depth0)
    finally:
        ctx.clear_plan(2)


def section_c(ctx, key):
    if key == "nearest":
        layer, entry = LAYERS_C[NEAREST[0]], NEAREST[1]
        text, c = _run_entry(ctx, layer, entry, 1)
        return [("C-nearest/%s,%d,%d,%d@1" % ((layer,) + tuple(entry)), text, c)]
    layer = LAYERS_C[key]
    out = []
    for k in KINDS_C:
        for t in tiles_of(k, VARIANTS_SET_PLAN, second=False):
            for ks in (1, 2, 1001) if k == 1 else (1, 2):
                text, c = _run_entry(ctx, layer, [k, t, ks], 2)
                out.append(("C-%s/%d,%d,%d" % (key, k, t, ks), text, c))
    return out


def trace_section(ctx, name):
    sec, key = name.split("-", 1)
    return {"A": section_a, "B": section_b, "C": section_c}[sec](ctx, key)


def load_golden(path=GOLDEN):
    """{entry: (text, crc32 or None)}, metadata"""
    with np.load(path, allow_pickle=False) as z:
        texts = [t.decode() for t in z["texts"]]
        entries = {e.decode(): (texts[i], int(c) if h else None) for e, i, c, h in zip(z["entries"], z["text_index"], z["crc32"], z["has_crc32"])}
        return entries, json.loads(bytes(z["meta"]).decode())


def _run_once(path):
    import time
    ctx = make_context()
    rows = []
    try:
        for name in SECTIONS:
            t0 = time.time()
            got = trace_section(ctx, name)
            print("%-16s %5d entries %6.2f s" % (name, len(got), time.time() - t0), flush=True)
            rows += got
    finally:
        ctx.close()
    with open(path, "w") as f:
        json.dump(rows, f)


def _family(text):
    for sep in ("=", " "):
        text = text.rsplit(sep, 1)[-1]
    return text.split("<")[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--commit", help="commit of the recorded tree (default: git rev-parse HEAD)")
    ap.add_argument("--run-once", metavar="JSON", help="(internal) one trace in this process, written as JSON")
    args = ap.parse_args()
    if args.run_once:
        _run_once(args.run_once)
        return
    runs = []
    for i in range(2):   # two fresh processes: this one never opens the GPU
        path = "%s.run%d.tmp" % (args.out, i)
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--run-once", path])
        with open(path) as f:
            runs.append(json.load(f))
        os.remove(path)
    a, b = runs
    if [r[:2] for r in a] != [r[:2] for r in b]:
        bad = [(x[0], x[1], y[1]) for x, y in zip(a, b) if x[:2] != y[:2]]
        raise SystemExit("the two runs disagree on %d texts, nothing written; first: %s" % (len(bad), bad[:5]))
    unstable = [x[0] for x, y in zip(a, b) if x[2] != y[2]]
    families = sorted({_family(x[1]) for x, y in zip(a, b) if x[2] != y[2]})
    for e in unstable:
        print("checksum differs between the two runs, stored without: %s" % e)
    if len(families) > 1:
        raise SystemExit("entries of more than one kernel family are not reproducible (%s), nothing written" % families)
    from demon_amd import build
    hipcc = subprocess.run([build._hipcc(), "--version"], capture_output=True, text=True).stdout.splitlines()
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    meta = {"commit": commit, "csrc_sha": build.csrc_sha(), "hipcc": hipcc[0] if hipcc else "", "unstable": unstable}
    texts = sorted({r[1] for r in a})
    index = {t: i for i, t in enumerate(texts)}
    has = np.array([r[2] is not None and r[0] not in unstable for r in a])
    np.savez_compressed(args.out, entries=np.array([r[0].encode() for r in a]), texts=np.array([t.encode() for t in texts]),
                        text_index=np.array([index[r[1]] for r in a], np.int32),
                        crc32=np.array([r[2] if h else 0 for r, h in zip(a, has)], np.uint32), has_crc32=has,
                        meta=np.frombuffer(json.dumps(meta).encode(), np.uint8))
    for sec in "ABC":
        mine = [bool(h) for r, h in zip(a, has) if r[0].startswith(sec + "-")]
        print("section %s: %d entries, %d with a checksum" % (sec, len(mine), sum(mine)))
    print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
