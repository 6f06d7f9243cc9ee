"""What runs when a launch-plan entry does or does not fit its layer: the forced entries (DEMON_FORCE_PLAN), the tile encoding of
bench_layer and the tuned entries (set_plan) replayed against tests/golden/dispatch_trace.npz, which tools/record_dispatch_trace.py
recorded (see there for the three sections).  Kernel tags, accept / reject and error texts are always compared; the checksums of the
outputs only while the kernels and shipped plans are the recorded ones (demon_amd.build.csrc_sha() -- a kernel change re-records
the golden with the tool)."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_spec = importlib.util.spec_from_file_location("record_dispatch_trace", os.path.join(ROOT, "tools", "record_dispatch_trace.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)


@pytest.fixture(scope="module")
def golden():
    return T.load_golden()


@pytest.fixture(scope="module")
def trace_ctx():
    ctx = T.make_context()
    yield ctx
    ctx.close()


def test_golden_covers_every_section(golden):
    entries, meta = golden
    assert {e.split("/", 1)[0] for e in entries} == set(T.SECTIONS)
    assert meta["commit"] and meta["csrc_sha"] and meta["hipcc"]


@pytest.mark.parametrize("section", T.SECTIONS)
def test_dispatch_matches_recorded_trace(trace_ctx, golden, section):
    from demon_amd import build
    entries, meta = golden
    same_kernels = meta["csrc_sha"] == build.csrc_sha()
    got = T.trace_section(trace_ctx, section)
    want = {e: v for e, v in entries.items() if e.split("/", 1)[0] == section}
    assert [g[0] for g in got] == list(want), "the entries of %s are not the recorded ones: re-record the golden" % section
    wrong = [(e, text, want[e][0]) for e, text, _ in got if text != want[e][0]]
    assert not wrong, "%d of %d entries ran something else (entry, ran, recorded): %s" % (len(wrong), len(got), wrong[:8])
    if same_kernels:
        wrong = [(e, text) for e, text, c in got if want[e][1] is not None and c != want[e][1]]
        assert not wrong, "%d of %d entries gave other output bytes: %s" % (len(wrong), len(got), wrong[:8])
