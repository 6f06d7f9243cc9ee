"""bench.py --dump-outputs on the host side: float32 files named after the outputs, the 64 MB bound kept by a seeded sample of the
pairs that is the same in every array and from run to run."""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _outputs(n):
    rng = np.random.default_rng(5)
    return {"predict_depth0": rng.standard_normal((n, 1, 8, 8)), "predict_rotation": rng.standard_normal((n, 3)).astype(np.float32)}


def test_dump_writes_every_output_as_float32(tmp_path):
    arrays = _outputs(6)
    keep = bench.dump_outputs(str(tmp_path), arrays)
    assert list(keep) == list(range(6))
    assert sorted(os.listdir(str(tmp_path))) == ["predict_depth0.npy", "predict_rotation.npy"]
    for k, v in arrays.items():
        got = np.load(str(tmp_path / (k + ".npy")))
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, v.astype(np.float32))


def test_dump_over_the_bound_keeps_the_same_seeded_pairs(tmp_path, monkeypatch):
    arrays = _outputs(40)
    per_pair = 4 * (64 + 3)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 10 * per_pair)
    keep = bench.dump_outputs(str(tmp_path / "a"), arrays)
    again = bench.dump_outputs(str(tmp_path / "b"), arrays)
    assert len(keep) == 10 and list(keep) == sorted(set(keep)) and list(keep) == list(again)
    total = 0
    for k, v in arrays.items():
        a, b = np.load(str(tmp_path / "a" / (k + ".npy"))), np.load(str(tmp_path / "b" / (k + ".npy")))
        np.testing.assert_array_equal(a, v[keep].astype(np.float32))
        np.testing.assert_array_equal(a, b)
        total += a.nbytes
    assert total <= bench.DUMP_LIMIT_BYTES
