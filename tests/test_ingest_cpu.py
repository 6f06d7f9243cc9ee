"""The CPU statement of the uint8 ingest path (demon_amd/preprocess.py: nearest_index_table, prepare_input_arrays) against Pillow and
against the reference function's own arrays (tests/golden/sculpture_inputs.npz).  Everything is bit for bit: the resize is a gather
and the value is one float32 division and one float32 subtraction.  tests/test_ingest_gpu.py holds the GPU kernel to these functions."""
import hashlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
GOLDEN = os.path.join(HERE, "golden", "sculpture_inputs.npz")

DESTINATIONS = (48, 64, 192, 256, 480, 640)
# (src, dst) the GPU cases of tests/test_ingest_gpu.py resize along an axis
DISCRIMINATING = ((128, 192), (256, 640), (64, 480))


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _closed_form(src, dst):
    return np.floor((np.arange(dst) + 0.5) * src / dst).astype(np.int64)


@pytest.mark.parametrize("dst", DESTINATIONS)
def test_index_table_is_pillows_nearest(dst):
    """Image.resize(NEAREST) of an index ramp returns the source index of every output sample: every source length 1..700.
    A ramp longer than 256 does not fit one uint8 row, so mode "I" (32-bit integers) carries it."""
    from PIL import Image
    from demon_amd.preprocess import nearest_index_table
    for src in range(1, 701):
        ramp = Image.fromarray(np.arange(src, dtype=np.int32)[None, :])
        along_x = np.asarray(ramp.resize((dst, 1), Image.NEAREST))[0]
        table = nearest_index_table(src, dst)
        assert table.shape == (dst,) and table.min() >= 0 and table.max() < src, (src, dst)
        np.testing.assert_array_equal(table, along_x, err_msg="%d -> %d" % (src, dst))
    # rows follow the same rule as columns
    for src in (1, 33, 128, 384, 700):
        ramp = Image.fromarray(np.arange(src, dtype=np.int32)[:, None])
        np.testing.assert_array_equal(nearest_index_table(src, dst), np.asarray(ramp.resize((1, dst), Image.NEAREST))[:, 0])


def test_index_table_identity_and_quarter():
    from demon_amd.preprocess import nearest_index_table
    for d in DESTINATIONS + (1, 32, 700):
        np.testing.assert_array_equal(nearest_index_table(d, d), np.arange(d))
    for d in (192, 256, 480, 640, 32):   # ratio exactly 4: sample 4 x + 2 (what the kernel's quarter-size planes rely on)
        np.testing.assert_array_equal(nearest_index_table(d, d // 4), 4 * np.arange(d // 4) + 2)
    with pytest.raises(ValueError):
        nearest_index_table(0, 4)


@pytest.mark.parametrize("src,dst", DISCRIMINATING)
def test_closed_form_is_wrong_for_the_gpu_cases(src, dst):
    """the sizes the GPU tests use tell Pillow's running sum from floor((x + 0.5) src / dst): a kernel (or a table) built on the
    closed form fails them"""
    from demon_amd.preprocess import nearest_index_table
    assert (nearest_index_table(src, dst) != _closed_form(src, dst)).any()


@pytest.mark.parametrize("big", [False, True])
def test_prepare_input_arrays_is_prepare_input_data(big):
    from PIL import Image
    from demon_amd.preprocess import prepare_input_arrays, prepare_input_data
    from make_golden_inputs import big_pair
    g = np.load(GOLDEN)
    u1, u2 = g["image1_u8"], g["image2_u8"]
    if big:
        u1, u2 = big_pair(u1), big_pair(u2)   # 512 x 384
    want = prepare_input_data(Image.fromarray(u1), Image.fromarray(u2), "channels_first", resample="reference")
    pair, img22 = prepare_input_arrays(u1[None], u2[None])
    assert pair.dtype == np.float32 and img22.dtype == np.float32 and pair.flags["C_CONTIGUOUS"] and img22.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(pair, want["image_pair"])
    np.testing.assert_array_equal(img22, want["image2_2"])
    tag = "big_" if big else ""
    assert _sha(pair) == str(g["sha256_%simage_pair_channels_first_nearest" % tag])
    assert _sha(img22) == str(g["sha256_%simage2_2_channels_first_nearest" % tag])
    assert _sha(pair[:, :3]) == str(g["sha256_%simage1_channels_first_nearest" % tag])
    # a batch is the pairs one by one
    p2, q2 = prepare_input_arrays(np.stack([u1, u2]), np.stack([u2, u1]))
    np.testing.assert_array_equal(p2[0], pair[0])
    np.testing.assert_array_equal(p2[1, :3], pair[0, 3:])
    np.testing.assert_array_equal(q2[0], img22[0])


def test_prepare_input_arrays_at_480x640_against_pillow():
    """another context size, sources that shrink and grow, against Pillow directly (prepare_input_data is fixed to 192 x 256)"""
    from PIL import Image
    from demon_amd.preprocess import prepare_input_arrays
    g = np.load(GOLDEN)
    rng = np.random.default_rng(5)
    sources = [(g["image1_u8"], g["image2_u8"]), (rng.integers(0, 256, (64, 256, 3), dtype=np.uint8), rng.integers(0, 256, (64, 256, 3), dtype=np.uint8)),
               (rng.integers(0, 256, (600, 700, 3), dtype=np.uint8), rng.integers(0, 256, (600, 700, 3), dtype=np.uint8))]
    for u1, u2 in sources:
        pair, img22 = prepare_input_arrays(u1[None], u2[None], 480, 640)
        r1, r2 = (Image.fromarray(u).resize((640, 480), Image.NEAREST) for u in (u1, u2))
        q2 = r2.resize((160, 120), Image.NEAREST)
        f1, f2, fq = (np.array(im).astype(np.float32) / 255 - 0.5 for im in (r1, r2, q2))
        np.testing.assert_array_equal(pair[0], np.concatenate((f1.transpose(2, 0, 1), f2.transpose(2, 0, 1))))
        np.testing.assert_array_equal(img22[0], fq.transpose(2, 0, 1))


def test_prepare_input_arrays_refuses_what_it_does_not_do():
    from demon_amd.preprocess import prepare_input_arrays
    u = np.zeros((1, 8, 8, 3), np.uint8)
    with pytest.raises(ValueError):
        prepare_input_arrays(u.astype(np.float32), u)
    with pytest.raises(ValueError):
        prepare_input_arrays(u[..., :1], u[..., :1])      # grayscale
    with pytest.raises(ValueError):
        prepare_input_arrays(u, np.zeros((1, 8, 9, 3), np.uint8))


def test_python_argument_checks_need_no_gpu():
    """dtype, shape and contiguity are refused before any library call"""
    from demon_amd.engine import DemonError, _u8_pair
    u = np.zeros((2, 8, 10, 3), np.uint8)
    assert _u8_pair(u, u)[0] is u
    for bad in (u.astype(np.float32), u[0], u[..., :2], u[:, :, ::2], np.zeros((0, 8, 10, 3), np.uint8)):
        with pytest.raises(DemonError):
            _u8_pair(bad, bad)
    with pytest.raises(DemonError):
        _u8_pair(u, np.zeros((2, 8, 11, 3), np.uint8))
