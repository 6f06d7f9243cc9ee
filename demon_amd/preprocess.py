"""Host-side input preparation of the drivers: reference examples/example.py:15-42 (`prepare_input_data`).

Pure PIL / numpy, like the reference.  The reference calls `img.resize(size)` WITHOUT a filter, so its result depends on the
installed Pillow: NEAREST up to Pillow 6 -- including the 2.0.0 the reference pins (Dockerfile:15) -- and BICUBIC from 7.0 on
(hazard 1).  `resample` makes the choice explicit:
  "reference" (default)  NEAREST, what the reference's own environment computes
  "pil"                  no filter argument, i.e. whatever the installed Pillow defaults to (what the unmodified script does today)
  any PIL filter constant
tests/test_preprocess.py holds both modes to arrays produced by the reference function itself (tests/golden/make_golden_inputs.py).
"""
import numpy as np


def _resize(img, size, resample):
    from PIL import Image
    if resample == "pil":
        return img.resize(size)
    return img.resize(size, Image.NEAREST if resample == "reference" else resample)


def prepare_input_data(img1, img2, data_format, resample="reference"):
    """PIL images -> {'image_pair' [1,6,192,256], 'image1' [1,3,192,256], 'image2_2' [1,3,48,64]} in [-0.5, 0.5]
    (channels_last: [1,192,256,6], [1,192,256,3], [1,48,64,3]).  Same keys, shapes, dtype and values as the reference."""
    if data_format not in ("channels_first", "channels_last"):
        raise ValueError("data_format must be 'channels_first' or 'channels_last'")
    # scale images if necessary (:18-22); the quarter-size second image is made from the (resized) second image
    if img1.size[0] != 256 or img1.size[1] != 192:
        img1 = _resize(img1, (256, 192), resample)
    if img2.size[0] != 256 or img2.size[1] != 192:
        img2 = _resize(img2, (256, 192), resample)
    img2_2 = _resize(img2, (64, 48), resample)
    # [0, 255] -> [-0.5, 0.5] (:25-27): float32 division, then float32 subtraction, as numpy does for the reference
    arrs = [np.array(im).astype(np.float32) / 255 - 0.5 for im in (img1, img2, img2_2)]
    if data_format == "channels_first":
        arrs = [a.transpose([2, 0, 1]) for a in arrs]
        pair = np.concatenate((arrs[0], arrs[1]), axis=0)
    else:
        pair = np.concatenate((arrs[0], arrs[1]), axis=-1)
    return {"image_pair": pair[np.newaxis, :], "image1": arrs[0][np.newaxis, :], "image2_2": arrs[2][np.newaxis, :]}


def nearest_index_table(src, dst):
    """Source index of every output sample of a NEAREST resize of `src` samples to `dst`, as Pillow computes it: a running
    double-precision sum (xo = a0 / 2; idx[x] = int(xo); xo += a0), NOT floor((x + 0.5) * src / dst), which differs from it for
    e.g. 128 -> 192.  The identity when src == dst.  The GPU path (demon_amd/csrc/ingest.hip) builds its tables by the same rule."""
    src, dst = int(src), int(dst)
    if src < 1 or dst < 1:
        raise ValueError("src and dst must be >= 1")
    a0 = float(src) / dst
    idx = np.empty(dst, np.int64)
    xo = a0 * 0.5
    for x in range(dst):
        idx[x] = int(xo)
        xo += a0
    return idx


def prepare_input_arrays(image1_u8, image2_u8, height=192, width=256):
    """uint8 [n,h,w,3] (RGB) arrays -> (image_pair [n,6,H,W], image2_2 [n,3,H/4,W/4]) float32: prepare_input_data(..., "channels_first",
    resample="reference") for n pairs and any context size, in pure numpy.  This is the statement of what the GPU path computes
    (DemonContext.upload_images / prepare_inputs) and the expected value of its tests, bit for bit."""
    a1, a2 = np.asarray(image1_u8), np.asarray(image2_u8)
    if a1.dtype != np.uint8 or a2.dtype != np.uint8 or a1.ndim != 4 or a1.shape[3] != 3 or a1.shape != a2.shape:
        raise ValueError("images must be two uint8 arrays of the same shape [n,h,w,3]")
    if height % 4 or width % 4:
        raise ValueError("height and width must be multiples of 4")
    rows, cols = nearest_index_table(a1.shape[1], height), nearest_index_table(a1.shape[2], width)
    r1, r2 = (a[:, rows][:, :, cols] for a in (a1, a2))
    # the quarter-size image is a NEAREST resize of the RESIZED second image: ratio exactly 4, i.e. row 4 y + 2, column 4 x + 2
    q2 = r2[:, 2::4, 2::4]
    f1, f2, fq = (a.astype(np.float32) / 255 - 0.5 for a in (r1, r2, q2))
    pair = np.concatenate((f1.transpose(0, 3, 1, 2), f2.transpose(0, 3, 1, 2)), axis=1)
    return np.ascontiguousarray(pair), np.ascontiguousarray(fq.transpose(0, 3, 1, 2))
