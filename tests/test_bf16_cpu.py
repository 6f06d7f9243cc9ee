"""Option precision = bf16 without a GPU: argument checking before any HIP call, the kernel-name mapping of conv_bf16, and the
bf16-emulating oracle shim that tests/test_bf16_gpu.py checks whole nets against (defined here, imported there)."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


# ---- the bf16-emulating oracle shim ------------------------------------------------------------------------------------------------------
def bf16_round(a):
    """float32 -> the nearest bf16 value (round to nearest even; NaN stays NaN, overflow goes to inf), as float32"""
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def bf16_eligible(name, kernel_shape):
    """the rule of option precision = 1 (include/demon_hip.h) by TF variable name and kernel shape: conv HWIO [kh, kw, Cin, Cout],
    transposed conv [4, 4, Cout, Cin] (the nets have no 4 x 4 conv), dense [Cin, Cout]; Cin >= 16 and Cout >= 8, but motion_fc2"""
    if name.endswith("/motion_fc2"):
        return False
    if len(kernel_shape) == 2:
        cin, cout = kernel_shape
    elif tuple(kernel_shape[:2]) == (4, 4):
        cout, cin = kernel_shape[2], kernel_shape[3]
    else:
        cin, cout = kernel_shape[2], kernel_shape[3]
    return cin >= 16 and cout >= 8


class _RoundingF:
    """stands in for torch.nn.functional inside oracle.net_ref: conv2d / conv_transpose2d / linear round their input to bf16 when
    the weight they get was marked by the patched getters"""

    def __init__(self, F):
        self._F = F

    def __getattr__(self, key):
        return getattr(self._F, key)

    def _wrap(self, fn, x, w, *args, **kw):
        if getattr(w, "_bf16", False):
            x = x.to(torch.bfloat16).to(torch.float32)
        return fn(x, w, *args, **kw)

    def conv2d(self, x, w, *args, **kw):
        return self._wrap(self._F.conv2d, x, w, *args, **kw)

    def conv_transpose2d(self, x, w, *args, **kw):
        return self._wrap(self._F.conv_transpose2d, x, w, *args, **kw)

    def linear(self, x, w, *args, **kw):
        return self._wrap(self._F.linear, x, w, *args, **kw)


@contextlib.contextmanager
def emulate_bf16():
    """oracle.net_ref computes what option precision = 1 computes: the weights of eligible layers rounded to bf16 and marked by the
    Net weight getters (they know the layer name), and the input of every contraction that gets a marked weight rounded by a
    wrapper around net_ref.F.  oracle/ itself is not edited; everything is restored on exit."""
    from oracle import net_ref
    saved = {k: getattr(net_ref.Net, k) for k in ("_conv_w", "_deconv_w", "_dense_w")}
    saved_F = net_ref.F
    cache = {}

    def patched(kind, orig):
        def getter(self, name):
            key = (id(self), kind, name)
            if key not in cache:
                w, b = orig(self, name)
                full = "%s/%s" % (self.scope, name)
                if bf16_eligible(full, np.shape(self.w[full + "/kernel"])):
                    w = w.to(torch.bfloat16).to(torch.float32)
                    w._bf16 = True
                cache[key] = (w, b, self)   # (self kept alive: its id stays unique while the cache exists)
            return cache[key][:2]
        return getter

    try:
        for k, orig in saved.items():
            setattr(net_ref.Net, k, patched(k, orig))
        net_ref.F = _RoundingF(saved_F)
        yield
    finally:
        for k, orig in saved.items():
            setattr(net_ref.Net, k, orig)
        net_ref.F = saved_F


# ---- tests ---------------------------------------------------------------------------------------------------------------------------
def test_precision_is_validated_before_any_hip_call():
    from demon_amd import DemonContext
    from demon_amd.engine import DemonError
    for bad in ("fp16", "bfloat16", 1, None):
        with pytest.raises(DemonError):
            DemonContext(0, 1, precision=bad)
    from demon_amd.lanes import LaneGroup
    with pytest.raises(DemonError):
        LaneGroup(None, lanes=2, precision="fp16")


def test_conv_bf16_kernel_names_round_trip():
    from demon_amd import kernel_names
    for bm, bn, wm, wn in ((128, 128, 2, 2), (64, 128, 2, 2), (32, 128, 1, 4), (64, 64, 2, 2), (32, 64, 1, 2), (32, 32, 1, 1),
                           (128, 32, 4, 1), (64, 32, 2, 1)):
        name = "void demon::conv_bf16_kernel<%d, %d, %d, %d>(demon::ConvArgs, __bf16 __attribute__((ext_vector_type(8))) const*, long)" % (bm, bn, wm, wn)
        tag = kernel_names.kernel_tag(name)
        assert tag == "conv_bf16<%dx%d>" % (bm, bn)
        assert len(tag + "+splitk") < 32   # LaunchRecord.kernel
        assert kernel_names.rocprof_kernel_name(tag + "+splitk") == "demon::conv_bf16_kernel<%d, %d, ...>" % (bm, bn)
    # the fp32 kernel keeps its own tag
    assert kernel_names.kernel_tag("void demon::conv_mfma_kernel<128, 32, 4, 1>(demon::ConvArgs)") == "conv_mfma<128x32>"


def test_bf16_round_is_round_to_nearest_even():
    one = np.float32(1.0)
    ulp = np.float32(2.0 ** -7)   # bf16 spacing at 1
    x = np.array([1 + 2.0 ** -9, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, -(1 + 2.0 ** -8), 3.4e38, -3.4e38,
                  np.inf, -np.inf, 1e-40, 0.0], np.float32)
    want = np.array([one, one, one + 2 * ulp, one + ulp, -one, np.inf, -np.inf, np.inf, -np.inf, 1e-40, 0.0], np.float32)
    got = bf16_round(x)
    np.testing.assert_array_equal(got[:9], want[:9])
    assert got[10] == 0.0
    # a tie goes to the even neighbour, in both directions
    assert bf16_round(np.float32(1 + 2.0 ** -8)) == 1.0 and bf16_round(np.float32(1 + 3 * 2.0 ** -8)) == np.float32(1 + 2.0 ** -6)
    # NaN stays NaN (also payloads an integer rounding would carry into the exponent)
    nan = np.array([0x7fc00000, 0x7f800001, 0xffffffff, 0x7fffffff], np.uint32).view(np.float32)
    assert np.isnan(bf16_round(nan)).all()
    # against an independent bit-level statement of round to nearest even on random values
    rng = np.random.default_rng(0)
    v = rng.standard_normal(100000).astype(np.float32) * np.float32(1e3)
    u = v.view(np.uint32).astype(np.uint64)
    ref = (((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
    np.testing.assert_array_equal(bf16_round(v), ref)


def test_the_shim_rounds_exactly_the_eligible_layers(synth_weights):
    from oracle import net_ref
    names = sorted(k[:-len("/kernel")] for k in synth_weights if k.endswith("/kernel"))
    eligible = {n for n in names if bf16_eligible(n, np.shape(synth_weights[n + "/kernel"]))}
    excluded = set(names) - eligible
    for n in ("netFlow1/conv1y", "netDM2/conv2_extra_inputsy", "netRefine/conv0", "netDM1/motion_fc2", "netDM1/motion_fc3",
              "netFlow2/upsample_flow5to4/upconv", "netFlow1/predict_flow5/conv2", "netDM1/predict_depthnormal2/conv2"):
        assert n in excluded, n
    assert len(excluded) == 21
    for n in ("netFlow1/conv1x", "netFlow1/conv2y", "netFlow1/conv5_1x", "netDM1/motion_fc1", "netRefine/conv1"):
        assert n in eligible, n
    # the excluded layers hold a small part of the parameters (about 0.28 M of 45.7 M in the real model)
    size = lambda ns: sum(int(np.prod(np.shape(synth_weights[n + "/kernel"]))) for n in ns)
    assert size(excluded) < 0.02 * size(names)

    torch.manual_seed(0)
    x = torch.randn(1, 512, 6, 8) + 1 / 512
    with emulate_bf16():
        net = net_ref.Net(synth_weights, "netFlow1")
        w, _ = net._conv_w("conv5_1y")
        assert getattr(w, "_bf16", False)
        np.testing.assert_array_equal(w.numpy(), bf16_round(np.transpose(synth_weights["netFlow1/conv5_1y/kernel"], (3, 2, 0, 1))))
        wx, _ = net._conv_w("conv1y")
        assert not getattr(wx, "_bf16", False)
        y = net.conv(x, "conv5_1y")
    y_ref = net_ref.lrelu(torch.nn.functional.conv2d(torch.nn.functional.pad(torch.from_numpy(bf16_round(x.numpy())), (0, 0, 1, 1)),
                                                     torch.from_numpy(bf16_round(np.transpose(synth_weights["netFlow1/conv5_1y/kernel"], (3, 2, 0, 1)))),
                                                     torch.from_numpy(synth_weights["netFlow1/conv5_1y/bias"])))
    np.testing.assert_array_equal(y.numpy(), y_ref.numpy())
    # restored on exit
    assert net_ref.F is torch.nn.functional
    w2, _ = net_ref.Net(synth_weights, "netFlow1")._conv_w("conv5_1y")
    assert not getattr(w2, "_bf16", False)
