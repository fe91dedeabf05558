"""Host side of the bf16 dense backward (csrc/conv_bwd_dense_bf16.hip, slfp_conv2d_bwd_dense_bf16): the supported set and its
refusals with their reasons, the agreement of the three host queries, the argument checks and the option.  No device is touched."""
import ctypes
import os

import pytest

from cnns_slfp_quantization_amd import _lib
from cnns_slfp_quantization_amd import conv2d_func as cf

DENSE = _lib.BWD_DENSE


def _desc(n=3, h=17, w=17, c_in=64, c_out=64, k=3, stride=1, pad=1, groups=1, dil=1, layout=_lib.LAYOUT_NHWC, qbits=8):
    return _lib.ConvDesc(n=n, c_in=c_in, h=h, w=w, c_out=c_out, kh=k, kw=k, stride_h=stride, stride_w=stride, pad_h=pad, pad_w=pad,
                         dil_h=dil, dil_w=dil, groups=groups, x_layout=layout, y_layout=layout, qbits=qbits, ka=0.2, kw_scale=0.1,
                         mfma_passes=0, reserved=0)


SUPPORTED = (dict(), dict(qbits=7), dict(stride=2), dict(k=1, stride=2, pad=0), dict(k=7, stride=2, pad=3, c_in=8, c_out=16),
             dict(n=128, h=56, w=56, c_in=64, c_out=64), dict(n=128, h=14, w=14, c_in=512, c_out=512))
REFUSED = {   # name: (descriptor, flags, a piece of the reason)
    "no flag": (dict(), 0, "SLFP_BWD_DENSE"),
    "pw": (dict(k=1, pad=0), DENSE, "pw family"),
    "depthwise": (dict(groups=64), DENSE, "depthwise"),
    "dilated": (dict(dil=2, pad=2), DENSE, "not a dense layer"),
    "nchw": (dict(layout=_lib.LAYOUT_NCHW), DENSE, "NHWC"),
    "stem C_in 3": (dict(c_in=3, k=7, stride=2, pad=3), DENSE, "multiples of 8"),
    "c_in % 8": (dict(c_in=68), DENSE, "multiples of 8"),
    "c_out % 8": (dict(c_out=60), DENSE, "multiples of 8"),
    "q_bit 32": (dict(qbits=32), DENSE, ""),
}


def test_supported_set_and_the_three_queries_agree():
    L = _lib.load()
    for kw in SUPPORTED:
        d = _desc(**kw)
        for codes in (0, 1):
            assert L.slfp_conv2d_bwd_dense_bf16_supported(ctypes.byref(d), DENSE, codes) == 1, kw
            assert L.slfp_debug_bwd_dense_bf16_instance(ctypes.byref(d), DENSE, codes, 1, 1).startswith(b"dnb/gx/tn"), kw
            assert L.slfp_conv2d_bwd_bf16_supported(ctypes.byref(d), DENSE, codes) == 0, kw   # the pw entry point keeps refusing
        sizes = [L.slfp_conv2d_bwd_dense_bf16_workspace_bytes(ctypes.byref(d), DENSE, gx, gw) for gx, gw in ((1, 1), (1, 0), (0, 1))]
        assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes[0] == sizes[1] + sizes[2]


@pytest.mark.parametrize("why", REFUSED)
def test_refusals_carry_their_reason(why):
    L = _lib.load()
    kw, flags, reason = REFUSED[why]
    d = _desc(**kw)
    for codes in (0, 1):
        assert L.slfp_conv2d_bwd_dense_bf16_supported(ctypes.byref(d), flags, codes) == 0
        assert _lib.last_error() and reason in _lib.last_error()
        assert L.slfp_debug_bwd_dense_bf16_instance(ctypes.byref(d), flags, codes, 1, 1) == b"none"
    assert L.slfp_conv2d_bwd_dense_bf16_workspace_bytes(ctypes.byref(d), flags, 1, 1) == 0
    x = L.slfp_conv2d_bwd_dense_bf16(ctypes.byref(d), flags, 16, None, 16, 16, 16, 16, 16, 16, None)
    assert x != _lib.OK and (x == _lib.ERR_UNSUPPORTED or why == "q_bit 32")


def test_without_a_threshold_table_the_codes_form_stays_whole():
    L, d = _lib.load(), _desc()
    old = os.environ.get("SLFP_LONG_ENCODE")
    os.environ["SLFP_LONG_ENCODE"] = "1"
    L.slfp_debug_reload_switches()
    try:
        assert L.slfp_conv2d_bwd_dense_bf16_supported(ctypes.byref(d), DENSE, 0) == 0 and "threshold table" in _lib.last_error()
        assert L.slfp_debug_bwd_dense_bf16_instance(ctypes.byref(d), DENSE, 0, 1, 1) == b"none"
        assert L.slfp_conv2d_bwd_dense_bf16_supported(ctypes.byref(d), DENSE, 1) == 1
        # M = 867: three splits of 304 rows (19 k-steps of 16), the last one 259 rows
        assert L.slfp_debug_bwd_dense_bf16_instance(ctypes.byref(d), DENSE, 1, 1, 1) == b"dnb/gx/tn1/t6+dnb/gw/tm1tn2/t6/codes/p3k304"
        assert L.slfp_debug_bwd_dense_bf16_instance(ctypes.byref(d), DENSE, 1, 0, 0) == b"none"
        assert L.slfp_conv2d_bwd_dense_bf16_workspace_bytes(ctypes.byref(d), DENSE, 1, 1) > 0   # does not depend on the table
    finally:
        os.environ.pop("SLFP_LONG_ENCODE") if old is None else os.environ.__setitem__("SLFP_LONG_ENCODE", old)
        L.slfp_debug_reload_switches()


def test_argument_checks_come_before_any_device_work():
    """Null pointers stand for the tensors: every refusal below is made on the host.  16 is an aligned non-null address never read."""
    L, d, p = _lib.load(), _desc(), 16
    call = lambda d_, flags, x, xc, *rest: L.slfp_conv2d_bwd_dense_bf16(d_, flags, x, xc, *rest, None)   # noqa: E731
    assert call(None, DENSE, p, None, p, p, p, p, p, p) == _lib.ERR_BAD_ARG
    assert call(ctypes.byref(d), 2, p, None, p, p, p, p, p, p) == _lib.ERR_BAD_ARG and "unknown flag bits" in _lib.last_error()
    assert L.slfp_conv2d_bwd_dense_bf16_supported(ctypes.byref(d), 2, 0) == 0
    for x, xc in ((p, p), (None, None)):
        assert call(ctypes.byref(d), DENSE, x, xc, p, p, p, p, p, p) == _lib.ERR_BAD_ARG and "exactly one" in _lib.last_error()
    assert call(ctypes.byref(d), DENSE, p + 4, None, p, p, p, p, p, p) == _lib.ERR_ALIGNMENT
    assert call(ctypes.byref(d), DENSE, None, p + 2, p, p, p, p, p, p) == _lib.ERR_ALIGNMENT
    assert call(ctypes.byref(d), DENSE, p, None, p, None, p, p, p, p) == _lib.ERR_BAD_ARG      # null gy
    assert call(ctypes.byref(d), DENSE, p, None, None, p, p, p, p, p) == _lib.ERR_BAD_ARG      # gx needs the weights
    assert call(ctypes.byref(d), DENSE, p, None, p, p, p, None, p, p) == _lib.ERR_BAD_ARG      # gb comes with gw
    assert call(ctypes.byref(d), DENSE, p, None, p, p, p, p, p, None) == _lib.ERR_BAD_ARG and "workspace" in _lib.last_error()
    assert call(ctypes.byref(d), DENSE, p, None, p, p, None, None, None, None) == _lib.OK       # nothing asked for


def test_option_takes_the_third_value():
    with pytest.raises(ValueError, match="backward_gemm"):
        cf.options.backward_gemm = "bf16"
    try:
        cf.options.backward_gemm = "bf16x3_all"
        assert cf.options.backward_gemm == "bf16x3_all"
    finally:
        cf.options.backward_gemm = "f32"
