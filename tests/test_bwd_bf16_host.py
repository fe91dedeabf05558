"""Host side of the bf16 pointwise backward (csrc/conv_bwd_bf16.hip, slfp_conv2d_bwd_bf16): the supported set and its refusals, the
workspace query, the instance reporter and the option that selects it.  No device is touched."""
import ctypes
import os

import pytest

from cnns_slfp_quantization_amd import _lib
from cnns_slfp_quantization_amd import conv2d_func as cf


def _desc(n=2, h=17, w=17, c_in=64, c_out=128, k=1, stride=1, pad=0, groups=1, layout=_lib.LAYOUT_NHWC, qbits=8):
    return _lib.ConvDesc(n=n, c_in=c_in, h=h, w=w, c_out=c_out, kh=k, kw=k, stride_h=stride, stride_w=stride, pad_h=pad, pad_w=pad,
                         dil_h=1, dil_w=1, groups=groups, x_layout=layout, y_layout=layout, qbits=qbits, ka=0.2, kw_scale=0.1,
                         mfma_passes=0, reserved=0)


REFUSED = {
    "c_in % 8": dict(c_in=68), "c_out % 8": dict(c_out=124), "58 channels": dict(c_in=58, c_out=58), "nchw": dict(layout=_lib.LAYOUT_NCHW),
    "q_bit 32": dict(qbits=32), "measured slower: 25088 -> 4096 at batch 128": dict(n=128, h=1, w=1, c_in=25088, c_out=4096),
    "measured level: 256 -> 64 @56": dict(n=128, h=56, w=56, c_in=256, c_out=64),
    "measured level: 64 -> 128 @56": dict(n=128, h=56, w=56, c_in=64, c_out=128), "dense 3x3": dict(k=3, pad=1), "strided 1x1": dict(stride=2), "depthwise": dict(c_out=64, k=3, pad=1, groups=64),
}


@pytest.mark.parametrize("flags", [0, _lib.BWD_DENSE])
def test_supported_set_and_workspace(flags):
    L = _lib.load()
    for kw in (dict(), dict(qbits=7), dict(n=5, h=1, w=1, c_in=40, c_out=24), dict(c_in=8, c_out=8),
               dict(n=128, h=1, w=1, c_in=4096, c_out=4096), dict(n=512, h=1, w=1, c_in=25088, c_out=4096)):
        d = _desc(**kw)
        for codes in (0, 1):
            assert L.slfp_conv2d_bwd_bf16_supported(ctypes.byref(d), flags, codes) == 1, kw
        sizes = [L.slfp_conv2d_bwd_bf16_workspace_bytes(ctypes.byref(d), flags, gx, gw) for gx, gw in ((1, 1), (1, 0), (0, 1))]
        assert all(s > 0 for s in sizes) and sizes[0] == sizes[1] + sizes[2]
    for why, kw in REFUSED.items():
        d = _desc(**kw)
        for codes in (0, 1):
            assert L.slfp_conv2d_bwd_bf16_supported(ctypes.byref(d), flags, codes) == 0, why
            assert _lib.last_error(), why
            assert L.slfp_debug_bwd_bf16_instance(ctypes.byref(d), flags, codes, 1, 1) == b"none", why
        assert L.slfp_conv2d_bwd_bf16_workspace_bytes(ctypes.byref(d), flags, 1, 1) == 0, why


def test_without_a_threshold_table_the_codes_form_stays_whole():
    """SLFP_LONG_ENCODE leaves no table: float32 x is refused, codes (which need none) are taken, and the three queries agree."""
    L, d = _lib.load(), _desc()
    old = os.environ.get("SLFP_LONG_ENCODE")
    os.environ["SLFP_LONG_ENCODE"] = "1"
    L.slfp_debug_reload_switches()
    try:
        assert L.slfp_conv2d_bwd_bf16_supported(ctypes.byref(d), 0, 0) == 0 and "threshold table" in _lib.last_error()
        assert L.slfp_debug_bwd_bf16_instance(ctypes.byref(d), 0, 0, 1, 1) == b"none"
        assert L.slfp_conv2d_bwd_bf16_supported(ctypes.byref(d), 0, 1) == 1
        assert L.slfp_debug_bwd_bf16_instance(ctypes.byref(d), 0, 1, 1, 1) == b"pwb/gx/tm2tn1/t6+pwb/gw/tm2tn1/t6/codes/p2k304"
        assert L.slfp_conv2d_bwd_bf16_workspace_bytes(ctypes.byref(d), 0, 1, 1) > 0
        # the entry point gets as far as the next argument check (null gy), past support and the workspace
        assert L.slfp_conv2d_bwd_bf16(ctypes.byref(d), 0, None, 16, 16, None, 16, 16, 16, 16, None) == _lib.ERR_BAD_ARG
        assert "null gy" in _lib.last_error()
    finally:
        os.environ.pop("SLFP_LONG_ENCODE") if old is None else os.environ.__setitem__("SLFP_LONG_ENCODE", old)
        L.slfp_debug_reload_switches()


def test_argument_checks_come_before_any_device_work():
    """Null pointers stand for the tensors: every refusal below is made on the host.  16 is an aligned non-null address never read."""
    L, d, p = _lib.load(), _desc(), 16
    call = lambda d_, flags, x, xc, *rest: L.slfp_conv2d_bwd_bf16(d_, flags, x, xc, *rest, None)   # noqa: E731
    assert call(None, 0, p, None, p, p, p, p, p, p) == _lib.ERR_BAD_ARG
    assert call(ctypes.byref(d), 2, p, None, p, p, p, p, p, p) == _lib.ERR_BAD_ARG and "unknown flag bits" in _lib.last_error()
    assert L.slfp_conv2d_bwd_bf16_supported(ctypes.byref(d), 2, 0) == 0
    for x, xc in ((p, p), (None, None)):
        assert call(ctypes.byref(d), 0, x, xc, p, p, p, p, p, p) == _lib.ERR_BAD_ARG and "exactly one" in _lib.last_error()
    assert call(ctypes.byref(d), 0, p + 4, None, p, p, p, p, p, p) == _lib.ERR_ALIGNMENT
    assert call(ctypes.byref(d), 0, None, p + 2, p, p, p, p, p, p) == _lib.ERR_ALIGNMENT
    assert call(ctypes.byref(_desc(k=3, pad=1)), _lib.BWD_DENSE, p, None, p, p, p, p, p, p) == _lib.ERR_UNSUPPORTED
    assert call(ctypes.byref(_desc(c_in=68)), 0, p, None, p, p, p, p, p, p) == _lib.ERR_UNSUPPORTED and "multiples of 8" in _lib.last_error()
    assert call(ctypes.byref(d), 0, p, None, p, None, p, p, p, p) == _lib.ERR_BAD_ARG      # null gy
    assert call(ctypes.byref(d), 0, p, None, None, p, p, p, p, p) == _lib.ERR_BAD_ARG      # gx needs the weights
    assert call(ctypes.byref(d), 0, p, None, p, p, p, None, p, p) == _lib.ERR_BAD_ARG      # gb comes with gw
    assert call(ctypes.byref(d), 0, p, None, p, p, p, p, p, None) == _lib.ERR_BAD_ARG and "workspace" in _lib.last_error()
    assert call(ctypes.byref(d), 0, p, None, p, p, None, None, None, None) == _lib.OK       # nothing asked for


def test_instance_reporter():
    L = _lib.load()
    rep = lambda d, codes, gx, gw: L.slfp_debug_bwd_bf16_instance(ctypes.byref(d), 0, codes, gx, gw).decode()   # noqa: E731
    small = _desc(n=2, h=3, w=5, c_in=8, c_out=8)
    assert rep(small, 0, 1, 1) == "pwb/gx/tm1tn1/t6+pwb/gw/tm1tn1/t6/tab/p1k32"
    assert rep(small, 1, 0, 1) == "pwb/gw/tm1tn1/t6/codes/p1k32" and rep(small, 0, 0, 0) == "none"
    # M = 578: two splits of 304 rows (19 k-steps of 16, 9.5 of the kernel's 32), the last one 274 rows
    assert rep(_desc(), 0, 1, 1) == "pwb/gx/tm2tn1/t6+pwb/gw/tm2tn1/t6/tab/p2k304"
    assert rep(_desc(n=1, h=13, w=10, c_in=136, c_out=72), 1, 1, 1) == "pwb/gx/tm2tn2/t6+pwb/gw/tm1tn2/t6/codes/p1k144"


def test_option_is_validated():
    assert cf.options.backward_gemm == "f32"
    with pytest.raises(ValueError, match="backward_gemm"):
        cf.options.backward_gemm = "bf16"
    cf.options.backward_gemm = "bf16x3"
    cf.options.backward_gemm = "f32"
