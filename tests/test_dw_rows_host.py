"""Host side of the register-window depthwise kernel (csrc/conv_dw3.hip): which descriptors it takes, and how the SLFP_DW_ROWS
switch is read.  No device is touched: slfp_debug_dw3x3_variant evaluates the launch predicates only."""
import ctypes
import os

import numpy as np
import pytest

from cnns_slfp_quantization_amd import _lib


def _desc(c=64, h=112, w=None, stride=2, pad=1, n=4, groups=None, k=3):
    return _lib.ConvDesc(n=n, c_in=c, h=h, w=h if w is None else w, c_out=c, kh=k, kw=k, stride_h=stride, stride_w=stride, pad_h=pad,
                         pad_w=pad, dil_h=1, dil_w=1, groups=c if groups is None else groups, x_layout=_lib.LAYOUT_NHWC,
                         y_layout=_lib.LAYOUT_NHWC, qbits=8, ka=float(np.float32(0.17)), kw_scale=float(np.float32(0.12)),
                         mfma_passes=0, reserved=0)


def _variant(d, post=0):
    return _lib.load().slfp_debug_dw3x3_variant(ctypes.byref(d), post).decode()


@pytest.fixture
def switch():
    L = _lib.load()
    old = os.environ.get("SLFP_DW_ROWS")

    def set_to(v):
        if v is None:
            os.environ.pop("SLFP_DW_ROWS", None)
        else:
            os.environ["SLFP_DW_ROWS"] = v
        L.slfp_debug_reload_switches()

    yield set_to
    set_to(old)


NET = [(64, 112), (128, 56), (256, 28), (512, 14)]   # MobileNetV1's stride-2 depthwise layers, size classes 0 .. 3


def test_switch_zero_keeps_the_tile_kernel(switch):
    for v in ("0", "-1", "off"):   # anything that does not parse to a positive mask
        switch(v)
        for c, h in NET:
            assert _variant(_desc(c, h)) == "tile" and _variant(_desc(c, h), 1) == "tile", (v, c, h)


def test_switch_mask_selects_size_classes(switch):
    for mask in range(1, 16):
        switch(str(mask))
        for cls, (c, h) in enumerate(NET):
            want = "rows" if mask >> cls & 1 else "tile"
            assert _variant(_desc(c, h)) == want and _variant(_desc(c, h), 1) == want, (mask, c, h)
    switch("0xF")
    assert all(_variant(_desc(c, h)) == "rows" for c, h in NET)


def test_unset_switch_is_the_measured_rule(switch):
    """profiles/notes/README.md (round 4): every size class measured faster on k_dw3x3_rows, at N = 128 and N = 256."""
    switch(None)
    for c, h in NET:
        for n in (1, 128, 256):
            assert _variant(_desc(c, h, n=n)) == "rows" and _variant(_desc(c, h, n=n), 1) == "rows", (c, h, n)


def test_preconditions(switch):
    switch("15")
    assert _variant(_desc(64, 112, stride=1)) == "tile"          # stride 1 stays on the tile kernel
    assert _variant(_desc(1024, 7, stride=1)) == "general"       # 7 x 7 images: conv_dw.hip
    assert _variant(_desc(24, 56)) == "general"                  # C not a multiple of 32 (ShuffleNetV2)
    assert _variant(_desc(96, 57, w=30, pad=0)) == "rows"        # ragged tiles, no padding
    assert _variant(_desc(32, 3, pad=1, n=3)) == "rows"          # images smaller than a wave's tasks
    assert _variant(_desc(32, 20, pad=2)) == "rows"
    assert _variant(_desc(64, 56, groups=1, k=1, stride=1, pad=0)) == "none"   # not a depthwise layer
    # the offsets mark an invalid row / column in bits 31 / 30: images above 2^30 bytes stay on the tile kernel
    assert _variant(_desc(32, 2896, n=1)) == "rows" and _variant(_desc(32, 2900, n=1)) == "tile"
