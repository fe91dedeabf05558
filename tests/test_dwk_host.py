"""Host side of the opt-in depthwise k x k family (csrc/conv_dwk.hip; SLFP_DESC_DW_KXK in the descriptor's `reserved` word;
conv2d_func.options.depthwise): what plans onto it and with which selection, what stays where it was, and that the option reaches
the plan key.  No device is touched.  The table of shapes is shared with tests/test_gpu_dwk.py."""
import ctypes

import numpy as np
import pytest
import torch

from cnns_slfp_quantization_amd import _lib, conv2d_func as cf

BIT = _lib.DESC_DW_KXK
KA, KW = 0.21, 0.027

# the rows of tests/test_gpu_dwk.py, which runs them on the device
# (kernel, stride, (pad_h, pad_w), C, H, W, BN scale / shift + ReLU?, the selection the launch must report)
ROWS = {
    "full_group": (5, 1, (2, 2), 32, 13, 19, False, "k5/s1/14x14/r4x4"),
    "ragged_group_s2": (5, 2, (2, 2), 40, 13, 19, False, "k5/s2/7x8/r8x2"),
    "tiles_both_ways": (7, 1, (3, 3), 32, 17, 35, False, "k7/s1/14x14/r4x4"),
    "v3_width_s2": (7, 2, (3, 3), 72, 20, 21, False, "k7/s2/7x8/r8x1"),
    "no_padding": (5, 1, (0, 0), 8, 9, 11, False, "k5/s1/7x7/r4x2"),
    "window_mostly_padding": (7, 1, (3, 3), 32, 4, 4, False, "k7/s1/7x7/r4x2"),
    "unequal_padding": (5, 1, (2, 1), 64, 12, 14, False, "k5/s1/14x14/r4x4"),
    "map7_k7": (7, 1, (3, 3), 64, 7, 7, False, "k7/s1/7x7/r4x2"),
    "bias_post": (5, 2, (2, 2), 96, 14, 14, True, "k5/s2/7x8/r8x2"),
}


def row_desc(lib, name, qbits=8, reserved=None, **change):
    k, s, (ph, pw), c, h, w_ = ROWS[name][:6]
    f = dict(n=2, c_in=c, h=h, w=w_, c_out=c, kh=k, kw=k, stride_h=s, stride_w=s, pad_h=ph, pad_w=pw, dil_h=1, dil_w=1, groups=c,
             x_layout=lib.LAYOUT_NHWC, y_layout=lib.LAYOUT_NHWC, qbits=qbits, ka=float(np.float32(KA)), kw_scale=float(np.float32(KW)),
             mfma_passes=lib.MFMA_DEFAULT, reserved=lib.DESC_DW_KXK if reserved is None else reserved)
    f.update(change)
    return lib.ConvDesc(**f)


def _name(d):
    return _lib.load().slfp_conv2d_kernel_name(ctypes.byref(d)).decode()


def _variant(d):
    return _lib.load().slfp_debug_dwk_variant(ctypes.byref(d)).decode()


def _sizes(d):
    L = _lib.load()
    ho, wo = ctypes.c_int64(), ctypes.c_int64()
    assert L.slfp_conv2d_out_shape(ctypes.byref(d), ctypes.byref(ho), ctypes.byref(wo)) == _lib.OK
    return L.slfp_conv2d_wprep_bytes(ctypes.byref(d)), L.slfp_conv2d_workspace_bytes(ctypes.byref(d)), ho.value, wo.value


@pytest.mark.parametrize("name", ROWS)
def test_the_bit_plans_a_depthwise_kxk_layer_onto_the_window_kernel(name):
    k, c = ROWS[name][0], ROWS[name][3]
    d, d0 = row_desc(_lib, name), row_desc(_lib, name, reserved=0)
    assert _name(d) == "dwk_nhwc" == _name(row_desc(_lib, name, qbits=7)) and _variant(d) == ROWS[name][7]
    assert _name(row_desc(_lib, name, mfma_passes=_lib.MFMA_F16X3)) == "dwk_nhwc"
    assert _name(d0) == "direct_nhwc" and _variant(d0) == "none"
    # the direct kernel's blob [kh][kw][C] float32 and no workspace, under the bit and without it
    assert _sizes(d) == _sizes(d0) and _sizes(d)[:2] == (-(-k * k * c * 4 // 256) * 256, 0)
    nchw = dict(x_layout=_lib.LAYOUT_NCHW, y_layout=_lib.LAYOUT_NCHW)
    assert _name(row_desc(_lib, name, **nchw)) == "dwk_nhwc" and _sizes(row_desc(_lib, name, **nchw)) == _sizes(row_desc(_lib, name, reserved=0, **nchw))


REFUSED = {
    "k3": (dict(kh=3, kw=3, pad_h=1, pad_w=1), "dw3x3_nhwc"),
    "k9": (dict(kh=9, kw=9, pad_h=4, pad_w=4), "direct_nhwc"),
    "kh_ne_kw": (dict(kh=5, kw=7), "direct_nhwc"),
    "dil2": (dict(dil_h=2, dil_w=2), "direct_nhwc"),
    "stride3": (dict(stride_h=3, stride_w=3), "direct_nhwc"),
    "c6": (dict(c_in=6, c_out=6, groups=6), "direct_nhwc"),
    "pad_k": (dict(pad_h=5, pad_w=5), "direct_nhwc"),
    "half_groups": (dict(groups=16), "direct_nhwc"),
}


@pytest.mark.parametrize("why", REFUSED)
def test_what_the_kernel_refuses_stays_where_it_was(why):
    change, kernel = REFUSED[why]
    d = row_desc(_lib, "full_group", **change)
    assert _name(d) == kernel == _name(row_desc(_lib, "full_group", reserved=0, **change)) and _variant(d) == "none"
    assert _sizes(d) == _sizes(row_desc(_lib, "full_group", reserved=0, **change))


def test_the_bit_changes_nothing_else():
    L = _lib.load()
    d = row_desc(_lib, "bias_post")
    io = _lib.ConvIo(x_codes=1, y_codes=1, y_ka=0.2, y_qbits=8)
    assert L.slfp_conv2d_codes_supported(ctypes.byref(d), ctypes.byref(io), 0, 0) == 0
    assert L.slfp_conv2d_bwd_kernel_name(ctypes.byref(d)).decode() == "composite"
    # the other option bits next to it are fine and change nothing here; bits 2 and 4 stay unknown
    both = row_desc(_lib, "bias_post", reserved=BIT | _lib.DESC_DILATED_MFMA | _lib.DESC_GROUPED_MFMA)
    assert _name(both) == "dwk_nhwc" and _variant(both) == _variant(d) and _sizes(both) == _sizes(d)
    ho, wo = ctypes.c_int64(), ctypes.c_int64()
    bad = row_desc(_lib, "bias_post", reserved=BIT | 2)
    assert L.slfp_conv2d_out_shape(ctypes.byref(bad), ctypes.byref(ho), ctypes.byref(wo)) == _lib.ERR_BAD_ARG and _name(bad) == "invalid"


def test_the_option_is_validated_and_keys_the_plan():
    assert cf.options.depthwise == "direct"
    with pytest.raises(ValueError):
        cf.options.depthwise = "mfma"
    mod = cf.conv2d_Q(8, 0.027, 0.21)(64, 64, 5, padding=2, groups=64)
    x = torch.empty((2, 64, 13, 19), device="meta")
    try:
        names = {}
        for mode in ("direct", "kxk"):
            cf.options.depthwise = mode
            names[mode] = cf._plan(mod, x, mod.weight, True, True).kernel
    finally:
        cf.options.depthwise = "direct"
    assert names == {"direct": "direct_nhwc", "kxk": "dwk_nhwc"} and len(mod._plans) == 2
