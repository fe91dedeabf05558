"""Host side of the opt-in grouped family (csrc/conv_grouped.hip; SLFP_DESC_GROUPED_MFMA in the descriptor's `reserved` word;
conv2d_func.options.grouped): what plans onto it and with which selection, what stays where it was, and that the option reaches
the plan key.  No device is touched."""
import ctypes

import pytest
import torch

from cnns_slfp_quantization_amd import _lib, conv2d_func as cf
from test_gpu_grouped import ROWS, row_desc

BIT = _lib.DESC_GROUPED_MFMA


def _name(d):
    return _lib.load().slfp_conv2d_kernel_name(ctypes.byref(d)).decode()


def _variant(d):
    return _lib.load().slfp_debug_grouped_variant(ctypes.byref(d)).decode()


def _sizes(d):
    L = _lib.load()
    return L.slfp_conv2d_wprep_bytes(ctypes.byref(d)), L.slfp_conv2d_workspace_bytes(ctypes.byref(d))


@pytest.mark.parametrize("name", ROWS)
def test_the_bit_plans_a_grouped_layer_onto_the_block_diagonal_kernel(name):
    c, o, g, _, _, k = ROWS[name][:6]
    d = row_desc(_lib, name)
    assert _name(d) == "grouped_mfma_f16x1" and _name(row_desc(_lib, name, qbits=7)) == "grouped_mfma_f16_exact"
    assert _name(row_desc(_lib, name, mfma_passes=_lib.MFMA_DEFAULT)) == "grouped_mfma_f16x1"
    assert _variant(d) == ROWS[name][9]
    # the blob [set][n_tile][k_step][64][8] fp16 as the variant spells it; no operand workspace
    gs, sp, nt, ks = (int(f[2:]) for f in _variant(d).split("/")[:4])
    assert _sizes(d) == (-(-g // gs) * nt * ks * 1024, 0)
    assert _name(row_desc(_lib, name, x_layout=_lib.LAYOUT_NCHW, y_layout=_lib.LAYOUT_NCHW)) == "grouped_mfma_f16x1"
    # bit clear: today's plan and today's blob
    d0 = row_desc(_lib, name, reserved=0)
    assert _name(d0) == "direct_nhwc" and _variant(d0) == "none"
    assert _sizes(d0)[0] == -(-k * k * (c // g) * o * 4 // 256) * 256


REFUSED = {
    "dil2": dict(dil_h=2, dil_w=2, pad_h=2, pad_w=2),
    "stride3": dict(stride_h=3, stride_w=3),
    "f16x3": dict(mfma_passes=_lib.MFMA_F16X3),
    "cg2": dict(c_in=16, c_out=32),                  # groups 8: Cg = 2
    "width128": dict(c_in=256, c_out=256, groups=2),
    "groups1": dict(groups=1, dil_h=2, dil_w=2, pad_h=2, pad_w=2),   # (at dilation 1 a groups-1 layer is dense_mfma_*)
}


@pytest.mark.parametrize("why", REFUSED)
def test_what_the_kernel_refuses_stays_on_the_direct_kernel(why):
    d = row_desc(_lib, "two_sets_two_taps_per_step", **REFUSED[why])
    assert _name(d) == "direct_nhwc" and _variant(d) == "none"
    assert _sizes(d) == _sizes(row_desc(_lib, "two_sets_two_taps_per_step", reserved=0, **REFUSED[why]))


def test_the_bit_changes_nothing_else():
    L = _lib.load()
    dw = dict(c_in=32, c_out=32, groups=32)
    assert _name(row_desc(_lib, "post_op", **dw)) == "dw3x3_nhwc" == _name(row_desc(_lib, "post_op", reserved=0, **dw))
    assert _name(row_desc(_lib, "post_op", groups=1)) == _name(row_desc(_lib, "post_op", reserved=0, groups=1)) == "dense_mfma_f16x1"
    d = row_desc(_lib, "post_op")
    io = _lib.ConvIo(x_codes=1, y_codes=1, y_ka=0.2, y_qbits=8)
    assert L.slfp_conv2d_codes_supported(ctypes.byref(d), ctypes.byref(io), 0, 0) == 0
    assert L.slfp_conv2d_bwd_kernel_name(ctypes.byref(d)).decode() == "composite"
    # both option bits together are fine; bits 2 and 4 stay unknown
    assert _name(row_desc(_lib, "post_op", reserved=BIT | _lib.DESC_DILATED_MFMA)) == "grouped_mfma_f16x1"
    ho, wo = ctypes.c_int64(), ctypes.c_int64()
    bad = row_desc(_lib, "post_op", reserved=BIT | 2)
    assert L.slfp_conv2d_out_shape(ctypes.byref(bad), ctypes.byref(ho), ctypes.byref(wo)) == _lib.ERR_BAD_ARG and _name(bad) == "invalid"


def test_the_option_is_validated_and_keys_the_plan():
    assert cf.options.grouped == "direct"
    with pytest.raises(ValueError):
        cf.options.grouped = "dense"
    mod = cf.conv2d_Q(8, 0.027, 0.21)(64, 64, 3, padding=1, groups=16)
    x = torch.empty((2, 64, 13, 19), device="meta")
    try:
        names = {}
        for mode in ("direct", "mfma"):
            cf.options.grouped = mode
            names[mode] = cf._plan(mod, x, mod.weight, True, True).kernel
    finally:
        cf.options.grouped = "direct"
    assert names == {"direct": "direct_nhwc", "mfma": "grouped_mfma_f16x1"} and len(mod._plans) == 2
