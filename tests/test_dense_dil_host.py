"""Host side of the opt-in dilated dense family (csrc/conv_dense_dil.hip; SLFP_DESC_DILATED_MFMA in the descriptor's `reserved`
word; conv2d_func.options.dilated): what plans onto it, what stays where it was, and that the option reaches the plan key.
No device is touched."""
import ctypes

import pytest
import torch

from cnns_slfp_quantization_amd import _lib, conv2d_func as cf

BIT = _lib.DESC_DILATED_MFMA


def _desc(reserved=BIT, **kw):
    f = dict(n=2, c_in=64, h=13, w=19, c_out=32, kh=3, kw=3, stride_h=1, stride_w=1, pad_h=2, pad_w=2, dil_h=2, dil_w=2, groups=1,
             x_layout=_lib.LAYOUT_NHWC, y_layout=_lib.LAYOUT_NHWC, qbits=8, ka=0.21, kw_scale=0.027, mfma_passes=0, reserved=reserved)
    f.update(kw)
    return _lib.ConvDesc(**f)


def _name(d):
    return _lib.load().slfp_conv2d_kernel_name(ctypes.byref(d)).decode()


def _sizes(d):
    L = _lib.load()
    return L.slfp_conv2d_wprep_bytes(ctypes.byref(d)), L.slfp_conv2d_workspace_bytes(ctypes.byref(d))


def test_the_bit_plans_a_dilated_layer_onto_the_phase_tiled_kernel():
    assert _name(_desc()) == "dense_dil_mfma_f16x1"
    assert _name(_desc(qbits=7)) == "dense_dil_mfma_f16_exact"
    undilated = _desc(0, dil_h=1, dil_w=1, pad_h=1, pad_w=1)
    assert _name(undilated) == "dense_mfma_f16x1"
    assert _sizes(_desc()) == _sizes(undilated) and _sizes(_desc())[0] > 0
    assert _lib.load().slfp_debug_dense_dil_variant(ctypes.byref(_desc())).decode() == "16x1/811/ns3"
    # NCHW on either side is the entry point's transpose, as for every family
    assert _name(_desc(x_layout=_lib.LAYOUT_NCHW, y_layout=_lib.LAYOUT_NCHW)) == "dense_dil_mfma_f16x1"


@pytest.mark.parametrize("change", [dict(stride_h=2, stride_w=2), dict(groups=2), dict(c_in=8), dict(mfma_passes=_lib.MFMA_F16X3)],
                         ids=["stride2", "groups2", "c_in8", "f16x3"])
def test_what_the_kernel_refuses_stays_on_the_direct_kernel(change):
    d = _desc(**change)
    assert _name(d) == "direct_nhwc"
    assert _sizes(d) == _sizes(_desc(0, **change))
    assert _lib.load().slfp_debug_dense_dil_variant(ctypes.byref(d)).decode() == "none"


def test_the_bit_changes_nothing_else():
    L = _lib.load()
    for kw in (dict(dil_h=1, dil_w=1, pad_h=1, pad_w=1), dict(kh=1, kw=1, pad_h=0, pad_w=0, dil_h=1, dil_w=1)):
        assert _name(_desc(BIT, **kw)) == _name(_desc(0, **kw)) and _sizes(_desc(BIT, **kw)) == _sizes(_desc(0, **kw)), kw
    # bit clear: today's plan; the code queries and the backward do not know the family
    assert _name(_desc(0)) == "direct_nhwc"
    io = _lib.ConvIo(x_codes=1, y_codes=1, y_ka=0.2, y_qbits=8)
    assert L.slfp_conv2d_codes_supported(ctypes.byref(_desc()), ctypes.byref(io), 0, 0) == 0
    assert L.slfp_conv2d_bwd_kernel_name(ctypes.byref(_desc())).decode() == "composite"


def test_an_unknown_reserved_bit_is_a_bad_argument():
    L = _lib.load()
    ho, wo = ctypes.c_int64(), ctypes.c_int64()
    for reserved in (2, BIT | 4, -1):
        assert L.slfp_conv2d_out_shape(ctypes.byref(_desc(reserved)), ctypes.byref(ho), ctypes.byref(wo)) == _lib.ERR_BAD_ARG
        assert _name(_desc(reserved)) == "invalid"


def test_the_option_is_validated_and_keys_the_plan():
    assert cf.options.dilated == "direct"
    with pytest.raises(ValueError):
        cf.options.dilated = "wide_halo"
    mod = cf.conv2d_Q(8, 0.027, 0.21)(64, 32, 3, padding=2, dilation=2)
    x = torch.empty((2, 64, 13, 19), device="meta")
    try:
        names = {}
        for mode in ("direct", "mfma"):
            cf.options.dilated = mode
            names[mode] = cf._plan(mod, x, mod.weight, True, True).kernel
    finally:
        cf.options.dilated = "direct"
    assert names == {"direct": "direct_nhwc", "mfma": "dense_dil_mfma_f16x1"} and len(mod._plans) == 2
