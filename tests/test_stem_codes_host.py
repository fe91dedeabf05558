"""CPU: the host side of the large-kernel image stems with code output: the `stem_mfma_*` family -- ResNet-50's
7x7 s2 3->64, SqueezeNet's 7x7 s2 3->96 + bias, AlexNet's 11x11 s4 3->64 + bias -- reads the float32 image and writes the 1-byte codes
of the layer behind it (slfp_conv2d_codes_supported with x_codes = 0, y_codes = 1; slfp_conv2d_fwd_codes[_ws]), and
fusion.link_stem / unlink_stem.  No device work is done here: every pointer handed to the library is refused before it would be
dereferenced."""
import ctypes

import pytest
import torch

from cnns_slfp_quantization_amd import _lib, fusion
from cnns_slfp_quantization_amd import conv2d_func as cf


def _desc(k, s, p, c_out, n=2, hw=224, qbits=8, passes=0, x_layout=_lib.LAYOUT_NHWC, y_layout=_lib.LAYOUT_NHWC):
    return _lib.ConvDesc(n=n, c_in=3, h=hw, w=hw, c_out=c_out, kh=k, kw=k, stride_h=s, stride_w=s, pad_h=p, pad_w=p,
                         dil_h=1, dil_w=1, groups=1, x_layout=x_layout, y_layout=y_layout, qbits=qbits,
                         ka=0.25, kw_scale=0.02, mfma_passes=passes, reserved=0)


def _io(x_codes=0, y_codes=1, y_qbits=8, y_ka=0.3):
    return _lib.ConvIo(x_codes=x_codes, y_codes=y_codes, y_ka=y_ka, y_qbits=y_qbits)


def _q(name, d, io, has_bias, relu, *tail):
    return getattr(_lib.load(), name)(ctypes.byref(d), ctypes.byref(io), has_bias, relu, *tail)


# (kernel, stride, padding, C_out, bias) of the three reference stems
STEMS = ((7, 2, 3, 64, 0), (7, 2, 0, 96, 1), (11, 4, 2, 64, 1))


@pytest.mark.parametrize("k, s, p, c_out, bias", STEMS)
def test_reference_stems_have_the_code_output_route(k, s, p, c_out, bias):
    L = _lib.load()
    for n in (1, 128):
        for qbits in (8, 7):
            d = _desc(k, s, p, c_out, n=n, qbits=qbits)
            assert L.slfp_conv2d_kernel_name(ctypes.byref(d)).decode().startswith("stem_mfma_")
            for y_qbits in (8, 7):
                for relu in (0, 1):
                    io = _io(0, 1, y_qbits)
                    assert _q("slfp_conv2d_codes_supported", d, io, bias, relu) == 1, (n, qbits, y_qbits, relu)
                    # no channel-slice store, no pointwise entry, no residual operand for a stem
                    assert _q("slfp_conv2d_codes_slice_supported", d, io, bias, relu, 2 * c_out) == 0
                    assert _q("slfp_conv2d_entry_supported", d, io, bias, relu) == 0
                    assert _q("slfp_conv2d_res_supported", d, io, bias, relu) == 0
                    assert _q("slfp_conv2d_res_supported", d, _io(0, 0), bias, relu) == 0


@pytest.mark.parametrize("c_out", (32, 48, 80))
def test_other_whole_tile_widths_are_taken(c_out):
    for qbits in (8, 7):
        assert _q("slfp_conv2d_codes_supported", _desc(7, 2, 3, c_out, qbits=qbits), _io(0, 1, qbits), 1, 1) == 1


def test_everything_else_is_refused():
    d = _desc(7, 2, 3, 64)
    assert _q("slfp_conv2d_codes_supported", d, _io(0, 1), 0, 1) == 1          # the control
    refused = [
        ("x_codes", d, _io(1, 1), 1),
        ("x_codes, float32 out", d, _io(1, 0), 1),
        ("float32 both sides", d, _io(0, 0), 1),
        ("c_out24", _desc(7, 2, 3, 24), _io(0, 1), 1),
        ("c_out68", _desc(7, 2, 3, 68), _io(0, 1), 1),
        ("y_qbits5", d, _io(0, 1, 5), 1),
        ("y_ka0", d, _io(0, 1, 8, 0.0), 1),
        ("y_ka<0", d, _io(0, 1, 8, -0.3), 1),
        ("nchw_in", _desc(7, 2, 3, 64, x_layout=_lib.LAYOUT_NCHW), _io(0, 1), 1),
        ("nchw_out", _desc(7, 2, 3, 64, y_layout=_lib.LAYOUT_NCHW), _io(0, 1), 1),
        ("layerout", d, _io(0, 1), 1 | 2),
        ("layerout alone", d, _io(0, 1), 2),
        ("f16x3", _desc(7, 2, 3, 64, passes=_lib.MFMA_F16X3), _io(0, 1), 1),
    ]
    for name, dd, io, relu in refused:
        for bias in (0, 1):
            assert _q("slfp_conv2d_codes_supported", dd, io, bias, relu) == 0, name
    # the three-pass mode at qbits 7 is the exact single pass: the same kernel, taken
    assert _q("slfp_conv2d_codes_supported", _desc(7, 2, 3, 64, qbits=7, passes=_lib.MFMA_F16X3), _io(0, 1), 0, 1) == 1


def test_argument_checks_never_touch_the_device():
    L = _lib.load()
    x, w, y, ws = 1 << 20, 1 << 30, 1 << 32, 1 << 34      # 16-byte aligned, never touched
    rows, two = _desc(7, 2, 3, 64), _desc(11, 4, 2, 64)
    io = _io(0, 1)
    assert L.slfp_conv2d_workspace_bytes(ctypes.byref(two)) > 0

    def codes(d, y=y, x=x):
        return L.slfp_conv2d_fwd_codes(ctypes.byref(d), ctypes.byref(io), x, w, None, None, None, 1, y, None)

    def codes_ws(d, ws, y=y):
        return L.slfp_conv2d_fwd_codes_ws(ctypes.byref(d), ctypes.byref(io), x, w, None, None, None, 1, y, ws, None)

    # the two-kernel form reads its im2row copy from the workspace: the status the dense route gives without one
    dense = _lib.ConvDesc(n=2, c_in=64, h=28, w=28, c_out=64, kh=3, kw=3, stride_h=1, stride_w=1, pad_h=1, pad_w=1, dil_h=1, dil_w=1,
                          groups=1, x_layout=_lib.LAYOUT_NHWC, y_layout=_lib.LAYOUT_NHWC, qbits=8, ka=0.25, kw_scale=0.02,
                          mfma_passes=0, reserved=0)
    missing = codes(dense)
    assert missing == _lib.ERR_BAD_ARG and "workspace" in _lib.last_error()
    assert codes(two) == missing and "workspace" in _lib.last_error()
    assert codes_ws(two, None) == missing and "workspace" in _lib.last_error()
    assert codes_ws(two, ws + 8) == missing and "workspace" in _lib.last_error()
    # 10x10 s1 2->96: tile + W fit the rows form's 64 KiB (64704 B), tile + W + the 2056-byte code table do not: the code form
    # falls to the two-kernel form and asks for the workspace
    edge = _lib.ConvDesc(n=1, c_in=2, h=20, w=23, c_out=96, kh=10, kw=10, stride_h=1, stride_w=1, pad_h=4, pad_w=4, dil_h=1, dil_w=1,
                         groups=1, x_layout=_lib.LAYOUT_NHWC, y_layout=_lib.LAYOUT_NHWC, qbits=8, ka=0.25, kw_scale=0.02,
                         mfma_passes=0, reserved=0)
    assert _q("slfp_conv2d_codes_supported", edge, io, 0, 1) == 1
    assert codes(edge) == missing and "workspace" in _lib.last_error()
    for d in (rows, two):
        assert codes_ws(d, ws, y=y + 8) == _lib.ERR_ALIGNMENT
        assert codes(d, y=y + 4) == _lib.ERR_ALIGNMENT
        assert codes(d, x=x + 4) == _lib.ERR_ALIGNMENT
        assert codes(d, y=None) == _lib.ERR_BAD_ARG
    # refused descriptors keep the unsupported status on the entry points
    assert codes(_desc(7, 2, 3, 24)) == _lib.ERR_UNSUPPORTED and "slfp_conv2d_codes_supported" in _lib.last_error()
    assert L.slfp_conv2d_fwd_entry(ctypes.byref(rows), ctypes.byref(io), x, w, None, None, None, 1, y, None) == _lib.ERR_UNSUPPORTED
    assert L.slfp_conv2d_fwd_codes_slice(ctypes.byref(rows), ctypes.byref(io), x, w, None, None, None, 1, y, 128, None,
                                         None) == _lib.ERR_UNSUPPORTED
    assert L.slfp_version() == 1   # SLFP_ABI_VERSION: no new export


def test_link_stem_exists_and_refuses_what_it_cannot_link():
    assert callable(fusion.link_stem) and callable(fusion.unlink_stem)
    x = torch.zeros(1, 3, 8, 8)
    no_conv = torch.nn.Sequential(torch.nn.ReLU(), torch.nn.MaxPool2d(3, 2)).eval()
    assert fusion.link_stem(no_conv, x) == 0 and fusion.unlink_stem(no_conv) == 0
    C = cf.conv2d_Q_bias(8, 0.02, 0.25)
    m = torch.nn.Sequential(C(3, 64, 7, 0.02, 0.25, 2, 3), torch.nn.ReLU(), C(64, 64, 1, 0.02, 0.3, 1, 0))
    m.train()
    assert fusion.link_stem(m, x) == 0 and fusion.unlink_stem(m) == 0   # inference only: refused before any forward runs
    assert m[0]._code_out is None and m[0]._post is None and not hasattr(m[0], "_pre_link_post")
    assert isinstance(m[1], torch.nn.ReLU)
