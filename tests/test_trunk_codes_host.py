"""CPU: the host side of the residual epilogue that also writes the next block's codes (DESIGN section 18;
slfp_conv2d_res_codes_supported / slfp_conv2d_fwd_res_codes), the module's `_trunk_code_out` attribute and fusion.link_trunk /
unlink_trunk.  No device work is done here: every pointer handed to the library is refused before it would be dereferenced."""
import ctypes
import os
import re

import torch

from cnns_slfp_quantization_amd import _lib, fusion
from cnns_slfp_quantization_amd import conv2d_func as cf

NEW = ("slfp_conv2d_res_codes_supported", "slfp_conv2d_fwd_res_codes")
OLD = ("slfp_conv2d_codes_supported", "slfp_conv2d_codes_slice_supported", "slfp_conv2d_entry_supported", "slfp_conv2d_res_supported")
# conv3 of the four ResNet-50 stages: (C_in, C_out, H = W)
CONV3 = ((64, 256, 56), (128, 512, 28), (256, 1024, 14), (512, 2048, 7))


def _desc(c_in=64, c_out=256, hw=56, n=2, k=1, s=1, p=0, groups=1, qbits=8, passes=0, x_layout=_lib.LAYOUT_NHWC,
          y_layout=_lib.LAYOUT_NHWC):
    return _lib.ConvDesc(n=n, c_in=c_in, h=hw, w=hw, c_out=c_out, kh=k, kw=k, stride_h=s, stride_w=s, pad_h=p, pad_w=p,
                         dil_h=1, dil_w=1, groups=groups, x_layout=x_layout, y_layout=y_layout, qbits=qbits,
                         ka=0.14, kw_scale=0.0196, mfma_passes=passes, reserved=0)


def _io(x_codes=1, y_codes=1, y_qbits=8, y_ka=0.3):
    return _lib.ConvIo(x_codes=x_codes, y_codes=y_codes, y_ka=y_ka, y_qbits=y_qbits)


def _q(name, d, io, has_bias, relu, *tail):
    return getattr(_lib.load(), name)(ctypes.byref(d), ctypes.byref(io), has_bias, relu, *tail)


def _new(d, io, has_bias=0, relu=1):
    return _q(NEW[0], d, io, has_bias, relu)


# (name, descriptor, io, relu) of everything the new query refuses
def _refused():
    d = _desc()
    return [
        ("x_codes0", d, _io(0, 1), 1),
        ("y_codes0", d, _io(1, 0), 1),
        ("float32 both sides", d, _io(0, 0), 1),
        ("c_out24", _desc(c_out=24), _io(), 1),
        ("c_out68", _desc(c_out=68), _io(), 1),
        ("y_qbits5", d, _io(1, 1, 5), 1),
        ("y_ka0", d, _io(1, 1, 8, 0.0), 1),
        ("y_ka<0", d, _io(1, 1, 8, -0.3), 1),
        ("nchw_in", _desc(x_layout=_lib.LAYOUT_NCHW), _io(), 1),
        ("nchw_out", _desc(y_layout=_lib.LAYOUT_NCHW), _io(), 1),
        ("stride2", _desc(c_in=256, c_out=512, s=2), _io(), 1),
        ("3x3", _desc(c_in=64, c_out=64, k=3, p=1), _io(), 1),
        ("depthwise", _desc(c_in=64, c_out=64, k=3, p=1, groups=64), _io(), 1),
        ("stem", _desc(c_in=3, c_out=64, hw=224, k=7, s=2, p=3), _io(), 1),
        ("stem, float32 in", _desc(c_in=3, c_out=64, hw=224, k=7, s=2, p=3), _io(0, 1), 1),
        ("layerout", d, _io(), 1 | 2),
        ("layerout alone", d, _io(), 2),
        ("f16x3 at qbits 8", _desc(passes=_lib.MFMA_F16X3), _io(), 1),
    ]


def test_symbols_are_exported_and_declared():
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "slfp.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert hasattr(L, name)
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert L.slfp_version() == 1   # SLFP_ABI_VERSION stays
    assert cf._KINDS["res_codes"] == NEW and cf._KINDS["res"] == ("slfp_conv2d_res_supported", "slfp_conv2d_fwd_res")


def test_the_four_conv3_geometries_are_taken():
    for c_in, c_out, hw in CONV3:
        for n in (1, 4, 128):
            for qbits in (8, 7):
                for y_qbits in (8, 7):
                    for relu in (0, 1):
                        for bias in (0, 1):
                            d = _desc(c_in, c_out, hw, n=n, qbits=qbits)
                            assert _new(d, _io(1, 1, y_qbits), bias, relu) == 1, (c_in, n, qbits, y_qbits, relu, bias)
    # the three-pass mode at qbits 7 is the exact single pass: the same kernel, taken
    assert _new(_desc(qbits=7, passes=_lib.MFMA_F16X3), _io()) == 1
    # exactly where the residual route takes the layer on codes with float32 out
    for c_out in (16, 48, 80, 528):
        d = _desc(c_in=128, c_out=c_out, hw=7)
        assert _q("slfp_conv2d_res_supported", d, _io(1, 0), 0, 1) == 1 and _new(d, _io()) == 1, c_out


def test_everything_else_is_refused_by_the_query_and_by_the_entry_point():
    L = _lib.load()
    assert _new(_desc(), _io()) == 1   # the control
    x, w, y = 1 << 20, 1 << 30, 1 << 32                      # 16-byte aligned, far apart, never touched
    res, yc = 1 << 34, 1 << 36
    for name, d, io, relu in _refused():
        for bias in (0, 1):
            assert _new(d, io, bias, relu) == 0, name
        rc = L.slfp_conv2d_fwd_res_codes(ctypes.byref(d), ctypes.byref(io), x, w, None, None, None, relu, res, y, yc, None, None)
        assert rc == _lib.ERR_UNSUPPORTED, (name, rc, _lib.last_error())
        assert NEW[0] in _lib.last_error(), name
    assert L.slfp_conv2d_res_codes_supported(None, ctypes.byref(_io()), 0, 1) == 0
    assert L.slfp_conv2d_res_codes_supported(ctypes.byref(_desc()), None, 0, 1) == 0


def test_the_existing_queries_answer_what_they_answered():
    """For the descriptors above, the four queries that existed before: recorded from the parent's answers -- slfp_conv2d_res_supported
    keeps refusing y_codes with a residual, and no query gained or lost a layer."""
    d = _desc()
    for bias in (0, 1):
        for relu in (0, 1):
            assert _q("slfp_conv2d_res_supported", d, _io(1, 1), bias, relu) == 0
            assert _q("slfp_conv2d_res_supported", d, _io(0, 1), bias, relu) == 0
            assert _q("slfp_conv2d_res_supported", d, _io(1, 0), bias, relu) == 1
            assert _q("slfp_conv2d_res_supported", d, _io(0, 0), bias, relu) == 1
            assert _q("slfp_conv2d_codes_supported", d, _io(1, 1), bias, relu) == 1
            assert _q("slfp_conv2d_codes_supported", d, _io(1, 0), bias, relu) == 1
            assert _q("slfp_conv2d_codes_supported", d, _io(0, 1), bias, relu) == 0
            assert _q("slfp_conv2d_entry_supported", d, _io(0, 1), bias, relu) == 1
            assert _q("slfp_conv2d_entry_supported", d, _io(1, 1), bias, relu) == 0
            assert _q("slfp_conv2d_codes_slice_supported", d, _io(1, 1), bias, relu, 512) == 1
    # name -> (codes, slice at y_ld = 2048, entry, res) of the refused descriptors with their own io
    want = {
        "x_codes0": (0, 0, 1, 0), "y_codes0": (1, 0, 0, 1), "float32 both sides": (0, 0, 0, 1),
        "c_out24": (0, 0, 0, 0), "c_out68": (0, 0, 0, 0), "y_qbits5": (0, 0, 0, 0), "y_ka0": (0, 0, 0, 0), "y_ka<0": (0, 0, 0, 0),
        "nchw_in": (0, 0, 0, 0), "nchw_out": (0, 0, 0, 0), "stride2": (1, 1, 0, 0), "3x3": (1, 1, 0, 0), "depthwise": (1, 0, 0, 0),
        "stem": (0, 0, 0, 0), "stem, float32 in": (1, 0, 0, 0), "layerout": (0, 0, 0, 0), "layerout alone": (0, 0, 0, 0),
        "f16x3 at qbits 8": (0, 0, 0, 0),
    }
    for name, dd, io, relu in _refused():
        got = (_q(OLD[0], dd, io, 0, relu), _q(OLD[1], dd, io, 0, relu, 2048), _q(OLD[2], dd, io, 0, relu), _q(OLD[3], dd, io, 0, relu))
        assert got == want[name], (name, got)


def test_argument_checks_never_touch_the_device():
    L = _lib.load()
    d, io = _desc(), _io()
    nbytes = 2 * 256 * 56 * 56 * 4
    x, w, y = 1 << 20, 1 << 30, 1 << 32
    res, yc = y + 2 * nbytes, y + 4 * nbytes

    def call(d=d, io=io, x=x, w=w, relu=1, res=res, y=y, yc=yc, ps=None, psh=None):
        return L.slfp_conv2d_fwd_res_codes(ctypes.byref(d) if d is not None else None, ctypes.byref(io) if io is not None else None,
                                           x, w, None, ps, psh, relu, res, y, yc, None, None)

    # what slfp_conv2d_fwd_res checks, in its order
    assert call(d=None) == _lib.ERR_BAD_ARG
    assert call(io=None) == _lib.ERR_BAD_ARG
    for k in ("x", "w", "y", "res", "yc"):
        assert call(**{k: None}) == _lib.ERR_BAD_ARG, k
        assert "null pointer" in _lib.last_error()
    assert call(ps=1 << 21) == _lib.ERR_BAD_ARG
    assert call(res=res + 4) == _lib.ERR_ALIGNMENT
    assert call(y=y + 8) == _lib.ERR_ALIGNMENT
    assert call(res=y) == _lib.ERR_BAD_ARG and "res and y overlap" in _lib.last_error()
    # the second output: non-null (above), 16-byte aligned, outside y and res
    for off in (1, 4, 8):
        assert call(yc=yc + off) == _lib.ERR_ALIGNMENT, off
        assert "y_codes" in _lib.last_error()
    for bad in (y, y + nbytes - 16, y - nbytes // 4 + 16, res, res + nbytes - 16, res - nbytes // 4 + 16):
        assert call(yc=bad) == _lib.ERR_BAD_ARG, bad
        assert "y_codes overlaps" in _lib.last_error()
    # adjacent is not overlapping: the statuses of the checks behind it (a descriptor the route refuses)
    assert call(yc=y + nbytes, io=_io(1, 0)) == _lib.ERR_UNSUPPORTED
    assert call(yc=y - nbytes // 4, io=_io(1, 0)) == _lib.ERR_UNSUPPORTED
    # a defect in the arguments comes before the refusal of the route
    assert call(io=_io(0, 1), yc=yc + 4) == _lib.ERR_ALIGNMENT
    assert call(io=_io(0, 1), yc=None) == _lib.ERR_BAD_ARG
    bad = _desc()
    bad.n = 0
    assert call(d=bad) == _lib.ERR_SHAPE
    bad = _desc()
    bad.qbits = 5
    assert call(d=bad) == _lib.ERR_BAD_ARG


def test_module_attribute_and_link_trunk_defaults():
    for factory in (cf.conv2d_Q, cf.conv2d_Q_bias):
        m = factory(8, 0.1, 0.2)(8, 8, 1)
        assert m._trunk_code_out is None and m._code_out is None
    assert callable(fusion.link_trunk) and callable(fusion.unlink_trunk)
    x = torch.zeros(1, 3, 8, 8)
    no_conv = torch.nn.Sequential(torch.nn.ReLU(), torch.nn.MaxPool2d(3, 2)).eval()
    assert fusion.link_trunk(no_conv, x) == 0 and fusion.unlink_trunk(no_conv) == 0
    # nothing fused: nothing to link, refused before any forward runs
    C = cf.conv2d_Q_bias(8, 0.02, 0.25)
    m = torch.nn.Sequential(C(3, 64, 7, 0.02, 0.25, 2, 3), torch.nn.ReLU(), C(64, 64, 1, 0.02, 0.3, 1, 0)).eval()
    assert fusion.link_trunk(m, x) == 0 and fusion.unlink_trunk(m) == 0 and fusion.unlink_codes(m) == 0
    assert all(c._trunk_code_out is None and "_trunk_link" not in c.__dict__ for c in (m[0], m[2]))
