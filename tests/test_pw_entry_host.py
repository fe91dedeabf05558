"""CPU: the host side of the pointwise entry layer: a 1x1 layer that reads float32 and writes 1-byte codes
(slfp_conv2d_entry_supported / slfp_conv2d_fwd_entry), the module's `_code_entry` attribute and the `entries=` switch of
fusion.link_codes_traced / fusion.fuse_fire.  No device work is done here: every pointer handed to the library is refused
before it would be dereferenced."""
import ctypes
import inspect
import os
import re

from cnns_slfp_quantization_amd import _lib, fusion, layer_specs
from cnns_slfp_quantization_amd import conv2d_func as cf

NEW = ("slfp_conv2d_entry_supported", "slfp_conv2d_fwd_entry")


def _desc(c_in, c_out, h, k=1, pad=0, n=2, qbits=8, groups=1, stride=1, passes=0, x_layout=_lib.LAYOUT_NHWC,
          y_layout=_lib.LAYOUT_NHWC):
    return _lib.ConvDesc(n=n, c_in=c_in, h=h, w=h, c_out=c_out, kh=k, kw=k, stride_h=stride, stride_w=stride, pad_h=pad, pad_w=pad,
                         dil_h=1, dil_w=1, groups=groups, x_layout=x_layout, y_layout=y_layout, qbits=qbits,
                         ka=0.25, kw_scale=0.02, mfma_passes=passes, reserved=0)


def _spec_desc(s, n=2, qbits=8):
    return _lib.ConvDesc(n=n, c_in=s.c_in, h=s.h, w=s.w, c_out=s.c_out, kh=s.k[0], kw=s.k[1], stride_h=s.stride[0],
                         stride_w=s.stride[1], pad_h=s.pad[0], pad_w=s.pad[1], dil_h=1, dil_w=1, groups=s.groups,
                         x_layout=_lib.LAYOUT_NHWC, y_layout=_lib.LAYOUT_NHWC, qbits=qbits, ka=float(s.Ka), kw_scale=float(s.Kw),
                         mfma_passes=0, reserved=0)


def _io(x_codes=0, y_codes=1, y_qbits=8, y_ka=0.3):
    return _lib.ConvIo(x_codes=x_codes, y_codes=y_codes, y_ka=y_ka, y_qbits=y_qbits)


def _entry(d, io, has_bias=1, relu=1):
    return _lib.load().slfp_conv2d_entry_supported(ctypes.byref(d) if d is not None else None,
                                                   ctypes.byref(io) if io is not None else None, has_bias, relu)


def test_new_symbols_are_exported_and_declared():
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "slfp.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert hasattr(L, name)
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert L.slfp_version() == 1   # SLFP_ABI_VERSION: new exports only


def _entry_layers():
    """Every stride-1 1x1 layer of ResNet-50 with C_out a multiple of 16 (all 16 conv1 layers among them) and SqueezeNet's
    96 -> 16 squeeze behind the stem."""
    res = [s for s in layer_specs.conv_layers("resnet50_imagenet224")
           if tuple(s.k) == (1, 1) and tuple(s.stride) == (1, 1) and s.groups == 1 and s.c_out % 16 == 0]
    have = {(s.c_in, s.c_out, s.h) for s in res}
    for g in ((64, 64, 56), (256, 64, 56), (256, 128, 56), (512, 128, 28), (512, 256, 28), (1024, 256, 14), (1024, 512, 14),
              (2048, 512, 7)):   # the distinct conv1 geometries of the 16 Bottlenecks
        assert g in have, g
    assert len(res) >= 16 + 16   # conv1 and conv3 of the 16 blocks at the least
    sq = layer_specs.conv_layers("squeezenet1_0_imagenet224")[1]
    assert (sq.c_in, sq.c_out) == (96, 16)
    return res + [sq]


def test_entry_supported_on_resnet50_pointwise_layers_and_the_first_squeeze():
    for s in _entry_layers():
        for qbits in (8, 7):
            for relu in (0, 1):
                for has_bias in (0, 1):
                    for n in (1, 128):
                        d = _spec_desc(s, n=n, qbits=qbits)
                        assert _entry(d, _io(0, 1, qbits), has_bias, relu) == 1, (s.c_in, s.c_out, s.h, qbits, relu, has_bias, n)


def _refused():
    return [
        ("x_codes", _desc(64, 64, 56), _io(1, 1)),
        ("y_codes0", _desc(64, 64, 56), _io(0, 0)),
        ("y_qbits5", _desc(64, 64, 56), _io(0, 1, 5)),
        ("y_ka0", _desc(64, 64, 56), _io(0, 1, 8, 0.0)),
        ("y_ka<0", _desc(64, 64, 56), _io(0, 1, 8, -0.3)),
        ("f16x3", _desc(64, 64, 56, passes=_lib.MFMA_F16X3), _io(0, 1)),
        ("nchw_in", _desc(64, 64, 56, x_layout=_lib.LAYOUT_NCHW), _io(0, 1)),
        ("nchw_out", _desc(64, 64, 56, y_layout=_lib.LAYOUT_NCHW), _io(0, 1)),
        ("c_out58", _desc(58, 58, 28), _io(0, 1)),
        ("c_out24", _desc(64, 24, 28), _io(0, 1)),
        ("3x3", _desc(64, 64, 56, k=3, pad=1), _io(0, 1)),
        ("depthwise", _desc(64, 64, 56, k=3, pad=1, groups=64), _io(0, 1)),
    ]


def test_entry_refuses_everything_else():
    for name, d, io in _refused():
        for relu in (0, 1):
            assert _entry(d, io, 1, relu) == 0, (name, relu)
    d = _desc(64, 64, 56)
    assert _entry(d, _io(0, 1), 1, 1) == 1                      # the control: the same layer, plain
    assert _entry(d, _io(0, 1), 1, 1 | 2) == 0                   # SLFP_POST_LAYEROUT
    assert _entry(d, _io(0, 1), 1, 2) == 0
    assert _entry(None, _io(0, 1)) == 0                          # null descriptor
    assert _entry(d, None) == 0


def test_the_code_queries_keep_refusing_float32_in_codes_out():
    """slfp_conv2d_codes_supported / _slice_supported still say no where the entry query says yes: link_codes_traced(...) == 16 on
    ResNet-50 rests on it."""
    L = _lib.load()
    for s in _entry_layers():
        for qbits in (8, 7):
            d, io = _spec_desc(s, qbits=qbits), _io(0, 1, qbits)
            assert L.slfp_conv2d_codes_supported(ctypes.byref(d), ctypes.byref(io), 1, 1) == 0, (s.c_in, s.c_out)
            assert L.slfp_conv2d_codes_slice_supported(ctypes.byref(d), ctypes.byref(io), 1, 1, 2 * s.c_out) == 0, (s.c_in, s.c_out)
    for name, d, _ in _refused():
        if name in ("3x3",):
            continue   # dense k x k layers start a chain through slfp_conv2d_fwd_codes_ws (x_codes = 0, y_codes = 1): not this query's ground
        io = _io(0, 1)
        assert L.slfp_conv2d_codes_supported(ctypes.byref(d), ctypes.byref(io), 1, 1) == 0, name
        assert L.slfp_conv2d_codes_slice_supported(ctypes.byref(d), ctypes.byref(io), 1, 1, 128) == 0, name
    d, io = _desc(64, 64, 56), _io(0, 1)
    x, w, y = 1 << 20, 1 << 30, 1 << 32
    assert L.slfp_conv2d_fwd_codes(ctypes.byref(d), ctypes.byref(io), x, w, None, None, None, 1, y, None) == _lib.ERR_UNSUPPORTED
    assert L.slfp_conv2d_fwd_codes_ws(ctypes.byref(d), ctypes.byref(io), x, w, None, None, None, 1, y, None, None) == _lib.ERR_UNSUPPORTED
    assert L.slfp_conv2d_fwd_codes_slice(ctypes.byref(d), ctypes.byref(io), x, w, None, None, None, 1, y, 128, None, None) == _lib.ERR_UNSUPPORTED


def test_fwd_entry_argument_checks_return_error_codes():
    """Every check that precedes device work: no pointer here is dereferenced."""
    L = _lib.load()
    x, w, y, v = 1 << 20, 1 << 30, 1 << 32, 1 << 34      # 16-byte aligned, never touched

    def call(d=None, io=None, x=x, w=w, y=y, ps=None, psh=None, relu=1):
        d = _desc(64, 64, 56) if d is None else d
        io = _io(0, 1) if io is None else io
        return L.slfp_conv2d_fwd_entry(ctypes.byref(d) if d is not False else None, ctypes.byref(io) if io is not False else None,
                                       x, w, None, ps, psh, relu, y, None)

    assert call(d=False) == _lib.ERR_BAD_ARG
    assert call(io=False) == _lib.ERR_BAD_ARG
    assert call(x=None) == _lib.ERR_BAD_ARG
    assert call(w=None) == _lib.ERR_BAD_ARG
    assert call(y=None) == _lib.ERR_BAD_ARG
    assert call(ps=v) == _lib.ERR_BAD_ARG and "post_scale" in _lib.last_error()    # a lone post_scale
    assert call(psh=v) == _lib.ERR_BAD_ARG
    assert call(x=x + 4) == _lib.ERR_ALIGNMENT
    assert call(y=y + 8) == _lib.ERR_ALIGNMENT
    assert call(ps=v + 4, psh=v) == _lib.ERR_ALIGNMENT
    assert call(d=_desc(64, 64, 56, passes=_lib.MFMA_F16X3)) == _lib.ERR_UNSUPPORTED     # three-pass mode
    assert "slfp_conv2d_entry_supported" in _lib.last_error()
    assert call(d=_desc(64, 24, 28)) == _lib.ERR_UNSUPPORTED and "slfp_conv2d_entry_supported" in _lib.last_error()
    assert call(relu=1 | 2, ps=v, psh=v) == _lib.ERR_UNSUPPORTED                          # SLFP_POST_LAYEROUT
    for io in (_io(1, 1), _io(0, 0), _io(0, 1, 5), _io(0, 1, 8, 0.0)):
        assert call(io=io) in (_lib.ERR_BAD_ARG, _lib.ERR_UNSUPPORTED)
        assert "slfp_conv2d_entry_supported" in _lib.last_error()
    bad = _desc(64, 64, 56)
    bad.n = 0
    assert call(d=bad) == _lib.ERR_SHAPE


def test_module_and_fusion_defaults():
    m = cf.conv2d_Q_bias(8, 0.02, 0.25)(64, 64, 1)
    assert m._code_entry is False and m._code_out is None
    for fn in (fusion.link_codes_traced, fusion.fuse_fire):
        p = inspect.signature(fn).parameters
        assert "entries" in p and p["entries"].default is False, fn.__name__
    assert fusion.unlink_codes(m) == 0 and m._code_entry is False
