"""CPU: the host side of the residual epilogue (slfp_conv2d_res_supported / slfp_conv2d_fwd_res): which layers it covers,
its argument checks, and the `residual=` keyword of Conv2d_Q.forward.  No device work is done here."""
import ctypes
import inspect
import os
import re

from cnns_slfp_quantization_amd import _lib, layer_specs
from cnns_slfp_quantization_amd import conv2d_func as cf

NET = "resnet50_imagenet224"


def _desc(spec, n=2, x_layout=_lib.LAYOUT_NHWC, y_layout=_lib.LAYOUT_NHWC, qbits=8, passes=0):
    return _lib.ConvDesc(n=n, c_in=spec.c_in, h=spec.h, w=spec.w, c_out=spec.c_out, kh=spec.k[0], kw=spec.k[1],
                         stride_h=spec.stride[0], stride_w=spec.stride[1], pad_h=spec.pad[0], pad_w=spec.pad[1],
                         dil_h=1, dil_w=1, groups=spec.groups, x_layout=x_layout, y_layout=y_layout, qbits=qbits,
                         ka=float(spec.Ka), kw_scale=float(spec.Kw), mfma_passes=passes, reserved=0)


def _io(x_codes=0, y_codes=0):
    return _lib.ConvIo(x_codes=x_codes, y_codes=y_codes, y_ka=0.25, y_qbits=8)


def _supported(d, io, has_bias=0, relu=1):
    return _lib.load().slfp_conv2d_res_supported(ctypes.byref(d), ctypes.byref(io), has_bias, relu)


def _is_pw1(s):
    return s.k == (1, 1) and s.stride == (1, 1) and s.pad == (0, 0) and s.groups == 1


def test_symbols_are_exported_and_declared():
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "slfp.h")).read()
    for name in ("slfp_conv2d_res_supported", "slfp_conv2d_fwd_res"):
        assert name in _lib.SYMBOLS
        assert hasattr(L, name)
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert L.slfp_version() == 1   # SLFP_ABI_VERSION: two new exports, no change to an existing one
    assert ctypes.sizeof(_lib.ConvIo) == 16


def test_every_stride1_pointwise_layer_of_resnet50_is_supported():
    pw = [s for s in layer_specs.conv_layers(NET) if _is_pw1(s)]
    last = [s for s in pw if s.c_out == 4 * s.c_in]
    # the specs carry no names: count.  The 16 Bottlenecks' conv3 (3 + 4 + 6 + 3) and layer1's downsample, which is a 64 -> 256
    # layer of stride 1 as well (layer1 does not stride; the other three downsample layers do and are refused below)
    from collections import Counter
    assert Counter((s.c_in, s.c_out, s.h) for s in last) == {(64, 256, 56): 3 + 1, (128, 512, 28): 4, (256, 1024, 14): 6, (512, 2048, 7): 3}
    assert len(last) == 16 + 1
    for s in pw:
        for n in (4, 64, 128):
            for qbits in (8, 7):
                for relu in (0, 1):
                    assert _supported(_desc(s, n=n, qbits=qbits), _io(0), relu=relu) == 1, (s, n, qbits, relu)
                    assert _supported(_desc(s, n=n, qbits=qbits), _io(1), relu=relu) == 1, (s, n, qbits, relu)
            assert _supported(_desc(s, n=n, passes=_lib.MFMA_F16X3), _io(0)) == 1, (s, n)   # float32-equivalent mode, float32 in
            assert _supported(_desc(s, n=n), _io(0), has_bias=1) == 1, (s, n)


def test_everything_else_is_refused():
    layers = layer_specs.conv_layers(NET)
    others = [s for s in layers if not _is_pw1(s)]
    assert any(s.k == (3, 3) for s in others) and any(s.k == (7, 7) for s in others)   # 3x3 layers and the stem
    assert sum(1 for s in others if s.k == (1, 1) and s.stride == (2, 2)) >= 3          # strided downsample layers
    for s in others:
        for x_codes in (0, 1):
            assert _supported(_desc(s), _io(x_codes)) == 0, s
    s = next(s for s in layers if _is_pw1(s) and s.c_out == 4 * s.c_in)
    assert _supported(_desc(s), _io(0)) == 1
    assert _supported(_desc(s, x_layout=_lib.LAYOUT_NCHW), _io(0)) == 0
    assert _supported(_desc(s, y_layout=_lib.LAYOUT_NCHW), _io(0)) == 0
    assert _supported(_desc(s, x_layout=_lib.LAYOUT_NCHW, y_layout=_lib.LAYOUT_NCHW), _io(1)) == 0
    assert _supported(_desc(s), _io(0, y_codes=1)) == 0
    assert _supported(_desc(s), _io(1, y_codes=1)) == 0
    assert _supported(_desc(s), _io(0), relu=2) == 0      # SLFP_POST_LAYEROUT
    assert _supported(_desc(s), _io(0), relu=3) == 0
    assert _supported(_desc(s, passes=_lib.MFMA_F16X3), _io(1)) == 0   # code input exists in the single-pass mode only
    # a 58-channel layer (ShuffleNetV2's branches): the 8-byte forms of the stream kernel have no residual variant
    s58 = next(s for s in layer_specs.conv_layers("shufflenetv2_224") if _is_pw1(s) and s.c_in == 58 and s.c_out == 58)
    assert _supported(_desc(s58), _io(0)) == 0 and _supported(_desc(s58), _io(1)) == 0
    L = _lib.load()
    assert L.slfp_conv2d_res_supported(None, ctypes.byref(_io(0)), 0, 1) == 0
    assert L.slfp_conv2d_res_supported(ctypes.byref(_desc(s)), None, 0, 1) == 0


def test_bad_arguments_return_error_codes():
    """Every check that precedes device work: no pointer here is dereferenced."""
    L = _lib.load()
    layers = layer_specs.conv_layers(NET)
    s = next(s for s in layers if _is_pw1(s) and s.c_out == 4 * s.c_in)
    d, io = _desc(s), _io(0)
    nbytes = 2 * s.c_out * s.h_out * s.w_out * 4
    x, w, y = 1 << 20, 1 << 30, 1 << 32                              # 16-byte aligned, never touched
    res = y + 2 * nbytes

    def call(d=d, io=io, x=x, w=w, relu=1, res=res, y=y):
        return L.slfp_conv2d_fwd_res(ctypes.byref(d) if d is not None else None, ctypes.byref(io) if io is not None else None,
                                     x, w, None, None, None, relu, res, y, None, None)

    assert call(d=None) == _lib.ERR_BAD_ARG
    assert call(io=None) == _lib.ERR_BAD_ARG
    assert call(res=None) == _lib.ERR_BAD_ARG
    assert call(x=None) == _lib.ERR_BAD_ARG
    assert call(y=None) == _lib.ERR_BAD_ARG
    assert call(res=res + 4) == _lib.ERR_ALIGNMENT
    assert call(y=y + 8) == _lib.ERR_ALIGNMENT
    assert call(res=y) == _lib.ERR_BAD_ARG                           # in place
    assert "overlap" in _lib.last_error()
    assert call(res=y + nbytes - 16) == _lib.ERR_BAD_ARG             # partial overlap, either side
    assert call(res=y - nbytes + 16) == _lib.ERR_BAD_ARG
    fake = 1 << 21
    assert L.slfp_conv2d_fwd_res(ctypes.byref(d), ctypes.byref(io), x, w, None, fake, None, 1, res, y, None, None) == _lib.ERR_BAD_ARG
    assert call(relu=2) == _lib.ERR_UNSUPPORTED                      # SLFP_POST_LAYEROUT
    assert call(io=_io(0, y_codes=1)) == _lib.ERR_UNSUPPORTED
    assert call(d=_desc(s, x_layout=_lib.LAYOUT_NCHW)) == _lib.ERR_UNSUPPORTED
    s3 = next(s for s in layers if s.k == (3, 3))
    assert call(d=_desc(s3)) == _lib.ERR_UNSUPPORTED                 # a dense 3x3 layer
    assert "slfp_conv2d_res_supported" in _lib.last_error()
    sd = next(s for s in layers if s.k == (1, 1) and s.stride == (2, 2))
    assert call(d=_desc(sd)) == _lib.ERR_UNSUPPORTED                 # a strided downsample layer
    bad = _desc(s)
    bad.n = 0
    assert call(d=bad) == _lib.ERR_SHAPE
    bad = _desc(s)
    bad.qbits = 5
    assert call(d=bad) == _lib.ERR_BAD_ARG


def test_residual_is_a_keyword_only_argument_of_forward():
    for factory in (cf.conv2d_Q, cf.conv2d_Q_bias):
        m = factory(8, 0.1, 0.2)(8, 8, 1)
        sig = inspect.signature(m.forward)
        params = list(sig.parameters.values())
        assert [p.name for p in params] == ["input", "order", "residual"]
        assert params[0].kind == params[1].kind == inspect.Parameter.POSITIONAL_OR_KEYWORD   # the reference's surface
        assert params[1].default is None
        assert params[2].kind == inspect.Parameter.KEYWORD_ONLY and params[2].default is None
        assert m.residual_relu is False
    from cnns_slfp_quantization_amd import fusion
    assert callable(fusion.fuse_residual) and callable(fusion.unfuse_residual)
