"""CPU: the host side of the Fire-module code path: the channel-slice code output
(slfp_conv2d_codes_slice_supported / slfp_conv2d_fwd_codes_slice), 1x1 layers on codes with 16 and 48 input channels, the
ceil-mode code pool (slfp_maxpool2d_codes_ex / slfp_maxpool2d_out_shape) and Conv2d_Q.forward_slice.  No device work is done
here: every pointer handed to the library is refused before it would be dereferenced."""
import ctypes
import inspect
import os
import re

import pytest

from cnns_slfp_quantization_amd import _lib, layer_specs
from cnns_slfp_quantization_amd import conv2d_func as cf

NET = "squeezenet1_0_imagenet224"
NEW = ("slfp_conv2d_codes_slice_supported", "slfp_conv2d_fwd_codes_slice", "slfp_maxpool2d_codes_ex", "slfp_maxpool2d_out_shape")


def _desc(c_in, c_out, h, k=1, pad=0, n=2, qbits=7, groups=1, stride=1, passes=0, x_layout=_lib.LAYOUT_NHWC):
    return _lib.ConvDesc(n=n, c_in=c_in, h=h, w=h, c_out=c_out, kh=k, kw=k, stride_h=stride, stride_w=stride, pad_h=pad, pad_w=pad,
                         dil_h=1, dil_w=1, groups=groups, x_layout=x_layout, y_layout=_lib.LAYOUT_NHWC, qbits=qbits,
                         ka=0.25, kw_scale=0.02, mfma_passes=passes, reserved=0)


def _spec_desc(s, n=2, qbits=7):
    return _lib.ConvDesc(n=n, c_in=s.c_in, h=s.h, w=s.w, c_out=s.c_out, kh=s.k[0], kw=s.k[1], stride_h=s.stride[0],
                         stride_w=s.stride[1], pad_h=s.pad[0], pad_w=s.pad[1], dil_h=1, dil_w=1, groups=s.groups,
                         x_layout=_lib.LAYOUT_NHWC, y_layout=_lib.LAYOUT_NHWC, qbits=qbits, ka=float(s.Ka), kw_scale=float(s.Kw),
                         mfma_passes=0, reserved=0)


def _io(x_codes=1, y_codes=1, y_qbits=7):
    return _lib.ConvIo(x_codes=x_codes, y_codes=y_codes, y_ka=0.3, y_qbits=y_qbits)


def _codes(d, io, has_bias=1, relu=1):
    return _lib.load().slfp_conv2d_codes_supported(ctypes.byref(d), ctypes.byref(io), has_bias, relu)


def _slice(d, io, y_ld, has_bias=1, relu=1):
    return _lib.load().slfp_conv2d_codes_slice_supported(ctypes.byref(d), ctypes.byref(io), has_bias, relu, y_ld)


def test_new_symbols_are_exported_and_declared():
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "slfp.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert hasattr(L, name)
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert L.slfp_version() == 1   # SLFP_ABI_VERSION: new exports only


def test_pointwise_layers_with_16_and_48_input_channels_read_codes():
    """Fire 3/4 squeeze to 16 channels and Fire 8/9 to 48: the expand1x1 layers that read them run on codes."""
    for (c_in, c_out, h) in ((16, 64, 54), (48, 192, 27)):
        for qbits in (7, 8):
            for n in (3, 64):
                for relu in (0, 1):
                    d = _desc(c_in, c_out, h, n=n, qbits=qbits)
                    assert _codes(d, _io(1, 1, qbits), relu=relu) == 1, (c_in, qbits, n, relu)   # codes -> codes
                    assert _codes(d, _io(1, 0, qbits), relu=relu) == 1, (c_in, qbits, n, relu)   # codes -> float32
                    assert _codes(d, _io(1, 1, qbits), has_bias=0, relu=relu) == 1
    assert _codes(_desc(96, 16, 54), _io(1, 1)) == 1 and _codes(_desc(96, 16, 54), _io(1, 0)) == 1   # the squeeze behind the stem
    # what stays refused
    assert _codes(_desc(24, 64, 54), _io(1, 1)) == 0 and _codes(_desc(24, 64, 54), _io(1, 0)) == 0   # 24 channels
    assert _codes(_desc(40, 64, 54), _io(1, 0)) == 0
    for c_in in (16, 48, 32, 64):   # float32 in, codes out: the pointwise producer is not built (tests/test_gpu_codes.py pins it too)
        assert _codes(_desc(c_in, 64, 54), _io(0, 1)) == 0, c_in
    assert _codes(_desc(16, 64, 54, qbits=8, passes=_lib.MFMA_F16X3), _io(1, 0, 8)) == 0   # three-pass mode: no code input
    assert _codes(_desc(16, 72, 54), _io(1, 1)) == 0      # code output: C_out a multiple of 16
    assert _codes(_desc(16, 72, 54), _io(1, 0)) == 1      # float32 output: a multiple of 4
    assert _codes(_desc(16, 64, 54, x_layout=_lib.LAYOUT_NCHW), _io(1, 1)) == 0


def _fires():
    """The Fire modules of the layer table: (squeeze, expand1x1, expand3x3) specs."""
    ls = layer_specs.conv_layers(NET)
    fires = [(ls[i], ls[i + 1], ls[i + 2]) for i in range(1, 25, 3)]
    for sq, e1, e3 in fires:
        assert sq.k == (1, 1) and e1.k == (1, 1) and e3.k == (3, 3) and e1.c_in == e3.c_in == sq.c_out and e1.c_out == e3.c_out
    return fires


def test_every_expand_layer_of_squeezenet_can_write_a_channel_slice():
    fires = _fires()
    assert len(fires) == 8 and sorted({f[0].c_out for f in fires}) == [16, 32, 48, 64]
    n_expand = 0
    for sq, e1, e3 in fires:
        for s in (e1, e3):
            for n in (4, 64, 256):
                d = _spec_desc(s, n=n)
                assert _slice(d, _io(1, 1), 2 * s.c_out) == 1, (s, n)
                assert _slice(d, _io(1, 1), 2 * s.c_out + 16) == 1, (s, n)
                assert _slice(d, _io(1, 1), s.c_out) == 1, (s, n)          # the dense tensor itself
            n_expand += 1
        # the squeeze layer that feeds both expands writes ONE dense code tensor (codes in)
        assert _codes(_spec_desc(sq), _io(1, 1)) == 1, sq
    assert n_expand == 16
    # the last Fire's consumer (the 512 -> 1000 classifier conv) reads codes and writes float32
    cls = layer_specs.conv_layers(NET)[25]
    assert cls.c_in == 512 and cls.k == (1, 1)
    assert _codes(_spec_desc(cls), _io(1, 0)) == 1


def test_slice_refusals():
    sq, e1, e3 = _fires()[0]
    for s in (e1, e3):
        d = _spec_desc(s)
        assert _slice(d, _io(1, 1), 2 * s.c_out + 8) == 0      # y_ld % 16
        assert _slice(d, _io(1, 1), 2 * s.c_out + 4) == 0
        assert _slice(d, _io(1, 1), s.c_out - 16) == 0         # y_ld < c_out
        assert _slice(d, _io(1, 1), 0) == 0
        assert _slice(d, _io(1, 0), 2 * s.c_out) == 0          # float32 output has no slice form
    assert _slice(_spec_desc(e3), _io(0, 1), 2 * e3.c_out) == 1    # dense family: float32 in, codes out, as slfp_conv2d_fwd_codes_ws
    assert _slice(_spec_desc(e1), _io(0, 1), 2 * e1.c_out) == 0    # pointwise float32 -> codes: not built
    dw = _desc(64, 64, 28, k=3, pad=1, groups=64, qbits=8)
    assert _codes(dw, _io(1, 1, 8), has_bias=0) == 1               # the depthwise family runs on codes ...
    assert _slice(dw, _io(1, 1, 8), 128, has_bias=0) == 0          # ... but has no channel-slice store
    stem = _desc(3, 32, 224, k=3, pad=1, stride=2, qbits=8)
    assert _slice(stem, _io(0, 1, 8), 64, has_bias=0) == 0
    L = _lib.load()
    assert L.slfp_conv2d_codes_slice_supported(None, ctypes.byref(_io()), 0, 1, 128) == 0
    assert L.slfp_conv2d_codes_slice_supported(ctypes.byref(_spec_desc(e1)), None, 0, 1, 128) == 0


def test_fwd_codes_slice_argument_checks_return_error_codes():
    """Every check that precedes device work: no pointer here is dereferenced."""
    L = _lib.load()
    sq, e1, e3 = _fires()[0]
    x, w, y = 1 << 20, 1 << 30, 1 << 32      # 16-byte aligned, never touched

    def call(d=None, io=None, x=x, w=w, y=y, y_ld=2 * e1.c_out, ws=None, s=e1):
        d = _spec_desc(s) if d is None else d
        io = _io(1, 1) if io is None else io
        return L.slfp_conv2d_fwd_codes_slice(ctypes.byref(d) if d is not False else None, ctypes.byref(io) if io is not False else None,
                                             x, w, None, None, None, 1, y, y_ld, ws, None)

    assert call(d=False) == _lib.ERR_BAD_ARG
    assert call(io=False) == _lib.ERR_BAD_ARG
    assert call(x=None) == _lib.ERR_BAD_ARG
    assert call(w=None) == _lib.ERR_BAD_ARG
    assert call(y=None) == _lib.ERR_BAD_ARG
    assert call(io=_io(1, 0)) == _lib.ERR_BAD_ARG                # io->y_codes == 1 is required
    assert call(y=y + 8) == _lib.ERR_ALIGNMENT                   # a channel offset that is not a multiple of 16
    assert call(y=y + 4) == _lib.ERR_ALIGNMENT
    assert call(y_ld=2 * e1.c_out + 8) == _lib.ERR_BAD_ARG and "y_ld" in _lib.last_error()
    assert call(y_ld=e1.c_out - 16) == _lib.ERR_BAD_ARG
    assert call(y_ld=0) == _lib.ERR_BAD_ARG
    assert call(y_ld=-16) == _lib.ERR_BAD_ARG
    assert call(x=x + 4) == _lib.ERR_ALIGNMENT
    assert call(io=_io(0, 1)) == _lib.ERR_UNSUPPORTED            # pointwise float32 -> codes
    assert "slfp_conv2d_codes_slice_supported" in _lib.last_error()
    dw = _desc(64, 64, 28, k=3, pad=1, groups=64, qbits=8)
    assert call(d=dw, io=_io(1, 1, 8), y_ld=128) == _lib.ERR_UNSUPPORTED
    assert call(s=e3, ws=None) == _lib.ERR_BAD_ARG and "workspace" in _lib.last_error()   # the dense family needs its workspace
    bad = _spec_desc(e1)
    bad.n = 0
    assert call(d=bad) == _lib.ERR_SHAPE
    bad = _spec_desc(e1)
    bad.qbits = 5
    assert call(d=bad) == _lib.ERR_BAD_ARG


def _pool_shape(h, w, k, s, p, ceil_mode):
    ho, wo = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = _lib.load().slfp_maxpool2d_out_shape(h, w, k, k, s, s, p, p, ceil_mode, ctypes.byref(ho), ctypes.byref(wo))
    return rc, ho.value, wo.value


def test_ceil_mode_pool_sizes_follow_max_pool2d():
    import torch
    import torch.nn.functional as F
    # SqueezeNet's three pools (nets_imgnet/squeezenet1_0.py: MaxPool2d(3, 2, ceil_mode=True))
    assert _pool_shape(109, 109, 3, 2, 0, 1) == (0, 54, 54)
    assert _pool_shape(54, 54, 3, 2, 0, 1) == (0, 27, 27)
    assert _pool_shape(27, 27, 3, 2, 0, 1) == (0, 13, 13)
    assert _pool_shape(54, 54, 3, 2, 0, 0) == (0, 26, 26)
    # the last window must start inside the input or its left padding: ceil((4 - 2) / 3) + 1 = 2, and window 1 starts at 3 < 4 ...
    assert _pool_shape(4, 4, 2, 3, 0, 1) == (0, 2, 2)
    # ... but with h = 3 it would start at 3 = h: dropped
    assert _pool_shape(3, 3, 2, 3, 0, 1) == (0, 1, 1)
    assert _pool_shape(5, 5, 2, 2, 1, 1)[1:] == tuple(F.max_pool2d(torch.zeros(1, 1, 5, 5), 2, 2, 1, ceil_mode=True).shape[2:])
    for h in range(1, 24):
        for k, s, p in ((3, 2, 0), (3, 2, 1), (2, 2, 0), (2, 3, 0), (2, 3, 1), (3, 1, 1), (4, 3, 2), (5, 4, 2), (3, 3, 1)):
            if h + 2 * p < k:
                assert _pool_shape(h, h, k, s, p, 1)[0] == _lib.ERR_SHAPE, (h, k, s, p)
                continue
            for cm in (0, 1):
                want = tuple(F.max_pool2d(torch.zeros(1, 1, h, h + 1), k, s, p, ceil_mode=bool(cm)).shape[2:])
                ho, wo = ctypes.c_int64(), ctypes.c_int64()
                assert _lib.load().slfp_maxpool2d_out_shape(h, h + 1, k, k, s, s, p, p, cm, ctypes.byref(ho), ctypes.byref(wo)) == 0
                assert (ho.value, wo.value) == want, (h, k, s, p, cm, (ho.value, wo.value), want)
    assert _pool_shape(8, 8, 3, 2, 0, 2)[0] == _lib.ERR_BAD_ARG     # ceil_mode is 0 or 1
    assert _pool_shape(8, 8, 2, 2, 2, 1)[0] == _lib.ERR_SHAPE       # padding beyond half the window
    assert _pool_shape(0, 8, 2, 2, 0, 1)[0] == _lib.ERR_SHAPE
    assert _pool_shape(8, 8, 2, 0, 0, 1)[0] == _lib.ERR_SHAPE


def test_maxpool_codes_ex_rejects_bad_geometry():
    L = _lib.load()
    x, y = 1 << 20, 1 << 30

    def call(x=x, y=y, n=1, h=8, w=8, c=16, k=3, s=2, p=0, qbits=7, ceil_mode=1):
        return L.slfp_maxpool2d_codes_ex(x, y, n, h, w, c, k, k, s, s, p, p, qbits, ceil_mode, None)

    assert call(x=None) == _lib.ERR_BAD_ARG
    assert call(y=None) == _lib.ERR_BAD_ARG
    assert call(qbits=6) == _lib.ERR_BAD_ARG
    assert call(ceil_mode=2) == _lib.ERR_BAD_ARG
    assert call(ceil_mode=-1) == _lib.ERR_BAD_ARG
    assert call(h=0) == _lib.ERR_SHAPE
    assert call(s=0) == _lib.ERR_SHAPE
    assert call(k=2, p=2) == _lib.ERR_SHAPE
    assert call(h=2, w=2, k=3) == _lib.ERR_SHAPE           # ceil mode: the window is larger than the input
    assert call(c=6) == _lib.ERR_UNSUPPORTED               # the C % 4 rule of slfp_maxpool2d_codes
    assert call(x=x + 4) == _lib.ERR_ALIGNMENT
    assert call(n=0) == _lib.OK                            # nothing to do: no launch


def test_forward_slice_is_a_method_of_its_own_and_needs_a_linked_producer():
    import torch
    for factory in (cf.conv2d_Q, cf.conv2d_Q_bias):
        m = factory(7, 0.1, 0.2)(16, 64, 1)
        assert list(inspect.signature(m.forward_slice).parameters) == ["input", "out_slice"]
        assert list(inspect.signature(m.forward).parameters) == ["input", "order", "residual"]   # forward's surface is unchanged
        buf = torch.zeros((1, 128, 4, 4), dtype=torch.uint8).contiguous(memory_format=torch.channels_last)
        x = torch.zeros((1, 16, 4, 4), dtype=torch.uint8).contiguous(memory_format=torch.channels_last)
        m.eval()
        with pytest.raises(RuntimeError, match="linked code producer"):
            m.forward_slice(x, (buf, 0))                       # `_code_out` is not set
        m._code_out = (0.3, 7)
        m.train()
        with pytest.raises(RuntimeError, match="linked code producer"):
            m.forward_slice(x, (buf, 0))                       # training mode
        m.eval()
        if m.bias is None:
            with pytest.raises(RuntimeError, match="ROCm"):
                m.forward_slice(x, (buf, 0))                   # a CPU tensor: there is no other way to compute this
    from cnns_slfp_quantization_amd import fusion, sfp_quant
    assert callable(fusion.fuse_fire) and callable(fusion.unfuse_fire)
    assert inspect.signature(sfp_quant.hip_maxpool_codes).parameters["ceil_mode"].default is False
