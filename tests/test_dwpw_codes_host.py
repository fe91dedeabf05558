"""CPU: the host side of the depthwise -> pointwise block as ONE kernel on 1-byte codes (csrc/conv_dwpw_codes.hip):
slfp_dwpw_codes_supported / slfp_dwpw_fwd_codes, options.dwpw_codes_pairs and fusion.DwPwBlock off the device.  No device work is
done here: every pointer handed to the library is refused before it would be dereferenced."""
import ctypes
import os
import re

import torch
import torch.nn as nn

from cnns_slfp_quantization_amd import _lib, fusion
from cnns_slfp_quantization_amd import conv2d_func as cf

NEW = ("slfp_dwpw_codes_supported", "slfp_dwpw_fwd_codes")
NHWC, NCHW = _lib.LAYOUT_NHWC, _lib.LAYOUT_NCHW


def _pair(c, n_out, stride, h, w=None, n=2, qbits=8, qbits_pw=None, pad=1, dil=1, passes=0, dw_layouts=(NHWC, NHWC), pw_layouts=(NHWC, NHWC)):
    """The two descriptors of a block: 3x3 depthwise on c channels at h x w, then 1x1 -> n_out on its output."""
    w = h if w is None else w
    ho, wo = (h + 2 * pad - dil * 2 - 1) // stride + 1, (w + 2 * pad - dil * 2 - 1) // stride + 1
    dw = _lib.ConvDesc(n=n, c_in=c, h=h, w=w, c_out=c, kh=3, kw=3, stride_h=stride, stride_w=stride, pad_h=pad, pad_w=pad, dil_h=dil,
                       dil_w=dil, groups=c, x_layout=dw_layouts[0], y_layout=dw_layouts[1], qbits=qbits, ka=0.17, kw_scale=0.12,
                       mfma_passes=passes, reserved=0)
    pw = _lib.ConvDesc(n=n, c_in=c, h=ho, w=wo, c_out=n_out, kh=1, kw=1, stride_h=1, stride_w=1, pad_h=0, pad_w=0, dil_h=1, dil_w=1,
                       groups=1, x_layout=pw_layouts[0], y_layout=pw_layouts[1], qbits=qbits if qbits_pw is None else qbits_pw, ka=0.25,
                       kw_scale=0.02, mfma_passes=passes, reserved=0)
    return dw, pw


def _io(x_codes=1, y_codes=1, y_qbits=8, y_ka=0.3):
    return _lib.ConvIo(x_codes=x_codes, y_codes=y_codes, y_ka=y_ka, y_qbits=y_qbits)


def _q(dw, pw, io, has_bias=0, relu1=1, relu2=1):
    ref = lambda s: ctypes.byref(s) if s is not None else None
    return _lib.load().slfp_dwpw_codes_supported(ref(dw), ref(pw), ref(io), has_bias, relu1, relu2)


SUPPORTED = [(32, 64, 1, 28, 28), (64, 128, 2, 30, 30), (128, 128, 1, 14, 14), (128, 256, 2, 28, 28), (32, 64, 1, 20, 33)]


def test_new_symbols_are_exported_and_declared():
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "slfp.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert hasattr(L, name)
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert L.slfp_version() == 1   # SLFP_ABI_VERSION: new exports only


def test_query_says_yes_on_the_lds_resident_blocks():
    for c, n_out, s, h, w in SUPPORTED:
        for qbits in (8, 7):
            for y_codes in (0, 1):
                for relu1, relu2, has_bias in ((1, 1, 0), (0, 0, 1), (1, 0, 0)):
                    dw, pw = _pair(c, n_out, s, h, w, qbits=qbits)
                    assert _q(dw, pw, _io(1, y_codes, qbits), has_bias, relu1, relu2) == 1, (c, n_out, s, h, w, qbits, y_codes, relu1, relu2)
    dw, pw = _pair(64, 128, 2, 30, qbits=8)
    assert _q(dw, pw, _io(1, 1, 7)) == 1          # the reader's q_bit is its own
    dw, pw = _pair(32, 64, 1, 28, qbits=7, passes=_lib.MFMA_F16X3)
    assert _q(dw, pw, _io(1, 1, 7)) == 1          # SFP<3,3> is exact in one pass whatever the mode


def _refused():
    ok = lambda **kw: _pair(32, 64, 1, 28, **kw)
    return [
        ("x_codes0", ok(), _io(0, 1)),
        ("x_codes2", ok(), _io(2, 1)),
        ("y_codes2", ok(), _io(1, 2)),
        ("f16x3", ok(passes=_lib.MFMA_F16X3), _io()),
        ("c256", _pair(256, 128, 1, 28), _io()),
        ("n512", _pair(64, 512, 1, 28), _io()),
        ("128->512", _pair(128, 512, 2, 28), _io()),
        ("c48", _pair(48, 64, 1, 28), _io()),
        ("mixed_qbits", ok(qbits=8, qbits_pw=7), _io()),
        ("dilated", ok(pad=2, dil=2), _io()),
        ("nchw_in", ok(dw_layouts=(NCHW, NHWC)), _io()),
        ("nchw_mid_dw", ok(dw_layouts=(NHWC, NCHW)), _io()),
        ("nchw_mid_pw", ok(pw_layouts=(NCHW, NHWC)), _io()),
        ("nchw_out", ok(pw_layouts=(NHWC, NCHW)), _io()),
        ("s1_13rows", _pair(32, 64, 1, 13, 28), _io()),
        ("s1_13cols", _pair(32, 64, 1, 28, 13), _io()),
        ("y_qbits5", ok(), _io(1, 1, 5)),
        ("y_ka0", ok(), _io(1, 1, 8, 0.0)),
        ("y_ka<0", ok(), _io(1, 1, 8, -0.3)),
    ]


def test_query_refuses_everything_else():
    for name, (dw, pw), io in _refused():
        assert _q(dw, pw, io) == 0, name
    dw, pw = _pair(32, 64, 1, 28)
    assert _q(dw, pw, _io()) == 1                       # the control: the same pair, plain
    for relu1, relu2 in ((1 | 2, 1), (1, 1 | 2), (2, 0), (0, 2), (4, 0), (-1, 1)):
        assert _q(dw, pw, _io(), 0, relu1, relu2) == 0, (relu1, relu2)   # SLFP_POST_LAYEROUT / unknown bits
    assert _q(None, pw, _io()) == 0 and _q(dw, None, _io()) == 0 and _q(dw, pw, None) == 0   # null descriptors
    pw2 = _pair(32, 64, 1, 28)[1]
    pw2.h = 27                                           # not the depthwise layer's output
    assert _q(dw, pw2, _io()) == 0
    big = _pair(128, 256, 1, 2048, 1025, n=1)           # past the tensor-size limits of the kernels' 32-bit offsets
    assert _q(*big, _io()) == 0


def test_the_existing_queries_answer_as_before():
    """slfp_dwpw_supported knows nothing of codes, and slfp_conv2d_codes_supported keeps taking the two layers one by one."""
    L = _lib.load()
    for c, n_out, s, h, w in SUPPORTED:
        for qbits in (8, 7):
            dw, pw = _pair(c, n_out, s, h, w, qbits=qbits)
            assert L.slfp_dwpw_supported(ctypes.byref(dw), ctypes.byref(pw)) == 1
            io_mid, io_f32, io_out = _io(1, 1, qbits, 0.25), _io(1, 0), _io(1, 1, qbits)
            assert L.slfp_conv2d_codes_supported(ctypes.byref(dw), ctypes.byref(io_mid), 0, 1) == 1
            assert L.slfp_conv2d_codes_supported(ctypes.byref(pw), ctypes.byref(io_f32), 0, 1) == 1
            assert L.slfp_conv2d_codes_supported(ctypes.byref(pw), ctypes.byref(io_out), 1, 0) == 1
    for name, (dw, pw), io in _refused():
        if name.startswith("nchw_mid"):
            continue
        want = 0 if name in ("f16x3", "c256", "n512", "128->512", "c48", "mixed_qbits", "dilated", "nchw_in", "nchw_out",
                             "s1_13rows", "s1_13cols") else 1   # the io struct and the layouts between the layers are not its business
        assert L.slfp_dwpw_supported(ctypes.byref(dw), ctypes.byref(pw)) == want, name
    dw, pw = _pair(256, 256, 1, 28)   # a K >= 256 block: two code kernels, as before
    io_mid, io_out = _io(1, 1, 8, 0.25), _io(1, 1)
    assert L.slfp_conv2d_codes_supported(ctypes.byref(dw), ctypes.byref(io_mid), 0, 1) == 1
    assert L.slfp_conv2d_codes_supported(ctypes.byref(pw), ctypes.byref(io_out), 0, 1) == 1
    assert _q(dw, pw, io_out) == 0


def test_fwd_codes_argument_checks_return_error_codes():
    """Every check that precedes device work: no pointer here is dereferenced."""
    L = _lib.load()
    x, w1, w2, y, v = 1 << 20, 1 << 30, 1 << 31, 1 << 32, 1 << 34      # 16-byte aligned, never touched

    def call(pair=None, io=None, x=x, w1=w1, w2=w2, y=y, s1=v, h1=v + 1024, bias=None, s2=None, h2=None, relu1=1, relu2=1, nulls=()):
        dw, pw = _pair(32, 64, 1, 28) if pair is None else pair
        io = _io() if io is None else io
        ref = lambda s, k: None if k in nulls else ctypes.byref(s)
        return L.slfp_dwpw_fwd_codes(ref(dw, "dw"), ref(pw, "pw"), ref(io, "io"), x, w1, s1, h1, relu1, w2, bias, s2, h2, relu2, y, None)

    for k in ("dw", "pw", "io"):
        assert call(nulls=(k,)) == _lib.ERR_BAD_ARG, k
    for kw in (dict(x=None), dict(w1=None), dict(w2=None), dict(y=None), dict(s1=None), dict(h1=None), dict(s2=v), dict(h2=v)):
        assert call(**kw) == _lib.ERR_BAD_ARG, kw
        assert _lib.last_error()
    for kw in (dict(x=x + 4), dict(y=y + 8), dict(w1=w1 + 4), dict(w2=w2 + 2), dict(s1=v + 4), dict(bias=v + 4), dict(s2=v + 4, h2=v)):
        assert call(**kw) == _lib.ERR_ALIGNMENT, kw
    for name, pair, io in _refused():
        assert call(pair=pair, io=io) == _lib.ERR_UNSUPPORTED, name
        assert "slfp_dwpw_codes_supported" in _lib.last_error()
    assert call(relu1=1 | 2) == _lib.ERR_UNSUPPORTED and _lib.last_error()
    assert call(relu2=2, s2=v, h2=v) == _lib.ERR_UNSUPPORTED


def _block(q_bit, c=32, n_out=64, stride=1):
    dw = cf.conv2d_Q_bias(q_bit, 0.12, 0.17)(c, c, 3, stride=stride, padding=1, groups=c, bias=False)
    pw = cf.conv2d_Q_bias(q_bit, 0.02, 0.25)(c, n_out, 1, bias=False)
    return nn.Sequential(dw, nn.BatchNorm2d(c), nn.ReLU(), pw, nn.BatchNorm2d(n_out), nn.ReLU()).eval()


def test_option_default_and_block_off_the_device():
    assert len(cf.options.dwpw_codes_pairs) == 0 and cf.options.dwpw_all is False
    assert cf.options.dwpw_pairs == {(32, 1)}                      # the float32 form's default is what it was
    torch.manual_seed(0)
    m = _block(32)                                                 # identity quantizers: stock ATen on the CPU
    x = torch.randn(2, 32, 16, 16)
    with torch.no_grad():
        y0 = m(x)
        assert fusion.fuse_bn_relu(m) == 2 and fusion.fuse_dw_pw(m) == 1
        blk = [b for b in m if isinstance(b, fusion.DwPwBlock)][0]
        y1 = m(x)
        assert blk._last_kernel is None                            # its two convs ran
        assert torch.allclose(y1, y0, rtol=1e-5, atol=1e-6)
        x8 = torch.zeros(2, 32, 16, 16, dtype=torch.uint8)
        assert blk._forward_codes(x8) is None                      # codes off the device: not this path's
    assert fusion.unfuse(m) == 2 and not any(isinstance(b, fusion.DwPwBlock) for b in m)
    # the pass order with links: the block holds the linked convs, unlink_codes reaches them
    m = _block(8)
    fusion.fuse_bn_relu(m)
    assert fusion.link_codes(m) == 1 and m[0]._code_out == (0.25, 8)
    assert fusion.fuse_dw_pw(m) == 1
    blk = [b for b in m if isinstance(b, fusion.DwPwBlock)][0]
    assert blk.dw._code_out == fusion._reader_quant(blk.pw) and blk.pw._code_out is None
    assert fusion.unlink_codes(m) == 1 and blk.dw._code_out is None
    assert fusion.unfuse_dw_pw(m) == 1 and m[0] is blk.dw and m[3] is blk.pw
