"""CPU: the host side of the table epilogue behind the layer-output quantizer (csrc/slfp_layerout_lut.hpp): the
class index and its inverse against the oracle's layerout on every input class the index treats differently, the support query of
slfp_conv2d_fwd_codes_lut, its argument checks, and the older entry points' refusal of SLFP_POST_LAYEROUT.  No device work is
done here: every pointer handed to the library is refused before it would be dereferenced."""
import ctypes
import os
import re

import numpy as np
import pytest

from cnns_slfp_quantization_amd import _lib, fusion
from cnns_slfp_quantization_amd import conv2d_func as cf
from oracle import slfp_oracle as so

NEW = ("slfp_layerout_lut_classes", "slfp_layerout_lut_values", "slfp_layerout_lut_index", "slfp_conv2d_codes_lut_supported",
       "slfp_conv2d_fwd_codes_lut", "slfp_debug_layerout_lut_mismatches")
LUT_BYTES = _lib.LAYEROUT_LUT_BYTES


def _desc(c_in, c_out, h, w=None, k=1, pad=0, n=2, qbits=8, groups=1, stride=1, passes=0, x_layout=_lib.LAYOUT_NHWC,
          y_layout=_lib.LAYOUT_NHWC):
    return _lib.ConvDesc(n=n, c_in=c_in, h=h, w=h if w is None else w, c_out=c_out, kh=k, kw=k, stride_h=stride, stride_w=stride,
                         pad_h=pad, pad_w=pad, dil_h=1, dil_w=1, groups=groups, x_layout=x_layout, y_layout=y_layout, qbits=qbits,
                         ka=0.25, kw_scale=0.02, mfma_passes=passes, reserved=0)


def _io(x_codes=1, y_codes=1, y_qbits=8, y_ka=0.3):
    return _lib.ConvIo(x_codes=x_codes, y_codes=y_codes, y_ka=y_ka, y_qbits=y_qbits)


def _lut_ok(d, io, has_bias=0, y_ld=None):
    return _lib.load().slfp_conv2d_codes_lut_supported(ctypes.byref(d) if d is not None else None, ctypes.byref(io) if io is not None else None,
                                                       has_bias, d.c_out if y_ld is None else y_ld)


@pytest.fixture(scope="module")
def values():
    L = _lib.load()
    v = np.full(LUT_BYTES, 7.0, dtype=np.float32)
    assert L.slfp_layerout_lut_values(v.ctypes.data, LUT_BYTES) == _lib.OK
    return v


def _index(bits):
    """slfp_layerout_lut_index of every uint32 pattern in `bits`"""
    L = _lib.load()
    f = np.asarray(bits, dtype=np.uint32).view(np.float32)
    return np.fromiter((L.slfp_layerout_lut_index(ctypes.c_float(float(x))) for x in f), dtype=np.int64, count=f.size)


def _index_all(lo_bits):
    """slfp_layerout_lut_index of every element: the quantizer's image is a few thousand values, so the library is asked once per
    distinct pattern."""
    uniq, inv = np.unique(np.asarray(lo_bits, dtype=np.uint32), return_inverse=True)
    assert uniq.size <= LUT_BYTES
    return _index(uniq)[inv.ravel()]


def test_new_symbols_are_exported_and_declared():
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "slfp.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert hasattr(L, name)
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert re.search(r"#define\s+SLFP_LAYEROUT_LUT_BYTES\s+%d\b" % LUT_BYTES, header)
    assert L.slfp_version() == 1   # SLFP_ABI_VERSION: new exports only


def test_table_size_and_padding(values):
    n = _lib.load().slfp_layerout_lut_classes()
    assert 0 < n <= LUT_BYTES <= 8192 and LUT_BYTES % 16 == 0
    assert np.isnan(values[0]) and not np.isnan(values[1:n]).any()          # the NaN slot is index 0, alone
    assert (values[n:].view(np.uint32) == 0).all()                          # padding holds +0
    assert len(set(values[1:n].view(np.uint32).tolist())) == n - 1          # distinct values: the index is injective
    assert _lib.load().slfp_layerout_lut_values(None, 4) == _lib.ERR_BAD_ARG


def test_values_and_index_are_inverse_on_every_index(values):
    n = _lib.load().slfp_layerout_lut_classes()
    idx = _index(values[:n].view(np.uint32))
    assert np.array_equal(idx, np.arange(n))
    # every table value is a fixed point of the quantizer (NaN stays NaN)
    lo = so.layerout(values[1:n]).view(np.uint32)
    assert np.array_equal(lo, values[1:n].view(np.uint32))
    # values outside the quantizer's image have no index
    for x in (0.0, -0.0, 1.03125, 249.0, float("inf")):
        assert _lib.load().slfp_layerout_lut_index(ctypes.c_float(x)) == -1, x


def _roundtrip(bits, values, n):
    """index(layerout(x)) is below n and values[index] == layerout(x) in bits (every NaN equal to every NaN)"""
    x = np.asarray(bits, dtype=np.uint32).view(np.float32)
    lo = so.layerout(x).view(np.uint32)
    idx = _index_all(lo)
    assert idx.min() >= 0 and idx.max() < n
    back = values[idx].view(np.uint32)
    nan = (lo & 0x7FFFFFFF) > 0x7F800000
    assert np.array_equal(nan, idx == 0)
    assert np.array_equal(back[~nan], lo[~nan])
    return lo, idx


def test_index_of_layerout_round_trips_on_all_positive_denormals(values):
    n = _lib.load().slfp_layerout_lut_classes()
    bits = np.arange(1, 1 << 23, dtype=np.uint32)
    lo, idx = _roundtrip(bits, values, n)
    assert idx.min() == 1 and idx.max() == 320          # up to the smallest normal, which 0x007FFFFF rounds to
    lo_n, idx_n = _roundtrip(bits | np.uint32(0x80000000), values, n)
    assert np.array_equal(idx_n, idx + 2463)            # the negative side mirrors the positive one


def test_index_of_layerout_round_trips_on_the_rounding_edges_of_every_binade(values):
    n = _lib.load().slfp_layerout_lut_classes()
    hi = np.arange(1 << 16, dtype=np.uint32) << np.uint32(16)
    seen = set()
    for low in (0x0000, 0x7FFF, 0x8000, 0xFFFF):
        lo, idx = _roundtrip(hi | np.uint32(low), values, n)      # both signs: the high half covers the sign bit
        seen |= set(idx.tolist())
    assert len(seen) > 4300                                        # all normal classes of both signs are reached


def test_index_of_layerout_on_the_special_values(values):
    n = _lib.load().slfp_layerout_lut_classes()
    L = _lib.load()
    x = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 247.9, 248.0, 1e30, -247.9, -248.0, -1e30], dtype=np.float32)
    lo, idx = _roundtrip(x.view(np.uint32), values, n)
    assert idx[0] == 0 and idx[1] == 0 and idx[4] == 0                        # exact zero -> NaN, NaN -> NaN: the NaN slot
    assert values[idx[2]] == 248.0 and values[idx[3]] == -248.0               # +-inf clamp
    assert values[idx[5]] == 248.0 and values[idx[6]] == 248.0 and values[idx[7]] == 248.0
    assert values[idx[8]] == -248.0 and values[idx[10]] == -248.0
    assert L.slfp_layerout_lut_index(ctypes.c_float(248.0)) == idx[6] < n


# what tests/test_gpu_layerout_lut.py runs: (descriptor, io)
def _supported_cases():
    out = []
    for c in (32, 64):
        for s in (1, 2):
            for h, w in ((1, 1), (2, 2), (5, 7)):
                out.append((f"dw{c}s{s}@{h}x{w}", _desc(c, c, h, w, k=3, pad=1, groups=c, stride=s), _io(1, 1)))
    for k_in, n_out in ((32, 64), (64, 32), (256, 256), (512, 512), (1024, 1024)):
        for h, w in ((1, 1), (3, 5)):
            out.append((f"pw{k_in}-{n_out}@{h}x{w}", _desc(k_in, n_out, h, w), _io(1, 1)))
    for c_in, c_out in ((64, 64), (128, 256)):
        for h, w in ((2, 2), (5, 7)):
            for xc in (0, 1):
                out.append((f"dense{c_in}-{c_out}@{h}x{w}/x{xc}", _desc(c_in, c_out, h, w, k=3, pad=1), _io(xc, 1)))
    out.append(("stem32", _desc(3, 32, 6, 10, k=3, pad=1, stride=2), _io(0, 1)))
    out.append(("stem64", _desc(3, 64, 6, 10, k=3, pad=1), _io(0, 1)))
    return out


def test_lut_supported_on_the_tested_shapes_and_the_two_nets():
    for name, d, io in _supported_cases():
        for yq in (8, 7):
            io.y_qbits = yq
            assert _lut_ok(d, io) == 1, (name, yq)
    # slices: the 1x1 and the dense code stores take a pixel stride; depthwise and stem layers do not
    assert _lut_ok(_desc(64, 32, 3, 5), _io(1, 1), y_ld=64) == 1
    assert _lut_ok(_desc(64, 64, 5, 7, k=3, pad=1), _io(0, 1), y_ld=128) == 1
    assert _lut_ok(_desc(64, 64, 5, 7, k=3, pad=1, groups=64), _io(1, 1), y_ld=128) == 0
    assert _lut_ok(_desc(3, 32, 6, 10, k=3, pad=1, stride=2), _io(0, 1), y_ld=64) == 0
    assert _lut_ok(_desc(64, 32, 3, 5), _io(1, 1), y_ld=40) == 0       # not a multiple of 16
    assert _lut_ok(_desc(64, 32, 3, 5), _io(1, 1), y_ld=16) == 0       # narrower than the layer
    # MobileNetV1_swish at 32 x 32, batch 256 (nets_cifar/mobilenetv1.py:232-246) and VGG16_gelu (nets_cifar/vgg16.py:186-293)
    mb = [(32, 64, 16, 1), (64, 128, 16, 2), (128, 128, 8, 1), (128, 256, 8, 2), (256, 256, 4, 1), (256, 512, 4, 2),
          (512, 512, 2, 1), (512, 1024, 2, 2), (1024, 1024, 1, 1)]
    assert _lut_ok(_desc(3, 32, 32, k=3, pad=1, stride=2, n=256), _io(0, 1)) == 1
    for c_in, c_out, h, s in mb:
        assert _lut_ok(_desc(c_in, c_in, h, k=3, pad=1, groups=c_in, stride=s, n=256), _io(1, 1)) == 1, ("dw", c_in, h, s)
        assert _lut_ok(_desc(c_in, c_out, h // s, n=256), _io(1, 1)) == 1, ("pw", c_in, c_out, h // s)
    assert _lut_ok(_desc(3, 64, 32, k=3, pad=1, n=256), _io(0, 1)) == 1
    for c_in, c_out, h in ((64, 64, 32), (64, 128, 16), (128, 128, 16), (128, 256, 8), (256, 256, 8), (256, 512, 4), (512, 512, 4),
                           (512, 512, 2)):
        assert _lut_ok(_desc(c_in, c_out, h, k=3, pad=1, n=256), _io(1, 1)) == 1, ("dense", c_in, c_out, h)


def test_lut_refuses_everything_else():
    ok = _desc(64, 64, 8)
    assert _lut_ok(ok, _io(1, 1)) == 1                                              # the control
    L = _lib.load()
    assert L.slfp_conv2d_codes_lut_supported(None, ctypes.byref(_io(1, 1)), 0, 64) == 0
    assert L.slfp_conv2d_codes_lut_supported(ctypes.byref(ok), None, 0, 64) == 0
    refused = [
        ("entry: float32 in, 1x1", ok, _io(0, 1)),
        ("float32 out", ok, _io(1, 0)),
        ("nchw in", _desc(64, 64, 8, x_layout=_lib.LAYOUT_NCHW), _io(1, 1)),
        ("nchw out", _desc(64, 64, 8, y_layout=_lib.LAYOUT_NCHW), _io(1, 1)),
        ("f16x3 at qbits 8", _desc(64, 64, 8, passes=_lib.MFMA_F16X3), _io(1, 1)),
        ("f16x3 dense", _desc(64, 64, 8, k=3, pad=1, passes=_lib.MFMA_F16X3), _io(1, 1)),
        ("c_out % 16", _desc(64, 24, 8), _io(1, 1)),
        ("c_out % 16 dense", _desc(64, 72, 8, k=3, pad=1), _io(1, 1)),
        ("y_qbits 5", ok, _io(1, 1, 5)),
        ("y_ka 0", ok, _io(1, 1, 8, 0.0)),
        ("large-kernel stem", _desc(3, 64, 32, k=7, pad=3, stride=2), _io(0, 1)),
        ("16-channel squeeze (half k-step)", _desc(16, 64, 8), _io(1, 1)),
        ("96 channels (three k-steps)", _desc(96, 64, 8), _io(1, 1)),
        ("58 channels", _desc(58, 58, 8), _io(1, 1)),
    ]
    for name, d, io in refused:
        assert _lut_ok(d, io) == 0, name


def test_residual_and_dual_forms_have_no_table_and_old_entry_points_refuse_layerout():
    """RES / DUAL: slfp_conv2d_fwd_res / _res_codes have no lut argument and refuse the layer-output bit, as do the code, slice and
    entry queries -- with and without the ReLU bit."""
    L = _lib.load()
    d, dd = _desc(64, 64, 8), _desc(64, 64, 8, k=3, pad=1)
    for flags in (2, 3):
        assert L.slfp_conv2d_codes_supported(ctypes.byref(d), ctypes.byref(_io(1, 1)), 0, flags) == 0
        assert L.slfp_conv2d_codes_supported(ctypes.byref(d), ctypes.byref(_io(1, 0)), 0, flags) == 0
        assert L.slfp_conv2d_codes_supported(ctypes.byref(dd), ctypes.byref(_io(0, 1)), 0, flags) == 0
        assert L.slfp_conv2d_codes_slice_supported(ctypes.byref(d), ctypes.byref(_io(1, 1)), 0, flags, 128) == 0
        assert L.slfp_conv2d_entry_supported(ctypes.byref(d), ctypes.byref(_io(0, 1)), 0, flags) == 0
        assert L.slfp_conv2d_res_supported(ctypes.byref(d), ctypes.byref(_io(1, 0)), 0, flags) == 0
        assert L.slfp_conv2d_res_codes_supported(ctypes.byref(d), ctypes.byref(_io(1, 1)), 0, flags) == 0
    for flags in (0, 1):   # the controls: the same layers without the bit
        assert L.slfp_conv2d_codes_supported(ctypes.byref(d), ctypes.byref(_io(1, 1)), 0, flags) == 1
        assert L.slfp_conv2d_res_codes_supported(ctypes.byref(d), ctypes.byref(_io(1, 1)), 0, flags) == 1
    x, w, y, v = 1 << 20, 1 << 30, 1 << 32, 1 << 34
    io = _io(1, 1)
    assert L.slfp_conv2d_fwd_codes(ctypes.byref(d), ctypes.byref(io), x, w, None, v, v, 2, y, None) == _lib.ERR_UNSUPPORTED
    assert L.slfp_conv2d_fwd_codes_slice(ctypes.byref(d), ctypes.byref(io), x, w, None, v, v, 3, y, 128, None, None) == _lib.ERR_UNSUPPORTED
    assert L.slfp_conv2d_fwd_res_codes(ctypes.byref(d), ctypes.byref(io), x, w, None, v, v, 2, v + (1 << 30), y, y + (1 << 30), None, None) == _lib.ERR_UNSUPPORTED


def test_fwd_codes_lut_argument_checks_return_error_codes():
    """Every check that precedes device work: no pointer here is dereferenced."""
    L = _lib.load()
    x, w, y, v, t = 1 << 20, 1 << 30, 1 << 32, 1 << 34, 1 << 36      # 16-byte aligned, never touched

    def call(d=None, io=None, x=x, w=w, y=y, ps=v, psh=v + 4096, lut=t, y_ld=None, ws=None):
        d = _desc(64, 64, 8) if d is None else d
        io = _io(1, 1) if io is None else io
        return L.slfp_conv2d_fwd_codes_lut(ctypes.byref(d) if d is not False else None, ctypes.byref(io) if io is not False else None,
                                           x, w, None, ps, psh, lut, y, d.c_out if y_ld is None and d is not False else (y_ld or 0), ws, None)

    assert call(d=False) == _lib.ERR_BAD_ARG
    assert call(io=False) == _lib.ERR_BAD_ARG
    assert call(x=None) == _lib.ERR_BAD_ARG
    assert call(w=None) == _lib.ERR_BAD_ARG
    assert call(y=None) == _lib.ERR_BAD_ARG
    assert call(lut=None) == _lib.ERR_BAD_ARG
    assert call(ps=None, psh=None) == _lib.ERR_BAD_ARG and "post_scale" in _lib.last_error()     # the table needs the affine
    assert call(ps=None) == _lib.ERR_BAD_ARG
    assert call(lut=t + 4) == _lib.ERR_ALIGNMENT and "lut" in _lib.last_error()
    assert call(x=x + 4) == _lib.ERR_ALIGNMENT
    assert call(y=y + 8) == _lib.ERR_ALIGNMENT
    assert call(ps=v + 4) == _lib.ERR_ALIGNMENT
    assert call(io=_io(1, 0)) == _lib.ERR_BAD_ARG
    assert call(io=_io(1, 1, 5)) == _lib.ERR_BAD_ARG
    assert call(io=_io(1, 1, 8, 0.0)) == _lib.ERR_BAD_ARG
    assert call(y_ld=72) == _lib.ERR_BAD_ARG
    assert call(io=_io(0, 1)) == _lib.ERR_UNSUPPORTED and "slfp_conv2d_codes_lut_supported" in _lib.last_error()   # the entry kernel
    assert call(d=_desc(64, 24, 8)) == _lib.ERR_UNSUPPORTED
    assert call(d=_desc(64, 64, 8, x_layout=_lib.LAYOUT_NCHW)) == _lib.ERR_UNSUPPORTED
    assert call(d=_desc(64, 64, 8, passes=_lib.MFMA_F16X3)) == _lib.ERR_UNSUPPORTED
    assert call(d=_desc(64, 64, 8, k=3, pad=1, groups=64), y_ld=128) == _lib.ERR_UNSUPPORTED   # depthwise: no slice store
    assert call(d=_desc(64, 64, 8, k=3, pad=1)) == _lib.ERR_BAD_ARG and "workspace" in _lib.last_error()   # dense: needs one
    bad = _desc(64, 64, 8)
    bad.n = 0
    assert call(d=bad) == _lib.ERR_SHAPE


def test_module_attribute_and_state_dict_keys():
    m = cf.conv2d_Q_bias(8, 0.02, 0.25)(64, 64, 1)
    assert m._code_lut is None and m._code_out is None
    assert "_code_lut" in m._buffers and "_code_lut" in m._non_persistent_buffers_set
    keys = set(m.state_dict().keys())
    import torch
    m._code_lut = torch.zeros(LUT_BYTES, dtype=torch.uint8)
    assert set(m.state_dict().keys()) == keys == {"weight", "bias"}      # the reference's keys, linked or not
    m._code_out = (0.3, 8)
    assert fusion.unlink_codes(m) == 1 and m._code_lut is None and m._code_out is None
    assert callable(fusion.link_layerout) and issubclass(fusion.CodeAct, torch.nn.Module)
    act = torch.nn.GELU()
    wrapped = fusion.CodeAct(act)
    c = torch.arange(8, dtype=torch.uint8)
    assert wrapped(c) is c and torch.equal(wrapped(torch.ones(3)), act(torch.ones(3)))
