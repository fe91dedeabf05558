"""CPU: the host side of the global average pool: slfp_global_avgpool_supported / slfp_global_avgpool_f32's
refusals, and fusion.GlobalAvgPool2d / use_device_avgpool / link_pool_head on a model without a device.  No device work is done
here: the library loads without a GPU, the query is host only and every refusal comes before the launch."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

from cnns_slfp_quantization_amd import _lib, fusion
from cnns_slfp_quantization_amd import conv2d_func as cf

NEW = ("slfp_global_avgpool_supported", "slfp_global_avgpool_f32")
NHWC, NCHW = _lib.LAYOUT_NHWC, _lib.LAYOUT_NCHW


def _io(y_codes=0, y_ka=0.3, y_qbits=8, x_codes=0):
    return _lib.ConvIo(x_codes=x_codes, y_codes=y_codes, y_ka=y_ka, y_qbits=y_qbits)


def _ok(n, h, w, c, layout, io=None):
    io = io if io is not None else _io()
    return _lib.load().slfp_global_avgpool_supported(n, h, w, c, layout, ctypes.byref(io))


def test_new_symbols_are_exported_and_declared():
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "slfp.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert hasattr(L, name)
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    doc = header[header.index("csrc/pool_avg.hip"):]
    # the order of summation is part of the interface, and the reference lines the kernel replaces are cited
    for text in ("(mod 4)", "((s_0 + s_1) + (s_2 + s_3))", "+0.0f", "IEEE float32 division", "nets_imgnet/resnet50.py:146-147",
                 "nets_cifar/mobilenetv1.py:62-86", "nets_imgnet/mobilenetv1.py:58", "nets_imgnet/squeezenet1_0.py:85"):
        assert text in doc, text
    assert L.slfp_version() == 1   # SLFP_ABI_VERSION: new exports only


def test_supported_truth_table():
    for c in (4, 20, 64, 1000, 2048):
        assert _ok(3, 7, 7, c, NHWC) == 1
        assert _ok(3, 7, 7, c, NCHW) == 1
        for q in (8, 7):
            assert _ok(3, 7, 7, c, NHWC, _io(1, y_qbits=q)) == 1
            assert _ok(3, 7, 7, c, NCHW, _io(1, y_qbits=q)) == 1
    for c in (1, 2, 10, 57):
        assert _ok(3, 7, 7, c, NHWC) == 0            # NHWC reads 4 channels per load
        assert _ok(3, 7, 7, c, NCHW) == 1            # NCHW takes any C
        assert _ok(3, 7, 7, c, NCHW, _io(1)) == 0    # ... but a code dword is 4 channels
    for h, w in ((1, 1), (1, 2), (13, 13), (1, 7)):
        assert _ok(1, h, w, 64, NHWC) == 1 and _ok(1, h, w, 64, NCHW) == 1
    assert _ok(0, 7, 7, 64, NHWC) == 1               # an empty batch is no error


@pytest.mark.parametrize("args,io", [
    ((3, 0, 7, 64, NHWC), None), ((3, 7, 0, 64, NHWC), None), ((3, 7, 7, 0, NCHW), None), ((-1, 7, 7, 64, NHWC), None),
    ((3, 7, 7, 64, 2), None), ((3, 7, 7, 64, -1), None),                    # a bad layout
    ((3, 7, 7, 64, NHWC), _io(1, y_qbits=6)), ((3, 7, 7, 64, NCHW), _io(1, y_qbits=32)),
    ((3, 7, 7, 64, NHWC), _io(1, y_ka=0.0)), ((3, 7, 7, 64, NHWC), _io(1, y_ka=-1.0)),
    ((3, 7, 7, 64, NHWC), _io(0, x_codes=1)),                              # the pool reads float32
    ((3, 7, 7, 64, NHWC), _io(2)),
])
def test_refusals(args, io):
    assert _ok(*args, io) == 0


def test_null_io_is_refused():
    L = _lib.load()
    assert L.slfp_global_avgpool_supported(3, 7, 7, 64, NHWC, None) == 0
    assert L.slfp_global_avgpool_f32(16, 16, 3, 7, 7, 64, NHWC, 0, None, None) == _lib.ERR_BAD_ARG


def test_refused_before_any_device_work():
    # the pointers are never dereferenced and no launch is made: the refusal comes first (this machine may have no GPU)
    L = _lib.load()
    io = _io()

    def call(x, y, n, h, w, c, layout, relu=0, io=io):
        return L.slfp_global_avgpool_f32(x, y, n, h, w, c, layout, relu, ctypes.byref(io), None)

    assert call(None, 16, 3, 7, 7, 64, NHWC) == _lib.ERR_BAD_ARG
    assert "null pointer" in _lib.last_error()
    assert call(16, None, 3, 7, 7, 64, NHWC) == _lib.ERR_BAD_ARG
    assert call(16, 24, 3, 7, 7, 64, NHWC) == _lib.ERR_ALIGNMENT      # NHWC: 16 bytes
    assert "16-byte" in _lib.last_error()
    assert call(24, 16, 3, 7, 7, 64, NHWC) == _lib.ERR_ALIGNMENT
    assert call(16, 18, 3, 7, 7, 10, NCHW) == _lib.ERR_ALIGNMENT      # NCHW: 4 bytes
    assert "4-byte" in _lib.last_error()
    assert call(16, 16, 3, 0, 7, 64, NHWC) == _lib.ERR_SHAPE
    assert call(16, 16, 3, 7, 7, 10, NHWC) == _lib.ERR_UNSUPPORTED
    assert "slfp_global_avgpool_supported" in _lib.last_error()
    assert call(16, 16, 3, 7, 7, 10, NCHW, io=_io(1)) == _lib.ERR_UNSUPPORTED
    assert call(16, 16, 3, 7, 7, 64, 5) == _lib.ERR_BAD_ARG
    assert call(16, 16, 3, 7, 7, 64, NHWC, relu=2) == _lib.ERR_BAD_ARG
    assert call(16, 16, 3, 7, 7, 64, NHWC, io=_io(1, y_qbits=6)) == _lib.ERR_BAD_ARG
    assert call(16, 16, 0, 7, 7, 64, NHWC) == _lib.OK                 # n == 0: nothing to do


class _Head(nn.Module):
    def __init__(self):
        super().__init__()
        Conv, Lin = cf.conv2d_Q(8, 0.02, 0.25), cf.linear_Q(8, 0.02, 0.25)
        self.features = nn.Sequential(Conv(3, 64, 3, padding=1), nn.BatchNorm2d(64), nn.ReLU())
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.flatten = nn.Flatten()
        self.fc = Lin(64, 16)

    def forward(self, x):
        return self.fc(self.flatten(self.avgpool(self.features(x))))


def test_passes_on_a_cpu_model_change_nothing():
    model = _Head().eval()
    slots = {name: mod for name, mod in model.named_modules()}
    x = torch.zeros(2, 3, 8, 8)
    assert fusion.use_device_avgpool(model, x) == 0
    assert fusion.link_pool_head(model, x) == 0
    assert {name: mod for name, mod in model.named_modules()} == slots
    assert model.fc._code_in is False
    assert fusion.unlink_pool_head(model) == 0 and fusion.restore_avgpool(model) == 0
    assert {name: mod for name, mod in model.named_modules()} == slots


@pytest.mark.parametrize("pool", [nn.AdaptiveAvgPool2d(1), nn.AdaptiveAvgPool2d((1, 1)), nn.AvgPool2d(5), nn.AvgPool2d(2),
                                  nn.AdaptiveAvgPool2d(2)])
def test_wrapper_on_a_cpu_tensor_is_the_module(pool):
    wrap = fusion.GlobalAvgPool2d(pool.eval())
    assert wrap.mod is pool and wrap._code_out is None and wrap._relu is False and wrap._last_kernel is None
    assert not wrap.training and list(wrap.state_dict()) == []
    x = torch.randn(3, 8, 5, 5)
    with torch.no_grad():
        assert torch.equal(wrap(x), pool(x))
    assert wrap._last_kernel == "aten"
    xg = x.clone().requires_grad_(True)
    y = wrap(xg)                                  # grad enabled: the ATen module, differentiable
    assert torch.equal(y, pool(x)) and y.requires_grad
    wrap._relu = True                             # a folded ReLU is applied on the ATen path too
    with torch.no_grad():
        assert torch.equal(wrap(x), pool(torch.relu(x)))


def test_candidates():
    assert fusion._avgpool_candidate(nn.AdaptiveAvgPool2d(1)) and fusion._avgpool_candidate(nn.AdaptiveAvgPool2d((1, 1)))
    assert not fusion._avgpool_candidate(nn.AdaptiveAvgPool2d(2)) and not fusion._avgpool_candidate(nn.AdaptiveAvgPool2d((1, None)))
    assert fusion._avgpool_candidate(nn.AvgPool2d(7)) and fusion._avgpool_candidate(nn.AvgPool2d(7, count_include_pad=False))
    assert not fusion._avgpool_candidate(nn.AvgPool2d(7, padding=1)) and not fusion._avgpool_candidate(nn.AvgPool2d(7, ceil_mode=True))
    assert not fusion._avgpool_candidate(nn.AvgPool2d(7, divisor_override=3)) and not fusion._avgpool_candidate(nn.MaxPool2d(7))
    x = torch.zeros(1, 4, 7, 7)
    assert fusion._avgpool_global(nn.AvgPool2d(7), x) and not fusion._avgpool_global(nn.AvgPool2d(3), x)
    assert fusion._avgpool_global(nn.AvgPool2d((7, 7)), x) and not fusion._avgpool_global(nn.AvgPool2d((7, 1)), x)
