"""CPU: the host side of the weight-streaming Linear_Q kernel: slfp_linear_fc_supported /
slfp_linear_fc_workspace_bytes / slfp_linear_fwd_fc, `options.linear_kernel`, the uint8 guard of Linear_Q and fusion.link_head on a
model without a device.  No device work is done here: the library loads without a GPU and every query is host only."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

from cnns_slfp_quantization_amd import _lib, fusion
from cnns_slfp_quantization_amd import conv2d_func as cf

NEW = ("slfp_linear_fc_supported", "slfp_linear_fc_workspace_bytes", "slfp_linear_fwd_fc")


def _io(x_codes=0, y_codes=0, y_ka=0.3, y_qbits=8):
    return _lib.ConvIo(x_codes=x_codes, y_codes=y_codes, y_ka=y_ka, y_qbits=y_qbits)


def _ok(batch, in_f, out_f, qbits=8, passes=_lib.MFMA_DEFAULT, io=None, relu=0):
    io = io if io is not None else _io()
    return _lib.load().slfp_linear_fc_supported(batch, in_f, out_f, qbits, passes, ctypes.byref(io), 1, relu)


def test_new_symbols_are_exported_and_declared():
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "slfp.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert hasattr(L, name)
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, header), name
    assert "utils/conv2d_func.py:60-65" in header[header.index("csrc/linear_fc.hip"):]
    assert L.slfp_version() == 1   # SLFP_ABI_VERSION: new exports only


def test_supported_shapes():
    assert _ok(5, 96, 100) == 1                                           # float32 in and out, a ragged last n-tile
    assert _ok(17, 320, 272, io=_io(1, 1), relu=1) == 1                   # codes in and out
    assert _ok(17, 320, 272, qbits=7, io=_io(1, 1, y_qbits=8)) == 1       # a reader with the other q_bit
    assert _ok(1, 9216, 4096, passes=_lib.MFMA_F16X1) == 1
    assert _ok(256, 25088, 4096, qbits=7, passes=_lib.MFMA_F16X3) == 1    # SFP<3,3> is exact in fp16: one pass whatever the mode


@pytest.mark.parametrize("kw", [
    dict(in_f=320, out_f=272, passes=_lib.MFMA_F16X3),        # the float32-equivalent mode at q_bit 8
    dict(in_f=48, out_f=272),                                 # K is not whole k-steps
    dict(in_f=320, out_f=18),                                 # N is not whole float4s
    dict(in_f=320, out_f=100, io=_io(0, 1)),                  # code output needs whole n-tiles
    dict(in_f=320, out_f=272, qbits=6),
    dict(in_f=320, out_f=272, io=_io(1, 1, y_ka=0.0)),
    dict(in_f=320, out_f=272, io=_io(1, 1, y_ka=-1.0)),
    dict(in_f=320, out_f=272, io=_io(1, 1, y_qbits=6)),
    dict(in_f=320, out_f=272, relu=2),                        # SLFP_POST_LAYEROUT is no flag of this entry point
])
def test_refusals(kw):
    assert _ok(17, **kw) == 0


def test_refused_before_any_device_work():
    # never dereferenced: the refusal comes first
    L = _lib.load()
    io = _io()
    rc = L.slfp_linear_fwd_fc(16, 16, None, 16, 17, 48, 272, 0.25, 0.02, 8, 0, ctypes.byref(io), 0, 16, None)
    assert rc == _lib.ERR_UNSUPPORTED
    assert "slfp_linear_fc_supported" in _lib.last_error()
    rc = L.slfp_linear_fwd_fc(16, 16, None, 16, 17, 320, 272, 0.25, 0.02, 8, _lib.MFMA_F16X3, ctypes.byref(io), 0, 16, None)
    assert rc == _lib.ERR_UNSUPPORTED


def test_workspace_is_for_a_float32_input_only():
    L = _lib.load()
    assert L.slfp_linear_fc_workspace_bytes(17, 320, 272, ctypes.byref(_io(1, 0))) == 0
    assert L.slfp_linear_fc_workspace_bytes(17, 320, 272, ctypes.byref(_io(1, 1))) == 0
    n = L.slfp_linear_fc_workspace_bytes(17, 320, 272, ctypes.byref(_io(0, 0)))
    assert n >= 17 * 320 and n % 16 == 0


def test_linear_kernel_option():
    assert cf.options.linear_kernel == "pointwise"
    with pytest.raises(ValueError):
        cf.options.linear_kernel = "gemv"
    assert cf.options.linear_kernel == "pointwise"
    try:
        cf.options.linear_kernel = "fc"
        assert cf.options.linear_kernel == "fc"
    finally:
        cf.options.linear_kernel = "pointwise"


def test_unmarked_uint8_input_raises():
    lin = cf.linear_Q(8, 0.02, 0.25)(64, 16).eval()
    assert lin._code_in is False and lin._code_out is None and lin._code_relu is False
    with torch.no_grad(), pytest.raises(TypeError):
        lin(torch.zeros(2, 64, dtype=torch.uint8))


def test_link_head_on_a_cpu_model_makes_no_links():
    Lin = cf.linear_Q(8, 0.02, 0.25)
    model = nn.Sequential(Lin(64, 32), nn.ReLU(), nn.Dropout(), Lin(32, 16)).eval()
    slots = list(model._modules.values())
    assert fusion.link_head(model, torch.zeros(2, 64)) == 0
    assert list(model._modules.values()) == slots
    for m in (model[0], model[3]):
        assert m._code_in is False and m._code_out is None and m._code_relu is False and "_head_link" not in m.__dict__
    assert fusion.unlink_head(model) == 0
