"""CPU: the host side of the HIP backward (slfp_conv2d_bwd_*): which layers it covers, its workspace sizes and its argument
checks.  No compute call is made here."""
import ctypes

import pytest
import torch

from cnns_slfp_quantization_amd import _lib, layer_specs
from cnns_slfp_quantization_amd import conv2d_func as cf


def _desc(spec, n=2, x_layout=_lib.LAYOUT_NHWC, y_layout=_lib.LAYOUT_NHWC, qbits=8):
    return _lib.ConvDesc(n=n, c_in=spec.c_in, h=spec.h, w=spec.w, c_out=spec.c_out, kh=spec.k[0], kw=spec.k[1],
                         stride_h=spec.stride[0], stride_w=spec.stride[1], pad_h=spec.pad[0], pad_w=spec.pad[1],
                         dil_h=1, dil_w=1, groups=spec.groups, x_layout=x_layout, y_layout=y_layout, qbits=qbits,
                         ka=float(spec.Ka), kw_scale=float(spec.Kw), mfma_passes=0, reserved=0)


def _expected(spec):
    if (spec.groups == spec.c_in == spec.c_out and spec.k == (3, 3) and spec.stride[0] == spec.stride[1]
            and spec.stride[0] in (1, 2) and spec.pad == (1, 1)):
        return "dw3x3_bwd"
    if spec.k == (1, 1) and spec.groups == 1 and spec.stride == (1, 1) and spec.pad == (0, 0):
        return "pw_bwd_mfma_f32"
    return "composite"


@pytest.mark.parametrize("net", sorted(layer_specs.nets()))
def test_kernel_name_per_layer(net):
    L = _lib.load()
    for spec in layer_specs.conv_layers(net):
        d = _desc(spec)
        name = L.slfp_conv2d_bwd_kernel_name(ctypes.byref(d)).decode()
        assert name == _expected(spec), (net, spec, name)
        assert bool(L.slfp_conv2d_bwd_supported(ctypes.byref(d))) == (name != "composite")


@pytest.mark.parametrize("net", ["mobilenetv1_imagenet224", "mobilenetv1_cifar32"])
def test_mobilenet_non_stem_layers_all_covered(net):
    L = _lib.load()
    layers = layer_specs.conv_layers(net)[1:]
    assert len(layers) == 26
    for spec in layers:
        assert L.slfp_conv2d_bwd_supported(ctypes.byref(_desc(spec, n=128))), spec


@pytest.mark.parametrize("net", ["mobilenetv1_imagenet224", "mobilenetv1_cifar32", "shufflenetv2_224"])
def test_workspace_sizes(net):
    L = _lib.load()
    for spec in layer_specs.conv_layers(net):
        if _expected(spec) == "composite":
            continue
        nhwc = _desc(spec, n=128)
        nchw = _desc(spec, n=128, x_layout=_lib.LAYOUT_NCHW, y_layout=_lib.LAYOUT_NCHW)
        for gx, gw in ((1, 1), (1, 0), (0, 1)):
            a = L.slfp_conv2d_bwd_workspace_bytes(ctypes.byref(nhwc), gx, gw)
            b = L.slfp_conv2d_bwd_workspace_bytes(ctypes.byref(nchw), gx, gw)
            assert 0 <= a < 64 << 20, (spec, a)            # wq + partials: a few tens of MB at most
            assert b > a, (spec, gx, gw, a, b)              # NCHW adds the transposed copies
            assert a % 256 == 0 and b % 256 == 0
        # partial sums are capped at 32 MiB however large the layer
        big = _desc(spec, n=4096)
        assert L.slfp_conv2d_bwd_workspace_bytes(ctypes.byref(big), 0, 1) < 40 << 20


def test_uncovered_and_invalid_descriptors():
    L = _lib.load()
    spec = layer_specs.conv_layers("mobilenetv1_cifar32")[1]        # 3x3 depthwise
    d = _desc(spec)
    d.dil_h = d.dil_w = 2
    assert not L.slfp_conv2d_bwd_supported(ctypes.byref(d))
    assert L.slfp_conv2d_bwd_kernel_name(ctypes.byref(d)) == b"composite"
    assert L.slfp_conv2d_bwd_workspace_bytes(ctypes.byref(d), 1, 1) == 0
    d = _desc(spec)
    d.qbits = 32
    assert not L.slfp_conv2d_bwd_supported(ctypes.byref(d))
    d = _desc(spec)
    d.ka = -1.0
    assert not L.slfp_conv2d_bwd_supported(ctypes.byref(d))
    assert not L.slfp_conv2d_bwd_supported(None)
    assert L.slfp_conv2d_bwd_kernel_name(None) == b"composite"
    pw = _desc(layer_specs.conv_layers("mobilenetv1_cifar32")[2])
    pw.stride_h = pw.stride_w = 2                                   # strided 1x1: composite
    assert L.slfp_conv2d_bwd_kernel_name(ctypes.byref(pw)) == b"composite"


def test_bad_arguments_return_error_codes():
    """Every check that precedes device work: no pointer here is dereferenced."""
    L = _lib.load()
    spec = layer_specs.conv_layers("mobilenetv1_cifar32")[1]
    d = _desc(spec)
    fake = 1 << 20                                                   # 16-byte aligned, never touched
    assert L.slfp_conv2d_bwd(None, fake, fake, fake, fake, fake, None, fake, None) == _lib.ERR_BAD_ARG
    assert L.slfp_conv2d_bwd(ctypes.byref(d), fake, fake, None, fake, fake, None, fake, None) == _lib.ERR_BAD_ARG   # no gy
    assert L.slfp_conv2d_bwd(ctypes.byref(d), fake, None, fake, fake, None, None, fake, None) == _lib.ERR_BAD_ARG   # gx, no w
    assert L.slfp_conv2d_bwd(ctypes.byref(d), None, fake, fake, None, fake, None, fake, None) == _lib.ERR_BAD_ARG   # gw, no x
    assert L.slfp_conv2d_bwd(ctypes.byref(d), fake, fake, fake, None, None, fake, fake, None) == _lib.ERR_BAD_ARG   # gb, no gw
    assert L.slfp_conv2d_bwd(ctypes.byref(d), fake + 4, fake, fake, fake, fake, None, fake, None) == _lib.ERR_ALIGNMENT
    assert L.slfp_conv2d_bwd(ctypes.byref(d), fake, fake, fake, fake, fake, None, None, None) == _lib.ERR_BAD_ARG   # no workspace
    assert "workspace" in _lib.last_error()
    bad = _desc(spec)
    bad.dil_h = bad.dil_w = 2
    assert L.slfp_conv2d_bwd(ctypes.byref(bad), fake, fake, fake, fake, fake, None, fake, None) == _lib.ERR_UNSUPPORTED
    bad = _desc(spec)
    bad.n = 0
    assert L.slfp_conv2d_bwd(ctypes.byref(bad), fake, fake, fake, fake, fake, None, fake, None) == _lib.ERR_SHAPE
    bad = _desc(spec)
    bad.qbits = 5
    assert L.slfp_conv2d_bwd(ctypes.byref(bad), fake, fake, fake, fake, fake, None, fake, None) == _lib.ERR_BAD_ARG
    # nothing requested: nothing to do
    assert L.slfp_conv2d_bwd(ctypes.byref(d), fake, fake, fake, None, None, None, None, None) == _lib.OK


def test_backward_option():
    assert cf.options.backward == "composite"                        # the default is unchanged
    with pytest.raises(ValueError):
        cf.options.backward = "fast"
    assert cf.options.backward == "composite"
    cf.options.backward = "hip"
    try:
        assert cf.options.backward == "hip"
    finally:
        cf.options.backward = "composite"
    m = cf.conv2d_Q(8, 0.1, 0.2)(8, 8, 3, padding=1, groups=8)
    assert m._last_bwd_kernel is None
    assert cf.linear_Q(8, 0.1, 0.2)(8, 4)._last_bwd_kernel is None
