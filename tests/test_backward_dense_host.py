"""CPU: the host side of the dense backward family (slfp_conv2d_bwd_*_ex with SLFP_BWD_DENSE): flags == 0 is the old API,
which layers the flag adds, workspace sizes (xq is never materialised) and the argument checks.  No compute call is made."""
import ctypes

import pytest

from cnns_slfp_quantization_amd import _lib, layer_specs
from cnns_slfp_quantization_amd import conv2d_func as cf

DENSE = _lib.BWD_DENSE
NEEDS = ((1, 1), (1, 0), (0, 1))
MiB = 1 << 20


def _desc(spec, n=2, x_layout=_lib.LAYOUT_NHWC, y_layout=_lib.LAYOUT_NHWC, qbits=8):
    return _lib.ConvDesc(n=n, c_in=spec.c_in, h=spec.h, w=spec.w, c_out=spec.c_out, kh=spec.k[0], kw=spec.k[1],
                         stride_h=spec.stride[0], stride_w=spec.stride[1], pad_h=spec.pad[0], pad_w=spec.pad[1],
                         dil_h=1, dil_w=1, groups=spec.groups, x_layout=x_layout, y_layout=y_layout, qbits=qbits,
                         ka=float(spec.Ka), kw_scale=float(spec.Kw), mfma_passes=0, reserved=0)


def _nchw(spec, **kw):
    return _desc(spec, x_layout=_lib.LAYOUT_NCHW, y_layout=_lib.LAYOUT_NCHW, **kw)


def _is_pw(s):
    return s.k == (1, 1) and s.groups == 1 and s.stride == (1, 1) and s.pad == (0, 0)


def _dense_layers(net):
    return [s for s in layer_specs.conv_layers(net) if s.groups == 1 and not _is_pw(s)]


@pytest.mark.parametrize("net", sorted(layer_specs.nets()))
def test_flags_zero_is_the_old_api(net):
    L = _lib.load()
    for spec in layer_specs.conv_layers(net):
        for d in (_desc(spec), _nchw(spec)):
            r = ctypes.byref(d)
            assert L.slfp_conv2d_bwd_supported_ex(r, 0) == L.slfp_conv2d_bwd_supported(r)
            assert L.slfp_conv2d_bwd_kernel_name_ex(r, 0) == L.slfp_conv2d_bwd_kernel_name(r)
            for gx, gw in NEEDS:
                assert L.slfp_conv2d_bwd_workspace_bytes_ex(r, 0, gx, gw) == L.slfp_conv2d_bwd_workspace_bytes(r, gx, gw)


@pytest.mark.parametrize("net", sorted(layer_specs.nets()))
def test_dense_flag_names_every_layer(net):
    L = _lib.load()
    for spec in layer_specs.conv_layers(net):
        r = ctypes.byref(_desc(spec))
        old = L.slfp_conv2d_bwd_kernel_name(r).decode()
        new = L.slfp_conv2d_bwd_kernel_name_ex(r, DENSE).decode()
        assert L.slfp_conv2d_bwd_supported_ex(r, DENSE) == (new != "composite")
        if old != "composite":
            assert new == old, (net, spec)                       # depthwise and pointwise keep their kernels
        elif spec.groups == 1:
            assert new == "dense_bwd_mfma_f32", (net, spec, new)
        assert spec.groups != 1 or new != "composite"
        if spec.groups == 1 and not _is_pw(spec):
            assert new == "dense_bwd_mfma_f32", (net, spec, new)


def test_nothing_in_any_net_is_left_on_the_composite():
    L = _lib.load()
    left = [(net, s) for net in sorted(layer_specs.nets()) for s in layer_specs.conv_layers(net)
            if L.slfp_conv2d_bwd_kernel_name_ex(ctypes.byref(_desc(s, n=128)), DENSE) == b"composite"]
    assert not left, left


def test_resnet_downsamples_and_stems_are_dense():
    L = _lib.load()
    ds = [s for s in layer_specs.conv_layers("resnet50_imagenet224") if s.k == (1, 1) and s.stride == (2, 2)]
    assert len({(s.c_in, s.c_out, s.h) for s in ds}) == 3
    stems = {(s.c_out, s.k, s.stride, s.pad, s.h) for net in layer_specs.nets() for s in layer_specs.conv_layers(net) if s.c_in == 3}
    assert len(stems) >= 6, stems
    for s in ds + [s for net in sorted(layer_specs.nets()) for s in layer_specs.conv_layers(net) if s.c_in == 3]:
        assert L.slfp_conv2d_bwd_kernel_name_ex(ctypes.byref(_desc(s)), DENSE) == b"dense_bwd_mfma_f32", s
        assert L.slfp_conv2d_bwd_kernel_name(ctypes.byref(_desc(s))) == b"composite", s


@pytest.mark.parametrize("net", sorted(layer_specs.nets()))
def test_workspace_sizes_hold_no_activation_sized_term(net):
    """NHWC: wq (OIHW and tap-major, at most 9.4 MB each) + partials capped at 32 MiB.  A float32 xq of VGG-16's first
    layers at n = 128 would be 1.6 GB, so the 64 MiB bound is what keeps xq from being materialised."""
    L = _lib.load()
    for spec in _dense_layers(net):
        nhwc, nchw = _desc(spec, n=128), _nchw(spec, n=128)
        for gx, gw in NEEDS:
            a = L.slfp_conv2d_bwd_workspace_bytes_ex(ctypes.byref(nhwc), DENSE, gx, gw)
            b = L.slfp_conv2d_bwd_workspace_bytes_ex(ctypes.byref(nchw), DENSE, gx, gw)
            assert 0 < a < 64 * MiB, (spec, gx, gw, a)
            assert b > a, (spec, gx, gw, a, b)
            assert a % 256 == 0 and b % 256 == 0
        big = _desc(spec, n=4096)
        assert 0 < L.slfp_conv2d_bwd_workspace_bytes_ex(ctypes.byref(big), DENSE, 0, 1) < 64 * MiB, spec


def _dense_spec():
    return layer_specs.ConvSpec(16, 32, (3, 3), (1, 1), (1, 1), 1, False, 14, 14, 14, 14, 0.2, 0.1)


def test_refusals_under_the_flag():
    L = _lib.load()

    def refused(d):
        r = ctypes.byref(d) if d is not None else None
        return (not L.slfp_conv2d_bwd_supported_ex(r, DENSE) and L.slfp_conv2d_bwd_kernel_name_ex(r, DENSE) == b"composite"
                and L.slfp_conv2d_bwd_workspace_bytes_ex(r, DENSE, 1, 1) == 0)

    ok = _desc(_dense_spec())
    assert L.slfp_conv2d_bwd_supported_ex(ctypes.byref(ok), DENSE)
    d = _desc(_dense_spec()); d.groups = 2
    assert refused(d)
    d = _desc(_dense_spec()); d.dil_h = d.dil_w = 2
    assert refused(d)
    d = _desc(_dense_spec()); d.dil_w = 2
    assert refused(d)
    d = _desc(_dense_spec()); d.qbits = 32
    assert refused(d)
    d = _desc(_dense_spec()); d.ka = -1.0
    assert refused(d)
    assert refused(None)
    # an unknown flag bit
    r = ctypes.byref(ok)
    fake = 1 << 20
    for flags in (2, DENSE | 2, 1 << 31):
        assert not L.slfp_conv2d_bwd_supported_ex(r, flags)
        assert L.slfp_conv2d_bwd_kernel_name_ex(r, flags) == b"composite"
        assert L.slfp_conv2d_bwd_workspace_bytes_ex(r, flags, 1, 1) == 0
        assert L.slfp_conv2d_bwd_ex(r, flags, fake, fake, fake, fake, fake, None, fake, None) == _lib.ERR_BAD_ARG
        assert "flag" in _lib.last_error()
    # without the flag the dense descriptor is not covered
    assert L.slfp_conv2d_bwd_ex(r, 0, fake, fake, fake, fake, fake, None, fake, None) == _lib.ERR_UNSUPPORTED
    assert L.slfp_conv2d_bwd(r, fake, fake, fake, fake, fake, None, fake, None) == _lib.ERR_UNSUPPORTED


def test_bad_arguments_return_error_codes_on_a_dense_descriptor():
    """Every check that precedes device work: no pointer here is dereferenced."""
    L = _lib.load()
    d = _desc(_dense_spec())
    r = ctypes.byref(d)
    fake = 1 << 20                                                   # 16-byte aligned, never touched
    bwd = L.slfp_conv2d_bwd_ex
    assert bwd(None, DENSE, fake, fake, fake, fake, fake, None, fake, None) == _lib.ERR_BAD_ARG
    assert bwd(r, DENSE, fake, fake, None, fake, fake, None, fake, None) == _lib.ERR_BAD_ARG   # no gy
    assert bwd(r, DENSE, fake, None, fake, fake, None, None, fake, None) == _lib.ERR_BAD_ARG   # gx, no w
    assert bwd(r, DENSE, None, fake, fake, None, fake, None, fake, None) == _lib.ERR_BAD_ARG   # gw, no x
    assert bwd(r, DENSE, fake, fake, fake, None, None, fake, fake, None) == _lib.ERR_BAD_ARG   # gb, no gw
    assert bwd(r, DENSE, fake + 4, fake, fake, fake, fake, None, fake, None) == _lib.ERR_ALIGNMENT
    assert bwd(r, DENSE, fake, fake, fake, fake, fake, None, None, None) == _lib.ERR_BAD_ARG   # no workspace
    assert "workspace" in _lib.last_error()
    bad = _desc(_dense_spec()); bad.dil_h = bad.dil_w = 2
    assert bwd(ctypes.byref(bad), DENSE, fake, fake, fake, fake, fake, None, fake, None) == _lib.ERR_UNSUPPORTED
    bad = _desc(_dense_spec()); bad.groups = 2
    assert bwd(ctypes.byref(bad), DENSE, fake, fake, fake, fake, fake, None, fake, None) == _lib.ERR_UNSUPPORTED
    bad = _desc(_dense_spec()); bad.n = 0
    assert bwd(ctypes.byref(bad), DENSE, fake, fake, fake, fake, fake, None, fake, None) == _lib.ERR_SHAPE
    bad = _desc(_dense_spec()); bad.qbits = 5
    assert bwd(ctypes.byref(bad), DENSE, fake, fake, fake, fake, fake, None, fake, None) == _lib.ERR_BAD_ARG
    # nothing requested: nothing to do
    assert bwd(r, DENSE, fake, fake, fake, None, None, None, None, None) == _lib.OK


def test_backward_option_hip_all():
    assert cf.options.backward == "composite"                        # the default is unchanged
    with pytest.raises(ValueError):
        cf.options.backward = "fast"
    assert cf.options.backward == "composite"
    cf.options.backward = "hip_all"
    try:
        assert cf.options.backward == "hip_all"
    finally:
        cf.options.backward = "composite"
