"""CPU: the host side of the byte-input image stems: the four exports, what slfp_conv2d_u8_supported accepts and
refuses and what slfp_conv2d_fwd_u8 answers before any device work, the reporter strings of tests/_image_u8_cases.py, the first layers
of the seven reference nets, image_u8.pixel_table against the written-out torchvision and IEEE expressions, and the bookkeeping of
fusion.link_image_u8 / unlink_image_u8.  Every pointer handed to the library here is refused before it would be dereferenced."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

from _image_u8_cases import (CIFAR_MEAN, CIFAR_STD, IMAGENET_MEAN, IMAGENET_STD, KA_NORM, ROWS, u8_instance, u8_supported)
from _stem_variants import KA, KA_NEXT, KW, make_desc, set_switches
from cnns_slfp_quantization_amd import _lib, fusion, image_u8, layer_specs
from cnns_slfp_quantization_amd import conv2d_func as cf

EXPORTS = ("slfp_conv2d_u8_supported", "slfp_conv2d_fwd_u8", "slfp_debug_stem_u8_instance", "slfp_image_u8_expand_f32")


def test_the_four_exports_exist():
    L = _lib.load()
    assert L.slfp_version() == 1                      # SLFP_ABI_VERSION stays 1
    for name in EXPORTS:
        assert name in _lib.SYMBOLS and getattr(L, name) is not None
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "slfp.h")).read()
    for name in EXPORTS:
        assert name + "(" in header


def _desc(c_in=3, c_out=32, k=3, s=2, p=1, hw=(33, 36), n=2, qbits=8, passes=0, groups=1, dil=1, x_layout=_lib.LAYOUT_NHWC,
          y_layout=_lib.LAYOUT_NHWC, ka=KA):
    return _lib.ConvDesc(n=n, c_in=c_in, h=hw[0], w=hw[1], c_out=c_out, kh=k, kw=k, stride_h=s, stride_w=s, pad_h=p, pad_w=p, dil_h=dil,
                         dil_w=dil, groups=groups, x_layout=x_layout, y_layout=y_layout, qbits=qbits, ka=float(np.float32(ka)),
                         kw_scale=float(np.float32(KW)), mfma_passes=passes, reserved=0)


def _io(x_codes=0, y_codes=1, y_qbits=8, y_ka=KA_NEXT):
    return _lib.ConvIo(x_codes=x_codes, y_codes=y_codes, y_ka=float(np.float32(y_ka)), y_qbits=y_qbits)


def _ok(d, io=None, flags=0, bias=0):
    return _lib.load().slfp_conv2d_u8_supported(ctypes.byref(d), ctypes.byref(io) if io is not None else None, bias, flags)


def _name(d, io=None, flags=0, bias=0, post=0):
    return _lib.load().slfp_debug_stem_u8_instance(ctypes.byref(d), ctypes.byref(io) if io is not None else None, bias, flags, post).decode()


def _call(d, io=None, flags=0, x=4096 + 1, pix=4096, y=8192, wprep=16384, post=None):
    """slfp_conv2d_fwd_u8 with made-up addresses (x at an odd one): only ever used where the call must be refused before device work"""
    return _lib.load().slfp_conv2d_fwd_u8(ctypes.byref(d), ctypes.byref(io) if io is not None else None, x, pix, wprep, None, post, post,
                                          flags, y, None, None)


# one accepted descriptor per family: (descriptor arguments, family word)
FAMILIES = ((dict(), "stem"), (dict(c_out=64, s=1, hw=(9, 35)), "small"), (dict(c_out=64, k=7, p=3, hw=(20, 70)), "rows"),
            (dict(c_out=64, k=11, s=4, p=2, hw=(35, 51)), "im2row"))


@pytest.mark.parametrize("kw, word", FAMILIES, ids=[w for _, w in FAMILIES])
def test_controls_and_refusals(kw, word):
    L = _lib.load()
    set_switches(L, None)
    d = _desc(**kw)
    assert _ok(d) == 1 and _ok(d, _io(0, 0)) == 1 and _name(d).startswith(word) and "/u8/" in _name(d)
    assert _ok(d, _io(0, 1), 1) == 1 and _name(d, _io(0, 1), 1).endswith("/u8/yc") and _name(d, _io(0, 1), 0).endswith("/u8/yc-signed")
    assert _ok(d, None, 2) == 1 and _ok(d, None, 3) == 1            # the layer-output quantizer with float32 out
    refused = {
        "x_codes": (d, _io(1, 0), 0), "x_codes + y_codes": (d, _io(1, 1), 1),
        "layerout with codes out": (d, _io(0, 1), 2), "layerout + relu with codes out": (d, _io(0, 1), 3),
        "unknown flag": (d, None, 4),
        "nchw in": (_desc(x_layout=_lib.LAYOUT_NCHW, **kw), None, 0), "nchw out": (_desc(y_layout=_lib.LAYOUT_NCHW, **kw), None, 0),
        "f16x3 at qbits 8": (_desc(passes=_lib.MFMA_F16X3, **kw), None, 0),
        "bad reader format": (d, _io(0, 1, y_qbits=5), 1), "bad reader scale": (d, _io(0, 1, y_ka=0.0), 1),
    }
    for why, (dd, io, flags) in refused.items():
        assert _ok(dd, io, flags) == 0, why
        assert _name(dd, io, flags, 0, 1) == "none", why
        assert _call(dd, io, flags, post=32768 if flags & 2 else None) == _lib.ERR_UNSUPPORTED, (why, _lib.last_error())
    # NULL operands: a bad argument, whatever else holds
    for nul in ("x", "pix", "y", "wprep"):
        assert _call(d, None, 0, **{nul: None}) == _lib.ERR_BAD_ARG, nul
    assert _lib.load().slfp_conv2d_fwd_u8(None, None, 1, 4096, 16384, None, None, None, 0, 8192, None, None) == _lib.ERR_BAD_ARG
    # alignment: pix_table and y at 16 bytes; x at any address
    assert _call(d, None, 0, pix=4096 + 4) == _lib.ERR_ALIGNMENT and _call(d, None, 0, y=8192 + 8) == _lib.ERR_ALIGNMENT


def test_layers_without_a_byte_form_are_refused():
    L = _lib.load()
    set_switches(L, None)
    cases = {
        "groups 2": _desc(c_in=4, c_out=32, groups=2),
        "c_in 5": _desc(c_in=5, c_out=32),
        "c_in 8 dense": _desc(c_in=8, c_out=32, s=1),
        "k_direct (dilation 2)": _desc(dil=2, p=2),
        "k_direct (c_out 12)": _desc(c_out=12, k=4, s=1, qbits=7),
        "k_stem generic (stride 3)": _desc(s=3, hw=(25, 50), p=0, passes=0, k=4, qbits=7),
        "k_stem generic (4x4x3, K = 48)": _desc(k=4, s=1, hw=(10, 19), qbits=7),
        "pointwise": _desc(c_in=4, c_out=32, k=1, s=1, p=0),
    }
    for why, d in cases.items():
        assert _ok(d) == 0 and _ok(d, _io(0, 1), 1) == 0 and _name(d) == "none", why
        assert _call(d) == _lib.ERR_UNSUPPORTED, why
    # each of them is a layer the float32 interface runs on k_direct / k_stem (or another family altogether)
    for why in ("k_direct (dilation 2)", "k_direct (c_out 12)"):
        assert L.slfp_debug_stem_instance(ctypes.byref(cases[why]), None, 0, 0, 0).decode().startswith("direct/"), why
    for why in ("k_stem generic (stride 3)", "k_stem generic (4x4x3, K = 48)"):
        assert L.slfp_debug_stem_instance(ctypes.byref(cases[why]), None, 0, 0, 0).decode().startswith("stem/gen/"), why
    try:   # k_stem_fixed without a threshold table (the long-form quantizer forced): no byte form
        set_switches(L, {"SLFP_LONG_ENCODE": "1"})
        d = _desc()
        assert L.slfp_debug_stem_instance(ctypes.byref(d), None, 0, 0, 0).decode() == "stem/fixed/act8/long"
        assert _ok(d) == 0 and _name(d) == "none" and _call(d) == _lib.ERR_UNSUPPORTED
    finally:
        set_switches(L, None)


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_every_row_is_accepted_and_reports_its_instance(row):
    L = _lib.load()
    try:
        for ka in (KA, KA_NORM):
            set_switches(L, row.env)
            d = make_desc(_lib, row, ka, KW)
            assert u8_supported(_lib, d, row, KA_NEXT) == 1, row
            assert u8_instance(_lib, d, row, KA_NEXT) == row.variant, row
        # under no switch is it another family: the vector-ALU switch leaves the string alone, the im2row switch moves rows to im2row only
        d = make_desc(_lib, row, KA, KW)
        set_switches(L, {"SLFP_STEM_OLD": "1"})
        assert u8_instance(_lib, d, row, KA_NEXT) == (row.variant if not dict(row.env) else row.variant.replace("im2row", "rows", 1)), row
        set_switches(L, {"SLFP_STEM_IM2ROW": "1"})
        assert u8_instance(_lib, d, row, KA_NEXT) == row.variant.replace("rows/", "im2row/", 1), row
        set_switches(L, {"SLFP_LONG_ENCODE": "1"})   # code output and k_stem_fixed need the threshold tables: refused, never another kernel
        got = u8_instance(_lib, d, row, KA_NEXT)
        assert got in (row.variant.replace("im2row", "rows", 1) if dict(row.env) else row.variant, "none"), (row, got)
        assert (got == "none") == (u8_supported(_lib, d, row, KA_NEXT) == 0)
    finally:
        set_switches(L, None)


def test_the_table_names_each_kernel_and_output_form():
    heads = {"/".join(r.variant.split("/u8/")[0].split("/")[:1]) for r in ROWS}
    assert heads == {"stem", "small", "rows", "im2row"}
    for head in heads:
        outs = {r.variant.rsplit("/", 1)[1] for r in ROWS if r.variant.startswith(head)}
        assert {"f32", "yc"} <= outs and (head == "im2row" or "yc-signed" in outs), (head, outs)
    assert any(r.n * r.h * r.w * r.c_in % 2 and (r.h * r.w * r.c_in) % 2 for r in ROWS)   # images at odd addresses


NETS = ("mobilenetv1_imagenet224", "mobilenetv1_cifar32", "vgg16_224", "shufflenetv2_224", "resnet50_imagenet224",
        "squeezenet1_0_imagenet224", "alexnet_imagenet224")


@pytest.mark.parametrize("net", NETS)
def test_first_layers_of_the_reference_nets(net):
    L = _lib.load()
    set_switches(L, None)
    s = layer_specs.conv_layers(net)[0]
    assert s.c_in == 3 and s.groups == 1
    for n in (1, 128):
        for qbits in (8, 7):
            d = _lib.ConvDesc(n=n, c_in=s.c_in, h=s.h, w=s.w, c_out=s.c_out, kh=s.k[0], kw=s.k[1], stride_h=s.stride[0], stride_w=s.stride[1],
                              pad_h=s.pad[0], pad_w=s.pad[1], dil_h=1, dil_w=1, groups=1, x_layout=_lib.LAYOUT_NHWC, y_layout=_lib.LAYOUT_NHWC,
                              qbits=qbits, ka=float(np.float32(s.Ka)), kw_scale=float(np.float32(s.Kw)), mfma_passes=0, reserved=0)
            assert _ok(d, None, 1, int(s.bias)) == 1, (net, n, qbits)
            name = _name(d, None, 1, int(s.bias), 1)
            assert "/u8/" in name, name
            f32 = L.slfp_debug_stem_instance(ctypes.byref(d), None, int(s.bias), 1, 1).decode()
            # the same instance family as the float32 interface -- but for k_stem_mx's geometry, which the byte entry sends to fixed/tab
            assert name.replace("/u8", "") == f32.replace("stem/mx/", "stem/fixed/tab/"), (name, f32)
            if n == 128:
                print(f"{net} qbits {qbits}: {f32} -> {name}")


def _torchvision_written_out(mean, std):
    """ToTensor() + Normalize(mean, std) on a [3, 7, 256] uint8 CPU image whose rows are the ramp, with torchvision's operations"""
    img = torch.arange(256, dtype=torch.uint8).repeat(3, 7, 1)
    t = img.to(torch.float32).div(255)
    m, s = torch.as_tensor(mean, dtype=torch.float32), torch.as_tensor(std, dtype=torch.float32)
    return t.sub_(m.view(-1, 1, 1)).div_(s.view(-1, 1, 1))


@pytest.mark.parametrize("mean, std", ((IMAGENET_MEAN, IMAGENET_STD), (CIFAR_MEAN, CIFAR_STD)), ids=("imagenet", "cifar"))
def test_pixel_table_is_torchvision_and_ieee(mean, std):
    p = image_u8.pixel_table(mean, std)
    assert p.dtype == torch.float32 and tuple(p.shape) == (3, 256) and p.device.type == "cpu" and p.is_contiguous()
    tv = _torchvision_written_out(mean, std)
    for row in range(7):
        assert torch.equal(tv[:, row, :].view(torch.int32), p.view(torch.int32))
    v = np.arange(256, dtype=np.float32)
    ieee = np.stack([((v / np.float32(255)) - np.float32(mean[c])) / np.float32(std[c]) for c in range(3)]).astype(np.float32)
    assert np.array_equal(ieee.view(np.uint32), p.numpy().view(np.uint32))
    assert len(np.unique(p.numpy())) == 768
    # the general form gives the same table from the same operations as a callable
    q = image_u8.pixel_table_from(lambda im: im.to(torch.float32).div(255).sub_(torch.tensor(mean).view(-1, 1, 1)).div_(torch.tensor(std).view(-1, 1, 1)), 3)
    assert torch.equal(q.view(torch.int32), p.view(torch.int32))
    with pytest.raises(ValueError):
        image_u8.pixel_table(mean, (0.2, 0.0, 0.2))
    with pytest.raises(ValueError):
        image_u8.pixel_table_from(lambda im: im.float()[:, :, :5], 3)


def _cpu_model(q_bit=32, c_in=3):
    C = cf.conv2d_Q_bias(q_bit=q_bit, Kw=0.02, Ka=0.3)
    return torch.nn.Sequential(C(c_in, 8, 3, 0.02, 0.3, 2, 1), torch.nn.ReLU(), C(8, 8, 1, 0.02, 0.3)).eval()


def test_link_bookkeeping_on_cpu_modules():
    table = image_u8.pixel_table(IMAGENET_MEAN, IMAGENET_STD)
    m = _cpu_model()
    keys = list(m.state_dict().keys())
    stem = m[0]
    assert stem._image_table is None and fusion.unlink_image_u8(m) == 0
    # the mark: a registered, non-persistent buffer
    fusion._mark_image_stem(stem, table)
    assert torch.equal(stem._image_table, table) and "_image_table" in dict(stem.named_buffers())
    assert list(m.state_dict().keys()) == keys and "_image_table" not in stem.state_dict()
    assert m[2]._image_table is None
    assert fusion.unlink_image_u8(m) == 1 and stem._image_table is None and fusion.unlink_image_u8(m) == 0
    assert list(m.state_dict().keys()) == keys
    # a table of another channel count, another shape or dtype is refused
    with pytest.raises(ValueError):
        fusion._mark_image_stem(stem, table[:2])
    with pytest.raises(ValueError):
        fusion._mark_image_stem(stem, table.double())
    with pytest.raises(ValueError):
        fusion._mark_image_stem(m[2], table)       # 8 input channels
    x = torch.randint(0, 256, (2, 3, 9, 10), dtype=torch.uint8).contiguous(memory_format=torch.channels_last)
    assert fusion.link_image_u8(m, table[:1].contiguous(), x) == 0 and stem._image_table is None       # C mismatch: refused, untouched
    with pytest.raises(TypeError):
        fusion.link_image_u8(m, table, x.float())
    # on the CPU nothing can run the bytes: the trace finds the stem, the verification refuses (a CPU tensor is a TypeError), the
    # mark is rolled back with a warning
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert fusion.link_image_u8(m, table, x) == 0
    assert stem._image_table is None and any("link_image_u8" in str(i.message) for i in w)
    # a marked stem refuses CPU bytes; float32 input goes on as before; an unmarked module still takes uint8 as codes (q_bit 32: ATen)
    fusion._mark_image_stem(stem, table)
    with pytest.raises(TypeError):
        m(x)
    y = m(torch.randn(2, 3, 9, 10))
    assert y.shape == (2, 8, 5, 5)
    assert fusion.unlink_image_u8(m) == 1
