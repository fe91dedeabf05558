"""CPU: the host side of the pointwise (1x1) kernels on codes in the float32-equivalent (three-pass) mode:
slfp_conv2d_codes_x3_supported / slfp_conv2d_fwd_codes_x3 / slfp_debug_pwc_x3_variant, the module's `_code_x3` mark and the `x3=`
keyword of fusion.link_codes / fusion.link_codes_traced.  No device work is done here: every pointer handed to the library is
refused before it would be dereferenced."""
import ctypes
import inspect
import os
import re

import pytest
import torch.nn as nn

from _pw_x3_cases import ROWS, SWITCHES, make_desc, make_io, set_switches, strip_grid, variant
from cnns_slfp_quantization_amd import _lib, fusion, layer_specs
from cnns_slfp_quantization_amd import conv2d_func as cf

NEW = {"slfp_conv2d_codes_x3_supported": "int", "slfp_conv2d_fwd_codes_x3": "int", "slfp_debug_pwc_x3_variant": r"const\s+char\s*\*"}


@pytest.fixture
def switches():
    L = _lib.load()
    old = {k: os.environ.get(k) for k in SWITCHES}
    try:
        yield lambda env: set_switches(L, env)
    finally:
        set_switches(L, {k: v for k, v in old.items() if v is not None})


def _desc(c_in=64, c_out=64, h=12, k=1, pad=0, n=2, qbits=8, groups=1, stride=1, passes=_lib.MFMA_F16X3, x_layout=_lib.LAYOUT_NHWC,
          y_layout=_lib.LAYOUT_NHWC):
    return _lib.ConvDesc(n=n, c_in=c_in, h=h, w=h, c_out=c_out, kh=k, kw=k, stride_h=stride, stride_w=stride, pad_h=pad, pad_w=pad,
                         dil_h=1, dil_w=1, groups=groups, x_layout=x_layout, y_layout=y_layout, qbits=qbits,
                         ka=0.25, kw_scale=0.02, mfma_passes=passes, reserved=0)


def _io(x_codes=1, y_codes=0, y_qbits=8, y_ka=0.3):
    return _lib.ConvIo(x_codes=x_codes, y_codes=y_codes, y_ka=y_ka, y_qbits=y_qbits)


def _x3(d, io, has_bias=1, relu=1):
    return _lib.load().slfp_conv2d_codes_x3_supported(ctypes.byref(d) if d is not None else None,
                                                      ctypes.byref(io) if io is not None else None, has_bias, relu)


def _name(d, io):
    return _lib.load().slfp_debug_pwc_x3_variant(ctypes.byref(d) if d is not None else None,
                                                 ctypes.byref(io) if io is not None else None).decode()


def test_new_symbols_are_exported_and_declared():
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "slfp.h")).read()
    for name, ret in NEW.items():
        assert name in _lib.SYMBOLS
        assert hasattr(L, name)
        assert re.search(r"\b%s\s*%s\s*\(" % (ret, name), header), name
    assert L.slfp_version() == 1   # SLFP_ABI_VERSION: new exports only
    assert "codes_x3" in cf._KINDS and cf._KINDS["codes_x3"] == ("slfp_conv2d_codes_x3_supported", "slfp_conv2d_fwd_codes_x3")


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_the_table_reaches_what_it_claims(switches, row):
    switches(row.env)
    d = make_desc(_lib, row)
    assert _lib.load().slfp_conv2d_kernel_name(ctypes.byref(d)).decode() == "pw_mfma_f16x3"
    for y_qbits in (8, 7):
        io = make_io(_lib, row.iface, y_qbits=y_qbits)
        for relu in (0, 1):
            for has_bias in (0, 1):
                assert _x3(d, io, has_bias, relu) == 1, (row, y_qbits, relu, has_bias)
        assert variant(_lib, d, io) == row.variant, row


def test_names_are_unique_and_every_selectable_instance_has_a_row():
    assert len({r.name for r in ROWS}) == len(ROWS)
    have = {strip_grid(r.variant) for r in ROWS}
    want = {f"pwc-stream/{w}/act8/{f}/p3" for w in ("ks1/dw", "ks2/xw", "ks3/dw", "ks4/xw", "ks8/xw") for f in ("f32", "yc")}
    want |= {f"pwc-tiled/{t}/act8/{f}/p3" for t in (411, 222, 144) for f in ("f32", "yc")}   # launch_pwc_x3_sel's dispatch
    assert have == want, have ^ want
    for kern in ("pwc-stream", "pwc-tiled"):
        assert any(r.stride == 2 and r.variant.startswith(kern) for r in ROWS), kern
    assert any("/grid1" in r.variant and "/f32/" in r.variant for r in ROWS) and any("/grid1" in r.variant and "/yc/" in r.variant for r in ROWS)


def test_the_grid_switch_only_adds_its_word(switches):
    for row in ROWS:
        if row.env:
            continue
        switches({"SLFP_PW_GRID": "2"})
        v = variant(_lib, make_desc(_lib, row), make_io(_lib, row.iface))
        assert v == row.variant + ("/grid2" if row.variant.startswith("pwc-stream") else ""), (row, v)


def _refused():
    return [
        ("qbits7", _desc(qbits=7), _io(1, 0, 7)),
        ("passes0", _desc(passes=_lib.MFMA_DEFAULT), _io()),
        ("passes1", _desc(passes=_lib.MFMA_F16X1), _io()),
        ("float32_in", _desc(), _io(0, 0)),
        ("entry", _desc(), _io(0, 1)),                       # float32 in -> codes out
        ("x_codes2", _desc(), _io(2, 0)),
        ("y_codes2", _desc(), _io(1, 2)),
        ("k16_half", _desc(16, 64), _io()),                  # the half-live last k-step
        ("k48_half", _desc(48, 64), _io()),
        ("k40", _desc(40, 64), _io()),
        ("k160", _desc(160, 64), _io()),                     # five k-steps: no stream instance, not a multiple of 64
        ("k288", _desc(288, 64), _io()),                     # beyond the stream kernel, not a multiple of 64
        ("c_out58", _desc(64, 58), _io()),                   # C_out % 4 != 0 (channel re-padding on the float32 interface)
        ("c_out40_codes", _desc(64, 40), _io(1, 1)),         # C_out % 16 != 0 with code output
        ("y_qbits5", _desc(), _io(1, 1, 5)),
        ("y_ka0", _desc(), _io(1, 1, 8, 0.0)),
        ("y_ka<0", _desc(), _io(1, 1, 8, -0.3)),
        ("nchw_in", _desc(x_layout=_lib.LAYOUT_NCHW), _io()),
        ("nchw_out", _desc(y_layout=_lib.LAYOUT_NCHW), _io()),
        ("3x3", _desc(k=3, pad=1), _io()),
        ("depthwise", _desc(k=3, pad=1, groups=64), _io()),
        ("grouped_1x1", _desc(groups=2), _io()),
    ]


def test_query_refuses_everything_else_and_the_reporter_says_none():
    for name, d, io in _refused():
        for relu in (0, 1):
            assert _x3(d, io, 1, relu) == 0, (name, relu)
        assert _name(d, io) == "none", name
    d = _desc()
    for io in (_io(1, 0), _io(1, 1), _io(1, 1, 7)):
        assert _x3(d, io, 1, 1) == 1 and _x3(d, io, 0, 0) == 1    # the control: the same layer, plain
        assert _x3(d, io, 1, 1 | 2) == 0 and _x3(d, io, 1, 2) == 0   # SLFP_POST_LAYEROUT
        assert _x3(d, io, 1, 4) == 0                                 # unknown flag bits
    assert _name(d, _io(1, 0)) == "pwc-stream/ks2/xw/act8/f32/p3" and _name(d, _io(1, 1)) == "pwc-stream/ks2/xw/act8/yc/p3"
    assert _x3(None, _io()) == 0 and _x3(d, None) == 0
    assert _name(None, _io()) == "none" and _name(d, None) == "none"


def test_the_older_queries_keep_refusing_three_pass_descriptors_on_codes():
    """slfp_conv2d_codes_supported, _slice_supported, _res_supported, _res_codes_supported, _entry_supported and
    _codes_lut_supported answer 0 for a three-pass qbits-8 1x1 descriptor with code input (or output), also where the new query says
    yes: every link count of the default passes rests on it; slfp_debug_pw_variant keeps saying "none" there."""
    L = _lib.load()
    for row in ROWS:
        d = make_desc(_lib, row)
        dp = ctypes.byref(d)
        for io in (_io(1, 0), _io(1, 1), _io(0, 1)):
            iop = ctypes.byref(io)
            for relu in (0, 1):
                assert L.slfp_conv2d_codes_supported(dp, iop, 1, relu) == 0, row
                assert L.slfp_conv2d_entry_supported(dp, iop, 1, relu) == 0, row
                assert L.slfp_conv2d_res_codes_supported(dp, iop, 1, relu) == 0, row
                assert L.slfp_conv2d_codes_slice_supported(dp, iop, 1, relu, 2 * row.c_out) == 0, row
            assert L.slfp_conv2d_codes_lut_supported(dp, iop, 1, row.c_out) == 0, row
            if io.x_codes:
                assert L.slfp_conv2d_res_supported(dp, iop, 1, 0) == 0, row
                assert L.slfp_debug_pw_variant(dp, iop, 0, 0, 0) == b"none", row
    d, io = _desc(), _io(1, 1)
    x, w, y = 1 << 20, 1 << 30, 1 << 32
    assert L.slfp_conv2d_fwd_codes(ctypes.byref(d), ctypes.byref(io), x, w, None, None, None, 1, y, None) == _lib.ERR_UNSUPPORTED


def test_fwd_codes_x3_argument_checks_return_error_codes():
    """Every check that precedes device work: no pointer here is dereferenced."""
    L = _lib.load()
    x, w, y, v = 1 << 20, 1 << 30, 1 << 32, 1 << 34      # 16-byte aligned, never touched

    def call(d=None, io=None, x=x, w=w, y=y, ps=None, psh=None, relu=1):
        d = _desc() if d is None else d
        io = _io(1, 1) if io is None else io
        return L.slfp_conv2d_fwd_codes_x3(ctypes.byref(d) if d is not False else None, ctypes.byref(io) if io is not False else None,
                                          x, w, None, ps, psh, relu, y, None)

    assert call(d=False) == _lib.ERR_BAD_ARG
    assert call(io=False) == _lib.ERR_BAD_ARG
    assert call(x=None) == _lib.ERR_BAD_ARG
    assert call(w=None) == _lib.ERR_BAD_ARG
    assert call(y=None) == _lib.ERR_BAD_ARG
    assert call(ps=v) == _lib.ERR_BAD_ARG and "post_scale" in _lib.last_error()    # a lone post_scale
    assert call(x=x + 4) == _lib.ERR_ALIGNMENT
    assert call(y=y + 8) == _lib.ERR_ALIGNMENT
    assert call(ps=v + 4, psh=v) == _lib.ERR_ALIGNMENT
    assert call(relu=1 | 2, ps=v, psh=v) == _lib.ERR_UNSUPPORTED                    # SLFP_POST_LAYEROUT
    for name, d, io in _refused():
        assert call(d=d, io=io) == _lib.ERR_UNSUPPORTED, name
        assert "slfp_conv2d_codes_x3_supported" in _lib.last_error(), name
    bad = _desc()
    bad.n = 0
    assert call(d=bad) == _lib.ERR_SHAPE


def test_every_three_pass_pointwise_layer_of_the_nets_runs_an_instance_of_the_table(switches):
    """The 1x1 layers of every net that runs SLFP<3,4> (qbits 8), in three-pass mode, at a small and at a measured batch: where the
    query says yes, the instance the launcher selects has a small-shape row in tests/_pw_x3_cases.py -- a new instance fails here
    until it has one.  MobileNetV1's 13 pointwise layers and ResNet-50's 16 conv3 layers are all taken, in both output forms where
    C_out allows codes."""
    switches(None)
    table = {strip_grid(r.variant) for r in ROWS}
    seen, taken = set(), {}
    for net in layer_specs.nets():
        for i, s in enumerate(layer_specs.conv_layers(net)):
            if tuple(s.k) != (1, 1) or s.groups != 1:
                continue
            for n in (2, 128):
                d = _lib.ConvDesc(n=n, c_in=s.c_in, h=s.h, w=s.w, c_out=s.c_out, kh=1, kw=1, stride_h=s.stride[0], stride_w=s.stride[1],
                                  pad_h=s.pad[0], pad_w=s.pad[1], dil_h=1, dil_w=1, groups=1, x_layout=_lib.LAYOUT_NHWC,
                                  y_layout=_lib.LAYOUT_NHWC, qbits=8, ka=float(s.Ka), kw_scale=float(s.Kw), mfma_passes=_lib.MFMA_F16X3,
                                  reserved=0)
                for io in (_io(1, 0), _io(1, 1, 8, float(s.Ka))):
                    v = _name(d, io)
                    assert (v != "none") == bool(_x3(d, io, 0, 1)), (net, i, v)
                    if v != "none":
                        assert v in table, (net, i, v)
                        seen.add(v)
                        taken.setdefault(net, set()).add((i, io.y_codes))
    mb = [i for i, s in enumerate(layer_specs.conv_layers("mobilenetv1_imagenet224")) if tuple(s.k) == (1, 1) and s.groups == 1]
    assert len(mb) == 13 and all((i, y) in taken["mobilenetv1_imagenet224"] for i in mb for y in (0, 1))
    r50 = [i for i, s in enumerate(layer_specs.conv_layers("resnet50_imagenet224"))
           if tuple(s.k) == (1, 1) and tuple(s.stride) == (1, 1) and s.c_out == 4 * s.c_in]
    assert len(r50) >= 16 and all((i, 0) in taken["resnet50_imagenet224"] for i in r50)
    assert any(v.startswith("pwc-stream") for v in seen) and any(v.startswith("pwc-tiled") for v in seen)


def _chain():
    conv = cf.conv2d_Q(8, 0.02, 0.25)
    return nn.Sequential(conv(32, 64, 1), conv(64, 64, 1), conv(64, 48, 1)).eval()


def test_module_and_fusion_defaults_mark_nothing():
    m = cf.conv2d_Q_bias(8, 0.02, 0.25)(64, 64, 1)
    assert m._code_x3 is False and m._code_out is None
    for fn in (fusion.link_codes, fusion.link_codes_traced):
        p = inspect.signature(fn).parameters
        assert "x3" in p and p["x3"].default is False, fn.__name__
    assert list(inspect.signature(fusion.link_codes).parameters) == ["model", "example_input", "x3"]
    assert list(inspect.signature(fusion.link_codes_traced).parameters) == ["model", "example_input", "entries", "x3"]
    # without an example input every candidate is linked; the default marks no module
    net = _chain()
    assert fusion.link_codes(net) == 2
    assert [c._code_x3 for c in net] == [False, False, False] and net[0]._code_out is not None and net[2]._code_out is None
    assert fusion.unlink_codes(net) == 2
    # x3=True without shapes: every code reader may try the three-pass entry point; unlink_codes clears the mark, also on the last
    # reader, which writes float32
    net = _chain()
    assert fusion.link_codes(net, x3=True) == 2
    assert [c._code_x3 for c in net] == [False, True, True]
    assert fusion.unlink_codes(net) == 2
    assert [c._code_x3 for c in net] == [False, False, False] and all(c._code_out is None for c in net)
