"""Host side of the one-kernel depthwise -> pointwise block's instance selection (csrc/conv_dwpw.hip: dwpw_select, csrc/conv_dwpw_codes.hip:
dwpw_codes_select; one list of built instances, SLFP_DWPW_INSTANCES in csrc/slfp_host.hpp): the case table of tests/_dwpw_variants.py
reaches the instances it names, is exactly the set the two launchers can select, and that set is exactly what the queries accept -- no
supported pair without an instance; every block of the MobileNetV1 nets of layer_specs that the queries accept has a small-shape row.
No device is touched: slfp_debug_dwpw_instance prints the selection the launch consumes, and every pointer handed to slfp_dwpw_fwd
here is refused before it would be looked at."""
import ctypes
import itertools
import os

import numpy as np
import pytest

from _dwpw_variants import (KSS, NTS, ROWS, STRIDES, instance, instance_name, kernel_of, make_descs, make_io, out_hw, selectable,
                            workgroups)
from cnns_slfp_quantization_amd import _lib, layer_specs
from test_dwpw_codes_host import _io, _pair, _refused

MOBILENETS = ("mobilenetv1_imagenet224", "mobilenetv1_cifar32")


def _supported(r, dw, pw):
    L = _lib.load()
    if r.iface == "f32":
        return L.slfp_dwpw_supported(ctypes.byref(dw), ctypes.byref(pw))
    return L.slfp_dwpw_codes_supported(ctypes.byref(dw), ctypes.byref(pw), ctypes.byref(make_io(_lib, r)), int(r.bias), r.relu1, r.relu2)


@pytest.fixture
def long_encode():
    """sets SLFP_LONG_ENCODE for the test and puts the environment back"""
    L = _lib.load()
    old = os.environ.get("SLFP_LONG_ENCODE")
    try:
        os.environ["SLFP_LONG_ENCODE"] = "1"
        L.slfp_debug_reload_switches()
        yield
    finally:
        os.environ.pop("SLFP_LONG_ENCODE", None)
        if old is not None:
            os.environ["SLFP_LONG_ENCODE"] = old
        L.slfp_debug_reload_switches()


def test_the_reporter_is_exported_and_declared():
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "slfp.h")).read()
    assert "slfp_debug_dwpw_instance" in _lib.SYMBOLS and hasattr(_lib.load(), "slfp_debug_dwpw_instance")
    assert "const char* slfp_debug_dwpw_instance(" in header
    assert _lib.load().slfp_version() == 1   # SLFP_ABI_VERSION: a new export only


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_the_table_reaches_what_it_claims(row):
    dw, pw = make_descs(_lib, row)
    L = _lib.load()
    assert L.slfp_conv2d_kernel_name(ctypes.byref(dw)).decode() == "dw3x3_nhwc"
    assert L.slfp_conv2d_kernel_name(ctypes.byref(pw)).decode().startswith("pw_mfma_f16")
    assert (pw.h, pw.w) == out_hw(row)
    assert _supported(row, dw, pw) == 1, row
    assert instance(_lib, row, dw, pw) == row.instance, row


def _query_set():
    """The instances the queries accept over C x N x stride x q_bit (and, on codes, the two output forms), named from the PAIR alone
    (not by the reporter), next to what the reporter says for each accepted pair."""
    L = _lib.load()
    accepted, reported = set(), {}
    for c, n_out, s, qbits in itertools.product((32, 64, 128), (64, 128, 256), STRIDES, (8, 7)):
        dw, pw = _pair(c, n_out, s, 30, 34, qbits=qbits)
        if L.slfp_dwpw_supported(ctypes.byref(dw), ctypes.byref(pw)) == 1:
            name = instance_name("f32", s, c // 32, n_out // 16, qbits)
            accepted.add(name)
            reported[name] = L.slfp_debug_dwpw_instance(ctypes.byref(dw), ctypes.byref(pw), None, 0, 1, 1).decode()
        for y_codes, y_qbits in ((0, 8), (1, 8), (1, 7)):
            io = _io(1, y_codes, y_qbits)
            if L.slfp_dwpw_codes_supported(ctypes.byref(dw), ctypes.byref(pw), ctypes.byref(io), 0, 1, 1) == 1:
                name = instance_name("cio8" if y_codes else "cin", s, c // 32, n_out // 16, qbits)
                accepted.add(name)
                reported[name] = L.slfp_debug_dwpw_instance(ctypes.byref(dw), ctypes.byref(pw), ctypes.byref(io), 0, 1, 1).decode()
    return accepted, reported


def test_table_launchers_and_queries_span_the_same_set_of_instances():
    """table == what the launchers can select (the grammar: 18 + 72) == what the queries accept.  A pair a query accepts and no
    launcher instance takes (32 -> 256 on the float32 interface, before the two lists became one) fails the last equality."""
    assert len({r.name for r in ROWS}) == len(ROWS)
    table, want = {r.instance for r in ROWS}, selectable()
    assert len(want) == 18 + 72
    assert table == want, sorted(table ^ want)
    accepted, reported = _query_set()
    assert accepted == want, sorted(accepted ^ want)
    # no supported pair without an instance: the reporter (= the launcher's dispatch) names the pair's own instance
    assert all(name == got for name, got in reported.items()), {k: v for k, v in reported.items() if k != v}
    # the interfaces the strings do not carry
    for q in (8, 7):
        fmt = "act8" if q == 8 else "sfp7"
        assert {r.iface for r in ROWS if r.instance.endswith(f"/{fmt}/yc")} == {"cio8", "cio7"}, q
    assert {r.qbits for r in ROWS if r.iface == "f32"} == {8, 7}
    for kern in ("k_dwpw", "k_dwpw_codes"):
        rows = [r for r in ROWS if kernel_of(r) == kern]
        for s in STRIDES:
            for ks in KSS:   # phase 1 is per (S, KS): pad 0, 1 and 2 on each
                assert {r.pad for r in rows if r.stride == s and r.c == 32 * ks} == {0, 1, 2}, (kern, s, ks)
        assert {(r.bias, r.post2) for r in rows} == {(True, True), (True, False), (False, False), (False, True)}, kern
        assert {(r.relu1, r.relu2) for r in rows} == {(0, 0), (0, 1), (1, 0), (1, 1)}, kern
        assert any(r.special for r in rows), kern
        assert {r.n_out // 16 for r in rows} == set(NTS)


def test_the_mobilenet_blocks_the_queries_accept_are_in_the_table():
    """Every depthwise -> pointwise pair of layer_specs' MobileNetV1 nets, at q_bit 8 and 7: where a query says 1, the reporter names an
    instance and the table has a row for it."""
    L = _lib.load()
    table = {r.instance for r in ROWS}
    census, pairs = {}, 0
    for net in MOBILENETS:
        layers = layer_specs.conv_layers(net)
        for i, (a, b) in enumerate(zip(layers, layers[1:])):
            if not (a.groups == a.c_in and a.groups > 1 and a.k == (3, 3) and b.k == (1, 1) and b.groups == 1 and b.c_in == a.c_out):
                continue
            pairs += 1
            for qbits in (8, 7):
                common = dict(n=8, dil_h=1, dil_w=1, x_layout=_lib.LAYOUT_NHWC, y_layout=_lib.LAYOUT_NHWC, qbits=qbits, mfma_passes=0, reserved=0)
                dw = _lib.ConvDesc(c_in=a.c_in, h=a.h, w=a.w, c_out=a.c_out, kh=3, kw=3, stride_h=a.stride[0], stride_w=a.stride[1],
                                   pad_h=a.pad[0], pad_w=a.pad[1], groups=a.groups, ka=float(np.float32(a.Ka)), kw_scale=float(np.float32(a.Kw)), **common)
                pw = _lib.ConvDesc(c_in=b.c_in, h=b.h, w=b.w, c_out=b.c_out, kh=1, kw=1, stride_h=1, stride_w=1, pad_h=0, pad_w=0, groups=1,
                                   ka=float(np.float32(b.Ka)), kw_scale=float(np.float32(b.Kw)), **common)
                ios = [None] + [_lib.ConvIo(x_codes=1, y_codes=yc, y_ka=0.25, y_qbits=yq) for yc, yq in ((0, 8), (1, 8), (1, 7))]
                for io in ios:
                    ref = ctypes.byref(io) if io is not None else None
                    ok = (L.slfp_dwpw_supported(ctypes.byref(dw), ctypes.byref(pw)) if io is None else
                          L.slfp_dwpw_codes_supported(ctypes.byref(dw), ctypes.byref(pw), ref, 0, 1, 1))
                    name = L.slfp_debug_dwpw_instance(ctypes.byref(dw), ctypes.byref(pw), ref, 0, 1, 1).decode()
                    assert (name != "none") == (ok == 1), (net, i, qbits, name, ok)
                    if ok:
                        census.setdefault(name, set()).add((net, i))
    print("\none-kernel block instance census (instance: blocks)")
    for v in sorted(census):
        print(f"  {v:32s} {len(census[v]):3d}")
    assert pairs >= 13 and len(census) >= 4 * 5   # the ImageNet net's first four blocks, on five interfaces
    assert set(census) <= table, sorted(set(census) - table)


def test_every_kernel_has_a_small_and_an_uneven_grid():
    """xcd_remap deals logical workgroup ids to the eight XCDs: each kernel gets a grid below 8 and one >= 8 that is no multiple of 8."""
    for kern in ("k_dwpw", "k_dwpw_codes"):
        counts = {workgroups(r) for r in ROWS if kernel_of(r) == kern}
        assert any(c < 8 for c in counts), (kern, sorted(counts))
        assert any(c >= 8 and c % 8 for c in counts), (kern, sorted(counts))


def test_the_inputs_span_the_quantizers_classes():
    """The generator behind every row: both signs, both clamps reached from beyond, the tiny class, exact zeros of both signs, most of
    each format's classes; the special sites are a NaN / +inf / -inf / -0.0 pixel and the last image's last element."""
    from _dwpw_variants import KA_DW, make_inputs, special_sites
    from oracle import slfp_oracle as so
    for row in (ROWS[0], next(r for r in ROWS if r.stride == 2)):
        a = make_inputs(row)
        x = a["x"]
        assert np.isfinite(x).all() and (x > 15.5 * KA_DW).any() and (x < -15.5 * KA_DW).any()
        assert (np.abs(x[x != 0]) < 2.0 ** -4 * KA_DW).any()                     # below the smallest regular class
        zeros = x[x == 0]
        assert np.signbit(zeros).any() and not np.signbit(zeros).all()
        for fmt, nclass in ((so.FMT_ACT8, 255), (so.FMT_SFP7, 127)):
            xq = so.quantize(x, np.float32(KA_DW), fmt)
            classes = np.unique(xq)
            assert len(classes) >= 0.8 * nclass, (fmt, len(classes))
            assert classes.min() == -classes.max() and (xq == 0).any()
        xs = a["x_special"]
        changed = np.argwhere(xs.view(np.uint32) != x.view(np.uint32))
        assert {tuple(c) for c in changed} <= {s[:4] for s in special_sites(row)}
        px = xs[0, row.h // 2, row.w // 2]
        assert np.isnan(px[0]) and px[1] == np.inf and px[2] == -np.inf and px[3] == 0 and np.signbit(px[3])
        assert np.isnan(xs[-1, -1, -1, -1]) and int(np.isnan(xs).sum()) == row.c // 4 + 1
        assert a["w_dw"].shape == (row.c, 1, 3, 3) and a["w_pw"].shape == (row.n_out, row.c, 1, 1)
        assert (a["sc2"] < 0).any() and (a["sc2"] > 0).any()


def _name(dw, pw, io, relu1=1, relu2=1):
    ref = lambda s: ctypes.byref(s) if s is not None else None   # noqa: E731
    return _lib.load().slfp_debug_dwpw_instance(ref(dw), ref(pw), ref(io), 0, relu1, relu2).decode()


def test_the_reporter_says_none_for_null_descriptors():
    dw, pw = _pair(32, 64, 1, 28)
    assert _name(dw, pw, None) == "f32/s1/k1/n4" and _name(dw, pw, _io()) == "codes/s1/k1/n4/act8/yc"   # the control
    for io in (None, _io()):
        assert _name(None, pw, io) == "none" and _name(dw, None, io) == "none" and _name(None, None, io) == "none"


@pytest.mark.parametrize("case", _refused(), ids=[c[0] for c in _refused()])
def test_the_reporter_says_none_for_every_refused_pair(case):
    """tests/test_dwpw_codes_host.py::_refused: "none" through the code interface for each; through the float32 interface exactly
    where slfp_dwpw_supported refuses (the io struct and the layouts between the two layers are not its business)."""
    name, (dw, pw), io = case
    L = _lib.load()
    assert L.slfp_dwpw_codes_supported(ctypes.byref(dw), ctypes.byref(pw), ctypes.byref(io), 0, 1, 1) == 0
    assert _name(dw, pw, io) == "none", name
    f32_ok = L.slfp_dwpw_supported(ctypes.byref(dw), ctypes.byref(pw))
    assert (_name(dw, pw, None) == "none") == (f32_ok == 0), name


def test_the_reporter_says_none_for_relu_bits_other_than_0_and_1():
    dw, pw = _pair(32, 64, 1, 28)
    for relu1, relu2 in ((1 | 2, 1), (1, 1 | 2), (2, 0), (0, 2), (4, 0), (-1, 1)):
        for io in (None, _io(), _io(1, 0)):
            assert _name(dw, pw, io, relu1, relu2) == "none", (relu1, relu2)
    for relu1, relu2 in ((0, 0), (0, 1), (1, 0), (1, 1)):
        assert _name(dw, pw, None, relu1, relu2) == "f32/s1/k1/n4"


def test_the_reporter_says_none_under_the_long_form_quantizer(long_encode):
    L = _lib.load()
    for r in ROWS[:5] + ROWS[-3:]:
        dw, pw = make_descs(_lib, r)
        assert _supported(r, dw, pw) == 0 and instance(_lib, r, dw, pw) == "none", r
    dw, pw = _pair(32, 64, 1, 28)
    assert L.slfp_dwpw_supported(ctypes.byref(dw), ctypes.byref(pw)) == 0 and _name(dw, pw, None) == "none"


def test_fwd_refuses_relu_values_other_than_0_and_1_before_any_pointer():
    """slfp_dwpw_fwd, as slfp_dwpw_fwd_codes and the header's "0 / 1": every pointer below is null or unaligned, the descriptors are
    null in one call -- the status is SLFP_ERR_BAD_ARG all the same, so the flags are checked first."""
    L = _lib.load()
    dw, pw = _pair(32, 64, 1, 28)
    for relu1, relu2 in ((2, 0), (0, 2), (3, 1), (1, 3), (-1, 0), (0, 256)):
        assert L.slfp_dwpw_fwd(ctypes.byref(dw), ctypes.byref(pw), None, None, None, None, relu1, None, None, None, None, relu2, None, None) == _lib.ERR_BAD_ARG
        assert "relu" in _lib.last_error()
        assert L.slfp_dwpw_fwd(None, None, 4, 4, 4, 4, relu1, 4, 4, 4, 4, relu2, 4, None) == _lib.ERR_BAD_ARG
    # the control: good flags get as far as the next checks
    assert L.slfp_dwpw_fwd(None, None, None, None, None, None, 1, None, None, None, None, 0, None, None) == _lib.ERR_UNSUPPORTED
    assert L.slfp_dwpw_fwd(ctypes.byref(dw), ctypes.byref(pw), None, None, None, None, 1, None, None, None, None, 1, None, None) == _lib.ERR_BAD_ARG
    assert "null pointer" in _lib.last_error()
    big = _pair(32, 256, 1, 28)   # the pair that had no instance: as far as the pointer checks now, like every supported pair
    assert L.slfp_dwpw_supported(ctypes.byref(big[0]), ctypes.byref(big[1])) == 1
    assert L.slfp_dwpw_fwd(ctypes.byref(big[0]), ctypes.byref(big[1]), None, None, None, None, 1, None, None, None, None, 1, None, None) == _lib.ERR_BAD_ARG
