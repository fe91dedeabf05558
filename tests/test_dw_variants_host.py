"""Host side of the depthwise 3x3 kernel selection (csrc/conv_dw.hip: dw_select, conv_dw2.hip: dw2_select, conv_dw3.hip: dwr_select,
conv_dwc.hip: dwc_select): the case table of tests/_dw_variants.py reaches the instances it names, is exactly the set of instances the
launchers can select, and covers every instance a net of layer_specs runs on; and the CPU restatement of the family's arithmetic
(oracle/slfp_oracle.c: slfp_oracle_dw3x3_f32) stays within its rounding count of the double-accumulating oracle.  No device is touched:
slfp_debug_dw3x3_instance prints the selection the launch consumes."""
import ctypes
import itertools
import os

import numpy as np
import pytest

from _dw_variants import (IFACES, KA, KW, LAYEROUT, RELU, ROWS, SWITCHES, instance, make_desc, make_inputs, out_hw, set_switches,
                          workgroups)
from cnns_slfp_quantization_amd import _lib, layer_specs
from oracle import slfp_oracle as so

SFP7_NETS = ("squeezenet1_0_imagenet224", "shufflenetv2_224")   # BASELINE.json config 5


@pytest.fixture
def switches():
    L = _lib.load()
    old = {k: os.environ.get(k) for k in SWITCHES}
    try:
        yield lambda env: set_switches(L, env)
    finally:
        set_switches(L, {k: v for k, v in old.items() if v is not None})


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_the_table_reaches_what_it_claims(switches, row):
    switches(row.env)
    d = make_desc(_lib, row)
    assert _lib.load().slfp_conv2d_kernel_name(ctypes.byref(d)).decode() == "dw3x3_nhwc"
    assert instance(_lib, d, row.iface, row.bias, row.post, row.flags, row.y_qbits) == row.variant, row
    # the coarse reporter still answers as before where it applies: bias-free float32 launches without the layer-output quantizer
    if row.iface in ("f32", "post") and not row.bias and not (row.flags & LAYEROUT):
        coarse = _lib.load().slfp_debug_dw3x3_variant(ctypes.byref(d), int(row.post)).decode()
        assert coarse == row.variant.split("/")[0], (row, coarse)


def selectable():
    """Every instance the four launchers can select: the product of the grammar minus the combinations no descriptor reaches."""
    fmts, out = ("act8", "sfp7"), set()
    for s, g, v, t, f, lo in itertools.product((1, 2), ("cb32iw16", "cb64iw9", "cb32iw15", "gen"), (4, 2), ("tab", "long"), fmts, ("", "/lo")):
        if g in ("cb32iw16", "cb64iw9") and s == 2:
            continue   # IW = 16 and 9 are stride-1 halo widths (14- and 7-wide tiles)
        if g == "cb32iw15" and s == 1:
            continue   # IW = 15 is the stride-2 halo of a 7-wide tile
        if g in ("cb64iw9", "cb32iw15") and v == 2:
            continue   # 8-byte lanes have one specialised form only: SLFP_DW_BY_FMT(1, 32, 16, 2) (C = 58 at 28 x 28)
        if lo and g != "gen":
            continue   # LO is compiled into the generic-geometry instantiations only
        out.add(f"general/s{s}/{g}/v{v}/{t}/{f}{lo}")
    out |= {f"tile/s{s}/{p}" for s in (1, 2) for p in ("plain", "post")}
    out |= {f"rows/{p}" for p in ("plain", "post")}
    for s, lc, form, p, f in itertools.product((1, 2), (3, 4, 5), ("f32", "yc", "yc-signed", "lut"), ("plain", "post"), fmts):
        if form == "lut" and p == "plain":
            continue   # the table is indexed by the class of the affine's result: LUTQ needs POST (static_assert in k_dwc)
        out.add(f"dwc/s{s}/lc{lc}/{form}/{p}/{f}")
    return out


def test_the_table_is_the_set_of_instances_the_launchers_can_select():
    assert len({r.name for r in ROWS}) == len(ROWS)
    table, want = {r.variant for r in ROWS}, selectable()
    assert table == want, sorted(table ^ want)
    # k_dw3x3: 8 geometry / lane forms x TAB x FMT + 16 LO; k_dw3x3_tile 4; k_dw3x3_rows 2; k_dwc 42, each with either input format
    assert len(want) == 32 + 16 + 4 + 2 + 84
    assert {k for r in ROWS for k, _ in r.env} == set(SWITCHES)
    assert {v for r in ROWS for k, v in r.env if k == "SLFP_DW_ROWS"} == {"0", "15"}
    assert {r.pad for r in ROWS if r.variant.startswith("dwc/")} == {0, 1, 2}
    assert {r.c for r in ROWS if r.variant.startswith("dwc/")} == {32, 64, 128, 256}
    assert {r.c for r in ROWS if r.variant.startswith("tile/s1")} == {32, 64, 96}


def test_every_kernel_has_a_small_and_an_uneven_grid():
    """xcd_remap deals logical workgroup ids to the eight XCDs: each kernel gets a grid below 8 and one >= 8 that is no multiple of 8."""
    for kind in ("general", "tile", "rows", "dwc"):
        counts = {workgroups(r) for r in ROWS if r.variant.split("/")[0] == kind}
        assert any(c < 8 for c in counts), (kind, sorted(counts))
        assert any(c >= 8 and c % 8 for c in counts), (kind, sorted(counts))


def test_the_reporter_says_none_off_the_family_and_where_the_entry_point_refuses(switches):
    switches(None)
    L = _lib.load()
    assert L.slfp_debug_dw3x3_instance(None, None, 0, 0, 0) == b"none"
    for s in layer_specs.conv_layers("vgg16_224"):   # dense 3x3 layers only
        d = _spec_desc(s, 4, 8)
        for iface in IFACES:
            assert instance(_lib, d, iface, False, iface == "lut", LAYEROUT if iface == "lut" else 0, 8) == "none", (s, iface)
    r = next(r for r in ROWS if r.name == "tile-s1-15x17")
    d = make_desc(_lib, r)
    assert instance(_lib, d, "cin", True, False, 0, 8) == "none"          # the code kernel takes no bias
    assert instance(_lib, d, "post", False, False, LAYEROUT, 8) == "none"  # the layer-output quantizer needs the affine
    assert instance(_lib, d, "lut", False, False, LAYEROUT, 8) == "none"   # so does the table epilogue
    assert instance(_lib, d, "post", False, False, 4, 8) == "none"         # unknown flag bits
    r24 = next(r for r in ROWS if r.name == "gen-cb32iw16-c24")
    assert instance(_lib, make_desc(_lib, r24), "cin", False, False, 0, 8) == "none"   # C = 24: no code kernel
    switches({"SLFP_LONG_ENCODE": "1"})
    assert instance(_lib, d, "cin", False, False, 0, 8) == "none"          # the code paths need the tables


def _spec_desc(s, n, qbits):
    return _lib.ConvDesc(n=n, c_in=s.c_in, h=s.h, w=s.w, c_out=s.c_out, kh=s.k[0], kw=s.k[1], stride_h=s.stride[0], stride_w=s.stride[1],
                         pad_h=s.pad[0], pad_w=s.pad[1], dil_h=1, dil_w=1, groups=s.groups, x_layout=_lib.LAYOUT_NHWC,
                         y_layout=_lib.LAYOUT_NHWC, qbits=qbits, ka=float(np.float32(s.Ka)), kw_scale=float(np.float32(s.Kw)),
                         mfma_passes=0, reserved=0)


def test_census_of_the_nets_is_covered_by_the_table(switches):
    """Every depthwise layer of every net of layer_specs, on every interface, with and without the post vectors and the ReLU: the
    instance the launchers give it has a small-shape row.  A new kernel instance fails here until it has one."""
    switches(None)
    L = _lib.load()
    table = {r.variant for r in ROWS}
    census, n_dw = {}, 0
    for net in layer_specs.nets():
        for i, s in enumerate(layer_specs.conv_layers(net)):
            for qbits in (8, 7) if net in SFP7_NETS else (8,):
                d = _spec_desc(s, 8, qbits)
                if L.slfp_conv2d_kernel_name(ctypes.byref(d)).decode() != "dw3x3_nhwc":
                    assert instance(_lib, d, "f32", False, False, 0, qbits) == "none", (net, i)
                    continue
                n_dw += 1
                for iface, post, flags in (("f32", False, 0), ("post", True, 0), ("post", True, RELU), ("post", True, RELU | LAYEROUT),
                                           ("cin", True, RELU), ("cin", False, 0), ("cout", True, RELU), ("cout", True, 0),
                                           ("cout", False, RELU), ("lut", True, LAYEROUT)):
                    for bias in (False, True):
                        v = instance(_lib, d, iface, bias, post, flags, qbits, s.Ka)
                        assert v != "none" or iface in ("cin", "cout", "lut"), (net, i, iface)
                        if v != "none":
                            census.setdefault(v, set()).add((net, i))
    print("\ndepthwise 3x3 instance census (instance: layers)")
    for v in sorted(census):
        print(f"  {v:44s} {len(census[v]):3d}")
    assert n_dw >= 13 and len(census) >= 20
    assert set(census) <= table, sorted(set(census) - table)


def _f32_cases():
    """the distinct float32-output computations of the table without the layer-output quantizer (a discontinuity no bound survives)"""
    seen, out = set(), []
    for r in ROWS:
        if r.iface in ("cout", "lut") or (r.flags & LAYEROUT):
            continue
        key = (r.c, r.stride, r.pad, r.n, r.h, r.w, r.qbits, r.bias, r.post, r.flags)
        if key not in seen:
            seen.add(key)
            out.append(r)
    return out


@pytest.mark.parametrize("row", _f32_cases(), ids=[r.name for r in _f32_cases()])
def test_restatement_is_within_its_rounding_count_of_the_double_accumulating_oracle(row):
    """slfp_oracle_dw3x3_f32 (nine float32 fmaf, two rescales) against slfp_oracle_conv2d (double accumulation, one rounding, two
    rescales): per element at most 12 * 2^-24 * Ka * Kw * sum |x_q w_q| (the bias counted among the terms); with the affine, that error
    times |scale| plus two roundings of the result's magnitude.  The sum of absolute terms is the oracle's own, on |x_q| and |w_q|."""
    x, _, w, bias, scale, shift = make_inputs(row)
    b = bias if row.bias else None
    got = so.dw3x3_f32(x, w, b, row.stride, row.pad, KA, KW, row.qbits, scale if row.post else None, shift if row.post else None,
                       False, bool(row.flags & RELU)).astype(np.float64)
    nchw = np.ascontiguousarray(x.transpose(0, 3, 1, 2))
    ref, xq, wq = so.conv2d(nchw, w, b, row.stride, row.pad, 1, row.c, KA, KW, row.qbits, want_q=True)
    bq_abs = np.abs((b / np.float32(KA)) / np.float32(KW)) if row.bias else None
    mag = so.conv2d(np.abs(xq), np.abs(wq), bq_abs, row.stride, row.pad, 1, row.c, 1.0, 1.0, 32).astype(np.float64) * (KA * KW)
    ref, mag = ref.transpose(0, 2, 3, 1).astype(np.float64), mag.transpose(0, 2, 3, 1)
    assert got.shape == ref.shape == (row.n,) + out_hw(row) + (row.c,)
    eps = 2.0 ** -24
    bound = 12 * eps * mag
    if row.post:
        s64, h64 = scale.astype(np.float64), shift.astype(np.float64)
        ref = ref * s64 + h64
        bound = bound * np.abs(s64) + 2 * eps * (mag * np.abs(s64) + np.abs(h64))
    if row.flags & RELU:
        ref = np.maximum(ref, 0.0)   # 1-Lipschitz: the bound carries over
    err = np.abs(got - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{row.name}: max err / bound {worst:.3f}")
    assert np.isfinite(got).all() and (err <= bound).all(), (row, worst)
