"""Host side of the image-stem and direct kernel selection (csrc/conv_direct.hip: stem_select, direct_select; conv_stem_small.hip:
stem_small_select; conv_stem_mfma.hip: stem_mfma_select): the case table of tests/_stem_variants.py reaches the instances it names, is
exactly the set of instances the launchers can select, and covers every instance the first layer of a net of layer_specs runs on; the
code-output queries answer 1 exactly where the selection has a code form; the CPU restatement of the float32 kernels' arithmetic
(oracle/slfp_oracle.c: slfp_oracle_conv_f32) stays within its rounding count of the double-accumulating oracle; and the fp16 kernels'
operand-level reference stays inside the bars of tests/_bars.py against that oracle, which is what lets the GPU test hold the fp16
kernels to it.  No device is touched: slfp_debug_stem_instance prints the selection the launch consumes."""
import ctypes
import itertools
import os

import numpy as np
import pytest

from _bars import ELEM_MIN, elem_frac_bar, tol as _tol
from _stem_variants import (F16_KINDS, F32_KINDS, FORMS, IFACES, KA, KW, LAYEROUT, RELU, ROWS, SWITCHES, chunk, f16_reference, instance, kind,
                            layer_key, make_desc, make_inputs, make_io, out_hw, set_switches, taps, workgroups)
from cnns_slfp_quantization_amd import _lib, layer_specs
from conftest import elem_exceed_frac, rel_errors
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


FAMILY = {"direct": ("direct_nhwc",), "stem": ("stem_nhwc",), "small": ("stem_small_mfma_f16x1", "stem_small_mfma_f16_exact"),
          "rows": ("stem_mfma_f16x1", "stem_mfma_f16_exact"), "im2row": ("stem_mfma_f16x1", "stem_mfma_f16_exact")}


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_the_table_reaches_what_it_claims(switches, row):
    switches(row.env)
    d = make_desc(_lib, row)
    assert _lib.load().slfp_conv2d_kernel_name(ctypes.byref(d)).decode() in FAMILY[kind(row)], row
    assert instance(_lib, d, row.iface, row.bias, row.post, row.flags, row.y_qbits) == row.variant, row


def direct_class(v):
    """direct/<fmt>/cc<CC>/oc<n>/<lanes> -> (fmt, several output chunks, lanes): CC and the chunk count are runtime numbers"""
    w = v.split("/")
    return (w[1], int(w[3][2:]) > 1, w[4])


def selectable():
    """Every instance the four launchers can select: the product of the grammar minus the combinations no descriptor reaches.  k_direct's
    CC and chunk count are numbers: its rows are compared by direct_class."""
    fmts, out = ("act8", "sfp7"), set()
    out |= {f"stem/gen/{f}/p{p}" for f in fmts for p in (2, 4, 8)}
    out |= {f"stem/fixed/{f}/long" for f in fmts}
    out |= {f"stem/{k}/{o}" for k in ("fixed/tab", "mx") for o in ("f32", "yc", "yc-signed", "lut")}
    for nt, f, o in itertools.product((1, 2, 3, 4), fmts, ("f32", "yc", "yc-signed", "lut")):
        if o != "f32" and nt != 4:
            continue   # code output regroups four channel tiles into one 16-byte store: the 64-channel form only
        out.add(f"small/nt{nt}/{f}/{o}")
    out |= {f"{k}/nt{nt}/{f}/{o}" for k in ("rows", "im2row") for nt in (4, 6) for f in fmts for o in ("f32", "yc", "yc-signed")}
    return out


def test_the_table_is_the_set_of_instances_the_launchers_can_select():
    assert len({r.name for r in ROWS}) == len(ROWS)
    table = {r.variant for r in ROWS if kind(r) != "direct"}
    want = selectable()
    assert table == want, sorted(table ^ want)
    # k_stem 6, k_stem_fixed 2 + 4, k_stem_mx 4, k_stem_small 8 + 6, k_stem_rows 12, the two-kernel form 12
    assert len(want) == 6 + 6 + 4 + 14 + 12 + 12
    # k_direct: both formats; one and several output chunks; every kind of lane; one channel chunk, several, and a chunk cut by LDS
    direct = [r for r in ROWS if kind(r) == "direct"]
    classes = {direct_class(r.variant) for r in direct}
    assert {c[0] for c in classes} == {"act8", "sfp7"} and {c[1] for c in classes} == {False, True}
    assert {c[2] for c in classes} == {"vec", "scalar", "mixed"}
    cg = lambda r: r.c_in // r.groups   # noqa: E731
    assert any(chunk(r) == cg(r) for r in direct) and any(chunk(r) == 32 and cg(r) % 32 for r in direct)
    assert any(chunk(r) < min(32, cg(r)) for r in direct), "a row whose CC the LDS budget cuts"
    assert {k for r in ROWS for k, _ in r.env} == set(SWITCHES)
    # the paddings of the MobileNetV1 stem rows: pad_w = 1 alone runs k_stem_mx
    mb = [r for r in ROWS if r.variant.startswith(("stem/mx", "stem/fixed/tab")) and not r.env]
    assert {r.pad for r in mb} == {(0, 0), (1, 1), (2, 2), (1, 0), (0, 1)}
    for r in mb:
        assert r.variant.startswith("stem/mx") == (r.pad[1] % 4 == 1 and (r.w * 3) % 4 == 0), r


def test_every_kernel_has_a_small_and_an_uneven_grid():
    """xcd_remap deals logical workgroup ids to the eight XCDs: each kernel gets a grid below 8 and one >= 8 that is no multiple of 8."""
    def kernel(r):
        v = r.variant.split("/")
        return v[0] if v[0] != "stem" else "stem/" + v[1]
    for k in sorted({kernel(r) for r in ROWS}):
        counts = {workgroups(r) for r in ROWS if kernel(r) == k}
        assert any(c < 8 for c in counts), (k, sorted(counts))
        assert any(c >= 8 and c % 8 for c in counts), (k, sorted(counts))


def _spec_desc(s, n, qbits, passes=0):
    return _lib.ConvDesc(n=n, c_in=s.c_in, h=s.h, w=s.w, c_out=s.c_out, kh=s.k[0], kw=s.k[1], stride_h=s.stride[0], stride_w=s.stride[1],
                         pad_h=s.pad[0], pad_w=s.pad[1], dil_h=1, dil_w=1, groups=s.groups, x_layout=_lib.LAYOUT_NHWC,
                         y_layout=_lib.LAYOUT_NHWC, qbits=qbits, ka=float(np.float32(s.Ka)), kw_scale=float(np.float32(s.Kw)),
                         mfma_passes=passes, reserved=0)


def test_the_reporter_says_none_off_the_family_and_where_the_entry_point_refuses(switches):
    switches(None)
    L = _lib.load()
    assert L.slfp_debug_stem_instance(None, None, 0, 0, 0) == b"none"
    seen = set()
    for net in ("mobilenetv1_imagenet224", "vgg16_224"):   # depthwise, pointwise and dense layers
        for s in layer_specs.conv_layers(net)[1:]:
            d = _spec_desc(s, 4, 8)
            fam = L.slfp_conv2d_kernel_name(ctypes.byref(d)).decode()
            seen.add(fam.split("_")[0])
            for iface in IFACES:
                assert instance(_lib, d, iface, False, iface == "lut", LAYEROUT if iface == "lut" else 0, 8) == "none", (s, iface)
    assert {"dw3x3", "pw", "dense"} <= seen, seen
    mx = next(r for r in ROWS if r.name == "mb-33x36p1-plain")
    d = make_desc(_lib, mx)
    assert instance(_lib, d, "post", False, False, LAYEROUT, 8) == "none"   # the layer-output quantizer needs the affine
    assert instance(_lib, d, "lut", False, False, LAYEROUT, 8) == "none"    # so does the table epilogue
    assert instance(_lib, d, "post", False, False, 4, 8) == "none"          # unknown flag bits
    io = _lib.ConvIo(x_codes=1, y_codes=0, y_ka=1.0, y_qbits=8)
    assert L.slfp_debug_stem_instance(ctypes.byref(d), ctypes.byref(io), 0, 0, 0) == b"none"   # these kernels read float32
    gen = next(r for r in ROWS if r.name == "gen-3x3c3-o64")
    assert instance(_lib, make_desc(_lib, gen), "cout", False, True, RELU, 8) == "none"   # k_stem writes float32 only
    dr = next(r for r in ROWS if r.name == "dir-dil2")
    assert instance(_lib, make_desc(_lib, dr), "cout", False, True, RELU, 8) == "none"    # so does k_direct
    s24 = next(r for r in ROWS if r.name == "small-k27-o24-s2-act8")
    assert instance(_lib, make_desc(_lib, s24), "cout", False, True, RELU, 8) == "none"   # k_stem_small: codes at C_out = 64 only
    r16 = next(r for r in ROWS if r.name == "rows-7x7s2-o16-act8")
    assert instance(_lib, make_desc(_lib, r16), "lut", False, True, LAYEROUT, 8) == "none"   # the large-kernel stems have no table epilogue
    switches({"SLFP_LONG_ENCODE": "1"})
    assert instance(_lib, d, "cout", False, True, RELU, 8) == "none"        # the code paths need the tables


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_the_code_queries_agree_with_the_selection(switches, row):
    """slfp_conv2d_codes_supported / slfp_conv2d_codes_lut_supported answer 1 exactly where the selection of the row's layer, asked for
    that output form, names an instance."""
    switches(row.env)
    L = _lib.load()
    d = make_desc(_lib, row)
    for form, (iface, post, flags) in FORMS.items():
        if form == "f32":
            continue
        for y_qbits in (8, 7):
            io = make_io(_lib, iface, y_qbits)
            v = instance(_lib, d, iface, row.bias, post, flags, y_qbits)
            if form == "lut":
                q = L.slfp_conv2d_codes_lut_supported(ctypes.byref(d), ctypes.byref(io), int(row.bias), row.c_out)
            else:
                q = L.slfp_conv2d_codes_supported(ctypes.byref(d), ctypes.byref(io), int(row.bias), flags)
            assert q == int(v != "none"), (row.name, form, y_qbits, v, q)
            assert v == "none" or v.endswith("/" + form), (row.name, form, v)
    if row.iface in ("cout", "lut"):
        assert instance(_lib, d, row.iface, row.bias, row.post, row.flags, row.y_qbits) != "none"


def test_census_of_the_nets_first_layers_is_covered_by_the_table(switches):
    """The first layer of every net of layer_specs (and every other layer that falls to these families), on every interface, in both
    MFMA modes: the instance the launchers give it has a small-shape row.  k_direct's strings carry runtime numbers: its class counts."""
    switches(None)
    L = _lib.load()
    table = {r.variant for r in ROWS}
    dclasses = {direct_class(r.variant) for r in ROWS if kind(r) == "direct"}
    census, firsts = {}, 0
    for net in layer_specs.nets():
        for i, s in enumerate(layer_specs.conv_layers(net)):
            for qbits in (8, 7) if net in SFP7_NETS else (8,):
                for passes in (0, 3):
                    d = _spec_desc(s, 8, qbits, passes)
                    fam = L.slfp_conv2d_kernel_name(ctypes.byref(d)).decode()
                    ours = fam in ("direct_nhwc", "stem_nhwc") or fam.startswith(("stem_small_mfma", "stem_mfma"))
                    v0 = instance(_lib, d, "f32", False, False, 0, qbits)
                    assert (v0 != "none") == ours, (net, i, fam, v0)
                    if not ours:
                        continue
                    firsts += i == 0
                    for iface, post, flags in (("f32", False, 0), ("post", True, 0), ("post", True, RELU), ("post", True, RELU | LAYEROUT),
                                               ("cout", True, RELU), ("cout", True, 0), ("cout", False, RELU), ("lut", True, LAYEROUT)):
                        for bias in (False, True):
                            v = instance(_lib, d, iface, bias, post, flags, qbits, s.Ka)
                            assert v != "none" or iface in ("cout", "lut"), (net, i, iface)
                            if v != "none":
                                census.setdefault(v, set()).add((net, i))
    print("\nstem / direct instance census (instance: layers)")
    for v in sorted(census):
        print(f"  {v:44s} {len(census[v]):3d}")
    assert firsts >= len(layer_specs.nets()) and len(census) >= 8
    for v in census:
        assert (direct_class(v) in dclasses) if v.startswith("direct/") else (v in table), v


def _distinct(rows):
    seen, out = set(), []
    for r in rows:
        if layer_key(r) not in seen:
            seen.add(layer_key(r))
            out.append(r)
    return out


_F32_CASES = _distinct([r for r in ROWS if kind(r) in F32_KINDS and r.iface in ("f32", "post") and not (r.flags & LAYEROUT)])
_F16_CASES = _distinct([r for r in ROWS if kind(r) in F16_KINDS and r.iface in ("f32", "post")])


def _oracle(row, x, w, bias, scale, shift, want_mag=False):
    """slfp_oracle_conv2d (double accumulation) of the row's layer with the affine and the ReLU in float64, NHWC"""
    b = bias if row.bias else None
    nchw = np.ascontiguousarray(x.transpose(0, 3, 1, 2))
    ref, xq, wq = so.conv2d(nchw, w, b, row.stride, row.pad, row.dil, row.groups, KA, KW, row.qbits, want_q=True)
    ref = ref.transpose(0, 2, 3, 1).astype(np.float64)
    mag = None
    if want_mag:
        bq_abs = np.abs((b / np.float32(KA)) / np.float32(KW)) if row.bias else None
        mag = so.conv2d(np.abs(xq), np.abs(wq), bq_abs, row.stride, row.pad, row.dil, row.groups, 1.0, 1.0, 32).astype(np.float64)
        mag = mag.transpose(0, 2, 3, 1) * (float(np.float32(KA)) * float(np.float32(KW)))
    if row.post:
        ref = ref * scale.astype(np.float64) + shift.astype(np.float64)
    if row.flags & RELU:
        ref = np.maximum(ref, 0.0)
    return ref, mag


@pytest.mark.parametrize("row", _F32_CASES, ids=[r.name for r in _F32_CASES])
def test_restatement_is_within_its_rounding_count_of_the_double_accumulating_oracle(row):
    """slfp_oracle_conv_f32 (K float32 fmaf, the bias addition, two rescales) against slfp_oracle_conv2d (double accumulation, one
    rounding, two rescales): per element at most (K + 3) * 2^-24 * Ka * Kw * sum |x_q w_q|, K = the taps of one output (padded ones
    included) plus one where there is a bias (its term counted in the sum); with the affine, that error times |scale| plus two roundings of
    the result's magnitude.  The sum of absolute terms is the oracle's own, on |x_q| and |w_q|."""
    x, _, w, bias, scale, shift = make_inputs(row)
    got = so.conv_f32(x, w, bias if row.bias else None, row.stride, row.pad, row.dil, row.groups, KA, KW, row.qbits, chunk(row),
                      scale if row.post else None, shift if row.post else None, False, bool(row.flags & RELU)).astype(np.float64)
    ref, mag = _oracle(row, x, w, bias, scale, shift, want_mag=True)
    assert got.shape == ref.shape == (row.n,) + out_hw(row) + (row.c_out,)
    eps = 2.0 ** -24
    bound = (taps(row) + int(row.bias) + 3) * eps * mag
    if row.post:
        s64, h64 = np.abs(scale.astype(np.float64)), np.abs(shift.astype(np.float64))
        bound = bound * s64 + 2 * eps * (mag * s64 + h64)
    err = np.abs(got - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{row.name}: max err / bound {worst:.3f}")
    assert np.isfinite(got).all() and (err <= bound).all(), (row, worst)


@pytest.mark.parametrize("row", _F16_CASES, ids=[r.name for r in _F16_CASES])
def test_operand_level_reference_is_inside_the_bars_of_the_double_accumulating_oracle(row):
    """The fp16 kernels' operand-level reference alone (float16 operands, float64 contraction) against slfp_oracle_conv2d under the
    unchanged bars of tests/_bars.py: 1e-3 at qbits 8, 1e-5 at qbits 7, and the elementwise fraction from ELEM_MIN elements on."""
    x, _, w, bias, scale, shift = make_inputs(row)
    ref16, mag = f16_reference(row, x, w, bias, scale, shift, so)
    ref, _ = _oracle(row, x, w, bias, scale, shift)
    name = "stem_mfma_f16x1" if row.qbits == 8 else "stem_mfma_f16_exact"
    emax, el2 = rel_errors(ref16, ref)
    print(f"{row.name}: operand-level reference against the oracle: max-rel {emax:.3e} l2 {el2:.3e}")
    assert np.isfinite(ref16).all() and (mag >= 0).all()
    assert emax <= _tol(name) and el2 <= _tol(name), (row, emax, el2)
    if not row.post and ref.size >= ELEM_MIN:
        assert elem_exceed_frac(ref16, ref) <= elem_frac_bar(name), row
