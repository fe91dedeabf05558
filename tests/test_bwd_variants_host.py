"""Host side of the backward kernel selection (csrc/conv_bwd.hip: bwd_kind_ex, pw_shape, dense_shape, dw_geom / dw_blocks, act_form):
the case table of tests/_bwd_variants.py reaches the instances it names, is exactly the set of instances the launchers can select,
hits every edge it names (recomputed from the numbers the reporter gives), covers every instance a net of layer_specs runs on, and
has a float64 reference that leaves no gradient element unchecked.  No device is touched: slfp_debug_bwd_instance prints the
selection the launch consumes."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _bwd_variants as V
from _bwd_variants import ROWS
from cnns_slfp_quantization_amd import _lib, layer_specs

# the batch each net is measured at (bench.py / BASELINE.json), next to the smallest training batch
BATCHES = {"vgg16_224": 128, "resnet50_imagenet224": 128, "alexnet_imagenet224": 128, "squeezenet1_0_imagenet224": 256,
           "shufflenetv2_224": 256, "mobilenetv1_imagenet224": 256, "mobilenetv1_cifar32": 8}
SFP7_NETS = ("squeezenet1_0_imagenet224", "shufflenetv2_224")   # BASELINE.json config 5


@pytest.fixture
def switches():
    L = _lib.load()
    old = {k: os.environ.get(k) for k in V.SWITCHES}
    try:
        yield lambda env: V.set_switches(L, env)
    finally:
        V.set_switches(L, {k: v for k, v in old.items() if v is not None})


def _report(row, need_gx=1, need_gw=1):
    return V.instance(_lib, V.make_desc(_lib, row), row.flags, row.operand == "codes", need_gx, need_gw)


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_the_table_reaches_what_it_claims_and_hits_its_edges(switches, row):
    switches(row.env)
    d = V.make_desc(_lib, row)
    L = _lib.load()
    kern = {"dw": "dw3x3_bwd", "pw": "pw_bwd_mfma_f32", "dense": "dense_bwd_mfma_f32"}[row.kind]
    assert L.slfp_conv2d_bwd_kernel_name_ex(ctypes.byref(d), row.flags).decode() == kern
    if row.operand == "codes":
        assert L.slfp_conv2d_bwd_codes_supported(ctypes.byref(d), row.flags) == 1
    got = _report(row)
    assert V.strip(got) == row.variant, (row.name, got)
    nums = V.numbers(got)
    for word in row.edges:
        assert V.edge_holds(row, word, nums), (row.name, word, got)
    # the halves of the string are what the launches of one output alone report, and the split is the same
    if row.kind != "dw":
        assert _report(row, 1, 0) + "+" + _report(row, 0, 1) == got
    else:
        assert _report(row, 1, 0) == got == _report(row, 0, 1)
    assert _report(row, 0, 0) == "none"
    # the workspace the split implies: the partials of the reduction fit the stated size
    ws = L.slfp_conv2d_bwd_workspace_bytes_ex(ctypes.byref(d), row.flags, 0, 1)
    if row.kind == "dw":
        assert ws >= nums["b"] * 10 * row.c_in * 4
    else:
        ncol = row.k[0] * row.k[1] * row.c_in
        assert ws >= nums["p"] * row.c_out * 4 + (nums["p"] * row.c_out * ncol * 4 if nums["p"] > 1 or row.kind == "dense" else 0)


def test_the_reporter_refuses_where_the_entry_points_do(switches):
    switches(None)
    L = _lib.load()
    pw = next(r for r in ROWS if r.name == "pw-6x10")
    d = V.make_desc(_lib, pw)
    assert V.instance(_lib, d, 0, 0).startswith("pw/gx/")
    assert V.instance(_lib, d, 0, 1) == "composite"           # codes need C_in % 4 == 0
    assert V.instance(_lib, d, 2, 0) == "composite"           # unknown flag bits
    assert L.slfp_debug_bwd_instance(None, 0, 0, 1, 1) == b"composite"
    dense = V.make_desc(_lib, next(r for r in ROWS if r.name == "dense-6x10"))
    assert V.instance(_lib, dense, 0, 0) == "composite"       # the dense family is behind SLFP_BWD_DENSE
    assert V.instance(_lib, dense, V.DENSE, 0).startswith("dense/gx/")
    dense.dil_h = 2
    assert V.instance(_lib, dense, V.DENSE, 0) == "composite"
    codes = V.make_desc(_lib, next(r for r in ROWS if r.name == "pw-68x124-codes-off4"))
    codes.x_layout = _lib.LAYOUT_NCHW
    assert V.instance(_lib, codes, 0, 1) == "composite" and V.instance(_lib, codes, 0, 0).startswith("pw/gx/")


def test_the_table_is_the_set_of_instances_the_launchers_can_select():
    assert len({r.name for r in ROWS}) == len(ROWS)
    table, want = {part for r in ROWS for part in r.variant.split("+")}, V.reachable()
    assert not want - table, f"instances no row reaches: {sorted(want - table)}"
    assert not table - want, f"instances no launcher selects: {sorted(table - want)}"
    # k_dw3x3_bwd 2 x 6; k_gemm_f32 8 (gx) + 8 x 6 (gw); k_dense_gx 3; k_dense_gw (4 + 1) x 6 -- `tab` counted once per format
    assert len(want) == 12 + 8 + 48 + 3 + 30
    assert {k for r in ROWS for k, _ in r.env} == set(V.SWITCHES)


# the edges the table has to keep, per family: a row that leaves takes its word with it
REQUIRED_EDGES = {
    "pw": {"ragged-co", "ragged-ci", "ragged-rows", "m-under-128", "m-over-128", "short-split", "partial-kstep", "kb-off-tile", "red-p<16",
           "red-p16-63", "red-p65+", "red-ncols-ragged", "red-gb-ragged", "cin-scalar", "linear", "codes-off4"},
    "dense": {"ragged-co", "ragged-ci", "ragged-rows", "tap-seam", "odd-phases", "empty-phases", "stem", "short-split", "partial-kstep",
              "kb-off-tile", "red-p<16", "red-p16-63", "red-p65+", "red-ncols-ragged", "cin-scalar", "codes-off4"},
    "dw": {"idle-lanes", "dead-channels", "unit-ragged", "small-image", "h1", "parity", "units>slots", "red-p16-63", "red-p65+",
           "red-p65+x64", "codes-off4"},
}


def test_the_table_keeps_every_edge_and_the_codes_rows_the_issue_names():
    for kind, want in REQUIRED_EDGES.items():
        got = {w for r in ROWS if r.kind == kind for w in r.edges}
        assert want <= got, (kind, sorted(want - got))
    assert {r.c_in for r in ROWS if r.kind == "dw" and r.operand == "f32"} >= {3, 6, 36, 64, 100, 116}
    assert {(r.h % 2, r.w % 2) for r in ROWS if r.kind == "dw" and r.stride == (2, 2)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    codes = [r for r in ROWS if r.operand == "codes"]
    for kind in ("pw", "dense"):
        assert any(r.kind == kind and r.c_out % 4 != 0 for r in codes)
        assert any(r.kind == kind and r.c_in >= 128 for r in codes)
        assert any(r.kind == kind and "short-split" in r.edges for r in codes)     # p > 1
    for kind in ("pw", "dense", "dw"):
        assert any(r.kind == kind and r.align % 16 != 0 for r in codes)
    assert all(r.align == 0 for r in ROWS if r.operand == "f32")
    # no tensor above a few MB
    for r in ROWS:
        ho, wo = V.out_hw(r)
        assert max(r.n * r.h * r.w * r.c_in, r.n * ho * wo * r.c_out) * 4 <= 10 << 20, r.name


def _spec_desc(s, n, qbits):
    return _lib.ConvDesc(n=n, c_in=s.c_in, h=s.h, w=s.w, c_out=s.c_out, kh=s.k[0], kw=s.k[1], stride_h=s.stride[0], stride_w=s.stride[1],
                         pad_h=s.pad[0], pad_w=s.pad[1], dil_h=1, dil_w=1, groups=s.groups, x_layout=_lib.LAYOUT_NHWC,
                         y_layout=_lib.LAYOUT_NHWC, qbits=qbits, ka=float(np.float32(s.Ka)), kw_scale=float(np.float32(s.Kw)),
                         mfma_passes=0, reserved=0)


def test_census_of_the_nets_is_covered_by_the_table(switches):
    """Every layer of every net that the backward covers, under flags 0 and SLFP_BWD_DENSE, at n = 2 and at the batch the net is
    measured with, on float32 and (where the entry point takes them) on codes: the instances it reports must each have a row."""
    switches(None)
    L = _lib.load()
    assert set(BATCHES) == set(layer_specs.nets())
    table = {part for r in ROWS for part in r.variant.split("+")}
    census = {}
    for net, batch in BATCHES.items():
        for i, s in enumerate(layer_specs.conv_layers(net)):
            for n in (2, batch):
                for qbits in (8, 7) if net in SFP7_NETS else (8,):
                    d = _spec_desc(s, n, qbits)
                    for flags in (0, V.DENSE):
                        if not L.slfp_conv2d_bwd_supported_ex(ctypes.byref(d), flags):
                            assert V.instance(_lib, d, flags, 0) == "composite", (net, i)
                            continue
                        for x_codes in (0, 1):
                            if x_codes and not L.slfp_conv2d_bwd_codes_supported(ctypes.byref(d), flags):
                                assert V.instance(_lib, d, flags, 1) == "composite", (net, i)
                                continue
                            got = V.instance(_lib, d, flags, x_codes)
                            assert got not in ("composite", "none"), (net, i, got)
                            for part in V.strip(got).split("+"):
                                census.setdefault(part, set()).add((net, i))
    print("\nbackward instance census (instance: layers)")
    for v in sorted(census):
        print(f"  {v:36s} {len(census[v]):4d}")
    assert len(census) >= 12
    missing = sorted(set(census) - table)
    assert not missing, f"instances the nets run on without a row: {missing}"


_LAYERS = {}
for _r in ROWS:
    _LAYERS.setdefault(V.layer_key(_r), _r)


@pytest.mark.parametrize("row", list(_LAYERS.values()), ids=[r.name for r in _LAYERS.values()])
def test_the_reference_leaves_no_element_out(row):
    """The float64 reference of the row's seeded inputs is finite and every gx / gw / gb element has a non-zero sum of |terms|, so
    that _bwd_cases._errors measures all of them; where the geometry makes an element an exact zero (1x1 stride 2's dead phases, the
    taps of a one-row image that only meet padding) the row says so and the zeros are exactly those the geometry gives."""
    x, w, gy = V.inputs(row)
    a = x.abs()
    for lo_, hi_ in ((0.0, 0.0), (1e-30, 0.0625 * V.KA), (0.0625 * V.KA, 15.0 * V.KA), (16.0 * V.KA, 1e30)):   # every code range
        assert int(((a >= lo_) & (a <= hi_)).sum()) > 0
    (gx, ax), (gw, aw), (gb, ab) = V.reference(row)
    for t in (gx, ax, gw, aw, gb, ab):
        assert bool(torch.isfinite(t).all())
    assert bool((ab > 0).all())
    if not row.zeros:
        assert bool((ax > 0).all()) and bool((aw > 0).all()), (int((ax == 0).sum()), int((aw == 0).sum()))
        return
    if row.kind == "dense":   # 1x1 stride 2: only the even rows and columns are read
        live = torch.zeros(row.h, row.w, dtype=torch.bool)
        live[::2, ::2] = True
        assert bool((ax[:, :, live] > 0).all()) and bool((ax[:, :, ~live] == 0).all()) and bool((gx[:, :, ~live] == 0).all())
        assert bool((aw > 0).all())
    else:                     # H = 1, pad 1: the kh = 0 and kh = 2 taps only meet padding
        assert row.h == 1 and bool((ax > 0).all())
        assert bool((aw[:, :, 1, :] > 0).all()) and bool((aw[:, :, (0, 2), :] == 0).all()) and bool((gw[:, :, (0, 2), :] == 0).all())


def test_the_nan_placement_is_not_empty():
    for row in _LAYERS.values():
        m = V.nan_mask(row)
        assert 0 < int(m.sum()) < m.numel() or row.c_in == 1, row.name
