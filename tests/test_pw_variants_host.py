"""Host side of the pointwise (1x1) kernel selection (csrc/conv_pw.hip: pw_select, csrc/conv_pw_codes.hip: pwc_select): the case
table of tests/_pw_variants.py reaches the instances it names, spans every template argument a launcher can produce, and covers
every instance a measured workload runs on.  No device is touched: slfp_debug_pw_variant prints the selection the launch consumes."""
import ctypes
import os
import re

import numpy as np
import pytest

from _pw_variants import IFACES, ROWS, SWITCHES, make_desc, set_switches, strip_grid, variant
from cnns_slfp_quantization_amd import _lib, layer_specs

# the batch sizes the nets are measured at (bench.py; tests/test_dense_variants_host.py), each also as bench.py's two image groups
BATCHES = {"vgg16_224": (128, 64), "resnet50_imagenet224": (128, 64), "alexnet_imagenet224": (128, 64),
           "squeezenet1_0_imagenet224": (256, 128), "shufflenetv2_224": (256, 128),
           "mobilenetv1_imagenet224": (256, 128), "mobilenetv1_cifar32": (8,)}
SFP7_NETS = ("squeezenet1_0_imagenet224", "shufflenetv2_224")   # BASELINE.json config 5


@pytest.fixture
def switches():
    L = _lib.load()
    old = {k: os.environ.get(k) for k in SWITCHES}
    try:
        yield lambda env: set_switches(L, env)
    finally:
        set_switches(L, {k: v for k, v in old.items() if v is not None})


def _spec_desc(s, n, qbits, passes):
    return _lib.ConvDesc(n=n, c_in=s.c_in, h=s.h, w=s.w, c_out=s.c_out, kh=s.k[0], kw=s.k[1], stride_h=s.stride[0], stride_w=s.stride[1],
                         pad_h=s.pad[0], pad_w=s.pad[1], dil_h=1, dil_w=1, groups=s.groups, x_layout=_lib.LAYOUT_NHWC,
                         y_layout=_lib.LAYOUT_NHWC, qbits=qbits, ka=float(np.float32(s.Ka)), kw_scale=float(np.float32(s.Kw)),
                         mfma_passes=passes, reserved=0)


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_the_table_reaches_what_it_claims(switches, row):
    switches(row.env)
    d = make_desc(_lib, row)
    name = _lib.load().slfp_conv2d_kernel_name(ctypes.byref(d)).decode()
    assert name == ("pw_mfma_f16_exact" if row.qbits == 7 else "pw_mfma_f16x3" if row.passes == 3 else "pw_mfma_f16x1"), name
    assert variant(_lib, d, row.iface, row.qbits) == row.variant, row


def test_names_are_unique_and_the_reporter_says_none_outside_the_family(switches):
    assert len({r.name for r in ROWS}) == len(ROWS)
    switches(None)
    L = _lib.load()
    for s in layer_specs.conv_layers("vgg16_224"):   # dense 3x3 layers only
        d = _spec_desc(s, 4, 8, 0)
        assert not L.slfp_conv2d_kernel_name(ctypes.byref(d)).decode().startswith("pw_mfma")
        for iface in IFACES:
            assert variant(_lib, d, iface, 8) == "none", (s, iface)
    assert L.slfp_debug_pw_variant(None, None, 0, 0, 0) == b"none"
    # refused calls report "none" as well: a residual operand on an 8-byte-access layer, code output of 40 channels
    r58 = next(r for r in ROWS if r.name == "st-a8-58-58")
    assert variant(_lib, make_desc(_lib, r58), "res", 8) == "none"
    r40 = next(r for r in ROWS if r.name == "st-k64")
    assert variant(_lib, make_desc(_lib, r40), "entry", 8) == "none" and variant(_lib, make_desc(_lib, r40), "cout", 8) == "none"


def test_the_grid_switch_only_adds_its_word(switches):
    """SLFP_PW_GRID changes no choice but the persistent grids' size: every row's string under its own switches plus the cap is the
    same string with /grid<n> on the persistent kernels and unchanged on the others."""
    for row in ROWS:
        if ("SLFP_PW_GRID", "1") in row.env or ("SLFP_PW_GRID", "3") in row.env:
            continue
        env = dict(row.env)
        env["SLFP_PW_GRID"] = "2"
        switches(env)
        v = variant(_lib, make_desc(_lib, row), row.iface, row.qbits)
        persistent = row.variant.split("/")[0] in ("stream", "pwc-stream", "slice")
        assert v == row.variant + ("/grid2" if persistent else ""), (row, v)


def test_census_of_the_measured_workloads_is_covered_by_the_table(switches):
    """Every pointwise layer of every net, at the batch sizes it is measured with, in every mode it is run in, on every interface
    a fusion pass can put it on: float32 (all modes); codes in, codes out and chain entry (fusion.link_codes / link_codes_traced:
    any net, single-pass modes); residual, residual on codes and residual + codes (fusion.fuse_residual / link_trunk: conv3 of a
    ResNet-50 bottleneck, C_out = 4 C_in at stride 1); the Fire slice (fusion.fuse_fire: SqueezeNet).  The instance the launchers
    give it must have a small-shape row: a new kernel instance fails here until it has one -- that is what keeps
    tests/test_gpu_pw_variants.py complete."""
    switches(None)
    L = _lib.load()
    census = {}
    assert set(BATCHES) == set(layer_specs.nets())
    for net, batches in BATCHES.items():
        modes = [(8, _lib.MFMA_F16X1), (8, _lib.MFMA_F16X3)] + ([(7, _lib.MFMA_F16X1)] if net in SFP7_NETS else [])
        for i, s in enumerate(layer_specs.conv_layers(net)):
            for n in batches:
                for qbits, passes in modes:
                    d = _spec_desc(s, n, qbits, passes)
                    kern = L.slfp_conv2d_kernel_name(ctypes.byref(d)).decode()
                    if "pw_mfma" not in kern:
                        assert variant(_lib, d, "f32", qbits, s.Ka) == "none", (net, i, kern)
                        continue
                    v = variant(_lib, d, "f32", qbits, s.Ka)
                    assert v != "none", (net, i, kern)
                    census.setdefault(v, []).append((net, i, "f32"))
                    bottleneck_conv3 = net.startswith("resnet50") and s.stride == (1, 1) and s.c_out == 4 * s.c_in
                    for iface in IFACES[1:]:
                        if passes == _lib.MFMA_F16X3 and iface != "res":
                            continue   # the code paths are single-pass
                        if iface in ("res", "cres", "cdual") and not bottleneck_conv3:
                            continue
                        if iface == "slice" and not net.startswith("squeezenet"):
                            continue
                        v = variant(_lib, d, iface, qbits, s.Ka)
                        if v != "none":
                            census.setdefault(v, []).append((net, i, iface))
    print("\npointwise variant census (variant: launches; layers)")
    for v in sorted(census):
        layers = sorted({(net, i) for net, i, _ in census[v]})
        print(f"  {v:40s} {len(census[v]):4d}  " + " ".join(f"{net.split('_')[0]}#{i}" for net, i in layers[:8]) + (" ..." if len(layers) > 8 else ""))
    table = {strip_grid(r.variant) for r in ROWS}
    assert len(census) >= 60   # five kernels, their forms, three modes
    assert all("/grid" not in v for v in census)
    assert set(census) <= table, sorted(set(census) - table)


def _has(pattern):
    return any(re.fullmatch(pattern, strip_grid(r.variant)) for r in ROWS)


def test_the_table_spans_every_instance_a_launcher_can_produce():
    # ---- k_pw_stream: every KS instance in both K forms and A8 where A8 can occur; TAB, STG, RES, YC both ways; the three modes
    for ks in (1, 2, 3, 4, 6, 8):
        for kform in ("kfull", "kpart"):
            assert _has(rf"stream/ks{ks}/{kform}/tab/(stg|dir)/p1/act8"), (ks, kform)
            assert _has(rf"stream/ks{ks}/{kform}/tab/dir/p1/act8/yc"), (ks, kform)
        assert _has(rf"stream/ks{ks}/k(full|part)/tab/(stg|dir)/p3/act8"), ks
        assert _has(rf"stream/ks{ks}/k(full|part)/tab/(stg|dir)/p1/sfp7"), ks
    for ks in (1, 2, 4, 6):   # A8 above KS = 2 included.  (KS 3 and 8 with A8 exist as instances too: K = 66..94 / 194..254 even,
        assert _has(rf"stream/ks{ks}/a8/tab/dir/p1/act8"), ks   # no multiple of 4 -- the same body, the same guarded loads)
    for word in ("long/dir/p1/act8", "long/dir/p3/act8", "long/dir/p1/sfp7"):
        assert _has(rf"stream/ks\d/kfull/{word}") or _has(rf"stream/ks\d/kpart/{word}"), word
    assert _has(r"stream/ks\d/a8/long/dir/p1/act8")
    assert _has(r"stream/ks6/kfull/tab/stg/p1/act8") and _has(r"stream/ks6/kpart/tab/stg/p1/act8")   # SLFP_PW_STG_MAXKS=8
    assert _has(r"stream/ks[1-4]/kfull/tab/dir/p1/act8") and _has(r"stream/ks8/kpart/tab/dir/p1/act8")   # SLFP_PW_NOSTG / MAXKS=0
    # RES: staged where the default rule stages, direct at KS 6 -- launch_stream_ks refuses any other pairing ("no residual form of
    # this kernel variant"), as it refuses RES with A8 or the long form, and YC with A8, three passes or the long form
    assert _has(r"stream/ks[1248]/kfull/tab/stg/p1/act8/res") and _has(r"stream/ks6/kfull/tab/dir/p1/act8/res")
    assert _has(r"stream/ks\d/kpart/tab/stg/p1/act8/res") and _has(r"stream/ks6/kpart/tab/dir/p1/act8/res")
    assert _has(r"stream/ks\d/k(full|part)/tab/(stg|dir)/p3/act8/res") and _has(r"stream/ks\d/kfull/tab/stg/p1/sfp7/res")
    # ---- k_pw_tiled: every tiling, KFULL both ways, each form; three passes have no {1,8,4} (pw_select: passes == 1)
    for t in (411, 222, 144, 184):
        for kform in ("kfull", "kpart"):
            assert _has(rf"tiled/{t}/{kform}/tab/stg/p1/act8"), (t, kform)
        assert _has(rf"tiled/{t}/k(full|part)/tab/stg/p1/sfp7"), t
        assert _has(rf"tiled/{t}/k(full|part)/tab/stg/p1/act8/res"), t
        assert _has(rf"tiled/{t}/k(full|part)/tab/dir/p1/act8/yc"), t
        if t != 184:
            assert _has(rf"tiled/{t}/k(full|part)/tab/stg/p3/act8"), t
    assert not _has(r"tiled/184/.*/p3/.*")
    for word in ("tab/dir/p1/act8", "tab/dir/p3/act8", "long/dir/p1/act8", "long/dir/p3/act8", "long/dir/p1/sfp7"):
        assert _has(rf"tiled/\d+/k(full|part)/{word}"), word
    assert _has(r"tiled/\d+/kfull/tab/stg/p3/act8/res") and _has(r"tiled/\d+/kfull/tab/stg/p1/sfp7/res")
    # ---- the kernels on codes: every (KS, XW, HALF) instance, both NTS, every tiling, each in its four forms (YC, RES, DUAL)
    forms = ("f32", "yc", "res", "res/dual")
    for w in ("ks1/half", "ks2/half", "ks1/dw", "ks2/xw", "ks3/dw", "ks4/xw", "ks8/xw"):   # pwc_applicable admits no other K
        for f in forms:
            assert _has(rf"pwc-stream/{w}/act8/{f}"), (w, f)
        assert _has(rf"pwc-stream/{w}/sfp7/(f32|yc)"), w
    for nts in (4, 8):
        for f in forms:
            assert _has(rf"slice/nts{nts}/act8/{f}"), (nts, f)
        assert _has(rf"slice/nts{nts}/sfp7/.*"), nts
    for t in (411, 222, 144, 184):
        for f in forms:
            assert _has(rf"pwc-tiled/{t}/act8/{f}"), (t, f)
    assert _has(r"pwc-tiled/\d+/sfp7/yc") and _has(r"pwc-tiled/\d+/sfp7/res")
    # ---- capped grids: every persistent kernel in each of its forms, the stream kernels with one and with three workgroups
    capped = {r.variant for r in ROWS if "/grid" in r.variant}
    for f in forms:
        assert any(re.fullmatch(rf"pwc-stream/.*/{f}/grid\d", v) for v in capped), f
        assert any(re.fullmatch(rf"slice/nts8/act8/{f}/grid1", v) for v in capped), f
    for tail in ("", "/res", "/yc"):
        assert any(re.fullmatch(rf"stream/ks\d/k(full|part)/tab/(stg|dir)/p1/act8{tail}/grid\d", v) for v in capped), tail
    assert any(v.startswith("stream/") and v.endswith("/grid3") for v in capped) and any(v.startswith("pwc-stream/") and v.endswith("/grid3") for v in capped)
    assert {k for r in ROWS for k, _ in r.env} == set(SWITCHES)
    # stride 2 and the slice-stride store on every kernel that has them
    assert {r.variant.split("/")[0] for r in ROWS if r.stride == 2} == {"stream", "tiled", "pwc-stream", "slice", "pwc-tiled"}
    assert {r.variant.split("/")[0] for r in ROWS if r.iface == "slice"} == {"pwc-stream", "slice", "pwc-tiled"}
