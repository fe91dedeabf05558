"""Host side of the dense k x k kernel selection (csrc/conv_dense.hip: dense_select): the case table of tests/_dense_variants.py
reaches the variants it names, and covers every variant a measured workload runs on.  No device is touched:
slfp_debug_dense_variant prints the selection the launch consumes."""
import ctypes
import os

import numpy as np
import pytest

from _dense_variants import ROWS, SWITCHES, TILINGS, make_desc, set_switches
from cnns_slfp_quantization_amd import _lib, layer_specs

# the batch sizes the dense nets are measured at: BASELINE.json configs 3-5 / bench.py's OTHER_CONFIGS (ResNet-50: the per-GPU
# slice of global batch 1024 on 8 GPUs), each also as bench.py's two image groups of half the batch; AlexNet like VGG-16
BATCHES = {"vgg16_224": (128, 64), "resnet50_imagenet224": (128, 64), "alexnet_imagenet224": (128, 64),
           "squeezenet1_0_imagenet224": (256, 128), "shufflenetv2_224": (256, 128),
           "mobilenetv1_imagenet224": (256, 128), "mobilenetv1_cifar32": (8,)}
SFP7_NETS = ("squeezenet1_0_imagenet224", "shufflenetv2_224")   # BASELINE.json config 5


def _variant(d, x_codes=0):
    return _lib.load().slfp_debug_dense_variant(ctypes.byref(d), x_codes).decode()


@pytest.fixture
def switches():
    L = _lib.load()
    old = {k: os.environ.get(k) for k in SWITCHES}
    yield lambda env: set_switches(L, env)
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
    assert name == ("dense_mfma_f16_exact" if row.qbits == 7 else "dense_mfma_f16x3" if row.passes == 3 else "dense_mfma_f16x1"), name
    assert _variant(d) == row.variant, row


def test_names_are_unique_and_the_reporter_says_none_outside_the_family(switches):
    assert len({r.name for r in ROWS}) == len(ROWS)
    switches(None)
    L = _lib.load()
    for s in layer_specs.conv_layers("mobilenetv1_imagenet224"):   # stem, depthwise and pointwise layers only
        d = _spec_desc(s, 4, 8, 0)
        assert not L.slfp_conv2d_kernel_name(ctypes.byref(d)).decode().startswith("dense_mfma")
        assert _variant(d) == "none" and _variant(d, 1) == "none", s


def test_census_of_the_measured_workloads_is_covered_by_the_table(switches):
    """Every dense layer of every net, at the batch sizes it is measured with, in every mode it is run in, with float32 and with
    codes on the input side: the variant the cost model gives it must have a small-shape row.  A tiling the cost model starts
    giving a workload without such a row fails here -- that is what keeps tests/test_gpu_dense_variants.py complete."""
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
                    if not kern.startswith("dense_mfma"):
                        assert _variant(d) == "none", (net, i, kern)
                        continue
                    for x_codes in (0, 1):
                        v = _variant(d, x_codes)
                        assert v != "none", (net, i, kern)
                        census.setdefault(v, []).append((net, i, n, kern, "codes" if x_codes else "f32"))
    print("\ndense variant census (variant: launches; layers)")
    for v in sorted(census):
        layers = sorted({(net, i) for net, i, _, _, _ in census[v]})
        print(f"  {v:24s} {len(census[v]):4d}  " + " ".join(f"{net.split('_')[0]}#{i}" for net, i in layers))
    table = {r.variant for r in ROWS}
    assert len(census) >= 4   # VGG-16 alone runs on several
    assert set(census) <= table, sorted(set(census) - table)


def _parts(v):
    return v.split("/")


def test_the_table_spans_every_tiling_body_and_specialisation():
    per_tile = [r for r in ROWS if not r.variant.startswith("res/")]
    for want_q, want_p in ((8, 1), (7, 1)):   # f16x1 and exact
        got = {int(_parts(r.variant)[0]) for r in per_tile if r.qbits == want_q and r.passes == want_p}
        assert got == set(TILINGS), (want_q, got)
    assert {_parts(r.variant)[1] for r in per_tile} == {"k3x3", "gen"}
    assert {_parts(r.variant)[2] for r in per_tile} == {"nwb2", "nwb3"}
    assert {_parts(r.variant)[3] for r in per_tile} == {"ns3", "ns6", "ns9"}
    assert {_parts(r.variant)[4] for r in per_tile} == {"p1", "p2"}
    assert {r.variant for r in ROWS if r.variant.startswith("res/")} == {"res/mt1/ns3", "res/mt2/ns6", "res/mt1/ns3/encx", "res/mt2/ns6/encx"}
    used = {k for r in ROWS for k, _ in r.env}
    assert used == {"SLFP_DENSE_CFG", "SLFP_DENSE_GENERIC", "SLFP_DENSE_NWB"}
    generic = {int(_parts(r.variant)[0]) for r in ROWS if ("SLFP_DENSE_GENERIC", "1") in r.env}
    assert generic >= {424, 244, 811}
    assert any(("SLFP_DENSE_NWB", "2") in r.env and r.variant.startswith("424/") for r in ROWS)
