"""GPU: the dense backward family (options.backward = "hip_all", SLFP_BWD_DENSE, kernel dense_bwd_mfma_f32) against the
float64 reference that tests/test_gpu_backward.py uses (tests/_bwd_cases.py: torch.nn.grad on the C oracle's xq / wq), with the
same error measures and bars: elementwise |g - ref| / sum|terms| <= 1e-5 and tensor-relative L2 <= 1e-6 for gx, gw and gb.  The composite's error on
the same inputs is printed next to it."""
import functools
import os

import numpy as np
import pytest
import torch

import _aniso_cases as A
import _bwd_cases
from _bwd_cases import DEV, _contractions, _conv_grads, _errors, _make, _reference, _x_values
from oracle import slfp_oracle
from cnns_slfp_quantization_amd import _lib, layer_specs, optimizer as O
from cnns_slfp_quantization_amd import conv2d_func as cf
from cnns_slfp_quantization_amd.conv2d_func import conv2d_Q, linear_Q

pytestmark = pytest.mark.gpu
DENSE = "dense_bwd_mfma_f32"
_check_case = functools.partial(_bwd_cases._check_case, mode="hip_all", kernels=(DENSE,))


@pytest.fixture(autouse=True)
def _composite_default():
    cf.options.backward = "composite"
    yield
    cf.options.backward = "composite"


def _two(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _spec(c_in, c_out, k, s, p, h, w=None, ka=0.2, kw=0.1):
    k, s, p = _two(k), _two(s), _two(p)
    w = h if w is None else w
    ho, wo = (h + 2 * p[0] - k[0]) // s[0] + 1, (w + 2 * p[1] - k[1]) // s[1] + 1
    return layer_specs.ConvSpec(c_in, c_out, k, s, p, 1, False, h, w, ho, wo, ka, kw)


# ---- 1. the geometry table ------------------------------------------------------------------------------------------------
TABLE = [
    ("3x3s1p1-16x32@14", _spec(16, 32, 3, 1, 1, 14)),      # baseline
    ("3x3s2p1-32x32@15", _spec(32, 32, 3, 2, 1, 15)),      # odd extent: the last window and the phase sizes differ
    ("3x3s2p1-32x32@14", _spec(32, 32, 3, 2, 1, 14)),
    ("1x1s2p0-32x64@14", _spec(32, 64, 1, 2, 0, 14)),      # three empty phases in gx
    ("1x1s2p0-32x64@15", _spec(32, 64, 1, 2, 0, 15)),
    ("5x5s1p2-8x16@13", _spec(8, 16, 5, 1, 2, 13)),
    ("3x3s1p1-40x24@9", _spec(40, 24, 3, 1, 1, 9)),        # C_out = 24: a tap seam inside a 16-deep k-chunk
    ("3x3s1p1-6x10@9", _spec(6, 10, 3, 1, 1, 9)),          # the scalar path: neither channel count a multiple of 4
    ("3x3s1p1-80x144@7", _spec(80, 144, 3, 1, 1, 7)),      # ragged 64 / 128 tiles on both GEMM sides
    ("3x3s1p0-16x16@8", _spec(16, 16, 3, 1, 0, 8)),        # no padding
    ("3x3s3p1-16x16@11", _spec(16, 16, 3, 3, 1, 11)),      # a stride with no special case
    ("stem3x3s2p1-3x32@32", _spec(3, 32, 3, 2, 1, 32)),
    ("stem7x7s2p3-3x16@32", _spec(3, 16, 7, 2, 3, 32)),
    ("stem7x7s2p0-3x24@33", _spec(3, 24, 7, 2, 0, 33)),
    ("stem11x11s4p2-3x8@35", _spec(3, 8, 11, 4, 2, 35)),
    ("stem3x3s1p1-3x24@20", _spec(3, 24, 3, 1, 1, 20)),
]
TABLE_BY_ID = dict(TABLE)


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("i", range(len(TABLE)), ids=[t[0] for t in TABLE])
def test_geometry_table_against_float64(i, channels_last):
    label, spec = TABLE[i]
    gen = torch.Generator().manual_seed(4000 + 2 * i + int(channels_last))
    _check_case(spec, 2 + i % 2, 8 if i % 2 == 0 else 7, (i // 2) % 2 == 0, gen, channels_last, label=label)


# ---- 2. non-square and anisotropic ---------------------------------------------------------------------------------------
def _aniso():
    out = []
    for c in A.ROWS:
        if c.g != 1 or c.dh != 1 or c.dw != 1:
            continue
        if (c.kh, c.kw, c.sh, c.sw, c.ph, c.pw) == (1, 1, 1, 1, 0, 0):
            continue
        out += [c, A.twin(c)]
    return out


ANISO = _aniso()


def _aniso_id(c):
    return f"{c.C}x{c.O}k{c.kh}x{c.kw}s{c.sh}x{c.sw}p{c.ph}x{c.pw}@{c.H}x{c.W}"


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("i", range(len(ANISO)), ids=[_aniso_id(c) for c in ANISO])
def test_non_square_and_anisotropic_against_float64(i, channels_last):
    c = ANISO[i]
    spec = _spec(c.C, c.O, (c.kh, c.kw), (c.sh, c.sw), (c.ph, c.pw), c.H, c.W, ka=A.KA, kw=A.KW)
    assert (spec.h_out, spec.w_out) == A.out_hw(c)
    gen = torch.Generator().manual_seed(5000 + 2 * i + int(channels_last))
    _check_case(spec, 2, 8 if i % 2 == 0 else 7, (i // 2) % 2 == 0, gen, channels_last, label="aniso")


# ---- 3. sparse gy ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["3x3s1p1-16x32@14", "3x3s2p1-32x32@15", "1x1s2p0-32x64@15", "stem7x7s2p3-3x16@32"])
def test_sparse_gy_probe(label):
    """gy non-zero at 2 positions per channel: each gw element sums a handful of terms, so one wrong gather index or one
    wrong quantization code is a percent-level error, not noise."""
    _check_case(TABLE_BY_ID[label], 2, 8, True, torch.Generator().manual_seed(9), channels_last=True, sparse=True, label="sparse")


# ---- 4. at size -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [_spec(128, 128, 3, 1, 1, 28, ka=0.21, kw=0.037), _spec(256, 256, 3, 2, 1, 28, ka=0.21, kw=0.037),
                                  _spec(512, 1024, 1, 2, 0, 28, ka=0.21, kw=0.037)], ids=["3x3s1-128@28", "3x3s2-256@28", "1x1s2-512x1024@28"])
def test_at_size(spec):
    """Many splits of the gw contraction, the reduction and the phase ordering at a real extent."""
    _check_case(spec, 32, 8, True, torch.Generator().manual_seed(7), channels_last=True, label="at size")


# ---- 5. module level --------------------------------------------------------------------------------------------------------
def test_module_level_kernel_names_layouts_and_needs():
    gen = torch.Generator().manual_seed(3)
    dense = _make(_spec(16, 32, 3, 1, 1, 14), 8, True, gen)
    x = _x_values((3, 16, 14, 14), 0.2, gen).to(DEV)
    gy = torch.randn(3, 32, 14, 14, generator=gen).to(DEV)
    for fmt in (torch.contiguous_format, torch.channels_last):
        xi = x.contiguous(memory_format=fmt)
        full = _conv_grads(dense, xi, gy, "hip_all")
        assert dense._last_bwd_kernel == DENSE
        assert full[0].is_contiguous(memory_format=fmt)
        for need in ((False, True, True), (True, False, True), (True, True, False), (False, False, True), (True, False, False)):
            got = _conv_grads(dense, xi, gy, "hip_all", need)
            assert dense._last_bwd_kernel == DENSE
            for k in range(3):
                assert (got[k] is None) == (not need[k]), (need, k)
                if need[k]:
                    assert torch.equal(got[k], full[k]), (need, k)
        # out.sum().backward(): a stride-0 gy
        ones = _conv_grads(dense, xi, torch.ones(3, 32, 14, 14, device=DEV), "hip_all")
        cf.options.backward = "hip_all"
        xs = xi.detach().clone().requires_grad_(True)
        dense.zero_grad(set_to_none=True)
        dense(xs).sum().backward()
        assert dense._last_bwd_kernel == DENSE
        assert xs.grad.is_contiguous(memory_format=fmt)
        assert torch.equal(xs.grad, ones[0]) and torch.equal(dense.weight.grad, ones[1]) and torch.equal(dense.bias.grad, ones[2])
        # the same module under "hip" stays on the composite
        _conv_grads(dense, xi, gy, "hip")
        assert dense._last_bwd_kernel == "composite"
        # the full run is right: the float64 reference and the bars of every other case (the composite is no yardstick
        # for single elements: two float32 sums of 288 signed terms differ by ~1e-6 of the sum of |terms| where they cancel)
        refs = _reference(x.cpu(), dense.weight.detach().cpu(), gy.cpu(), dense)
        for got, ref in zip(full[:3], refs):
            e, l = _errors(got, ref)
            assert e <= 1e-5 and l <= 1e-6, (e, l)
    dw = _make(layer_specs.ConvSpec(64, 64, (3, 3), (1, 1), (1, 1), 64, False, 14, 14, 14, 14, 0.2, 0.1), 8, False, gen, bias=False)
    _conv_grads(dw, _x_values((2, 64, 14, 14), 0.2, gen).to(DEV), torch.randn(2, 64, 14, 14, generator=gen).to(DEV), "hip_all")
    assert dw._last_bwd_kernel == "dw3x3_bwd"
    pw = _make(_spec(32, 48, 1, 1, 0, 8), 8, True, gen)
    _conv_grads(pw, _x_values((3, 32, 8, 8), 0.2, gen).to(DEV), torch.randn(3, 48, 8, 8, generator=gen).to(DEV), "hip_all")
    assert pw._last_bwd_kernel == "pw_bwd_mfma_f32"
    for m in (dw, pw, dense):
        m.weight.requires_grad_(True)


def test_linear_q_is_the_same_under_hip_all():
    gen = torch.Generator().manual_seed(4)
    lin = linear_Q(8, 0.05, 0.3)(256, 100).to(DEV)
    x = _x_values((4, 7, 256), 0.3, gen).to(DEV)
    gy = torch.randn(4, 7, 100, generator=gen).to(DEV)
    res = {}
    for mode in ("hip", "hip_all"):
        cf.options.backward = mode
        xi = x.clone().requires_grad_(True)
        lin.zero_grad(set_to_none=True)
        lin(xi).backward(gy)
        assert lin._last_bwd_kernel == "pw_bwd_mfma_f32"
        res[mode] = (xi.grad, lin.weight.grad, lin.bias.grad)
    for a, b in zip(res["hip"], res["hip_all"]):
        assert torch.equal(a, b)


# ---- 6. determinism -------------------------------------------------------------------------------------------------------
def test_deterministic():
    gen = torch.Generator().manual_seed(6)
    spec = TABLE_BY_ID["3x3s2p1-32x32@15"]
    mod = _make(spec, 8, True, gen)
    x = _x_values((3, spec.c_in, spec.h, spec.w), 0.2, gen).to(DEV).contiguous(memory_format=torch.channels_last)
    gy = torch.randn(3, spec.c_out, spec.h_out, spec.w_out, generator=gen).to(DEV)
    a = _conv_grads(mod, x, gy, "hip_all")[:3]
    b = _conv_grads(mod, x, gy, "hip_all")[:3]
    assert mod._last_bwd_kernel == DENSE
    for u, v in zip(a, b):
        assert torch.equal(u, v)


# ---- 7. quantizer identity ------------------------------------------------------------------------------------------------
def _class_edges(ka, fmt):
    """Both float32 neighbours of every class edge of Q_fmt(x / ka): the quantizer is monotone, so between two adjacent
    levels the edge is found by bisection on the float32 bit patterns (the oracle decides).  The probe values that locate
    the levels include the fixture's recorded inputs (tests/golden/quantizer_spot_golden.json, N(0, 5^2), scaled to Ka)."""
    from make_spot_golden import quantizer_inputs
    probe = np.concatenate([np.exp2(np.linspace(-12, 6, 4096)).astype(np.float32) * np.float32(ka),
                            np.abs(quantizer_inputs(torch).numpy()[:8192]) * np.float32(ka / 5.0)]).astype(np.float32)
    probe = np.unique(probe)                                     # sorted, positive
    q = slfp_oracle.quantize(probe, ka, fmt)
    first = np.concatenate([[True], q[1:] != q[:-1]])
    lo = probe[np.concatenate([first[1:], [False]])].view(np.uint32).astype(np.int64)   # last probe of a level
    hi = probe[first][1:].view(np.uint32).astype(np.int64)                              # first probe of the next one
    assert len(lo) == len(hi) and len(lo) >= 16
    lo_q = slfp_oracle.quantize(lo.astype(np.uint32).view(np.float32), ka, fmt)
    for _ in range(33):
        mid = (lo + hi) // 2
        same = slfp_oracle.quantize(mid.astype(np.uint32).view(np.float32), ka, fmt) == lo_q
        lo, hi = np.where(same, mid, lo), np.where(same, hi, mid)
    assert (hi - lo == 1).all()
    e = np.concatenate([lo, hi]).astype(np.uint32).view(np.float32)
    return np.concatenate([e, -e, np.zeros(1, np.float32)])


@pytest.mark.parametrize("q", [8, 7])
def test_quantizer_identity_on_class_edges(q):
    """x = every class edge of QA(x / Ka), tiled: gw from the kernel's encode-on-load equals the float64 contraction built
    from slfp_quantize_f32(x) on the device (and the device's xq equals the oracle's, bit for bit)."""
    gen = torch.Generator().manual_seed(11)
    spec = TABLE_BY_ID["3x3s1p1-16x32@14"]
    mod = _make(spec, q, True, gen)
    ka = cf._f32(mod.Ka)
    edges = _class_edges(ka, 0 if q == 8 else 2)
    shape = (2, spec.c_in, spec.h, spec.w)
    count = int(np.prod(shape))
    assert len(edges) < count
    x = torch.from_numpy(np.resize(edges, count)[torch.randperm(count, generator=gen).numpy()].reshape(shape).copy())
    gy = torch.randn(2, spec.c_out, spec.h_out, spec.w_out, generator=gen)
    xd = x.to(DEV).contiguous(memory_format=torch.channels_last)
    xq = cf.hip_quantize(xd, ka, cf._act_fmt(q)).cpu()
    assert np.array_equal(xq.numpy().view(np.uint32), slfp_oracle.quantize(x.numpy(), ka, 0 if q == 8 else 2).view(np.uint32))
    assert xq.unique().numel() >= 32
    w = mod.weight.detach().cpu()
    wq = torch.from_numpy(slfp_oracle.quantize(w.numpy(), cf._f32(mod.Kw), 1 if q == 8 else 2)).double()
    refs = _contractions(xq.double(), wq, gy, mod, x.shape, w.shape)
    for fmt in (torch.channels_last, torch.contiguous_format):
        _, gw, _, _ = _conv_grads(mod, xd.contiguous(memory_format=fmt), gy.to(DEV), "hip_all")
        assert mod._last_bwd_kernel == DENSE
        e, l = _errors(gw, refs[1])
        print(f"class edges q{q}: gw {e:.2e} {l:.2e}")
        assert e <= 1e-5 and l <= 1e-6, (e, l)


# ---- 8. a three-step fine-tune ----------------------------------------------------------------------------------------------
class _Block(torch.nn.Module):
    """A 3x3 stem, one bottleneck (1x1, 3x3 stride 2, 1x1) with a 1x1 stride-2 downsample shortcut, pool, linear_Q."""

    def __init__(self):
        super().__init__()
        C = conv2d_Q(8, 0.1, 0.2)
        bn, relu = torch.nn.BatchNorm2d, torch.nn.ReLU
        self.stem = torch.nn.Sequential(C(3, 16, 3, stride=1, padding=1), bn(16), relu())
        self.body = torch.nn.Sequential(C(16, 16, 1), bn(16), relu(), C(16, 16, 3, stride=2, padding=1), bn(16), relu(),
                                        C(16, 64, 1), bn(64))
        self.down = torch.nn.Sequential(C(16, 64, 1, stride=2), bn(64))
        self.head = torch.nn.Sequential(torch.nn.AdaptiveAvgPool2d(1), torch.nn.Flatten(), linear_Q(8, 0.05, 0.3)(64, 10))

    def forward(self, x):
        x = self.stem(x)
        return self.head(torch.relu(self.body(x) + self.down(x)))


def test_finetune_bottleneck_every_step_matches_composite():
    """Three NormalSGD steps on "hip_all".  At every step the composite runs on the same weights first: the losses are
    bit-identical (one forward path) and every parameter's gradient agrees with the composite's within the bars of
    test_finetune_mobilenetv1_cifar_every_step_matches_composite."""
    torch.manual_seed(0)
    m = _Block().to(DEV).to(memory_format=torch.channels_last)
    x = torch.randn(16, 3, 32, 32).to(DEV).contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 10, (16,)).to(DEV)
    loss_fn = torch.nn.CrossEntropyLoss()
    names = [n for n, _ in m.named_parameters()]
    opt = O.NormalSGD(m.parameters(), lr=1e-3, momentum=0.9)
    running = [b.clone() for b in m.buffers()]
    losses = []
    for step in range(3):
        grads, loss = {}, {}
        for mode in ("composite", "hip_all"):
            cf.options.backward = mode
            for b, r in zip(m.buffers(), running):   # both passes see the same BatchNorm state
                b.copy_(r)
            opt.zero_grad(set_to_none=True)
            out = loss_fn(m(x), y)
            out.backward()
            grads[mode] = [p.grad.detach().clone() for p in m.parameters()]
            loss[mode] = out.item()
            kinds = [mod._last_bwd_kernel for mod in m.modules() if hasattr(mod, "_last_bwd_kernel")]
            assert len(kinds) == 6
            if mode == "hip_all":
                assert all(k != "composite" for k in kinds), kinds
                assert sorted(set(kinds)) == [DENSE, "pw_bwd_mfma_f32"], kinds
                assert kinds.count(DENSE) == 3, kinds    # stem, 3x3 stride 2, 1x1 stride 2
            else:
                assert all(k == "composite" for k in kinds), kinds
        running = [b.clone() for b in m.buffers()]
        assert loss["hip_all"] == loss["composite"], (step, loss)
        for n, a, b in zip(names, grads["hip_all"], grads["composite"]):
            atol = (1e-3 if a.dim() == 1 else 1e-5) * b.abs().max().item()   # BN and bias grads compound over the layers
            torch.testing.assert_close(a, b, rtol=1e-4, atol=atol, msg=lambda s, n=n, step=step: f"step {step}, {n}: {s}")
        opt.step()   # with the HIP backward's gradients
        losses.append(loss["hip_all"])
    print("losses", losses)
    assert all(np.isfinite(losses))


# ---- 9. every instantiation, on both encodes ------------------------------------------------------------------------------
# The smallest shape that selects each (TM, TN) of the gw kernels and each TN of the gx kernels with float4 loads, and the scalar
# loads once per family (pw_shape / dense_shape in csrc/conv_bwd.hip): 128 channels or rows pick the 128-wide tile, 6 -> 10 the
# scalar loads.  INSTANCES says what slfp_debug_bwd_instance must report for each (n = 2, NHWC, the threshold table; split numbers
# stripped); the instances these shapes leave out (k_gemm_f32's gx at tm1tn2, its scalar forms beyond tm1tn1, the code operands)
# have their rows in tests/_bwd_variants.py.
INSTANTIATIONS = (
    [("hip", _spec(ci, co, 1, 1, 0, 8)) for ci, co in ((64, 64), (128, 64), (64, 128), (128, 128))]   # M = 128: tm_x = 2
    + [("hip", _spec(64, 64, 1, 1, 0, 4)),                                                            # M = 32: tm_x = 1
       ("hip", _spec(6, 10, 1, 1, 0, 8))]
    + [("hip_all", _spec(ci, co, 3, 1, 1, 6, 5)) for ci, co in ((8, 8), (16, 16), (8, 128), (16, 128), (128, 8), (6, 10))])


INSTANCES = (
    [f"pw/gx/tm2tn{tn}/v4+pw/gw/tm{tm}tn{tn}/v4/tab/act8" for tm, tn in ((1, 1), (1, 2), (2, 1), (2, 2))]
    + ["pw/gx/tm1tn1/v4+pw/gw/tm1tn1/v4/tab/act8", "pw/gx/tm2tn1/v1+pw/gw/tm1tn1/v1/tab/act8"]
    + [f"dense/gx/tn1/v4+dense/gw/tm{tm}tn{tn}/v4/tab/act8" for tm, tn in ((1, 1), (1, 2), (2, 1), (2, 2))]
    + ["dense/gx/tn2/v4+dense/gw/tm1tn2/v4/tab/act8", "dense/gx/tn1/v1+dense/gw/tm1tn1/v1/tab/act8"])


def test_instantiations_select_what_they_claim():
    """INSTANTIATIONS reaches the instances INSTANCES names, by the reporter that prints from the launch's own selection: a threshold
    moved in pw_shape or dense_shape fails here instead of leaving an instance unrun."""
    import ctypes
    import re
    L = _lib.load()
    os.environ.pop("SLFP_LONG_ENCODE", None)
    L.slfp_debug_reload_switches()
    got = []
    for mode, s in INSTANTIATIONS:
        d = _lib.ConvDesc(n=2, c_in=s.c_in, h=s.h, w=s.w, c_out=s.c_out, kh=s.k[0], kw=s.k[1], stride_h=s.stride[0], stride_w=s.stride[1],
                          pad_h=s.pad[0], pad_w=s.pad[1], dil_h=1, dil_w=1, groups=1, x_layout=_lib.LAYOUT_NHWC, y_layout=_lib.LAYOUT_NHWC,
                          qbits=8, ka=cf._f32(s.Ka), kw_scale=cf._f32(s.Kw), mfma_passes=0, reserved=0)
        said = L.slfp_debug_bwd_instance(ctypes.byref(d), _lib.BWD_DENSE if mode == "hip_all" else 0, 0, 1, 1).decode()
        got.append(re.sub(r"/p\d+k\d+$", "", said))
    assert got == INSTANCES
    parts = {p for g in got for p in g.split("+")}
    for fam in ("pw", "dense"):   # every float4 (TM, TN) of the gw kernels and the scalar form
        assert {p for p in parts if p.startswith(fam + "/gw/")} == (
            {f"{fam}/gw/tm{tm}tn{tn}/v4/tab/act8" for tm in (1, 2) for tn in (1, 2)} | {f"{fam}/gw/tm1tn1/v1/tab/act8"})
    assert {p for p in parts if p.startswith("dense/gx/")} == {"dense/gx/tn1/v4", "dense/gx/tn2/v4", "dense/gx/tn1/v1"}
    assert {p for p in parts if p.startswith("pw/gx/")} == {"pw/gx/tm2tn1/v4", "pw/gx/tm2tn2/v4", "pw/gx/tm1tn1/v4", "pw/gx/tm2tn1/v1"}


@pytest.mark.parametrize("q", [8, 7])
@pytest.mark.parametrize("mode,spec", INSTANTIATIONS, ids=[f"{m}-{s.c_in}x{s.c_out}k{s.k[0]}@{s.h}x{s.w}" for m, s in INSTANTIATIONS])
def test_every_instantiation_on_the_table_and_the_long_encode(mode, spec, q):
    """Each tile shape of the pointwise and dense families, once on the threshold table and once on the long-form encode
    (SLFP_LONG_ENCODE, which no other backward test reaches): both meet the float64 bars, and since both encodes are
    bit-identical to slfp_quantize_f32 and the sums and their order are the same, gx, gw and gb are equal bit for bit."""
    L = _lib.load()
    kernels = (DENSE,) if mode == "hip_all" else ("pw_bwd_mfma_f32",)
    runs = []
    try:
        for long_form in (False, True):
            os.environ.pop("SLFP_LONG_ENCODE", None)
            if long_form:
                os.environ["SLFP_LONG_ENCODE"] = "1"
            L.slfp_debug_reload_switches()
            gen = torch.Generator().manual_seed(9000 + spec.c_in * 131 + spec.c_out + q)
            runs.append(_bwd_cases._check_case(spec, 2, q, True, gen, True, mode, kernels, composite=False,
                                               label="long form" if long_form else "table"))
    finally:
        os.environ.pop("SLFP_LONG_ENCODE", None)
        L.slfp_debug_reload_switches()
    for name, a, b in zip(("gx", "gw", "gb"), *runs):
        assert torch.equal(a, b), name
