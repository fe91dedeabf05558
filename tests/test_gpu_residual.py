"""GPU (MI355X): the residual operand of the pointwise kernels (include/slfp.h slfp_conv2d_fwd_res), from the C ABI up to
fusion.fuse_residual.

What every residual block of the reference ends in (nets_imgnet/resnet50.py:82-88):
    out = relu(bn3(conv3(h)) + identity)
The contract: slfp_conv2d_fwd_res returns, BIT FOR BIT, what slfp_conv2d_fwd_post(relu = 0) followed by torch.add and
torch.relu returns (the conv result's roundings, then the affine's fma, then ONE float32 add, then the max).  The unfused
kernels themselves are pinned to the oracle / the reference's golden vectors in test_gpu_parity.py and test_gpu_codes.py; one
geometry per residual kernel is also compared with the CPU oracle directly here, under the families' existing bars."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.utils._python_dispatch

from oracle import slfp_oracle as so
from _bars import tol
from conftest import rel_errors

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from cnns_slfp_quantization_amd import _lib
    L = _lib.load()  # raises if libslfp_hip.so is missing: no fallback
    assert L.slfp_device_count() >= 1
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Spec:
    """A 1x1 stride-1 layer: c_in -> c_out on hw x hw pixels (hw x w with `w`) with the scales of a ResNet-50 conv3."""

    def __init__(self, c_in, c_out, hw, Ka=0.14, Kw=0.0196, w=None):
        self.c_in, self.c_out, self.h, self.w, self.Ka, self.Kw = c_in, c_out, hw, hw if w is None else w, Ka, Kw


def _conv3_specs():
    """conv3 of the four stages, with the layer table's own scales (the first block of each stage)."""
    from cnns_slfp_quantization_amd import layer_specs
    out = []
    for c_in, hw in ((64, 56), (128, 28), (256, 14), (512, 7)):
        s = next(s for s in layer_specs.conv_layers("resnet50_imagenet224")
                 if s.k == (1, 1) and s.stride == (1, 1) and s.c_in == c_in and s.c_out == 4 * c_in and s.h == hw)
        out.append(_Spec(s.c_in, s.c_out, s.h, s.Ka, s.Kw))
    return out


class _Layer:
    """One pointwise layer with random weights, folded-BN vectors and prepared weights."""

    def __init__(self, lib, s, n, qbits, dev, gen, passes=None, post=True):
        L = lib.load()
        self.lib, self.s, self.n, self.qbits = lib, s, n, qbits
        self.d = lib.ConvDesc(n=n, c_in=s.c_in, h=s.h, w=s.w, c_out=s.c_out, kh=1, kw=1, stride_h=1, stride_w=1, pad_h=0, pad_w=0,
                              dil_h=1, dil_w=1, groups=1, x_layout=lib.LAYOUT_NHWC, y_layout=lib.LAYOUT_NHWC, qbits=qbits,
                              ka=float(np.float32(s.Ka)), kw_scale=float(np.float32(s.Kw)),
                              mfma_passes=lib.MFMA_F16X1 if passes is None else passes, reserved=0)
        self.w = torch.randn((s.c_out, s.c_in, 1, 1), generator=gen, device=dev)
        self.w.mul_(min(5.0 * s.Kw, 3.0 * (2.0 / s.c_in) ** 0.5 + 2.0 * s.Kw))
        self.blob = torch.empty(L.slfp_conv2d_wprep_bytes(ctypes.byref(self.d)), dtype=torch.uint8, device=dev)
        lib.check(L.slfp_conv2d_prepare_weights(ctypes.byref(self.d), self.w.data_ptr(), self.blob.data_ptr(), None, _stream()))
        self.scale = (torch.rand(s.c_out, generator=gen, device=dev) + 0.5) if post else None
        self.shift = (torch.randn(s.c_out, generator=gen, device=dev) * 0.3) if post else None
        self.kernel = L.slfp_conv2d_kernel_name(ctypes.byref(self.d)).decode()

    def out_shape(self):
        return (self.n, self.s.h, self.s.w, self.s.c_out)

    def _post(self):
        return (self.scale.data_ptr() if self.scale is not None else None, self.shift.data_ptr() if self.shift is not None else None)

    def io(self, x_codes):
        return self.lib.ConvIo(x_codes=1 if x_codes else 0, y_codes=0, y_ka=1.0, y_qbits=8)

    def supported(self, x_codes, relu=1):
        return self.lib.load().slfp_conv2d_res_supported(ctypes.byref(self.d), ctypes.byref(self.io(x_codes)), 0, relu)

    def fwd_unfused(self, x, x_codes):
        """the parent's path, epilogue ReLU off: slfp_conv2d_fwd_post / slfp_conv2d_fwd_codes"""
        lib, L = self.lib, self.lib.load()
        y = torch.empty(self.out_shape(), device=x.device)
        ps, psh = self._post()
        if x_codes:
            lib.check(L.slfp_conv2d_fwd_codes(ctypes.byref(self.d), ctypes.byref(self.io(True)), x.data_ptr(), self.blob.data_ptr(), None,
                                              ps, psh, 0, y.data_ptr(), _stream()))
        else:
            lib.check(L.slfp_conv2d_fwd_post(ctypes.byref(self.d), x.data_ptr(), self.blob.data_ptr(), None, ps, psh, 0, y.data_ptr(),
                                             None, None, _stream()))
        return y

    def fwd_res(self, x, x_codes, res, relu, y=None):
        lib, L = self.lib, self.lib.load()
        y = torch.empty(self.out_shape(), device=x.device) if y is None else y
        ps, psh = self._post()
        lib.check(L.slfp_conv2d_fwd_res(ctypes.byref(self.d), ctypes.byref(self.io(x_codes)), x.data_ptr(), self.blob.data_ptr(), None,
                                        ps, psh, 1 if relu else 0, res.data_ptr(), y.data_ptr(), None, _stream()))
        return y


def _input(lib, s, n, dev, gen, x_codes, qbits):
    """post-ReLU-like activations spanning all binades and both clamps, with exact zeros; as float32 or as the layer's codes"""
    x = torch.relu(torch.randn((n, s.h, s.w, s.c_in), generator=gen, device=dev)) * (6.0 * s.Ka)
    x.view(-1)[::97] = 17.0 * s.Ka          # beyond the clamp
    x.view(-1)[5::193] = 0.05 * s.Ka        # the "tiny" class
    if not x_codes:
        return x, x
    c = torch.empty(x.shape, dtype=torch.uint8, device=dev)
    fmt = lib.FMT_ACT8 if qbits == 8 else lib.FMT_SFP7
    lib.check(lib.load().slfp_encode_f32(x.data_ptr(), c.data_ptr(), x.numel(), float(np.float32(s.Ka)), fmt | lib.FMT_EXT, _stream()))
    return c, x


def _residual(y0, gen):
    """Seeded, signed, NaN-free, several binades wide (2^-3 .. 2^2 times the conv output's spread); a tenth of the elements
    large and negative, so that the ReLU clamps a visible share of the sums."""
    sigma = float(y0.std())
    e = torch.randint(-3, 3, y0.shape, generator=gen, device=y0.device).float()
    r = sigma * (0.7 + torch.randn(y0.shape, generator=gen, device=y0.device)) * torch.exp2(e)
    big = torch.rand(y0.shape, generator=gen, device=y0.device) < 0.1
    r = torch.where(big, -8.0 * sigma * (1.0 + torch.rand(y0.shape, generator=gen, device=y0.device)), r)
    assert bool(torch.isfinite(r).all()) and float(r.min()) < 0 < float(r.max())
    return r.contiguous()


def _check_equal(lay, x, x_codes, gen, relus=(0, 1)):
    """torch.equal(fwd_res(...), relu?(fwd_post(relu = 0) + res)) and the share of sums the ReLU clamps"""
    y0 = lay.fwd_unfused(x, x_codes)
    assert bool(torch.isfinite(y0).all()) and float(y0.abs().max()) > 0
    res = _residual(y0, gen)
    for relu in relus:
        want = torch.add(y0, res)
        if relu:
            share = float((want < 0).float().mean())
            print(f"{lay.kernel} {lay.s.c_in}->{lay.s.c_out}@{lay.s.h} n={lay.n} codes_in={int(x_codes)} q{lay.qbits}: ReLU clamps {share:.3f}")
            assert 0.05 <= share <= 0.60, share
            want = torch.relu(want)
        got = lay.fwd_res(x, x_codes, res, relu)
        assert torch.equal(got, want), (lay.kernel, lay.s.c_in, lay.s.c_out, lay.s.h, x_codes, relu,
                                        float((got - want).abs().max()), int((got != want).sum()))
    return y0, res


# ------------------------------------------------------------------ 1. the C ABI against the unfused sequence
@pytest.mark.parametrize("qbits", [8, 7])
@pytest.mark.parametrize("x_codes", [False, True])
@pytest.mark.parametrize("geom", [0, 1, 2, 3])
def test_fused_launch_equals_the_unfused_sequence_bit_for_bit(lib, dev, geom, x_codes, qbits):
    s = _conv3_specs()[geom]
    gen = torch.Generator(device=dev).manual_seed(100 + 10 * geom + qbits + int(x_codes))
    lay = _Layer(lib, s, 4, qbits, dev, gen)
    assert lay.supported(x_codes) == 1
    x, _ = _input(lib, s, 4, dev, gen, x_codes, qbits)
    _check_equal(lay, x, x_codes, gen)


@pytest.mark.parametrize("geom", [0, 1, 2, 3])
def test_float32_equivalent_mode_with_float32_input(lib, dev, geom):
    s = _conv3_specs()[geom]
    gen = torch.Generator(device=dev).manual_seed(200 + geom)
    lay = _Layer(lib, s, 4, 8, dev, gen, passes=lib.MFMA_F16X3)
    assert lay.kernel == "pw_mfma_f16x3" and lay.supported(False) == 1 and lay.supported(True) == 0
    x, _ = _input(lib, s, 4, dev, gen, False, 8)
    _check_equal(lay, x, False, gen)


def test_widths_that_are_not_a_multiple_of_16(lib, dev):
    """C_out % 4 == 0 is what the library asks for: where it accepts a C_out that is not a multiple of 16 (ask it), the
    partial channel tile must come out right as well -- on both float32-input kernels and the code-input ones."""
    gen = torch.Generator(device=dev).manual_seed(300)
    ran = 0
    for c_in, c_out, hw in ((64, 40, 14), (128, 200, 14), (256, 1000, 7), (512, 2040, 7)):
        s = _Spec(c_in, c_out, hw)
        for x_codes in (False, True):
            lay = _Layer(lib, s, 3, 8, dev, gen)
            if lay.supported(x_codes) != 1:
                continue
            x, _ = _input(lib, s, 3, dev, gen, x_codes, 8)
            _check_equal(lay, x, x_codes, gen)
            ran += 1
    assert ran >= 1, "slfp_conv2d_res_supported accepts no width with C_out % 16 != 0"


@pytest.mark.parametrize("form", ["float32 in", "codes in", "f16x3"])
@pytest.mark.parametrize("width", [(64, 256), (256, 1024)])
def test_non_square_images(lib, dev, width, form):
    """6 x 15 and 15 x 6 pixels (every other residual case is square), n = 3: 270 rows, not a multiple of any row tile; the
    stream kernel (64 -> 256) and the tiled one (256 -> 1024), each with float32 input, code input and in the f16x3 mode."""
    gen = torch.Generator(device=dev).manual_seed(400 + width[0] + len(form))
    x_codes = form == "codes in"
    for h, w in ((6, 15), (15, 6)):
        s = _Spec(width[0], width[1], h, w=w)
        lay = _Layer(lib, s, 3, 8, dev, gen, passes=lib.MFMA_F16X3 if form == "f16x3" else None)
        assert lay.kernel == ("pw_mfma_f16x3" if form == "f16x3" else "pw_mfma_f16x1") and lay.supported(x_codes) == 1
        assert lay.out_shape() == (3, h, w, width[1])
        x, _ = _input(lib, s, 3, dev, gen, x_codes, 8)
        _check_equal(lay, x, x_codes, gen)


# ------------------------------------------------------------------ 2. at the size BASELINE config 4 runs
@pytest.mark.parametrize("x_codes", [False, True])
@pytest.mark.parametrize("geom", [0, 1, 2, 3])
def test_full_batch_fused_launch_equals_the_unfused_sequence(lib, dev, geom, x_codes):
    """Batch 128: the grids are persistent / remapped by workgroup count, so the size matters."""
    s = _conv3_specs()[geom]
    gen = torch.Generator(device=dev).manual_seed(400 + 10 * geom + int(x_codes))
    lay = _Layer(lib, s, 128, 8, dev, gen)
    x, _ = _input(lib, s, 128, dev, gen, x_codes, 8)
    _check_equal(lay, x, x_codes, gen, relus=(1,))


# ------------------------------------------------------------------ 3. one geometry per kernel against the CPU oracle
# (kernel the geometry reaches, c_in, c_out, hw, codes in)
ORACLE_CASES = [("k_pw_stream", 32, 64, 14, False), ("k_pw_tiled", 128, 512, 7, False), ("k_pwc_stream", 64, 256, 14, True),
                ("k_pwc_slice", 256, 1024, 7, True), ("k_pwc_tiled", 512, 2048, 7, True)]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=[c[0] for c in ORACLE_CASES])
def test_residual_kernels_against_the_cpu_oracle(lib, dev, case):
    """relu(affine(oracle.conv2d(x)) + res) in double against the fused launch, under the family's existing bar."""
    _, c_in, c_out, hw, x_codes = case
    s = _Spec(c_in, c_out, hw)
    gen = torch.Generator(device=dev).manual_seed(500 + c_in)
    lay = _Layer(lib, s, 2, 8, dev, gen)
    assert lay.supported(x_codes) == 1
    x, xf = _input(lib, s, 2, dev, gen, x_codes, 8)
    res = _residual(lay.fwd_unfused(x, x_codes), gen)
    y = lay.fwd_res(x, x_codes, res, 1).cpu().numpy().transpose(0, 3, 1, 2)
    ref = so.conv2d(np.ascontiguousarray(xf.cpu().numpy().transpose(0, 3, 1, 2)), lay.w.cpu().numpy(), None, (1, 1), (0, 0), (1, 1), 1,
                    np.float64(s.Ka), np.float64(s.Kw), 8).astype(np.float64)
    ref = ref * lay.scale.cpu().numpy().astype(np.float64)[None, :, None, None] + lay.shift.cpu().numpy().astype(np.float64)[None, :, None, None]
    ref = np.maximum(ref + res.cpu().numpy().transpose(0, 3, 1, 2).astype(np.float64), 0.0)
    emax, el2 = rel_errors(y, ref)
    print(f"{case[0]}: {lay.kernel} max {emax:.3e} l2 {el2:.3e} (bar {tol(lay.kernel):.0e})")
    assert emax <= tol(lay.kernel) and el2 <= tol(lay.kernel), (case, emax, el2)


# ------------------------------------------------------------------ 4. determinism, and nothing written past M rows / N channels
GUARD_CASES = [(32, 40, 7, False), (128, 200, 7, False), (64, 40, 7, True), (256, 1024, 7, True), (256, 1000, 7, True)]


@pytest.mark.parametrize("case", GUARD_CASES, ids=["%d-%d-%s" % (c[0], c[1], "codes" if c[3] else "f32") for c in GUARD_CASES])
def test_two_launches_give_the_same_bits_and_the_guard_bands_stay_untouched(lib, dev, case):
    """3 images of 7 x 7 = 147 pixel rows (not a multiple of any pixel tile), widths that end inside a channel tile: y sits
    inside a poisoned buffer whose guard bands in front of and behind it must survive the launch."""
    c_in, c_out, hw, x_codes = case
    s = _Spec(c_in, c_out, hw)
    gen = torch.Generator(device=dev).manual_seed(600 + c_in + c_out)
    lay = _Layer(lib, s, 3, 8, dev, gen)
    if lay.supported(x_codes) != 1:
        pytest.fail(f"slfp_conv2d_res_supported refuses {case}")
    x, _ = _input(lib, s, 3, dev, gen, x_codes, 8)
    y0, res = _check_equal(lay, x, x_codes, gen, relus=(1,))
    want = torch.relu(y0 + res)
    n_el, guard = want.numel(), 64 * 2048   # elements: more than any tile's rows x channels past the end
    poison = 0x7FC0DEAD   # a NaN pattern no kernel produces
    outs = []
    for _ in range(2):
        buf = torch.full((guard + n_el + guard,), poison, dtype=torch.int32, device=dev)
        y = buf[guard:guard + n_el].view(torch.float32).view(want.shape)
        assert y.data_ptr() % 16 == 0
        lay.fwd_res(x, x_codes, res, 1, y=y)
        assert bool((buf[:guard] == poison).all()) and bool((buf[guard + n_el:] == poison).all()), case
        assert torch.equal(y, want)
        outs.append(buf[guard:guard + n_el].clone())
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------ 5. the ResNet-50 fixture net
def _build_resnet50(dev):
    """nets_imgnet/resnet50.py:24-147 out of the drop-in modules (tests/golden/netgen_r3.py: this repo's own definition) with
    the fixture's name-seeded parameters, BatchNorm statistics, weight gains and per-module scales."""
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import netgen_r3 as ng
    import utils.conv2d_func as cf
    import utils.sfp_quant as sq
    gold = np.load(os.path.join(GOLDEN, "nets_r3_golden.npz"))
    q, batch, in_seed, seed = [int(v) for v in gold["resnet50:meta"]]
    manifest = json.loads(bytes(gold["resnet50:manifest"]).decode())
    gains = json.loads(bytes(gold["resnet50:gains"]).decode())
    m = ng.BUILDERS["resnet50"](ng.Factories(cf, q, manifest, layerout=sq.layerout_quantize_func))
    ng.fill_parameters_by_name(m, seed, gains)
    ng.load_bn_stats_by_name_(m, {k[len("resnet50") + 1:]: gold[k] for k in gold.files if k.startswith("resnet50:bn:")})
    m = m.to(dev).eval().to(memory_format=torch.channels_last)
    x = ng.net_input224(batch, in_seed).to(dev).contiguous(memory_format=torch.channels_last)
    return m, x


class _OpCount(torch.utils._python_dispatch.TorchDispatchMode):
    """Every ATen op a forward dispatches, by name."""

    def __init__(self):
        super().__init__()
        self.names = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.names.append(str(func))
        return func(*args, **(kwargs or {}))

    def count(self, what):
        return sum(1 for n in self.names if n.startswith("aten." + what + ".") or n.startswith("aten." + what + "_."))


def _blocks(m):
    return [b for b in m.modules() if type(b).__name__ == "_Bottleneck"]


def _fold(m, x):
    from cnns_slfp_quantization_amd import fusion
    assert fusion.fuse_bn_relu(m) == 4            # the four downsample nn.Sequential(conv, bn)
    assert fusion.fuse_named_bn(m, example_input=x) == 49


def test_resnet50_fuse_residual_is_bit_identical_and_composes(dev):
    from cnns_slfp_quantization_amd import fusion, graph
    m, x = _build_resnet50(dev)
    blocks = _blocks(m)
    assert len(blocks) == 16
    with torch.no_grad():
        y_stock = m(x)
        _fold(m, x)
        with _OpCount() as ops0:
            y_fused = m(x)
        assert ops0.count("add") == 16 and ops0.count("relu") == 1 + 3 * 16, (ops0.count("add"), ops0.count("relu"))
        assert fusion.fuse_residual(m, x) == 16
        with _OpCount() as ops1:
            y_res = m(x)
        assert torch.equal(y_res.view(torch.int32), y_fused.view(torch.int32))
        # the three launches per block are one: no add left, the block's relu module runs after conv1 and conv2 only
        assert ops1.count("add") == 0 and ops1.count("relu") == 1 + 2 * 16, (ops1.count("add"), ops1.count("relu"))
        for b in blocks:
            assert b.conv3._last_kernel.endswith("+res") and b.conv3._last_kernel.startswith("pw_mfma"), b.conv3._last_kernel
            assert bool((b.conv3.output >= 0).all())   # self.output is the tensor after the add and the ReLU
        # code hand-overs on top
        assert fusion.link_codes_traced(m, x) == 16
        y_link = m(x)
        assert torch.equal(y_link.view(torch.int32), y_fused.view(torch.int32))
        for b in blocks:
            assert b.conv3._last_kernel.endswith("+codes_in+res"), b.conv3._last_kernel
        # the same through one hipGraph
        g = graph.GraphedModule(m)
        assert torch.equal(g(x).view(torch.int32), y_fused.view(torch.int32))
        assert torch.equal(g(x).view(torch.int32), y_fused.view(torch.int32))   # replay
        # and back
        assert fusion.unfuse_residual(m) == 16 and fusion.unlink_codes(m) == 16
        y_back = m(x)
        assert torch.equal(y_back.view(torch.int32), y_fused.view(torch.int32))
        assert not any(b.conv3._last_kernel.endswith("+res") for b in blocks)
        assert not any("forward" in b.__dict__ for b in blocks) and not any(b.conv3.residual_relu for b in blocks)
        assert fusion.unfuse_named_bn(m) == 49
    assert y_stock.shape == y_fused.shape


def test_resnet50_link_first_then_fuse_residual_gives_the_same(dev):
    from cnns_slfp_quantization_amd import fusion, graph
    m, x = _build_resnet50(dev)
    blocks = _blocks(m)
    with torch.no_grad():
        _fold(m, x)
        y_fused = m(x)
        assert fusion.link_codes_traced(m, x) == 16
        assert fusion.fuse_residual(m, x) == 16
        y = m(x)
        assert torch.equal(y.view(torch.int32), y_fused.view(torch.int32))
        assert all(b.conv3._last_kernel.endswith("+codes_in+res") for b in blocks), [b.conv3._last_kernel for b in blocks]
        assert torch.equal(graph.GraphedModule(m)(x).view(torch.int32), y_fused.view(torch.int32))
        # undo in the other order as well
        assert fusion.unlink_codes(m) == 16
        y = m(x)
        assert torch.equal(y.view(torch.int32), y_fused.view(torch.int32))
        assert all(b.conv3._last_kernel.endswith("+res") and "codes" not in b.conv3._last_kernel for b in blocks)
        assert fusion.unfuse_residual(m) == 16
        assert torch.equal(m(x).view(torch.int32), y_fused.view(torch.int32))


# ------------------------------------------------------------------ 6. a name is only a convention: roll-back
def _named_block(kind, dev):
    import utils.conv2d_func as cf

    class Blk(torch.nn.Module):
        """The Bottleneck's child names; `kind` selects what forward() really does."""

        def __init__(self):
            super().__init__()
            C = cf.conv2d_Q(q_bit=8, Kw=0.02, Ka=0.3)
            self.conv1 = C(64, 32, 1, 0.02, 0.3)
            self.bn1 = torch.nn.Identity()
            self.conv2 = C(32, 32, 3, 0.02, 0.3, 1, 1)
            self.bn2 = torch.nn.Identity()
            self.conv3 = C(32, 64, 1, 0.02, 0.3)
            self.bn3 = torch.nn.Identity()
            self.relu = torch.nn.ReLU()
            self.downsample = None

        def forward(self, x):
            h = self.relu(self.bn1(self.conv1(x)))
            h = self.relu(self.bn2(self.conv2(h)))
            out = self.bn3(self.conv3(h))
            if kind == "scaled":
                return self.relu(out + 2.0 * x)
            if kind == "cat":
                return torch.cat([self.relu(out + x), h], 1)
            return self.relu(out + x)

    torch.manual_seed(7)
    m = Blk().to(dev).eval().to(memory_format=torch.channels_last)
    with torch.no_grad():
        for c in (m.conv1, m.conv2, m.conv3):
            c.weight.mul_(0.5)
    return m


@pytest.mark.parametrize("kind,want", [("scaled", 0), ("cat", 0), ("plain", 1)])
def test_blocks_that_only_look_like_a_bottleneck_are_left_alone(dev, kind, want):
    from cnns_slfp_quantization_amd import fusion
    m = _named_block(kind, dev)
    gen = torch.Generator(device=dev).manual_seed(8)
    x = torch.randn(2, 64, 12, 12, generator=gen, device=dev).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        y0 = m(x)
        assert fusion.fuse_residual(m, x) == want
        assert ("forward" in m.__dict__) == bool(want) and m.conv3.residual_relu == bool(want)
        y1 = m(x)
        assert y1.shape == y0.shape and torch.equal(y1, y0)
        assert m.conv3._last_kernel.endswith("+res") == bool(want)
        assert fusion.unfuse_residual(m) == want
        assert torch.equal(m(x), y0)


# ------------------------------------------------------------------ 7. where no residual kernel runs: the same values with ATen
def test_fallbacks_compute_the_same_values_with_aten(dev):
    import utils.conv2d_func as cf
    torch.manual_seed(9)
    gen = torch.Generator(device=dev).manual_seed(9)
    conv = cf.conv2d_Q(q_bit=8, Kw=0.02, Ka=0.3)(64, 128, 1, 0.02, 0.3).to(dev).eval().to(memory_format=torch.channels_last)
    conv.residual_relu = True
    x = torch.randn(2, 64, 14, 14, generator=gen, device=dev).contiguous(memory_format=torch.channels_last)
    r = torch.randn(2, 128, 14, 14, generator=gen, device=dev).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        want = torch.relu(conv(x) + r)
        got = conv(x, residual=r)
        assert conv._last_kernel.endswith("+res") and torch.equal(got, want) and conv.output is got
        # NCHW tensors
        got = conv(x.contiguous(), residual=r.contiguous())
        assert "+res" not in conv._last_kernel and torch.equal(got, want)
        # a residual of another layout / shape the kernel cannot take
        got = conv(x, residual=r.contiguous())
        assert "+res" not in conv._last_kernel and torch.equal(got, want)
    # grad enabled
    xg = x.clone().requires_grad_(True)
    got = conv(xg, residual=r)
    assert "+res" not in conv._last_kernel and got.requires_grad and torch.equal(got.detach(), want)
    # training mode
    conv.train()
    with torch.no_grad():
        got = conv(x, residual=r)
    assert "+res" not in conv._last_kernel and torch.equal(got, want)
    conv.eval()
    # without the ReLU
    conv.residual_relu = False
    with torch.no_grad():
        got = conv(x, residual=r)
        assert conv._last_kernel.endswith("+res") and torch.equal(got, conv(x) + r)
    # q_bit 32: the reference's passthrough, stock ATen
    c32 = cf.conv2d_Q(q_bit=32, Kw=0.02, Ka=0.3)(64, 128, 1, 0.02, 0.3).to(dev).eval()
    c32.residual_relu = True
    with torch.no_grad():
        got = c32(x, residual=r)
        assert "+res" not in (c32._last_kernel or "") and torch.equal(got, torch.relu(c32(x) + r))
