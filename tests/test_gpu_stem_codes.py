"""MI355X: the large-kernel image stems with code output -- the YC forms of k_stem_rows and k_stem_mfma read the
float32 image and write the 1-byte codes of the layer behind the stem (slfp_conv2d_fwd_codes[_ws] with x_codes = 0, y_codes = 1):
bit identity with slfp_encode_f32 of the float32 interface's output through the C ABI on both forms, the float32 leg against the CPU
oracle, the chain stem -> ceil-mode pool on codes -> 1x1 on codes, the module, and fusion.link_stem on the SqueezeNet and ResNet-50
fixture nets and an AlexNet head.  Every comparison of codes is torch.equal.

Which form runs: the float32 interface sizes its workspace for the two-kernel form on every stem_mfma descriptor (the SLFP_STEM_IM2ROW
switch can send any of them there; tests/test_aniso_host.py pins that), so slfp_conv2d_workspace_bytes cannot tell the forms apart.
What can: slfp_conv2d_fwd_codes takes no workspace -- it runs the rows form and answers the two-kernel form with the missing-workspace
status before anything is launched.  The rows-form cases are run through it, the two-kernel cases assert that status."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import slfp_oracle as so
from conftest import rel_errors, elem_exceed_frac
from _bars import tol, elem_frac_bar, ELEM_MIN

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
GUARD = 64


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


@pytest.fixture(scope="module")
def arena(dev):
    """A device allocation of its own (32 MiB: a whole number of 2 MiB pages that the caching allocator hands to the device as it
    is, once its free blocks are released): code tensors are placed at its very end, so nothing lies behind their last byte."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return torch.empty(32 << 20, dtype=torch.uint8, device=dev)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _fmt(lib, qbits):
    return lib.FMT_ACT8 if qbits == 8 else lib.FMT_SFP7


def _encode(lib, x, ka, qbits):
    c = torch.empty_like(x, dtype=torch.uint8)
    lib.check(lib.load().slfp_encode_f32(x.data_ptr(), c.data_ptr(), x.numel(), float(np.float32(ka)), _fmt(lib, qbits) | lib.FMT_EXT, _stream()))
    return c


def _p(t):
    return t.data_ptr() if t is not None else None


def _i32(t):
    return t.view(torch.int32)


class _Layer:
    """One Conv2d_Q layer on NHWC tensors (logical n x c_in x h x w) with weights, bias and a BN-like affine drawn on the CPU."""

    def __init__(self, lib, dev, gen, n, c_in, c_out, h, w, qbits, k, stride, pad, bias, ka=0.31, kw=0.02):
        L = lib.load()
        self.lib, self.n, self.c_in, self.c_out, self.h, self.wd, self.qbits, self.ka, self.kw = lib, n, c_in, c_out, h, w, qbits, ka, kw
        self.k, self.stride, self.pad = k, stride, pad
        self.d = lib.ConvDesc(n=n, c_in=c_in, h=h, w=w, c_out=c_out, kh=k, kw=k, stride_h=stride, stride_w=stride, pad_h=pad, pad_w=pad,
                              dil_h=1, dil_w=1, groups=1, x_layout=lib.LAYOUT_NHWC, y_layout=lib.LAYOUT_NHWC, qbits=qbits,
                              ka=float(np.float32(ka)), kw_scale=float(np.float32(kw)), mfma_passes=lib.MFMA_F16X1, reserved=0)
        ho, wo = ctypes.c_int64(), ctypes.c_int64()
        lib.check(L.slfp_conv2d_out_shape(ctypes.byref(self.d), ctypes.byref(ho), ctypes.byref(wo)))
        self.ho, self.wo = ho.value, wo.value
        fan = c_in * k * k
        self.w_cpu = torch.randn((c_out, c_in, k, k), generator=gen) * min(5.0 * kw, 3.0 * (2.0 / fan) ** 0.5 + 2.0 * kw)
        self.b_cpu = torch.randn(c_out, generator=gen) * 0.2 if bias else None
        self.w = self.w_cpu.to(dev)
        self.b = self.b_cpu.to(dev) if bias else None
        self.ps = (0.5 + torch.rand(c_out, generator=gen)).to(dev)
        self.psh = (torch.randn(c_out, generator=gen) * 0.1).to(dev)
        self.blob = torch.empty(L.slfp_conv2d_wprep_bytes(ctypes.byref(self.d)), dtype=torch.uint8, device=dev)
        lib.check(L.slfp_conv2d_prepare_weights(ctypes.byref(self.d), self.w.data_ptr(), self.blob.data_ptr(), None, _stream()))
        self.ws_bytes = L.slfp_conv2d_workspace_bytes(ctypes.byref(self.d))
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev) if self.ws_bytes else None
        self.kernel = L.slfp_conv2d_kernel_name(ctypes.byref(self.d)).decode()

    def out_shape(self):
        return (self.n, self.ho, self.wo, self.c_out)

    def _args(self, x, relu, post):
        return (x.data_ptr(), self.blob.data_ptr(), _p(self.b), _p(self.ps) if post else None, _p(self.psh) if post else None,
                1 if relu else 0)

    def fwd_f32(self, x, relu, post):
        y = torch.empty(self.out_shape(), device=x.device)
        self.lib.check(self.lib.load().slfp_conv2d_fwd_post(ctypes.byref(self.d), *self._args(x, relu, post), y.data_ptr(), None,
                                                            _p(self.ws), _stream()))
        return y

    def io(self, y_ka, y_qbits, x_codes=0, y_codes=1):
        return self.lib.ConvIo(x_codes=x_codes, y_codes=y_codes, y_ka=float(np.float32(y_ka)), y_qbits=y_qbits)

    def codes_ok(self, io, relu):
        return self.lib.load().slfp_conv2d_codes_supported(ctypes.byref(self.d), ctypes.byref(io), 1 if self.b is not None else 0,
                                                           1 if relu else 0) == 1

    def fwd_codes_status(self, x, relu, post, io, y_ptr):
        """slfp_conv2d_fwd_codes (no workspace): the status"""
        return self.lib.load().slfp_conv2d_fwd_codes(ctypes.byref(self.d), ctypes.byref(io), *self._args(x, relu, post), y_ptr, _stream())

    def fwd_codes_ws(self, x, relu, post, io, y_ptr):
        self.lib.check(self.lib.load().slfp_conv2d_fwd_codes_ws(ctypes.byref(self.d), ctypes.byref(io), *self._args(x, relu, post), y_ptr,
                                                                _p(self.ws), _stream()))


def _image(lay, dev, gen, special=False, graded=True):
    """An image batch of both signs; graded: the right half of the last image is 2^-10 of the rest (outputs down to the tiny class)
    and holds a block of exact zeros; special: a NaN, +inf, -inf and -0.0 pixel among the first pixels of the first image."""
    x = torch.randn((lay.n, lay.h, lay.wd, lay.c_in), generator=gen) * (4.0 * lay.ka)
    if graded:
        x[-1, :, lay.wd // 2:] *= 2.0 ** -10
        x[-1, lay.h // 2:, 3 * lay.wd // 4:] = 0.0
    if special:
        px = x.view(-1, lay.c_in)
        px[1, 0], px[2, 1], px[3, 2 % lay.c_in], px[4, 0] = float("nan"), float("inf"), float("-inf"), -0.0
    return x.to(dev)


def _consumer_scale(lay, want):
    """A consumer Ka for which `want` (the float32 interface's output without a ReLU) reaches the clamp and the top regular class:
    the k-th largest finite value sits at 15.0 Ka (top class of both formats: [14.75, 15.32] Ka and [14.5, inf) Ka); the first k for
    which the library has a code table in both code formats."""
    v = want[torch.isfinite(want)].flatten().sort(descending=True).values
    for k in range(max(2, v.numel() // 100), v.numel()):
        ka = float(np.float32(float(v[k]) / 15.0))
        if ka > 0 and float(v[0]) > 15.4 * ka and all(lay.codes_ok(lay.io(ka, q), True) and lay.codes_ok(lay.io(ka, q), False) for q in (8, 7)):
            return ka
    raise AssertionError("no consumer scale found")


# kernel, stride, pad, C_out, (H, W), N, bias, what it reaches
ROWS_FORM = [
    (7, 2, 3, 64, (37, 45), 2, False, "ragged 8 x 32 tiles both ways"),
    (7, 2, 0, 96, (41, 35), 2, True, "second tile group"),
    (7, 2, 3, 32, (16, 16), 1, False, "one tile, dead tiles"),
    (7, 2, 3, 80, (33, 70), 3, True, "dead tile 5, ragged second column tile"),
]
TWO_KERNEL = [
    (11, 4, 2, 64, (67, 51), 2, True, "Rp = 64"),
    (7, 1, 3, 64, (20, 27), 2, False, "odd S*C, ragged last segment"),
    (11, 4, 2, 96, (43, 43), 1, True, "NT = 6"),
]
ALL = [(r, True) for r in ROWS_FORM] + [(r, False) for r in TWO_KERNEL]


def _row_layer(lib, dev, gen, row, qbits):
    k, s, p, c_out, (h, w), n, bias, _ = row
    return _Layer(lib, dev, gen, n, 3, c_out, h, w, qbits, k, s, p, bias)


@pytest.mark.parametrize("qbits", [8, 7])
@pytest.mark.parametrize("row, rows_form", ALL, ids=["%dx%d-s%d-p%d-%d" % (r[0], r[0], r[1], r[2], r[3]) for r, _ in ALL])
def test_stem_codes_equal_the_encoded_float32_output(lib, dev, arena, row, rows_form, qbits):
    """slfp_conv2d_fwd_codes[_ws] == slfp_encode_f32(slfp_conv2d_fwd_post(...), y_ka, fmt | EXT), byte for byte: consumer formats 8 and
    7, the ReLU folded and signed codes, with and without the affine, a NaN / +inf / -inf / -0.0 pixel in the image; 64 guard bytes of
    0xA5 on each side stay untouched and the codes end at the last byte of their allocation."""
    gen = torch.Generator().manual_seed(4000 + 10 * qbits + row[0] + row[3] + row[4][0])
    lay = _row_layer(lib, dev, gen, row, qbits)
    assert lay.kernel == ("stem_mfma_f16x1" if qbits == 8 else "stem_mfma_f16_exact"), lay.kernel
    x = _image(lay, dev, gen, special=True)
    nbytes = lay.n * lay.ho * lay.wo * lay.c_out
    assert nbytes % 16 == 0
    y_ka = _consumer_scale(lay, lay.fwd_f32(x, False, False))
    end = arena.numel()
    assert lay.ws_bytes > 0   # the float32 interface's (see the module docstring)
    for y_qbits in (8, 7):
        io = lay.io(y_ka, y_qbits)
        for relu in (True, False):
            for post in (False, True):
                assert lay.codes_ok(io, relu)
                f32 = lay.fwd_f32(x, relu, post)
                want = _encode(lib, f32, y_ka, y_qbits).flatten()
                buf = arena[end - nbytes - GUARD:]          # the codes end at the allocation's last byte
                buf.fill_(0xA5)
                at = end - 2 * nbytes - 4 * GUARD
                front = arena[at:at + nbytes + 2 * GUARD]   # guards on both sides
                front.fill_(0xA5)
                assert (buf.data_ptr() + GUARD) % 16 == 0 and (front.data_ptr() + GUARD) % 16 == 0
                if rows_form:   # no workspace: only k_stem_rows can have run
                    lib.check(lay.fwd_codes_status(x, relu, post, io, buf.data_ptr() + GUARD))
                else:
                    assert lay.fwd_codes_status(x, relu, post, io, buf.data_ptr() + GUARD) == lib.ERR_BAD_ARG
                    assert "workspace" in lib.last_error()
                    assert bool((buf == 0xA5).all())
                    lay.fwd_codes_ws(x, relu, post, io, buf.data_ptr() + GUARD)
                lay.fwd_codes_ws(x, relu, post, io, front.data_ptr() + GUARD)
                got = buf[GUARD:]
                ndiff = int((got != want).sum())
                print(f"{row[:6]} qbits {qbits} y_qbits {y_qbits} relu {relu} post {post}: {ndiff} of {nbytes} codes differ")
                assert torch.equal(got, want), (row, qbits, y_qbits, relu, post, ndiff)
                assert bool((buf[:GUARD] == 0xA5).all()), (row, qbits, y_qbits, relu, post)
                assert torch.equal(front[GUARD:GUARD + nbytes], want)
                assert bool((front[:GUARD] == 0xA5).all()) and bool((front[GUARD + nbytes:] == 0xA5).all()), (row, qbits, y_qbits, relu, post)
                if relu and not post:
                    assert bool(torch.isnan(lay.fwd_f32(x, False, False)).any())   # the NaN pixel reaches the output
                    if row is ROWS_FORM[0]:   # the reference codes span the code space: exact zero, tiny, the clamp, the top regular code
                        have = set(torch.unique(want).tolist())
                        top = 0x7F if y_qbits == 8 else 0x3F
                        print(f"{row[:6]} qbits {qbits} y_qbits {y_qbits}: y_ka {y_ka:.6g}, {len(have)} distinct codes")
                        assert {0x01, 0x00, top} <= have, sorted(have)
                        assert y_qbits == 7 or 0x02 in have, sorted(have)
    torch.cuda.synchronize()


@pytest.mark.parametrize("qbits", [8, 7])
@pytest.mark.parametrize("row", [ROWS_FORM[0], TWO_KERNEL[0]], ids=["rows", "two-kernel"])
def test_the_float32_leg_against_the_cpu_oracle(lib, dev, row, qbits):
    """What the code comparison rests on: the float32 output of one row per form against oracle.conv2d (contraction in double) under
    the family's bars (tests/_bars.py).  A plain image: inputs in the tiny class (+-1e-10) are flushed to zero by every fp16-operand
    kernel, which the elementwise bar would count on the graded image of the code tests."""
    gen = torch.Generator().manual_seed(4100 + qbits + row[0])
    lay = _row_layer(lib, dev, gen, row, qbits)
    x = _image(lay, dev, gen, graded=False)
    got = lay.fwd_f32(x, False, False).permute(0, 3, 1, 2).contiguous().cpu().numpy()
    xn = x.cpu().permute(0, 3, 1, 2).contiguous().numpy()
    ref = so.conv2d(xn, lay.w_cpu.numpy(), None if lay.b_cpu is None else lay.b_cpu.numpy(), lay.stride, lay.pad, 1, 1,
                    float(np.float32(lay.ka)), float(np.float32(lay.kw)), qbits)
    emax, el2 = rel_errors(got, ref)
    frac = elem_exceed_frac(got, ref)
    print(f"{lay.kernel} {row[:6]}: max-rel {emax:.3g}, l2 {el2:.3g}, beyond 1e-3 |ref|: {frac:.3g}")
    assert emax <= tol(lay.kernel) and el2 <= tol(lay.kernel), (lay.kernel, emax, el2)
    assert got.size >= ELEM_MIN and frac <= elem_frac_bar(lay.kernel), (lay.kernel, frac)


@pytest.mark.parametrize("qbits", [8, 7])
def test_a_pooled_pointwise_consumer_reads_the_stem_codes(lib, dev, qbits):
    """SqueezeNet's head on the second row's geometry: stem codes -> slfp_maxpool2d_codes_ex(3, 2, ceil) -> 96 -> 16 1x1 on codes equals
    the float32 chain stem -> ReLU -> ATen pool -> 1x1, bit for bit."""
    from cnns_slfp_quantization_amd import sfp_quant
    gen = torch.Generator().manual_seed(4200 + qbits)
    stem = _row_layer(lib, dev, gen, ROWS_FORM[1], qbits)
    x = _image(stem, dev, gen)
    f32 = stem.fwd_f32(x, True, True)
    pooled = F.max_pool2d(f32.permute(0, 3, 1, 2), 3, 2, ceil_mode=True)
    assert pooled.is_contiguous(memory_format=torch.channels_last)
    n, c, hp, wp = pooled.shape
    sq = _Layer(lib, dev, gen, n, 96, 16, hp, wp, qbits, 1, 1, 0, True, ka=0.27)
    want = sq.fwd_f32(pooled.permute(0, 2, 3, 1), True, False)
    assert want.shape == (n, hp, wp, 16)
    io = stem.io(sq.ka, qbits)
    assert stem.codes_ok(io, True)
    codes = torch.empty(stem.out_shape(), dtype=torch.uint8, device=dev)
    lib.check(stem.fwd_codes_status(x, True, True, io, codes.data_ptr()))
    pc = sfp_quant.hip_maxpool_codes(codes.permute(0, 3, 1, 2), 3, 2, 0, qbits, ceil_mode=True)
    assert tuple(pc.shape) == (n, c, hp, wp)
    assert torch.equal(pc, _encode(lib, pooled, sq.ka, qbits))
    io_in = sq.io(1.0, qbits, x_codes=1, y_codes=0)
    assert sq.codes_ok(io_in, True)
    got = torch.empty(sq.out_shape(), device=dev)
    sq.fwd_codes_ws(pc.permute(0, 2, 3, 1), True, False, io_in, got.data_ptr())
    assert torch.equal(_i32(got), _i32(want)), float((got - want).abs().max())


@pytest.mark.parametrize("qbits", [8, 7])
def test_a_geometry_whose_code_table_does_not_fit_falls_to_the_two_kernel_form(lib, dev, qbits):
    """10x10 s1 2->96: halo tile + W take 64704 B of LDS, so the float32 form is k_stem_rows, and the 2056-byte code table no longer
    fits the 64 KiB: the code form asks for the workspace and runs k_stem_im2row + k_stem_mfma.  The two forms compute the same bits,
    so the bytes still equal slfp_encode_f32 of the float32 output."""
    gen = torch.Generator().manual_seed(4300 + qbits)
    lay = _Layer(lib, dev, gen, 1, 2, 96, 20, 23, qbits, 10, 1, 4, True)
    assert lay.kernel.startswith("stem_mfma"), lay.kernel
    x = _image(lay, dev, gen, special=True)
    y_ka = _consumer_scale(lay, lay.fwd_f32(x, False, False))
    for relu in (True, False):
        io = lay.io(y_ka, qbits)
        assert lay.codes_ok(io, relu)
        want = _encode(lib, lay.fwd_f32(x, relu, True), y_ka, qbits)
        got = torch.full(lay.out_shape(), 0xA5, dtype=torch.uint8, device=dev)
        assert lay.fwd_codes_status(x, relu, True, io, got.data_ptr()) == lib.ERR_BAD_ARG and "workspace" in lib.last_error()
        assert bool((got == 0xA5).all())
        lay.fwd_codes_ws(x, relu, True, io, got.data_ptr())
        assert torch.equal(got, want), (qbits, relu, int((got != want).sum()))


# ---------------------------------------------------------------------------------------------- the module
@pytest.mark.parametrize("k, s, p, hw", [(7, 2, 3, (37, 45)), (11, 4, 2, (67, 51))], ids=["rows", "two-kernel"])
@pytest.mark.parametrize("qbits", [8, 7])
def test_module_route(dev, monkeypatch, qbits, k, s, p, hw):
    import utils.conv2d_func as cf
    from cnns_slfp_quantization_amd import sfp_quant
    from cnns_slfp_quantization_amd import conv2d_func as impl
    torch.manual_seed(11)
    m = cf.conv2d_Q_bias(q_bit=qbits, Kw=0.02, Ka=0.3)(3, 64, k, 0.02, 0.3, s, p).to(dev).eval().to(memory_format=torch.channels_last)
    x = (torch.randn(2, 3, *hw, device=dev) * 1.2).contiguous(memory_format=torch.channels_last)
    out = (0.27, qbits)
    with torch.no_grad():
        m.weight.mul_(0.5)
        y = m(x)
        xq = m.input_q.clone()
        assert m._last_kernel.startswith("stem_mfma") and "codes" not in m._last_kernel, m._last_kernel
        want = sfp_quant.hip_encode(y, out[0], impl._act_fmt(qbits))
        m._code_out = out
        got = m(x)
        assert got.dtype == torch.uint8 and torch.equal(got, want), int((got != want).sum())
        assert m._last_kernel.startswith("stem_mfma") and m._last_kernel.endswith("+codes_out") and "codes_in" not in m._last_kernel, m._last_kernel
        assert torch.equal(_i32(m.input_q), _i32(xq))
        # the kernel route disabled: where the query says no, the float32 kernel plus slfp_encode_f32
        monkeypatch.setattr(impl, "_supported", lambda *a, **kw: False)
        m._plans.clear()
        old = m(x)
        assert old.dtype == torch.uint8 and torch.equal(old, want)
        assert "codes" not in m._last_kernel, m._last_kernel


# ---------------------------------------------------------------------------------------------- the fixture nets
def _build(net, dev):
    """The fixture's net out of the drop-in modules (tests/golden/netgen_r3.py) with its name-seeded parameters, BatchNorm
    statistics, weight gains and per-module scales, as tests/test_gpu_fire.py / tests/test_gpu_pw_entry.py build it; channels_last."""
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import netgen_r3 as ng
    import utils.conv2d_func as cf
    import utils.sfp_quant as sq
    gold = np.load(os.path.join(GOLDEN, "nets_r3_golden.npz"))
    q, batch, in_seed, seed = [int(v) for v in gold[net + ":meta"]]
    manifest = json.loads(bytes(gold[net + ":manifest"]).decode())
    gains = json.loads(bytes(gold[net + ":gains"]).decode())
    m = ng.BUILDERS[net](ng.Factories(cf, q, manifest, layerout=sq.layerout_quantize_func))
    ng.fill_parameters_by_name(m, seed, gains)
    bn = {k[len(net) + 1:]: gold[k] for k in gold.files if k.startswith(net + ":bn:")}
    if bn:
        ng.load_bn_stats_by_name_(m, bn)
    m = m.to(dev).eval().to(memory_format=torch.channels_last)
    x = ng.net_input224(batch, in_seed).to(dev).contiguous(memory_format=torch.channels_last)
    return m, x


def named_now(m):
    return dict(m.named_modules())


def _tree(m):
    return [(name, type(mod).__name__) for name, mod in m.named_modules()]


def test_squeezenet_chain_starts_at_the_image(dev, monkeypatch):
    """fuse_fire(entries=True) leaves the stem's in-place ReLU pass and float32 pool; link_stem removes them: features.0 writes
    features.3.squeeze's codes, the stem's pool runs on codes, no slfp_encode_f32 pass anywhere, the same logits."""
    from cnns_slfp_quantization_amd import fusion, graph, sfp_quant
    from cnns_slfp_quantization_amd import conv2d_func as impl
    m, x = _build("squeezenet", dev)
    tree0 = _tree(m)
    named = dict(m.named_modules())
    stem, sq3 = named["features.0"], named["features.3.squeeze"]
    calls = []
    real = sfp_quant.hip_encode

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)

    with torch.no_grad():
        y0 = m(x)
        assert fusion.fuse_fire(m, x, entries=True) == 8
        tree1 = _tree(m)
        assert fusion.link_stem(m, x) == 1
        assert fusion.link_stem(m, x) == 0   # already linked
        monkeypatch.setattr(sfp_quant, "hip_encode", counting)
        monkeypatch.setattr(impl, "hip_encode", counting)
        y1 = m(x)
        assert len(calls) == 0, len(calls)
        monkeypatch.setattr(sfp_quant, "hip_encode", real)
        monkeypatch.setattr(impl, "hip_encode", real)
        assert torch.equal(_i32(y1), _i32(y0)), float((y1 - y0).abs().max())
        k0 = stem._last_kernel
        assert k0.startswith("stem_mfma") and k0.endswith("+codes_out") and "codes_in" not in k0, k0
        pools = [n for n, c in m.named_modules() if isinstance(c, fusion.CodeMaxPool2d)]
        assert pools[0] == "features.2" and len(pools) == 3, pools
        assert isinstance(named_now(m)["features.1"], fusion.CodeReLU)   # the stem's in-place ReLU: no pass over the codes
        assert sq3._last_kernel.endswith("+codes_in+codes_out"), sq3._last_kernel
        g = graph.GraphedModule(m)
        assert torch.equal(_i32(g(x)), _i32(y0))
        assert torch.equal(_i32(g(x)), _i32(y0))
        del g
        assert fusion.unlink_stem(m) == 1 and fusion.unlink_stem(m) == 0
        assert _tree(m) == tree1 and stem._code_out is None and stem._post is None and not hasattr(stem, "_pre_link_post")
        assert torch.equal(_i32(m(x)), _i32(y0)) and "codes" not in stem._last_kernel
        assert fusion.unfuse_fire(m) == 8
        assert _tree(m) == tree0
        assert torch.equal(_i32(m(x)), _i32(y0))


def test_resnet50_stem_serves_both_readers_with_one_code_tensor(dev):
    """layer1.0.conv1 and layer1.0.downsample.0 read the same pooled tensor with the same Ka: after link_codes_traced(entries=True) the
    stem links to both, with and without fuse_residual."""
    from cnns_slfp_quantization_amd import fusion, layer_specs
    specs = layer_specs.conv_layers("resnet50_imagenet224")
    first = [specs[1], specs[4]]   # execution order: conv1, layer1.0.conv1 / conv2 / conv3 / downsample.0
    assert all(s.c_in == 64 and s.h == 56 and tuple(s.k) == (1, 1) for s in first) and [s.c_out for s in first] == [64, 256]
    assert first[0].Ka == first[1].Ka and specs[3].Ka != first[0].Ka   # the two readers of the pooled stem output share Ka; conv3 has its own
    m, x = _build("resnet50", dev)
    named = dict(m.named_modules())
    stem, c1, ds = named["conv1"], named["layer1.0.conv1"], named["layer1.0.downsample.0"]
    assert float(c1.Ka) == float(ds.Ka) and c1.q_bit == ds.q_bit
    with torch.no_grad():
        assert fusion.fuse_bn_relu(m) == 4            # the four downsample nn.Sequential(conv, bn)
        assert fusion.fuse_named_bn(m, example_input=x) == 49
        y_fused = m(x)
        for residual in (False, True):
            if residual:
                assert fusion.fuse_residual(m, x) == 16
            assert fusion.link_codes_traced(m, x, entries=True) == 32
            assert "codes" not in stem._last_kernel
            tree1 = _tree(m)
            assert fusion.link_stem(m, x) == 1
            y = m(x)
            assert torch.equal(_i32(y), _i32(y_fused)), float((y - y_fused).abs().max())
            assert stem._last_kernel == "stem_mfma_f16x1+codes_out", stem._last_kernel
            assert isinstance(m.maxpool, fusion.CodeMaxPool2d) and isinstance(m.relu, fusion.CodeReLU)
            # conv1 carries _code_entry from link_codes_traced and receives uint8: the code-input route, not the entry
            assert c1._code_entry and c1._last_kernel.endswith("+codes_in+codes_out"), c1._last_kernel
            assert "+codes_in" in ds._last_kernel and "codes_out" not in ds._last_kernel, ds._last_kernel
            if not residual:   # unlink_stem undoes exactly this link
                assert fusion.unlink_stem(m) == 1
                assert _tree(m) == tree1 and stem._code_out is None
                assert torch.equal(_i32(m(x)), _i32(y_fused)) and "codes" not in stem._last_kernel
                assert c1._last_kernel.endswith("+codes_out") and "codes_in" not in c1._last_kernel
                assert fusion.link_stem(m, x) == 1
            assert fusion.unlink_codes(m) == 33       # every link, the stem's among them
            assert not any(isinstance(c, (fusion.CodeMaxPool2d, fusion.CodeReLU)) for c in m.modules())
            assert not any(c._code_entry or c._code_out is not None or "_stem_link" in c.__dict__
                           for c in m.modules() if isinstance(c, torch.nn.Conv2d))
            assert fusion.unlink_stem(m) == 0
            assert torch.equal(_i32(m(x)), _i32(y_fused))


def _alexnet_head(dev, ka2=0.9):
    import utils.conv2d_func as cf
    C = cf.conv2d_Q_bias(q_bit=8, Kw=0.02, Ka=0.3)
    m = torch.nn.Sequential(C(3, 64, 11, 0.02, 0.3, 4, 2), torch.nn.ReLU(inplace=True), torch.nn.MaxPool2d(3, 2),
                            C(64, 192, 5, 0.02, ka2, 1, 2), torch.nn.ReLU(inplace=True))
    return m.to(dev).eval().to(memory_format=torch.channels_last)


def test_alexnet_head(dev):
    from cnns_slfp_quantization_amd import fusion
    torch.manual_seed(21)
    m = _alexnet_head(dev)
    x = (torch.randn(2, 3, 67, 67, device=dev) * 1.2).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        m[0].weight.mul_(0.5); m[3].weight.mul_(0.3)
        y0 = m(x)
        assert fusion.link_stem(m, x) == 1
        y1 = m(x)
        assert torch.equal(_i32(y1), _i32(y0)), float((y1 - y0).abs().max())
        assert m[0]._last_kernel == "stem_mfma_f16x1+codes_out" and isinstance(m[2], fusion.CodeMaxPool2d)
        assert isinstance(m[1], fusion.CodeReLU) and isinstance(m[4], torch.nn.ReLU)
        assert m[3]._last_kernel.startswith("dense_mfma") and "+codes_in" in m[3]._last_kernel, m[3]._last_kernel
        assert fusion.unlink_stem(m) == 1 and isinstance(m[2], torch.nn.MaxPool2d) and isinstance(m[1], torch.nn.ReLU) and m[0]._post is None
        assert torch.equal(_i32(m(x)), _i32(y0))


class _TwoReaders(torch.nn.Module):
    """stem -> ReLU -> pool -> two 1x1 readers (their outputs added); leak: the pooled tensor also goes into a torch.cat"""

    def __init__(self, ka_a, ka_b, leak):
        super().__init__()
        import utils.conv2d_func as cf
        C = cf.conv2d_Q(q_bit=8, Kw=0.02, Ka=0.3)
        self.stem = C(3, 64, 7, 0.02, 0.3, 2, 3)
        self.relu = torch.nn.ReLU()
        self.pool = torch.nn.MaxPool2d(3, 2, 1)
        self.a = C(64, 64, 1, 0.02, ka_a, 1, 0)
        self.b = C(64, 64, 1, 0.02, ka_b, 1, 0)
        self.leak = leak

    def forward(self, x):
        p = self.pool(self.relu(self.stem(x)))
        y = self.a(p) + self.b(p)
        return torch.cat([y, p], 1) if self.leak else y


@pytest.mark.parametrize("ka_b, leak, want", [(0.5, False, 1), (0.4, False, 0), (0.5, True, 0)], ids=["control", "other-Ka", "cat"])
def test_refusals_leave_the_model_untouched(dev, ka_b, leak, want):
    """Two readers with different Ka cannot share one code tensor; a torch.cat of the pooled tensor is a use no hook sees: the link is
    made, fails its own verification and is rolled back.  The control links."""
    from cnns_slfp_quantization_amd import fusion
    torch.manual_seed(31)
    m = _TwoReaders(0.5, ka_b, leak).to(dev).eval().to(memory_format=torch.channels_last)
    x = (torch.randn(2, 3, 37, 45, device=dev) * 1.2).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        m.stem.weight.mul_(0.5)
        y0 = m(x)
        tree0 = _tree(m)
        assert fusion.link_stem(m, x) == want
        y1 = m(x)
        assert torch.equal(_i32(y1), _i32(y0))
        if want:
            assert m.stem._last_kernel == "stem_mfma_f16x1+codes_out" and m.a._last_kernel.endswith("+codes_in")
            assert m.b._last_kernel.endswith("+codes_in") and isinstance(m.pool, fusion.CodeMaxPool2d) and isinstance(m.relu, fusion.CodeReLU)
            assert fusion.unlink_stem(m) == 1
        assert _tree(m) == tree0 and m.stem._code_out is None and m.stem._post is None and not hasattr(m.stem, "_pre_link_post")
        assert "_stem_link" not in m.stem.__dict__ and fusion.unlink_stem(m) == 0
        assert torch.equal(_i32(m(x)), _i32(y0)) and "codes" not in m.stem._last_kernel
