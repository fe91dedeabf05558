"""MI355X: the pointwise entry layer -- a 1x1 Conv2d_Q layer that reads float32 and writes the consumer's 1-byte
codes in one launch (slfp_conv2d_fwd_entry; the YC forms of k_pw_stream / k_pw_tiled): bit identity with slfp_encode_f32 of the
float32 interface's output through the C ABI on every code path, the consumer side, the CPU oracle, the module, and the two
fixture nets through fusion.link_codes_traced(entries=True) / fusion.fuse_fire(entries=True)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import slfp_oracle as so

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


class _Layer:
    """One Conv2d_Q layer on NHWC tensors (logical n x c_in x h x w) with weights, bias and a BN-like affine drawn on the CPU."""

    def __init__(self, lib, dev, gen, n, c_in, c_out, h, w, qbits, k=1, stride=1, bias=False, ka=0.31, kw=0.02):
        L = lib.load()
        self.lib, self.n, self.c_in, self.c_out, self.h, self.wd, self.qbits, self.ka, self.kw = lib, n, c_in, c_out, h, w, qbits, ka, kw
        self.d = lib.ConvDesc(n=n, c_in=c_in, h=h, w=w, c_out=c_out, kh=k, kw=k, stride_h=stride, stride_w=stride, pad_h=k // 2, pad_w=k // 2,
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
        ws_n = L.slfp_conv2d_workspace_bytes(ctypes.byref(self.d))
        self.ws = torch.empty(ws_n, dtype=torch.uint8, device=dev) if ws_n else None
        self.kernel = L.slfp_conv2d_kernel_name(ctypes.byref(self.d)).decode()

    def out_shape(self):
        return (self.n, self.ho, self.wo, self.c_out)

    def fwd_f32(self, x, relu, post):
        y = torch.empty(self.out_shape(), device=x.device)
        self.lib.check(self.lib.load().slfp_conv2d_fwd_post(ctypes.byref(self.d), x.data_ptr(), self.blob.data_ptr(), _p(self.b),
                                                            _p(self.ps) if post else None, _p(self.psh) if post else None,
                                                            1 if relu else 0, y.data_ptr(), None, _p(self.ws), _stream()))
        return y

    def io(self, y_ka, y_qbits=None):
        return self.lib.ConvIo(x_codes=0, y_codes=1, y_ka=float(np.float32(y_ka)), y_qbits=y_qbits or self.qbits)

    def entry_ok(self, y_ka, relu):
        io = self.io(y_ka)
        return self.lib.load().slfp_conv2d_entry_supported(ctypes.byref(self.d), ctypes.byref(io), 1 if self.b is not None else 0, 1 if relu else 0) == 1

    def fwd_entry(self, x, relu, post, y_ka, y_ptr):
        """slfp_conv2d_fwd_entry into the out_shape() bytes at y_ptr"""
        io = self.io(y_ka)
        self.lib.check(self.lib.load().slfp_conv2d_fwd_entry(ctypes.byref(self.d), ctypes.byref(io), x.data_ptr(), self.blob.data_ptr(), _p(self.b),
                                                             _p(self.ps) if post else None, _p(self.psh) if post else None,
                                                             1 if relu else 0, y_ptr, _stream()))


def _input(lay, dev, gen, special=False):
    """activations of both signs whose pixels span six binades (so the outputs reach from the tiny class to the clamp), one pixel of
    exact zeros; special: a NaN, +inf, -inf and -0.0 among them"""
    x = torch.randn((lay.n, lay.h, lay.wd, lay.c_in), generator=gen) * (4.0 * lay.ka)
    px = x.view(-1, lay.c_in)
    px *= torch.pow(2.0, -(torch.arange(px.shape[0]) % 6).float()).unsqueeze(1)
    px[px.shape[0] // 2] = 0.0
    if special:
        px[1, 3], px[2, 5], px[3, 7], px[4, 9] = float("nan"), float("inf"), float("-inf"), -0.0
    return x.to(dev)


def _consumer_scale(lay, want, relu):
    """A consumer Ka for which `want` (the float32 interface's output without a ReLU) reaches the clamp and the top regular class:
    the k-th largest finite value sits at 15.0 Ka (top class of both formats: [14.75, 15.32] Ka and [14.5, inf) Ka); the first k for
    which the library has a code table."""
    v = want[torch.isfinite(want)].flatten().sort(descending=True).values
    for k in range(max(2, v.numel() // 100), v.numel()):
        ka = float(np.float32(float(v[k]) / 15.0))
        if ka > 0 and float(v[0]) > 15.4 * ka and lay.entry_ok(ka, relu):
            return ka
    raise AssertionError("no consumer scale found")


# C_in, C_out, n, h, w, stride, bias, what it reaches
ROWS = [
    (64, 64, 1, 5, 7, 1, False, "stream KS 2, ragged last unit (M = 35)"),
    (32, 16, 2, 3, 3, 1, False, "stream KS 1, one live tile of the four-tile group"),
    (64, 48, 1, 4, 4, 1, False, "stream, M = 16 exactly, N = 48"),
    (96, 16, 1, 6, 5, 1, True, "stream KS 3: features.3.squeeze"),
    (40, 32, 1, 5, 4, 1, False, "stream, K not a multiple of 32"),
    (64, 64, 1, 9, 7, 2, False, "x_row_offset on a non-square strided input"),
    (256, 64, 2, 7, 7, 1, False, "tiled 64 x 64, M = 98"),
    (256, 128, 2, 7, 7, 1, False, "tiled 64 x 128"),
    (512, 256, 2, 7, 7, 1, False, "tiled 64 x 256"),
    (1024, 512, 2, 7, 7, 1, False, "tiled 64 x 512, 8 waves"),
    (2048, 512, 1, 7, 7, 1, False, "layer4 conv1, M = 49 < one tile"),
    (96, 256, 1, 10, 7, 1, False, "tiled, K not a multiple of 64"),
    (256, 80, 1, 13, 5, 1, False, "tiled, channel tiles past C_out, M = 65"),
]


@pytest.mark.parametrize("qbits", [8, 7])
@pytest.mark.parametrize("row", ROWS, ids=["%d-%d-%dx%dx%d-s%d" % r[:6] for r in ROWS])
def test_entry_codes_equal_the_encoded_float32_output(lib, dev, arena, row, qbits):
    """slfp_conv2d_fwd_entry == slfp_encode_f32(slfp_conv2d_fwd_post(...), y_ka, fmt | EXT), byte for byte, with the ReLU folded and
    without (signed codes), with and without the affine; 64 guard bytes of 0xA5 on each side stay untouched, the guarded buffer
    ends at the last byte of its allocation; and once more with the codes themselves ending there."""
    c_in, c_out, n, h, w, stride, bias, _ = row
    gen = torch.Generator().manual_seed(1000 * qbits + c_in + c_out + h)
    lay = _Layer(lib, dev, gen, n, c_in, c_out, h, w, qbits, stride=stride, bias=bias)
    assert lay.kernel.startswith("pw_mfma"), lay.kernel
    x = _input(lay, dev, gen, special=(row is ROWS[0]))
    nbytes = lay.n * lay.ho * lay.wo * c_out
    assert nbytes % 16 == 0
    y_ka = _consumer_scale(lay, lay.fwd_f32(x, False, False), True)
    end = arena.numel()
    for relu in (True, False):
        for post in (False, True):
            assert lay.entry_ok(y_ka, relu)
            want = _encode(lib, lay.fwd_f32(x, relu, post), y_ka, qbits).flatten()
            buf = arena[end - nbytes - 2 * GUARD:]
            buf.fill_(0xA5)
            assert (buf.data_ptr() + GUARD) % 16 == 0
            lay.fwd_entry(x, relu, post, y_ka, buf.data_ptr() + GUARD)
            got = buf[GUARD:GUARD + nbytes]
            assert torch.equal(got, want), (row, qbits, relu, post, int((got != want).sum()))
            assert bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + nbytes:] == 0xA5).all()), (row, qbits, relu, post)
            if relu and not post:
                have = set(torch.unique(want).tolist())
                top = 0x7F if qbits == 8 else 0x3F
                if row is ROWS[0]:   # the reference codes span the whole code space: exact zero, tiny, the clamp, the top regular code
                    print(f"{row[:6]} qbits {qbits}: y_ka {y_ka:.6g}, {len(have)} distinct codes")
                    assert {0x01, 0x00, top} <= have, sorted(have)
                    assert qbits == 7 or 0x02 in have, sorted(have)
                tail = arena[end - nbytes - GUARD:]   # the codes end at the allocation's last byte
                tail.fill_(0xA5)
                lay.fwd_entry(x, relu, post, y_ka, tail.data_ptr() + GUARD)
                assert torch.equal(tail[GUARD:], want) and bool((tail[:GUARD] == 0xA5).all())
    torch.cuda.synchronize()


@pytest.mark.parametrize("qbits", [8, 7])
def test_a_dense_consumer_reads_the_entry_codes(lib, dev, qbits):
    """64 -> 64 @ 2 x 8 x 6 written as codes by the new kernel, read by a 3 x 3 64 -> 64 dense layer (x_codes = 1, float32 out): the
    float32 chain's result, bit for bit."""
    gen = torch.Generator().manual_seed(77 + qbits)
    pw = _Layer(lib, dev, gen, 2, 64, 64, 8, 6, qbits)
    dn = _Layer(lib, dev, gen, 2, 64, 64, 8, 6, qbits, k=3, ka=0.27)
    x = _input(pw, dev, gen)
    want = dn.fwd_f32(pw.fwd_f32(x, True, True), True, False)
    codes = torch.empty(pw.out_shape(), dtype=torch.uint8, device=dev)
    assert pw.entry_ok(dn.ka, True)
    pw.fwd_entry(x, True, True, dn.ka, codes.data_ptr())
    L = lib.load()
    io = lib.ConvIo(x_codes=1, y_codes=0, y_ka=1.0, y_qbits=qbits)
    assert L.slfp_conv2d_codes_supported(ctypes.byref(dn.d), ctypes.byref(io), 0, 1) == 1
    got = torch.empty(dn.out_shape(), device=dev)
    lib.check(L.slfp_conv2d_fwd_codes_ws(ctypes.byref(dn.d), ctypes.byref(io), codes.data_ptr(), dn.blob.data_ptr(), None, None, None, 1,
                                         got.data_ptr(), _p(dn.ws), _stream()))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), float((got - want).abs().max())


def test_the_squeeze_row_against_the_cpu_oracle(lib, dev):
    """SFP<3,3>, 96 -> 16 @ 1 x 6 x 5 with bias and the ReLU folded: the new kernel's codes against oracle.conv2d (contraction in double,
    rounded once) quantized for y_ka.  Products are exact in this format, so the two differ only where a float32 accumulation lands
    on the other side of a class boundary of the consumer's quantizer; the number of such codes may not exceed the number by which
    the oracle's own float32 accumulation (ATen on the CPU, the reference's arithmetic) differs from its double accumulation on
    the same case.  The bound is computed here and printed."""
    gen = torch.Generator().manual_seed(96)
    lay = _Layer(lib, dev, gen, 1, 96, 16, 6, 5, 7, bias=True)
    x = _input(lay, dev, gen)
    y_ka = 0.4
    xn = x.cpu().permute(0, 3, 1, 2).contiguous().numpy()
    wn, bn = lay.w_cpu.numpy(), lay.b_cpu.numpy()
    ka, kw = np.float32(lay.ka), np.float32(lay.kw)
    ref = np.maximum(so.conv2d(xn, wn, bn, 1, 0, 1, 1, np.float64(ka), np.float64(kw), 7), 0.0)
    ref_codes = so.encode(ref.astype(np.float32), np.float32(y_ka), so.FMT_SFP7 | so.FMT_EXT)
    xq = torch.from_numpy(so.quantize(xn, ka, so.FMT_SFP7))
    wq = torch.from_numpy(so.quantize(wn, kw, so.FMT_SFP7))
    f32 = torch.relu(F.conv2d(xq, wq, torch.from_numpy(bn) / ka / kw) * ka * kw).numpy()
    f32_codes = so.encode(f32, np.float32(y_ka), so.FMT_SFP7 | so.FMT_EXT)
    bound = int(np.sum(ref_codes != f32_codes))
    assert lay.entry_ok(y_ka, True)
    codes = torch.empty(lay.out_shape(), dtype=torch.uint8, device=dev)
    lay.fwd_entry(x, True, False, y_ka, codes.data_ptr())
    got = codes.cpu().permute(0, 3, 1, 2).numpy()
    diff = int(np.sum(got != ref_codes))
    print(f"entry 96 -> 16 vs oracle (double): {diff} of {got.size} codes differ; oracle float32 vs double: {bound}")
    assert len(np.unique(ref_codes)) > 8
    assert diff <= bound, (diff, bound)


# ---------------------------------------------------------------------------------------------- the module
@pytest.mark.parametrize("qbits", [8, 7])
def test_module_with_code_entry(dev, qbits):
    import utils.conv2d_func as cf
    from cnns_slfp_quantization_amd import sfp_quant
    from cnns_slfp_quantization_amd.conv2d_func import _act_fmt
    torch.manual_seed(3)
    m = cf.conv2d_Q_bias(q_bit=qbits, Kw=0.02, Ka=0.3)(64, 64, 1, 0.02, 0.3).to(dev).eval().to(memory_format=torch.channels_last)
    x = (torch.randn(2, 64, 9, 5, device=dev) * 1.2).contiguous(memory_format=torch.channels_last)
    out = (0.27, qbits)
    with torch.no_grad():
        m.weight.mul_(0.5)
        y = m(x)
        xq = m.input_q.clone()
        assert "codes" not in m._last_kernel
        want = sfp_quant.hip_encode(y, out[0], _act_fmt(qbits))
        m._code_out, m._code_entry = out, True
        got = m(x)
        assert got.dtype == torch.uint8 and torch.equal(got, want)
        assert m._last_kernel.startswith("pw_mfma") and m._last_kernel.endswith("+codes_out") and "codes_in" not in m._last_kernel, m._last_kernel
        assert torch.equal(m.input_q.view(torch.int32), xq.view(torch.int32))
        m._code_entry = False
        old = m(x)
        assert old.dtype == torch.uint8 and torch.equal(old, want)
        assert "codes" not in m._last_kernel, m._last_kernel   # the old route: the float32 kernel, then slfp_encode_f32


# ---------------------------------------------------------------------------------------------- the ResNet-50 fixture
def _build_resnet50(dev):
    """nets_imgnet/resnet50.py:24-147 out of the drop-in modules (tests/golden/netgen_r3.py) with the fixture's name-seeded
    parameters, BatchNorm statistics, weight gains and per-module scales, as tests/test_gpu_residual.py builds it."""
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


def _i32(t):
    return t.view(torch.int32)


def test_resnet50_with_entry_links(dev):
    """conv1 -> conv2 of every Bottleneck becomes a code hand-over too: 32 links instead of 16, the same logits, every block on
    pw_mfma+codes_out / +codes_in+codes_out / +codes_in+res; the stem and the downsample convs keep float32."""
    from cnns_slfp_quantization_amd import fusion, graph
    m, x = _build_resnet50(dev)
    blocks = [b for b in m.modules() if type(b).__name__ == "_Bottleneck"]
    assert len(blocks) == 16
    with torch.no_grad():
        assert fusion.fuse_bn_relu(m) == 4            # the four downsample nn.Sequential(conv, bn)
        assert fusion.fuse_named_bn(m, example_input=x) == 49
        assert fusion.fuse_residual(m, x) == 16
        y_fused = m(x)
        assert fusion.link_codes_traced(m, x) == 16   # the control: the default is what it was
        assert not any(c._code_entry for c in m.modules() if isinstance(c, torch.nn.Conv2d))
        assert fusion.unlink_codes(m) == 16
        assert fusion.link_codes_traced(m, x, entries=True) == 32
        y = m(x)
        assert torch.equal(_i32(y), _i32(y_fused)), float((y - y_fused).abs().max())
        for b in blocks:
            k1, k2, k3 = b.conv1._last_kernel, b.conv2._last_kernel, b.conv3._last_kernel
            assert k1.startswith("pw_mfma") and k1.endswith("+codes_out") and "codes_in" not in k1, k1
            assert b.conv1._code_entry
            assert k2.endswith("+codes_in+codes_out"), k2
            assert k3.endswith("+codes_in+res"), k3
        inside = {c for b in blocks for c in (b.conv1, b.conv2, b.conv3)}
        others = [c for c in m.modules() if isinstance(c, torch.nn.Conv2d) and c not in inside]
        assert len(others) == 5 and all("codes" not in c._last_kernel for c in others), [c._last_kernel for c in others]
        g = graph.GraphedModule(m)
        assert torch.equal(_i32(g(x)), _i32(y_fused))
        assert torch.equal(_i32(g(x)), _i32(y_fused))
        del g
        assert fusion.unlink_codes(m) == 32
        assert not any(c._code_entry or c._code_out is not None for c in m.modules() if isinstance(c, torch.nn.Conv2d))
        assert torch.equal(_i32(m(x)), _i32(y_fused))
        # the other order: links first, the residual fusion on top
        assert fusion.unfuse_residual(m) == 16
        assert fusion.link_codes_traced(m, x, entries=True) == 32
        assert fusion.fuse_residual(m, x) == 16
        assert torch.equal(_i32(m(x)), _i32(y_fused))
        assert all(b.conv3._last_kernel.endswith("+codes_in+res") and b.conv1._last_kernel.endswith("+codes_out") for b in blocks)


# ---------------------------------------------------------------------------------------------- the SqueezeNet fixture
def _build_squeezenet(dev):
    """The fixture's SqueezeNet 1.0 out of the drop-in modules, as tests/test_gpu_fire.py builds it; channels_last."""
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import netgen_r3 as ng
    import utils.conv2d_func as cf
    import utils.sfp_quant as sq
    gold = np.load(os.path.join(GOLDEN, "nets_r3_golden.npz"))
    q, batch, in_seed, seed = [int(v) for v in gold["squeezenet:meta"]]
    manifest = json.loads(bytes(gold["squeezenet:manifest"]).decode())
    gains = json.loads(bytes(gold["squeezenet:gains"]).decode())
    m = ng.BUILDERS["squeezenet"](ng.Factories(cf, q, manifest, layerout=sq.layerout_quantize_func))
    ng.fill_parameters_by_name(m, seed, gains)
    m = m.to(dev).eval().to(memory_format=torch.channels_last)
    x = ng.net_input224(batch, in_seed).to(dev).contiguous(memory_format=torch.channels_last)
    return m, x


def test_squeezenet_fire_chain_starts_without_an_encode_pass(dev, monkeypatch):
    from cnns_slfp_quantization_amd import fusion, sfp_quant
    m, x = _build_squeezenet(dev)
    tree0 = [(name, type(mod).__name__) for name, mod in m.named_modules()]
    named = dict(m.named_modules())
    sq3 = named["features.3.squeeze"]
    calls = []
    real = sfp_quant.hip_encode

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)

    with torch.no_grad():
        y0 = m(x)
        assert fusion.fuse_fire(m, x, entries=True) == 8
        monkeypatch.setattr(sfp_quant, "hip_encode", counting)
        y1 = m(x)
        assert len(calls) == 0, len(calls)
        assert torch.equal(_i32(y1), _i32(y0)), float((y1 - y0).abs().max())
        k = sq3._last_kernel
        assert "+codes_out" in k and "codes_in" not in k and sq3._code_entry, k
        monkeypatch.setattr(sfp_quant, "hip_encode", real)
        assert fusion.unfuse_fire(m) == 8
        assert [(name, type(mod).__name__) for name, mod in m.named_modules()] == tree0
        assert not any(c._code_entry or c._code_out is not None for c in m.modules() if isinstance(c, torch.nn.Conv2d))
        # the control: without entries the head of the chain is one slfp_encode_f32 pass
        assert fusion.fuse_fire(m, x) == 8
        monkeypatch.setattr(sfp_quant, "hip_encode", counting)
        y2 = m(x)
        assert len(calls) == 1, len(calls)
        assert torch.equal(_i32(y2), _i32(y0)) and "codes_in" in sq3._last_kernel
        monkeypatch.setattr(sfp_quant, "hip_encode", real)
        assert fusion.unfuse_fire(m) == 8


# ---------------------------------------------------------------------------------------------- roll-back
def test_entry_links_roll_back_when_a_tensor_has_a_use_hooks_cannot_see(dev):
    """A block that also concatenates the 1x1 producer's output in its forward() (a functional use no module hook records): with
    entries=True the candidate link passes the wiring checks, fails the bit-for-bit verification and is rolled back."""
    from cnns_slfp_quantization_amd import fusion
    import utils.conv2d_func as cf

    class Blk(torch.nn.Module):
        def __init__(self, leak):
            super().__init__()
            C = cf.conv2d_Q(q_bit=8, Kw=0.02, Ka=0.3)
            self.a = C(32, 32, 1, 0.02, 0.3, 1, 0)
            self.b = C(32, 64, 1, 0.02, 0.25, 1, 0)
            self.relu = torch.nn.ReLU()
            self.leak = leak

        def forward(self, x):
            h = self.relu(self.a(x))
            y = self.b(h)
            return torch.cat([y, h], 1) if self.leak else y

    torch.manual_seed(5)
    x = torch.randn(2, 32, 12, 12, device=dev).contiguous(memory_format=torch.channels_last)
    for leak, entries, want in ((True, True, 0), (False, False, 0), (False, True, 1)):
        m = Blk(leak).to(dev).eval().to(memory_format=torch.channels_last)
        with torch.no_grad():
            m.a.weight.mul_(0.5); m.b.weight.mul_(0.5)
            y0 = m(x)
            assert fusion.link_codes_traced(m, x, entries=entries) == want, (leak, entries)
            assert (m.a._code_out is not None) == bool(want) and m.a._code_entry == bool(want)
            assert torch.equal(m(x), y0)
            if want:
                assert m.a._last_kernel.endswith("+codes_out") and "codes_in" not in m.a._last_kernel, m.a._last_kernel
            assert fusion.unlink_codes(m) == want and m.a._post is None and not m.a._code_entry
