"""GPU (MI355X): the residual epilogue that also writes the next block's codes: slfp_conv2d_fwd_res_codes -- the
dual forms of k_pwc_stream / k_pwc_slice / k_pwc_tiled --, the module's `_trunk_code_out` route and fusion.link_trunk.

The contract, for every input: `y` is byte-equal to what slfp_conv2d_fwd_res writes for the same arguments with io->y_codes = 0, and
`y_codes` is byte-equal to slfp_encode_f32(y, io->y_ka, fmt(io->y_qbits) | SLFP_FMT_EXT) of that y; nothing else is touched.  Both
references are computed on the same device.  One geometry per kernel is also compared with the CPU oracle, under the family's bar."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

from oracle import slfp_oracle as so
from _bars import tol
from conftest import rel_errors

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GUARD = 256   # bytes of 0xA5 on both sides of both outputs


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from cnns_slfp_quantization_amd import _lib
    L = _lib.load()  # raises if libslfp_hip.so is missing: no fallback
    assert L.slfp_device_count() >= 1
    assert hasattr(L, "slfp_conv2d_fwd_res_codes")
    return _lib


@pytest.fixture(scope="module")
def arena(dev):
    """A device allocation of its own (32 MiB: a whole number of 2 MiB pages that the caching allocator hands to the device as it
    is, once its free blocks are released): the code tensor of one row is placed at its very end, so nothing lies behind its last byte."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return torch.empty(32 << 20, dtype=torch.uint8, device=dev)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return t.data_ptr() if t is not None else None


def _fmt(lib, qbits):
    return lib.FMT_ACT8 if qbits == 8 else lib.FMT_SFP7


def _encode(lib, x, ka, qbits):
    c = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    lib.check(lib.load().slfp_encode_f32(x.data_ptr(), c.data_ptr(), x.numel(), float(np.float32(ka)), _fmt(lib, qbits) | lib.FMT_EXT, _stream()))
    return c


def _decode(lib, c, qbits):
    x = torch.empty(c.shape, dtype=torch.float32, device=c.device)
    lib.check(lib.load().slfp_decode_f32(c.data_ptr(), x.data_ptr(), c.numel(), _fmt(lib, qbits) | lib.FMT_EXT, _stream()))
    return x


class _Layer:
    """A 1x1 stride-1 layer on NHWC tensors (n x h x w x c_in) that reads codes: weights, bias and a BN-like affine drawn on the CPU."""

    def __init__(self, lib, dev, gen, n, c_in, c_out, h, w, qbits, bias=False, ka=0.14, kw=0.0196):
        L = lib.load()
        self.lib, self.n, self.c_in, self.c_out, self.h, self.wd, self.qbits, self.ka, self.kw = lib, n, c_in, c_out, h, w, qbits, ka, kw
        self.d = lib.ConvDesc(n=n, c_in=c_in, h=h, w=w, c_out=c_out, kh=1, kw=1, stride_h=1, stride_w=1, pad_h=0, pad_w=0,
                              dil_h=1, dil_w=1, groups=1, x_layout=lib.LAYOUT_NHWC, y_layout=lib.LAYOUT_NHWC, qbits=qbits,
                              ka=float(np.float32(ka)), kw_scale=float(np.float32(kw)), mfma_passes=lib.MFMA_F16X1, reserved=0)
        self.w_cpu = torch.randn((c_out, c_in, 1, 1), generator=gen) * min(5.0 * kw, 3.0 * (2.0 / c_in) ** 0.5 + 2.0 * kw)
        self.b_cpu = torch.randn(c_out, generator=gen) * 0.2 if bias else None
        self.w = self.w_cpu.to(dev)
        self.b = self.b_cpu.to(dev) if bias else None
        self.ps = (0.5 + torch.rand(c_out, generator=gen)).to(dev)
        self.psh = (torch.randn(c_out, generator=gen) * 0.1).to(dev)
        self.blob = torch.empty(L.slfp_conv2d_wprep_bytes(ctypes.byref(self.d)), dtype=torch.uint8, device=dev)
        lib.check(L.slfp_conv2d_prepare_weights(ctypes.byref(self.d), self.w.data_ptr(), self.blob.data_ptr(), None, _stream()))
        self.kernel = L.slfp_conv2d_kernel_name(ctypes.byref(self.d)).decode()
        # post-ReLU-like activations over all binades and both clamps, with exact zeros and the tiny class, as this layer's codes
        x = torch.relu(torch.randn((n, h, w, c_in), generator=gen)) * (6.0 * ka)
        x.view(-1)[::97] = 17.0 * ka
        x.view(-1)[5::193] = 0.05 * ka
        self.x = _encode(lib, x.to(dev), ka, qbits)

    def out_shape(self):
        return (self.n, self.h, self.wd, self.c_out)

    def io(self, y_codes, y_ka=1.0, y_qbits=8):
        return self.lib.ConvIo(x_codes=1, y_codes=1 if y_codes else 0, y_ka=float(np.float32(y_ka)), y_qbits=y_qbits)

    def head(self, io, post):
        return (ctypes.byref(self.d), ctypes.byref(io), self.x.data_ptr(), self.blob.data_ptr(), _p(self.b),
                _p(self.ps) if post else None, _p(self.psh) if post else None)

    def supported(self, y_ka, y_qbits, relu):
        io = self.io(True, y_ka, y_qbits)
        return self.lib.load().slfp_conv2d_res_codes_supported(ctypes.byref(self.d), ctypes.byref(io), 1 if self.b is not None else 0, 1 if relu else 0)

    def fwd_codes(self, post):
        """the convolution alone, float32 out, no ReLU: slfp_conv2d_fwd_codes"""
        y = torch.empty(self.out_shape(), device=self.x.device)
        self.lib.check(self.lib.load().slfp_conv2d_fwd_codes(*self.head(self.io(False), post), 0, y.data_ptr(), _stream()))
        return y

    def fwd_res(self, res, relu, post):
        """the reference: slfp_conv2d_fwd_res with io->y_codes = 0"""
        y = torch.empty(self.out_shape(), device=self.x.device)
        self.lib.check(self.lib.load().slfp_conv2d_fwd_res(*self.head(self.io(False), post), 1 if relu else 0, res.data_ptr(), y.data_ptr(), None, _stream()))
        return y

    def fwd_dual(self, res, relu, post, y_ka, y_qbits, y_ptr, yc_ptr):
        io = self.io(True, y_ka, y_qbits)
        self.lib.check(self.lib.load().slfp_conv2d_fwd_res_codes(*self.head(io, post), 1 if relu else 0, res.data_ptr(), y_ptr, yc_ptr, None, _stream()))


def _residual(y0, y_ka, gen, special=True):
    """res = target - y0, so that the sums y0 + res land on a designed set of values of the consumer's quantizer (y_ka): both signs
    over eleven binades, exact zero (res = -y0), the tiny class, the top regular class and the clamp; then (special) a NaN, +inf,
    -inf and -0.0 element and a region at 2^-10 of the rest."""
    n = y0.numel()
    e = torch.rand(n, generator=gen) * 11.0 - 7.0
    t = y_ka * torch.exp2(e) * torch.where(torch.rand(n, generator=gen) < 0.3, -1.0, 1.0)
    t[::97] = 17.0 * y_ka     # beyond the clamp
    t[3::101] = 15.0 * y_ka   # the top regular class of both formats
    t[5::103] = 0.01 * y_ka   # the tiny class
    t[7::107] = 0.0           # exact zero, with and without the ReLU
    res = t.to(y0.device).view(y0.shape) - y0
    if special:
        flat = res.view(-1)
        lo = n // 2
        flat[lo:lo + n // 8] *= 2.0 ** -10
        flat[11], flat[n // 3], flat[n // 3 + 1], flat[n - 5] = float("nan"), float("inf"), float("-inf"), -0.0
    return res.contiguous()


def _guarded(nbytes, dev):
    buf = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    assert (buf.data_ptr() + GUARD) % 16 == 0
    return buf


def _guards_ok(buf, nbytes):
    return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + nbytes:] == 0xA5).all())


# form, C_in, C_out, images (n, h, w), bias
ROWS = [
    ("stream KS 1 (no XW)", 32, 48, [(3, 9, 7)], False),
    ("stream KS 2 XW", 64, 256, [(3, 9, 7), (3, 7, 9)], True),
    ("stream KS 4 XW", 128, 512, [(2, 7, 5)], False),
    ("stream KS 8 XW, dead channels in the last tile group", 256, 80, [(2, 7, 5)], False),
    ("stream KS 3", 96, 32, [(2, 7, 5)], False),
    ("stream half k-step", 48, 64, [(2, 7, 5)], False),
    ("slice NTS 8", 256, 1024, [(2, 7, 5), (1, 5, 7)], False),
    ("slice NTS 4", 256, 192, [(2, 7, 5)], True),
    ("tiled 64 x 512", 512, 2048, [(3, 5, 3)], False),
    ("tiled 64 x 512, channels past C_out, three row blocks", 512, 528, [(2, 15, 5), (2, 5, 15)], False),
    ("tiled 64 x 256", 512, 256, [(2, 15, 5)], False),
    ("tiled 64 x 128", 512, 128, [(2, 15, 5)], False),
    ("tiled 64 x 64", 512, 64, [(2, 15, 5)], False),
]


@pytest.mark.parametrize("qbits", [8, 7])
@pytest.mark.parametrize("row", ROWS, ids=["%d-%d" % (r[1], r[2]) for r in ROWS])
def test_both_outputs_are_byte_equal_to_their_references(lib, dev, arena, row, qbits):
    """Layer q_bit 8 / 7 (parametrised) x consumer q_bit 8 / 7 x ReLU folded / signed x with / without the affine, per image shape:
    y against slfp_conv2d_fwd_res (io->y_codes = 0), y_codes against slfp_encode_f32 of that y; guard bands of 0xA5 around both
    outputs; two launches give the same bits; for the first row the codes once more at the very end of an allocation."""
    form, c_in, c_out, images, bias = row
    for n, h, w in images:
        m = n * h * w
        assert m % 16 != 0 and m % 64 != 0
        gen = torch.Generator().manual_seed(1000 * qbits + c_in + c_out + h)
        lay = _Layer(lib, dev, gen, n, c_in, c_out, h, w, qbits, bias=bias)
        assert lay.kernel == ("pw_mfma_f16x1" if qbits == 8 else "pw_mfma_f16_exact"), lay.kernel
        y_ka = 0.31
        res = _residual(lay.fwd_codes(False), y_ka, gen)
        n_el = m * c_out
        for y_qbits in (8, 7):
            for relu in (True, False):
                for post in (False, True):
                    assert lay.supported(y_ka, y_qbits, relu) == 1, (form, y_qbits, relu)
                    want = lay.fwd_res(res, relu, post)
                    want_c = _encode(lib, want, y_ka, y_qbits).flatten()
                    first = row is ROWS[0] and y_qbits == qbits and not post
                    if first:   # the comparison is not vacuous: exact zero, tiny, the clamp (q_bit 8), the top regular code; NaN is 0x00 too
                        have = set(torch.unique(want_c).tolist())
                        top = 0x7F if y_qbits == 8 else 0x3F
                        assert {0x01, 0x00, top} <= have and (y_qbits == 7 or 0x02 in have), sorted(have)
                        assert relu or any(c & (0x80 if y_qbits == 8 else 0x40) for c in have), sorted(have)
                        assert int(torch.isnan(want).sum()) == (0 if relu else 1) and bool(torch.isinf(want).any())
                    outs = []
                    for _ in range(2):
                        yb, cb = _guarded(4 * n_el, dev), _guarded(n_el, dev)
                        lay.fwd_dual(res, relu, post, y_ka, y_qbits, yb.data_ptr() + GUARD, cb.data_ptr() + GUARD)
                        got, got_c = yb[GUARD:GUARD + 4 * n_el].view(torch.int32), cb[GUARD:GUARD + n_el]
                        key = (form, (n, h, w), qbits, y_qbits, relu, post)
                        assert torch.equal(got, want.view(torch.int32).flatten()), (key, int((got != want.view(torch.int32).flatten()).sum()))
                        assert torch.equal(got_c, want_c), (key, int((got_c != want_c).sum()))
                        assert _guards_ok(yb, 4 * n_el) and _guards_ok(cb, n_el), key
                        outs.append((got.clone(), got_c.clone()))
                    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
                    if first and relu:   # y_codes ends at the last byte of its allocation
                        tail = arena[arena.numel() - n_el - GUARD:]
                        tail.fill_(0xA5)
                        y = torch.empty(lay.out_shape(), device=dev)
                        lay.fwd_dual(res, relu, post, y_ka, y_qbits, y.data_ptr(), tail.data_ptr() + GUARD)
                        assert torch.equal(tail[GUARD:], want_c) and bool((tail[:GUARD] == 0xA5).all())
                        assert torch.equal(y.view(torch.int32), want.view(torch.int32))
    torch.cuda.synchronize()


ORACLE_CASES = [("k_pwc_stream", 64, 256, (3, 9, 7)), ("k_pwc_slice", 256, 1024, (2, 7, 5)), ("k_pwc_tiled", 512, 2048, (3, 5, 3))]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=[c[0] for c in ORACLE_CASES])
def test_float32_output_against_the_cpu_oracle(lib, dev, case):
    """relu(oracle.conv2d(decoded input) * scale + shift + res) in float64 against the float32 output of the dual launch, under the
    family's existing bar (tests/_bars.py); the codes of that output against the oracle's encoder.  Measured on
    the MI355X (max / l2 against the bar of 1e-3): k_pwc_stream 1.35e-04 / 8.0e-05, k_pwc_slice 2.29e-04 / 1.57e-04, k_pwc_tiled
    3.34e-04 / 2.26e-04."""
    _, c_in, c_out, (n, h, w) = case
    gen = torch.Generator().manual_seed(500 + c_in)
    lay = _Layer(lib, dev, gen, n, c_in, c_out, h, w, 8)
    y_ka = 0.31
    res = _residual(lay.fwd_codes(True), y_ka, gen, special=False)
    assert lay.supported(y_ka, 8, True) == 1
    y = torch.empty(lay.out_shape(), device=dev)
    yc = torch.empty(lay.out_shape(), dtype=torch.uint8, device=dev)
    lay.fwd_dual(res, True, True, y_ka, 8, y.data_ptr(), yc.data_ptr())
    # decode(code) is input_q = QA(x / Ka): times Ka it is an input whose quantizer returns exactly these classes
    xf = (_decode(lib, lay.x, 8).cpu().numpy().astype(np.float64) * np.float64(np.float32(lay.ka))).astype(np.float32).transpose(0, 3, 1, 2)
    ref = so.conv2d(np.ascontiguousarray(xf), lay.w_cpu.numpy(), None, (1, 1), (0, 0), (1, 1), 1, np.float64(lay.ka), np.float64(lay.kw),
                    8).astype(np.float64)
    ref = ref * lay.ps.cpu().numpy().astype(np.float64)[None, :, None, None] + lay.psh.cpu().numpy().astype(np.float64)[None, :, None, None]
    ref = np.maximum(ref + res.cpu().numpy().transpose(0, 3, 1, 2).astype(np.float64), 0.0)
    emax, el2 = rel_errors(y.cpu().numpy().transpose(0, 3, 1, 2), ref)
    print(f"{case[0]}: {lay.kernel} max {emax:.3e} l2 {el2:.3e} (bar {tol(lay.kernel):.0e})")
    assert emax <= tol(lay.kernel) and el2 <= tol(lay.kernel), (case, emax, el2)
    assert np.array_equal(yc.cpu().numpy(), so.encode(y.cpu().numpy(), np.float32(y_ka), so.FMT_ACT8 | so.FMT_EXT)), "codes != oracle"


# ------------------------------------------------------------------ the module
def _module_pair(dev, ka_next=0.31):
    import utils.conv2d_func as cf
    from cnns_slfp_quantization_amd.sfp_quant import hip_encode
    torch.manual_seed(11)
    gen = torch.Generator(device=dev).manual_seed(11)
    nhwc = torch.channels_last
    conv = cf.conv2d_Q(q_bit=8, Kw=0.02, Ka=0.3)(64, 256, 1, 0.02, 0.3).to(dev).eval().to(memory_format=nhwc)
    conv.residual_relu = True
    reader = cf.conv2d_Q(q_bit=8, Kw=0.02, Ka=ka_next)(256, 64, 1, 0.02, ka_next).to(dev).eval().to(memory_format=nhwc)
    x = torch.relu(torch.randn(3, 64, 9, 7, generator=gen, device=dev)).contiguous(memory_format=nhwc)
    xc = hip_encode(x, float(np.float32(0.3)), 0)
    r = torch.randn(3, 256, 9, 7, generator=gen, device=dev).contiguous(memory_format=nhwc)
    return conv, reader, xc, r


def test_module_route_fallback_and_scale_mismatch(dev, monkeypatch):
    from cnns_slfp_quantization_amd import conv2d_func as cfi
    from cnns_slfp_quantization_amd.sfp_quant import hip_encode
    conv, reader, xc, r = _module_pair(dev)
    with torch.no_grad():
        want = conv(xc, residual=r)
        assert conv._last_kernel == "pw_mfma_f16x1+codes_in+res" and "_trunk_codes" not in want.__dict__
        want_r = reader(want)
        assert "codes_in" not in reader._last_kernel
        # the route
        conv._trunk_code_out = (float(reader.Ka), 8)
        got = conv(xc, residual=r)
        assert conv._last_kernel == "pw_mfma_f16x1+codes_in+res+trunk_codes", conv._last_kernel
        assert got.dtype == torch.float32 and torch.equal(got, want) and conv.output is got
        codes, ka, q = got._trunk_codes
        assert (ka, q) == (float(reader.Ka), 8) and codes.dtype == torch.uint8 and codes.shape == got.shape
        assert torch.equal(codes, hip_encode(want, float(np.float32(float(reader.Ka))), 0))
        # the reader takes the codes: the same bits as from the float32 tensor
        got_r = reader(got)
        assert reader._last_kernel == "pw_mfma_f16x1+codes_in", reader._last_kernel
        assert torch.equal(got_r, want_r)
        # any op in between makes a tensor without the attribute
        assert torch.equal(reader(got * 1.0), want_r) and "codes_in" not in reader._last_kernel
        # a reader with another scale, or whose scale has changed since, reads the float32 tensor
        other = _module_pair(dev, ka_next=0.29)[1]
        want_o = other(want)
        assert torch.equal(other(got), want_o) and "codes_in" not in other._last_kernel
        reader.Ka = torch.tensor(0.29)
        stale = reader(got)
        assert "codes_in" not in reader._last_kernel and torch.equal(stale, reader(want))
        reader.Ka = torch.tensor(0.31)
        # float32 input: the residual route without codes (no dual form of the float32-input kernels)
        xf = torch.relu(torch.randn(3, 64, 9, 7, device=dev)).contiguous(memory_format=torch.channels_last)
        out = conv(xf, residual=r)
        assert conv._last_kernel == "pw_mfma_f16x1+res" and "_trunk_codes" not in out.__dict__
        # the query disabled: the old route, the same bytes, no codes handed on
        real = cfi._supported
        monkeypatch.setattr(cfi, "_supported", lambda mod, shape, kind, *a, **k: False if kind == "res_codes" else real(mod, shape, kind, *a, **k))
        conv._plans.clear()
        fb = conv(xc, residual=r)
        assert conv._last_kernel == "pw_mfma_f16x1+codes_in+res" and "_trunk_codes" not in fb.__dict__ and torch.equal(fb, want)
        assert torch.equal(reader(fb), want_r)
        monkeypatch.undo()


# ------------------------------------------------------------------ the ResNet-50 fixture net
def _build_resnet50(dev):
    """nets_imgnet/resnet50.py:24-147 out of the drop-in modules (tests/golden/netgen_r3.py) with the fixture's name-seeded
    parameters, BatchNorm statistics, weight gains and per-module scales (as tests/test_gpu_residual.py builds it)."""
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


def _blocks(m):
    return [b for b in m.modules() if type(b).__name__ == "_Bottleneck"]


def _readers(blk):
    ds = getattr(blk, "downsample", None)
    return [blk.conv1] + ([ds[0]] if ds is not None else [])


def _snapshot(m):
    return [(id(c), c._code_out, c._code_entry, c._trunk_code_out, c._post, "_trunk_link" in c.__dict__)
            for c in m.modules() if hasattr(c, "_trunk_code_out")] + [(id(b), "forward" in b.__dict__) for b in _blocks(m)]


def test_resnet50_link_trunk(dev, lib, monkeypatch):
    from cnns_slfp_quantization_amd import fusion, graph
    m, x = _build_resnet50(dev)
    blocks = _blocks(m)
    assert len(blocks) == 16
    L = lib.load()
    entries = []
    real_entry = L.slfp_conv2d_fwd_entry
    monkeypatch.setattr(L, "slfp_conv2d_fwd_entry", lambda *a: (entries.append(1), real_entry(*a))[1])
    with torch.no_grad():
        assert fusion.fuse_bn_relu(m) == 4 and fusion.fuse_named_bn(m, example_input=x) == 49
        # the reference's own forward (out += identity): nothing to link, nothing touched
        before = _snapshot(m)
        assert fusion.link_trunk(m, x) == 0 and _snapshot(m) == before
        assert fusion.fuse_residual(m, x) == 16
        before_links = _snapshot(m)
        assert fusion.link_trunk(m, x) == 0 and _snapshot(m) == before_links   # conv3 reads float32: no dual form of those kernels
        n_codes = fusion.link_codes_traced(m, x, entries=True)
        assert n_codes >= 32
        assert fusion.link_stem(m, x) == 1
        y0 = m(x)
        del entries[:]
        m(x)
        assert len(entries) == 15, len(entries)   # every conv1 but layer1.0's (which reads the stem's codes) enters through float32
        linked = _snapshot(m)
        # the blocks whose readers share a scale
        want_links = sum(1 for a, b in zip(blocks, blocks[1:]) if len({(float(r.Ka), int(r.q_bit)) for r in _readers(b)}) == 1)
        assert want_links == 15
        assert fusion.link_trunk(m, x) == want_links
        del entries[:]
        y1 = m(x)
        assert torch.equal(y1.view(torch.int32), y0.view(torch.int32))
        assert len(entries) == 0   # no slfp_conv2d_fwd_entry launch is left in the forward
        for i, b in enumerate(blocks):
            assert "+codes_in" in b.conv1._last_kernel, (i, b.conv1._last_kernel)
            if getattr(b, "downsample", None) is not None:
                assert "+codes_in" in b.downsample[0]._last_kernel, (i, b.downsample[0]._last_kernel)
            want = "+codes_in+res+trunk_codes" if i < 15 else "+codes_in+res"
            assert b.conv3._last_kernel.endswith(want), (i, b.conv3._last_kernel)
        assert sum(1 for b in blocks if getattr(b, "downsample", None) is not None) == 4
        # two replays of one hipGraph
        g = graph.GraphedModule(m)
        assert torch.equal(g(x).view(torch.int32), y0.view(torch.int32))
        assert torch.equal(g(x).view(torch.int32), y0.view(torch.int32))
        # and back
        assert fusion.unlink_trunk(m) == want_links and _snapshot(m) == linked
        assert torch.equal(m(x).view(torch.int32), y0.view(torch.int32))
        assert fusion.link_trunk(m, x) == want_links
        # unlink_codes and unfuse_residual leave no trunk consumer behind
        assert fusion.unlink_codes(m) == n_codes + 1
        assert all(c._trunk_code_out is None and "_trunk_link" not in c.__dict__ for c in m.modules() if hasattr(c, "_trunk_code_out"))
        assert fusion.unlink_trunk(m) == 0 and _snapshot(m) == before_links
        assert torch.equal(m(x).view(torch.int32), y0.view(torch.int32))
        assert fusion.unfuse_residual(m) == 16 and _snapshot(m) == before
        assert torch.equal(m(x).view(torch.int32), y0.view(torch.int32))


def test_unfuse_residual_takes_the_trunk_links_along(dev):
    from cnns_slfp_quantization_amd import fusion
    m, x = _tiny_net(dev)
    with torch.no_grad():
        y0 = m(x)
        assert fusion.fuse_residual(m, x) == 4 and fusion.link_codes_traced(m, x, entries=True) >= 4
        assert fusion.link_trunk(m, x) == 3
        assert fusion.unfuse_residual(m) == 4
        assert all(c._trunk_code_out is None and "_trunk_link" not in c.__dict__ for c in m.modules() if hasattr(c, "_trunk_code_out"))
        assert torch.equal(m(x), y0)


# ------------------------------------------------------------------ refusals, on four small blocks with the Bottleneck's child names
def _tiny_net(dev, down_ka=0.3, grouped=False):
    import utils.conv2d_func as cf

    class _Bottleneck(torch.nn.Module):
        def __init__(self, down=None, groups=1):
            super().__init__()
            C = cf.conv2d_Q(q_bit=8, Kw=0.02, Ka=0.3)
            self.conv1 = C(64, 32, 1, 0.02, 0.3, groups=groups)
            self.bn1 = torch.nn.Identity()
            self.conv2 = C(32, 32, 3, 0.02, 0.3, 1, 1)
            self.bn2 = torch.nn.Identity()
            self.conv3 = C(32, 64, 1, 0.02, 0.3)
            self.bn3 = torch.nn.Identity()
            self.relu = torch.nn.ReLU()
            self.downsample = torch.nn.Sequential(C(64, 64, 1, 0.02, down)) if down is not None else None

        def forward(self, x):
            h = self.relu(self.bn1(self.conv1(x)))
            h = self.relu(self.bn2(self.conv2(h)))
            out = self.bn3(self.conv3(h))
            return self.relu(out + (x if self.downsample is None else self.downsample(x)))

    torch.manual_seed(7)
    m = torch.nn.Sequential(_Bottleneck(), _Bottleneck(down=down_ka), _Bottleneck(), _Bottleneck(groups=2 if grouped else 1))
    m = m.to(dev).eval().to(memory_format=torch.channels_last)
    with torch.no_grad():
        for c in m.modules():
            if hasattr(c, "_trunk_code_out"):
                c.weight.mul_(0.5)
    gen = torch.Generator(device=dev).manual_seed(8)
    x = torch.randn(2, 64, 9, 7, generator=gen, device=dev).contiguous(memory_format=torch.channels_last)
    return m, x


@pytest.mark.parametrize("down_ka, grouped, want", [(0.3, False, [1, 1, 1]), (0.27, False, [0, 1, 1]), (0.3, True, [1, 1, 0]),
                                                     (0.27, True, [0, 1, 0])])
def test_a_block_whose_readers_cannot_share_the_codes_is_left_alone(dev, down_ka, grouped, want):
    """Block 1 has a downsample conv: with another Ka than its conv1 the two readers cannot share one code tensor -- block 0 is not
    linked, the others are.  Block 3's conv1 is a grouped 1x1 with `grouped`: no code-input kernel -- block 2 is not linked."""
    from cnns_slfp_quantization_amd import fusion
    m, x = _tiny_net(dev, down_ka, grouped)
    with torch.no_grad():
        y0 = m(x)
        assert fusion.fuse_residual(m, x) == 4
        assert fusion.link_codes_traced(m, x, entries=True) >= 4
        assert all(b.conv3._last_kernel.endswith("+codes_in+res") for b in m)
        assert fusion.link_trunk(m, x) == sum(want)
        assert [int(b.conv3._trunk_code_out is not None) for b in m][:3] == want and m[3].conv3._trunk_code_out is None
        y1 = m(x)
        assert torch.equal(y1, y0) and "_trunk_codes" not in y1.__dict__
        for i in range(3):
            assert m[i].conv3._last_kernel.endswith("+res+trunk_codes") == bool(want[i]), (i, m[i].conv3._last_kernel)
            readers = [m[i + 1].conv1] + ([m[i + 1].downsample[0]] if m[i + 1].downsample is not None else [])
            for r in readers:
                assert ("+codes_in" in r._last_kernel) == bool(want[i]), (i, r._last_kernel)
        assert fusion.unlink_trunk(m) == sum(want)
        assert torch.equal(m(x), y0)
