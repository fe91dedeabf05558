"""GPU (MI355X): the depthwise -> pointwise block as ONE kernel on 1-byte codes (csrc/conv_dwpw_codes.hip;
include/slfp.h: slfp_dwpw_fwd_codes), through the C ABI and through fusion.DwPwBlock.

The bar is bit-identity with what runs today: the same two layers through slfp_conv2d_fwd_codes_ws twice -- depthwise codes -> codes
for the pointwise layer's Ka (k_dwc), pointwise codes -> float32 or the reader's codes (k_pwc_stream).  float32 is compared as
int32, codes as bytes; there is no tolerance anywhere in this file.  Every refused combination is checked through the query or a
status code on the host (tests/test_dwpw_codes_host.py), never by launching it."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

KA_DW, KW_DW, KA_PW, KW_PW, KA_NEXT = 0.17, 0.11, 0.33, 0.07, 0.29


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


def _ptr(t):
    return t.data_ptr() if t is not None else None


class _Block:
    """The two layers of a block (NHWC tensors, C ABI): descriptors, random weights, prepared blobs, folded-BN vectors."""

    def __init__(self, lib, dev, gen, C, N, S, H, W, B, qbits, pad=1, bias=False, shift_by=0.0):
        L = lib.load()
        self.lib, self.qbits, self.B, self.C, self.N = lib, qbits, B, C, N
        self.Ho, self.Wo = (H + 2 * pad - 3) // S + 1, (W + 2 * pad - 3) // S + 1
        self.H, self.W = H, W
        common = dict(dil_h=1, dil_w=1, x_layout=lib.LAYOUT_NHWC, y_layout=lib.LAYOUT_NHWC, qbits=qbits, mfma_passes=lib.MFMA_F16X1, reserved=0)
        self.d1 = lib.ConvDesc(n=B, c_in=C, h=H, w=W, c_out=C, kh=3, kw=3, stride_h=S, stride_w=S, pad_h=pad, pad_w=pad, groups=C,
                               ka=float(np.float32(KA_DW)), kw_scale=float(np.float32(KW_DW)), **common)
        self.d2 = lib.ConvDesc(n=B, c_in=C, h=self.Ho, w=self.Wo, c_out=N, kh=1, kw=1, stride_h=1, stride_w=1, pad_h=0, pad_w=0, groups=1,
                               ka=float(np.float32(KA_PW)), kw_scale=float(np.float32(KW_PW)), **common)
        self.w1 = torch.randn((C, 1, 3, 3), generator=gen, device=dev) * (4.0 * KW_DW)
        self.w2 = torch.randn((N, C, 1, 1), generator=gen, device=dev) * min(5.0 * KW_PW, 3.0 * (2.0 / C) ** 0.5 + 2.0 * KW_PW)
        self.blob1, self.blob2 = (self._prep(d, w) for d, w in ((self.d1, self.w1), (self.d2, self.w2)))
        self.sc1 = torch.rand(C, generator=gen, device=dev) + 0.5
        self.sh1 = torch.randn(C, generator=gen, device=dev) * 0.3 - shift_by
        self.sc2 = torch.rand(N, generator=gen, device=dev) + 0.5
        self.sh2 = torch.randn(N, generator=gen, device=dev) * 0.3 - shift_by
        self.bias2 = torch.randn(N, generator=gen, device=dev) * 0.2 if bias else None
        assert L.slfp_conv2d_kernel_name(ctypes.byref(self.d1)).decode() == "dw3x3_nhwc"
        assert L.slfp_conv2d_kernel_name(ctypes.byref(self.d2)).decode().startswith("pw_mfma_f16")

    def _prep(self, d, w):
        L = self.lib.load()
        blob = torch.empty(L.slfp_conv2d_wprep_bytes(ctypes.byref(d)), dtype=torch.uint8, device=w.device)
        self.lib.check(L.slfp_conv2d_prepare_weights(ctypes.byref(d), w.data_ptr(), blob.data_ptr(), None, _stream()))
        return blob

    def input(self, gen, signed, zero=False):
        """codes of the depthwise layer's own quantizer, from a tensor that spans all binades, both clamps, the tiny class and zeros"""
        dev = self.w1.device
        x = torch.randn((self.B, self.H, self.W, self.C), generator=gen, device=dev)
        x = (x if signed else torch.relu(x)) * (6.0 * KA_DW)
        x.view(-1)[::97] = 17.0 * KA_DW          # beyond the clamp
        x.view(-1)[5::193] = 0.05 * KA_DW        # the "tiny" class
        if zero:
            x.zero_()
        self.x_f32 = x   # the float32 tensor the codes stand for: quantized with Ka_dw it gives the decoded values (checked below)
        return _encode(self.lib, x, KA_DW, self.qbits)

    def _io(self, out):
        """out: None (float32) or the reader's q_bit"""
        return self.lib.ConvIo(x_codes=1, y_codes=0 if out is None else 1, y_ka=float(np.float32(KA_NEXT)) if out is not None else 1.0,
                               y_qbits=out if out is not None else 8)

    def _y(self, out):
        return torch.empty((self.B, self.Ho, self.Wo, self.N), dtype=torch.float32 if out is None else torch.uint8, device=self.w1.device)

    def two_kernels(self, xc, relu1, relu2, out):
        """today's chain: k_dwc writes the pointwise layer's codes, k_pwc_* reads them.  Returns (intermediate codes, y)."""
        lib, L = self.lib, self.lib.load()
        io1 = lib.ConvIo(x_codes=1, y_codes=1, y_ka=float(np.float32(KA_PW)), y_qbits=self.qbits)
        io2 = self._io(out)
        assert L.slfp_conv2d_codes_supported(ctypes.byref(self.d1), ctypes.byref(io1), 0, relu1) == 1
        assert L.slfp_conv2d_codes_supported(ctypes.byref(self.d2), ctypes.byref(io2), 1 if self.bias2 is not None else 0, relu2) == 1
        mid = torch.empty((self.B, self.Ho, self.Wo, self.C), dtype=torch.uint8, device=xc.device)
        y = self._y(out)
        lib.check(L.slfp_conv2d_fwd_codes_ws(ctypes.byref(self.d1), ctypes.byref(io1), xc.data_ptr(), self.blob1.data_ptr(), None,
                                             self.sc1.data_ptr(), self.sh1.data_ptr(), relu1, mid.data_ptr(), None, _stream()))
        lib.check(L.slfp_conv2d_fwd_codes_ws(ctypes.byref(self.d2), ctypes.byref(io2), mid.data_ptr(), self.blob2.data_ptr(), _ptr(self.bias2),
                                             self.sc2.data_ptr(), self.sh2.data_ptr(), relu2, y.data_ptr(), None, _stream()))
        return mid, y

    def one_kernel(self, xc, relu1, relu2, out):
        lib, L = self.lib, self.lib.load()
        io = self._io(out)
        assert L.slfp_dwpw_codes_supported(ctypes.byref(self.d1), ctypes.byref(self.d2), ctypes.byref(io),
                                           1 if self.bias2 is not None else 0, relu1, relu2) == 1
        y = self._y(out)
        rc = L.slfp_dwpw_fwd_codes(ctypes.byref(self.d1), ctypes.byref(self.d2), ctypes.byref(io), xc.data_ptr(), self.blob1.data_ptr(),
                                   self.sc1.data_ptr(), self.sh1.data_ptr(), relu1, self.blob2.data_ptr(), _ptr(self.bias2),
                                   self.sc2.data_ptr(), self.sh2.data_ptr(), relu2, y.data_ptr(), _stream())
        assert rc == lib.OK, (rc, lib.last_error())
        return y

    def one_kernel_f32(self, x, xc, relu1, relu2):
        """the float32 interface's one-kernel form (slfp_dwpw_fwd) on the float32 input whose quantizer output is the decoded codes"""
        lib, L = self.lib, self.lib.load()
        xq = torch.empty_like(x)
        lib.check(L.slfp_quantize_f32(x.data_ptr(), xq.data_ptr(), x.numel(), float(np.float32(KA_DW)), _fmt(lib, self.qbits), _stream()))
        assert _same(xq, _decode(lib, xc, self.qbits))
        assert L.slfp_dwpw_supported(ctypes.byref(self.d1), ctypes.byref(self.d2)) == 1
        y = self._y(None)
        lib.check(L.slfp_dwpw_fwd(ctypes.byref(self.d1), ctypes.byref(self.d2), x.data_ptr(), self.blob1.data_ptr(), self.sc1.data_ptr(),
                                  self.sh1.data_ptr(), relu1, self.blob2.data_ptr(), _ptr(self.bias2), self.sc2.data_ptr(),
                                  self.sh2.data_ptr(), relu2, y.data_ptr(), _stream()))
        return y


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


#         C    N  stride H   W  batch
CASES = [(32, 64, 1, 28, 28, 3), (64, 128, 2, 30, 30, 2), (128, 128, 1, 14, 14, 2), (128, 256, 2, 28, 28, 2), (32, 64, 1, 33, 33, 2),
         (64, 64, 2, 15, 15, 1), (32, 64, 1, 20, 33, 2), (32, 64, 1, 33, 20, 2), (64, 128, 2, 20, 33, 2), (64, 128, 2, 33, 20, 2)]
F32_FORM = {(32, 64, 1, 28, 28, 3), (64, 128, 2, 30, 30, 2)}   # one case per stride: also against slfp_dwpw_fwd
BIAS_CASE = (128, 128, 1, 14, 14, 2)


@pytest.mark.parametrize("qbits", [8, 7])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%d-%d-s%d-%dx%d-b%d" % c)
def test_one_kernel_equals_the_two_code_kernels(lib, dev, case, qbits):
    """Every (stride, K) shape, ragged tiles in both directions, tiles_h != tiles_w; ReLUs on, and both off with the shifts lowered so
    that the intermediate and the output carry signs; float32 out and codes for a q_bit 8 and a q_bit 7 reader."""
    C, N, S, H, W, B = case
    gen = torch.Generator(device=dev).manual_seed(C * 1000 + N + 7 * S + H + 3 * W + qbits)
    for relu in (1, 0):
        blk = _Block(lib, dev, gen, C, N, S, H, W, B, qbits, bias=case == BIAS_CASE, shift_by=0.0 if relu else 0.6)
        xc = blk.input(gen, signed=not relu)
        for out in (None, 8, 7):
            mid, want = blk.two_kernels(xc, relu, relu, out)
            got = blk.one_kernel(xc, relu, relu, out)
            torch.cuda.synchronize()
            assert _same(got, want), (case, qbits, relu, out, int((got != want).sum()))
            if out is None and not relu:
                neg_mid = float((_decode(lib, mid, qbits) < 0).float().mean())
                neg_out = float((want < 0).float().mean())
                print("negative share: intermediate %.3f, output %.3f" % (neg_mid, neg_out))
                assert neg_mid > 0.05 and neg_out > 0.05, (neg_mid, neg_out)
            if out is None and relu:
                assert float((want > 0).float().mean()) > 0.05 and float((_decode(lib, mid, qbits) > 0).float().mean()) > 0.05
        if case in F32_FORM:
            # the float32 interface's one-kernel form on the input behind the codes: equal float32; its slfp_encode_f32 = the code output
            y32 = blk.one_kernel_f32(blk.x_f32, xc, relu, relu)
            assert _same(y32, blk.one_kernel(xc, relu, relu, None)), (case, qbits, relu)
            for out in (8, 7):
                assert _same(_encode(lib, y32, KA_NEXT, out), blk.one_kernel(xc, relu, relu, out)), (case, qbits, relu, out)


@pytest.mark.parametrize("qbits", [8, 7])
def test_zero_image_and_no_padding(lib, dev, qbits):
    """An all-zero image puts padding and data on the same code (0x01); pad = 0 has no out-of-image tap at the top / left and ragged
    tiles at the bottom / right."""
    gen = torch.Generator(device=dev).manual_seed(99 + qbits)
    for (C, N, S, H, W, B, pad, zero) in ((32, 64, 1, 28, 28, 2, 1, True), (64, 128, 2, 30, 30, 2, 1, True),
                                          (32, 64, 1, 28, 28, 2, 0, False), (64, 128, 2, 30, 30, 2, 0, False), (128, 256, 2, 29, 17, 1, 0, False)):
        blk = _Block(lib, dev, gen, C, N, S, H, W, B, qbits, pad=pad)
        xc = blk.input(gen, signed=False, zero=zero)
        if zero:
            assert bool((xc == 1).all())
        for out in (None, 8):
            _, want = blk.two_kernels(xc, 1, 1, out)
            got = blk.one_kernel(xc, 1, 1, out)
            assert _same(got, want), (C, N, S, pad, zero, out)
            assert _same(blk.one_kernel(xc, 1, 1, out), got)   # run twice: the same bytes


# ---------------------------------------------------------------------------------------------------------------- module level
def _net(q_bit, dev):
    """A 3 -> 32 stride-2 stem and MobileNetV1's first four blocks, each conv with BatchNorm and ReLU."""
    from cnns_slfp_quantization_amd import conv2d_func as cf
    layers = []

    def add(conv, c_out):
        layers.extend([conv, nn.BatchNorm2d(c_out), nn.ReLU(inplace=True)])

    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1234 + q_bit)
        add(cf.conv2d_Q(q_bit, 0.03, 0.2)(3, 32, 3, stride=2, padding=1, bias=False), 32)
        for c, s, n in ((32, 1, 64), (64, 2, 128), (128, 1, 128), (128, 2, 256)):
            add(cf.conv2d_Q(q_bit, 0.06, 0.2)(c, c, 3, stride=s, padding=1, groups=c, bias=False), c)
            add(cf.conv2d_Q(q_bit, 0.02, 0.25)(c, n, 1, bias=False), n)
        m = nn.Sequential(*layers)
        g = torch.Generator().manual_seed(77)
        with torch.no_grad():
            for bn in [b for b in m if isinstance(b, nn.BatchNorm2d)]:
                bn.running_mean.normal_(0.0, 0.2, generator=g)
                bn.running_var.uniform_(0.5, 1.5, generator=g)
                bn.weight.uniform_(0.8, 1.6, generator=g)
                bn.bias.normal_(0.1, 0.2, generator=g)
            for conv in [c for c in m if isinstance(c, nn.Conv2d) and c.groups > 1]:
                conv.weight.mul_(3.0)
        x = torch.randn((2, 3, 64, 64), generator=g)
    return m.to(dev).eval().to(memory_format=torch.channels_last), x.to(dev).contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("q_bit", [8, 7])
def test_linked_blocks_run_as_one_kernel_each(dev, q_bit):
    """fuse_bn_relu -> link_codes(model, x) -> fuse_dw_pw: under options.dwpw_all every block is ONE launch that reads and writes codes;
    under the default options it is the two code kernels; the bits never change; every pass undoes."""
    from cnns_slfp_quantization_amd import conv2d_func as cf, fusion
    m, x = _net(q_bit, dev)
    fused = "dwpw_fused_f16x1" if q_bit == 8 else "dwpw_fused_f16_exact"
    assert cf.options.dwpw_all is False and len(cf.options.dwpw_codes_pairs) == 0
    try:
        with torch.no_grad():
            assert fusion.fuse_bn_relu(m) == 9
            y_fused = m(x).clone()
            assert fusion.link_codes(m, x) == 8            # stem -> dw1 -> pw1 -> ... -> pw4
            y_linked = m(x).clone()
            assert y_linked.dtype == torch.float32 and torch.equal(y_linked, y_fused)
            convs = [c for c in m if isinstance(c, nn.Conv2d)]
            dws, pws = convs[1::2], convs[2::2]
            # the reference pair runs the code kernels
            assert all(c._last_kernel == "dw3x3_nhwc+codes_in+codes_out" for c in dws), [c._last_kernel for c in dws]
            assert all(c._last_kernel.startswith("pw_mfma_f16") and "+codes_in" in c._last_kernel for c in pws), [c._last_kernel for c in pws]
            assert all(c._last_kernel.endswith("+codes_out") for c in pws[:3]) and not pws[3]._last_kernel.endswith("+codes_out")

            cf.options.dwpw_all = True
            assert fusion.fuse_dw_pw(m) == 4
            blocks = [b for b in m if isinstance(b, fusion.DwPwBlock)]
            seen = []
            hooks = [b.register_forward_hook(lambda mod, inp, out: seen.append((inp[0].dtype, out.dtype, out.clone()))) for b in blocks]
            y_one = m(x).clone()
            assert torch.equal(y_one.view(torch.int32), y_linked.view(torch.int32))
            assert [b._last_kernel for b in blocks] == [fused + "+codes_in+codes_out"] * 3 + [fused + "+codes_in"]
            assert [(a, b) for a, b, _ in seen] == [(torch.uint8, torch.uint8)] * 3 + [(torch.uint8, torch.float32)]
            assert all(b.dw._last_codes is not None and b.dw._last_input is None and b.pw._last_codes is None for b in blocks)
            first = [t for _, _, t in seen]
            del seen[:]
            assert torch.equal(m(x), y_one)                  # determinism: the same bytes, block by block
            assert all(torch.equal(a, b) for a, (_, _, b) in zip(first, seen))

            cf.options.dwpw_all = False                     # the default options: two code kernels per block, the same bits
            del seen[:]
            assert torch.equal(m(x), y_one)
            assert all(b._last_kernel is None for b in blocks)
            assert all(b.dw._last_kernel == "dw3x3_nhwc+codes_in+codes_out" for b in blocks)
            assert all(torch.equal(a, b) for a, (_, _, b) in zip(first, seen))
            cf.options.dwpw_codes_pairs = {(64, 2)}          # one pair by the option
            assert torch.equal(m(x), y_one)
            assert [b._last_kernel is not None for b in blocks] == [False, True, False, False]
            cf.options.dwpw_codes_pairs = set()
            for h in hooks:
                h.remove()

            cf.options.dwpw_all = True
            assert fusion.unlink_codes(m) == 8               # reaches blk.dw / blk.pw: the blocks take float32 again
            y_unlinked = m(x)
            assert [b._last_kernel for b in blocks] == [fused] * 4
            assert torch.equal(y_unlinked, y_fused)
            assert fusion.unfuse_dw_pw(m) == 4
            assert [c for c in m if isinstance(c, nn.Conv2d)] == convs and not any(isinstance(b, fusion.DwPwBlock) for b in m)
            assert torch.equal(m(x), y_fused)
    finally:
        cf.options.dwpw_all = False
        cf.options.dwpw_codes_pairs = set()
