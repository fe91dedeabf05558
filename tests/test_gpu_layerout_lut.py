"""MI355X: the table epilogue behind the layer-output quantizer (slfp_conv2d_fwd_codes_lut).  For every
kernel family with a table form, the bytes it writes equal the reference composition
    slfp_conv2d_fwd_post(relu = SLFP_POST_LAYEROUT)  ->  the activation in torch  ->  slfp_encode_f32(., Ka, fmt | SLFP_FMT_EXT)
bit for bit, for the reader's q_bit 8 and 7 and five activations, one of them not monotone.  Where the layer reads codes, the
reference reads the float32 tensor x whose codes they are: slfp_decode_f32 gives QA(x / Ka), the value in the quantizer's domain,
which is what the float32 interface computes from x itself (tests/test_gpu_codes.py compares the two interfaces the same way).  The table is built here, from slfp_layerout_lut_values, not by fusion.  The float32 reference of a case is computed
once and shared by its activations and formats."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
LAYEROUT = 2   # SLFP_POST_LAYEROUT


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
    x = x.contiguous()
    c = torch.empty_like(x, dtype=torch.uint8)
    lib.check(lib.load().slfp_encode_f32(x.data_ptr(), c.data_ptr(), x.numel(), float(np.float32(ka)), _fmt(lib, qbits) | lib.FMT_EXT, _stream()))
    return c


class CosGate(nn.Module):
    """x * cos(3 x): elementwise and far from monotone"""

    def forward(self, x):
        return x * torch.cos(3.0 * x)


class Swish(nn.Module):
    def forward(self, x):
        return x * torch.sigmoid(x)


class KernelReLU(nn.Module):
    """the ReLU folded into the epilogue, as the kernels compute it: fmaxf(NaN, 0) is 0"""

    def forward(self, x):
        return torch.where(x > 0, x, torch.zeros_like(x))


ACTS = [("none", nn.Identity()), ("relu", KernelReLU()), ("swish", Swish()), ("gelu", nn.GELU()), ("xcos3x", CosGate())]


@pytest.fixture(scope="module")
def lut_values(lib, dev):
    n = lib.LAYEROUT_LUT_BYTES
    v = np.zeros(n, dtype=np.float32)
    lib.check(lib.load().slfp_layerout_lut_values(v.ctypes.data, n))
    assert n % 16 == 0 and lib.load().slfp_layerout_lut_classes() <= n
    return torch.from_numpy(v).to(dev)


def _table(lib, lut_values, act, y_ka, y_qbits):
    with torch.no_grad():
        t = _encode(lib, act(lut_values.clone()), y_ka, y_qbits)
    assert t.data_ptr() % 16 == 0 and t.numel() == lib.LAYEROUT_LUT_BYTES
    return t


class _Layer:
    """One Conv2d_Q layer on NHWC tensors with random weights and a BN-like affine whose shift is 0 on every fourth channel."""

    def __init__(self, lib, dev, gen, n, c_in, c_out, h, w, k, stride, groups, x_codes, qbits=8, ka=0.31, kw=0.02):
        L = lib.load()
        self.lib, self.n, self.c_in, self.c_out, self.h, self.wd, self.qbits, self.ka, self.x_codes = lib, n, c_in, c_out, h, w, qbits, ka, x_codes
        self.d = lib.ConvDesc(n=n, c_in=c_in, h=h, w=w, c_out=c_out, kh=k, kw=k, stride_h=stride, stride_w=stride, pad_h=k // 2, pad_w=k // 2,
                              dil_h=1, dil_w=1, groups=groups, x_layout=lib.LAYOUT_NHWC, y_layout=lib.LAYOUT_NHWC, qbits=qbits,
                              ka=float(np.float32(ka)), kw_scale=float(np.float32(kw)), mfma_passes=lib.MFMA_F16X1, reserved=0)
        ho, wo = ctypes.c_int64(), ctypes.c_int64()
        lib.check(L.slfp_conv2d_out_shape(ctypes.byref(self.d), ctypes.byref(ho), ctypes.byref(wo)))
        self.ho, self.wo = ho.value, wo.value
        fan = (c_in // groups) * k * k
        self.w = (torch.randn((c_out, c_in // groups, k, k), generator=gen) * min(5.0 * kw, 3.0 * (2.0 / fan) ** 0.5 + 2.0 * kw)).to(dev)
        # scales of both signs over several binades: the outputs reach from denormal-free tiny values to the 248 clamp
        ps = (0.5 + torch.rand(c_out, generator=gen)) * torch.pow(2.0, (torch.arange(c_out) % 7).float() - 1.0)
        ps[1::2] *= -1.0
        psh = torch.randn(c_out, generator=gen) * 0.3
        psh[::4] = 0.0
        self.ps, self.psh = ps.to(dev), psh.to(dev)
        self.blob = torch.empty(L.slfp_conv2d_wprep_bytes(ctypes.byref(self.d)), dtype=torch.uint8, device=dev)
        lib.check(L.slfp_conv2d_prepare_weights(ctypes.byref(self.d), self.w.data_ptr(), self.blob.data_ptr(), None, _stream()))
        ws_n = L.slfp_conv2d_workspace_bytes(ctypes.byref(self.d))
        self.ws = torch.empty(ws_n, dtype=torch.uint8, device=dev) if ws_n else None
        self.kernel = L.slfp_conv2d_kernel_name(ctypes.byref(self.d)).decode()
        # the input: image 0 random over six binades, image 1 all zero (exact zero -> NaN behind the quantizer where shift is 0)
        x = torch.randn((n, h, w, c_in), generator=gen) * (4.0 * ka)
        px = x.view(-1, c_in)
        px *= torch.pow(2.0, -(torch.arange(px.shape[0]) % 6).float()).unsqueeze(1)
        x[1] = 0.0
        x = x.to(dev)
        self.x_f32 = x
        self.x = _encode(lib, x, ka, qbits) if x_codes else x

    def reference_f32(self):
        """slfp_conv2d_fwd_post(relu = SLFP_POST_LAYEROUT) on the float32 input (whose codes a code-reading layer is given)"""
        y = torch.empty((self.n, self.ho, self.wo, self.c_out), device=self.x.device)
        self.lib.check(self.lib.load().slfp_conv2d_fwd_post(ctypes.byref(self.d), self.x_f32.data_ptr(), self.blob.data_ptr(), None,
                                                            self.ps.data_ptr(), self.psh.data_ptr(), LAYEROUT, y.data_ptr(), None,
                                                            self.ws.data_ptr() if self.ws is not None else None, _stream()))
        return y

    def io(self, y_ka, y_qbits):
        return self.lib.ConvIo(x_codes=1 if self.x_codes else 0, y_codes=1, y_ka=float(np.float32(y_ka)), y_qbits=y_qbits)

    def supported(self, y_ka, y_qbits, y_ld):
        io = self.io(y_ka, y_qbits)
        return self.lib.load().slfp_conv2d_codes_lut_supported(ctypes.byref(self.d), ctypes.byref(io), 0, y_ld) == 1

    def fwd_lut(self, table, y_ka, y_qbits, y_ptr, y_ld):
        io = self.io(y_ka, y_qbits)
        self.lib.check(self.lib.load().slfp_conv2d_fwd_codes_lut(ctypes.byref(self.d), ctypes.byref(io), self.x.data_ptr(), self.blob.data_ptr(), None,
                                                                 self.ps.data_ptr(), self.psh.data_ptr(), table.data_ptr(), y_ptr, y_ld,
                                                                 self.ws.data_ptr() if self.ws is not None else None, _stream()))


def _check_case(lib, dev, lut_values, lay, slice_ld=None):
    ref = lay.reference_f32()
    fin = ref[torch.isfinite(ref)].abs()
    assert fin.numel() > 0
    assert bool(torch.isnan(ref[1, :, :, ::4]).all()), "the zero image with shift 0 must give NaN behind the quantizer"
    assert float(fin.max()) <= 248.0
    # the reader's scale: the 90th percentile of |ref| sits at 12 Ka, so the top classes and the clamp are reached
    y_ka = float(np.float32(max(float(torch.quantile(fin.flatten().float()[:1 << 20], 0.9)) / 12.0, 1e-3)))
    c_out, npix = lay.c_out, lay.n * lay.ho * lay.wo
    ld = slice_ld or c_out
    for y_qbits in (8, 7):
        assert lay.supported(y_ka, y_qbits, ld), (lay.kernel, y_qbits, ld)
        for name, act in ACTS:
            with torch.no_grad():
                want = _encode(lib, act(ref.clone()), y_ka, y_qbits).view(npix, c_out)
            table = _table(lib, lut_values, act, y_ka, y_qbits)
            buf = torch.full((npix, ld), 0xA5, dtype=torch.uint8, device=dev)
            off = (ld - c_out) if slice_ld else 0          # the slice is the tensor's LAST c_out channels
            assert (buf.data_ptr() + off) % 16 == 0
            lay.fwd_lut(table, y_ka, y_qbits, buf.data_ptr() + off, ld)
            got = buf[:, off:off + c_out]
            bad = int((got != want).sum())
            assert bad == 0, (lay.kernel, name, y_qbits, bad, got.numel())
            if slice_ld:
                assert bool((buf[:, :off] == 0xA5).all()), "bytes outside the slice were written"
            z = got.view(lay.n, lay.ho, lay.wo, c_out)[1, :, :, ::4]
            if name == "none":
                assert bool((z == 0x00).all())            # NaN has no code
            if name == "relu":
                assert bool((z == 0x01).all())            # fmaxf(NaN, 0) = 0: the code of exact zero
        if want.numel() >= 2048:
            assert len(torch.unique(want)) > 8             # the last activation's reference spans many classes
    torch.cuda.synchronize()


def test_layerout_class_sweep_over_all_float32(lib, dev):
    out = torch.full((1,), 7, dtype=torch.int64, device=dev)
    lib.check(lib.load().slfp_debug_layerout_lut_mismatches(out.data_ptr(), _stream()))
    assert int(out.item()) == 0


DW = [(c, s, h, w) for c in (32, 64) for s in (1, 2) for (h, w) in ((1, 1), (2, 2), (5, 7))]


@pytest.mark.parametrize("c,s,h,w", DW, ids=["c%d-s%d-%dx%d" % r for r in DW])
def test_depthwise_on_codes(lib, dev, lut_values, c, s, h, w):
    gen = torch.Generator().manual_seed(100 * c + 10 * s + h)
    lay = _Layer(lib, dev, gen, 2, c, c, h, w, 3, s, c, True, kw=0.08)
    assert lay.kernel == "dw3x3_nhwc"
    _check_case(lib, dev, lut_values, lay)


# K, N, h, w, slice pixel stride, the kernel slfp_debug_pw_variant must name
PW = [(32, 64, 1, 1, None, "pwc-stream"), (32, 64, 3, 5, None, "pwc-stream"), (64, 32, 1, 1, None, "pwc-stream"), (64, 32, 3, 5, 64, "pwc-stream"),
      (256, 256, 1, 1, None, "slice"), (256, 256, 3, 5, None, "slice"), (512, 512, 1, 1, None, "pwc-tiled"), (512, 512, 3, 5, None, "pwc-tiled"),
      (1024, 1024, 1, 1, None, "pwc-tiled"), (1024, 1024, 3, 5, None, "pwc-tiled")]


@pytest.mark.parametrize("k,n,h,w,ld,kern", PW, ids=["%d-%d-%dx%d-ld%s-%s" % r for r in PW])
def test_pointwise_on_codes(lib, dev, lut_values, k, n, h, w, ld, kern):
    gen = torch.Generator().manual_seed(k + n + h)
    lay = _Layer(lib, dev, gen, 2, k, n, h, w, 1, 1, 1, True)
    io = lay.io(0.3, 8)
    assert lib.load().slfp_debug_pw_variant(ctypes.byref(lay.d), ctypes.byref(io), 0, 0, 0).decode().startswith(kern + "/")
    _check_case(lib, dev, lut_values, lay, slice_ld=ld)


DENSE = [(64, 64, 2, 2, 0, None), (64, 64, 2, 2, 1, None), (64, 64, 5, 7, 0, None), (64, 64, 5, 7, 1, 128),
         (128, 256, 2, 2, 0, None), (128, 256, 2, 2, 1, None), (128, 256, 5, 7, 0, None), (128, 256, 5, 7, 1, None)]


@pytest.mark.parametrize("c_in,c_out,h,w,xc,ld", DENSE, ids=["%d-%d-%dx%d-x%d-ld%s" % r for r in DENSE])
def test_dense_3x3(lib, dev, lut_values, c_in, c_out, h, w, xc, ld):
    gen = torch.Generator().manual_seed(c_in + c_out + h + xc)
    lay = _Layer(lib, dev, gen, 2, c_in, c_out, h, w, 3, 1, 1, bool(xc))
    assert lay.kernel.startswith("dense_mfma"), lay.kernel
    _check_case(lib, dev, lut_values, lay, slice_ld=ld)


STEMS = [(32, 2, 6, 10), (64, 1, 6, 10), (32, 2, 8, 12)]   # 8 x 12: image rows of whole 16-byte pieces, the float32 matrix-core stem


@pytest.mark.parametrize("c_out,s,h,w", STEMS, ids=["3-%d-s%d-%dx%d" % r for r in STEMS])
def test_rgb_stems(lib, dev, lut_values, c_out, s, h, w):
    gen = torch.Generator().manual_seed(c_out + h)
    lay = _Layer(lib, dev, gen, 2, 3, c_out, h, w, 3, s, 1, False, ka=0.17, kw=0.06)
    assert lay.kernel in ("stem_nhwc", "stem_small_mfma_f16x1"), lay.kernel
    _check_case(lib, dev, lut_values, lay)
