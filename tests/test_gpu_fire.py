"""GPU (MI355X): SqueezeNet's Fire module on 1-byte codes without the concat.

  * 1x1 layers on codes with 16 and 48 input channels (k_pwc_stream, HALF form): bit-identical to the float32 interface;
  * the code output of the pw_mfma_* code kernels and of the dense k x k epilogue into a channel slice of a wider tensor
    (slfp_conv2d_fwd_codes_slice): the slice holds exactly the bytes slfp_conv2d_fwd_codes_ws writes, nothing else is touched;
  * nn.MaxPool2d(ceil_mode=True) on codes (slfp_maxpool2d_codes_ex);
  * one Fire against the CPU oracle;
  * fusion.fuse_fire on the committed SqueezeNet fixture net: bit-identical logits, no torch.cat, no in-place ReLU passes.
Every comparison is torch.equal unless stated."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_errors
from oracle import slfp_oracle as so

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
R3_SQUEEZENET_BARS = (3e-2, 2e-2)   # logits (max, l2): tests/test_gpu_parity.py R3_BARS["squeezenet"][1]
TOL_SFP7 = 1e-5                      # tests/_bars.py TOL_EXACT: the family bar of the SFP<3,3> kernels


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
    """elementwise in memory order (keeps the strides of a dense tensor)"""
    c = torch.empty_like(x, dtype=torch.uint8)
    lib.check(lib.load().slfp_encode_f32(x.data_ptr(), c.data_ptr(), x.numel(), float(np.float32(ka)), _fmt(lib, qbits) | lib.FMT_EXT, _stream()))
    return c


class _Layer:
    """One Conv2d_Q layer (NHWC tensors, logical sizes n x c_in x h x w; w defaults to h) with random weights and bias."""

    def __init__(self, lib, dev, gen, n, c_in, c_out, h, k, qbits, relu, ka=0.31, kw=0.02, bias=True, w=None):
        L = lib.load()
        self.lib, self.n, self.c_in, self.c_out, self.h, self.k, self.qbits, self.relu, self.ka = lib, n, c_in, c_out, h, k, qbits, relu, ka
        self.wd = h if w is None else w   # the input's width (self.w is the weight tensor)
        self.d = lib.ConvDesc(n=n, c_in=c_in, h=h, w=self.wd, c_out=c_out, kh=k, kw=k, stride_h=1, stride_w=1, pad_h=k // 2, pad_w=k // 2,
                              dil_h=1, dil_w=1, groups=1, x_layout=lib.LAYOUT_NHWC, y_layout=lib.LAYOUT_NHWC, qbits=qbits,
                              ka=float(np.float32(ka)), kw_scale=float(np.float32(kw)), mfma_passes=lib.MFMA_F16X1, reserved=0)
        fan = c_in * k * k
        self.w = torch.randn((c_out, c_in, k, k), generator=gen, device=dev) * min(5.0 * kw, 3.0 * (2.0 / fan) ** 0.5 + 2.0 * kw)
        self.b = (torch.randn(c_out, generator=gen, device=dev) * 0.2) if bias else None
        self.blob = torch.empty(L.slfp_conv2d_wprep_bytes(ctypes.byref(self.d)), dtype=torch.uint8, device=dev)
        lib.check(L.slfp_conv2d_prepare_weights(ctypes.byref(self.d), self.w.data_ptr(), self.blob.data_ptr(), None, _stream()))
        ws_n = L.slfp_conv2d_workspace_bytes(ctypes.byref(self.d))
        self.ws = torch.empty(ws_n, dtype=torch.uint8, device=dev) if ws_n else None
        self.kernel = L.slfp_conv2d_kernel_name(ctypes.byref(self.d)).decode()

    def _p(self, t):
        return t.data_ptr() if t is not None else None

    def out_shape(self, c=None):
        return (self.n, self.h, self.wd, self.c_out if c is None else c)

    def io(self, x_codes, y_ka, y_qbits=None):
        return self.lib.ConvIo(x_codes=1 if x_codes else 0, y_codes=0 if y_ka is None else 1,
                               y_ka=float(np.float32(y_ka if y_ka is not None else 1.0)), y_qbits=y_qbits or self.qbits)

    def fwd_f32(self, x):
        """the float32 interface: slfp_conv2d_fwd_post"""
        y = torch.empty(self.out_shape(), device=x.device)
        self.lib.check(self.lib.load().slfp_conv2d_fwd_post(ctypes.byref(self.d), x.data_ptr(), self.blob.data_ptr(), self._p(self.b), None, None,
                                                            1 if self.relu else 0, y.data_ptr(), None, self._p(self.ws), _stream()))
        return y

    def fwd_codes(self, x, x_codes, y_ka=None):
        """slfp_conv2d_fwd_codes_ws: y_ka None -> float32 out, else the consumer's codes"""
        L = self.lib.load()
        io = self.io(x_codes, y_ka)
        assert L.slfp_conv2d_codes_supported(ctypes.byref(self.d), ctypes.byref(io), 1 if self.b is not None else 0, 1 if self.relu else 0) == 1, \
            (self.kernel, self.c_in, self.c_out, x_codes, y_ka)
        y = torch.empty(self.out_shape(), dtype=torch.float32 if y_ka is None else torch.uint8, device=x.device)
        self.lib.check(L.slfp_conv2d_fwd_codes_ws(ctypes.byref(self.d), ctypes.byref(io), x.data_ptr(), self.blob.data_ptr(), self._p(self.b),
                                                  None, None, 1 if self.relu else 0, y.data_ptr(), self._p(self.ws), _stream()))
        return y

    def fwd_slice(self, x, x_codes, y_ka, buf, c_off):
        """slfp_conv2d_fwd_codes_slice into channels c_off.. of the NHWC code tensor `buf`"""
        L = self.lib.load()
        io = self.io(x_codes, y_ka)
        ld = buf.shape[-1]
        assert buf.is_contiguous() and buf.shape[:3] == self.out_shape()[:3] and c_off + self.c_out <= ld   # the store stays inside `buf`
        assert L.slfp_conv2d_codes_slice_supported(ctypes.byref(self.d), ctypes.byref(io), 1 if self.b is not None else 0,
                                                   1 if self.relu else 0, ld) == 1, (self.kernel, self.c_in, self.c_out, ld)
        self.lib.check(L.slfp_conv2d_fwd_codes_slice(ctypes.byref(self.d), ctypes.byref(io), x.data_ptr(), self.blob.data_ptr(), self._p(self.b),
                                                     None, None, 1 if self.relu else 0, buf.data_ptr() + c_off, ld, self._p(self.ws), _stream()))
        return buf


def _synthetic(shape, ka, dev, gen, signed=False):
    """post-ReLU-like activations spanning all binades and both clamps, with exact zeros"""
    x = torch.randn(shape, generator=gen, device=dev)
    if not signed:
        x = torch.relu(x)
    x = x * (6.0 * ka)
    x.view(-1)[::97] = 17.0 * ka          # beyond the clamp
    x.view(-1)[5::193] = 0.05 * ka        # the "tiny" class
    return x


def _at_the_end_of_an_allocation(codes):
    """A copy of the code tensor whose last byte is the last byte of a device allocation of its own: the caching allocator's free
    blocks are released first, so the 32 MiB request (a whole number of 2 MiB pages, above the size up to which the allocator
    rounds large requests up or carves them out of a bigger block) goes to the device as it is.  Nothing the kernel may read
    lies behind the last pixel."""
    n = codes.numel()
    assert n % 16 == 0
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    big = torch.empty(32 << 20, dtype=torch.uint8, device=codes.device)
    tail = big[big.numel() - n:]
    assert tail.data_ptr() % 16 == 0 and tail.data_ptr() + n == big.data_ptr() + big.numel()
    tail.copy_(codes.reshape(-1))
    return tail.view(codes.shape), big


# ---------------------------------------------------------------------------------------------- pointwise K = 16 / 48
@pytest.mark.parametrize("qbits", [7, 8])
@pytest.mark.parametrize("geom", [(16, 64, 54), (48, 192, 27)])
def test_pointwise_16_and_48_channels_on_codes_equal_the_float32_interface(lib, dev, qbits, geom):
    """The expand1x1 layers behind a 16- / 48-channel squeeze: the last 32-deep k-step is half live.  Float32 output == the float32
    interface's (k_pw_stream), code output == slfp_encode_f32 of it; batches with M % 16 != 0 (1, 3) and == 0 (16); the codes sit at
    the very end of their allocation."""
    c_in, c_out, h = geom
    gen = torch.Generator(device=dev).manual_seed(1000 * qbits + c_in)
    y_ka = 0.27
    for n in (3, 1, 16):
        assert ((n * h * h) % 16 == 0) == (n == 16)
        for relu in (True, False):
            lay = _Layer(lib, dev, gen, n, c_in, c_out, h, 1, qbits, relu)
            assert lay.kernel.startswith("pw_mfma")
            x = _synthetic((n, h, h, c_in), lay.ka, dev, gen, signed=not relu)
            xc, keep = _at_the_end_of_an_allocation(_encode(lib, x, lay.ka, qbits))
            want = lay.fwd_f32(x)
            got = lay.fwd_codes(xc, True)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (geom, qbits, n, relu, float((got - want).abs().max()))
            gotc = lay.fwd_codes(xc, True, y_ka)
            wantc = _encode(lib, want, y_ka, qbits)
            assert torch.equal(gotc, wantc), (geom, qbits, n, relu, int((gotc != wantc).sum()))
            torch.cuda.synchronize()
            del keep


def test_the_96_channel_squeeze_behind_the_stem_runs_on_codes(lib, dev):
    """96 -> 16 @ 54 (three whole k-steps of the stream kernel): the first Fire's squeeze, fed by one slfp_encode_f32 pass."""
    gen = torch.Generator(device=dev).manual_seed(96)
    for qbits in (7, 8):
        lay = _Layer(lib, dev, gen, 3, 96, 16, 54, 1, qbits, True)
        x = _synthetic((3, 54, 54, 96), lay.ka, dev, gen)
        xc = _encode(lib, x, lay.ka, qbits)
        want = lay.fwd_f32(x)
        assert torch.equal(lay.fwd_codes(xc, True).view(torch.int32), want.view(torch.int32))
        assert torch.equal(lay.fwd_codes(xc, True, 0.4), _encode(lib, want, 0.4, qbits))


# ---------------------------------------------------------------------------------------------- channel-slice stores
SLICE_GEOMS = [
    # (what runs, c_in, c_out, h, k, n)
    ("k_pwc_stream", 32, 128, 27, 1, 3),
    ("k_pwc_stream (half k-step)", 16, 64, 54, 1, 3),
    ("k_pwc_slice", 256, 256, 14, 1, 3),
    ("k_pwc_tiled", 512, 256, 13, 1, 3),
    ("dense 3x3 (16 channels)", 16, 64, 54, 3, 2),
    ("dense 3x3 (resident weights)", 64, 256, 13, 3, 3),
    ("dense 3x3 (64 -> 64: float32 input encoded in the kernel)", 64, 64, 14, 3, 2),
    ("dense 3x3 (generic tiling)", 128, 128, 13, 3, 2),
    # h given as (h, w): non-square inputs and their twins (a pixel's slice starts at (row * W + col) * y_ld)
    ("k_pwc_stream, 12 x 21", 32, 128, (12, 21), 1, 3),
    ("k_pwc_stream, 21 x 12", 32, 128, (21, 12), 1, 3),
    ("dense 3x3, 12 x 21", 64, 256, (12, 21), 3, 3),
    ("dense 3x3, 21 x 12", 64, 256, (21, 12), 3, 3),
]


def _hw(h):
    return h if isinstance(h, tuple) else (h, h)


@pytest.mark.parametrize("qbits", [7, 8])
@pytest.mark.parametrize("geom", SLICE_GEOMS, ids=[g[0] for g in SLICE_GEOMS])
def test_code_output_into_a_channel_slice(lib, dev, qbits, geom):
    what, c_in, c_out, h, k, n = geom
    h, w = _hw(h)
    gen = torch.Generator(device=dev).manual_seed(7 * qbits + c_in + k)
    y_ka = 0.29
    for relu in (True, False):
        lay = _Layer(lib, dev, gen, n, c_in, c_out, h, k, qbits, relu, w=w)
        assert lay.kernel.startswith("dense_mfma" if k == 3 else "pw_mfma"), lay.kernel
        x = _synthetic((n, h, w, c_in), lay.ka, dev, gen, signed=not relu)
        xc = _encode(lib, x, lay.ka, qbits)
        dense = lay.fwd_codes(xc, True, y_ka)
        assert torch.equal(dense, _encode(lib, lay.fwd_f32(x), y_ka, qbits))
        for ld in (2 * c_out, 2 * c_out + 16):
            for c_off in (0, c_out):
                buf = torch.full(lay.out_shape(ld), 0xA5, dtype=torch.uint8, device=dev)
                lay.fwd_slice(xc, True, y_ka, buf, c_off)
                assert torch.equal(buf[..., c_off:c_off + c_out], dense), (what, qbits, relu, ld, c_off)
                outside = torch.cat([buf[..., :c_off], buf[..., c_off + c_out:]], -1)
                assert bool((outside == 0xA5).all()), (what, qbits, relu, ld, c_off, int((outside != 0xA5).sum()))
        buf = torch.full(lay.out_shape(), 0xA5, dtype=torch.uint8, device=dev)
        lay.fwd_slice(xc, True, y_ka, buf, 0)      # y_ld == C_out: slfp_conv2d_fwd_codes_ws
        assert torch.equal(buf, dense)
        if k == 3:   # the dense family also takes float32 in
            buf = torch.full(lay.out_shape(2 * c_out), 0xA5, dtype=torch.uint8, device=dev)
            lay.fwd_slice(x, False, y_ka, buf, c_out)
            assert torch.equal(buf[..., c_out:], dense) and bool((buf[..., :c_out] == 0xA5).all())


@pytest.mark.parametrize("qbits", [7, 8])
@pytest.mark.parametrize("geom", [(16, 64, 54), (48, 192, 27), (64, 256, 13), (16, 64, (12, 21)), (16, 64, (21, 12))])
def test_both_halves_of_a_fire_equal_the_encoded_concat(lib, dev, qbits, geom):
    """expand1x1 and expand3x3 write the two halves of ONE buffer: encode(cat(relu(e1), relu(e3))), with no byte left over."""
    c_in, c_out, h = geom
    h, w = _hw(h)
    gen = torch.Generator(device=dev).manual_seed(31 * qbits + c_in)
    n, y_ka = 3, 0.33
    e1 = _Layer(lib, dev, gen, n, c_in, c_out, h, 1, qbits, True, w=w)
    e3 = _Layer(lib, dev, gen, n, c_in, c_out, h, 3, qbits, True, w=w)
    x = _synthetic((n, h, w, c_in), e1.ka, dev, gen)
    xc = _encode(lib, x, e1.ka, qbits)
    buf = torch.full(e1.out_shape(2 * c_out), 0xA5, dtype=torch.uint8, device=dev)
    e1.fwd_slice(xc, True, y_ka, buf, 0)
    e3.fwd_slice(xc, True, y_ka, buf, c_out)
    want = _encode(lib, torch.cat([e1.fwd_f32(x), e3.fwd_f32(x)], -1).contiguous(), y_ka, qbits)
    assert torch.equal(buf, want), int((buf != want).sum())


# ---------------------------------------------------------------------------------------------- ceil-mode pool
@pytest.mark.parametrize("qbits", [8, 7])
def test_ceil_mode_maxpool_on_codes_equals_encoding_the_pooled_tensor(lib, dev, qbits):
    """slfp_maxpool2d_codes_ex(ceil_mode = 1) == slfp_encode_f32(F.max_pool2d(x, ..., ceil_mode=True)): SqueezeNet's 3x3 / 2 pools
    on 54 x 54 and 27 x 27 (windows hang over the edge), the h = 4, k = 2, s = 3 case (the last window starts at 3 < 4: kept),
    post-ReLU and signed, with the special classes tests/test_gpu_codes.py plants; ceil_mode = 0 is slfp_maxpool2d_codes."""
    from cnns_slfp_quantization_amd.sfp_quant import hip_maxpool_codes
    L = lib.load()
    gen = torch.Generator(device=dev).manual_seed(23 + qbits)
    ka = 0.23
    cases = (((3, 128, 54, 54), (3, 2, 0)), ((2, 256, 27, 27), (3, 2, 0)), ((2, 12, 27, 27), (3, 2, 0)), ((2, 16, 4, 4), (2, 3, 0)),
             ((2, 16, 3, 5), (2, 3, 0)), ((2, 32, 10, 11), (3, 2, 1)),
             # window, stride and padding as (h, w) pairs on non-square inputs
             ((2, 16, 13, 22), ((3, 2), (2, 1), (1, 0))), ((2, 12, 22, 13), ((2, 3), (1, 2), (0, 1))))
    for (n, c, h, w), (k, st, pd) in cases:
        for signed in (False, True):
            x = torch.randn((n, c, h, w), generator=gen, device=dev) * (5.0 * ka)
            x = x if signed else torch.relu(x)
            x.view(-1)[::7] = 15.4 * ka            # the top regular class
            x.view(-1)[3::11] = 40.0 * ka          # beyond the clamp
            x.view(-1)[5::13] = 0.03 * ka          # the 1e-10 class
            x.view(-1)[6::17] = 0.0
            if signed:
                x.view(-1)[8::19] = -40.0 * ka
            x = x.contiguous(memory_format=torch.channels_last)

            def enc(t):
                return _encode(lib, t.contiguous(memory_format=torch.channels_last), ka, qbits)
            xc = enc(x)
            want = enc(F.max_pool2d(x, k, st, pd, ceil_mode=True))
            got = hip_maxpool_codes(xc, k, st, pd, qbits, ceil_mode=True)
            assert got.shape == want.shape and torch.equal(got, want), ((n, c, h, w), (k, st, pd), signed, int((got != want).sum()))
            floor = hip_maxpool_codes(xc, k, st, pd, qbits)
            assert torch.equal(floor, enc(F.max_pool2d(x, k, st, pd)))
            y0 = torch.empty_like(floor)
            (kh, kw), (sh, sw), (ph, pw) = _hw(k), _hw(st), _hw(pd)
            lib.check(L.slfp_maxpool2d_codes_ex(xc.data_ptr(), y0.data_ptr(), n, h, w, c, kh, kw, sh, sw, ph, pw, qbits, 0, _stream()))
            assert torch.equal(y0, floor)
    assert tuple(F.max_pool2d(torch.zeros(1, 1, 4, 4), 2, 3, ceil_mode=True).shape[2:]) == (2, 2)


# ---------------------------------------------------------------------------------------------- the fixture net
def _golden():
    return np.load(os.path.join(HERE, "golden", "nets_r3_golden.npz"))


def _build_squeezenet(dev, qbits=None):
    """The fixture's SqueezeNet 1.0 out of the drop-in modules, as tests/test_gpu_parity.py builds it: name-seeded parameters,
    weight gains and per-module scales of tests/golden/nets_r3_golden.npz; channels_last."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import netgen_r3 as ng
    import utils.conv2d_func as cf
    import utils.sfp_quant as sq
    gold = _golden()
    q, batch, in_seed, seed = [int(v) for v in gold["squeezenet:meta"]]
    manifest = json.loads(bytes(gold["squeezenet:manifest"]).decode())
    gains = json.loads(bytes(gold["squeezenet:gains"]).decode())
    m = ng.BUILDERS["squeezenet"](ng.Factories(cf, qbits or q, manifest, layerout=sq.layerout_quantize_func))
    ng.fill_parameters_by_name(m, seed, gains)
    m = m.to(dev).eval().to(memory_format=torch.channels_last)
    x = ng.net_input224(batch, in_seed).to(dev).contiguous(memory_format=torch.channels_last)
    return m, x, gold


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


def _fires(m):
    return [b for b in m.modules() if type(b).__name__ == "_Fire"]


def _tree(m):
    return [(name, type(mod).__name__) for name, mod in m.named_modules()]


@pytest.mark.parametrize("qbits", [7, 8])
def test_fuse_fire_on_the_fixture_squeezenet(dev, qbits):
    """All 8 Fire modules of the fixture net on codes: bit-identical logits (q_bit 7: also inside the fixture's bars), every Fire
    conv reads and writes codes, the expands write channel slices, the two pools behind a Fire pool codes in ceil mode, no
    aten::cat and no in-place ReLU of a Fire is left; unfuse_fire restores the module tree; replays as one hipGraph."""
    from cnns_slfp_quantization_amd import fusion, graph
    m, x, gold = _build_squeezenet(dev, qbits)
    fires = _fires(m)
    assert len(fires) == 8
    named = dict(m.named_modules())
    fire_convs = {n: c for n, c in named.items() if isinstance(c, torch.nn.Conv2d) and n.startswith("features.") and n != "features.0"}
    assert len(fire_convs) == 24
    tree0 = _tree(m)
    with torch.no_grad():
        assert fusion.fuse_bn_relu(m) == 0 and fusion.link_codes_traced(m, x) == 0   # the tools of the earlier rounds change nothing here
        with _OpCount() as ops0:
            y0 = m(x)
        assert ops0.count("cat") == 8
        n = fusion.fuse_fire(m, x)
        assert n == 8, n
        with _OpCount() as ops1:
            y1 = m(x)
    assert torch.equal(y1.view(torch.int32), y0.view(torch.int32)), float((y1 - y0).abs().max())
    # no concat is left, and of the in-place ReLUs only the stem's and the classifier's: 24 ReLU passes of the Fires are gone
    assert ops1.count("cat") == 0 and ops1.count("relu") == 2 and ops0.count("relu") - ops1.count("relu") == 24, \
        (ops1.count("cat"), ops0.count("relu"), ops1.count("relu"))
    if qbits == 7:   # the fixture's own logits: the bars of tests/test_gpu_parity.py
        Lg, G = y1.cpu().numpy(), gold["squeezenet:logits"]
        el = rel_errors(Lg, G)
        print(f"squeezenet fuse_fire: logits vs fixture {el}")
        assert el[0] <= R3_SQUEEZENET_BARS[0] and el[1] <= R3_SQUEEZENET_BARS[1], el
        assert Lg.shape[0] == 4 and int((Lg.argmax(1) == G.argmax(1)).sum()) == 4
    kernels = {n: c._last_kernel for n, c in fire_convs.items()}
    for name, k in kernels.items():
        assert "codes_in" in k, (name, k)      # features.3.squeeze too: its float32 input goes through one slfp_encode_f32 pass
        assert "codes_out" in k, (name, k)
        assert k.endswith("+slice") == (".expand" in name), (name, k)
    assert sum(k.endswith("+slice") for k in kernels.values()) == 16
    assert "codes_in" in named["classifier.1"]._last_kernel and "codes_out" not in named["classifier.1"]._last_kernel
    assert named["features.0"]._last_kernel is not None and "codes" not in named["features.0"]._last_kernel
    wrapped = [n for n, c in m.named_modules() if isinstance(c, fusion.CodeMaxPool2d)]
    assert wrapped == ["features.6", "features.11"], wrapped      # exactly the two pools behind a Fire; the stem's pool is not
    assert all(c.pool.ceil_mode for c in m.modules() if isinstance(c, fusion.CodeMaxPool2d))
    with torch.no_grad():
        g = graph.GraphedModule(m)
        assert torch.equal(g(x).view(torch.int32), y0.view(torch.int32))
        assert torch.equal(g(x).view(torch.int32), y0.view(torch.int32))
        assert fusion.unfuse_fire(m) == 8
        assert _tree(m) == tree0
        assert all("forward" not in f.__dict__ for f in fires)
        assert all(c._code_out is None and c._post is None for c in fire_convs.values())
        y2 = m(x)
        assert torch.equal(y2.view(torch.int32), y0.view(torch.int32))
        assert all("codes" not in c._last_kernel for c in fire_convs.values())
        assert fusion.unfuse_fire(m) == 0


def test_fused_fire_modules_refuse_training(dev):
    from cnns_slfp_quantization_amd import fusion
    m, x, _ = _build_squeezenet(dev)
    with torch.no_grad():
        assert fusion.fuse_fire(m, x) == 8
    m.train()
    with pytest.raises(RuntimeError, match="inference-only"):
        m(x)
    m.eval()
    with torch.no_grad():
        assert fusion.unfuse_fire(m) == 8
    m.train()
    assert fusion.fuse_fire(m, x) == 0      # a model in training mode is not rewritten


# ---------------------------------------------------------------------------------------------- refusals
def _small_fire_net(dev, ka_e3=0.3, leak=None):
    import utils.conv2d_func as cf

    def conv(cin, cout, k, ka, pad=0):
        return cf.conv2d_Q_bias(q_bit=7, Kw=0.02, Ka=ka)(cin, cout, k, 0.02, ka, 1, pad)

    class Fire(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.squeeze = conv(32, 16, 1, 0.4)
            self.squeeze_activation = torch.nn.ReLU(inplace=True)
            self.expand1x1 = conv(16, 64, 1, 0.3)
            self.expand1x1_activation = torch.nn.ReLU(inplace=True)
            self.expand3x3 = conv(16, 64, 3, ka_e3, 1)
            self.expand3x3_activation = torch.nn.ReLU(inplace=True)

        def forward(self, x):
            h = self.squeeze_activation(self.squeeze(x))
            parts = [self.expand1x1_activation(self.expand1x1(h)), self.expand3x3_activation(self.expand3x3(h))]
            if leak == "block":      # the squeeze output leaves the block too: a use no module hook records
                parts.append(h.repeat(1, 8, 1, 1))
            return torch.cat(parts, 1)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.fire = Fire()
            self.pool = torch.nn.MaxPool2d(3, 2, ceil_mode=True)
            self.head = conv(256 if leak == "block" else 128, 32, 1, 0.35)

        def forward(self, x):
            y = self.fire(x)
            out = self.head(self.pool(y))
            if leak == "model":      # the block's output is also read by a functional op behind the block
                out = out + y.mean()
            return out

    torch.manual_seed(12)
    m = Net().to(dev).eval().to(memory_format=torch.channels_last)
    with torch.no_grad():
        for c in m.modules():
            if isinstance(c, torch.nn.Conv2d):
                c.weight.mul_(0.5)
    x = (torch.relu(torch.randn(3, 32, 12, 12, device=dev)) * 1.5).contiguous(memory_format=torch.channels_last)
    return m, x


@pytest.mark.parametrize("case", ["ok", "different Ka", "leak in the block", "leak behind the block"])
def test_fuse_fire_refuses_what_it_cannot_prove(dev, case):
    from cnns_slfp_quantization_amd import fusion
    m, x = _small_fire_net(dev, ka_e3=0.26 if case == "different Ka" else 0.3,
                           leak={"leak in the block": "block", "leak behind the block": "model"}.get(case))
    tree0 = _tree(m)
    with torch.no_grad():
        y0 = m(x)
        n = fusion.fuse_fire(m, x)
        y1 = m(x)
    assert torch.equal(y1.view(torch.int32), y0.view(torch.int32))
    if case == "ok":
        assert n == 1 and "+slice" in m.fire.expand3x3._last_kernel and isinstance(m.pool, fusion.CodeMaxPool2d)
        assert "codes_in" in m.head._last_kernel
        assert fusion.unfuse_fire(m) == 1
    else:
        assert n == 0
        assert "forward" not in m.fire.__dict__ and _tree(m) == tree0
        assert all(c._code_out is None and c._post is None for c in m.modules() if isinstance(c, torch.nn.Conv2d))
        assert "codes" not in m.fire.expand3x3._last_kernel and "codes" not in m.head._last_kernel
    assert _tree(m) == tree0


def test_out_slice_raises_outside_a_linked_producer(dev):
    import utils.conv2d_func as cf
    m = cf.conv2d_Q_bias(q_bit=7, Kw=0.02, Ka=0.3)(16, 64, 1, 0.02, 0.3).to(dev).eval().to(memory_format=torch.channels_last)
    x = torch.ones((2, 16, 6, 6), dtype=torch.uint8, device=dev).contiguous(memory_format=torch.channels_last)
    buf = torch.zeros((2, 128, 6, 6), dtype=torch.uint8, device=dev).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="linked code producer"):
            m.forward_slice(x, (buf, 0))               # unlinked
        m._code_out = (0.3, 7)
        assert m.forward_slice(x, (buf, 64)) is buf and m._last_kernel.endswith("+codes_in+codes_out+slice")
        assert bool((buf[:, :64] == 0).all())
        with pytest.raises(RuntimeError, match="no kernel"):
            m.forward_slice(x, (buf, 8))               # the channel offset is a multiple of 16
        with pytest.raises(RuntimeError, match="do not"):
            m.forward_slice(x, (buf, 80))              # does not fit
        with pytest.raises(RuntimeError, match="buffer"):
            m.forward_slice(x, (buf.float(), 0))
        m.train()
        with pytest.raises(RuntimeError, match="linked code producer"):
            m.forward_slice(x, (buf, 0))


# ---------------------------------------------------------------------------------------------- one Fire against the CPU oracle
def _fire3_of_the_fixture():
    """features.3 of the fixture net on the CPU: (weights, biases, (Ka, Kw)) of squeeze / expand1x1 / expand3x3 and the Ka of the
    layer that reads its output (features.4.squeeze), all from the fixture's manifest and name-seeded parameters."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import netgen_r3 as ng
    gold = _golden()
    seed = int(gold["squeezenet:meta"][3])
    manifest = json.loads(bytes(gold["squeezenet:manifest"]).decode())
    gains = json.loads(bytes(gold["squeezenet:gains"]).decode())
    out = {}
    for name, shape in (("squeeze", (16, 96, 1, 1)), ("expand1x1", (64, 16, 1, 1)), ("expand3x3", (64, 16, 3, 3))):
        key = f"features.3.{name}"
        w = ng.param_by_name(key + ".weight", shape, seed)
        if key + ".weight" in gains:
            w = (w * np.float32(gains[key + ".weight"])).astype(np.float32)
        out[name] = (w, ng.param_by_name(key + ".bias", (shape[0],), seed), tuple(np.float64(v) for v in manifest[key]))
    return out, np.float64(manifest["features.4.squeeze"][0])


def _fire_input(ka, seed=2024):
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.standard_normal((2, 96, 54, 54)), 0.0) * (3.0 * ka)
    return x.astype(np.float32)


def _oracle_fire_codes(fire, ka_next, x, double=True):
    """encode(cat(relu(e1(h)), relu(e3(h)))), h = relu(squeeze(x)), for the next layer's quantizer (NCHW codes).  double=True:
    oracle.conv2d (quantizers of the oracle, contraction accumulated in double, rounded once); double=False: the same quantized
    operands through ATen's float32 convolution with the reference's arithmetic, conv(xq, wq, b / Ka / Kw) * Ka * Kw."""
    def conv(name, t, pad):
        w, b, (ka, kw) = fire[name]
        if double:
            return so.conv2d(t, w, b, 1, pad, 1, 1, ka, kw, 7)
        xq = torch.from_numpy(so.quantize(t, np.float32(ka), so.FMT_SFP7))
        wq = torch.from_numpy(so.quantize(w, np.float32(kw), so.FMT_SFP7))
        bq = torch.from_numpy(b) / np.float32(ka) / np.float32(kw)
        return (F.conv2d(xq, wq, bq, 1, pad) * np.float32(ka) * np.float32(kw)).numpy()
    h = np.maximum(conv("squeeze", x, 0), 0.0)
    y = np.concatenate([np.maximum(conv("expand1x1", h, 0), 0.0), np.maximum(conv("expand3x3", h, 1), 0.0)], 1)
    return so.encode(y, np.float32(ka_next), so.FMT_SFP7 | so.FMT_EXT), y


def test_one_fire_against_the_cpu_oracle(lib, dev):
    """features.3 of the fixture net (96 -> 16 -> 64 + 64 @ 54 x 54, SFP<3,3>) as one fused block against oracle.conv2d of the
    three layers chained in double.  The block's output is codes, so two things are compared: the decoded values under the family
    bar tol = 1e-5 wherever the code is the oracle's, and the share of elements whose code differs (a value within float32
    round-off of a class boundary of the next layer's quantizer lands on the other side).  That share may not exceed what the
    oracle's own chain produces when its contraction runs in float32 (ATen on the CPU) instead of double, on the same inputs:
    measured on the CPU for the input below, seed 2024, 2 x 128 x 54 x 54 = 746 496 elements:
        float32 chain vs double chain: 0 differing codes, share 0.0 (< 1e-4); 67 940 float32 values differ by an ulp or more
        fused block on the MI355X vs double chain: 0 differing codes, share 0.0
    so the bound below is computed, not assumed, and the fused block has to give the oracle's codes wherever the float32 chain does."""
    from cnns_slfp_quantization_amd import fusion
    import utils.conv2d_func as cf
    fire, ka_next = _fire3_of_the_fixture()
    x = _fire_input(fire["squeeze"][2][0])
    ref_codes, ref = _oracle_fire_codes(fire, ka_next, x, double=True)
    f32_codes, _ = _oracle_fire_codes(fire, ka_next, x, double=False)
    share_ref = float(np.mean(ref_codes != f32_codes))
    print(f"oracle float32 chain vs double chain: {int(np.sum(ref_codes != f32_codes))} of {ref_codes.size} codes differ, share {share_ref:.3e}")
    assert share_ref < 1e-4

    class Fire(torch.nn.Module):
        def __init__(self):
            super().__init__()
            for name, k, pad in (("squeeze", 1, 0), ("expand1x1", 1, 0), ("expand3x3", 3, 1)):
                w, b, (ka, kw) = fire[name]
                c = cf.conv2d_Q_bias(q_bit=7, Kw=kw, Ka=ka)(w.shape[1], w.shape[0], k, kw, ka, 1, pad)
                with torch.no_grad():
                    c.weight.copy_(torch.from_numpy(w)); c.bias.copy_(torch.from_numpy(b))
                setattr(self, name, c)
                setattr(self, name + "_activation", torch.nn.ReLU(inplace=True))

        def forward(self, t):
            t = self.squeeze_activation(self.squeeze(t))
            return torch.cat([self.expand1x1_activation(self.expand1x1(t)), self.expand3x3_activation(self.expand3x3(t))], 1)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.fire = Fire()
            self.next = cf.conv2d_Q_bias(q_bit=7, Kw=0.05, Ka=ka_next)(128, 16, 1, 0.05, ka_next)

        def forward(self, t):
            return self.next(self.fire(t))

    m = Net().to(dev).eval().to(memory_format=torch.channels_last)
    xg = torch.from_numpy(x).to(dev).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        assert fusion.fuse_fire(m, xg) == 1
        codes = m.fire(xg)
    assert codes.dtype == torch.uint8 and "+slice" in m.fire.expand1x1._last_kernel
    got_codes = codes.cpu().numpy()          # logical NCHW, like the oracle's
    flips = got_codes != ref_codes
    share = float(np.mean(flips))
    got = so.decode(got_codes, so.FMT_SFP7 | so.FMT_EXT).astype(np.float64)
    want = so.decode(ref_codes, so.FMT_SFP7 | so.FMT_EXT).astype(np.float64)
    e = rel_errors(got[~flips], want[~flips])
    print(f"fused Fire vs oracle: {int(flips.sum())} of {flips.size} codes differ, share {share:.3e} (oracle float32 vs double: {share_ref:.3e}); "
          f"decoded values elsewhere: {e}")
    assert max(e) <= TOL_SFP7, e
    assert share <= share_ref, (share, share_ref)
