"""GPU (MI355X): the pointwise (1x1) kernels on codes in the float32-equivalent (three-pass) mode (DESIGN section 34;
slfp_conv2d_fwd_codes_x3), every instance at the small ragged shapes of tests/_pw_x3_cases.py straight through the C ABI, then two
whole nets through fusion.link_codes(x3=True) / fusion.link_codes_traced(x3=True).

Per row, with every tensor a launch reads or writes inside an arena with 4 KiB guards (NaN around the float32 input, 0x7F around the
codes, 0xA5 around the outputs, which must stay untouched):

  * codes in -> float32 out is BIT-IDENTICAL to slfp_conv2d_fwd_post with the same three-pass descriptor on the float32 tensor whose
    slfp_encode_f32 codes were fed -- plain (conv + bias) and with post scale / shift for ReLU 0 and 1;
  * that output is held to the CPU oracle at TOL_EXACT, with the elementwise bar of a float32-equivalent kernel;
  * codes out are byte-equal to slfp_encode_f32 of the float32-interface output for the reader's (Ka, q_bit), q_bit 8 and 7;
  * a second launch gives the same bits.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from _bars import ELEM_MIN, TOL_EXACT, elem_frac_bar
from _pw_x3_cases import ROWS, make_desc, make_io, set_switches, variant as _variant
from conftest import elem_exceed_frac, rel_errors
from oracle import slfp_oracle as so

pytestmark = pytest.mark.gpu

KA, KW, KA_NEXT = 0.21, 0.027, 0.2345
GUARD = 4096     # bytes on each side of every tensor
KERN = "pw_mfma_f16x3"
RAN = set()      # reporter strings of the launches the row tests made
_LAYERS = {}


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


class _Arena:
    """A tensor as a view into a byte buffer with GUARD bytes in front of and behind it."""

    def __init__(self, shape, dtype, dev, fill, src=None):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.nbytes = n
        if dtype == torch.float32 and fill != fill:   # NaN guards around a float32 input
            self.buf = torch.full(((2 * GUARD + n) // 4,), float("nan"), dtype=torch.float32, device=dev).view(torch.uint8)
            self.fill = None
        else:
            self.buf = torch.full((2 * GUARD + n,), fill, dtype=torch.uint8, device=dev)
            self.fill = fill
        self.t = self.buf[GUARD:GUARD + n].view(dtype).view(shape)
        assert self.t.data_ptr() % 16 == 0
        if src is not None:
            self.t.copy_(src)

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        return bool((self.buf[:GUARD] == self.fill).all()) and bool((self.buf[GUARD + self.nbytes:] == self.fill).all())


class _Layer:
    """One descriptor of the table: the seeded input as float32 and as codes in guarded arenas, weights, bias, post vectors, the
    prepared three-pass blob, and -- computed once, never written again -- the oracle's output and the float32-interface launches."""

    def __init__(self, lib, row, dev):
        L = lib.load()
        self.lib, self.L, self.row, self.dev = lib, L, row, dev
        self.d = make_desc(lib, row, KA, KW)
        gen = torch.Generator(device=dev).manual_seed(9000 + row.c_in + 3 * row.c_out + row.stride)
        x = torch.randn((row.n, row.h, row.w, row.c_in), generator=gen, device=dev) * (2.5 * KA)
        x.view(-1)[::97] = 17.0 * KA    # beyond the clamp: the clamp literal's hi / lo pair
        x.view(-1)[5::193] = 0.0        # exact zeros
        x.view(-1)[11::211] = 1e-7      # the tiny class: 0 / 0
        self.x = _Arena(x.shape, torch.float32, dev, float("nan"), x)
        self.w = torch.randn((row.c_out, row.c_in, 1, 1), generator=gen, device=dev) * (4.0 * KW)
        self.bias = torch.randn(row.c_out, generator=gen, device=dev) * 0.3
        self.scale = torch.rand(row.c_out, generator=gen, device=dev) + 0.5
        self.shift = torch.randn(row.c_out, generator=gen, device=dev) * 0.3
        ho, wo = ctypes.c_int64(), ctypes.c_int64()
        lib.check(L.slfp_conv2d_out_shape(ctypes.byref(self.d), ctypes.byref(ho), ctypes.byref(wo)))
        self.out_shape = (row.n, ho.value, wo.value, row.c_out)
        assert L.slfp_conv2d_kernel_name(ctypes.byref(self.d)).decode() == KERN
        self.blob = torch.empty(L.slfp_conv2d_wprep_bytes(ctypes.byref(self.d)), dtype=torch.uint8, device=dev)
        lib.check(L.slfp_conv2d_prepare_weights(ctypes.byref(self.d), self.w.data_ptr(), self.blob.data_ptr(), None, _stream()))
        self.xc = _Arena(x.shape, torch.uint8, dev, 0x7F, self.encode(x, KA, 8))
        self.ref = so.conv2d(x.permute(0, 3, 1, 2).contiguous().cpu().numpy(), self.w.cpu().numpy(), self.bias.cpu().numpy(),
                             row.stride, 0, 1, 1, KA, KW, 8)
        set_switches(L, None)
        self.base = self.f32()
        self.check_oracle(self.base, "float32 interface")
        self.post = {relu: self.f32(post=True, relu=relu) for relu in (0, 1)}

    def encode(self, t, ka, qbits):
        c = torch.empty(t.shape, dtype=torch.uint8, device=t.device)
        fmt = (self.lib.FMT_ACT8 if qbits == 8 else self.lib.FMT_SFP7) | self.lib.FMT_EXT
        self.lib.check(self.L.slfp_encode_f32(t.contiguous().data_ptr(), c.data_ptr(), t.numel(), float(np.float32(ka)), fmt, _stream()))
        return c

    def _vecs(self, post):
        return (self.bias.data_ptr(), self.scale.data_ptr() if post else None, self.shift.data_ptr() if post else None)

    def _done(self, y):
        assert y.guards_intact(), (self.row, "guard band written")
        return y.t

    def f32(self, post=False, relu=0):
        y = _Arena(self.out_shape, torch.float32, self.dev, 0xA5)
        b, sc, sh = self._vecs(post)
        self.lib.check(self.L.slfp_conv2d_fwd_post(ctypes.byref(self.d), self.x.ptr(), self.blob.data_ptr(), b, sc, sh, relu, y.ptr(), None, None,
                                                   _stream()))
        return self._done(y)

    def x3(self, y_codes, post=False, relu=0, y_qbits=8):
        y = _Arena(self.out_shape, torch.uint8 if y_codes else torch.float32, self.dev, 0xA5)
        io = make_io(self.lib, "cout" if y_codes else "cin", KA_NEXT, y_qbits)
        b, sc, sh = self._vecs(post)
        assert self.L.slfp_conv2d_codes_x3_supported(ctypes.byref(self.d), ctypes.byref(io), 1, relu) == 1, self.row
        self.lib.check(self.L.slfp_conv2d_fwd_codes_x3(ctypes.byref(self.d), ctypes.byref(io), self.xc.ptr(), self.blob.data_ptr(), b, sc, sh, relu,
                                                       y.ptr(), _stream()))
        assert self.xc.guards_intact(), (self.row, "guard band of the code input written")
        return self._done(y)

    def check_oracle(self, y, what):
        assert not bool(torch.isnan(y).any()), (self.row, what, "NaN in the output of clean input: a read outside the tensor")
        got = y.permute(0, 3, 1, 2).contiguous().cpu().numpy()
        emax, el2 = rel_errors(got, self.ref)
        frac = elem_exceed_frac(got, self.ref)
        print(f"{self.row.name}: {what} max-rel {emax:.3e} l2 {el2:.3e} elem-frac {frac:.4f}")
        assert emax <= TOL_EXACT and el2 <= TOL_EXACT, (self.row, what, emax, el2)
        assert got.size >= ELEM_MIN
        assert frac <= elem_frac_bar(KERN), (self.row, what, frac)


def _layer(lib, row, dev):
    key = (row.c_in, row.c_out, row.stride, row.n, row.h, row.w)
    if key not in _LAYERS:
        _LAYERS[key] = _Layer(lib, row, dev)
    return _LAYERS[key]


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_pw_codes_x3_row(lib, dev, row):
    L = lib.load()
    try:
        lay = _layer(lib, row, dev)   # (leaves the switches unset)
        set_switches(L, row.env)
        got_v = _variant(lib, lay.d, make_io(lib, row.iface, KA_NEXT))
        assert got_v == row.variant, (row, got_v)
        print(f"{row.name}: {row.iface} -> {got_v}")
        if row.iface == "cin":
            y = lay.x3(False)
            assert _same(y, lay.base), (row, "codes in differs from float32 in", int((y != lay.base).sum()))
            lay.check_oracle(y, got_v)
            for relu in (0, 1):
                yp = lay.x3(False, post=True, relu=relu)
                assert _same(yp, lay.post[relu]), (row, relu, "post-op launch", int((yp != lay.post[relu]).sum()))
            assert _same(lay.x3(False), y), (row, "run to run")
        else:
            for y_qbits in (8, 7):
                c = lay.x3(True, y_qbits=y_qbits)
                want = lay.encode(lay.base, KA_NEXT, y_qbits)           # base is held to the oracle when the layer is built
                assert torch.equal(c, want), (row, y_qbits, "codes of conv + bias", int((c != want).sum()))
                for relu in (1, 0):
                    cp = lay.x3(True, post=True, relu=relu, y_qbits=y_qbits)
                    want = lay.encode(lay.post[relu], KA_NEXT, y_qbits)
                    assert torch.equal(cp, want), (row, y_qbits, relu, "post-op launch", int((cp != want).sum()))
                assert torch.equal(lay.x3(True, y_qbits=y_qbits), c), (row, y_qbits, "run to run")
        RAN.add(got_v)
    finally:
        set_switches(L, None)


def test_zz_every_variant_of_the_table_ran():
    """Closes the row tests: what they launched, by the reporter's own account, is the table's set of variants."""
    assert RAN == {r.variant for r in ROWS}, RAN ^ {r.variant for r in ROWS}


# ------------------------------------------------------------------------------------------------------------ whole nets
def _pointwise(m):
    return [c for c in m.modules() if isinstance(c, nn.Conv2d) and hasattr(c, "_code_x3") and tuple(c.kernel_size) == (1, 1) and c.groups == 1]


def test_mobilenetv1_cifar_linked_in_three_pass_mode(dev):
    """CIFAR-size MobileNetV1 after fuse_bn_relu: link_codes(x3=True) in three-pass mode makes the links single-pass mode makes, all 13
    pointwise layers run slfp_conv2d_fwd_codes_x3, and the logits are those of the unlinked three-pass model, bit for bit."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import netgen
    from cnns_slfp_quantization_amd import conv2d_func as cf
    from cnns_slfp_quantization_amd import fusion, layer_specs
    scales = [(r["Ka"], r["Kw"]) for r in layer_specs.nets()["mobilenetv1_cifar32"]["layers"]]
    x = netgen.net_input().to(dev).contiguous(memory_format=torch.channels_last)

    def fused():
        m = netgen.fill_parameters(netgen.build_mobilenetv1_cifar(cf.conv2d_Q, cf.linear_Q, 8, scales)).to(dev).eval()
        m = m.to(memory_format=torch.channels_last)
        assert fusion.fuse_bn_relu(m) >= 27
        return m

    prev = cf.options.mfma_passes
    try:
        with torch.no_grad():
            cf.options.mfma_passes = 0
            n_single = fusion.link_codes(fused(), x)
            assert n_single >= 13
            cf.options.mfma_passes = 3
            m = fused()
            y0 = m(x).clone()
            assert all(c._last_kernel == "pw_mfma_f16x3" for c in _pointwise(m))
            n_plain = fusion.link_codes(fused(), x)
            n = fusion.link_codes(m, x, x3=True)
            print(f"links: single-pass {n_single}, three-pass without x3 {n_plain}, with x3 {n}")
            assert n == n_single and n_plain < n
            y = m(x)
            pw = _pointwise(m)
            assert len(pw) == 13
            for c in pw:
                assert c._code_x3 and c._last_kernel.startswith("pw_mfma_f16x3+codes_in") and c._last_kernel.endswith("+x3"), c._last_kernel
            assert torch.equal(y, y0), int((y != y0).sum())
            assert fusion.unlink_codes(m) == n and not any(c._code_x3 for c in pw)
            assert torch.equal(m(x), y0)
    finally:
        cf.options.mfma_passes = prev


def _bottlenecks(dev):
    from cnns_slfp_quantization_amd import conv2d_func as cf

    def C(cin, cout, k, ka, stride=1, pad=0):
        return cf.conv2d_Q(q_bit=8, Kw=0.02, Ka=ka)(cin, cout, k, 0.02, ka, stride, pad)

    class Bottleneck(nn.Module):
        def __init__(self, cin, mid, cout, ka, down):
            super().__init__()
            self.conv1, self.bn1 = C(cin, mid, 1, ka[0]), nn.BatchNorm2d(mid)
            self.conv2, self.bn2 = C(mid, mid, 3, ka[1], 1, 1), nn.BatchNorm2d(mid)
            self.conv3, self.bn3 = C(mid, cout, 1, ka[2]), nn.BatchNorm2d(cout)
            self.relu = nn.ReLU(inplace=True)
            self.downsample = nn.Sequential(C(cin, cout, 1, ka[0])) if down else None

        def forward(self, x):
            out = self.relu(self.bn1(self.conv1(x)))
            out = self.relu(self.bn2(self.conv2(out)))
            out = self.bn3(self.conv3(out))
            # (out of place: an in-place add would make conv3's own output tensor the next block's input, a link the trace would try)
            return self.relu(out + (x if self.downsample is None else self.downsample(x)))

    torch.manual_seed(34)
    m = nn.Sequential(Bottleneck(64, 64, 128, (0.29, 0.27, 0.25), True), Bottleneck(128, 64, 128, (0.31, 0.26, 0.24), False))
    gen = torch.Generator().manual_seed(35)
    with torch.no_grad():
        for bn in [b for b in m.modules() if isinstance(b, nn.BatchNorm2d)]:
            bn.running_mean.copy_(torch.randn(bn.num_features, generator=gen) * 0.1)
            bn.running_var.copy_(0.5 + torch.rand(bn.num_features, generator=gen))
            bn.weight.copy_(0.5 + torch.rand(bn.num_features, generator=gen))
            bn.bias.copy_(torch.randn(bn.num_features, generator=gen) * 0.1)
    x = torch.rand(2, 64, 16, 16, generator=gen)
    m = m.to(dev).eval().to(memory_format=torch.channels_last)
    return m, x.to(dev).contiguous(memory_format=torch.channels_last)


def test_bottleneck_stack_traced_links_in_three_pass_mode(dev):
    """Two hand-wired Bottlenecks at 16 x 16 after fuse_named_bn: link_codes_traced(x3=True) links conv2 -> conv3 of each block (conv3
    then runs slfp_conv2d_fwd_codes_x3) with the logits of the unlinked three-pass model, bit for bit; without x3 neither is linked."""
    from cnns_slfp_quantization_amd import conv2d_func as cf
    from cnns_slfp_quantization_amd import fusion
    prev = cf.options.mfma_passes
    try:
        cf.options.mfma_passes = 3
        with torch.no_grad():
            m, x = _bottlenecks(dev)
            assert fusion.fuse_named_bn(m, example_input=x) == 6
            y0 = m(x).clone()
            n_plain = fusion.link_codes_traced(m, x)
            assert all(b.conv2._code_out is None and not b.conv3._code_x3 for b in m), n_plain
            assert all(b.conv3._last_kernel == "pw_mfma_f16x3" for b in m)
            fusion.unlink_codes(m)
            n = fusion.link_codes_traced(m, x, x3=True)
            print(f"traced links: without x3 {n_plain}, with x3 {n}")
            assert n == n_plain + 2
            y = m(x)
            for b in m:
                assert b.conv2._code_out is not None and b.conv3._code_x3
                assert b.conv2._last_kernel.endswith("+codes_out"), b.conv2._last_kernel
                assert b.conv3._last_kernel == "pw_mfma_f16x3+codes_in+x3", b.conv3._last_kernel
            assert torch.equal(y, y0), int((y != y0).sum())
            assert fusion.unlink_codes(m) == n and not any(b.conv3._code_x3 for b in m)
            assert torch.equal(m(x), y0)
    finally:
        cf.options.mfma_passes = prev
