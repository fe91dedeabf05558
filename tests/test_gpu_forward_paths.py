"""MI355X: every forward path of a Conv2d_Q module, once -- plain float32, codes in, codes out, the float32 -> codes entry layer,
forward_slice, forward(residual=), the dense k x k route (with its workspace) and the depthwise-on-codes route.  For each path:
the matching slfp_conv2d_*_supported query says yes (so no path is skipped silently), the module's output equals the same C entry
point called by hand through _lib with the module's own weight blob, code outputs equal slfp_encode_f32 of the float32
interface's result, and the module's bookkeeping is exact: the `_last_kernel` string, exactly one of `_last_input` /
`_last_codes`, `input_q`, one new plan on the first call and none on the second, one weight blob for all paths of a module.
Everything is channels_last, eval mode, no_grad, N = 2 on 8 x 8 images.  Every geometry below is taken by its query as it stands;
none had to be replaced by one from tests/test_gpu_codes.py / tests/test_gpu_fire.py."""
import ctypes

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
KA, KW, KA_NEXT = 0.25, 0.02, 0.3
N, C, HW = 2, 32, 8
PW_KERNEL = {8: "pw_mfma_f16x1", 7: "pw_mfma_f16_exact"}
DENSE_KERNEL = {8: "dense_mfma_f16x1", 7: "dense_mfma_f16_exact"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _layer(dev, q_bit, k, groups, bias, relu, seed):
    """A Conv2d_Q layer C -> C with a BatchNorm folded into its epilogue (fusion.fuse_pair), on the device, in eval mode."""
    import utils.conv2d_func as cf
    from cnns_slfp_quantization_amd import fusion
    g = torch.Generator().manual_seed(seed)
    m = cf.conv2d_Q_bias(q_bit, KW, KA)(C, C, k, KW, KA, 1, k // 2, groups=groups, bias=bias)
    bn = nn.BatchNorm2d(C)
    with torch.no_grad():
        m.weight.copy_(torch.randn(m.weight.shape, generator=g) * 2.5 * KW)
        if bias:
            m.bias.copy_(torch.randn(C, generator=g) * 0.1)
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g) * 0.2)
        bn.running_mean.copy_(torch.randn(C, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    m, bn = m.to(dev).eval(), bn.to(dev).eval()
    fusion.fuse_pair(m, bn, relu=relu)
    return m


class _Hand:
    """The C entry points called by hand for module `m` on an input of x's shape: descriptor and io from the module's own
    builders, the weight blob the module prepared, its bias and its folded epilogue."""

    def __init__(self, m, shape):
        from cnns_slfp_quantization_amd import _lib
        from cnns_slfp_quantization_amd import conv2d_func as cfi
        self.lib, self.L, self.cfi, self.m = _lib, _lib.load(), cfi, m
        self.d = cfi._conv_desc(m, shape)
        self.kernel = self.L.slfp_conv2d_kernel_name(ctypes.byref(self.d)).decode()
        self.ws_bytes = self.L.slfp_conv2d_workspace_bytes(ctypes.byref(self.d))

    def io(self, x_codes, out):
        return self.cfi._conv_io(x_codes, out)

    def head(self, io, x):
        m = self.m
        ps, psh, _ = m._post
        assert m._prep.blob is not None, "the module has prepared its weights"
        return (ctypes.byref(self.d),) + ((ctypes.byref(io),) if io is not None else ()) + (
            x.data_ptr(), m._prep.blob.data_ptr(), _ptr(m.bias), _ptr(ps), _ptr(psh))

    def flags(self):
        return int(self.m._post[2])

    def has_bias(self):
        return 1 if self.m.bias is not None else 0

    def out(self, dtype):
        return torch.empty((N, C, HW, HW), dtype=dtype, device=self.m.weight.device, memory_format=torch.channels_last)

    def workspace(self):
        return torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.m.weight.device) if self.ws_bytes else None

    def post(self, x):
        y = self.out(torch.float32)
        ws = self.workspace()
        self.lib.check(self.L.slfp_conv2d_fwd_post(*self.head(None, x), self.flags(), y.data_ptr(), None, _ptr(ws), _stream()))
        return y

    def codes(self, x, out):
        io = self.io(x.dtype == torch.uint8, out)
        assert self.L.slfp_conv2d_codes_supported(ctypes.byref(self.d), ctypes.byref(io), self.has_bias(), self.flags()) == 1
        y = self.out(torch.uint8 if out is not None else torch.float32)
        ws = self.workspace()
        self.lib.check(self.L.slfp_conv2d_fwd_codes_ws(*self.head(io, x), self.flags(), y.data_ptr(), _ptr(ws), _stream()))
        return y

    def entry(self, x, out):
        io = self.io(False, out)
        assert self.L.slfp_conv2d_entry_supported(ctypes.byref(self.d), ctypes.byref(io), self.has_bias(), self.flags()) == 1
        y = self.out(torch.uint8)
        self.lib.check(self.L.slfp_conv2d_fwd_entry(*self.head(io, x), self.flags(), y.data_ptr(), _stream()))
        return y

    def slice(self, x, out, buf, c_off):
        io, ld = self.io(x.dtype == torch.uint8, out), buf.shape[1]
        assert self.L.slfp_conv2d_codes_slice_supported(ctypes.byref(self.d), ctypes.byref(io), self.has_bias(), self.flags(), ld) == 1
        ws = self.workspace()
        self.lib.check(self.L.slfp_conv2d_fwd_codes_slice(*self.head(io, x), self.flags(), buf.data_ptr() + c_off, ld, _ptr(ws),
                                                          _stream()))
        return buf

    def res(self, x, r, relu):
        io = self.io(x.dtype == torch.uint8, None)
        assert self.flags() == 0   # a ReLU in the epilogue would sit in front of the add
        assert self.L.slfp_conv2d_res_supported(ctypes.byref(self.d), ctypes.byref(io), self.has_bias(), 1 if relu else 0) == 1
        y = self.out(torch.float32)
        self.lib.check(self.L.slfp_conv2d_fwd_res(*self.head(io, x), 1 if relu else 0, r.data_ptr(), y.data_ptr(), None, _stream()))
        return y


def _run(m, call, x, kernel, q_bit):
    """Runs one module path twice and checks the bookkeeping every path shares; returns the first call's output (a copy, for
    paths that write into a caller's buffer) and asserts the second call's equals it."""
    from cnns_slfp_quantization_amd import _lib
    from cnns_slfp_quantization_amd.sfp_quant import hip_quantize, hip_decode
    fmt = _lib.FMT_ACT8 if q_bit == 8 else _lib.FMT_SFP7
    plans = len(m._plans)
    y = call().clone(memory_format=torch.channels_last)
    assert len(m._plans) == plans + 1, "the first call makes exactly one plan"
    assert m._last_kernel == kernel
    x_codes = x.dtype == torch.uint8
    assert (m._last_input is None) != (m._last_codes is None), "exactly one of _last_input / _last_codes"
    assert (m._last_codes if x_codes else m._last_input).data_ptr() == x.data_ptr()
    assert torch.equal(m.input_q, hip_decode(x, fmt) if x_codes else hip_quantize(x, KA, fmt))
    blob = m._prep.blob
    assert torch.equal(call(), y)
    assert len(m._plans) == plans + 1, "the second call finds the plan"
    assert m._prep.blob is blob
    return y


@pytest.mark.parametrize("q_bit", [8, 7])
def test_every_forward_path_of_a_pointwise_layer(dev, q_bit):
    from cnns_slfp_quantization_amd import _lib
    from cnns_slfp_quantization_amd.sfp_quant import hip_encode
    fmt = _lib.FMT_ACT8 if q_bit == 8 else _lib.FMT_SFP7
    g = torch.Generator().manual_seed(10 + q_bit)
    x = (torch.randn(N, C, HW, HW, generator=g) * 0.8).to(dev).contiguous(memory_format=torch.channels_last)
    r = torch.randn(N, C, HW, HW, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    xc = hip_encode(x, KA, fmt)
    out = (KA_NEXT, q_bit)
    m = _layer(dev, q_bit, 1, 1, bias=True, relu=True, seed=q_bit)
    hand = _Hand(m, x.shape)
    name = PW_KERNEL[q_bit]
    assert hand.kernel == name and hand.ws_bytes == 0
    with torch.no_grad():
        # plain float32
        y32 = _run(m, lambda: m(x), x, name, q_bit)
        blob = m._prep.blob
        assert torch.equal(y32, hand.post(x))
        want = hip_encode(y32, KA_NEXT, fmt)
        # codes in -> float32: the same values as the float32 interface (decode(encode(x)) is what the layer's own quantizer keeps)
        y = _run(m, lambda: m(xc), xc, name + "+codes_in", q_bit)
        assert y.dtype == torch.float32 and torch.equal(y, hand.codes(xc, None)) and torch.equal(y, y32)
        # codes in -> codes
        m._code_out = out
        y = _run(m, lambda: m(xc), xc, name + "+codes_in+codes_out", q_bit)
        assert y.dtype == torch.uint8 and torch.equal(y, hand.codes(xc, out)) and torch.equal(y, want)
        # float32 -> codes in one launch
        m._code_entry = True
        y = _run(m, lambda: m(x), x, name + "+codes_out", q_bit)
        assert y.dtype == torch.uint8 and torch.equal(y, hand.entry(x, out)) and torch.equal(y, want)
        m._code_entry = False
        # both halves of a 64-channel code buffer
        buf = torch.full((N, 2 * C, HW, HW), 0xA5, dtype=torch.uint8, device=dev).contiguous(memory_format=torch.channels_last)
        buf2 = buf.clone(memory_format=torch.channels_last)
        plans = len(m._plans)
        _run(m, lambda: m.forward_slice(xc, (buf, 0)), xc, name + "+codes_in+codes_out+slice", q_bit)
        assert m.output is buf
        assert m.forward_slice(xc, (buf, C)) is buf and m._last_kernel == name + "+codes_in+codes_out+slice"
        for c_off in (0, C):
            hand.slice(xc, out, buf2, c_off)
        assert len(m._plans) == plans + 1, "both halves share one plan"
        assert torch.equal(buf, buf2) and torch.equal(buf[:, :C], want) and torch.equal(buf[:, C:], want)
        m._code_out = None
        # the residual operand, with and without the ReLU behind the add (the epilogue's own ReLU comes off: it would sit in front)
        m._post = (m._post[0], m._post[1], 0)
        y_lin = m(x).clone(memory_format=torch.channels_last)
        for relu in (False, True):
            m.residual_relu = relu
            y = _run(m, lambda: m(x, residual=r), x, name + "+res", q_bit)
            ref = torch.relu(y_lin + r) if relu else y_lin + r
            assert torch.equal(y, hand.res(x, r, relu)) and torch.equal(y, ref)
            assert m.output is not None and torch.equal(m.output, y)
        assert m._prep.blob is blob, "one weight blob serves every path of the module"


@pytest.mark.parametrize("q_bit", [8, 7])
def test_dense_and_depthwise_routes_on_codes(dev, q_bit):
    from cnns_slfp_quantization_amd import _lib
    from cnns_slfp_quantization_amd.sfp_quant import hip_encode
    fmt = _lib.FMT_ACT8 if q_bit == 8 else _lib.FMT_SFP7
    g = torch.Generator().manual_seed(20 + q_bit)
    x = (torch.randn(N, C, HW, HW, generator=g) * 0.8).to(dev).contiguous(memory_format=torch.channels_last)
    xc = hip_encode(x, KA, fmt)
    out = (KA_NEXT, q_bit)
    with torch.no_grad():
        # dense 3x3, pad 1: codes in -> codes out through the workspace
        m = _layer(dev, q_bit, 3, 1, bias=True, relu=True, seed=30 + q_bit)
        hand = _Hand(m, x.shape)
        assert hand.kernel == DENSE_KERNEL[q_bit] and hand.ws_bytes > 0
        y32 = _run(m, lambda: m(x), x, hand.kernel, q_bit)
        blob = m._prep.blob
        assert torch.equal(y32, hand.post(x))
        m._code_out = out
        y = _run(m, lambda: m(xc), xc, hand.kernel + "+codes_in+codes_out", q_bit)
        assert y.dtype == torch.uint8 and torch.equal(y, hand.codes(xc, out)) and torch.equal(y, hip_encode(y32, KA_NEXT, fmt))
        assert m._prep.blob is blob
        # depthwise 3x3, stride 1 (the family takes no bias): codes in -> codes out and codes in -> float32
        m = _layer(dev, q_bit, 3, C, bias=False, relu=True, seed=40 + q_bit)
        hand = _Hand(m, x.shape)
        assert hand.kernel == "dw3x3_nhwc" and hand.ws_bytes == 0
        y32 = _run(m, lambda: m(x), x, "dw3x3_nhwc", q_bit)
        blob = m._prep.blob
        assert torch.equal(y32, hand.post(x))
        y = _run(m, lambda: m(xc), xc, "dw3x3_nhwc+codes_in", q_bit)
        assert y.dtype == torch.float32 and torch.equal(y, hand.codes(xc, None)) and torch.equal(y, y32)
        m._code_out = out
        y = _run(m, lambda: m(xc), xc, "dw3x3_nhwc+codes_in+codes_out", q_bit)
        assert y.dtype == torch.uint8 and torch.equal(y, hand.codes(xc, out)) and torch.equal(y, hip_encode(y32, KA_NEXT, fmt))
        assert m._prep.blob is blob
