"""GPU (MI355X): the opt-in depthwise 5x5 / 7x7 kernel (csrc/conv_dwk.hip) at the smallest shapes at which its tiles, units, ragged
channel group, de-interleaved stride-2 columns and halo loader can go wrong, straight through the C ABI: bit for bit against the
direct kernel on the same inputs (the same descriptor with `reserved` = 0), against the CPU oracle under the project's bar for
float32-exact paths (1e-5 tensor-relative), run to run, and -- with NaNs planted in x -- against the direct kernel's NaN mask, which
it must equal exactly.  One case runs Conv2d_Q itself under options.depthwise = "kxk"."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_errors, same_bits
from oracle import slfp_oracle as so
from test_dwk_host import KA, KW, ROWS, row_desc

pytestmark = pytest.mark.gpu

BAR = 1e-5


@pytest.fixture(scope="module")
def lib():
    from cnns_slfp_quantization_amd import _lib
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _forward(lib, d, x, w, bias, post=None):
    """slfp_conv2d_fwd_post of descriptor d with a blob and a workspace of its own; post: (scale, shift) + ReLU"""
    L = lib.load()
    ho, wo = ctypes.c_int64(), ctypes.c_int64()
    lib.check(L.slfp_conv2d_out_shape(ctypes.byref(d), ctypes.byref(ho), ctypes.byref(wo)))
    blob = torch.empty(L.slfp_conv2d_wprep_bytes(ctypes.byref(d)), dtype=torch.uint8, device=x.device)
    lib.check(L.slfp_conv2d_prepare_weights(ctypes.byref(d), w.data_ptr(), blob.data_ptr(), None, _stream()))
    ws = torch.empty(max(L.slfp_conv2d_workspace_bytes(ctypes.byref(d)), 16), dtype=torch.uint8, device=x.device)
    y = torch.empty((d.n, ho.value, wo.value, d.c_out), device=x.device)
    ps, psh = (post[0].data_ptr(), post[1].data_ptr()) if post else (None, None)
    lib.check(L.slfp_conv2d_fwd_post(ctypes.byref(d), x.data_ptr(), blob.data_ptr(), bias.data_ptr(), ps, psh, 1 if post else 0,
                                     y.data_ptr(), None, ws.data_ptr(), _stream()))
    return y.cpu().numpy()


@pytest.mark.parametrize("qbits", [8, 7])
@pytest.mark.parametrize("name", ROWS)
def test_dwk_row(lib, name, qbits):
    k, s, pad, c, h, w_, with_post, variant = ROWS[name]
    dev = torch.device("cuda:0")
    L = lib.load()
    d, d_direct = row_desc(lib, name, qbits), row_desc(lib, name, qbits, reserved=0)
    assert L.slfp_conv2d_kernel_name(ctypes.byref(d)).decode() == "dwk_nhwc"
    assert L.slfp_debug_dwk_variant(ctypes.byref(d)).decode() == variant
    assert L.slfp_conv2d_kernel_name(ctypes.byref(d_direct)).decode() == "direct_nhwc"

    gen = torch.Generator(device=dev).manual_seed(4800 + c + h + k)
    x = torch.relu(torch.randn((2, h, w_, c), generator=gen, device=dev)) * (5.0 * KA)
    w = torch.randn((c, 1, k, k), generator=gen, device=dev) * (4.0 * KW)
    bias = torch.randn(c, generator=gen, device=dev) * 0.3
    post = (torch.rand(c, generator=gen, device=dev) + 0.5, torch.randn(c, generator=gen, device=dev) * 0.3) if with_post else None

    ref = so.conv2d(x.permute(0, 3, 1, 2).contiguous().cpu().numpy(), w.cpu().numpy(), bias.cpu().numpy(), s, pad, 1, c, KA, KW, qbits)
    ref = ref.transpose(0, 2, 3, 1)
    if post:
        ref = np.maximum(ref * post[0].cpu().numpy() + post[1].cpu().numpy(), np.float32(0))
    y = _forward(lib, d, x, w, bias, post)
    emax, el2 = rel_errors(y, ref)
    print(f"{name} q{qbits}: {variant} max-rel {emax:.3e} l2 {el2:.3e}")
    assert same_bits(y, _forward(lib, d_direct, x, w, bias, post)), "bit-equal to the direct kernel"
    assert y.shape == ref.shape and emax <= BAR and el2 <= BAR, (name, emax, el2)
    assert same_bits(_forward(lib, d, x, w, bias, post), y), "run to run"

    # a NaN marks its own channel at the pixels whose window holds it: the direct kernel's mask exactly (no ReLU, which would drop it)
    x_nan = x.clone()
    x_nan.view(-1)[13::1009] = float("nan")
    m, m_direct = np.isnan(_forward(lib, d, x_nan, w, bias)), np.isnan(_forward(lib, d_direct, x_nan, w, bias))
    assert m.any() and not m.all() and np.array_equal(m, m_direct), (name, int(m.sum()), int(m_direct.sum()))


@pytest.mark.parametrize("layout", ["channels_last", "nchw"])
def test_conv2d_q_under_the_option(lib, layout):
    from cnns_slfp_quantization_amd import conv2d_func as cf, fusion
    dev = torch.device("cuda:0")
    mod = cf.conv2d_Q(8, KW, KA)(64, 64, 5, padding=2, groups=64).eval().to(dev)
    gen = torch.Generator(device=dev).manual_seed(4848)
    x = torch.relu(torch.randn((2, 64, 14, 18), generator=gen, device=dev)) * (5.0 * KA)
    with torch.no_grad():
        mod.weight.copy_(torch.randn(mod.weight.shape, generator=gen, device=dev) * (4.0 * KW))
    xin = x.contiguous(memory_format=torch.channels_last) if layout == "channels_last" else x
    ref = so.conv2d(x.cpu().numpy(), mod.weight.detach().cpu().numpy(), None, 1, 2, 1, 64, KA, KW, 8)
    try:
        cf.options.depthwise = "kxk"
        with torch.no_grad():
            y = mod(xin)
        assert mod._last_kernel == "dwk_nhwc"
        emax, el2 = rel_errors(y.cpu().numpy(), ref)
        assert emax <= BAR and el2 <= BAR, (emax, el2)
        # [Conv2d_Q, BatchNorm2d, ReLU] fused by fuse_bn_relu: the same kernel, the affine and the ReLU in its epilogue
        bn = torch.nn.BatchNorm2d(64).to(dev)
        with torch.no_grad():
            bn.running_mean.copy_(torch.randn(64, generator=gen, device=dev) * 0.3)
            bn.running_var.copy_(torch.rand(64, generator=gen, device=dev) + 0.5)
        seq = torch.nn.Sequential(mod, bn, torch.nn.ReLU()).eval()
        ref_seq = torch.relu(bn.cpu()(torch.from_numpy(ref))).detach().numpy()
        assert fusion.fuse_bn_relu(seq) == 1
        with torch.no_grad():
            ys = seq(xin)
        assert mod._last_kernel == "dwk_nhwc"
        emax, el2 = rel_errors(ys.cpu().numpy(), ref_seq)
        assert emax <= BAR and el2 <= BAR, (emax, el2)
    finally:
        cf.options.depthwise = "direct"
    with torch.no_grad():
        seq(xin)
    assert mod._last_kernel == "direct_nhwc"
