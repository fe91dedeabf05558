"""GPU (MI355X): the opt-in dilated dense kernel (csrc/conv_dense_dil.hip) at the smallest shapes at which its phase tiling can
go wrong, straight through the C ABI: against the CPU oracle under the project's bars (1e-3 tensor-relative for f16x1, 1e-5 for
the exact SFP<3,3> mode), run to run, and -- with NaNs planted in x -- against the NaN mask of the direct kernel, which marks
exactly the outputs whose receptive field holds one.  One case runs Conv2d_Q itself under options.dilated = "mfma"."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_errors, same_bits
from oracle import slfp_oracle as so

pytestmark = pytest.mark.gpu

KA, KW = 0.21, 0.027
BAR = {"dense_dil_mfma_f16x1": 1e-3, "dense_dil_mfma_f16_exact": 1e-5}

# (C_in, C_out, H, W, kernel, dilation, padding, post-op?, the selection the launch must report)
ROWS = {
    "ragged_phases": (64, 32, 13, 19, (3, 3), (2, 2), (2, 2), False, "16x1/811/ns3"),      # phase grids of 7/6 rows, 10/9 columns
    "channel_tails": (80, 20, 13, 19, (3, 3), (2, 2), (2, 2), False, "16x1/811/ns3"),      # tail inside a chunk; C_out % 16 != 0
    "two_chunks_two_slices": (128, 136, 9, 37, (3, 3), (2, 2), (2, 2), False, "8x2/421/ns3"),   # halo double buffer; 19-column phase grid
    "one_pixel_phases": (64, 32, 5, 7, (3, 3), (4, 4), (4, 4), False, "8x2/421/ns3"),      # dilation close to the image size
    "workload_7x7": (64, 64, 28, 28, (3, 3), (4, 4), (4, 4), False, "8x2/421/ns3"),        # the 7 x 7 phase grid of layer4
    "anisotropic": (32, 48, 12, 20, (3, 3), (3, 2), (0, 1), False, "16x1/421/ns3"),        # output smaller than input
    "one_axis_undilated": (32, 48, 12, 19, (1, 3), (1, 2), (0, 2), False, "16x1/811/ns3"),  # a single tap row, two taps in flight
    "post_op": (64, 32, 13, 19, (3, 3), (2, 2), (2, 2), True, "16x1/811/ns3"),             # bias, BN scale / shift, ReLU
    "two_rows_per_wave": (16, 128, 16, 32, (3, 3), (2, 2), (2, 2), False, "16x1/422/ns3"),  # the MT = 2 tiling; C_in below a chunk
    "nine_slots_5x5": (32, 32, 16, 20, (5, 5), (2, 2), (4, 4), False, "16x1/811/ns9"),     # a halo of more than 24 pieces
}


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
def test_dilated_row(lib, name, qbits):
    c, o, h, w_, k, dil, pad, with_post, variant = ROWS[name]
    dev = torch.device("cuda:0")
    L = lib.load()
    f = dict(n=2, c_in=c, h=h, w=w_, c_out=o, kh=k[0], kw=k[1], stride_h=1, stride_w=1, pad_h=pad[0], pad_w=pad[1], dil_h=dil[0],
             dil_w=dil[1], groups=1, x_layout=lib.LAYOUT_NHWC, y_layout=lib.LAYOUT_NHWC, qbits=qbits, ka=float(np.float32(KA)),
             kw_scale=float(np.float32(KW)), mfma_passes=lib.MFMA_F16X1)
    d, d_direct = lib.ConvDesc(reserved=lib.DESC_DILATED_MFMA, **f), lib.ConvDesc(reserved=0, **f)
    kern = L.slfp_conv2d_kernel_name(ctypes.byref(d)).decode()
    assert kern == ("dense_dil_mfma_f16x1" if qbits == 8 else "dense_dil_mfma_f16_exact")
    assert L.slfp_debug_dense_dil_variant(ctypes.byref(d)).decode() == variant
    assert L.slfp_conv2d_kernel_name(ctypes.byref(d_direct)).decode() == "direct_nhwc"

    gen = torch.Generator(device=dev).manual_seed(4600 + c + o + h)
    x = torch.relu(torch.randn((2, h, w_, c), generator=gen, device=dev)) * (5.0 * KA)
    w = torch.randn((o, c, k[0], k[1]), generator=gen, device=dev) * (4.0 * KW)
    bias = torch.randn(o, generator=gen, device=dev) * 0.3
    post = (torch.rand(o, generator=gen, device=dev) + 0.5, torch.randn(o, generator=gen, device=dev) * 0.3) if with_post else None

    ref = so.conv2d(x.permute(0, 3, 1, 2).contiguous().cpu().numpy(), w.cpu().numpy(), bias.cpu().numpy(), 1, pad, dil, 1, KA, KW, qbits)
    ref = ref.transpose(0, 2, 3, 1)
    if post:
        ref = np.maximum(ref * post[0].cpu().numpy() + post[1].cpu().numpy(), np.float32(0))
    y = _forward(lib, d, x, w, bias, post)
    emax, el2 = rel_errors(y, ref)
    print(f"{name} q{qbits}: {variant} {kern} max-rel {emax:.3e} l2 {el2:.3e}")
    assert y.shape == ref.shape and emax <= BAR[kern] and el2 <= BAR[kern], (name, emax, el2)
    assert same_bits(_forward(lib, d, x, w, bias, post), y), "run to run"

    # a NaN reaches exactly the outputs whose receptive field holds it: the direct kernel's mask (no ReLU, which would drop it)
    x_nan = x.clone()
    x_nan.view(-1)[13::1009] = float("nan")
    m, m_direct = np.isnan(_forward(lib, d, x_nan, w, bias)), np.isnan(_forward(lib, d_direct, x_nan, w, bias))
    assert m.any() and not m.all() and np.array_equal(m, m_direct), (name, int(m.sum()), int(m_direct.sum()))


@pytest.mark.parametrize("layout", ["channels_last", "nchw"])
def test_conv2d_q_under_the_option(lib, layout):
    from cnns_slfp_quantization_amd import conv2d_func as cf, fusion
    dev = torch.device("cuda:0")
    mod = cf.conv2d_Q(8, KW, KA)(64, 64, 3, padding=2, dilation=2).eval().to(dev)
    gen = torch.Generator(device=dev).manual_seed(4646)
    x = torch.relu(torch.randn((2, 64, 14, 18), generator=gen, device=dev)) * (5.0 * KA)
    with torch.no_grad():
        mod.weight.copy_(torch.randn(mod.weight.shape, generator=gen, device=dev) * (4.0 * KW))
    xin = x.contiguous(memory_format=torch.channels_last) if layout == "channels_last" else x
    ref = so.conv2d(x.cpu().numpy(), mod.weight.detach().cpu().numpy(), None, 1, 2, 2, 1, KA, KW, 8)
    try:
        cf.options.dilated = "mfma"
        with torch.no_grad():
            y = mod(xin)
        assert mod._last_kernel == "dense_dil_mfma_f16x1"
        emax, el2 = rel_errors(y.cpu().numpy(), ref)
        assert emax <= 1e-3 and el2 <= 1e-3, (emax, el2)
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
        assert mod._last_kernel == "dense_dil_mfma_f16x1"
        emax, el2 = rel_errors(ys.cpu().numpy(), ref_seq)
        assert emax <= 1e-3 and el2 <= 1e-3, (emax, el2)
    finally:
        cf.options.dilated = "direct"
    with torch.no_grad():
        seq(xin)
    assert mod._last_kernel == "direct_nhwc"
