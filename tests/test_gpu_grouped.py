"""GPU (MI355X): the opt-in grouped kernel (csrc/conv_grouped.hip) at the smallest shapes at which its group sets, ragged last
set, flattened contraction and halo loader can go wrong, straight through the C ABI: against the CPU oracle under the project's
bars (1e-3 tensor-relative for f16x1, 1e-5 for the exact SFP<3,3> mode), run to run, and -- with NaNs planted in x -- against
the NaN mask of the direct kernel widened from groups to group sets (the documented difference).  One case runs Conv2d_Q itself
under options.grouped = "mfma"."""
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import rel_errors, same_bits
from oracle import slfp_oracle as so

pytestmark = pytest.mark.gpu

KA, KW = 0.21, 0.027
BAR = {"grouped_mfma_f16x1": 1e-3, "grouped_mfma_f16_exact": 1e-5}

# (C_in, C_out, groups, H, W, kernel, stride, padding, post-op?, the selection the launch must report at n = 2)
ROWS = {
    "two_sets_two_taps_per_step": (32, 32, 8, 13, 19, 3, 1, 1, False, "gs4/sp16/nt1/ks5/sw2/wk4"),
    "ragged_last_set": (24, 24, 6, 13, 19, 3, 1, 1, False, "gs4/sp16/nt1/ks5/sw2/wk4"),      # 2 of 4 groups: guarded loads and stores
    "og16_stride2_odd_sets": (80, 80, 5, 13, 19, 3, 2, 1, False, "gs1/sp16/nt1/ks5/sw2/wk1"),
    "set64_lds_maximum": (128, 128, 2, 9, 11, 3, 2, 1, False, "gs1/sp64/nt4/ks18/sw1/wk1"),
    "og24_k_ends_mid_step": (96, 96, 4, 9, 11, 3, 1, 1, False, "gs2/sp48/nt3/ks14/sw1/wk2"),  # K = 432
    "cg_ne_og_no_padding": (32, 64, 4, 8, 9, 3, 1, 0, False, "gs1/sp8/nt1/ks3/sw4/wk1"),
    "og4_cg16_span64": (64, 16, 4, 8, 9, 3, 1, 1, False, "gs4/sp64/nt1/ks18/sw1/wk1"),
    "grouped_1x1_half_step": (64, 64, 4, 7, 7, 1, 1, 0, False, "gs1/sp16/nt1/ks1/sw2/wk1"),   # K = 16
    "taps25": (32, 32, 4, 10, 12, 5, 1, 2, False, "gs2/sp16/nt1/ks13/sw2/wk2"),
    "image_smaller_than_tile": (32, 32, 8, 3, 3, 3, 1, 1, False, "gs4/sp16/nt1/ks5/sw2/wk1"),
    "post_op": (32, 32, 8, 13, 19, 3, 1, 1, True, "gs4/sp16/nt1/ks5/sw2/wk4"),              # bias, BN scale / shift, ReLU
}


def row_desc(lib, name, qbits=8, reserved=None, **change):
    c, o, g, h, w_, k, s, pad = ROWS[name][:8]
    f = dict(n=2, c_in=c, h=h, w=w_, c_out=o, kh=k, kw=k, stride_h=s, stride_w=s, pad_h=pad, pad_w=pad, dil_h=1, dil_w=1, groups=g,
             x_layout=lib.LAYOUT_NHWC, y_layout=lib.LAYOUT_NHWC, qbits=qbits, ka=float(np.float32(KA)), kw_scale=float(np.float32(KW)),
             mfma_passes=lib.MFMA_F16X1, reserved=lib.DESC_GROUPED_MFMA if reserved is None else reserved)
    f.update(change)
    return lib.ConvDesc(**f)


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
def test_grouped_row(lib, name, qbits):
    c, o, g, h, w_, k, s, pad, with_post, variant = ROWS[name]
    dev = torch.device("cuda:0")
    L = lib.load()
    d, d_direct = row_desc(lib, name, qbits), row_desc(lib, name, qbits, reserved=0)
    kern = L.slfp_conv2d_kernel_name(ctypes.byref(d)).decode()
    assert kern == ("grouped_mfma_f16x1" if qbits == 8 else "grouped_mfma_f16_exact")
    assert L.slfp_debug_grouped_variant(ctypes.byref(d)).decode() == variant
    assert L.slfp_conv2d_kernel_name(ctypes.byref(d_direct)).decode() == "direct_nhwc"

    gen = torch.Generator(device=dev).manual_seed(4700 + c + o + h)
    x = torch.relu(torch.randn((2, h, w_, c), generator=gen, device=dev)) * (5.0 * KA)
    w = torch.randn((o, c // g, k, k), generator=gen, device=dev) * (4.0 * KW)
    bias = torch.randn(o, generator=gen, device=dev) * 0.3
    post = (torch.rand(o, generator=gen, device=dev) + 0.5, torch.randn(o, generator=gen, device=dev) * 0.3) if with_post else None

    ref = so.conv2d(x.permute(0, 3, 1, 2).contiguous().cpu().numpy(), w.cpu().numpy(), bias.cpu().numpy(), s, pad, 1, g, KA, KW, qbits)
    ref = ref.transpose(0, 2, 3, 1)
    if post:
        ref = np.maximum(ref * post[0].cpu().numpy() + post[1].cpu().numpy(), np.float32(0))
    y = _forward(lib, d, x, w, bias, post)
    emax, el2 = rel_errors(y, ref)
    print(f"{name} q{qbits}: {variant} {kern} max-rel {emax:.3e} l2 {el2:.3e}")
    assert y.shape == ref.shape and emax <= BAR[kern] and el2 <= BAR[kern], (name, emax, el2)
    assert same_bits(_forward(lib, d, x, w, bias, post), y), "run to run"

    # a NaN reaches every channel of its group SET at the pixels whose window holds it: the direct kernel's mask (no ReLU, which
    # would drop it), widened from groups to sets of gs = 16 / gcd(Og, 16) groups
    x_nan = x.clone()
    x_nan.view(-1)[13::1009] = float("nan")
    m, m_direct = np.isnan(_forward(lib, d, x_nan, w, bias)), np.isnan(_forward(lib, d_direct, x_nan, w, bias))
    width = 16 // math.gcd(o // g, 16) * (o // g)
    sets = -(-o // width)
    wide = np.pad(m_direct, [(0, 0)] * 3 + [(0, sets * width - o)]).reshape(m.shape[:3] + (sets, width)).any(-1, keepdims=True)
    wide = np.broadcast_to(wide, m.shape[:3] + (sets, width)).reshape(m.shape[:3] + (sets * width,))[..., :o]
    assert m.any() and not m.all() and np.array_equal(m, wide), (name, int(m.sum()), int(wide.sum()))


@pytest.mark.parametrize("layout", ["channels_last", "nchw"])
def test_conv2d_q_under_the_option(lib, layout):
    from cnns_slfp_quantization_amd import conv2d_func as cf, fusion
    dev = torch.device("cuda:0")
    mod = cf.conv2d_Q(8, KW, KA)(64, 64, 3, padding=1, groups=16).eval().to(dev)
    gen = torch.Generator(device=dev).manual_seed(4747)
    x = torch.relu(torch.randn((2, 64, 14, 18), generator=gen, device=dev)) * (5.0 * KA)
    with torch.no_grad():
        mod.weight.copy_(torch.randn(mod.weight.shape, generator=gen, device=dev) * (4.0 * KW))
    xin = x.contiguous(memory_format=torch.channels_last) if layout == "channels_last" else x
    ref = so.conv2d(x.cpu().numpy(), mod.weight.detach().cpu().numpy(), None, 1, 1, 1, 16, KA, KW, 8)
    try:
        cf.options.grouped = "mfma"
        with torch.no_grad():
            y = mod(xin)
        assert mod._last_kernel == "grouped_mfma_f16x1"
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
        assert mod._last_kernel == "grouped_mfma_f16x1"
        emax, el2 = rel_errors(ys.cpu().numpy(), ref_seq)
        assert emax <= 1e-3 and el2 <= 1e-3, (emax, el2)
    finally:
        cf.options.grouped = "direct"
    with torch.no_grad():
        seq(xin)
    assert mod._last_kernel == "direct_nhwc"
