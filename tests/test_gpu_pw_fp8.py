"""GPU (MI355X): SFP<3,3> 1x1 layers on 1-byte codes with E4M3 operands (SLFP_MFMA_FP8, csrc/conv_pw_fp8.hip),
through the C ABI, against the float64 oracle under the SFP<3,3> bar of DESIGN section 2 (max and l2, tensor-relative, 1e-5).

The kernel feeds the tiny class (|x| < 0.0625 Ka: +-1e-10 in the reference) as 0, like the fp16 kernels.  In the scaled domain that
moves an output by at most K * 15 * 1e-10 = 7.7e-7 at K = 512, while max|ref| there is far above 1 (K products of values up to
15 x 15): below 1e-6 of the bar for every shape used here.

One MFMA per k-step missed the bar (max 1.1e-5 .. 2.8e-5: the matrix unit aligns the 8 products of a lane to the largest and
drops low bits); with both operands split by exponent every row measures 0 .. 1.1e-7 (max), 0 .. 4.0e-8 (l2) on an MI355X."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import rel_errors
from oracle import slfp_oracle as so

pytestmark = pytest.mark.gpu
TOL = 1e-5
KA, KW = 0.31, 0.02


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cnns_slfp_quantization_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture
def force_pg(lib):
    def force(pg):
        os.environ["SLFP_PW8_PG"] = str(pg)
        lib.load().slfp_debug_reload_switches()
    yield force
    os.environ.pop("SLFP_PW8_PG", None)
    lib.load().slfp_debug_reload_switches()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _desc(lib, c_in, c_out, n, h, w, qbits=7, mode=None, ka=KA, kw=KW, **over):
    f = dict(n=n, c_in=c_in, h=h, w=w, c_out=c_out, kh=1, kw=1, stride_h=1, stride_w=1, pad_h=0, pad_w=0, dil_h=1, dil_w=1, groups=1,
             x_layout=lib.LAYOUT_NHWC, y_layout=lib.LAYOUT_NHWC, qbits=qbits, ka=float(np.float32(ka)), kw_scale=float(np.float32(kw)),
             mfma_passes=lib.MFMA_FP8 if mode is None else mode, reserved=0)
    f.update(over)
    return lib.ConvDesc(**f)


def _input(shape, seed):
    """about half negative, an eighth exact zeros, an eighth tiny (below 0.0625 Ka), some at or above the clamp 15 Ka"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(shape, generator=g, device="cuda") * (3.0 * KA)
    sel = torch.rand(shape, generator=g, device="cuda")
    x[sel < 0.125] = 0.0
    x[(sel >= 0.125) & (sel < 0.25)] *= 0.01 / 3.0
    x[sel > 0.99] = 17.0 * KA
    return x


def _codes(lib, x, ka=KA):
    c = torch.empty_like(x, dtype=torch.uint8)
    lib.check(lib.load().slfp_encode_f32(x.data_ptr(), c.data_ptr(), x.numel(), float(np.float32(ka)), lib.FMT_SFP7 | lib.FMT_EXT, _st()))
    return c


def _blob(lib, d, w):
    L = lib.load()
    b = torch.empty(L.slfp_conv2d_wprep_bytes(ctypes.byref(d)), dtype=torch.uint8, device="cuda")
    lib.check(L.slfp_conv2d_prepare_weights(ctypes.byref(d), w.data_ptr(), b.data_ptr(), None, _st()))
    return b


def _run(lib, d, xc, blob, bias, post, relu, io, y, y_ld=None):
    p = lambda t: None if t is None else t.data_ptr()
    head = (ctypes.byref(d), ctypes.byref(io), xc.data_ptr(), blob.data_ptr(), p(bias), p(post[0]), p(post[1]), relu)
    L = lib.load()
    if y_ld is None:
        lib.check(L.slfp_conv2d_fwd_codes(*head, y.data_ptr(), _st()))
    else:
        lib.check(L.slfp_conv2d_fwd_codes_slice(*head, y if isinstance(y, int) else y.data_ptr(), y_ld, None, _st()))
    return y


def _layer(lib, c_in, c_out, m, bias, post, seed):
    n, h, w = (1, 5, 7) if m == 35 else (2, 9, 9)
    g = torch.Generator(device="cuda").manual_seed(seed)
    d = _desc(lib, c_in, c_out, n, h, w)
    wt = torch.randn((c_out, c_in, 1, 1), generator=g, device="cuda") * (3.0 * KW)
    b = torch.randn(c_out, generator=g, device="cuda") * 0.2 if bias else None
    ps = (torch.rand(c_out, generator=g, device="cuda") + 0.5, torch.randn(c_out, generator=g, device="cuda") * 0.1) if post else (None, None)
    x = _input((n, h, w, c_in), seed + 1)
    return d, wt, b, ps, x


# c_in, c_out, pixels (35 = 3 groups: a PG = 2 pair half dead, the last group ragged; 162), bias, post, relu, PG, variant
TABLE = [(16, 16, 35, 0, 0, 0, 2, "fp8/ks1/pg2/ns1/f32"), (32, 64, 162, 1, 0, 1, 1, "fp8/ks1/pg1/ns1/f32"),
         (48, 64, 35, 0, 1, 0, 2, "fp8/ks2/pg2/ns1/f32"), (64, 16, 162, 1, 1, 1, 2, "fp8/ks2/pg2/ns1/f32"),
         (96, 16, 35, 0, 0, 0, 1, "fp8/ks3/pg1/ns1/f32"), (384, 64, 35, 1, 0, 0, 2, "fp8/ks12/pg2/ns1/f32"),
         (512, 1000, 35, 1, 0, 1, 1, "fp8/ks16/pg1/ns16/f32"), (512, 256, 162, 0, 1, 0, 2, "fp8/ks16/pg2/ns4/f32")]


@pytest.mark.parametrize("row", TABLE, ids=lambda r: f"{r[0]}-{r[1]}-m{r[2]}-pg{r[6]}")
def test_float32_output_against_the_oracle(lib, force_pg, row):
    c_in, c_out, m, bias, post, relu, pg, variant = row
    force_pg(pg)
    d, wt, b, ps, x = _layer(lib, c_in, c_out, m, bias, post, 100 + c_in + c_out)
    io = lib.ConvIo(x_codes=1, y_codes=0, y_ka=1.0, y_qbits=8)
    assert lib.load().slfp_debug_pw_variant(ctypes.byref(d), ctypes.byref(io), 0, 0, 0).decode() == variant
    y = _run(lib, d, _codes(lib, x), _blob(lib, d, wt), b, ps, relu, io, torch.empty((d.n, d.h, d.w, c_out), device="cuda"))
    ref = so.conv2d(np.ascontiguousarray(x.cpu().numpy().transpose(0, 3, 1, 2)), wt.cpu().numpy(), None if b is None else b.cpu().numpy(),
                    (1, 1), (0, 0), (1, 1), 1, np.float64(d.ka), np.float64(d.kw_scale), 7).astype(np.float64).transpose(0, 2, 3, 1)
    if post:
        ref = ref * ps[0].cpu().numpy().astype(np.float64) + ps[1].cpu().numpy().astype(np.float64)
    if relu:
        ref = np.maximum(ref, 0.0)
    e_max, e_l2 = rel_errors(y.cpu().numpy(), ref)
    print(variant, "max", e_max, "l2", e_l2)
    assert e_max <= TOL and e_l2 <= TOL


def test_every_code_value_once(lib):
    """W = identity, Ka = Kw = 1: pixel i of image 0 holds code byte i in channel i among tiny codes, image 1 among zero codes; the
    output is decode(code) with the tiny class as 0 -- no byte of the 128 can convert wrongly and pass."""
    d = _desc(lib, 128, 128, 2, 1, 128, ka=1.0, kw=1.0)
    xc = torch.zeros((2, 1, 128, 128), dtype=torch.uint8, device="cuda")
    xc[1] = 1
    idx = torch.arange(128, device="cuda")
    xc[:, 0, idx, idx] = idx.to(torch.uint8)
    io = lib.ConvIo(x_codes=1, y_codes=0, y_ka=1.0, y_qbits=8)
    y = _run(lib, d, xc, _blob(lib, d, torch.eye(128, device="cuda").reshape(128, 128, 1, 1).contiguous()), None, (None, None), 0, io,
             torch.empty((2, 1, 128, 128), device="cuda")).cpu().numpy()
    want = so.decode(xc.cpu().numpy(), so.FMT_SFP7 | so.FMT_EXT).astype(np.float64)
    want[np.abs(want) < 1e-9] = 0.0
    e_max, e_l2 = rel_errors(y, want)
    assert e_max <= TOL and e_l2 <= TOL and np.array_equal(y.astype(np.float64), want)


# row of TABLE, ReLU, channels of the wider tensor (0: dense), channel offset
@pytest.mark.parametrize("row,relu,ld,off", [(3, 1, 0, 0), (1, 1, 96, 32), (7, 0, 0, 0)], ids=["dense", "slice", "signed"])
@pytest.mark.parametrize("y_qbits", [7, 8])
def test_code_output_is_the_oracles_encode_of_the_float32_output(lib, force_pg, row, relu, ld, off, y_qbits):
    c_in, c_out, m, bias, post, _, pg, _ = TABLE[row]
    force_pg(pg)
    d, wt, b, ps, x = _layer(lib, c_in, c_out, m, bias, post, 300 + row)
    xc, blob, y_ka = _codes(lib, x), _blob(lib, d, wt), 0.4
    y32 = _run(lib, d, xc, blob, b, ps, relu, lib.ConvIo(x_codes=1, y_codes=0, y_ka=1.0, y_qbits=8), torch.empty((d.n, d.h, d.w, c_out), device="cuda"))
    io = lib.ConvIo(x_codes=1, y_codes=1, y_ka=float(np.float32(y_ka)), y_qbits=y_qbits)
    assert lib.load().slfp_debug_pw_variant(ctypes.byref(d), ctypes.byref(io), 0, 0, ld).decode() == TABLE[row][7].replace("f32", "yc")
    buf = torch.full((d.n, d.h, d.w, ld or c_out), 0xAB, dtype=torch.uint8, device="cuda")
    _run(lib, d, xc, blob, b, ps, relu, io, buf.data_ptr() + off if ld else buf, ld or None)
    want = so.encode(y32.cpu().numpy(), np.float32(y_ka), (so.FMT_SFP7 if y_qbits == 7 else so.FMT_ACT8) | so.FMT_EXT)
    got = buf.cpu().numpy()
    assert np.array_equal(got[..., off:off + c_out], want)
    assert (got[..., :off] == 0xAB).all() and (got[..., off + c_out:] == 0xAB).all()


def test_refusals_return_before_device_work(lib):
    """Every entry point the mode does not serve: SLFP_ERR_UNSUPPORTED, the output untouched."""
    L = lib.load()
    d = _desc(lib, 32, 64, 1, 4, 4)
    dw = _desc(lib, 32, 32, 1, 4, 4, kh=3, kw=3, pad_h=1, pad_w=1, groups=32, mode=lib.MFMA_DEFAULT)
    x = torch.zeros((1, 4, 4, 32), device="cuda")
    blob = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    y = torch.full((1, 4, 4, 64), 7.0, device="cuda")
    v = torch.ones(64, device="cuda")
    f32 = lib.ConvIo(x_codes=0, y_codes=0, y_ka=1.0, y_qbits=8)
    cin = lib.ConvIo(x_codes=1, y_codes=0, y_ka=1.0, y_qbits=8)
    cio = lib.ConvIo(x_codes=1, y_codes=1, y_ka=0.5, y_qbits=7)
    ent = lib.ConvIo(x_codes=0, y_codes=1, y_ka=0.5, y_qbits=7)
    D, X, B, Y, V, S, I = ctypes.byref(d), x.data_ptr(), blob.data_ptr(), y.data_ptr(), v.data_ptr(), _st(), ctypes.byref
    calls = [L.slfp_conv2d_fwd(D, X, B, None, Y, None, None, S), L.slfp_conv2d_fwd_post(D, X, B, None, None, None, 0, Y, None, None, S),
             L.slfp_conv2d_fwd_codes(D, I(f32), X, B, None, None, None, 0, Y, S),          # float32 in
             L.slfp_conv2d_fwd_codes(D, I(cin), X, B, None, None, None, 2, Y, S),   # the layer-output bit
             L.slfp_conv2d_fwd_res(D, I(cin), X, B, None, None, None, 0, X, Y, None, S),
             L.slfp_conv2d_fwd_res_codes(D, I(cio), X, B, None, None, None, 0, X, Y, B, None, S),
             L.slfp_conv2d_fwd_codes_lut(D, I(cio), X, B, None, V, V, B, Y, 64, None, S),
             L.slfp_conv2d_fwd_codes_x3(D, I(cin), X, B, None, None, None, 0, Y, S),
             L.slfp_conv2d_fwd_entry(D, I(ent), X, B, None, None, None, 0, Y, S),
             L.slfp_conv2d_fwd_u8(D, I(f32), X, V, B, None, None, None, 0, Y, None, S),
             L.slfp_dwpw_fwd(ctypes.byref(dw), D, X, B, None, None, 0, B, None, None, None, 0, Y, S),
             L.slfp_dwpw_fwd_codes(ctypes.byref(dw), D, I(cin), X, B, None, None, 0, B, None, None, None, 0, Y, S),
             L.slfp_linear_fwd_prepared(X, B, None, Y, 16, 32, 64, 0.31, 0.02, 7, lib.MFMA_FP8, S),
             L.slfp_linear_prepare_weights(X, Y, 32, 64, 0.02, 7, lib.MFMA_FP8, S),
             L.slfp_linear_fwd_fc(X, X, None, Y, 16, 32, 64, 0.31, 0.02, 7, lib.MFMA_FP8, I(cin), 0, None, S),
             L.slfp_conv2d_bwd(D, X, X, Y, Y, None, None, None, S),
             L.slfp_conv2d_fwd_codes(ctypes.byref(_desc(lib, 32, 64, 1, 4, 4, qbits=8)), I(cin), X, B, None, None, None, 0, Y, S)]   # q_bit 8
    assert calls == [lib.ERR_UNSUPPORTED] * len(calls)
    torch.cuda.synchronize()
    assert (y == 7.0).all()
    assert L.slfp_conv2d_codes_supported(D, I(cin), 1, 1) == 1 and L.slfp_conv2d_codes_slice_supported(D, I(cio), 0, 1, 96) == 1
