"""GPU (MI355X): the bf16 pointwise backward (csrc/conv_bwd_bf16.hip) through the C ABI, slfp_conv2d_bwd_bf16, against the float64
reference of tests/_bwd_cases.py (torch.nn.grad contractions of the C oracle's xq / wq) under the project's bars: elementwise
|d| / sum|terms| <= 1e-5 and tensor-relative L2 <= 1e-6 for gx, gw and gb.  gy is seeded, spread over 2^+-20, with exact zeros,
one-bit values and values with all 24 significand bits set: the edge cases of the three-way split.  Every output and a workspace of
exactly the stated size sit between 0xA5 bands that must stay untouched."""
import ctypes
import functools
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from _bwd_cases import _errors, _reference, _x_values
from cnns_slfp_quantization_amd import _lib
from cnns_slfp_quantization_amd import conv2d_func as cf

pytestmark = pytest.mark.gpu
DEV = "cuda"
KA, KW = 0.2, 0.1
GUARD = 4096
# n, H, W, C_in, C_out
ROWS = [(2, 3, 5, 8, 8),          # below one MFMA tile in every dimension, M = 30
        (5, 1, 1, 40, 24),        # Linear_Q form, M below one k-step, K = 24 for gx
        (2, 9, 7, 24, 40),        # M = 126, one short of a 128-row tile; ragged channel tiles
        (1, 13, 10, 136, 72),     # M = 130, one past; C_in eight past a 128 tile
        (2, 17, 17, 64, 128),     # M = 578: two gw splits, a short last one, a partial last k-step
        (300, 1, 1, 256, 1000)]   # classifier form, ragged 1000
NEEDS = ((1, 1, 1), (1, 1, 0), (0, 1, 1), (0, 1, 0), (1, 0, 0))   # (gx, gw, gb): gb is computed together with gw


def _desc(row, q):
    n, h, w, ci, co = row
    return _lib.ConvDesc(n=n, c_in=ci, h=h, w=w, c_out=co, kh=1, kw=1, stride_h=1, stride_w=1, pad_h=0, pad_w=0, dil_h=1, dil_w=1,
                         groups=1, x_layout=_lib.LAYOUT_NHWC, y_layout=_lib.LAYOUT_NHWC, qbits=q, ka=float(np.float32(KA)),
                         kw_scale=float(np.float32(KW)), mfma_passes=0, reserved=0)


def _gy_values(shape, gen):
    g = torch.exp2(torch.empty(shape).uniform_(-20, 20, generator=gen)) * torch.empty(shape).uniform_(1, 2, generator=gen)
    g = g * torch.where(torch.rand(shape, generator=gen) < 0.5, -1.0, 1.0)
    kind = torch.rand(shape, generator=gen)
    bits = g.float().view(torch.int32)
    bits = torch.where(kind < 0.05, bits & ~0x7FFFFF, bits)                     # one significant bit
    bits = torch.where((kind >= 0.05) & (kind < 0.10), bits | 0x7FFFFF, bits)   # all 24 set
    g = bits.view(torch.float32).clone()
    g[(kind >= 0.10) & (kind < 0.15)] = 0.0
    return g


@functools.lru_cache(maxsize=None)
def _case(row, q):
    """Seeded inputs (NCHW on the CPU, NHWC on the device, x also as codes) and the float64 reference; made once, never written."""
    n, h, w, ci, co = row
    gen = torch.Generator().manual_seed(9000 + 13 * ci + 7 * co + n + q)
    x = _x_values((n, ci, h, w), KA, gen)
    wt = torch.randn((co, ci, 1, 1), generator=gen) * (2.0 / ci) ** 0.5
    gy = _gy_values((n, co, h, w), gen)
    mod = SimpleNamespace(q_bit=q, Ka=KA, Kw=KW, stride=(1, 1), padding=(0, 0), dilation=(1, 1), groups=1)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)   # noqa: E731
    c = SimpleNamespace(row=row, q=q, x=nhwc(x), w=wt.to(DEV), gy=nhwc(gy), gy_cpu=gy, x_cpu=x, mod=mod, ref=_reference(x, wt, gy, mod))
    c.codes = torch.empty(c.x.shape, dtype=torch.uint8, device=DEV)
    fmt = (_lib.FMT_ACT8 if q == 8 else _lib.FMT_SFP7) | _lib.FMT_EXT
    _lib.check(_lib.load().slfp_encode_f32(c.x.data_ptr(), c.codes.data_ptr(), c.codes.numel(), float(np.float32(KA)), fmt,
                                           torch.cuda.current_stream().cuda_stream))
    return c


def _banded(nbytes):
    buf = torch.full((2 * GUARD + nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf, buf[GUARD:GUARD + nbytes]


def _launch(c, codes, need=(1, 1, 1), gy=None):
    """One slfp_conv2d_bwd_bf16 call: [gx, gw, gb] as NCHW / OIHW / [C_out] CPU tensors (None: not asked for)."""
    L, d = _lib.load(), _desc(c.row, c.q)
    n, h, w, ci, co = c.row
    shapes = ((n, h, w, ci), (co, ci, 1, 1), (co,))
    bufs = [_banded(4 * int(np.prod(s))) for s in shapes]
    nbytes = L.slfp_conv2d_bwd_bf16_workspace_bytes(ctypes.byref(d), 0, need[0], need[1])
    assert nbytes > 0
    ws = _banded(nbytes)
    ptr = lambda k: bufs[k][1].data_ptr() if need[k] else None   # noqa: E731
    gy = c.gy if gy is None else gy
    _lib.check(L.slfp_conv2d_bwd_bf16(ctypes.byref(d), 0, None if codes else c.x.data_ptr(), c.codes.data_ptr() if codes else None,
                                      c.w.data_ptr(), gy.data_ptr(), ptr(0), ptr(1), ptr(2), ws[1].data_ptr(),
                                      torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    out = []
    for k, ((buf, view), s) in enumerate(zip(bufs + [ws], shapes + (None,))):
        assert bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + view.numel():] == 0xA5).all()), ("band", k)
        if s is None:
            break
        if not need[k]:
            assert bool((view == 0xA5).all()), ("not asked for, written", k)
        t = view.view(torch.float32).view(s).cpu()
        out.append((t.permute(0, 3, 1, 2) if k == 0 else t) if need[k] else None)
    return out


@pytest.mark.parametrize("q", [8, 7])
@pytest.mark.parametrize("row", ROWS, ids=lambda r: "x".join(map(str, r)))
def test_against_float64_codes_and_twice(row, q):
    c = _case(row, q)
    got = _launch(c, False)
    errs = [_errors(g, r) for g, r in zip(got, c.ref)]
    print(f"\nbf16x3 {row} q{q}: " + "  ".join(f"{name} elem {e:.2e} l2 {l:.2e}" for name, (e, l) in zip(("gx", "gw", "gb"), errs)))
    for e, l in errs:
        assert e <= 1e-5 and l <= 1e-6, errs
    for other in (_launch(c, False), _launch(c, True)):   # a second call; x as codes: the same bits
        for a, b in zip(got, other):
            assert torch.equal(a, b)


def test_m578_runs_two_splits_with_a_short_last_one_and_a_partial_kstep():
    s = _lib.load().slfp_debug_bwd_bf16_instance(ctypes.byref(_desc(ROWS[4], 8)), 0, 0, 1, 1).decode()
    p, k = map(int, re.search(r"/p(\d+)k(\d+)$", s).groups())
    last = 578 - (p - 1) * k
    assert p >= 2 and 0 < last < k and last % 32 != 0 and k % 32 != 0, s


@pytest.mark.parametrize("row", [ROWS[2], ROWS[4]], ids=lambda r: "x".join(map(str, r)))
def test_need_subsets(row):
    c = _case(row, 8)
    full = _launch(c, True)
    for need in NEEDS[1:]:
        for codes in (False, True):
            got = _launch(c, codes, need)
            for k in range(3):
                assert (got[k] is None) == (not need[k])
                assert got[k] is None or torch.equal(got[k], full[k]), (need, codes, k)


@pytest.mark.parametrize("codes", [False, True], ids=["f32", "codes"])
@pytest.mark.parametrize("row", [ROWS[2], ROWS[4]], ids=lambda r: "x".join(map(str, r)))
def test_inf_and_nan_in_gy_reach_the_elements_the_reference_says(row, codes):
    c = _case(row, 8)
    gy = c.gy_cpu.clone()
    gy[0, 3, 2, 1] = float("inf")
    gy[1, 17, 8, 6] = float("nan")
    ref = _reference(c.x_cpu, c.w.cpu(), gy, c.mod)
    got = _launch(c, codes, gy=gy.permute(0, 2, 3, 1).contiguous().to(DEV))
    for g, (r, _) in zip(got, ref):
        assert (~torch.isfinite(r)).any() and torch.isfinite(r).any()
        assert torch.equal(~torch.isfinite(g), ~torch.isfinite(r))


def test_modules_take_the_kernel_where_it_covers_the_layer():
    gen = torch.Generator().manual_seed(11)
    pw = cf.conv2d_Q_bias(8, KW, KA)(24, 40, 1).to(DEV)
    dw = cf.conv2d_Q(8, KW, KA)(24, 24, 3, padding=1, groups=24, bias=False).to(DEV)
    lin = cf.linear_Q(8, KW, KA)(40, 24).to(DEV)
    x = _x_values((2, 24, 9, 7), KA, gen).to(DEV).contiguous(memory_format=torch.channels_last)
    try:
        cf.options.backward = "hip"
        for gemm in ("f32", "bf16x3"):
            cf.options.backward_gemm = gemm
            for m in (pw, dw, lin):
                m.zero_grad(set_to_none=True)
            y = pw(dw(x.clone().requires_grad_(True)))
            y.backward(torch.randn_like(y))   # a channels_last gy (NCHW is the float32 kernels')
            lin(y.detach()[:, :, 0, 0].contiguous().requires_grad_(True)).square().sum().backward()
            name = "pw_bwd_mfma_f32" if gemm == "f32" else "pw_bwd_mfma_bf16x3"
            assert (pw._last_bwd_kernel, lin._last_bwd_kernel, dw._last_bwd_kernel) == (name, name, "dw3x3_bwd")
    finally:
        cf.options.backward, cf.options.backward_gemm = "composite", "f32"
