"""GPU (MI355X): the bf16 dense backward (csrc/conv_bwd_dense_bf16.hip) through the C ABI, slfp_conv2d_bwd_dense_bf16, against the
float64 reference of tests/_bwd_cases.py under the project's bars: elementwise |d| / sum|terms| <= 1e-5 and tensor-relative L2 <= 1e-6
for gx, gw and gb.  gy, the 0xA5 bands and the need subsets are those of tests/test_gpu_bwd_bf16.py."""
import ctypes
import functools
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from _bwd_cases import _errors, _reference, _x_values
from test_gpu_bwd_bf16 import GUARD, KA, KW, NEEDS, _banded, _gy_values
from cnns_slfp_quantization_amd import _lib
from cnns_slfp_quantization_amd import conv2d_func as cf

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLAGS = _lib.BWD_DENSE
# n, H, W, C_in, C_out, (kh, kw), (s_h, s_w), (pad_h, pad_w)
ROWS = [(2, 5, 7, 8, 8, (3, 3), (1, 1), (1, 1)),        # below one tile in every dimension; every tap clipped at some row
        (1, 9, 11, 24, 40, (3, 3), (2, 2), (1, 1)),     # odd extents, four unequal phases, taps skipped per phase, co run 32 + 8
        (2, 8, 6, 40, 24, (1, 1), (2, 2), (0, 0)),      # strided 1x1: three dead phases are exact zeros
        (2, 7, 7, 16, 24, (3, 3), (1, 1), (0, 0)),      # no padding, H_out != H
        (2, 12, 9, 16, 32, (3, 5), (2, 1), (1, 2)),     # anisotropic kernel, stride and padding
        (1, 15, 15, 8, 16, (7, 7), (2, 2), (3, 3)),     # 49 taps, each one half-empty k-step; taps wider than the phase
        (1, 13, 10, 136, 72, (3, 3), (1, 1), (1, 1)),   # M = 130, one past a 128-row tile; C_in eight past a 128 tile; TN = 2 ragged
        (3, 17, 17, 64, 64, (3, 3), (1, 1), (1, 1))]    # M = 867: three gw splits
IDS = lambda r: "x".join(str(v) for v in r[:5]) + "k%dx%ds%dx%dp%dx%d" % (r[5] + r[6] + r[7])   # noqa: E731


def _desc(row, q):
    n, h, w, ci, co, k, s, p = row
    return _lib.ConvDesc(n=n, c_in=ci, h=h, w=w, c_out=co, kh=k[0], kw=k[1], stride_h=s[0], stride_w=s[1], pad_h=p[0], pad_w=p[1],
                         dil_h=1, dil_w=1, groups=1, x_layout=_lib.LAYOUT_NHWC, y_layout=_lib.LAYOUT_NHWC, qbits=q,
                         ka=float(np.float32(KA)), kw_scale=float(np.float32(KW)), mfma_passes=0, reserved=0)


@functools.lru_cache(maxsize=None)
def _case(row, q):
    """Seeded inputs (NCHW on the CPU, NHWC on the device, x also as codes) and the float64 reference; made once, never written."""
    n, h, w, ci, co, k, s, p = row
    ho, wo = (h + 2 * p[0] - k[0]) // s[0] + 1, (w + 2 * p[1] - k[1]) // s[1] + 1
    gen = torch.Generator().manual_seed(9100 + 13 * ci + 7 * co + n + q + k[0] * k[1])
    x = _x_values((n, ci, h, w), KA, gen)
    wt = torch.randn((co, ci) + k, generator=gen) * (2.0 / (ci * k[0] * k[1])) ** 0.5
    gy = _gy_values((n, co, ho, wo), gen)
    mod = SimpleNamespace(q_bit=q, Ka=KA, Kw=KW, stride=s, padding=p, dilation=(1, 1), groups=1)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)   # noqa: E731
    c = SimpleNamespace(row=row, q=q, x=nhwc(x), w=wt.to(DEV), gy=nhwc(gy), gy_cpu=gy, x_cpu=x, mod=mod, ref=_reference(x, wt, gy, mod))
    c.codes = torch.empty(c.x.shape, dtype=torch.uint8, device=DEV)
    fmt = (_lib.FMT_ACT8 if q == 8 else _lib.FMT_SFP7) | _lib.FMT_EXT
    _lib.check(_lib.load().slfp_encode_f32(c.x.data_ptr(), c.codes.data_ptr(), c.codes.numel(), float(np.float32(KA)), fmt,
                                           torch.cuda.current_stream().cuda_stream))
    return c


def _launch(c, codes, need=(1, 1, 1), gy=None, f32=False):
    """One slfp_conv2d_bwd_dense_bf16 call (f32: the float32 dense kernels, slfp_conv2d_bwd_ex, for the printed comparison):
    [gx, gw, gb] as NCHW / OIHW / [C_out] CPU tensors (None: not asked for)."""
    L, d = _lib.load(), _desc(c.row, c.q)
    n, h, w, ci, co, k = c.row[:6]
    shapes = ((n, h, w, ci), (co, ci) + k, (co,))
    bufs = [_banded(4 * int(np.prod(s))) for s in shapes]
    size = L.slfp_conv2d_bwd_workspace_bytes_ex if f32 else L.slfp_conv2d_bwd_dense_bf16_workspace_bytes
    nbytes = size(ctypes.byref(d), FLAGS, need[0], need[1])
    assert nbytes > 0
    ws = _banded(nbytes)
    ptr = lambda i: bufs[i][1].data_ptr() if need[i] else None   # noqa: E731
    gy = c.gy if gy is None else gy
    tail = (c.w.data_ptr(), gy.data_ptr(), ptr(0), ptr(1), ptr(2), ws[1].data_ptr(), torch.cuda.current_stream().cuda_stream)
    if f32:
        _lib.check(L.slfp_conv2d_bwd_ex(ctypes.byref(d), FLAGS, c.x.data_ptr(), *tail))
    else:
        _lib.check(L.slfp_conv2d_bwd_dense_bf16(ctypes.byref(d), FLAGS, None if codes else c.x.data_ptr(),
                                                c.codes.data_ptr() if codes else None, *tail))
    torch.cuda.synchronize()
    out = []
    for i, ((buf, view), s) in enumerate(zip(bufs + [ws], shapes + (None,))):
        assert bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + view.numel():] == 0xA5).all()), ("band", i)
        if s is None:
            break
        if not need[i]:
            assert bool((view == 0xA5).all()), ("not asked for, written", i)
        t = view.view(torch.float32).view(s).cpu()
        out.append((t.permute(0, 3, 1, 2) if i == 0 else t) if need[i] else None)
    return out


@pytest.mark.parametrize("q", [8, 7])
@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_against_float64_codes_and_twice(row, q):
    c = _case(row, q)
    got = _launch(c, False)
    for label, res in (("bf16x3", got), ("float32", _launch(c, False, f32=True))):
        errs = [_errors(g, r) for g, r in zip(res, c.ref)]
        print(f"\n{label} {IDS(row)} q{q}: " + "  ".join(f"{nm} elem {e:.2e} l2 {l:.2e}" for nm, (e, l) in zip(("gx", "gw", "gb"), errs)))
        if label == "bf16x3":
            for e, l in errs:
                assert e <= 1e-5 and l <= 1e-6, errs
    if row[5] == (1, 1) and row[6] == (2, 2):   # the three phases no output position reads: written, exact zeros
        live = torch.zeros(row[1], row[2], dtype=torch.bool)
        live[::2, ::2] = True
        assert (got[0][:, :, ~live] == 0).all() and (got[0][:, :, live] != 0).any()
    for other in (_launch(c, False), _launch(c, True)):   # a second call; x as codes: the same bits
        for a, b in zip(got, other):
            assert torch.equal(a, b)


def test_m867_runs_several_splits_with_a_short_last_one_and_a_partial_kstep():
    s = _lib.load().slfp_debug_bwd_dense_bf16_instance(ctypes.byref(_desc(ROWS[7], 8)), FLAGS, 0, 1, 1).decode()
    p, k = map(int, re.search(r"/p(\d+)k(\d+)$", s).groups())
    last = 867 - (p - 1) * k
    assert s.startswith("dnb/gx/tn1/t6+dnb/gw/tm1tn2/t6/tab/") and p >= 2 and 0 < last < k and k % 32 != 0, s


@pytest.mark.parametrize("row", [ROWS[1], ROWS[7]], ids=IDS)
def test_need_subsets(row):
    c = _case(row, 8)
    full = _launch(c, True)
    for need in NEEDS[1:]:
        for codes in (False, True):
            got = _launch(c, codes, need)
            for i in range(3):
                assert (got[i] is None) == (not need[i])
                assert got[i] is None or torch.equal(got[i], full[i]), (need, codes, i)


@pytest.mark.parametrize("codes", [False, True], ids=["f32", "codes"])
def test_inf_and_nan_in_gy_reach_the_elements_the_reference_says(codes):
    """Interior output positions of a stride-1 padded row: no tap of theirs touches padding, so no padding zero meets the inf."""
    c = _case(ROWS[7], 8)
    gy = c.gy_cpu.clone()
    gy[0, 3, 5, 6] = float("inf")
    gy[1, 17, 8, 9] = float("nan")
    ref = _reference(c.x_cpu, c.w.cpu(), gy, c.mod)
    got = _launch(c, codes, gy=gy.permute(0, 2, 3, 1).contiguous().to(DEV))
    for g, (r, _) in zip(got, ref):
        assert (~torch.isfinite(r)).any() and torch.isfinite(r).any()
        assert torch.equal(~torch.isfinite(g), ~torch.isfinite(r))


def test_modules_take_the_kernel_under_bf16x3_all_only():
    gen = torch.Generator().manual_seed(12)
    k3 = cf.conv2d_Q_bias(8, KW, KA)(16, 24, 3, padding=1).to(DEV)
    s2 = cf.conv2d_Q_bias(8, KW, KA)(24, 16, 1, stride=2).to(DEV)
    pw = cf.conv2d_Q_bias(8, KW, KA)(16, 24, 1).to(DEV)
    x = _x_values((2, 16, 9, 7), KA, gen).to(DEV).contiguous(memory_format=torch.channels_last)
    try:
        cf.options.backward = "hip_all"
        for gemm, dense, point in (("f32", "dense_bwd_mfma_f32", "pw_bwd_mfma_f32"), ("bf16x3", "dense_bwd_mfma_f32", "pw_bwd_mfma_bf16x3"),
                                   ("bf16x3_all", "dense_bwd_mfma_bf16x3", "pw_bwd_mfma_bf16x3")):
            cf.options.backward_gemm = gemm
            y = pw(s2(k3(x.clone().requires_grad_(True))))
            y.backward(torch.randn_like(y))
            assert (k3._last_bwd_kernel, s2._last_bwd_kernel, pw._last_bwd_kernel) == (dense, dense, point), gemm
    finally:
        cf.options.backward, cf.options.backward_gemm = "composite", "f32"
