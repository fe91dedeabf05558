"""GPU: training-mode BatchNorm2d (+ReLU) that writes the next Conv2d_Q's 1-byte codes, the code forms of csrc/bn_train.hip.  The
contract of include/slfp.h is exact:
  forward    save_mean, save_invstd, running statistics = slfp_bn_train_fwd's, save_lo = slfp_bn_lut_train_fwd's;
             y_codes = slfp_encode_f32(slfp_bn_train_fwd's y, Ka, fmt | EXT), byte for byte; and, without passing through the
             library's encoder, decode(y_codes) = oracle.quantize(_bn_cases.kernel_order_forward's y), bit for bit
  backward   gx, ggamma, gbeta = slfp_bn_train_bwd(relu) fed the plain forward's y, compared with torch.equal
Then slfp_conv2d_bwd_codes against slfp_conv2d_bwd_ex on the float32 operand (torch.equal) and _bwd_cases' float64 bars, and
fusion.link_codes_train at module level against the unlinked model (torch.equal).  DESIGN section 35.
BN cases: the C % 4 == 0 shapes of _bn_cases.py.  Four channels of every case are pinned (gamma = 0 makes t = beta exactly) so that
exact zeros, the classes below 0.0625 Ka and the clamp occur whatever the shape; the assertions in _classes_occur check it."""
import contextlib
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import _bn_cases as B
import _bwd_cases as W
from _bn_calls import _bwd as _plain_bwd, _fwd as _plain_fwd, _lut_fwd, _ptr, _same, _stream, _ws
from cnns_slfp_quantization_amd import _lib, batchnorm, fusion, layer_specs
from cnns_slfp_quantization_amd import conv2d_func as cf
from cnns_slfp_quantization_amd import optimizer as O
from cnns_slfp_quantization_amd.layer_specs import ConvSpec
from oracle import slfp_oracle as so

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NHWC = _lib.LAYOUT_NHWC
KAS = (2.6023073196411133 / 15.5, 6.629735469818115 / 15.5)   # two Ka of the reference's MobileNetV1
SMALL, BIG = 0.004, 50.0      # |t| < 0.0625 Ka and |t| > 16 Ka for both Ka
CASES = [(s, False) for s in ((2, 5, 7, 32), (3, 1, 1, 64), (2, 3, 3, 1024), B.ragged(32))] + [(B.ragged(32), True)]
_cache = {}


def _fmt(qbits):
    return _lib.FMT_SFP7 if qbits == 7 else _lib.FMT_ACT8


def _inputs(case):
    """_bn_cases.inputs with channels 0..3 pinned: t = 0, +SMALL, -SMALL (0 behind a ReLU), BIG in every row."""
    if case not in _cache:
        d = dict(B.inputs(*case))
        gamma, beta = d["gamma"].clone(), d["beta"].clone()
        gamma[:4] = 0.0
        beta[:4] = torch.tensor([0.0, SMALL, -SMALL, BIG])
        d["gamma"], d["beta"] = gamma, beta
        _cache[case] = d
    return _cache[case]


def _plain(case, relu):
    """slfp_bn_train_fwd's (y, save_mean, save_invstd, running_mean, running_var) of a case, computed once."""
    key = (case, relu, "plain")
    if key not in _cache:
        d = _inputs(case)
        rm, rv = d["rm"].to(DEV), d["rv"].to(DEV)
        _cache[key] = _plain_fwd(case[0], d, relu, rm, rv) + (rm, rv)
        torch.cuda.synchronize()
    return _cache[key]


def _kernel_order_y(case, relu):
    """_bn_cases.kernel_order_forward's y [M, C] from the device's save_mean and save_invstd, computed once (relu = 0) per case."""
    key = (case, "ko")
    if key not in _cache:
        d = _inputs(case)
        _, sm, si, _, _ = _plain(case, False)
        _cache[key] = B.kernel_order_forward(d["x"], d["gamma"], d["beta"], sm.cpu().numpy(), si.cpu().numpy(), False)
    y = _cache[key]
    return np.where(y < 0, np.float32(0), y) if relu else y


def _codes_fwd(shape, d, relu, ka, qbits, rm=None, rv=None, x=None):
    """slfp_bn_codes_train_fwd on the current stream: y_codes (uint8, channels_last), save_mean, save_invstd, save_lo."""
    n, h, w, c = shape
    x = d["x"].to(DEV) if x is None else x
    gamma, beta = d["gamma"].to(DEV), d["beta"].to(DEV)
    codes = torch.full((n, c, h, w), 0xEE, dtype=torch.uint8, device=DEV).contiguous(memory_format=torch.channels_last)
    sm, si, lo = (torch.empty(c, device=DEV) for _ in range(3))
    ws, nbytes = _ws(shape)
    assert _lib.load().slfp_bn_codes_train_supported(n, h, w, c, NHWC, ka, qbits) == 1
    _lib.check(_lib.load().slfp_bn_codes_train_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(rm), _ptr(rv), B.MOMENTUM,
                                                   B.EPS, int(relu), ka, qbits, codes.data_ptr(), sm.data_ptr(), si.data_ptr(),
                                                   lo.data_ptr(), n, h, w, c, NHWC, ws.data_ptr(), nbytes, _stream()))
    return codes, sm, si, lo


def _codes_bwd(shape, d, relu, sm, si, lo, gy, params=True, x=None):
    n, h, w, c = shape
    x = d["x"].to(DEV) if x is None else x
    gamma, beta, gy = d["gamma"].to(DEV), d["beta"].to(DEV), gy.to(DEV)
    gx = torch.empty_like(x)
    gg, gb = (torch.empty(c, device=DEV), torch.empty(c, device=DEV)) if params else (None, None)
    ws, nbytes = _ws(shape)
    _lib.check(_lib.load().slfp_bn_codes_train_bwd(x.data_ptr(), gy.data_ptr(), gamma.data_ptr(), beta.data_ptr(), sm.data_ptr(),
                                                   si.data_ptr(), lo.data_ptr(), int(relu), gx.data_ptr(), _ptr(gg), _ptr(gb), n, h, w,
                                                   c, NHWC, ws.data_ptr(), nbytes, _stream()))
    return gx, gg, gb


def _encode(y, ka, qbits):
    out = torch.empty(y.shape, dtype=torch.uint8, device=DEV).contiguous(memory_format=torch.channels_last)
    _lib.check(_lib.load().slfp_encode_f32(y.data_ptr(), out.data_ptr(), y.numel(), ka, _fmt(qbits) | _lib.FMT_EXT, _stream()))
    return out


def _decode(codes, qbits):
    out = torch.empty(codes.shape, dtype=torch.float32, device=DEV).contiguous(memory_format=torch.channels_last)
    _lib.check(_lib.load().slfp_decode_f32(codes.data_ptr(), out.data_ptr(), codes.numel(), _fmt(qbits) | _lib.FMT_EXT, _stream()))
    return out


def _eq(a, b):
    """Bytes for the codes, bits for float32."""
    return torch.equal(a, b) if a.dtype == torch.uint8 else _same(a, b)


def _classes_occur(y, ka, relu):
    """Exact zeros, values below 0.0625 Ka, values in the log range and values above the clamp all occur in y."""
    a = y.abs()
    assert int((y == 0).sum()) > 0
    assert int(((a > 0) & (a < 0.0625 * ka)).sum()) > 0
    assert int(((a >= 0.0625 * ka) & (a <= 15.0 * ka)).sum()) > 0
    assert int((a > 16.0 * ka).sum()) > 0
    if not relu:
        assert int((y < -0.0625 * ka).sum()) > 0 and int(((y < 0) & (y > -0.0625 * ka)).sum()) > 0


@pytest.mark.parametrize("ka", KAS, ids=["ka0", "ka1"])
@pytest.mark.parametrize("qbits", [8, 7])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=B.case_id)
def test_forward_is_the_plain_forward_then_the_readers_quantizer(case, relu, qbits, ka):
    shape, _ = case
    d = _inputs(case)
    y_plain, sm0, si0, rm0, rv0 = _plain(case, relu)
    _classes_occur(y_plain, ka, relu)
    rm, rv = d["rm"].to(DEV), d["rv"].to(DEV)
    codes, sm, si, lo = _codes_fwd(shape, d, relu, ka, qbits, rm, rv)
    want = _encode(y_plain, ka, qbits)
    dec = _decode(codes, qbits)
    torch.cuda.synchronize()
    assert torch.equal(codes, want)
    for a, b in ((sm, sm0), (si, si0), (rm, rm0), (rv, rv0)):
        assert _same(a, b)
    # without the library's encoder: the oracle's quantizer on the NumPy model of the apply pass
    yk = _kernel_order_y(case, relu)
    ref = so.quantize(yk, np.float32(ka), so.FMT_SFP7 if qbits == 7 else so.FMT_ACT8)
    got = dec.permute(0, 2, 3, 1).reshape(-1, shape[3]).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("case", CASES, ids=B.case_id)
def test_save_lo_is_the_lut_forms(case):
    shape, _ = case
    d = _inputs(case)
    ftab, _ = batchnorm.layerout_act_tables([nn.ReLU()], DEV)
    x, gamma, beta = d["x"].to(DEV), d["gamma"].to(DEV), d["beta"].to(DEV)
    _, sm1, si1, lo1 = _lut_fwd(shape, ftab, x, gamma, beta)
    _, sm, si, lo = _codes_fwd(shape, d, 1, KAS[0], 8)
    torch.cuda.synchronize()
    assert _same(lo, lo1) and _same(sm, sm1) and _same(si, si1)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=B.case_id)
def test_backward_is_the_plain_backward(case, relu):
    shape, _ = case
    d = _inputs(case)
    y_plain, sm0, si0, _, _ = _plain(case, relu)
    _, sm, si, lo = _codes_fwd(shape, d, relu, KAS[1], 7)
    for key in ("gy", "gy_sparse"):
        want = _plain_bwd(shape, d, relu, y_plain, sm0, si0, d[key])
        got = _codes_bwd(shape, d, relu, sm, si, lo, d[key])
        gx_only = _codes_bwd(shape, d, relu, sm, si, lo, d[key], params=False)[0]   # ggamma / gbeta NULL
        torch.cuda.synchronize()
        for name, a, b in zip(("gx", "ggamma", "gbeta"), got, want):
            assert torch.equal(a, b), (key, name)
        assert torch.equal(gx_only, got[0]), key
    if relu:
        assert int((y_plain > 0).sum()) > 0 and int((y_plain == 0).sum()) > 0   # the mask masks


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape", [(2, 5, 7, 32), B.ragged(32)], ids=lambda s: "x".join(map(str, s)))
def test_nan_and_inf_stay_in_their_channel(shape, relu):
    case = (shape, False)
    d = _inputs(case)
    n, h, w, c = shape
    bad = d["x"].clone()
    bad[n - 1, 7, h - 1, w - 1] = float("nan")    # (the last slab of the ragged shape)
    bad[0, 9, 0, 1] = float("inf")
    bad = bad.to(DEV)
    hit = [7, 9]
    keep = [i for i in range(c) if i not in hit]
    res = []
    for xi in (None, bad):
        codes, sm, si, lo = _codes_fwd(shape, d, relu, KAS[0], 8, x=xi)
        res.append((codes, sm, si) + _codes_bwd(shape, d, relu, sm, si, lo, d["gy"], x=xi))
    y_bad, sm_bad, si_bad = _plain_fwd(shape, d, relu, x=bad)
    want = _encode(y_bad, KAS[0], 8)
    torch.cuda.synchronize()
    (c0, _, _, gx0, gg0, gb0), (c1, sm1, si1, gx1, gg1, gb1) = res
    assert torch.equal(c1[:, keep], c0[:, keep]) and _same(gx1[:, keep], gx0[:, keep])
    assert _same(gg1[keep], gg0[keep]) and _same(gb1[keep], gb0[keep])
    assert _same(sm1, sm_bad) and _same(si1, si_bad) and bool(torch.isnan(si1[hit]).all())
    assert bool(torch.isnan(y_bad[:, hit]).all())
    assert bool((c1[:, hit] == 0).all())                              # the statistics are NaN: every value is a NaN, code 0x00
    assert torch.equal(c1, want)


@pytest.mark.parametrize("case", [(B.ragged(32), False), ((2, 3, 3, 1024), False)], ids=B.case_id)
def test_deterministic(case):
    shape, _ = case
    d = _inputs(case)
    runs = []
    for _ in range(2):
        rm, rv = d["rm"].to(DEV), d["rv"].to(DEV)
        codes, sm, si, lo = _codes_fwd(shape, d, 1, KAS[0], 8, rm, rv)
        runs.append((codes, sm, si, lo, rm, rv) + _codes_bwd(shape, d, 1, sm, si, lo, d["gy"]))
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert _eq(a, b)


def test_outputs_untouched_by_a_refusal():
    shape = (2, 5, 7, 32)
    d = _inputs((shape, False))
    n, h, w, c = shape
    x = d["x"].to(DEV)
    codes = torch.full((n * h * w * c,), 0xEE, dtype=torch.uint8, device=DEV)
    sm = torch.full((c,), 7.0, device=DEV)
    ws, nbytes = _ws(shape)
    rc = _lib.load().slfp_bn_codes_train_fwd(x.data_ptr(), sm.data_ptr(), sm.data_ptr(), None, None, 0.1, 1e-5, 1, KAS[0], 32,
                                             codes.data_ptr(), sm.data_ptr(), sm.data_ptr(), sm.data_ptr(), n, h, w, c, NHWC,
                                             ws.data_ptr(), nbytes, _stream())
    torch.cuda.synchronize()
    assert rc == _lib.ERR_UNSUPPORTED
    assert bool((codes == 0xEE).all()) and bool((sm == 7.0).all())


def test_runs_on_the_current_stream():
    """The default stream is held by a sleep; a call on another stream completes meanwhile, with the same bits."""
    case = (B.ragged(32), False)
    shape = case[0]
    d = _inputs(case)

    def run():
        codes, sm, si, lo = _codes_fwd(shape, d, 1, KAS[0], 8)
        return (codes, sm, si, lo) + _codes_bwd(shape, d, 1, sm, si, lo, d["gy"])

    want = run()
    from test_gpu_headline import _sleep_cycles
    cycles = _sleep_cycles(200)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    held, done = torch.cuda.Event(), torch.cuda.Event()
    torch.cuda._sleep(cycles)               # 0.2 s on the default stream
    held.record()
    with torch.cuda.stream(side):
        got = run()
        done.record()
    done.synchronize()
    still_held = not held.query()
    torch.cuda.synchronize()
    assert still_held, "the side stream's work waited for the default stream (or the sleep was too short to tell)"
    for a, b in zip(got, want):
        assert _eq(a, b)


# ---- slfp_conv2d_bwd_codes: the activation operand of the weight gradient as 1-byte codes ------------------------------------
def _spec(c_in, c_out, k, stride, pad, groups, h, w):
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    return ConvSpec(c_in, c_out, (k, k), (stride, stride), (pad, pad), groups, True, h, w, ho, wo, KAS[0], 0.9 / 15.5)


# the smallest ragged NHWC shapes per family (flags, n, spec): M is no multiple of a tile, C no multiple of the lanes
BWD_CASES = {
    "dw-s1-c8": (0, 3, _spec(8, 8, 3, 1, 1, 8, 7, 5)), "dw-s2-c8": (0, 3, _spec(8, 8, 3, 2, 1, 8, 7, 5)),
    "dw-s1-c36": (0, 3, _spec(36, 36, 3, 1, 1, 36, 7, 5)), "dw-s2-c36": (0, 3, _spec(36, 36, 3, 2, 1, 36, 7, 5)),
    "pw-12-20": (0, 3, _spec(12, 20, 1, 1, 0, 1, 5, 7)), "pw-64-136": (0, 3, _spec(64, 136, 1, 1, 0, 1, 5, 7)),
    "dense-3x3-s1": (_lib.BWD_DENSE, 3, _spec(4, 8, 3, 1, 1, 1, 7, 6)), "dense-3x3-s2": (_lib.BWD_DENSE, 3, _spec(4, 8, 3, 2, 1, 1, 7, 6)),
    "dense-1x1-s2": (_lib.BWD_DENSE, 3, _spec(8, 12, 1, 2, 0, 1, 7, 6)), "dense-5x5": (_lib.BWD_DENSE, 3, _spec(4, 4, 5, 1, 2, 1, 7, 6)),
}
KERNELS = {"dw": b"dw3x3_bwd", "pw": b"pw_bwd_mfma_f32", "dense": b"dense_bwd_mfma_f32"}


def _raw_bwd(entry, desc, flags, x, w, gy, need):
    """slfp_conv2d_bwd_ex / slfp_conv2d_bwd_codes on the current stream: (gx, gw, gb), None for what `need` leaves out."""
    L = _lib.load()
    r = ctypes.byref(desc)
    gx = torch.full((desc.n, desc.c_in, desc.h, desc.w), 7.0, device=DEV).contiguous(memory_format=torch.channels_last) if need[0] else None
    gw = torch.full_like(w, 7.0) if need[1] else None
    gb = torch.full((desc.c_out,), 7.0, device=DEV) if need[2] else None
    nbytes = L.slfp_conv2d_bwd_workspace_bytes_ex(r, flags, int(need[0]), int(need[1]))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
    _lib.check(getattr(L, entry)(r, flags, x.data_ptr(), w.data_ptr(), gy.data_ptr(), _ptr(gx), _ptr(gw), _ptr(gb), ws.data_ptr(),
                                 _stream()))
    return gx, gw, gb


@pytest.mark.parametrize("qbits", [8, 7])
@pytest.mark.parametrize("name", list(BWD_CASES))
def test_conv_backward_on_codes_equals_the_float32_operand(name, qbits):
    flags, n, spec = BWD_CASES[name]
    gen = torch.Generator().manual_seed(100 + len(name) + qbits)
    mod = W._make(spec, qbits, True, gen)
    x = W._x_values((n, spec.c_in, spec.h, spec.w), spec.Ka, gen)
    gy = torch.randn((n, spec.c_out, spec.h_out, spec.w_out), generator=gen)
    xd = x.to(DEV).contiguous(memory_format=torch.channels_last)
    gyd = gy.to(DEV).contiguous(memory_format=torch.channels_last)
    w = mod.weight.detach().contiguous()
    desc = cf._conv_desc(mod, xd.shape, True, True)
    L = _lib.load()
    assert L.slfp_conv2d_bwd_codes_supported(ctypes.byref(desc), flags) == 1
    assert L.slfp_conv2d_bwd_kernel_name_ex(ctypes.byref(desc), flags) == KERNELS[name.split("-")[0]]
    codes = _encode(xd, cf._f32(mod.Ka), qbits)
    ka = spec.Ka
    a = x.abs()
    for lo_, hi_ in ((0.0, 0.0), (1e-30, 0.0625 * ka), (0.0625 * ka, 15.0 * ka), (16.0 * ka, 1e30)):   # every code range, signed
        sel = (a >= lo_) & (a <= hi_)
        assert int(sel.sum()) > 0 and (lo_ == 0.0 or (int((sel & (x < 0)).sum()) > 0 and int((sel & (x > 0)).sum()) > 0))
    refs = W._reference(x, w.cpu(), gy, mod)
    full = None
    for need in ((True, True, True), (False, True, True), (True, False, False), (True, True, False)):
        want = _raw_bwd("slfp_conv2d_bwd_ex", desc, flags, xd, w, gyd, need)
        got = _raw_bwd("slfp_conv2d_bwd_codes", desc, flags, codes, w, gyd, need)
        torch.cuda.synchronize()
        for what, g, e, wanted in zip(("gx", "gw", "gb"), got, want, need):
            assert (g is not None) == wanted
            if wanted:
                assert torch.equal(g, e), (need, what)
        full = got if full is None else full
    for what, g, ref in zip(("gx", "gw", "gb"), full, refs):   # the float64 bars of _bwd_cases
        elem, l2 = W._errors(g, ref)
        print(name, qbits, what, "elem", elem, "l2", l2)
        assert elem <= 1e-5 and l2 <= 1e-6, (what, elem, l2)


def test_conv_backward_on_codes_is_deterministic_and_refuses_before_device_work():
    flags, n, spec = BWD_CASES["pw-64-136"]
    gen = torch.Generator().manual_seed(5)
    mod = W._make(spec, 8, True, gen)
    xd = W._x_values((n, spec.c_in, spec.h, spec.w), spec.Ka, gen).to(DEV).contiguous(memory_format=torch.channels_last)
    gyd = torch.randn((n, spec.c_out, spec.h_out, spec.w_out), generator=gen).to(DEV).contiguous(memory_format=torch.channels_last)
    w = mod.weight.detach().contiguous()
    desc = cf._conv_desc(mod, xd.shape, True, True)
    codes = _encode(xd, cf._f32(mod.Ka), 8)
    a = _raw_bwd("slfp_conv2d_bwd_codes", desc, flags, codes, w, gyd, (True, True, True))
    b = _raw_bwd("slfp_conv2d_bwd_codes", desc, flags, codes, w, gyd, (True, True, True))
    torch.cuda.synchronize()
    assert all(_same(p, q) for p, q in zip(a, b))
    nchw = cf._conv_desc(mod, xd.shape, False, True)
    gw = torch.full_like(w, 7.0)
    L = _lib.load()
    assert L.slfp_conv2d_bwd_codes_supported(ctypes.byref(nchw), flags) == 0
    rc = L.slfp_conv2d_bwd_codes(ctypes.byref(nchw), flags, codes.data_ptr(), w.data_ptr(), gyd.data_ptr(), None, gw.data_ptr(), None,
                                 codes.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == _lib.ERR_UNSUPPORTED and bool((gw == 7.0).all())


# ---- module level: fusion.link_codes_train ---------------------------------------------------------------------------------------
_MB = layer_specs.conv_layers("mobilenetv1_imagenet224")   # the reference's Ka / Kw pattern: stem, then (dw, pw) pairs


def _q(spec, c_in, c_out, k, stride, pad, groups=1, q_bit=8):
    return cf.conv2d_Q(q_bit, spec.Kw, spec.Ka)(c_in, c_out, k, stride=stride, padding=pad, groups=groups, bias=False)


def _mobilenet_stack(q_bit=8):
    """conv_bn(3 -> 32, stride 2), conv_dw(32 -> 64, 1), conv_dw(64 -> 64, 2) of nets_imgnet/mobilenetv1.py:24-41 as nested
    nn.Sequentials, and a 10-class head."""
    def conv_dw(i, inp, oup, s):
        return nn.Sequential(_q(_MB[i], inp, inp, 3, s, 1, inp, q_bit), nn.BatchNorm2d(inp), nn.ReLU(inplace=True),
                             _q(_MB[i + 1], inp, oup, 1, 1, 0, 1, q_bit), nn.BatchNorm2d(oup), nn.ReLU(inplace=True))
    torch.manual_seed(4)
    body = nn.Sequential(nn.Sequential(_q(_MB[0], 3, 32, 3, 2, 1, 1, q_bit), nn.BatchNorm2d(32), nn.ReLU(inplace=True)),
                         conv_dw(1, 32, 64, 1), conv_dw(3, 64, 64, 2))
    m = nn.Sequential(body, nn.AdaptiveAvgPool2d(1), nn.Flatten(), cf.linear_Q(q_bit, 0.05, 0.3)(64, 10))
    return _spread(m).to(DEV).to(memory_format=torch.channels_last)


def _vgg_stack():
    """[3x3 conv, BN, ReLU, 3x3 conv, BN, ReLU] in the style of nets_imgnet/vgg16.py, scaled-bias convs, and a 10-class head."""
    Conv = cf.conv2d_Q_bias(8, 0.06, 0.17)
    torch.manual_seed(6)
    m = nn.Sequential(Conv(3, 16, 3, padding=1), nn.BatchNorm2d(16), nn.ReLU(inplace=True), Conv(16, 16, 3, padding=1),
                      nn.BatchNorm2d(16), nn.ReLU(inplace=True), nn.AdaptiveAvgPool2d(1), nn.Flatten(), cf.linear_Q(8, 0.05, 0.3)(16, 10))
    return _spread(m).to(DEV).to(memory_format=torch.channels_last)


def _spread(m):
    """BatchNorm parameters and statistics off their initial values; weights large enough that every code range is met."""
    g = torch.Generator().manual_seed(17)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                c = mod.num_features
                mod.weight.copy_(torch.rand(c, generator=g) + 0.5)
                mod.bias.copy_(torch.randn(c, generator=g) * 0.3)
                mod.running_mean.copy_(torch.randn(c, generator=g) * 0.2)
                mod.running_var.copy_(torch.rand(c, generator=g) + 0.5)
    return m


def _image():
    return torch.randn(2, 3, 19, 13, generator=torch.Generator().manual_seed(8)).to(DEV).contiguous(memory_format=torch.channels_last)


@contextlib.contextmanager
def _backward(mode):
    prev, det = cf.options.backward, torch.backends.cudnn.deterministic
    cf.options.backward = mode
    torch.backends.cudnn.deterministic = True   # the layers "hip" leaves to the composite run MIOpen: the same algorithm in both models
    try:
        yield
    finally:
        cf.options.backward, torch.backends.cudnn.deterministic = prev, det


def _convs(m):
    return [c for c in m.modules() if fusion._is_conv_q(c)]


def _step(m, x, grad=True):
    """One forward (+ backward): logits, input gradient, parameter gradients, buffers, every Conv2d_Q's input_q."""
    m.zero_grad(set_to_none=True)
    xi = x.clone(memory_format=torch.preserve_format).requires_grad_(grad)
    with contextlib.nullcontext() if grad else torch.no_grad():
        out = m(xi)
    if grad:
        (out.square().mean() + out.sum() * 0.1).backward()
    return dict(logits=out.detach().clone(), gx=xi.grad, grads=[p.grad for p in m.parameters()],
                buffers=[b.clone() for b in m.buffers()], input_q=[c.input_q.clone() for c in _convs(m)])


def _assert_same(a, b, what=""):
    for key in a:
        va, vb = (a[key], b[key]) if isinstance(a[key], list) else ([a[key]], [b[key]])
        assert len(va) == len(vb), (what, key)
        for i, (p, q) in enumerate(zip(va, vb)):
            assert (p is None) == (q is None) and (p is None or torch.equal(p, q)), (what, key, i)


def _pair(make):
    """(linked, unlinked reference): deep copies, both on use_device_bn_train(min_elements=0), which is also what a linked
    wrapper falls back to."""
    model = make()
    ref = copy.deepcopy(model)
    for m in (model, ref):
        assert fusion.use_device_bn_train(m, min_elements=0) > 0
        m.train()
    return model, ref


def _no_record_reachable(m):
    for mod in m.modules():
        for v in mod.__dict__.values():
            if torch.is_tensor(v):
                assert "_train_link" not in v.__dict__, type(mod).__name__


@pytest.mark.parametrize("mode", ["hip", "hip_all"])
def test_linked_mobilenet_stack_trains_bit_for_bit(mode):
    model, ref = _pair(_mobilenet_stack)
    assert fusion.link_codes_train(model, min_elements=0) == 4
    wraps = [w for w in model.modules() if isinstance(w, fusion.TrainBatchNormCodes2d)]
    assert len(wraps) == 4 and [w._conv for w in wraps] == _convs(model)[1:]
    x = _image()
    opts = [O.DSGD(m.parameters(), 8, lr=0.05, momentum=0.9) for m in (model, ref)]
    with _backward(mode):
        for step in range(2):
            got, want = _step(model, x), _step(ref, x)
            for w in wraps:   # the test cannot pass with nothing linked
                assert w._last_kernel == "bn_codes_train+relu", w._last_kernel
                assert "+codes_in" in w._conv._last_kernel and w._conv._last_kernel.split("+")[0] != "", w._conv._last_kernel
                assert w._conv._last_bwd_kernel in ("dw3x3_bwd", "pw_bwd_mfma_f32"), w._conv._last_bwd_kernel
                assert w._conv._last_codes is not None and w._conv._last_input is None
            _assert_same(got, want, (mode, step))
            assert all(g is not None for g in got["grads"]) and got["gx"] is not None
            for o in opts:
                o.step()                                   # weights change through .data
            for p, q in zip(model.parameters(), ref.parameters()):
                assert torch.equal(p, q)
        _no_record_reachable(model)
        _assert_same(_step(model, x), _step(ref, x), "third")   # backward(), then a fresh forward
        _no_record_reachable(model)
        # what the code path does not take runs what the unlinked model runs
        _assert_same(_step(model, x, grad=False), _step(ref, x, grad=False), "no_grad")     # training mode, nothing records: codes all the same
        assert all(w._last_kernel == "bn_codes_train+relu" for w in wraps)
        for m in (model, ref):
            m.eval()
        _assert_same(_step(model, x, grad=False), _step(ref, x, grad=False), "eval")
        assert all(w._last_kernel == "aten" for w in wraps)
        for m in (model, ref):
            m.train()
        xn = x.contiguous()                                                                  # NCHW
        _assert_same(_step(model, xn), _step(ref, xn), "nchw")
        assert all(w._last_kernel == "aten" for w in wraps)
    with _backward("composite"):
        _assert_same(_step(model, x), _step(ref, x), "composite")
        assert all(w._last_kernel == "bn_train+relu" for w in wraps)
    with _backward(mode):
        # a Ka changed after linking: that pair falls back to float32 and still matches
        for m in (model, ref):
            _convs(m)[2].Ka = torch.tensor(float(_convs(m)[2].Ka) * 1.25)
        _assert_same(_step(model, x), _step(ref, x), "ka")
        assert [w._last_kernel for w in wraps] == ["bn_codes_train+relu", "bn_train+relu", "bn_codes_train+relu", "bn_codes_train+relu"]
        # unlink, then a step: the never-linked model
        assert fusion.unlink_codes_train(model) == 4
        _assert_same(_step(model, x), _step(ref, x), "unlinked")
        assert not any(isinstance(w, fusion.TrainBatchNormCodes2d) for w in model.modules())
        assert all("codes" not in c._last_kernel for c in _convs(model))


def test_below_min_elements_stays_float32():
    model, ref = _pair(_mobilenet_stack)
    assert fusion.link_codes_train(model, min_elements=1 << 30) == 4
    x = _image()
    with _backward("hip"):
        _assert_same(_step(model, x), _step(ref, x))
    wraps = [w for w in model.modules() if isinstance(w, fusion.TrainBatchNormCodes2d)]
    assert all(w._last_kernel == "bn_train+relu" for w in wraps) and all("codes" not in c._last_kernel for c in _convs(model))


def test_linked_sfp7_stack_trains_bit_for_bit():
    model, ref = _pair(lambda: _mobilenet_stack(q_bit=7))
    assert fusion.link_codes_train(model, min_elements=0) == 4
    x = _image()
    with _backward("hip_all"):
        _assert_same(_step(model, x), _step(ref, x))
    assert all(w._last_kernel == "bn_codes_train+relu" for w in model.modules() if isinstance(w, fusion.TrainBatchNormCodes2d))


def test_linked_vgg_pair_trains_bit_for_bit_under_hip_all():
    model, ref = _pair(_vgg_stack)
    assert fusion.link_codes_train(model, min_elements=0) == 1
    x = _image()
    opts = [O.DSGD(m.parameters(), 8, lr=0.05, momentum=0.9) for m in (model, ref)]
    with _backward("hip_all"):
        for step in range(2):
            _assert_same(_step(model, x), _step(ref, x), step)
            assert model[1]._last_kernel == "bn_codes_train+relu"
            assert "+codes_in" in model[3]._last_kernel and model[3]._last_bwd_kernel == "dense_bwd_mfma_f32"
            for o in opts:
                o.step()
    with _backward("hip"):   # no backward kernel reads this layer's codes without SLFP_BWD_DENSE: float32
        _assert_same(_step(model, x), _step(ref, x), "hip")
        assert model[1]._last_kernel == "bn_train+relu" and model[3]._last_bwd_kernel == "composite"
