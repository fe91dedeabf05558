"""GPU: training-mode BatchNorm2d -> layer-output quantizer -> activation that writes the next Conv2d_Q's 1-byte codes, the
table-and-codes form of csrc/bn_train.hip.  The contract of include/slfp.h is exact:
  forward    save_mean, save_invstd, save_lo, running statistics = slfp_bn_lut_train_fwd's; y_codes = T[class], the class found as
             test_gpu_bn_layerout_train.py finds it; y_codes = slfp_encode_f32(slfp_bn_lut_train_fwd's y, Ka, fmt | EXT); and, without
             the library's encoder, decode(y_codes) = oracle.quantize(F[index(oracle.layerout(_bn_cases.kernel_order_forward's y))])
  backward   slfp_bn_lut_train_bwd as it is: the chain new forward -> slfp_conv2d_bwd_codes -> slfp_bn_lut_train_bwd is torch.equal to
             LUT forward -> slfp_conv2d_bwd_ex -> slfp_bn_lut_train_bwd
Then fusion.link_layerout_codes_train at module level against the unlinked model on use_device_bn_layerout_train (torch.equal).
BN cases: the C % 4 == 0 shapes of _bn_cases.py.  Six channels of every case are pinned (gamma = 0 makes t = beta exactly) so that
the reader's exact-zero, tiny, log-range and clamp classes occur whatever the shape; _classes_occur asserts it."""
import contextlib
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import _bn_cases as B
import _bwd_cases as W
import _layerout_codes_models as M
from _bn_calls import _lut_bwd, _lut_fwd, _ptr, _same, _stream, _ws
from test_gpu_bn_layerout_train import ACTS, _classes, _quantize, _tables, _values
from test_gpu_bn_codes_train import BWD_CASES, _assert_same, _decode, _encode, _raw_bwd
from cnns_slfp_quantization_amd import _lib, batchnorm, fusion
from cnns_slfp_quantization_amd import conv2d_func as cf
from cnns_slfp_quantization_amd import optimizer as O
from oracle import slfp_oracle as so

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NHWC = _lib.LAYOUT_NHWC
NT = _lib.LAYEROUT_LUT_BYTES
KAS = (2.6023073196411133 / 15.5, 6.629735469818115 / 15.5)   # two Ka of the reference's MobileNetV1
SMALL, BIG = 0.004, 50.0      # act(+-SMALL) lies below 0.0625 Ka and act(BIG) above 16 Ka for both Ka and the three activations
PINNED = [0.0, SMALL, -SMALL, BIG, -BIG, -300.0]   # the NaN class; tiny; tiny (ReLU: 0); the clamp; a negative (ReLU: 0); act = -0.0
CASES = [(s, False) for s in ((2, 5, 7, 32), (3, 1, 1, 64), (2, 3, 3, 1024), B.ragged(32))] + [(B.ragged(32), True)]
_cache = {}


def _inputs(case):
    """_bn_cases.inputs with channels 0..5 pinned to PINNED in every row."""
    if case not in _cache:
        d = dict(B.inputs(*case))
        gamma, beta = d["gamma"].clone(), d["beta"].clone()
        gamma[:len(PINNED)] = 0.0
        beta[:len(PINNED)] = torch.tensor(PINNED)
        d["gamma"], d["beta"] = gamma, beta
        _cache[case] = d
    return _cache[case]


def _ctab(act, ka, qbits):
    key = ("ctab", act, ka, qbits)
    if key not in _cache:
        _cache[key] = batchnorm.layerout_code_table([ACTS[act]()], ka, qbits, DEV)
    return _cache[key]


def _lut(case, act):
    """slfp_bn_lut_train_fwd's (y, save_mean, save_invstd, save_lo, running_mean, running_var) of a case, computed once."""
    key = (case, act, "lut")
    if key not in _cache:
        d = _inputs(case)
        rm, rv = d["rm"].to(DEV), d["rv"].to(DEV)
        _cache[key] = _lut_fwd(case[0], _tables(act)[0], d["x"].to(DEV), d["gamma"].to(DEV), d["beta"].to(DEV), rm, rv) + (rm, rv)
        torch.cuda.synchronize()
    return _cache[key]


def _plain_classes(case):
    """The class of every element: slfp_bn_train_fwd(relu = 0), slfp_quantize_layerout_f32, a search in slfp_layerout_lut_values."""
    key = (case, "cls")
    if key not in _cache:
        from _bn_calls import _fwd as _plain_fwd
        y_plain, sm, si = _plain_fwd(case[0], _inputs(case), False)
        _cache[key] = (_classes(_quantize(y_plain)), sm, si)
        torch.cuda.synchronize()
    return _cache[key]


def _lc_fwd(shape, ctab, x, gamma, beta, rm=None, rv=None, codes=None):
    """slfp_bn_lut_codes_train_fwd on the current stream: y_codes (uint8, channels_last), save_mean, save_invstd, save_lo."""
    n, h, w, c = shape
    if codes is None:
        codes = torch.full((n, c, h, w), 0xEE, dtype=torch.uint8, device=DEV).contiguous(memory_format=torch.channels_last)
    sm, si, lo = (torch.empty(c, device=DEV) for _ in range(3))
    ws, nbytes = _ws(shape)
    assert _lib.load().slfp_bn_lut_codes_train_supported(n, h, w, c, NHWC) == 1
    assert ctab.dtype == torch.uint8 and ctab.numel() == NT and ctab.data_ptr() % 16 == 0
    _lib.check(_lib.load().slfp_bn_lut_codes_train_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(rm), _ptr(rv), B.MOMENTUM,
                                                       B.EPS, ctab.data_ptr(), codes.data_ptr(), sm.data_ptr(), si.data_ptr(),
                                                       lo.data_ptr(), n, h, w, c, NHWC, ws.data_ptr(), nbytes, _stream()))
    return codes, sm, si, lo


def _dev(d):
    return d["x"].to(DEV), d["gamma"].to(DEV), d["beta"].to(DEV)


def _classes_occur(y, ka):
    """The reader's exact-zero, tiny, log-range and clamp classes all occur in y = act(layerout(bn(x))), and so does the NaN class."""
    a = y.abs()
    assert int((y == 0).sum()) > 0
    assert int(((a > 0) & (a < 0.0625 * ka)).sum()) > 0
    assert int(((a >= 0.0625 * ka) & (a <= 15.0 * ka)).sum()) > 0
    assert int((a > 16.0 * ka).sum()) > 0
    assert int(torch.isnan(y).sum()) > 0


@pytest.mark.parametrize("ka", KAS, ids=["ka0", "ka1"])
@pytest.mark.parametrize("qbits", [8, 7])
@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("case", CASES, ids=B.case_id)
def test_forward_is_the_composition(case, act, qbits, ka):
    shape, _ = case
    d = _inputs(case)
    x, gamma, beta = _dev(d)
    y_lut, sm0, si0, lo0, rm0, rv0 = _lut(case, act)
    _classes_occur(y_lut, ka)
    ctab = _ctab(act, ka, qbits)
    rm, rv = d["rm"].to(DEV), d["rv"].to(DEV)
    codes, sm, si, lo = _lc_fwd(shape, ctab, x, gamma, beta, rm, rv)
    cls = _plain_classes(case)[0]
    want = _encode(y_lut, ka, qbits)
    torch.cuda.synchronize()
    assert codes.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(codes, ctab[cls])                            # T[class]
    assert torch.equal(codes, want)                                 # the reader's encoder on the LUT form's y (a NaN: 0x00 in both)
    for a, b in ((sm, sm0), (si, si0), (lo, lo0), (rm, rm0), (rv, rv0)):
        assert _same(a, b)


@pytest.mark.parametrize("qbits", [8, 7])
@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("case", CASES, ids=B.case_id)
def test_forward_without_the_librarys_encoder(case, act, qbits):
    """decode(y_codes) against the oracle: its layer-output step on the NumPy model of the apply pass, the activation value from
    layerout_act_tables' F at that value's index (torch's CPU and device GELU need not agree in the last bit), then its activation
    quantizer.  A NaN behind the layer-output step (an exact zero) reads as the tiny class: the stated difference."""
    shape, _ = case
    ka = KAS[1]
    d = _inputs(case)
    key = (case, "ko")
    if key not in _cache:
        _, sm, si = _plain_classes(case)
        yk = B.kernel_order_forward(d["x"], d["gamma"], d["beta"], sm.cpu().numpy(), si.cpu().numpy(), False)
        _cache[key] = so.layerout(np.ascontiguousarray(yk, dtype=np.float32))
    q = _cache[key]
    vals, ncls = _values()
    index = {int(b): i for i, b in enumerate(vals[:ncls].numpy().view(np.uint32)) if i > 0}
    idx = np.array([0 if np.isnan(v) else index[int(b)] for v, b in zip(q.ravel(), q.view(np.uint32).ravel())]).reshape(q.shape)
    assert (idx == 0).sum() > 0 and (idx > 0).sum() > 0
    fvals = _tables(act)[0].cpu().numpy()
    fmt = so.FMT_SFP7 if qbits == 7 else so.FMT_ACT8
    ref = so.quantize(np.ascontiguousarray(fvals[idx]), np.float32(ka), fmt)
    tiny = so.quantize(np.array([1e-30], dtype=np.float32), np.float32(ka), fmt)[0]
    ref = np.where(idx == 0, tiny, ref)
    x, gamma, beta = _dev(d)
    codes = _lc_fwd(shape, _ctab(act, ka, qbits), x, gamma, beta)[0]
    dec = _decode(codes, qbits)
    torch.cuda.synchronize()
    got = dec.permute(0, 2, 3, 1).reshape(-1, shape[3]).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), ref.astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("act", list(ACTS))
def test_every_class(act):
    """gamma = 0 makes t = +-0 + beta = beta exactly: one channel per class, then channels whose beta lies off the grid."""
    vals, ncls = _values()
    ctab = _ctab(act, KAS[0], 8)
    shape = (2, 1, 1, NT)
    x = torch.randn(2, NT, 1, 1, generator=torch.Generator().manual_seed(11)).to(DEV).contiguous(memory_format=torch.channels_last)
    codes = _lc_fwd(shape, ctab, x, torch.zeros(NT, device=DEV), vals.to(DEV))[0]
    torch.cuda.synchronize()
    got = codes.view(2, NT)
    assert int(ctab[0]) == 0 and len(set(ctab[:ncls].tolist())) > 32   # (not a table of a few bytes: behind a ReLU half the 8-bit codes)
    for r in range(2):
        assert torch.equal(got[r, 1:ncls], ctab[1:ncls])             # every class with a nonzero value
        assert bool((got[r, ncls:] == ctab[0]).all())                 # beta = 0: the NaN class
        assert int(got[r, 0]) == int(ctab[0])                         # beta = NaN
    off = np.array([2.0 ** -8 * 1.01, -(2.0 ** -8) * 1.01, 300.0, -300.0, 1e-40, -1e-40, 1.03, 0.0, 247.9, 2.0 ** -8, 3e-39, -1e-44],
                   dtype=np.float32)
    want_q = torch.from_numpy(so.layerout(off))
    cls = _classes(want_q.to(DEV))
    assert int(cls[7]) == 0 and float(want_q[2]) == 248.0 and float(want_q[3]) == -248.0
    shape = (2, 1, 1, off.size)
    x = torch.randn(2, off.size, 1, 1, generator=torch.Generator().manual_seed(12)).to(DEV).contiguous(memory_format=torch.channels_last)
    codes = _lc_fwd(shape, ctab, x, torch.zeros(off.size, device=DEV), torch.from_numpy(off).to(DEV))[0]
    torch.cuda.synchronize()
    for r in range(2):
        assert torch.equal(codes.view(2, -1)[r], ctab[cls]), r


@pytest.mark.parametrize("shape", [(2, 5, 7, 32), B.ragged(32)], ids=lambda s: "x".join(map(str, s)))
def test_nan_and_inf_stay_in_their_channel(shape):
    case = (shape, False)
    d = _inputs(case)
    n, h, w, c = shape
    x, gamma, beta = _dev(d)
    ctab = _ctab("gelu", KAS[0], 8)
    bad = d["x"].clone()
    bad[n - 1, 7, h - 1, w - 1] = float("nan")    # (the last slab of the ragged shape)
    bad[0, 9, 0, 1] = float("inf")
    bad[1, 10, 1, 0] = -float("inf")
    bad = bad.to(DEV)
    hit = [7, 9, 10]
    keep = [i for i in range(c) if i not in hit]
    c0, sm0, si0, lo0 = _lc_fwd(shape, ctab, x, gamma, beta)
    c1, sm1, si1, lo1 = _lc_fwd(shape, ctab, bad, gamma, beta)
    _, sm2, si2, lo2 = _lut_fwd(shape, _tables("gelu")[0], bad, gamma, beta)
    torch.cuda.synchronize()
    assert torch.equal(c1[:, keep], c0[:, keep])
    assert _same(sm1[keep], sm0[keep]) and _same(si1[keep], si0[keep]) and _same(lo1[keep], lo0[keep])
    assert _same(sm1, sm2) and _same(si1, si2) and _same(lo1, lo2) and bool(torch.isnan(si1[hit]).all())
    assert bool((c1[:, hit] == ctab[0]).all())                        # the statistics are NaN: every value is the NaN class


def test_nothing_beyond_the_code_tensor_is_written():
    """Guard bytes around the codes; then a code tensor that is its whole allocation (a multiple of the allocator's block)."""
    guard = 64
    for shape in ((2, 5, 7, 32), B.ragged(32), (2, 3, 3, 1024)):
        n, h, w, c = shape
        d = _inputs((shape, False))
        x, gamma, beta = _dev(d)
        ctab = _ctab("swish", KAS[0], 8)
        want = _lc_fwd(shape, ctab, x, gamma, beta)[0]
        nbytes = n * h * w * c
        buf = torch.full((guard + nbytes + guard,), 0xEE, dtype=torch.uint8, device=DEV)
        inner = buf[guard:guard + nbytes].view(n, h, w, c).permute(0, 3, 1, 2)
        assert inner.data_ptr() % 4 == 0 and inner.is_contiguous(memory_format=torch.channels_last)
        _lc_fwd(shape, ctab, x, gamma, beta, codes=inner)
        torch.cuda.synchronize()
        assert torch.equal(inner, want) and bool((buf[:guard] == 0xEE).all()) and bool((buf[guard + nbytes:] == 0xEE).all())
    assert nbytes % 512 == 0
    whole = torch.empty(nbytes, dtype=torch.uint8, device=DEV)       # the codes end at the last byte of their allocation
    got = _lc_fwd(shape, ctab, x, gamma, beta, codes=whole.view(n, h, w, c).permute(0, 3, 1, 2))[0]
    torch.cuda.synchronize()
    assert torch.equal(got, want)


@pytest.mark.parametrize("case", [(B.ragged(32), False), ((2, 3, 3, 1024), False)], ids=B.case_id)
def test_deterministic(case):
    shape, _ = case
    d = _inputs(case)
    x, gamma, beta = _dev(d)
    runs = []
    for _ in range(2):
        rm, rv = d["rm"].to(DEV), d["rv"].to(DEV)
        runs.append(_lc_fwd(shape, _ctab("swish", KAS[0], 8), x, gamma, beta, rm, rv) + (rm, rv))
    torch.cuda.synchronize()
    assert torch.equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1:], runs[1][1:]):
        assert _same(a, b)


def test_outputs_untouched_by_a_refusal():
    shape = (2, 5, 7, 32)
    d = _inputs((shape, False))
    n, h, w, c = shape
    x = d["x"].to(DEV)
    codes = torch.full((n * h * w * c,), 0xEE, dtype=torch.uint8, device=DEV)
    sm = torch.full((c,), 7.0, device=DEV)
    ws, nbytes = _ws(shape)
    ctab = _ctab("swish", KAS[0], 8)
    L = _lib.load()
    for kw in (dict(tab=ctab.data_ptr() + 4), dict(layout=_lib.LAYOUT_NCHW), dict(y=codes.data_ptr() + 2), dict(ws_bytes=nbytes - 1)):
        rc = L.slfp_bn_lut_codes_train_fwd(x.data_ptr(), sm.data_ptr(), sm.data_ptr(), None, None, 0.1, 1e-5,
                                           kw.get("tab", ctab.data_ptr()), kw.get("y", codes.data_ptr()), sm.data_ptr(), sm.data_ptr(),
                                           sm.data_ptr(), n, h, w, c, kw.get("layout", NHWC), ws.data_ptr(), kw.get("ws_bytes", nbytes),
                                           _stream())
        torch.cuda.synchronize()
        assert rc in (_lib.ERR_ALIGNMENT, _lib.ERR_UNSUPPORTED, _lib.ERR_BAD_ARG), kw
        assert bool((codes == 0xEE).all()) and bool((sm == 7.0).all()), kw


def test_runs_on_the_current_stream():
    """The default stream is held by a sleep; a call on another stream completes meanwhile, with the same bits."""
    case = (B.ragged(32), False)
    shape = case[0]
    d = _inputs(case)
    x, gamma, beta = _dev(d)
    ctab = _ctab("swish", KAS[0], 8)

    def run():
        return _lc_fwd(shape, ctab, x, gamma, beta)

    want = run()
    from test_gpu_headline import _sleep_cycles
    cycles = _sleep_cycles(200)
    torch.cuda.synchronize()
    # HIP puts streams on a few hardware queues in turn, and a stream that shares the default stream's queue waits for the sleep
    # whatever the library does.  Four new streams, each used once: one of them runs beside the default stream, and the streams the
    # later test files draw keep the places in that turn that they had without this file.
    probe = torch.zeros(64, device=DEV)
    side = None
    for cand in [torch.cuda.Stream(device=DEV) for _ in range(4)]:
        cand.wait_stream(torch.cuda.current_stream())
        held, done = torch.cuda.Event(), torch.cuda.Event()
        torch.cuda._sleep(cycles // 10)
        held.record()
        with torch.cuda.stream(cand):
            probe.add_(1.0)
            done.record()
        done.synchronize()
        if side is None and not held.query():
            side = cand
        torch.cuda.synchronize()
    assert side is not None, "none of four streams runs beside the default stream"
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
    assert torch.equal(got[0], want[0])
    for a, b in zip(got[1:], want[1:]):
        assert _same(a, b)


# ---- the chain of a training step at the C level --------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["swish", "gelu"])
@pytest.mark.parametrize("name", ["dw-s1-c8", "pw-12-20", "dense-3x3-s1"])
def test_the_chain_equals_the_float32_chain(name, act):
    """new forward -> slfp_conv2d_bwd_codes -> slfp_bn_lut_train_bwd against LUT forward -> slfp_conv2d_bwd_ex ->
    slfp_bn_lut_train_bwd, for a depthwise 3x3, a 1x1 and a dense 3x3 reader: gw, gb of the conv and gx, ggamma, gbeta of the BN."""
    flags, n, spec = BWD_CASES[name]
    gen = torch.Generator().manual_seed(200 + len(name))
    mod = W._make(spec, 8, True, gen)
    ka = cf._f32(mod.Ka)
    shape = (n, spec.h, spec.w, spec.c_in)
    c = spec.c_in
    x = (torch.randn((n, c, spec.h, spec.w), generator=gen) * 1.5 + 0.3).to(DEV).contiguous(memory_format=torch.channels_last)
    gamma, beta = (torch.rand(c, generator=gen) + 0.5).to(DEV), (torch.randn(c, generator=gen) * 0.5).to(DEV)
    gy = torch.randn((n, spec.c_out, spec.h_out, spec.w_out), generator=gen).to(DEV).contiguous(memory_format=torch.channels_last)
    w = mod.weight.detach().contiguous()
    ftab, dtab = _tables(act)
    desc = cf._conv_desc(mod, x.shape, True, True)
    assert _lib.load().slfp_conv2d_bwd_codes_supported(ctypes.byref(desc), flags) == 1
    y, sm0, si0, lo0 = _lut_fwd(shape, ftab, x, gamma, beta)
    codes, sm, si, lo = _lc_fwd(shape, batchnorm.layerout_code_table([ACTS[act]()], ka, 8, DEV), x, gamma, beta)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(y).any())                             # the stated difference does not arise in this data
    want = _raw_bwd("slfp_conv2d_bwd_ex", desc, flags, y, w, gy, (True, True, True))
    got = _raw_bwd("slfp_conv2d_bwd_codes", desc, flags, codes, w, gy, (True, True, True))
    want += _lut_bwd(shape, dtab, x, want[0], gamma, beta, sm0, si0, lo0)
    got += _lut_bwd(shape, dtab, x, got[0], gamma, beta, sm, si, lo)
    torch.cuda.synchronize()
    for what, a, b in zip(("g", "gw", "gb", "gx", "ggamma", "gbeta"), got, want):
        assert torch.equal(a, b), what
    assert float(got[3].abs().max()) > 0 and float(got[1].abs().max()) > 0


def test_the_code_table_is_the_encoded_activation_table():
    vals, ncls = _values()
    conv = cf.conv2d_Q(8, 0.1, 0.2)(8, 8, 1)
    conv._post = (None, None, 2)                                      # a producer with the layer-output quantizer, no folded ReLU
    from cnns_slfp_quantization_amd.sfp_quant import hip_encode
    for act in ACTS:
        for ka, qbits in ((KAS[0], 8), (KAS[1], 7)):
            t = batchnorm.layerout_code_table([ACTS[act]()], ka, qbits, DEV)
            f = _tables(act)[0]
            enc = hip_encode(f, ka, _lib.FMT_SFP7 if qbits == 7 else _lib.FMT_ACT8)
            inf = fusion._layerout_table(conv, [ACTS[act]()], (ka, qbits), DEV)
            torch.cuda.synchronize()
            assert t.dtype == torch.uint8 and t.shape == (NT,) and t.data_ptr() % 16 == 0
            assert torch.equal(t[:ncls], enc[:ncls]) and torch.equal(t[:ncls], inf[:ncls])
            assert int(t[0]) == 0 and bool((t[ncls:] == 0).all())      # the NaN class and the padding
            assert torch.equal(inf[ncls:], enc[ncls:])                 # (the inference table encodes act(0) there)


# ---- module level: fusion.link_layerout_codes_train ---------------------------------------------------------------------------------
@contextlib.contextmanager
def _backward(mode):
    prev, det = cf.options.backward, torch.backends.cudnn.deterministic
    cf.options.backward = mode
    torch.backends.cudnn.deterministic = True   # the layers "hip" leaves to the composite run MIOpen: the same algorithm in both models
    try:
        yield
    finally:
        cf.options.backward, torch.backends.cudnn.deterministic = prev, det


def _image(seed=8):
    return torch.randn(4, 3, 8, 8, generator=torch.Generator().manual_seed(seed)).to(DEV).contiguous(memory_format=torch.channels_last)


def _step(m, x, grad=True):
    """One forward (+ backward) with hooks on every Conv2d_Q: logits, input gradient, parameter gradients, buffers, every input_q,
    and the dtype each conv received."""
    m.zero_grad(set_to_none=True)
    seen = []
    hooks = [c.register_forward_hook(lambda mod, inp, out: seen.append(inp[0].dtype)) for c in M.convs(m)]
    xi = x.clone(memory_format=torch.preserve_format).requires_grad_(grad)
    with contextlib.nullcontext() if grad else torch.no_grad():
        out = m(xi)
    if grad:
        (out.square().mean() + out.sum() * 0.1).backward()
    for hk in hooks:
        hk.remove()
    res = dict(logits=out.detach().clone(), gx=xi.grad, grads=[p.grad for p in m.parameters()],
               buffers=[b.clone() for b in m.buffers()], input_q=[c.input_q.clone() for c in M.convs(m)])
    return res, seen


def _pair(make):
    """(linked-to-be, unlinked reference): deep copies on the device, both on use_device_bn_layerout_train(min_elements=0), which is
    also what a linked wrapper falls back to."""
    model = make().to(DEV).to(memory_format=torch.channels_last)
    ref = copy.deepcopy(model)
    for m in (model, ref):
        assert fusion.use_device_bn_layerout_train(m, min_elements=0) > 0
        m.train()
    return model, ref


def _no_nan(res):
    assert all(bool(torch.isfinite(t).all()) for t in [res["logits"], *res["input_q"]])


def _wraps(m):
    return [w for w in m.modules() if isinstance(w, fusion.TrainBatchNormLayeroutCodes2d)]


def _received(model, wraps):
    linked = {id(w._conv) for w in wraps}
    return [torch.uint8 if id(c) in linked else torch.float32 for c in M.convs(model)]


@pytest.mark.parametrize("mode", ["hip", "hip_all"])
def test_linked_mobilenet_swish_stack_trains_bit_for_bit(mode):
    model, ref = _pair(M.mobilenet_swish_stack)
    assert fusion.link_layerout_codes_train(model, min_elements=0) == M.MOBILENET_LINKS
    wraps = _wraps(model)
    assert [w._conv for w in wraps] == M.convs(model)[1:] and M.intact(model) is None
    x = _image()
    opts = [O.DSGD(m.parameters(), 8, lr=0.05, momentum=0.9) for m in (model, ref)]
    with _backward(mode):
        for step in range(2):
            (got, seen), (want, seen_ref) = _step(model, x), _step(ref, x)
            _no_nan(want)                                             # the precondition: no exact zero behind a quantizer in this run
            assert seen == _received(model, wraps) and seen_ref == [torch.float32] * 5
            for w in wraps:   # the test cannot pass with nothing linked
                assert w._last_kernel == "bn_lut_codes_train", w._last_kernel
                assert "+codes_in" in w._conv._last_kernel, w._conv._last_kernel
                assert w._conv._last_bwd_kernel in ("dw3x3_bwd", "pw_bwd_mfma_f32"), w._conv._last_bwd_kernel
                assert w._conv._last_codes is not None and w._conv._last_input is None
            _assert_same(got, want, (mode, step))
            assert all(g is not None for g in got["grads"]) and got["gx"] is not None
            for o in opts:
                o.step()                                   # weights change through .data
            for p, q in zip(model.parameters(), ref.parameters()):
                assert torch.equal(p, q)
        # what the code path does not take runs what the unlinked model runs
        for m in (model, ref):
            m.eval()
        (got, seen), (want, _) = _step(model, x, grad=False), _step(ref, x, grad=False)
        _assert_same(got, want, "eval")
        assert seen == [torch.float32] * 5 and all(w._last_kernel == "aten" for w in wraps)
        stock = M.mobilenet_swish_stack().to(DEV).to(memory_format=torch.channels_last).eval()   # eval mode: the stock modules, bit for bit
        stock.load_state_dict(model.state_dict())
        _assert_same(got, _step(stock, x, grad=False)[0], "eval against the stock modules")
        for m in (model, ref):
            m.train()
    with _backward("composite"):
        (got, seen), (want, _) = _step(model, x), _step(ref, x)
        _assert_same(got, want, "composite")
        assert seen == [torch.float32] * 5 and all(w._last_kernel == "bn_lut_train" for w in wraps)
    with _backward(mode):
        # a Ka changed after linking: that pair falls back to float32 and still matches
        for m in (model, ref):
            M.convs(m)[2].Ka = torch.tensor(float(M.convs(m)[2].Ka) * 1.25)
        (got, seen), (want, _) = _step(model, x), _step(ref, x)
        _assert_same(got, want, "ka")
        assert [w._last_kernel for w in wraps] == ["bn_lut_codes_train", "bn_lut_train", "bn_lut_codes_train", "bn_lut_codes_train"]
        assert seen == [torch.float32, torch.uint8, torch.float32, torch.uint8, torch.uint8]
        # unlink, then a step: the never-linked model
        assert fusion.unlink_layerout_codes_train(model) == M.MOBILENET_LINKS
        (got, seen), (want, _) = _step(model, x), _step(ref, x)
        _assert_same(got, want, "unlinked")
        assert seen == [torch.float32] * 5 and not _wraps(model)


def test_linked_vgg_gelu_stack_trains_bit_for_bit_under_hip_all():
    model, ref = _pair(M.vgg_gelu_stack)
    assert fusion.link_layerout_codes_train(model, min_elements=0) == M.VGG_LINKS
    wraps = _wraps(model)
    x = _image()
    opts = [O.DSGD(m.parameters(), 8, lr=0.05, momentum=0.9) for m in (model, ref)]
    with _backward("hip_all"):
        for step in range(2):
            (got, seen), (want, _) = _step(model, x), _step(ref, x)
            _no_nan(want)
            _assert_same(got, want, step)
            assert seen == [torch.float32, torch.uint8, torch.float32, torch.uint8]   # never across a pool
            for w in wraps:
                assert w._last_kernel == "bn_lut_codes_train" and w._conv._last_bwd_kernel == "dense_bwd_mfma_f32"
            assert [type(model[i]).__name__ for i in (5, 14)] == ["TrainBatchNormLayerout2d"] * 2 and model[5]._last_kernel == "bn_lut_train"
            for o in opts:
                o.step()
    with _backward("hip"):   # no backward kernel reads these layers' codes without SLFP_BWD_DENSE: float32
        (got, seen), (want, _) = _step(model, x), _step(ref, x)
        _assert_same(got, want, "hip")
        assert seen == [torch.float32] * 4 and all(w._last_kernel == "bn_lut_train" for w in wraps)


def test_linked_sfp7_stack_trains_bit_for_bit():
    model, ref = _pair(lambda: M.mobilenet_swish_stack(q_bit=7, act=nn.GELU))
    assert fusion.link_layerout_codes_train(model, min_elements=0) == M.MOBILENET_LINKS
    wraps = _wraps(model)
    x = _image(9)
    with _backward("hip_all"):
        (got, seen), (want, _) = _step(model, x), _step(ref, x)
    _no_nan(want)
    _assert_same(got, want)
    assert seen == _received(model, wraps) and all(w._last_kernel == "bn_lut_codes_train" and w._q_bit == 7 for w in wraps)


def test_a_link_made_on_stock_modules_falls_back_to_them():
    """Linked without use_device_bn_layerout_train: below the size rule, and by default where the rule admits nothing, the call is
    F.batch_norm, the kept quantizer, the kept activation, and the conv sees float32."""
    make = lambda: M.mobilenet_swish_stack().to(DEV).to(memory_format=torch.channels_last).train()
    model, ref = make(), make()
    assert fusion.link_layerout_codes_train(model, min_elements=1 << 30) == M.MOBILENET_LINKS
    x = _image()
    with _backward("hip"):
        (got, seen), (want, _) = _step(model, x), _step(ref, x)
    _assert_same(got, want)
    assert seen == [torch.float32] * 5 and all(w._last_kernel == "aten" for w in _wraps(model))
    default = make()
    assert fusion.link_layerout_codes_train(default) == M.MOBILENET_LINKS
    floor = batchnorm.LUT_CODES_MIN_ELEMENTS
    if floor is None or 4 * 64 * 8 * 8 < floor:
        with _backward("hip"):
            (got, seen) = _step(default, x)
        _assert_same(got, want)
        assert seen == [torch.float32] * 5


def test_below_min_elements_stays_float32():
    model, ref = _pair(M.mobilenet_swish_stack)
    assert fusion.link_layerout_codes_train(model, min_elements=1 << 30) == M.MOBILENET_LINKS
    x = _image()
    with _backward("hip"):
        (got, seen), (want, _) = _step(model, x), _step(ref, x)
    _assert_same(got, want)
    assert seen == [torch.float32] * 5 and all(w._last_kernel == "bn_lut_train" for w in _wraps(model))
    assert all("codes" not in c._last_kernel for c in M.convs(model))
