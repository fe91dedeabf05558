"""GPU (MI355X): the weight-streaming Linear_Q kernel (csrc/linear_fc.hip) and fusion.link_head.

The contract is bit-identity with the pointwise path: float32 output torch.equal to slfp_linear_fwd_prepared (+ torch.relu) for the same
arguments, whether x arrives as float32 or as its codes, and code output equal to slfp_encode_f32 of that float32 result for the
reader's (Ka, q_bit).  Shapes are the smallest at which the kernel can go wrong: M ragged against the 16-row MFMA tile and the 64-row
block (1, 5, 16, 17, 64, 65, 130), K with an odd k-step count (96), on both sides of the stream / tiled threshold of the path it must
match (<= 256 / above) and on both code-load forms (K % 64), N ragged against the 16-channel tile (100) and across the 256 / 512 tile
thresholds of the pointwise selection (272, 528)."""
import ctypes
import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn

from _bars import TOL_EXACT, TOL_F16X1
from conftest import rel_errors
from oracle import slfp_oracle as so

pytestmark = pytest.mark.gpu

KA, KW = 0.25, 0.02
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from cnns_slfp_quantization_amd import _lib
    L = _lib.load()   # raises if libslfp_hip.so is missing: no fallback
    assert L.slfp_device_count() >= 1
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _fmt(lib, q):
    return lib.FMT_ACT8 if q == 8 else lib.FMT_SFP7


def _inputs(M, K, N, dev, seed):
    """x with |x / Ka| from far below the smallest class (2^-9) to beyond the clamp (2^5), both signs, some exact zeros."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp2(torch.rand(M, K, generator=g) * 14.0 - 9.0) * KA
    sign = torch.where(torch.rand(M, K, generator=g) < 0.5, -1.0, 1.0)
    x = mag * sign
    x[torch.rand(M, K, generator=g) < 0.03] = 0.0
    w = torch.randn(N, K, generator=g) * (KW * 3.0)
    b = torch.randn(N, generator=g) * 0.5
    return x.to(dev), w.to(dev), b.to(dev)


def _encode(lib, t, ka, q):
    c = torch.empty(t.shape, dtype=torch.uint8, device=t.device)
    lib.check(lib.load().slfp_encode_f32(t.data_ptr(), c.data_ptr(), t.numel(), ka, _fmt(lib, q) | lib.FMT_EXT, _stream()))
    return c


def _blob(lib, w, q, passes=0):
    L = lib.load()
    N, K = w.shape
    blob = torch.empty(max(L.slfp_linear_workspace_bytes(1, K, N), 16), dtype=torch.uint8, device=w.device)
    lib.check(L.slfp_linear_prepare_weights(w.data_ptr(), blob.data_ptr(), K, N, KW, q, passes, _stream()))
    return blob


def _pointwise(lib, x, blob, b, N, q, passes=0):
    M, K = x.shape
    y = torch.empty(M, N, dtype=torch.float32, device=x.device)
    lib.check(lib.load().slfp_linear_fwd_prepared(x.data_ptr(), blob.data_ptr(), b.data_ptr(), y.data_ptr(), M, K, N, KA, KW, q, passes, _stream()))
    return y


def _fc(lib, x, blob, b, N, q, out=None, relu=0, passes=0, expect=0):
    """slfp_linear_fwd_fc into a buffer pre-filled with NaN (float32) / 0xA5 (codes) and followed by 64 guard bytes, which must come
    back unchanged.  out = (Ka, q_bit) of the reader for code output.  Returns the output tensor (expect != 0: the untouched fill)."""
    L = lib.load()
    M, K = x.shape
    io = lib.ConvIo(x_codes=1 if x.dtype == torch.uint8 else 0, y_codes=1 if out else 0, y_ka=out[0] if out else 1.0,
                    y_qbits=out[1] if out else 8)
    nbytes = M * N * (1 if out else 4)
    buf = torch.full((nbytes + GUARD,), 0xA5 if out else 0xFF, dtype=torch.uint8, device=x.device)
    buf[nbytes:] = 0x5C
    fill = buf[:nbytes].clone()
    ws_bytes = L.slfp_linear_fc_workspace_bytes(M, K, N, ctypes.byref(io))
    assert (ws_bytes == 0) == (x.dtype == torch.uint8)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=x.device)
    rc = L.slfp_linear_fwd_fc(x.data_ptr(), blob.data_ptr(), b.data_ptr(), buf.data_ptr(), M, K, N, KA, KW, q, passes, ctypes.byref(io),
                              relu, ws.data_ptr() if ws_bytes else None, _stream())
    assert rc == expect, (rc, lib.last_error())
    torch.cuda.synchronize()
    assert bool((buf[nbytes:] == 0x5C).all()), "guard bytes behind y were written"
    if expect != 0:
        assert torch.equal(buf[:nbytes], fill), "y was touched by a refused call"
    y = buf[:nbytes]
    return y.view(M, N) if out else y.view(torch.float32).view(M, N)


def _cases():
    """A pruned cross product: every (K, N) pair once with M cycling through its list, then every M against the shapes that cross
    the most thresholds.  q_bit, ReLU and the reader's q_bit alternate."""
    Ms, Ks, Ns = (1, 5, 16, 17, 64, 65, 130), (32, 96, 256, 320, 1024), (16, 48, 100, 272, 528)
    out, i = [], 0
    for K in Ks:
        for N in Ns:
            out.append((Ms[i % len(Ms)], K, N))
            i += 1
    for M in Ms:
        out.append((M, 320, 272))
        out.append((M, 256, 528 if M % 2 else 100))
    cases = []
    for j, (M, K, N) in enumerate(dict.fromkeys(out)):
        q = 8 if j % 2 == 0 else 7
        cases.append(pytest.param(M, K, N, q, j % 3 != 0, 7 if (j // 2) % 2 else 8, id=f"M{M}-K{K}-N{N}-q{q}"))
    assert len(cases) <= 40
    return cases


@pytest.mark.parametrize("M,K,N,q,relu,yq", _cases())
def test_fc_is_bit_identical_to_the_pointwise_path(lib, dev, M, K, N, q, relu, yq):
    x, w, b = _inputs(M, K, N, dev, seed=1000 * M + K + N)
    blob = _blob(lib, w, q)
    ref = _pointwise(lib, x, blob, b, N, q)
    ref = torch.relu(ref) if relu else ref
    xc = _encode(lib, x, KA, q)
    for xin in (x, xc):
        y = _fc(lib, xin, blob, b, N, q, relu=1 if relu else 0)
        assert not torch.isnan(y).any(), "an element of y was not written"
        assert torch.equal(y.view(torch.int32), ref.view(torch.int32)), (str(xin.dtype), float((y - ref).abs().max()))
    assert torch.equal(_fc(lib, xc, blob, b, N, q, relu=1 if relu else 0), y)   # two runs are equal
    if N % 16 == 0:
        y_ka = 0.37
        want = _encode(lib, ref, y_ka, yq)
        for xin in (x, xc):
            c = _fc(lib, xin, blob, b, N, q, out=(y_ka, yq), relu=1 if relu else 0)
            assert torch.equal(c, want), (str(xin.dtype), int((c != want).sum()))
        assert torch.equal(_fc(lib, xc, blob, b, N, q, out=(y_ka, yq), relu=1 if relu else 0), c)


@pytest.mark.parametrize("M,K,N,q", [(5, 96, 100, 8), (17, 320, 272, 8), (130, 1024, 528, 8), (65, 256, 48, 7), (16, 1024, 272, 7)])
def test_fc_against_the_oracle(lib, dev, M, K, N, q):
    """Bars by analogy with the pointwise families (tests/_bars.py): TOL_F16X1 for the single-pass mode at q_bit 8, TOL_EXACT at q_bit 7
    (SFP<3,3> operands are exact in fp16)."""
    x, w, b = _inputs(M, K, N, dev, seed=7 + M + K + N)
    y = _fc(lib, x, _blob(lib, w, q), b, N, q)
    ref = so.linear(x.cpu().numpy(), w.cpu().numpy(), b.cpu().numpy(), KA, KW, q)
    e_max, e_l2 = rel_errors(y.cpu().numpy(), ref)
    print(f"fc vs oracle M{M} K{K} N{N} q{q}: max {e_max:.3e} l2 {e_l2:.3e}")
    bar = TOL_F16X1 if q == 8 else TOL_EXACT
    assert e_max <= bar and e_l2 <= bar, (e_max, e_l2)


def test_rows_do_not_depend_on_the_batch(lib, dev):
    M, K, N, q = 130, 320, 272, 8
    x, w, b = _inputs(M, K, N, dev, seed=3)
    blob = _blob(lib, w, q)
    y = _fc(lib, x, blob, b, N, q)
    c = _fc(lib, x, blob, b, N, q, out=(0.37, 8), relu=1)
    for r in (0, 15, 16, 63, 64, 129):
        xr = x[r:r + 1].clone()
        assert torch.equal(_fc(lib, xr, blob, b, N, q), y[r:r + 1]), r
        assert torch.equal(_fc(lib, xr, blob, b, N, q, out=(0.37, 8), relu=1), c[r:r + 1]), r


def test_forced_tilings_give_the_same_bits(lib, dev):
    """slfp_debug_linear_fc_tiles: every n-tile width and row-tile count the kernel is built with computes the same element."""
    M, K, N, q = 65, 320, 272, 8
    x, w, b = _inputs(M, K, N, dev, seed=4)
    blob = _blob(lib, w, q)
    ref = _pointwise(lib, x, blob, b, N, q)
    L = lib.load()
    try:
        for ntw in (1, 2, 4):
            for mt in (1, 2, 4):
                assert L.slfp_debug_linear_fc_tiles(ntw, mt) == 0
                assert torch.equal(_fc(lib, x, blob, b, N, q), ref), (ntw, mt)
        assert L.slfp_debug_linear_fc_tiles(3, 0) == lib.ERR_BAD_ARG
    finally:
        assert L.slfp_debug_linear_fc_tiles(0, 0) == 0


def test_unsupported_arguments_leave_y_untouched(lib, dev):
    x, w, b = _inputs(17, 320, 272, dev, seed=5)
    blob = _blob(lib, w, 8, passes=lib.MFMA_F16X3)
    _fc(lib, x, blob, b, 272, 8, passes=lib.MFMA_F16X3, expect=lib.ERR_UNSUPPORTED)
    _fc(lib, x, blob, b, 272, 8, out=(0.0, 8), expect=lib.ERR_UNSUPPORTED)
    _fc(lib, x, blob, b, 272, 8, out=(0.37, 6), expect=lib.ERR_UNSUPPORTED)
    _fc(lib, x, blob, b, 272, 8, relu=2, expect=lib.ERR_UNSUPPORTED)
    _fc(lib, x[:, :48].contiguous(), blob, b, 272, 8, expect=lib.ERR_UNSUPPORTED)
    x2, w2, b2 = _inputs(5, 96, 100, dev, seed=6)
    _fc(lib, x2, _blob(lib, w2, 8), b2, 100, 8, out=(0.37, 8), expect=lib.ERR_UNSUPPORTED)


# ------------------------------------------------------------------ the module
@pytest.mark.parametrize("M,K,N", [(17, 320, 272), (5, 256, 100)])
def test_linear_q_under_the_fc_option_returns_the_same_tensor(dev, M, K, N):
    import utils.conv2d_func as cf
    from cnns_slfp_quantization_amd.sfp_quant import hip_quantize
    x, w, b = _inputs(M, K, N, dev, seed=11)
    lin = cf.linear_Q(8, KW, KA)(K, N).to(dev).eval()
    with torch.no_grad():
        lin.weight.copy_(w)
        lin.bias.copy_(b)
        y0 = lin(x)
        try:
            cf.options.linear_kernel = "fc"
            assert lin._last_kernel == "linear_pointwise"
            y1 = lin(x)
            assert lin._last_kernel == "linear_fc"   # the option selected the new kernel
            assert torch.equal(y1.view(torch.int32), y0.view(torch.int32))
            assert torch.equal(lin.input_q, hip_quantize(x, KA, 0))
            cf.options.mfma_passes = 3   # F16X3: no fc kernel, the option falls back to the pointwise path
            y3 = lin(x)
            assert lin._last_kernel == "linear_pointwise"
            cf.options.linear_kernel = "pointwise"
            assert torch.equal(lin(x).view(torch.int32), y3.view(torch.int32))
        finally:
            cf.options.linear_kernel = "pointwise"
            cf.options.mfma_passes = 0
    with pytest.raises(TypeError):
        lin(torch.zeros(M, K, dtype=torch.uint8, device=dev))   # not marked as a reader


# ------------------------------------------------------------------ heads
def _vgg16(dev):
    """tests/golden/netgen_r3.VGG16_Q with the fixture's name-seeded parameters, on a 32 x 32 batch of 4 (the CIFAR geometry: 1 x 1
    behind the fifth pool, so the adaptive pool in front of fc1 is an identity)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import netgen_r3 as ng
    import utils.conv2d_func as cf
    import utils.sfp_quant as sq
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nets_r3_golden.npz"))
    q, batch, in_seed, seed = [int(v) for v in gold["vgg16:meta"]]
    manifest = json.loads(bytes(gold["vgg16:manifest"]).decode())
    gains = json.loads(bytes(gold["vgg16:gains"]).decode())
    m = ng.BUILDERS["vgg16"](ng.Factories(cf, q, manifest, layerout=sq.layerout_quantize_func))
    ng.fill_parameters_by_name(m, seed, gains)
    ng.load_bn_stats_by_name_(m, {k[len("vgg16") + 1:]: gold[k] for k in gold.files if k.startswith("vgg16:bn:")})
    m = m.to(dev).eval().to(memory_format=torch.channels_last)
    x = ng.net_input224(4, in_seed)[:, :, :32, :32].to(dev).contiguous(memory_format=torch.channels_last)
    return m, x


class _AlexHead(nn.Module):
    """An AlexNet-shaped head: conv -> ReLU -> MaxPool(3, 2) -> flatten -> Dropout -> three Linear_Q with ReLU / Dropout between."""

    def __init__(self, cf, scale_flat=None):
        super().__init__()
        Conv, Lin = cf.conv2d_Q_bias(8, KW, KA), cf.linear_Q(8, KW, KA)
        self.features = nn.Sequential(Conv(16, 32, 3, padding=1), nn.ReLU(), nn.MaxPool2d(3, 2))
        self.classifier = nn.Sequential(nn.Dropout(), Lin(1152, 64), nn.ReLU(), nn.Dropout(), Lin(64, 64), nn.ReLU(), Lin(64, 12))
        self.scale_flat = scale_flat

    def forward(self, x):
        t = torch.flatten(self.features(x), 1)
        if self.scale_flat is not None:
            t = t * self.scale_flat   # arithmetic on the flattened tensor: hooks cannot see it
        return self.classifier(t)


def _alex(dev, scale_flat=None):
    import utils.conv2d_func as cf
    torch.manual_seed(5)
    m = _AlexHead(cf, scale_flat)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(KW * 40 if p.dim() > 1 else 1.0)
    m = m.to(dev).eval().to(memory_format=torch.channels_last)
    x = (torch.randn(4, 16, 13, 13) * KA * 4).to(dev).contiguous(memory_format=torch.channels_last)
    return m, x


def _hand_overs(m, x):
    """dtype of the input of every Linear_Q during one forward."""
    seen, hooks = [], []
    for mod in m.modules():
        if isinstance(mod, nn.Linear):
            hooks.append(mod.register_forward_hook(lambda mod, inp, out: seen.append(inp[0].dtype)))
    with torch.no_grad():
        y = m(x)
    for h in hooks:
        h.remove()
    return y, seen


def _check_head(m, x, prepare, n_links):
    from cnns_slfp_quantization_amd import fusion
    with torch.no_grad():
        prepare(m, x)
        y0 = m(x)
        slots = {name: mod for name, mod in m.named_modules()}
        n = fusion.link_head(m, x)
        assert n == n_links, n
        y1, seen = _hand_overs(m, x)
        assert torch.equal(y1.view(torch.int32), y0.view(torch.int32)), float((y1 - y0).abs().max())
        assert seen == [torch.uint8] * len(seen) and len(seen) == 3, seen   # every linked hand-over is 1-byte codes
        lins = [mod for mod in m.modules() if isinstance(mod, nn.Linear)]
        assert [l._code_in for l in lins] == [True, True, True]
        assert [l._last_kernel for l in lins] == ["linear_fc+codes_in+codes_out"] * 2 + ["linear_fc+codes_in"]
        assert lins[0]._code_out is not None and lins[1]._code_out is not None and lins[2]._code_out is None
        assert torch.equal(lins[1].input_q, torch.relu(lins[1].input_q))   # decoded codes, behind the folded ReLU
        assert fusion.unlink_head(m) == n_links
        assert {name: mod for name, mod in m.named_modules()} == slots   # every slot is back
        for l in lins:
            assert l._code_in is False and l._code_out is None and l._code_relu is False
        y2, seen = _hand_overs(m, x)
        assert seen == [torch.float32] * 3 and torch.equal(y2.view(torch.int32), y0.view(torch.int32))


def test_link_head_vgg16(dev):
    from cnns_slfp_quantization_amd import fusion

    def prepare(m, x):
        assert fusion.fuse_bn_relu(m) == 13
        assert fusion.link_codes(m, x) > 0   # the last conv of layer5 reads codes
    m, x = _vgg16(dev)
    _check_head(m, x, prepare, 3)   # layer5 -> fc1, fc1 -> fc2, fc2 -> fc3


def test_link_head_alexnet_shaped(dev):
    m, x = _alex(dev)
    _check_head(m, x, lambda m, x: None, 3)   # conv -> fc1 (ReLU, pool and flatten on codes), fc1 -> fc2, fc2 -> fc3


def test_link_head_rolls_back_arithmetic_on_the_flattened_tensor(dev):
    from cnns_slfp_quantization_amd import fusion
    m, x = _alex(dev, scale_flat=1.0)   # t * 1.0: the values flatten(1) gave, so the conv -> fc1 candidate is found
    with torch.no_grad():
        y0 = m(x)
        slots = {name: mod for name, mod in m.named_modules()}
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            assert fusion.link_head(m, x) == 0
        assert any("link_head" in str(i.message) for i in w), [str(i.message) for i in w]
        assert {name: mod for name, mod in m.named_modules()} == slots
        assert all(not l._code_in and l._code_out is None for l in m.modules() if isinstance(l, nn.Linear))
        assert m.features[0]._code_out is None
        assert torch.equal(m(x), y0)


def test_linked_head_without_the_fc_kernel_keeps_the_bits(dev):
    """options.mfma_passes = 3 (F16X3) has no fc kernel: a head linked in the single-pass mode then runs every Linear_Q through
    decode -> float32 interface -> encode.  The codes stand for QA(x / Ka), so the float32 interface must be handed that times Ka
    (Ka = 0.25 here: a missing scale makes every operand 4x too large); the logits must be those of the unlinked head under F16X3."""
    import utils.conv2d_func as cf
    from cnns_slfp_quantization_amd import fusion
    m, x = _alex(dev)
    lins = [mod for mod in m.modules() if isinstance(mod, nn.Linear)]
    try:
        with torch.no_grad():
            cf.options.mfma_passes = 3
            y3 = m(x)
            cf.options.mfma_passes = 0
            y1 = m(x)
            assert fusion.link_head(m, x) == 3
            assert torch.equal(m(x).view(torch.int32), y1.view(torch.int32))
            cf.options.mfma_passes = 3
            y, seen = _hand_overs(m, x)
            assert seen == [torch.uint8] * 3 and [l._last_kernel for l in lins] == ["linear_pointwise"] * 3
            assert torch.equal(y.view(torch.int32), y3.view(torch.int32)), float((y - y3).abs().max())
            assert not torch.equal(y3, y1)   # the two modes differ on this input: the comparison above is no tautology
    finally:
        cf.options.mfma_passes = 0
