"""GPU (MI355X): the global average pool kernel (csrc/pool_avg.hip), fusion.use_device_avgpool and
fusion.link_pool_head.

The kernel's contract is a fixed order of summation (include/slfp.h), restated here in NumPy from the header comment:
    s_j = float32 sum of v_p over p == j (mod 4), p ascending, from +0;   y = ((s_0 + s_1) + (s_2 + s_3)) / float32(HW)
so the result must equal the restatement bit for bit, in both layouts, whatever the batch.  Independently of any order, float32
accumulation of HW terms plus one division obeys  |y - mean64(v)| <= (HW + 1) 2^-24 mean64(|v|)  per element, and two such
results (the kernel's and ATen's) differ by at most twice that: both bounds are derived, not measured.
Shapes: every HW mod 4, HW < 4 and the workload sizes 7 x 7 and 13 x 13; C ragged against the 64 channel groups of a workgroup
(4, 20, 64, 1000; NCHW also 1, 10, 57); N = 1, 3, 130 (more than one workgroup).  Linear_Q needs out_features % 4 == 0 for its
weight-streaming kernel, so the small nets have 16 classes."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

GUARD = 64
HWS = [(1, 1), (1, 2), (1, 3), (2, 2), (1, 5), (2, 3), (1, 7), (3, 4), (7, 7), (13, 13)]
CS_NHWC, CS_NCHW_ONLY, NS = (4, 20, 64, 1000), (1, 10, 57), (1, 3, 130)
KINDS = {"signed1e-3": 1e-3, "signed1": 1.0, "signed30": 30.0, "postrelu": 1.0}
U = 2.0 ** -24


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


def _data(N, C, H, W, kind, seed):
    """[N, H, W, C] float32 on the host: signed normal data at the kind's scale, or max(normal, 0) with its exact zeros."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, C, generator=g) * KINDS[kind]
    return torch.relu(x) if kind == "postrelu" else x


def _contract(x_nhwc, relu):
    """The order of summation of include/slfp.h in NumPy float32; x_nhwc: [N, H, W, C]."""
    n, h, w, c = x_nhwc.shape
    v = x_nhwc.reshape(n, h * w, c).astype(np.float32)
    if relu:
        v = np.maximum(v, np.float32(0))
    s = np.zeros((4, n, c), dtype=np.float32)   # each partial starts from +0.0f
    for p in range(h * w):
        s[p % 4] = s[p % 4] + v[:, p, :]
    y = ((s[0] + s[1]) + (s[2] + s[3])) / np.float32(h * w)
    assert y.dtype == np.float32
    return y


def _pool(lib, x, layout, dims, relu=0, out=None, expect=0, y_offset=0):
    """slfp_global_avgpool_f32 into a buffer pre-filled with 0xFF (float32: NaN) / 0xA5 (codes) and followed by 64 guard bytes, which
    must come back unchanged.  x: the device tensor as it lies in memory; dims = (N, H, W, C); out = (Ka, q_bit) of the reader for
    code output; y_offset: bytes by which y is moved off its alignment.  Returns [N, C]; a refused call (expect != 0) must leave the
    whole buffer as it was filled and returns None."""
    N, H, W, C = dims
    io = lib.ConvIo(x_codes=0, y_codes=1 if out else 0, y_ka=out[0] if out else 1.0, y_qbits=out[1] if out else 8)
    nbytes = N * C * (1 if out else 4)
    buf = torch.full((y_offset + nbytes + GUARD,), 0xA5 if out else 0xFF, dtype=torch.uint8, device=x.device)
    buf[y_offset + nbytes:] = 0x5C
    fill = buf.clone()
    rc = lib.load().slfp_global_avgpool_f32(x.data_ptr(), buf.data_ptr() + y_offset, N, H, W, C, layout, relu, ctypes.byref(io), _stream())
    assert rc == expect, (rc, lib.last_error())
    torch.cuda.synchronize()
    assert bool((buf[y_offset + nbytes:] == 0x5C).all()), "guard bytes behind y were written"
    if expect != 0:
        assert torch.equal(buf, fill), "y was touched by a refused call"
        return None
    y = buf[y_offset:y_offset + nbytes]
    return y.view(N, C) if out else y.view(torch.float32).view(N, C)


def _encode(lib, t, ka, q):
    c = torch.empty(t.shape, dtype=torch.uint8, device=t.device)
    fmt = lib.FMT_ACT8 if q == 8 else lib.FMT_SFP7
    lib.check(lib.load().slfp_encode_f32(t.data_ptr(), c.data_ptr(), t.numel(), float(np.float32(ka)), fmt | lib.FMT_EXT, _stream()))
    return c


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("H,W", HWS, ids=[f"{h}x{w}" for h, w in HWS])
def test_kernel_contract(lib, dev, H, W, kind):
    """For every C and N of the module docstring, at this map size and kind of data:
    1. the float32 result is the NumPy restatement of the order bit for bit, in both layouts, relu 0 and 1;
    2. it lies within (HW + 1) 2^-24 mean64(|v|) of the double-precision mean;
    3. the NCHW result is torch.equal to the NHWC result on the same values;
    4. code output is torch.equal to slfp_encode_f32 of the kernel's own float32 output, q_bit 8 and 7, for reader scales that put
       y / Ka below the smallest class (Ka 1 on 1e-3 data), across the classes, and into both clamps (Ka 0.05 on data of scale 30)."""
    hw, scale = H * W, KINDS[kind]
    kas = (0.05, 1.0, float(np.float32(scale * 0.25 / math.sqrt(hw))))
    for C in CS_NHWC + CS_NCHW_ONLY:
        for N in NS:
            xh = _data(N, C, H, W, kind, seed=hw * 100003 + C * 131 + N)
            xn = xh.numpy()
            dims, tag = (N, H, W, C), (kind, H, W, C, N)
            x_nchw = xh.permute(0, 3, 1, 2).contiguous().to(dev)
            x_nhwc = xh.to(dev) if C % 4 == 0 else None
            for relu in (0, 1):
                want = _contract(xn, relu)
                v64 = (np.maximum(xn, 0) if relu else xn).astype(np.float64).reshape(N, hw, C)
                mean64, bound = v64.mean(axis=1), (hw + 1) * U * np.abs(v64).mean(axis=1)
                y_c = _pool(lib, x_nchw, lib.LAYOUT_NCHW, dims, relu)
                got = y_c.cpu().numpy()
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), ("NCHW vs the order", tag, relu, float(np.abs(got - want).max()))
                err = np.abs(got.astype(np.float64) - mean64)
                assert bool((err <= bound).all()), ("bound", tag, relu, float((err - bound).max()))
                if x_nhwc is not None:
                    y_l = _pool(lib, x_nhwc, lib.LAYOUT_NHWC, dims, relu)
                    assert np.array_equal(y_l.cpu().numpy().view(np.uint32), want.view(np.uint32)), ("NHWC vs the order", tag, relu)
                    assert torch.equal(y_c.view(torch.int32), y_l.view(torch.int32)), ("NCHW vs NHWC", tag, relu)
                    for q in (8, 7):
                        for ka in kas:
                            codes = _encode(lib, y_l.contiguous(), ka, q)
                            for x, layout in ((x_nhwc, lib.LAYOUT_NHWC), (x_nchw, lib.LAYOUT_NCHW)):
                                c = _pool(lib, x, layout, dims, relu, out=(ka, q))
                                assert torch.equal(c, codes), ("codes", tag, relu, q, ka, layout, int((c != codes).sum()))


def test_codes_cover_the_class_range(lib, dev):
    """The reader scales of test_kernel_contract reach what they are meant to: both clamps, exact zero, the tiny class, and most of
    the regular classes of SLFP<3,4> in between."""
    N, H, W, C = 130, 7, 7, 64
    seen = set()
    for kind, ka in (("signed30", 0.05), ("signed1e-3", 1.0), ("signed1", float(np.float32(0.25 / 7))), ("postrelu", 0.05)):
        x = _data(N, C, H, W, kind, seed=9).to(dev)
        seen |= set(_pool(lib, x, lib.LAYOUT_NHWC, (N, H, W, C), 0, out=(ka, 8)).unique().tolist())
    assert {0x02, 0x82} <= seen, "both clamp literals"
    assert 0x00 in seen or 0x80 in seen, "the tiny class"
    assert len(seen) > 128, len(seen)
    z = torch.zeros(2, H, W, C, device=dev)
    assert _pool(lib, z, lib.LAYOUT_NHWC, (2, H, W, C), 0, out=(0.05, 8)).unique().tolist() == [0x01]   # exact zero


@pytest.mark.parametrize("H,W,C", [(7, 7, 64), (13, 13, 1000), (1, 3, 20), (2, 3, 57)])
def test_rows_do_not_depend_on_the_batch(lib, dev, H, W, C):
    N = 130
    xh = _data(N, C, H, W, "signed1", seed=3)
    forms = [(xh.permute(0, 3, 1, 2).contiguous().to(dev), lib.LAYOUT_NCHW, lambda t, r: t[r:r + 1].clone())]
    if C % 4 == 0:
        forms.append((xh.to(dev), lib.LAYOUT_NHWC, lambda t, r: t[r:r + 1].clone()))
    for x, layout, row in forms:
        outs = [None] + ([(0.11, 8), (0.11, 7)] if C % 4 == 0 else [])
        for out in outs:
            y = _pool(lib, x, layout, (N, H, W, C), 1, out=out)
            for r in (0, 1, 15, 16, 63, 64, 65, 129):
                y1 = _pool(lib, row(x, r), layout, (1, H, W, C), 1, out=out)
                assert torch.equal(y1.view(torch.uint8), y[r:r + 1].contiguous().view(torch.uint8)), (layout, out, r)


def test_unsupported_arguments_leave_y_untouched(lib, dev):
    N, H, W = 3, 7, 7
    x64 = _data(N, 64, H, W, "signed1", seed=5).to(dev)
    x10 = _data(N, 10, H, W, "signed1", seed=6).to(dev)
    U_, B, A, S = lib.ERR_UNSUPPORTED, lib.ERR_BAD_ARG, lib.ERR_ALIGNMENT, lib.ERR_SHAPE
    _pool(lib, x10, lib.LAYOUT_NHWC, (N, H, W, 10), expect=U_)                       # NHWC needs C % 4 == 0
    _pool(lib, x10, lib.LAYOUT_NCHW, (N, H, W, 10), out=(0.3, 8), expect=U_)         # so do codes
    _pool(lib, x64, lib.LAYOUT_NHWC, (N, H, W, 64), out=(0.0, 8), expect=U_)
    _pool(lib, x64, lib.LAYOUT_NHWC, (N, H, W, 64), out=(0.3, 6), expect=B)
    _pool(lib, x64, 7, (N, H, W, 64), expect=B)
    _pool(lib, x64, lib.LAYOUT_NHWC, (N, H, W, 64), relu=2, expect=B)
    _pool(lib, x64, lib.LAYOUT_NHWC, (N, 0, W, 64), expect=S)
    _pool(lib, x64, lib.LAYOUT_NHWC, (N, H, W, 64), expect=A, y_offset=4)            # NHWC: 16-byte aligned y
    _pool(lib, x64, lib.LAYOUT_NCHW, (N, H, W, 64), expect=A, y_offset=2)            # NCHW: 4-byte aligned y
    assert _pool(lib, x64, lib.LAYOUT_NCHW, (N, H, W, 64), y_offset=4).shape == (N, 64)   # ... which is enough there
    _pool(lib, x64, lib.LAYOUT_NHWC, (0, H, W, 64))                                  # n == 0: SLFP_OK, nothing written


def test_binding(lib, dev):
    from cnns_slfp_quantization_amd.sfp_quant import hip_global_avgpool, hip_encode
    xh = _data(5, 20, 3, 4, "signed1", seed=8)
    x = xh.permute(0, 3, 1, 2).contiguous().to(dev)                    # [N, C, H, W]
    want = torch.from_numpy(_contract(xh.numpy(), 0)).to(dev).view(5, 20, 1, 1)
    for t in (x, x.contiguous(memory_format=torch.channels_last), x[:, :, :, :]):
        y = hip_global_avgpool(t)
        assert y.shape == (5, 20, 1, 1) and y.dtype == torch.float32 and torch.equal(y, want)
    y = hip_global_avgpool(x[:, :10].contiguous(memory_format=torch.channels_last))   # C = 10: read as NCHW after a copy
    assert torch.equal(y, want[:, :10])
    assert torch.equal(hip_global_avgpool(x, relu=True), torch.from_numpy(_contract(xh.numpy(), 1)).to(dev).view(5, 20, 1, 1))
    c = hip_global_avgpool(x, code_out=(0.11, 7))
    assert c.dtype == torch.uint8 and c.shape == (5, 20, 1, 1) and torch.equal(c, hip_encode(want, 0.11, lib.FMT_SFP7))
    with pytest.raises(RuntimeError):
        hip_global_avgpool(x.cpu())


# ------------------------------------------------------------------ the passes on small nets
KA, KW, CH, CLASSES = 0.25, 0.02, 64, 16


class _Net(nn.Module):
    """conv2d_Q 3x3 -> BN -> ReLU -> pool -> flatten -> Linear_Q with the reference nets' spellings of the head."""

    def __init__(self, spelling, aux=False):
        super().__init__()
        from cnns_slfp_quantization_amd import conv2d_func as cf
        Conv, Lin = cf.conv2d_Q(8, KW, KA), cf.linear_Q(8, KW, KA)
        self.spelling = spelling
        if spelling == "squeeze":   # nets_imgnet/squeezenet1_0.py: final conv -> ReLU -> pool inside one nn.Sequential, no Linear
            self.classifier = nn.Sequential(Conv(16, 20, 3, padding=1), nn.ReLU(inplace=True), nn.AdaptiveAvgPool2d((1, 1)))
            return
        self.features = nn.Sequential(Conv(16, CH, 3, padding=1), nn.BatchNorm2d(CH), nn.ReLU())
        self.avgpool = {"module": nn.AdaptiveAvgPool2d(1), "functional": nn.AdaptiveAvgPool2d((1, 1)), "view": nn.AvgPool2d(8)}[spelling]
        self.flatten = nn.Flatten() if spelling == "module" else None
        self.fc = Lin(CH, CLASSES)
        self.aux = nn.Linear(CH, 1) if aux else None

    def forward(self, x):
        if self.spelling == "squeeze":
            t = self.classifier(x)
            return t.view(t.size(0), -1)
        t = self.avgpool(self.features(x))
        t = self.flatten(t) if self.spelling == "module" else (torch.flatten(t, 1) if self.spelling == "functional" else t.view(-1, CH))
        y = self.fc(t)
        return y + self.aux(t) if self.aux is not None else y


def _net(dev, spelling, aux=False):
    torch.manual_seed(7)
    m = _Net(spelling, aux)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() > 1 and "aux" not in name:
                p.mul_(KW * 40)
        for b in m.modules():
            if isinstance(b, nn.BatchNorm2d):
                b.running_mean.normal_(0, 0.1)
                b.running_var.uniform_(0.5, 2.0)
    m = m.to(dev).eval().to(memory_format=torch.channels_last)
    x = (torch.randn(6, 16, 8, 8) * KA * 4).to(dev).contiguous(memory_format=torch.channels_last)
    return m, x


def _pool_io(m, x):
    """(input, output) of the pool slot during one forward, and the model's output."""
    slot = m.classifier[2] if m.spelling == "squeeze" else m.avgpool
    seen = []
    h = slot.register_forward_hook(lambda mod, inp, out: seen.append((inp[0].detach().clone(), out.detach().clone())))
    with torch.no_grad():
        y = m(x)
    h.remove()
    assert len(seen) == 1
    return seen[0][0], seen[0][1], y


def _within_aten_bound(got, want, pooled_in):
    hw = pooled_in.shape[2] * pooled_in.shape[3]
    bound = 2 * (hw + 1) * U * pooled_in.double().abs().mean(dim=(2, 3), keepdim=True)
    err = (got.double() - want.double()).abs()
    return got.shape == want.shape and bool((err <= bound).all()), float((err - bound).max())


@pytest.mark.parametrize("spelling", ["module", "functional", "view", "squeeze"])
def test_passes_on_small_nets(dev, spelling):
    from cnns_slfp_quantization_amd import fusion
    m, x = _net(dev, spelling)
    slots = {name: mod for name, mod in m.named_modules()}
    keys = list(m.state_dict())
    xin, p_aten, y_aten = _pool_io(m, x)
    with torch.no_grad():
        assert fusion.use_device_avgpool(m, x) == 1
        pool = m.classifier[2] if spelling == "squeeze" else m.avgpool
        assert isinstance(pool, fusion.GlobalAvgPool2d) and pool.mod is slots["classifier.2" if spelling == "squeeze" else "avgpool"]
        assert list(m.state_dict()) == keys
        _, p_dev, y_dev = _pool_io(m, x)
        # (an in-place ReLU in front has run on `xin` by the time the hook copies it: the pooled values either way)
        ok, over = _within_aten_bound(p_dev, p_aten, torch.relu(xin))
        assert ok, over
        if spelling == "squeeze":
            assert pool._relu is True and isinstance(m.classifier[1], fusion.FoldedReLU) and pool._last_kernel == "global_avgpool+relu"
            assert fusion.link_pool_head(m, x) == 0   # no Linear_Q behind the pool
        else:
            assert pool._relu is False and pool._last_kernel == "global_avgpool"
            assert fusion.link_pool_head(m, x) == 1
            assert pool._code_out == (KA, 8) and m.fc._code_in is True
            y_link = m(x)
            assert torch.equal(y_link.view(torch.int32), y_dev.view(torch.int32)), float((y_link - y_dev).abs().max())
            assert pool._last_kernel == "global_avgpool+codes_out" and m.fc._last_kernel == "linear_fc+codes_in"
            assert fusion.link_pool_head(m, x) == 0   # nothing left to link
            assert fusion.link_head(m, x) == 0        # the reader is linked already: no second link, no exception
            assert torch.equal(m(x).view(torch.int32), y_dev.view(torch.int32))
            assert fusion.unlink_pool_head(m) == 1
            assert pool._code_out is None and m.fc._code_in is False and "_pool_link" not in pool.__dict__
            assert torch.equal(m(x).view(torch.int32), y_dev.view(torch.int32)) and m.fc._last_kernel == "linear_pointwise"
        assert fusion.restore_avgpool(m) == 1
        assert {name: mod for name, mod in m.named_modules()} == slots   # every slot holds its original module
        assert torch.equal(m(x).view(torch.int32), y_aten.view(torch.int32))


def test_restore_takes_the_link_along(dev):
    from cnns_slfp_quantization_amd import fusion
    m, x = _net(dev, "module")
    slots = {name: mod for name, mod in m.named_modules()}
    with torch.no_grad():
        y_aten = m(x)
        assert fusion.use_device_avgpool(m, x) == 1 and fusion.link_pool_head(m, x) == 1
        assert fusion.restore_avgpool(m) == 1
        assert {name: mod for name, mod in m.named_modules()} == slots and m.fc._code_in is False
        assert torch.equal(m(x), y_aten)


def test_a_second_reader_of_the_pooled_tensor_prevents_the_link(dev):
    from cnns_slfp_quantization_amd import fusion
    m, x = _net(dev, "module", aux=True)
    with torch.no_grad():
        assert fusion.use_device_avgpool(m, x) == 1
        y_dev = m(x)
        assert fusion.link_pool_head(m, x) == 0
        assert m.avgpool._code_out is None and m.fc._code_in is False
        assert torch.equal(m(x), y_dev)


def test_wrapper_falls_back_where_the_kernel_does_not_apply(dev):
    from cnns_slfp_quantization_amd import fusion
    wrap = fusion.GlobalAvgPool2d(nn.AvgPool2d(4).eval())
    x = torch.randn(2, 8, 8, 8, device=dev)
    with torch.no_grad():
        assert torch.equal(wrap(x), wrap.mod(x)) and wrap._last_kernel == "aten"      # 8 x 8 under a 4 x 4 window: not global
        y = wrap(x[:, :, :4, :4].contiguous())
        assert wrap._last_kernel == "global_avgpool" and y.shape == (2, 8, 1, 1)
    xg = x[:, :, :4, :4].clone().requires_grad_(True)
    assert wrap(xg).requires_grad and wrap._last_kernel == "aten"                     # grad enabled


def test_image_groups_give_the_same_logits(dev):
    """Every kernel of the forward is row-independent once the pool is: groups of 3 + 3 images equal the batch of 6, bit for bit."""
    from cnns_slfp_quantization_amd import fusion, streams
    m, x = _net(dev, "functional")
    with torch.no_grad():
        assert fusion.use_device_avgpool(m, x) == 1
        y = m(x)
        yg = streams.forward_image_groups(m, x, groups=2)
        torch.cuda.synchronize()
        assert torch.equal(yg.view(torch.int32), y.view(torch.int32)), float((yg - y).abs().max())
        assert fusion.link_pool_head(m, x) == 1
        yg = streams.forward_image_groups(m, x, groups=2)
        torch.cuda.synchronize()
        assert torch.equal(yg.view(torch.int32), y.view(torch.int32))
