"""CPU: the host side of the training-mode BatchNorm2d kernels: the five exports and the contract text, the
query and the refusals of slfp_bn_train_fwd / slfp_bn_train_bwd (all before any device work), the split rule, the CPU pre-check
of the GPU test's inputs, and fusion.TrainBatchNorm2d / use_device_bn_train / restore_bn_train on a model without a device."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _bn_cases as B
from _bars import TOL_EXACT
from _bn_calls import _bars_ok, _sum_bars_ok
from cnns_slfp_quantization_amd import _lib, fusion
from cnns_slfp_quantization_amd.sfp_quant import layerout_quantize_func

NEW = ("slfp_bn_train_supported", "slfp_bn_train_workspace_bytes", "slfp_bn_train_fwd", "slfp_bn_train_bwd", "slfp_debug_bn_split")
NHWC, NCHW = _lib.LAYOUT_NHWC, _lib.LAYOUT_NCHW


def test_new_symbols_are_exported_and_declared():
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "slfp.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert hasattr(L, name)
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, header), name
    doc = header[header.index("csrc/bn_train.hip"):]
    for text in ("nets_cifar/mobilenetv1.py:30-45", "nets_imgnet/mobilenetv1.py:24-41", "No atomics", "d = x - k", "s2 = s2 + d * d",
                 "ty = 0, 1, ..., TY - 1", "Chan's formula in slab order", "delta * (n_b / n)", "rounded once",
                 "y = (((x - save_mean) - lo) * sc) + beta", "read from the forward's own output y",
                 "gx = a * ((g - mb) - (xh * mg))", "Contiguous NCHW is not built", "Expected more than 1 value per"):
        assert text in doc, text
    assert L.slfp_version() == 1   # new exports only


def test_supported_truth_table():
    ok = _lib.load().slfp_bn_train_supported
    for c in (1, 3, 4, 58, 64, 1024):
        assert ok(2, 5, 7, c, NHWC) == 1
        assert ok(2, 5, 7, c, NCHW) == 0          # contiguous NCHW is not built
        assert ok(1, 1, 1, c, NHWC) == 0          # M == 1: no variance
        assert ok(1, 1, 2, c, NHWC) == 1
        assert ok(0, 5, 7, c, NHWC) == 1          # an empty batch is no error
    for args in ((2, 5, 7, 64, 2), (2, 5, 7, 64, -1), (-1, 5, 7, 64, NHWC), (2, 0, 7, 64, NHWC), (2, 5, -3, 64, NHWC),
                 (2, 5, 7, 0, NHWC), (2, 5, 7, -4, NHWC), (2 ** 20, 2 ** 6, 2 ** 6, 4, NHWC)):
        assert ok(*args) == 0, args


def _fwd(x=16, gamma=16, beta=16, rm=None, rv=None, relu=0, y=32, sm=16, si=16, shape=(2, 5, 7, 64), layout=NHWC, ws=16,
         ws_bytes=1 << 30):
    return _lib.load().slfp_bn_train_fwd(x, gamma, beta, rm, rv, 0.1, 1e-5, relu, y, sm, si, *shape, layout, ws, ws_bytes, None)


def _bwd(x=16, y=32, gy=48, gamma=16, sm=16, si=16, relu=0, gx=64, gg=None, gb=None, shape=(2, 5, 7, 64), layout=NHWC, ws=16,
         ws_bytes=1 << 30):
    return _lib.load().slfp_bn_train_bwd(x, y, gy, gamma, sm, si, relu, gx, gg, gb, *shape, layout, ws, ws_bytes, None)


def test_refused_before_any_device_work():
    # the pointers are never dereferenced and no launch is made: every refusal comes first (this machine may have no GPU)
    L = _lib.load()
    need = L.slfp_bn_train_workspace_bytes(2, 5, 7, 64)
    for call, names in ((_fwd, ("x", "gamma", "beta", "y", "sm", "si")), (_bwd, ("x", "y", "gy", "gamma", "sm", "si", "gx"))):
        for name in names:
            assert call(**{name: None}) == _lib.ERR_BAD_ARG, name
            assert "null pointer" in _lib.last_error()
        assert call(layout=NCHW) == _lib.ERR_UNSUPPORTED
        assert "slfp_bn_train_supported" in _lib.last_error()
        assert call(shape=(1, 1, 1, 64)) == _lib.ERR_UNSUPPORTED            # M == 1
        assert call(layout=7) == _lib.ERR_BAD_ARG
        assert call(relu=2) == _lib.ERR_BAD_ARG
        assert call(shape=(2, 0, 7, 64)) == _lib.ERR_SHAPE
        assert call(shape=(-1, 5, 7, 64)) == _lib.ERR_SHAPE
        assert call(x=24) == _lib.ERR_ALIGNMENT and "16-byte" in _lib.last_error()   # the vector path
        assert call(ws_bytes=need - 1) == _lib.ERR_BAD_ARG                   # the code of the conv workspace
        assert "workspace" in _lib.last_error()
        assert call(ws=None) == _lib.ERR_BAD_ARG
        assert call(ws=8) == _lib.ERR_BAD_ARG
        assert call(shape=(0, 5, 7, 64), ws=None, ws_bytes=0) == _lib.OK     # n == 0: nothing to do
    assert _fwd(y=24) == _lib.ERR_ALIGNMENT and _bwd(gy=24) == _lib.ERR_ALIGNMENT and _bwd(gx=72) == _lib.ERR_ALIGNMENT
    assert _fwd(x=18, shape=(2, 5, 7, 58), ws_bytes=0) == _lib.ERR_ALIGNMENT and "4-byte" in _lib.last_error()
    assert _fwd(x=20, y=36, shape=(2, 5, 7, 58), ws_bytes=0) == _lib.ERR_BAD_ARG     # 4-byte alignment passes; the workspace is short
    assert _fwd(y=16) == _lib.ERR_BAD_ARG and "alias" in _lib.last_error()
    assert _bwd(gx=16) == _lib.ERR_BAD_ARG and _bwd(gx=32) == _lib.ERR_BAD_ARG
    assert _fwd(rm=16) == _lib.ERR_BAD_ARG                                   # running_mean without running_var


def test_split_rule():
    L = _lib.load()
    seen = {}
    for c in (1, 3, 4, 6, 32, 58, 64, 116, 256, 512, 1000, 1024, 4096):
        for m in (2, 3, 7, 64, 127, 128, 129, 392, 1000, 6272, 25088, 100352, 401408, 1605632, 2 ** 31 - 1):
            r, s = B.split(m, c)
            assert (r, s) == B.split(m, c)                       # a pure function of (M, C)
            assert 1 <= s <= 1024 and r >= 1
            assert r * (s - 1) < m <= r * s, (m, c, r, s)
            seen[(m, c)] = (r, s)
    assert seen[(1605632, 64)][1] > 256                          # a few workgroups per CU on the large layers
    assert seen[(2, 64)] == (2, 1)
    r, s = ctypes.c_int64(), ctypes.c_int64()
    assert L.slfp_debug_bn_split(0, 64, ctypes.byref(r), ctypes.byref(s)) == _lib.ERR_SHAPE
    assert L.slfp_debug_bn_split(64, 0, ctypes.byref(r), ctypes.byref(s)) == _lib.ERR_SHAPE
    assert L.slfp_debug_bn_split(64, 64, None, ctypes.byref(s)) == _lib.ERR_BAD_ARG
    # the workspace holds one 16-byte record per (slab, channel) and three floats per channel, rounded up to 256 bytes
    for (n, h, w, c) in B.shapes() + [(128, 112, 112, 64), (128, 7, 7, 1024)]:
        rr, ss = B.split(n * h * w, c)
        want = ss * c * 16 + 3 * c * 4
        assert L.slfp_bn_train_workspace_bytes(n, h, w, c) == (want + 255) // 256 * 256
    assert L.slfp_bn_train_workspace_bytes(0, 5, 7, 64) == 0
    for shape in (B.ragged(32), B.ragged(6)):
        n, h, w, c = shape
        rr, ss = B.split(n * h * w, c)
        assert ss >= 3 and (n * h * w) % rr, shape


@pytest.mark.parametrize("case", B.cases(), ids=B.case_id)
def test_inputs_hold_the_statistics_bars_on_the_cpu(case):
    """Before the GPU test's inputs are fixed: ATen's float32 CPU batch_norm and a float32 NumPy model of the kernel's order of
    summation both stay inside the mean and variance bars against the float64 reference, the offset case (mu = 1000 sigma)
    included; a plain E[x^2] - E[x]^2 in float32 misses the variance bar there by orders of magnitude."""
    shape, offset = case
    d = B.inputs(shape, offset)
    x = d["x"]
    mean64, var64, _ = B.forward64(x, d["gamma"], d["beta"], False)
    rm, rv = torch.zeros(shape[3]), torch.zeros(shape[3])
    F.batch_norm(x, rm, rv, None, None, True, 1.0, B.EPS)      # momentum 1: the running statistics are the batch's
    m = x.numel() // shape[3]
    assert B.mean_bar_ok(rm.numpy(), mean64, x)
    assert B.var_bar_ok(rv.double().numpy() * (m - 1) / m, var64, TOL_EXACT)
    km, kv = B.kernel_order_stats(x)
    assert B.mean_bar_ok(km, mean64, x)
    assert B.var_bar_ok(kv, var64, TOL_EXACT)
    if offset:
        xr = x.permute(0, 2, 3, 1).reshape(-1, shape[3])
        naive = (xr * xr).mean(dim=0) - xr.mean(dim=0) ** 2    # float32
        assert np.median(np.abs(naive.double().numpy() - var64) / var64) > 100 * TOL_EXACT


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("case", B.cases(), ids=B.case_id)
def test_kernel_order_model_holds_the_float64_bars_on_the_cpu(case, relu):
    """The float32 NumPy model of the apply and backward orders (the GPU test compares the kernels with it bit for bit), fed its
    own statistics and f32(1 / sqrt(var + eps)): y, gx, ggamma and gbeta hold the bars of test_gpu_bn_train.py against float64."""
    shape, offset = case
    d = B.inputs(shape, offset)
    x, gamma, beta = d["x"], d["gamma"], d["beta"]
    km, kv = B.kernel_order_stats(x)
    sm, si = km.astype(np.float32), (1.0 / np.sqrt(kv + B.EPS)).astype(np.float32)
    y = B.kernel_order_forward(x, gamma, beta, sm, si, relu)
    y64 = B.forward64(x, gamma, beta, relu)[2]
    centred = B.forward64(x, gamma, beta, False)[2] - beta.double().numpy() if offset else None
    assert _bars_ok(y, y64, centred)
    for key in ("gy", "gy_sparse"):
        gx, gg, gb = B.kernel_order_backward(x, d[key], y, gamma, sm, si, relu)
        g = B.rows(d[key])
        if relu:
            g = g * (y > 0)
        gx64, gg64, gb64, agg, agb = B.backward64(x, g, gamma)
        assert _sum_bars_ok("ggamma", gg, gg64, agg) and _sum_bars_ok("gbeta", gb, gb64, agb), key
        assert _bars_ok(gx, gx64), key


class _Block(nn.Module):
    """A hand-wired block: its BatchNorm2d sits in a named slot and its ReLU module is shared (ResNet-50's bn1..3)."""

    def __init__(self):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(8, 8, 1), nn.BatchNorm2d(8)
        self.conv2, self.bn2 = nn.Conv2d(8, 8, 1), nn.BatchNorm2d(8)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        return self.relu(self.bn2(self.conv2(out)) + x)


def _model():
    torch.manual_seed(3)
    seq = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.BatchNorm2d(8), nn.ReLU(inplace=True),
                        nn.Conv2d(8, 8, 3, padding=1), nn.BatchNorm2d(8), layerout_quantize_func(32), nn.ReLU())
    return nn.Sequential(seq, _Block())


def _step(model, x):
    model.zero_grad(set_to_none=True)
    y = model(x)
    if model.training:
        y.square().mean().backward()
    return y.detach().clone(), [p.grad.clone() for p in model.parameters() if p.grad is not None]


def test_swap_fallback_and_restore_on_a_cpu_model():
    model, ref = _model(), None
    ref = copy.deepcopy(model)
    before = dict(model.named_modules())
    ids = [id(p) for p in model.parameters()]
    keys = list(model.state_dict().keys())
    opt = torch.optim.SGD(model.parameters(), lr=0.1)

    assert fusion.use_device_bn_train(model) == 4
    seq, blk = model[0], model[1]
    assert isinstance(seq[1], fusion.TrainBatchNorm2d) and seq[1]._relu and isinstance(seq[2], fusion.FoldedReLU)
    assert isinstance(seq[4], fusion.TrainBatchNorm2d) and not seq[4]._relu and type(seq[6]) is nn.ReLU   # the quantizer sits between
    assert isinstance(blk.bn1, fusion.TrainBatchNorm2d) and not blk.bn1._relu and type(blk.relu) is nn.ReLU
    assert not any(isinstance(m, nn.BatchNorm2d) for m in model.modules())
    assert "_bn" not in seq[1]._modules and seq[1]._bn is before["0.1"]
    assert fusion.use_device_bn_train(model) == 0                       # nothing left to swap

    assert list(model.state_dict().keys()) == keys
    assert [id(p) for p in model.parameters()] == ids
    assert all(a is b for a, b in zip(opt.param_groups[0]["params"], model.parameters()))
    for k, v in ref.state_dict().items():
        assert torch.equal(model.state_dict()[k], v), k
    assert model.state_dict()._metadata["0.1"]["version"] == ref.state_dict()._metadata["0.1"]["version"]

    x = torch.randn(4, 3, 6, 5)
    for training in (True, True, False):                                # two training steps, then eval
        model.train(training)
        ref.train(training)
        y, g = _step(model, x)
        y0, g0 = _step(ref, x)
        assert torch.equal(y, y0)
        assert len(g) == len(g0) == (len(ids) if training else 0) and all(torch.equal(a, b) for a, b in zip(g, g0))
        for k, v in ref.state_dict().items():                           # running statistics and num_batches_tracked
            assert torch.equal(model.state_dict()[k], v), k
        assert seq[1]._last_kernel == "aten"
    assert int(seq[1].num_batches_tracked) == 2

    model.eval()
    assert fusion.fuse_bn_relu(model) == 0                              # the eval passes leave the wrappers alone
    assert fusion.restore_avgpool(model) == 0 and isinstance(seq[2], fusion.FoldedReLU)   # ... and so does the pool's undo
    model.double()                                                      # buffers are replaced by a cast: restore re-points them
    assert fusion.restore_bn_train(model) == 4
    assert dict(model.named_modules()) == before                        # the very same module objects
    assert seq[1].running_mean.dtype == torch.float64 and seq[1].running_mean is model.state_dict(keep_vars=True)["0.1.running_mean"]
    assert not seq[1].training
    assert fusion.restore_bn_train(model) == 0
    model.float()
    assert torch.allclose(model(x), ref(x), rtol=1e-6, atol=1e-6)


def test_wrapper_refuses_what_the_stock_module_refuses():
    wrap = fusion.TrainBatchNorm2d(nn.BatchNorm2d(4))
    with pytest.raises(ValueError, match="expected 4D input"):
        wrap(torch.zeros(2, 4, 3))
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        wrap.train()(torch.zeros(1, 4, 1, 1))
    assert fusion.use_device_bn_train(nn.Sequential(nn.BatchNorm2d(4, affine=False), nn.BatchNorm2d(4, momentum=None))) == 0
    plain = nn.Sequential(nn.BatchNorm2d(4, track_running_stats=False), nn.ReLU())
    x = torch.randn(3, 4, 2, 2)
    want = plain(x)
    assert fusion.use_device_bn_train(plain) == 1 and plain[0]._relu     # swapped; without buffers it stays on the stock path
    assert torch.equal(plain(x), want) and plain[0]._last_kernel == "aten" and list(plain.state_dict()) == ["0.weight", "0.bias"]
