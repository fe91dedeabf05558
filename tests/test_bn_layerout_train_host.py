"""CPU: the host side of training-mode BatchNorm2d -> layer-output quantizer -> activation: the exports, the
refusals of slfp_bn_lut_train_fwd / slfp_bn_lut_train_bwd (all before any device work), batchnorm.layerout_act_tables, and
fusion.TrainBatchNormLayerout2d / use_device_bn_layerout_train / restore_bn_layerout_train on a model without a device.  The
package's layerout_quantize_func has no CPU path, so the test model's quantizers compute with the oracle's CPU restatement
(straight-through backward, as the package's)."""
import copy
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from cnns_slfp_quantization_amd import _lib, activation_func as af, batchnorm, fusion
from cnns_slfp_quantization_amd.sfp_quant import layerout_quantize_func

NEW = ("slfp_bn_lut_train_fwd", "slfp_bn_lut_train_bwd")
NHWC, NCHW = _lib.LAYOUT_NHWC, _lib.LAYOUT_NCHW


def test_new_symbols_are_exported_bound_and_declared():
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "slfp.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert hasattr(L, name)
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert re.search(r"#define\s+SLFP_LAYEROUT_TABLE_FLOATS\s+SLFP_LAYEROUT_LUT_BYTES", header)
    assert _lib.LAYEROUT_TABLE_FLOATS == _lib.LAYEROUT_LUT_BYTES == 4928
    assert L.slfp_layerout_lut_classes() == 4927
    doc = header[header.index("the LUT forms"):]
    for text in ("save_lo[c] = lo = f32(mean - save_mean)", "y = act_table[layerout_class(q)]", "g = gy * dact_table[class]",
                 "a saved y is never read", "straight-through", "ggamma and gbeta may be NULL", "No atomics", "cold branch"):
        assert text in doc, text
    assert L.slfp_version() == 1   # new exports only


def _fwd(x=16, gamma=16, beta=16, rm=None, rv=None, tab=128, y=32, sm=16, si=16, lo=16, shape=(2, 5, 7, 64), layout=NHWC, ws=16,
         ws_bytes=1 << 30):
    return _lib.load().slfp_bn_lut_train_fwd(x, gamma, beta, rm, rv, 0.1, 1e-5, tab, y, sm, si, lo, *shape, layout, ws, ws_bytes, None)


def _bwd(x=16, gy=48, gamma=16, beta=16, sm=16, si=16, lo=16, tab=128, gx=64, gg=None, gb=None, shape=(2, 5, 7, 64), layout=NHWC,
         ws=16, ws_bytes=1 << 30):
    return _lib.load().slfp_bn_lut_train_bwd(x, gy, gamma, beta, sm, si, lo, tab, gx, gg, gb, *shape, layout, ws, ws_bytes, None)


def test_refused_before_any_device_work():
    # the pointers are never dereferenced and no launch is made: every refusal comes first (this machine may have no GPU)
    need = _lib.load().slfp_bn_train_workspace_bytes(2, 5, 7, 64)
    for call, names in ((_fwd, ("x", "gamma", "beta", "y", "sm", "si")), (_bwd, ("x", "gy", "gamma", "beta", "sm", "si", "gx"))):
        for name in names + ("tab", "lo"):
            assert call(**{name: None}) == _lib.ERR_BAD_ARG, name
            assert "null pointer" in _lib.last_error()
        for tab in (132, 136, 129):
            assert call(tab=tab) == _lib.ERR_ALIGNMENT and "table" in _lib.last_error()
        assert call(tab=132, shape=(2, 5, 7, 58)) == _lib.ERR_ALIGNMENT      # 16 bytes whatever c is
        assert call(lo=24) == _lib.ERR_ALIGNMENT
        assert call(layout=NCHW) == _lib.ERR_UNSUPPORTED
        assert "slfp_bn_train_supported" in _lib.last_error()
        assert call(shape=(1, 1, 1, 64)) == _lib.ERR_UNSUPPORTED             # M == 1
        assert call(layout=7) == _lib.ERR_BAD_ARG
        assert call(shape=(2, 0, 7, 64)) == _lib.ERR_SHAPE
        assert call(x=24) == _lib.ERR_ALIGNMENT
        assert call(ws_bytes=need - 1) == _lib.ERR_BAD_ARG and "workspace" in _lib.last_error()
        assert call(ws=None) == _lib.ERR_BAD_ARG
        assert call(shape=(0, 5, 7, 64), ws=None, ws_bytes=0) == _lib.OK     # n == 0: nothing to do
        # the order of slfp_bn_train_fwd / _bwd: null pointers, the layout, the geometry, what is unsupported, alignment, workspace
        assert call(tab=None, layout=NCHW, ws_bytes=0) == _lib.ERR_BAD_ARG
        assert call(layout=NCHW, tab=132, ws_bytes=0) == _lib.ERR_UNSUPPORTED
        assert call(tab=132, ws_bytes=0) == _lib.ERR_ALIGNMENT
    assert _fwd(y=16) == _lib.ERR_BAD_ARG and "alias" in _lib.last_error()
    assert _bwd(gx=16) == _lib.ERR_BAD_ARG and "alias" in _lib.last_error()
    assert _fwd(rm=16) == _lib.ERR_BAD_ARG                                    # running_mean without running_var


def _values():
    n = _lib.LAYEROUT_TABLE_FLOATS
    vals = np.zeros(n, dtype=np.float32)
    _lib.check(_lib.load().slfp_layerout_lut_values(vals.ctypes.data, n))
    return torch.from_numpy(vals)


def _phi(v):
    return torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)


def _Phi(v):
    return 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0)))


def _sig(v):
    return 1.0 / (1.0 + torch.exp(-v))


CLOSED = {   # the float64 derivative at v
    "relu": (nn.ReLU, lambda v: (v > 0).double()),
    "relu_inplace": (lambda: nn.ReLU(inplace=True), lambda v: (v > 0).double()),
    "gelu": (nn.GELU, lambda v: _Phi(v) + v * _phi(v)),
    "swish": (af.Swish, lambda v: _sig(v) * (1.0 + v * (1.0 - _sig(v)))),
    "silu": (nn.SiLU, lambda v: _sig(v) * (1.0 + v * (1.0 - _sig(v)))),
}


@pytest.mark.parametrize("name", list(CLOSED))
def test_tables_are_the_modules_and_their_derivative(name):
    make, d64 = CLOSED[name]
    act = make()
    v = _values()
    classes = _lib.load().slfp_layerout_lut_classes()
    F, D = batchnorm.layerout_act_tables([act], torch.device("cpu"))
    assert F.dtype == D.dtype == torch.float32 and F.shape == D.shape == (_lib.LAYEROUT_TABLE_FLOATS,)
    assert not F.requires_grad and not D.requires_grad
    want = make()(v.clone())
    assert torch.equal(F[1:classes].view(torch.int32), want[1:classes].view(torch.int32))   # bit for bit, -0.0 included
    assert bool(torch.isnan(F[0])) and bool(torch.isnan(want[0]))
    assert bool((F[classes:] == 0).all()) and bool((D[classes:] == 0).all())
    ref = d64(v[1:classes].double())
    got = D[1:classes].double()
    assert bool(torch.isfinite(got).all())
    # max|D - ref| <= 1e-6 * max|ref| over the finite classes: the project's max-norm bar (_bars.py), not a pointwise relative one.
    # The modules compute in float32: Phi = 0.5 (1 + erf) and the sigmoid carry an ABSOLUTE error of about 2^-24 (GELU'(-6.25) =
    # -8e-9 comes out as 0, SiLU'(-92) = -1e-38 underflows), and a bar relative to a derivative that passes through zero cannot
    # be met by any float32 evaluation.  max|ref| is 1 (ReLU), 1.13 (GELU) and 1.10 (Swish / SiLU).
    err = float((got - ref).abs().max() / ref.abs().max())
    print(name, "max|D - ref| / max|ref|", err)
    assert err <= 1e-6


def test_tables_refuse_stl_and_unknown_modules():
    with pytest.raises(TypeError):
        batchnorm.layerout_act_tables([af.STL()], torch.device("cpu"))
    with pytest.raises(TypeError):
        batchnorm.layerout_act_tables([nn.Tanh()], torch.device("cpu"))

    class Sub(nn.ReLU):   # by exact type
        pass
    with pytest.raises(TypeError):
        batchnorm.layerout_act_tables([Sub()], torch.device("cpu"))
    with pytest.raises(TypeError):
        fusion.TrainBatchNormLayerout2d(nn.BatchNorm2d(4), layerout_quantize_func(8), [af.STL()])


class _CpuLayerout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        from oracle import slfp_oracle
        return torch.from_numpy(slfp_oracle.layerout(x.detach().contiguous().numpy()).reshape(x.shape))

    @staticmethod
    def backward(ctx, g):
        return g.clone()


def _layerout(q_bit):
    m = layerout_quantize_func(q_bit)
    if q_bit != 32:
        m.quantize = _CpuLayerout.apply
    return m


class _Block(nn.Module):
    """A hand-wired block: the pass matches inside nn.Sequential only."""

    def __init__(self):
        super().__init__()
        self.bn, self.lo, self.act = nn.BatchNorm2d(8), _layerout(8), nn.GELU()

    def forward(self, x):
        return self.act(self.lo(self.bn(x)))


def _model():
    torch.manual_seed(5)
    seq = nn.Sequential(
        nn.Conv2d(3, 8, 3, padding=1), nn.BatchNorm2d(8), _layerout(8), af.Swish(),            # 1..3: taken
        nn.Conv2d(8, 8, 3, padding=1), nn.BatchNorm2d(8), _layerout(7), nn.GELU(),             # 5..7: taken
        nn.Conv2d(8, 8, 3, padding=1), nn.BatchNorm2d(8), _layerout(8), nn.ReLU(inplace=True),  # 9..11: taken
        nn.Conv2d(8, 8, 1), nn.BatchNorm2d(8), _layerout(32), nn.ReLU(),                       # 13..15: q_bit 32, no table
        nn.Conv2d(8, 8, 1), nn.BatchNorm2d(8), _layerout(8), af.STL(),                         # 17..19: STL
        nn.Conv2d(8, 8, 1), nn.BatchNorm2d(8), nn.ReLU())                                      # 21..22: plain BN + ReLU
    return nn.Sequential(seq, _Block())


def _step(model, x):
    model.zero_grad(set_to_none=True)
    y = model(x)
    if model.training:
        y.square().mean().backward()
    return y.detach().clone(), [p.grad.clone() for p in model.parameters() if p.grad is not None]


TAKEN = (1, 5, 9)


def _check_swapped(seq, before):
    for i in TAKEN:
        assert isinstance(seq[i], fusion.TrainBatchNormLayerout2d) and not isinstance(seq[i], nn.BatchNorm2d)
        assert isinstance(seq[i + 1], fusion.FoldedTail) and seq[i + 1].mod is before[f"0.{i + 1}"]
        assert isinstance(seq[i + 2], fusion.FoldedTail) and seq[i + 2].mod is before[f"0.{i + 2}"]
        assert seq[i]._bn is before[f"0.{i}"] and seq[i]._layerout is before[f"0.{i + 1}"] and seq[i]._acts == (before[f"0.{i + 2}"],)
        assert not seq[i]._modules and not seq[i + 1]._modules


def test_swap_fallback_and_restore_on_a_cpu_model():
    model = _model()
    ref = copy.deepcopy(model)
    before = dict(model.named_modules())
    ids = [id(p) for p in model.parameters()]
    keys = list(model.state_dict().keys())
    opt = torch.optim.SGD(model.parameters(), lr=0.1)

    assert fusion.use_device_bn_layerout_train(model) == 3
    seq, blk = model[0], model[1]
    _check_swapped(seq, before)
    for i in (13, 14, 15, 17, 18, 19, 21, 22):
        assert seq[i] is before[f"0.{i}"], i
    assert blk.bn is before["1.bn"] and blk.lo is before["1.lo"] and blk.act is before["1.act"]
    assert fusion.use_device_bn_layerout_train(model) == 0                # nothing left to take

    assert list(model.state_dict().keys()) == keys
    assert [id(p) for p in model.parameters()] == ids
    assert all(a is b for a, b in zip(opt.param_groups[0]["params"], model.parameters()))
    for k, v in ref.state_dict().items():
        assert torch.equal(model.state_dict()[k], v), k
    assert model.state_dict()._metadata["0.1"]["version"] == ref.state_dict()._metadata["0.1"]["version"]

    x = torch.randn(4, 3, 6, 5)
    for training in (True, True, False):                                  # two training steps, then eval
        model.train(training)
        ref.train(training)
        y, g = _step(model, x)
        y0, g0 = _step(ref, x)
        assert torch.equal(y, y0)
        assert len(g) == len(g0) == (len(ids) if training else 0) and all(torch.equal(a, b) for a, b in zip(g, g0))
        for k, v in ref.state_dict().items():                             # running statistics and num_batches_tracked
            assert torch.equal(model.state_dict()[k], v), k
        assert [seq[i]._last_kernel for i in TAKEN] == ["aten"] * 3
    assert int(seq[1].num_batches_tracked) == 2

    # the other undo passes leave the wrappers and the placeholders alone
    assert fusion.restore_bn_train(model) == 0 and fusion.restore_avgpool(model) == 0
    _check_swapped(seq, before)
    model.double()                                                        # buffers are replaced by a cast: restore re-points them
    assert fusion.restore_bn_layerout_train(model) == 3
    assert dict(model.named_modules()) == before                          # the very same module objects
    assert seq[1].running_mean.dtype == torch.float64 and seq[1].running_mean is model.state_dict(keep_vars=True)["0.1.running_mean"]
    assert not seq[1].training and not seq[3].training
    assert fusion.restore_bn_layerout_train(model) == 0


@pytest.mark.parametrize("order", ["bn_train_first", "layerout_first"])
def test_either_order_with_use_device_bn_train(order):
    model = _model()
    before = dict(model.named_modules())
    if order == "bn_train_first":
        assert fusion.use_device_bn_train(model) == 7
        assert isinstance(model[0][1], fusion.TrainBatchNorm2d) and not model[0][1]._relu
        assert fusion.use_device_bn_layerout_train(model, min_elements=0) == 3
    else:
        assert fusion.use_device_bn_layerout_train(model, min_elements=0) == 3
        assert fusion.use_device_bn_train(model) == 4
    seq = model[0]
    _check_swapped(seq, before)
    assert all(seq[i].min_elements == 0 for i in TAKEN)
    for i in (13, 17):
        assert isinstance(seq[i], fusion.TrainBatchNorm2d) and not seq[i]._relu and seq[i]._bn is before[f"0.{i}"]
    assert isinstance(seq[21], fusion.TrainBatchNorm2d) and seq[21]._relu and isinstance(seq[22], fusion.FoldedReLU)
    assert isinstance(model[1].bn, fusion.TrainBatchNorm2d)
    # either undo first
    if order == "bn_train_first":
        assert fusion.restore_bn_train(model) == 4 and fusion.restore_bn_layerout_train(model) == 3
    else:
        assert fusion.restore_bn_layerout_train(model) == 3 and fusion.restore_bn_train(model) == 4
    assert dict(model.named_modules()) == before


def test_shared_modules_are_skipped():
    act = nn.GELU()
    m = nn.Sequential(nn.BatchNorm2d(4), _layerout(8), act, nn.BatchNorm2d(4), _layerout(8), act)
    assert fusion.use_device_bn_layerout_train(m) == 0
    with pytest.raises(ValueError, match="expected 4D input"):
        fusion.TrainBatchNormLayerout2d(nn.BatchNorm2d(4), _layerout(8), [nn.GELU()])(torch.zeros(2, 4, 3))


def test_a_cast_between_the_two_passes_keeps_the_current_parameters_and_buffers():
    """use_device_bn_train, then a cast (Module._apply replaces the buffer objects on the wrapper alone: the stock module sits
    outside _modules), then this pass: the new module must register the wrapper's CURRENT tensors, not the stock module's old ones."""
    model = _model()
    before = dict(model.named_modules())
    assert fusion.use_device_bn_train(model) == 7
    model.train()
    model(torch.randn(4, 3, 6, 5))                                        # the running statistics move off their initial values
    model.double()
    seq = model[0]
    current = {i: {**seq[i]._parameters, **seq[i]._buffers} for i in TAKEN}
    assert all(before[f"0.{i}"].running_mean.dtype == torch.float32 for i in TAKEN)   # the stock modules are stale now
    want = {k: v.clone() for k, v in model.state_dict().items()}
    assert fusion.use_device_bn_layerout_train(model) == 3
    sd = model.state_dict(keep_vars=True)
    for i in TAKEN:
        wrap = seq[i]
        assert isinstance(wrap, fusion.TrainBatchNormLayerout2d) and wrap._bn is before[f"0.{i}"]
        for key, t in current[i].items():
            assert getattr(wrap, key) is t and sd[f"0.{i}.{key}"] is t and getattr(wrap._bn, key) is t, (i, key)
        assert wrap.weight.dtype == wrap.running_mean.dtype == wrap.running_var.dtype == torch.float64
        assert int(wrap.num_batches_tracked) == 1 and not torch.equal(wrap.running_mean, torch.zeros(8, dtype=torch.float64))
    assert list(sd.keys()) == list(want.keys())
    for k, v in want.items():
        assert torch.equal(sd[k], v), k
    model.float()                                                         # ... and a cast after this pass, before its undo
    assert fusion.restore_bn_layerout_train(model) == 3 and fusion.restore_bn_train(model) == 4
    assert dict(model.named_modules()) == before
    sd = model.state_dict(keep_vars=True)
    for i in TAKEN:
        assert seq[i].running_mean is sd[f"0.{i}.running_mean"] and seq[i].running_mean.dtype == torch.float32
        assert torch.equal(seq[i].running_mean.double(), want[f"0.{i}.running_mean"].float().double())

