"""MI355X: the training-mode passes composed.  restore_avgpool between link_codes_train and a training step
changes nothing of the step; and one training forward of a fully linked Bottleneck stack asks for no more plans and makes no more
library queries than it did before the reader check became one function."""
import contextlib
import copy

import pytest
import torch
import torch.nn as nn

import _bottleneck_q_blocks as Q
from cnns_slfp_quantization_amd import _lib, fusion
from cnns_slfp_quantization_amd import conv2d_func as cf

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@contextlib.contextmanager
def _backward(mode):
    prev, det = cf.options.backward, torch.backends.cudnn.deterministic
    cf.options.backward = mode
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        cf.options.backward, torch.backends.cudnn.deterministic = prev, det


def _image():
    return torch.randn(2, 16, 8, 8, generator=torch.Generator().manual_seed(9)).to(DEV).contiguous(memory_format=torch.channels_last)


# ---- the defect, end to end --------------------------------------------------------------------------------------------------------
def _pair_model():
    """[Conv2d_Q, BN, ReLU, Conv2d_Q, BN, ReLU, AdaptiveAvgPool2d(1)] at 16 channels, out-of-place ReLUs: one hand-over on codes."""
    def conv():
        return cf.conv2d_Q(8, 0.06, 0.17)(16, 16, 1, bias=False)
    torch.manual_seed(6)
    m = nn.Sequential(conv(), nn.BatchNorm2d(16), nn.ReLU(), conv(), nn.BatchNorm2d(16), nn.ReLU(), nn.AdaptiveAvgPool2d(1))
    return m.to(DEV).to(memory_format=torch.channels_last).train()


def _step(m, x):
    m.zero_grad(set_to_none=True)
    xi = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
    out = m(xi)
    (out.square().mean() + out.sum() * 0.1).backward()
    return [out.detach().clone(), xi.grad] + [p.grad for p in m.parameters()] + [b.clone() for b in m.buffers()]


def test_restore_avgpool_between_link_and_step_changes_nothing():
    model = _pair_model()
    ref = copy.deepcopy(model)
    for m in (model, ref):
        assert fusion.link_codes_train(m, min_elements=0) == 1
    assert fusion.restore_avgpool(model) == 0
    assert isinstance(model[2], fusion.FoldedReLU) and isinstance(ref[2], fusion.FoldedReLU)
    x = _image()
    with _backward("hip"):
        got, want = _step(model, x), _step(ref, x)
    for m in (model, ref):
        assert m[1]._last_kernel == "bn_codes_train+relu" and "+codes_in" in m[3]._last_kernel
    assert len(got) == len(want) and all(g is not None and torch.equal(g, w) for g, w in zip(got, want))


# ---- calls per training forward ----------------------------------------------------------------------------------------------------
# Counted with count_calls() below on the commit before the reader check was consolidated (the stack of width 16, 2 x 16 x 8 x 8,
# the three Bottleneck passes at min_elements=0, options.backward = "hip_all"; one training forward with autograd recording).
PLANS_BEFORE = 19
QUERIES_BEFORE = 41


def count_calls(monkeypatch):
    """(calls of conv2d_func._plan, calls of the library's slfp_*_supported queries) during one training forward."""
    model = Q.stack(mid=16).to(DEV).to(memory_format=torch.channels_last)
    x = _image()
    assert fusion.use_device_bn_train(model, min_elements=0) > 0
    assert fusion.use_device_bottleneck_train(model, x, min_elements=0) == Q.GENUINE
    model.train()
    assert fusion.link_bottleneck_codes_train(model, x, min_elements=0) == (6, 1)
    counts = {"plan": 0, "query": 0}
    L = _lib.load()

    def counted(fn, key):
        def call(*args, **kw):
            counts[key] += 1
            return fn(*args, **kw)
        return call

    with _backward("hip_all"):
        model(x.clone().requires_grad_(True))   # plans are cached per module: the counted forward is a steady-state one
        monkeypatch.setattr(cf, "_plan", counted(cf._plan, "plan"))
        for name in _lib.SYMBOLS:
            if name.startswith("slfp_") and "_supported" in name:
                monkeypatch.setattr(L, name, counted(getattr(L, name), "query"))
        model(x.clone().requires_grad_(True))
    wraps = [w for w in model.modules() if isinstance(w, fusion.TrainBatchNormCodes2d)]
    assert len(wraps) == 6 and all(w._last_kernel == "bn_codes_train+relu" for w in wraps)
    assert list(model)[0].bn3._last_kernel == "bn_res_codes_train+relu"
    return counts["plan"], counts["query"]


def test_a_training_forward_asks_for_no_more_plans_or_queries_than_before(monkeypatch):
    plans, queries = count_calls(monkeypatch)
    print(f"plans {plans} (before: {PLANS_BEFORE}), queries {queries} (before: {QUERIES_BEFORE})")
    assert plans <= PLANS_BEFORE and queries <= QUERIES_BEFORE
