"""CPU: the host side of training-mode BatchNorm2d -> residual add -> ReLU: the exports, the refusals of
slfp_bn_res_train_fwd / slfp_bn_res_train_bwd (all before any device work), and fusion.use_device_bottleneck_train /
restore_bottleneck_train on a model without a device, where training mode takes TrainBatchNorm2d's ATen fallback."""
import copy
import os
import re

import pytest
import torch
import torch.nn as nn

import _bn_res_blocks as R
from cnns_slfp_quantization_amd import _lib, batchnorm, fusion

NEW = ("slfp_bn_res_train_fwd", "slfp_bn_res_train_bwd")
NHWC, NCHW = _lib.LAYOUT_NHWC, _lib.LAYOUT_NCHW


def test_new_symbols_are_exported_bound_and_declared():
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "slfp.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert hasattr(L, name)
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    doc = header[header.index("the residual forms"):]
    for text in ("z = t + res", "y = z < 0 ? 0 : z", "gres = g", "gres == NULL", "ggamma and gbeta may be NULL", "No atomics",
                 "bit-identical to slfp_bn_train_fwd(relu = 0)", "bit-identical to slfp_bn_train_bwd(relu)"):
        assert text in doc, text
    assert L.slfp_version() == 1   # new exports only
    assert batchnorm.RES_MIN_ELEMENTS >= 0 and hasattr(batchnorm, "hip_bn_res_train")


def _fwd(x=16, res=80, gamma=16, beta=16, rm=None, rv=None, relu=1, y=32, sm=16, si=16, shape=(2, 5, 7, 64), layout=NHWC, ws=16,
         ws_bytes=1 << 30):
    return _lib.load().slfp_bn_res_train_fwd(x, res, gamma, beta, rm, rv, 0.1, 1e-5, relu, y, sm, si, *shape, layout, ws, ws_bytes, None)


def _bwd(x=16, y=32, gy=48, gamma=16, sm=16, si=16, relu=1, gx=64, gres=96, gg=None, gb=None, shape=(2, 5, 7, 64), layout=NHWC,
         ws=16, ws_bytes=1 << 30):
    return _lib.load().slfp_bn_res_train_bwd(x, y, gy, gamma, sm, si, relu, gx, gres, gg, gb, *shape, layout, ws, ws_bytes, None)


def test_refused_before_any_device_work():
    # the pointers are never dereferenced and no launch is made: every refusal comes first (this machine may have no GPU)
    need = _lib.load().slfp_bn_train_workspace_bytes(2, 5, 7, 64)
    assert need > 0
    for call, names in ((_fwd, ("x", "res", "gamma", "beta", "y", "sm", "si")), (_bwd, ("x", "y", "gy", "gamma", "sm", "si", "gx"))):
        for name in names:
            assert call(**{name: None}) == _lib.ERR_BAD_ARG, name
            assert "null pointer" in _lib.last_error()
        assert call(layout=NCHW) == _lib.ERR_UNSUPPORTED
        assert "slfp_bn_train_supported" in _lib.last_error()
        assert call(relu=2) == _lib.ERR_BAD_ARG and "relu" in _lib.last_error()
        assert call(shape=(1, 1, 1, 64)) == _lib.ERR_UNSUPPORTED             # M == 1
        assert call(layout=7) == _lib.ERR_BAD_ARG
        assert call(shape=(2, 0, 7, 64)) == _lib.ERR_SHAPE
        assert call(x=24) == _lib.ERR_ALIGNMENT
        assert call(ws_bytes=need - 1) == _lib.ERR_BAD_ARG and "workspace" in _lib.last_error()
        assert call(ws=None) == _lib.ERR_BAD_ARG
        assert call(shape=(0, 5, 7, 64), ws=None, ws_bytes=0) == _lib.OK     # n == 0: nothing to do
        # the order of slfp_bn_train_fwd / _bwd: null pointers, the layout, relu, the geometry, what is unsupported, alignment, workspace
        assert call(x=None, layout=NCHW, relu=2, ws_bytes=0) == _lib.ERR_BAD_ARG and "null pointer" in _lib.last_error()
        assert call(layout=7, relu=2, shape=(2, 0, 7, 64)) == _lib.ERR_BAD_ARG and "layout" in _lib.last_error()
        assert call(relu=2, shape=(2, 0, 7, 64)) == _lib.ERR_BAD_ARG and "relu" in _lib.last_error()
        assert call(layout=NCHW, x=24, ws_bytes=0) == _lib.ERR_UNSUPPORTED
        assert call(shape=(1, 1, 1, 64), x=24, ws_bytes=0) == _lib.ERR_UNSUPPORTED
        assert call(x=24, ws_bytes=0) == _lib.ERR_ALIGNMENT
    # res counts among the big arrays
    for res in (84, 88, 81):
        assert _fwd(res=res) == _lib.ERR_ALIGNMENT
    assert _fwd(res=81, shape=(2, 5, 7, 58)) == _lib.ERR_ALIGNMENT            # c % 4 != 0: 4 bytes
    assert _fwd(res=84, shape=(2, 5, 7, 58), ws_bytes=0) == _lib.ERR_BAD_ARG and "workspace" in _lib.last_error()   # 4 bytes do
    assert _fwd(res=None, layout=NCHW, ws_bytes=0) == _lib.ERR_BAD_ARG
    assert _fwd(res=84, layout=NCHW, ws_bytes=0) == _lib.ERR_UNSUPPORTED
    assert _fwd(res=84, ws_bytes=0) == _lib.ERR_ALIGNMENT
    assert _fwd(y=16) == _lib.ERR_BAD_ARG and "alias" in _lib.last_error()
    assert _fwd(y=80) == _lib.ERR_BAD_ARG and "alias" in _lib.last_error()    # y == res
    assert _fwd(rm=16) == _lib.ERR_BAD_ARG                                    # running_mean without running_var
    # gres is optional; given, it is aligned like gx and aliases nothing
    assert _bwd(gres=None, shape=(0, 5, 7, 64), ws=None, ws_bytes=0) == _lib.OK
    assert _bwd(gres=100) == _lib.ERR_ALIGNMENT and "gres" in _lib.last_error()
    for other in (16, 32, 48, 64):
        assert _bwd(gres=other) == _lib.ERR_BAD_ARG and "alias" in _lib.last_error()
    for other in (16, 32, 48):
        assert _bwd(gx=other) == _lib.ERR_BAD_ARG and "alias" in _lib.last_error()


def _step(model, x):
    model.zero_grad(set_to_none=True)
    xi = x.clone().requires_grad_(True)
    y = model(xi)
    y.square().mean().backward()
    # (a parameter that the forward does not use has no gradient: a zero stands in, on both sides of a comparison)
    return [y.detach().clone(), xi.grad.clone()] + [torch.zeros(()) if p.grad is None else p.grad.clone() for p in model.parameters()]


def _bns(blk):
    return [blk.bn1, blk.bn2, blk.bn3]


def test_pass_fallback_and_restore_on_a_cpu_model():
    model = R.stack().train()
    model[1].eval()                                                       # the training flags are put back module by module
    ref = copy.deepcopy(model)
    before = dict(model.named_modules())
    ids = [id(p) for p in model.parameters()]
    keys = list(model.state_dict().keys())
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    ref_opt = torch.optim.SGD(ref.parameters(), lr=0.1)
    x = R.example()

    assert fusion.use_device_bottleneck_train(model, x, min_elements=0) == 2
    assert fusion.use_device_bottleneck_train(model, x, min_elements=0) == 0   # nothing left to take
    for name, mod in before.items():
        now = dict(model.named_modules())[name]
        train = not (name + ".").startswith("1.")
        if name.split(".")[-1] in ("bn1", "bn2", "bn3") and not name.split(".")[-2] == "downsample":
            assert isinstance(now, fusion.TrainBatchNorm2d) and now._bn is mod and not now._relu and now.min_elements == 0
            assert now.training == mod.training == train
        else:
            assert now is mod and now.training == train, name
    assert type(model[0].downsample[1]) is nn.BatchNorm2d                 # use_device_bn_train's, not this pass's
    assert all("forward" in b.__dict__ for b in model)
    assert list(model.state_dict().keys()) == keys
    assert [id(p) for p in model.parameters()] == ids
    assert all(a is b for a, b in zip(opt.param_groups[0]["params"], model.parameters()))
    for k, v in ref.state_dict().items():
        assert torch.equal(model.state_dict()[k], v), k                   # the eval-mode verification updated nothing

    model.train(), ref.train()
    for step in range(2):                                                 # forward, input and parameter gradients, statistics
        for a, b in zip(_step(model, x), _step(ref, x)):
            assert torch.equal(a, b), step
        for k, v in ref.state_dict().items():
            assert torch.equal(model.state_dict()[k], v), (step, k)
        assert [bn._last_kernel for b in model for bn in _bns(b)] == ["aten"] * 6
        opt.step()                                                        # the optimizer built before the pass steps the
        ref_opt.step()                                                    # same parameters
        for p, q in zip(model.parameters(), ref.parameters()):
            assert torch.equal(p, q)
    model.eval(), ref.eval()
    with torch.no_grad():
        assert torch.equal(model(x), ref(x))

    model.double()                                                        # buffers are replaced by a cast: restore re-points them
    assert fusion.restore_bottleneck_train(model) == 2
    assert dict(model.named_modules()) == before
    assert not any("forward" in b.__dict__ or "_bn_bottleneck" in b.__dict__ for b in model)
    assert model[0].bn3.running_mean.dtype == torch.float64
    assert model[0].bn3.running_mean is model.state_dict(keep_vars=True)["0.bn3.running_mean"]
    assert not model[0].bn3.training and list(model.state_dict().keys()) == keys
    assert fusion.restore_bottleneck_train(model) == 0
    with torch.no_grad():
        assert torch.equal(model(x.double()), ref.double()(x.double()))


def test_look_alikes_are_left_alone():
    model = R.mixed().train()
    ref = copy.deepcopy(model)
    before = dict(model.named_modules())
    keys = list(model.state_dict().keys())
    x = R.example32()
    assert all(fusion._bn_bottleneck_candidate(b) for b in model)        # by name they all are Bottlenecks
    assert fusion.use_device_bottleneck_train(model, x, min_elements=0) == 1
    assert ["forward" in b.__dict__ for b in model] == [False, True, False, False]
    for i in (0, 2, 3):
        for name in ("bn1", "bn2", "bn3"):
            assert getattr(model[i], name) is before[f"{i}.{name}"]
    assert all(isinstance(bn, fusion.TrainBatchNorm2d) for bn in _bns(model[1]))
    assert model.training and all(m.training for m in model.modules())
    for a, b in zip(_step(model, x), _step(ref, x)):
        assert torch.equal(a, b)
    assert fusion.restore_bottleneck_train(model) == 1
    assert dict(model.named_modules()) == before and list(model.state_dict().keys()) == keys
    model.eval(), ref.eval()
    with torch.no_grad():
        assert torch.equal(model(x), ref(x))


def test_a_block_that_runs_twice_is_not_taken():
    """One recorded input and one recorded output per block is what the verification rests on; the training flags and the stock
    modules are as before."""
    torch.manual_seed(1)
    blk = R.randomize(R.Bottleneck(32, 8, 32))
    model = nn.Sequential(blk, blk).train()
    assert fusion.use_device_bottleneck_train(model, R.example32(), min_elements=0) == 0
    assert "forward" not in blk.__dict__ and type(blk.bn1) is nn.BatchNorm2d and blk.training and blk.bn1.training


@pytest.mark.parametrize("order", ["bn_train_first", "bottleneck_first"])
def test_either_order_with_use_device_bn_train(order):
    model = R.stack().train()
    ref = copy.deepcopy(model)
    before = dict(model.named_modules())
    x = R.example()
    if order == "bn_train_first":
        assert fusion.use_device_bn_train(model, min_elements=0) == 7
        early = _bns(model[0]) + _bns(model[1])
        assert fusion.use_device_bottleneck_train(model, x, min_elements=0) == 2
        assert _bns(model[0]) + _bns(model[1]) == early                  # wrappers that are there are reused
    else:
        assert fusion.use_device_bottleneck_train(model, x, min_elements=0) == 2
        assert fusion.use_device_bn_train(model, min_elements=0) == 1     # the downsample's BatchNorm
    assert isinstance(model[0].downsample[1], fusion.TrainBatchNorm2d)
    assert all(isinstance(bn, fusion.TrainBatchNorm2d) and not bn._relu and bn.training for b in model for bn in _bns(b))
    for a, b in zip(_step(model, x), _step(ref, x)):
        assert torch.equal(a, b)
    if order == "bn_train_first":
        # this pass's undo leaves the earlier wrappers; the blocks run their class forward on them again
        assert fusion.restore_bottleneck_train(model) == 2
        assert _bns(model[0]) + _bns(model[1]) == early and not any("forward" in b.__dict__ for b in model)
        for a, b in zip(_step(model, x), _step(ref, x)):
            assert torch.equal(a, b)
        assert fusion.restore_bn_train(model) == 7
    else:
        # restore_bn_train on rewritten blocks: no instance forward is left calling a stock BatchNorm with keywords
        assert fusion.restore_bn_train(model) == 1
        assert not any("forward" in b.__dict__ for b in model)
    assert dict(model.named_modules()) == before
    for a, b in zip(_step(model, x), _step(ref, x)):
        assert torch.equal(a, b)


def test_module_keywords_on_the_fallback():
    """relu=None keeps the module's own flag; relu / residual per call compute what the stock statements compute."""
    torch.manual_seed(2)
    bn = R.randomize(nn.BatchNorm2d(8)).train()
    ref = copy.deepcopy(bn)
    wrap = fusion.TrainBatchNorm2d(bn, 0)
    x, idt = torch.randn(3, 8, 4, 5), torch.randn(3, 8, 4, 5)
    assert torch.equal(wrap(x), ref(x)) and wrap._last_kernel == "aten"
    assert torch.equal(wrap(x, relu=True), torch.relu(ref(x)))
    out = ref(x)
    out += idt
    assert torch.equal(wrap(x, residual=idt, relu=True), torch.relu(out))
    out = ref(x)
    out += idt
    assert torch.equal(wrap(x, residual=idt, relu=False), out)
    assert int(wrap.num_batches_tracked) == int(ref.num_batches_tracked) == 4
    assert torch.equal(wrap.running_mean, ref.running_mean)
    wrap._relu = True
    assert torch.equal(wrap(x), torch.relu(ref(x))) and torch.equal(wrap(x, relu=False), ref(x))
