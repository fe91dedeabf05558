"""CPU: the host side of the QAT step on 1-byte codes for Bottlenecks.  The residual-and-codes form of
training-mode BatchNorm2d, slfp_bn_res_codes_train_supported / _fwd of csrc/bn_train.hip: the exports, the supported set and the
refusals, all before any device work (fake pointers, no device).  fusion.link_bottleneck_codes_train / unlink_bottleneck_codes_train
on models built on the CPU, where every call falls back."""
import copy
import itertools
import os
import re

import pytest
import torch
import torch.nn as nn

import _bn_res_blocks as R
import _bottleneck_q_blocks as Q
from cnns_slfp_quantization_amd import _lib, batchnorm, fusion
from cnns_slfp_quantization_amd import conv2d_func as cf

NEW = ("slfp_bn_res_codes_train_supported", "slfp_bn_res_codes_train_fwd")
NHWC, NCHW = _lib.LAYOUT_NHWC, _lib.LAYOUT_NCHW
KA = 2.6023073196411133 / 15.5


def test_new_symbols_are_exported_bound_and_declared():
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "slfp.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert hasattr(L, name) and getattr(L, name).argtypes is not None
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    doc = header[header.index("the\n * residual-and-codes form"):]
    for text in ("slfp_bn_res_train_fwd's, bit for bit", "SLFP_FMT_EXT", "A NaN in y takes code 0x00", "one dword",
                 "slfp_bn_res_train_bwd, as it is", "y_codes may alias no other operand", "No atomics"):
        assert text in doc, text
    assert L.slfp_version() == 1   # new exports only


def _sup(shape=(2, 5, 7, 64), layout=NHWC, ka=KA, qbits=8):
    return _lib.load().slfp_bn_res_codes_train_supported(*shape, layout, ka, qbits)


def test_supported_set():
    L = _lib.load()
    for qbits in (8, 7):
        for shape in ((2, 5, 7, 32), (3, 1, 1, 64), (2, 3, 3, 1024), (0, 5, 7, 64), (64, 56, 56, 256)):
            assert _sup(shape, qbits=qbits) == 1, shape
            assert _sup(shape, qbits=qbits) == L.slfp_bn_codes_train_supported(*shape, NHWC, KA, qbits)
    assert _sup((4, 9, 3, 58)) == 0 and _sup((5, 7, 3, 6)) == 0          # c % 4 != 0
    assert _sup((1, 1, 1, 64)) == 0                                       # what the plain form refuses
    assert _sup(layout=NCHW) == 0
    for qbits in (32, 0, 6, 9, -8):
        assert _sup(qbits=qbits) == 0, qbits
    for ka in (0.0, -KA, float("nan"), float("inf"), 1e-38):
        assert _sup(ka=ka) == 0, ka


def _fwd(x=16, res=32, gamma=16, beta=16, rm=None, rv=None, relu=1, ka=KA, qbits=8, y=48, yc=68, sm=16, si=16, shape=(2, 5, 7, 64),
         layout=NHWC, ws=80, ws_bytes=1 << 30):
    return _lib.load().slfp_bn_res_codes_train_fwd(x, res, gamma, beta, rm, rv, 0.1, 1e-5, relu, ka, qbits, y, yc, sm, si, *shape,
                                                   layout, ws, ws_bytes, None)


def test_refused_before_any_device_work():
    # the pointers are never dereferenced and no launch is made: every refusal comes first (this machine may have no GPU)
    need = _lib.load().slfp_bn_train_workspace_bytes(2, 5, 7, 64)
    for name in ("x", "res", "gamma", "beta", "y", "yc", "sm", "si"):
        assert _fwd(**{name: None}) == _lib.ERR_BAD_ARG, name
        assert "null pointer" in _lib.last_error()
    # what the residual form refuses, in its order
    assert _fwd(layout=7) == _lib.ERR_BAD_ARG and _fwd(relu=2) == _lib.ERR_BAD_ARG
    assert _fwd(shape=(2, 0, 7, 64)) == _lib.ERR_SHAPE
    assert _fwd(layout=NCHW) == _lib.ERR_UNSUPPORTED and "slfp_bn_train_supported" in _lib.last_error()
    assert _fwd(shape=(1, 1, 1, 64)) == _lib.ERR_UNSUPPORTED
    for name in ("x", "res", "y"):
        assert _fwd(**{name: 24}) == _lib.ERR_ALIGNMENT, name
    assert _fwd(ws_bytes=need - 1) == _lib.ERR_BAD_ARG and "workspace" in _lib.last_error()
    assert _fwd(ws=None) == _lib.ERR_BAD_ARG
    assert _fwd(y=16) == _lib.ERR_BAD_ARG and "alias" in _lib.last_error()          # y == x
    assert _fwd(y=32) == _lib.ERR_BAD_ARG and "alias" in _lib.last_error()          # y == res
    assert _fwd(rm=16) == _lib.ERR_BAD_ARG
    assert _fwd(shape=(0, 5, 7, 64), ws=None, ws_bytes=0) == _lib.OK                # n == 0: nothing to do
    # what the code form refuses
    for kw in (dict(shape=(4, 9, 3, 58)), dict(shape=(5, 7, 3, 6)), dict(qbits=6), dict(qbits=32), dict(ka=0.0), dict(ka=-KA),
               dict(ka=float("nan"))):
        assert _fwd(**kw) == _lib.ERR_UNSUPPORTED, kw
        assert "codes_train_supported" in _lib.last_error()
        assert _fwd(x=None, **kw) == _lib.ERR_BAD_ARG                               # ... behind the null pointers
    for yc in (65, 66, 67):
        assert _fwd(yc=yc) == _lib.ERR_ALIGNMENT and "y_codes" in _lib.last_error()
    assert _fwd(yc=68, ws_bytes=0) == _lib.ERR_BAD_ARG                              # 4 bytes are enough for y_codes
    # y_codes aliasing any other operand
    for name, at in (("x", 16), ("res", 32), ("y", 48), ("ws", 80)):
        assert _fwd(yc=at) == _lib.ERR_BAD_ARG and "alias" in _lib.last_error(), name
    assert _fwd(rm=112, rv=128, yc=112) == _lib.ERR_BAD_ARG and "alias" in _lib.last_error()
    assert _fwd(rm=112, rv=128, yc=128) == _lib.ERR_BAD_ARG and "alias" in _lib.last_error()


# ---- fusion.link_bottleneck_codes_train on models built on the CPU --------------------------------------------------------------
def _rewritten(**kw):
    model = Q.stack(host=True, **kw)
    x = R.example()
    assert fusion.use_device_bottleneck_train(model, x, min_elements=0) == Q.GENUINE
    return model, x


def test_without_rewritten_blocks_nothing_is_touched():
    model = Q.stack(host=True)
    before = dict(model.named_modules())
    assert fusion.link_bottleneck_codes_train(model, R.example(), min_elements=0) == (0, 0)
    assert dict(model.named_modules()) == before and not any("forward" in m.__dict__ for m in model.modules())
    assert fusion.unlink_bottleneck_codes_train(model) == (0, 0)


def test_candidates_refusals_and_counts():
    model, x = _rewritten()
    keys = list(model.state_dict().keys())
    ids = [id(p) for p in model.parameters()]
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    flags = [m.training for m in model.modules()]
    tree = dict(model.named_modules())
    assert Q.expected_links(model) == (6, 1)
    assert fusion.link_bottleneck_codes_train(model, x) == (6, 1)
    assert fusion.link_bottleneck_codes_train(model, x) == (0, 0)                  # nothing left to take
    a, b, c = list(model)[:3]
    for blk in (a, b, c):
        for bn, conv in ((blk.bn1, blk.conv2), (blk.bn2, blk.conv3)):
            assert isinstance(bn, fusion.TrainBatchNormCodes2d) and bn._conv is conv and bn.min_elements is None
            assert bn._ka == cf._f32(conv.Ka) and bn._q_bit == 8 and bn._fallback == (True, 0) and not bn._modules
        assert isinstance(blk.bn3, fusion.TrainBatchNorm2d)
    assert a.bn3._trunk == ((b.conv1,), cf._f32(b.conv1.Ka), 8, None)              # A -> B: one reader
    assert b.bn3._trunk is None                                                    # into C: conv1 and downsample.0 differ in Ka
    assert c.bn3._trunk is None                                                    # read by plain nn.Conv2d only
    assert not a.bn3._modules                                                      # the readers are no children of the wrapper
    for blk in list(model)[3:]:                                                    # the look-alikes: untouched
        assert "forward" not in blk.__dict__ and type(blk.bn1) is nn.BatchNorm2d
    assert all(c._post is None and c._code_out is None for c in Q.convs(model))    # the readers are not modified
    assert list(model.state_dict().keys()) == keys and [id(p) for p in model.parameters()] == ids
    assert all(p is q for p, q in zip(opt.param_groups[0]["params"], model.parameters()))
    assert [m.training for m in tree.values()] == flags
    assert fusion.unlink_bottleneck_codes_train(model) == (6, 1)
    assert dict(model.named_modules()) == tree and a.bn3._trunk is None
    assert fusion.unlink_bottleneck_codes_train(model) == (0, 0)


def test_each_refusal_costs_exactly_its_own_link():
    model, x = _rewritten()
    model[0].conv2._post = (None, None, 1)                                         # something fused onto a reader: that pair alone
    model[1].conv1.q_bit = 32                                                      # the one reader of A's trunk is no code reader
    assert fusion.link_bottleneck_codes_train(model, x, min_elements=0) == (5, 0)
    assert isinstance(model[0].bn1, fusion.TrainBatchNorm2d) and isinstance(model[0].bn2, fusion.TrainBatchNormCodes2d)
    assert model[0].bn2.min_elements == 0
    model2, x = _rewritten()
    model2[2].downsample[0].Ka = model2[2].conv1.Ka.clone()                        # the boundary's readers agree: B's trunk links too
    assert fusion.link_bottleneck_codes_train(model2, x, min_elements=0) == (6, 2)
    assert model2[1].bn3._trunk[0] == (model2[2].conv1, model2[2].downsample[0]) and model2[1].bn3._trunk[3] == 0


UNDO = {"unlink": fusion.unlink_bottleneck_codes_train, "bottleneck": fusion.restore_bottleneck_train, "bn": fusion.restore_bn_train,
        "codes": fusion.unlink_codes_train}


@pytest.mark.parametrize("order", list(itertools.permutations(UNDO)), ids="-".join)
def test_the_undo_functions_in_each_order_give_back_the_module_tree(order):
    model = Q.stack(host=True)
    ref = copy.deepcopy(model)
    tree = dict(model.named_modules())
    x = R.example()
    assert fusion.use_device_bottleneck_train(model, x, min_elements=0) == Q.GENUINE
    assert fusion.link_bottleneck_codes_train(model, x, min_elements=0) == (6, 1)
    model.double()                                                                 # buffers are replaced by a cast: the undo re-points them
    model.float()
    for i, name in enumerate(order):
        UNDO[name](model)
        for blk in model:                                                          # consistent after every call: no slot that owns its
            if "forward" not in blk.__dict__:                                      # ReLU under a forward that does not know it
                assert not any(isinstance(m, fusion.TrainBatchNormCodes2d) for m in blk.modules()), (order, i)
        model.train()
        model(x)                                                                   # ... and it runs
    assert dict(model.named_modules()) == tree
    assert not any("forward" in m.__dict__ or "_bn_bottleneck_codes" in m.__dict__ for m in model.modules())
    for m in (model, ref):
        m.train()
    assert torch.equal(model(x), ref(x))
    assert model[0].bn1.running_mean is model.state_dict(keep_vars=True)["0.bn1.running_mean"]


def test_a_linked_cpu_model_computes_what_the_unlinked_one_computes():
    """No device: every call falls back, in training and in eval mode, through two optimizer steps."""
    model, x = _rewritten()
    ref = copy.deepcopy(model)
    stock = Q.stack(host=True)
    assert fusion.link_bottleneck_codes_train(model, x, min_elements=0) == (6, 1)
    opts = [torch.optim.SGD(m.parameters(), lr=0.05, momentum=0.9) for m in (model, ref, stock)]
    for training in (True, True, False):
        outs = []
        for m in (model, ref, stock):
            m.train(training)
            m.zero_grad(set_to_none=True)
            xi = x.clone(memory_format=torch.preserve_format).requires_grad_(training)
            y = m(xi)
            if training:
                y.square().mean().backward()
            outs.append((y.detach(), xi.grad, [p.grad for p in m.parameters()]))
        for other in outs[1:]:
            assert torch.equal(outs[0][0], other[0])
            assert (outs[0][1] is None and other[1] is None) or torch.equal(outs[0][1], other[1])
            assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(outs[0][2], other[2]))
        for k, v in ref.state_dict().items():
            assert torch.equal(model.state_dict()[k], v), k
        assert model[0].bn1._last_kernel == "aten" and model[0].bn3._last_kernel == "aten"
        if training:
            for o in opts:
                o.step()
    assert int(model[0].bn3.num_batches_tracked) == 2


def test_the_default_size_rule_follows_from_the_committed_measurement():
    """batchnorm.RES_CODES_MIN_ELEMENTS admits exactly the size classes the spread rule admits in both committed runs of
    profiles/bn_res_codes_train_bench.py; None where no class qualifies."""
    import json
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles")
    runs = [json.load(open(os.path.join(here, name))) for name in ("bn_res_codes_train_bench.json", "bn_res_codes_train_bench_second.json")]
    admitted = None
    for res in runs:
        rows = res["trunks"]
        classes = sorted({r["elements"] for r in rows}, reverse=True)
        mine = []
        for e in classes:
            if not all(r["faster_beyond_spread"] for r in rows if r["elements"] == e):
                break
            mine.append(e)
        assert res["rule"]["res_codes_min_elements_by_the_spread_rule"] == (mine[-1] if mine else None)
        admitted = set(mine) if admitted is None else admitted & set(mine)
        for r in rows:   # what a row claims is what its figures say
            other = r[r["better_unlinked_leg"] + "_ms"]
            assert other == min(r["stock_ms"], r["unlinked_ms"])
            assert r["faster_beyond_spread"] == (r["linked_ms"] < other * (1 - r[r["better_unlinked_leg"] + "_spread"]))
    floor = batchnorm.RES_CODES_MIN_ELEMENTS
    classes = sorted({r["elements"] for r in runs[0]["trunks"]}, reverse=True)
    top = []
    for e in classes:   # admitted in both runs, from the largest class down without a gap
        if e not in admitted:
            break
        top.append(e)
    if not top:
        assert floor is None
    else:
        assert floor is not None and [e for e in classes if e >= floor] == top
