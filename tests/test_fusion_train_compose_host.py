"""CPU: the training-mode passes of fusion_train.py and restore_avgpool in every order of apply and undo.  After
every single call each placeholder stands next to the wrapper of the pass that owns it and each wrapper has its placeholder(s)
(`intact`); after the last undo the module tree is the original by identity.  Nothing here runs a kernel: the passes that trace do
so in eval mode, where every wrapper computes with ATen."""
import itertools

import pytest
import torch
import torch.nn as nn

import _bottleneck_q_blocks as Q
from cnns_slfp_quantization_amd import activation_func as af, fusion
from cnns_slfp_quantization_amd import conv2d_func as cf
from cnns_slfp_quantization_amd.sfp_quant import layerout_quantize_func


def _conv(c_in, c_out, k=1):
    return cf.conv2d_Q(8, 0.1, 0.2)(c_in, c_out, k, padding=k // 2, bias=False)


def _siblings(model):
    for parent in model.modules():
        kids = list(parent._modules.values())
        for i, kid in enumerate(kids):
            yield kid, (kids[i - 1] if i else None), (kids[i + 1] if i + 1 < len(kids) else None), kids[max(i - 2, 0):i]


def intact(model):
    """Every FoldedReLU / FoldedTail in a slot stands where its owner puts it, next to that owner's wrapper, and every wrapper
    that folds something has its placeholder(s).  Returns the first violation as a string, or None."""
    for kid, prev, nxt, two_before in _siblings(model):
        if isinstance(kid, fusion.FoldedReLU):
            if kid.owner == "avgpool":
                ok = isinstance(nxt, fusion.GlobalAvgPool2d) and nxt._relu
            elif kid.owner == "bn_train":   # behind its TrainBatchNorm2d, or behind the link that holds both
                ok = (isinstance(prev, fusion.TrainBatchNorm2d) and prev._relu) or (
                    isinstance(prev, fusion.TrainBatchNormCodes2d) and prev._held[1] is kid
                    and isinstance(prev._held[0], fusion.TrainBatchNorm2d) and prev._held[0]._relu)
            else:
                ok = kid.owner == "codes_train" and isinstance(prev, fusion.TrainBatchNormCodes2d) and prev._held[1] is kid.relu
            if not ok:
                return f"FoldedReLU({kid.owner}) without its wrapper: prev={type(prev).__name__}, next={type(nxt).__name__}"
        elif isinstance(kid, fusion.FoldedTail):
            if not any(isinstance(w, fusion.TrainBatchNormLayerout2d) and (w._layerout is kid.mod or kid.mod in w._acts)
                       for w in two_before):
                return f"FoldedTail({type(kid.mod).__name__}) without its TrainBatchNormLayerout2d"
        elif isinstance(kid, fusion.TrainBatchNorm2d) and kid._relu:
            if not (isinstance(nxt, fusion.FoldedReLU) and nxt.owner == "bn_train"):
                return f"TrainBatchNorm2d(relu) in front of {type(nxt).__name__}"
        elif isinstance(kid, fusion.TrainBatchNormCodes2d) and kid._held[1] is not None:
            held = kid._held[1]
            ok = nxt is held if isinstance(held, fusion.FoldedReLU) else (
                isinstance(nxt, fusion.FoldedReLU) and nxt.owner == "codes_train" and nxt.relu is held)
            if not ok:
                return f"TrainBatchNormCodes2d in front of {type(nxt).__name__}"
        elif isinstance(kid, fusion.TrainBatchNormLayerout2d):
            after = [k for k, _, _, before in _siblings(model) if isinstance(k, fusion.FoldedTail) and kid in before]
            if [k.mod for k in after] != [kid._layerout, *kid._acts]:
                return "TrainBatchNormLayerout2d without its two FoldedTails"
    return None


def _snapshot(model):
    return (dict(model.named_modules()), dict(model.named_parameters()), dict(model.named_buffers()),
            {name: m.training for name, m in model.named_modules()})


def _assert_original(model, snap, what):
    modules, params, buffers, flags = snap
    now = dict(model.named_modules())
    assert list(now) == list(modules) and all(now[k] is modules[k] for k in now), what
    assert all(p is params[k] for k, p in model.named_parameters()) and len(dict(model.named_parameters())) == len(params), what
    assert all(b is buffers[k] for k, b in model.named_buffers()) and len(dict(model.named_buffers())) == len(buffers), what
    assert {name: m.training for name, m in now.items()} == flags, what
    assert not any("forward" in m.__dict__ for m in now.values()), what


def _all_orders(make, passes, undos):
    """Every order of `passes`, then every order of `undos`: `intact` after each call, the original tree at the end."""
    n = 0
    for apply in itertools.permutations(passes):
        for undo in itertools.permutations(undos):
            model = make()
            snap = _snapshot(model)
            for fn in apply + undo:
                fn(model)
                what = ([f.__name__ for f in apply], [f.__name__ for f in undo], fn.__name__)
                assert intact(model) is None, (intact(model), what)
            _assert_original(model, snap, what)
            n += 1
    return n


# ---- the defect: restore_avgpool took link_codes_train's placeholder -----------------------------------------------------------
def test_restore_avgpool_leaves_a_training_links_placeholder():
    m = nn.Sequential(_conv(3, 8, 3), nn.BatchNorm2d(8), nn.ReLU(), _conv(8, 8), nn.BatchNorm2d(8), nn.ReLU(), nn.AdaptiveAvgPool2d(1))
    m.train()
    snap = _snapshot(m)
    relu = m[2]
    assert fusion.link_codes_train(m, 0) == 1
    assert fusion.restore_avgpool(m) == 0
    assert isinstance(m[1], fusion.TrainBatchNormCodes2d)
    assert isinstance(m[2], fusion.FoldedReLU) and m[2].owner == "codes_train" and m[2].relu is relu   # still behind its wrapper
    assert intact(m) is None
    assert fusion.unlink_codes_train(m) == 1
    _assert_original(m, snap, "defect")


def test_a_placeholder_names_one_of_the_three_owners():
    for owner in ("avgpool", "bn_train", "codes_train"):
        assert fusion.FoldedReLU(nn.ReLU(), owner).owner == owner
    for bad in (None, "", "layerout"):
        with pytest.raises(ValueError):
            fusion.FoldedReLU(nn.ReLU(), bad)
    folded = fusion.FoldedReLU(nn.ReLU(), "avgpool")
    assert list(folded._modules) == ["relu"] and not hasattr(folded, "_bn_train") and not hasattr(folded, "_codes_train")
    tail = fusion.FoldedTail(nn.GELU())
    assert not tail._modules and isinstance(tail.mod, nn.GELU)


# ---- nn.Sequential blocks ----------------------------------------------------------------------------------------------------------
def _sequential():
    """Five blocks: three plain [conv, BN, ReLU] (one in place), one [conv, BN, layerout_quantize_func(8), Swish], and a last one in
    front of a global average pool.  link_codes_train finds three hand-overs, use_device_bn_layerout_train one block."""
    torch.manual_seed(2)
    m = nn.Sequential(nn.Sequential(_conv(3, 8, 3), nn.BatchNorm2d(8), nn.ReLU()),
                      nn.Sequential(_conv(8, 8), nn.BatchNorm2d(8), nn.ReLU(inplace=True)),
                      nn.Sequential(_conv(8, 8), nn.BatchNorm2d(8), layerout_quantize_func(8), af.Swish()),
                      nn.Sequential(_conv(8, 8), nn.BatchNorm2d(8), nn.ReLU()),
                      nn.Sequential(_conv(8, 8), nn.BatchNorm2d(8), nn.ReLU(), nn.AdaptiveAvgPool2d(1)))
    return m.train()


def use_device_bn_train(m):
    assert fusion.use_device_bn_train(m, 0) > 0


def use_device_bn_layerout_train(m):
    assert fusion.use_device_bn_layerout_train(m, 0) == 1


def link_codes_train(m):
    assert fusion.link_codes_train(m, 0) == 3


def test_sequential_passes_compose_in_every_order():
    passes = (use_device_bn_train, use_device_bn_layerout_train, link_codes_train)
    undos = (fusion.restore_bn_train, fusion.restore_bn_layerout_train, fusion.unlink_codes_train, fusion.restore_avgpool)
    assert _all_orders(_sequential, passes, undos) == 6 * 24


# ---- Bottlenecks -------------------------------------------------------------------------------------------------------------------
def _image():
    return torch.randn(2, 16, 8, 8, generator=torch.Generator().manual_seed(9)).contiguous(memory_format=torch.channels_last)


def _stack():
    return Q.stack(host=True).train()


def use_device_bottleneck_train(m):
    fusion.use_device_bottleneck_train(m, _image(), 0)


def link_bottleneck_codes_train(m):
    fusion.link_bottleneck_codes_train(m, _image(), 0)


def test_bottleneck_passes_compose_in_every_order():
    passes = (use_device_bn_train, use_device_bottleneck_train, link_bottleneck_codes_train)
    undos = (fusion.restore_bn_train, fusion.restore_bottleneck_train, fusion.unlink_bottleneck_codes_train, fusion.unlink_codes_train)
    assert _all_orders(_stack, passes, undos) == 6 * 24


def test_a_rewritten_block_keeps_one_forward_through_link_and_unlink():
    m, x = _stack(), _image()
    assert fusion.use_device_bottleneck_train(m, x, 0) == Q.GENUINE
    blocks = [b for b in m.modules() if "_bn_bottleneck" in b.__dict__]
    before = [b.__dict__["forward"].__func__ for b in blocks]
    assert len(blocks) == Q.GENUINE and len(set(before)) == 1
    assert fusion.link_bottleneck_codes_train(m, x, 0) == Q.expected_links(m)
    assert [b.__dict__["forward"].__func__ for b in blocks] == before
    assert any(isinstance(w, fusion.TrainBatchNormCodes2d) for w in m.modules())
    assert fusion.unlink_bottleneck_codes_train(m) == Q.expected_links(m)
    assert [b.__dict__["forward"].__func__ for b in blocks] == before
    assert all(b.__dict__["forward"].__self__ is b for b in blocks)
