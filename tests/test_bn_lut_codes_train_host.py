"""CPU: the host side of a QAT step on 1-byte codes for layer-output-quantized blocks.  The table-and-codes form
of training-mode BatchNorm2d, slfp_bn_lut_codes_train_supported / _fwd of csrc/bn_train.hip: the exports, the supported set and every
refusal in its order, all before any device work (fake pointers, no device).  fusion.link_layerout_codes_train /
unlink_layerout_codes_train on models built on the CPU, alone and with the two BatchNorm passes in every order."""
import copy
import itertools
import json
import os
import re

import pytest
import torch
import torch.nn as nn

import _bn_cases as B
import _layerout_codes_models as M
from cnns_slfp_quantization_amd import _lib, activation_func as af, batchnorm, fusion
from cnns_slfp_quantization_amd import conv2d_func as cf
from cnns_slfp_quantization_amd.sfp_quant import layerout_quantize_func

NEW = ("slfp_bn_lut_codes_train_supported", "slfp_bn_lut_codes_train_fwd")
NHWC, NCHW = _lib.LAYOUT_NHWC, _lib.LAYOUT_NCHW
HERE = os.path.dirname(os.path.abspath(__file__))


def test_new_symbols_are_exported_bound_and_declared():
    import ctypes
    L = _lib.load()
    header = open(os.path.join(HERE, "..", "include", "slfp.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert hasattr(L, name)
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    i64, vp, cf32, ci, sz = ctypes.c_int64, ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_size_t
    assert L.slfp_bn_lut_codes_train_supported.argtypes == [i64, i64, i64, i64, ci]
    assert L.slfp_bn_lut_codes_train_fwd.argtypes == [vp] * 5 + [cf32, cf32] + [vp] * 5 + [i64] * 4 + [ci, vp, sz, vp]
    assert L.slfp_bn_lut_codes_train_fwd.argtypes == L.slfp_bn_lut_train_fwd.argtypes   # y_codes where y stood, the table where it stood
    assert L.slfp_version() == 1   # new exports only


def _sup(shape=(2, 5, 7, 64), layout=NHWC):
    return _lib.load().slfp_bn_lut_codes_train_supported(*shape, layout)


def test_supported_set():
    L = _lib.load()
    vector = [s for s, _ in B.cases() if s[3] % 4 == 0]
    assert {(2, 5, 7, 32), (3, 1, 1, 64), (2, 3, 3, 1024), B.ragged(32)} == set(vector)
    for shape in vector + [(0, 5, 7, 64), (128, 32, 32, 64)]:
        assert L.slfp_bn_train_supported(*shape, NHWC) == 1 and _sup(shape) == 1, shape
    assert _sup((4, 9, 3, 58)) == 0 and L.slfp_bn_train_supported(4, 9, 3, 58, NHWC) == 1   # c % 4 != 0
    assert _sup((5, 7, 3, 6)) == 0 and L.slfp_bn_train_supported(5, 7, 3, 6, NHWC) == 1
    assert _sup((1, 1, 1, 64)) == 0                                                         # what the plain form refuses
    assert _sup(layout=NCHW) == 0 and _sup(layout=7) == 0


def _fwd(x=16, gamma=16, beta=16, rm=None, rv=None, tab=32, y=36, sm=16, si=16, lo=16, shape=(2, 5, 7, 64), layout=NHWC, ws=16,
         ws_bytes=1 << 30):
    return _lib.load().slfp_bn_lut_codes_train_fwd(x, gamma, beta, rm, rv, 0.1, 1e-5, tab, y, sm, si, lo, *shape, layout, ws, ws_bytes,
                                                   None)


def _lut(x=16, gamma=16, beta=16, rm=None, rv=None, tab=32, y=48, sm=16, si=16, lo=16, shape=(2, 5, 7, 64), layout=NHWC, ws=16,
         ws_bytes=1 << 30):
    return _lib.load().slfp_bn_lut_train_fwd(x, gamma, beta, rm, rv, 0.1, 1e-5, tab, y, sm, si, lo, *shape, layout, ws, ws_bytes, None)


def test_refused_before_any_device_work():
    # the pointers are never dereferenced and no launch is made: every refusal comes first (this machine may have no GPU), and a
    # refusal that wrote to an output would fault on these addresses
    need = _lib.load().slfp_bn_train_workspace_bytes(2, 5, 7, 64)
    for name in ("x", "gamma", "beta", "tab", "y", "sm", "si", "lo"):
        assert _fwd(**{name: None}) == _lib.ERR_BAD_ARG, name
        assert "null pointer" in _lib.last_error()
    assert _fwd(lo=24) == _lib.ERR_ALIGNMENT
    for tab in (40, 36, 33):
        assert _fwd(tab=tab) == _lib.ERR_ALIGNMENT and "table" in _lib.last_error()
    assert _fwd(layout=NCHW) == _lib.ERR_UNSUPPORTED
    assert "slfp_bn_train_supported" in _lib.last_error()
    assert _fwd(shape=(1, 1, 1, 64)) == _lib.ERR_UNSUPPORTED                 # M == 1
    assert _fwd(shape=(4, 9, 3, 58)) == _lib.ERR_UNSUPPORTED                 # c % 4 != 0
    assert "slfp_bn_lut_codes_train_supported" in _lib.last_error()
    assert _fwd(shape=(5, 7, 3, 6)) == _lib.ERR_UNSUPPORTED
    assert _fwd(layout=7) == _lib.ERR_BAD_ARG
    assert _fwd(shape=(2, 0, 7, 64)) == _lib.ERR_SHAPE
    assert _fwd(x=24) == _lib.ERR_ALIGNMENT
    for y in (33, 34, 35, 37):
        assert _fwd(y=y) == _lib.ERR_ALIGNMENT and "y_codes" in _lib.last_error()
        assert _fwd(y=y, ws_bytes=0) == _lib.ERR_ALIGNMENT                   # before the workspace
    assert _fwd(y=36, ws_bytes=0) == _lib.ERR_BAD_ARG                        # 4 bytes are enough for y_codes
    assert _fwd(ws_bytes=need - 1) == _lib.ERR_BAD_ARG and "workspace" in _lib.last_error()
    assert _fwd(ws=None) == _lib.ERR_BAD_ARG
    assert _fwd(ws=24) == _lib.ERR_BAD_ARG
    assert _fwd(shape=(0, 5, 7, 64), ws=None, ws_bytes=0) == _lib.OK         # n == 0: nothing to do
    assert _fwd(y=16) == _lib.ERR_BAD_ARG and "alias" in _lib.last_error()
    assert _fwd(rm=16) == _lib.ERR_BAD_ARG                                    # running_mean without running_var
    assert _fwd(rm=18, rv=16) == _lib.ERR_ALIGNMENT


def test_the_refusals_come_in_the_order_of_the_lut_form():
    """The same bad call to both entry points gives the same code, for every pair of faults (y_codes standing where y stood): null
    pointers, the layout, the geometry, what is unsupported, alignment (x / y, the per-channel arrays, the table), the workspace, the
    running statistics, aliasing."""
    faults = {"null_x": dict(x=None), "null_y": dict(y=None), "null_lo": dict(lo=None), "null_tab": dict(tab=None),
              "layout": dict(layout=7), "geometry": dict(shape=(2, 0, 7, 64)), "nchw": dict(layout=NCHW), "m1": dict(shape=(1, 1, 1, 64)),
              "x_align": dict(x=24), "lo_align": dict(lo=24), "tab_align": dict(tab=40), "ws": dict(ws_bytes=0), "rm": dict(rm=16),
              "rm_align": dict(rm=18, rv=16), "alias": dict(y=16)}
    codes = set()
    for a, b in itertools.combinations(faults, 2):
        kw = {**faults[a], **faults[b]}
        if len(kw) < len(faults[a]) + len(faults[b]):
            continue   # two faults of one argument
        got, want = _fwd(**kw), _lut(**kw)
        assert got == want, (a, b, got, want)
        codes.add(got)
    assert codes == {_lib.ERR_BAD_ARG, _lib.ERR_SHAPE, _lib.ERR_UNSUPPORTED, _lib.ERR_ALIGNMENT}
    # its own: c % 4 behind what the plain form refuses and in front of every alignment; y_codes behind x and in front of the arrays
    assert _fwd(shape=(4, 9, 3, 58), x=20, ws_bytes=0) == _lib.ERR_UNSUPPORTED and "lut_codes" in _lib.last_error()
    assert _fwd(shape=(4, 9, 3, 58), layout=NCHW) == _lib.ERR_UNSUPPORTED and "slfp_bn_train_supported" in _lib.last_error()
    assert _fwd(x=24, y=33) == _lib.ERR_ALIGNMENT and "y_codes" not in _lib.last_error()
    assert _fwd(y=33, lo=24, tab=40) == _lib.ERR_ALIGNMENT and "y_codes" in _lib.last_error()
    assert _fwd(lo=24, tab=40) == _lib.ERR_ALIGNMENT and "per-channel" in _lib.last_error()


# ---- the Python side that needs no device --------------------------------------------------------------------------------------
def test_the_table_builder_refuses_what_has_no_derivative_table():
    with pytest.raises(TypeError):
        batchnorm.layerout_code_table([af.STL()], 0.2, 8, "cpu")
    with pytest.raises(TypeError):
        batchnorm.layerout_code_table([nn.ReLU6()], 0.2, 8, "cpu")
    with pytest.raises(ValueError):
        batchnorm.layerout_code_table([nn.GELU()], 0.2, 32, "cpu")
    with pytest.raises(TypeError):
        batchnorm.layerout_act_tables([af.STL()], "cpu")                     # the same set


def test_the_size_rule_and_the_placeholders_owner():
    assert batchnorm.LUT_CODES_MIN_ELEMENTS is None or batchnorm.LUT_CODES_MIN_ELEMENTS > 0
    x = torch.zeros(2, 32, 4, 4).contiguous(memory_format=torch.channels_last)
    assert batchnorm.bn_lut_codes_train_supported(x, 0) is False             # a CPU tensor
    assert fusion.FoldedTail(nn.GELU()).owner == "bn_layerout_train"        # the existing owner is the default
    assert fusion.FoldedTail(nn.GELU(), "layerout_codes_train").owner == "layerout_codes_train"
    for bad in (None, "", "codes_train"):
        with pytest.raises(ValueError):
            fusion.FoldedTail(nn.GELU(), bad)
    link = batchnorm.TrainLink(None, None, None, (1, 2, 3), True, 0.2, 8, None)
    assert link.dtab is None and link.relu is True                          # the ReLU form's record is what it was
    assert batchnorm.TrainLink(None, None, None, (1, 2, 3), False, 0.2, 8, None, "D").dtab == "D"


# ---- fusion.link_layerout_codes_train on models built on the CPU -----------------------------------------------------------------
def _snapshot(model):
    return (dict(model.named_modules()), dict(model.named_parameters()), dict(model.named_buffers()),
            {name: m.training for name, m in model.named_modules()})


def _assert_original(model, snap, what=""):
    modules, params, buffers, flags = snap
    now = dict(model.named_modules())
    assert list(now) == list(modules) and all(now[k] is modules[k] for k in now), what
    assert all(p is params[k] for k, p in model.named_parameters()) and len(dict(model.named_parameters())) == len(params), what
    assert all(b is buffers[k] for k, b in model.named_buffers()) and len(dict(model.named_buffers())) == len(buffers), what
    assert {name: m.training for name, m in now.items()} == flags, what


@pytest.mark.parametrize("make,links", [(M.mobilenet_swish_stack, M.MOBILENET_LINKS), (M.vgg_gelu_stack, M.VGG_LINKS)],
                         ids=["mobilenet_swish", "vgg_gelu"])
def test_link_finds_the_hand_overs_and_unlink_restores_the_objects(make, links):
    model = make().train()
    snap = _snapshot(model)
    keys = list(model.state_dict().keys())
    ids = [id(p) for p in model.parameters()]
    want = {k: v.clone() for k, v in model.state_dict().items()}
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    assert fusion.link_layerout_codes_train(model) == links
    assert fusion.link_layerout_codes_train(model) == 0                    # nothing left to take
    assert M.intact(model) is None
    wraps = [m for m in model.modules() if isinstance(m, fusion.TrainBatchNormLayeroutCodes2d)]
    convs = M.convs(model)
    assert len(wraps) == links
    if make is M.mobilenet_swish_stack:
        assert [w._conv for w in wraps] == convs[1:]                       # a block's last activation meets the next block's first conv
        assert type(model[0][2][5]) is nn.BatchNorm2d                      # behind the last conv: the pool
    else:
        assert [w._conv for w in wraps] == [convs[1], convs[3]]            # never across a MaxPool2d
        assert type(model[5]) is nn.BatchNorm2d and type(model[6]) is layerout_quantize_func and isinstance(model[8], nn.MaxPool2d)
    for w, c in zip(wraps, [w._conv for w in wraps]):
        assert w._ka == cf._f32(c.Ka) and w._q_bit == 8 and w.min_elements is None and w._fallback == (False, None)
        assert not w._modules                                              # the held modules and the conv sit outside _modules
    assert list(model.state_dict().keys()) == keys
    assert [id(p) for p in model.parameters()] == ids
    assert all(a is b for a, b in zip(opt.param_groups[0]["params"], model.parameters()))
    for k, v in want.items():
        assert torch.equal(model.state_dict()[k], v), k
    model.double()                                                         # buffers are replaced by a cast: unlink re-points them
    assert fusion.unlink_layerout_codes_train(model) == links
    assert dict(model.named_modules()) == snap[0]                          # the very same module objects
    bn = [m for m in model.modules() if isinstance(m, nn.BatchNorm2d)][0]
    assert bn.running_mean.dtype == torch.float64 and any(bn.running_mean is b for b in model.buffers())
    assert fusion.unlink_layerout_codes_train(model) == 0


def test_link_leaves_ineligible_runs_alone():
    conv = cf.conv2d_Q_bias(8, 0.1, 0.2)
    shared_act, shared_lo = nn.GELU(), layerout_quantize_func(8)

    def run(bn=None, lo=None, act=None, c=None):
        return [bn or nn.BatchNorm2d(8), lo or layerout_quantize_func(8), act or af.Swish(), c or conv(8, 8, 1)]

    relu_bn = nn.Sequential(nn.BatchNorm2d(8), nn.ReLU())
    assert fusion.use_device_bn_train(relu_bn, 0) == 1 and relu_bn[0]._relu
    fused = conv(8, 8, 1); fused._post = (None, None, 1)
    m = nn.Sequential(*run(), *run(lo=layerout_quantize_func(7), act=nn.GELU(), c=conv(8, 8, 3, padding=1)),   # 0..7: two links
                      *run(act=af.STL()), *run(lo=layerout_quantize_func(32)), *run(act=shared_act), *run(act=shared_act),
                      *run(lo=shared_lo), *run(lo=shared_lo), *run(bn=relu_bn[0]), *run(bn=nn.BatchNorm2d(8, affine=False)),
                      *run(bn=nn.BatchNorm2d(8, momentum=None)), *run(c=fused), *run(c=cf.conv2d_Q(32, 0.1, 0.2)(8, 8, 1)),
                      *run(c=nn.Conv2d(8, 8, 1)), *run(c=cf.conv2d_Q(8, 0.1, 0.2)(8, 8, 1, bias=True)),
                      nn.BatchNorm2d(8), layerout_quantize_func(8), nn.GELU(), nn.MaxPool2d(2), conv(8, 8, 1),   # a pool in between
                      nn.BatchNorm2d(8), layerout_quantize_func(8), nn.GELU(), nn.ReLU(), conv(8, 8, 1),        # two activations
                      *run(act=nn.ReLU(inplace=True)))                                                          # a ReLU behind the quantizer: a link
    before = dict(m.named_modules())
    assert fusion.link_layerout_codes_train(m, min_elements=0) == 3
    taken = [i for i, c in enumerate(m) if isinstance(c, fusion.TrainBatchNormLayeroutCodes2d)]
    assert taken == [0, 4, len(m) - 4] and m[4]._q_bit == 8 and m[4]._layerout.q_bit == 7 and m[0].min_elements == 0
    assert M.intact(m) is None
    assert fusion.unlink_layerout_codes_train(m) == 3 and dict(m.named_modules()) == before
    twice = nn.Sequential(*run()[:3])                                      # a block held twice has two successors
    assert fusion.link_layerout_codes_train(nn.Sequential(twice, conv(8, 8, 1), twice, conv(8, 8, 1)), 0) == 0

    class Wired(nn.Module):                                                # a hand-wired block: no nn.Sequential, nothing to find
        def __init__(self):
            super().__init__()
            self.bn, self.lo, self.act, self.conv = run()

        def forward(self, x):
            return self.conv(self.act(self.lo(self.bn(x))))

    assert fusion.link_layerout_codes_train(nn.Sequential(Wired(), Wired()), 0) == 0


def link(m):
    assert fusion.link_layerout_codes_train(m, 0) > 0


def use_device_bn_layerout_train(m):
    fusion.use_device_bn_layerout_train(m, 0)


def use_device_bn_train(m):
    fusion.use_device_bn_train(m, 0)


@pytest.mark.parametrize("make,links,bns", [(M.mobilenet_swish_stack, M.MOBILENET_LINKS, 5), (M.vgg_gelu_stack, M.VGG_LINKS, 4)],
                         ids=["mobilenet_swish", "vgg_gelu"])
def test_the_three_passes_compose_in_every_order(make, links, bns):
    """Every order of the three passes, then every order of the three undo functions: after each single call no code-writing wrapper
    stands in front of a stock module and every placeholder stands behind its owner's wrapper (M.intact, the defect of DESIGN
    section 40); after the last undo the tree is the original by identity."""
    passes = (link, use_device_bn_layerout_train, use_device_bn_train)
    undos = (fusion.unlink_layerout_codes_train, fusion.restore_bn_layerout_train, fusion.restore_bn_train)
    n = 0
    for apply in itertools.permutations(passes):
        for undo in itertools.permutations(undos):
            model = make().train()
            snap = _snapshot(model)
            for fn in apply + undo:
                fn(model)
                what = ([f.__name__ for f in apply], [f.__name__ for f in undo], fn.__name__)
                assert M.intact(model) is None, (M.intact(model), what)
                if fn is link:
                    wraps = [w for w in model.modules() if isinstance(w, fusion.TrainBatchNormLayeroutCodes2d)]
                    assert len(wraps) == links, what
                    lut_first = apply.index(use_device_bn_layerout_train) < apply.index(link)
                    assert all(w._fallback == ((True, 0) if lut_first else (False, None)) for w in wraps), what
            _assert_original(model, snap, what)
            n += 1
    assert n == 36
    # before and after use_device_bn_layerout_train: that pass takes every block the link has not taken, and the other way round
    model = make().train()
    assert fusion.link_layerout_codes_train(model, 0) == links and fusion.use_device_bn_layerout_train(model, 0) == bns - links
    model = make().train()
    assert fusion.use_device_bn_layerout_train(model, 0) == bns and fusion.link_layerout_codes_train(model, 0) == links
    assert fusion.restore_bn_layerout_train(model) == bns                  # takes the links along
    assert not any(isinstance(m, (fusion.FoldedTail, fusion.TrainBatchNormLayeroutCodes2d)) for m in model.modules())


def test_a_device_batchnorm_in_the_slot_is_taken_as_its_stock_module():
    """use_device_bn_train, the link, then the link's undo alone: the slot holds the stock BatchNorm2d, not the TrainBatchNorm2d
    that stood there (as after use_device_bn_layerout_train and its undo); the wrapper's fallback is ATen."""
    model = M.mobilenet_swish_stack().train()
    snap = _snapshot(model)
    assert fusion.use_device_bn_train(model, 0) == 5
    assert fusion.link_layerout_codes_train(model, 0) == M.MOBILENET_LINKS
    wraps = [w for w in model.modules() if isinstance(w, fusion.TrainBatchNormLayeroutCodes2d)]
    assert all(type(w._held[0]) is nn.BatchNorm2d and w._fallback == (False, None) for w in wraps)
    assert fusion.unlink_layerout_codes_train(model) == M.MOBILENET_LINKS
    kinds = [type(m).__name__ for m in model.modules() if isinstance(m, (nn.BatchNorm2d, fusion.TrainBatchNorm2d))]
    assert kinds == ["BatchNorm2d"] * 4 + ["TrainBatchNorm2d"]             # the four linked slots, then the one in front of the pool
    assert fusion.restore_bn_train(model) == 1
    _assert_original(model, snap)


def test_a_linked_cpu_model_computes_what_the_stock_modules_compute():
    """No device: every call falls back (F.batch_norm, the kept quantizer, the kept activation), in training and in eval mode."""
    torch.manual_seed(1)
    conv = cf.conv2d_Q_bias(32, 0.1, 0.2)
    model = M.spread(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.BatchNorm2d(8), layerout_quantize_func(8), af.Swish(), conv(8, 8, 1),
                                   nn.BatchNorm2d(8), layerout_quantize_func(8), nn.GELU(), conv(8, 8, 3, padding=1)))
    for i in (4, 8):
        model[i].q_bit = 8                                                 # candidates for the pass ...
    ref = copy.deepcopy(model)
    assert fusion.link_layerout_codes_train(model, min_elements=0) == 2
    for m in (model, ref):
        for i in (4, 8):
            m[i].q_bit = 32                                                # ... that compute with stock ATen on the CPU
    for lo in (model[1]._layerout, model[5]._layerout, ref[2], ref[6]):
        lo.q_bit = 32                                                      # (the layer-output quantizer has no CPU path either)
    assert isinstance(model[2], fusion.FoldedTail) and model[2].mod is model[1]._layerout
    x = torch.randn(4, 3, 6, 5)
    for training in (True, True, False):
        outs = []
        for m in (model, ref):
            m.train(training)
            m.zero_grad(set_to_none=True)
            y = m(x)
            if training:
                y.square().mean().backward()
            outs.append((y.detach(), [p.grad for p in m.parameters()]))
        assert torch.equal(outs[0][0], outs[1][0]) and bool(torch.isfinite(outs[0][0]).all())
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))
        for k, v in ref.state_dict().items():
            assert torch.equal(model.state_dict()[k], v), k
        assert model[1]._last_kernel == "aten" and model[5]._last_kernel == "aten"
    assert int(model[1].num_batches_tracked) == 2


def test_the_default_size_rule_follows_from_the_committed_measurement():
    """batchnorm.LUT_CODES_MIN_ELEMENTS admits exactly the size classes the spread rule admits in BOTH committed runs of
    profiles/bn_lut_codes_train_bench.py; None where no class passes."""
    runs = [json.load(open(os.path.join(HERE, "..", "profiles", name)))
            for name in ("bn_lut_codes_train_bench.json", "bn_lut_codes_train_bench_first.json")]
    classes = sorted({r["elements"] for r in runs[0]["handovers"]}, reverse=True)
    assert classes == sorted({r["elements"] for r in runs[1]["handovers"]}, reverse=True)
    admitted = []
    for e in classes:
        if not all(r["faster_beyond_spread"] for res in runs for r in res["handovers"] if r["elements"] == e):
            break
        admitted.append(e)
    floor = batchnorm.LUT_CODES_MIN_ELEMENTS
    if not admitted:
        assert floor is None
    else:
        assert floor is not None and [e for e in classes if e >= floor] == admitted
    for res in runs:
        for r in res["handovers"]:   # what a row claims is what its figures say
            other = r[r["better_unlinked_leg"] + "_ms"]
            assert other == min(r["stock_ms"], r["unlinked_ms"])
            assert r["faster_beyond_spread"] == (r["linked_ms"] < other * (1 - r[r["better_unlinked_leg"] + "_spread"]))
