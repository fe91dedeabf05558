"""CPU: the host side of a QAT step on 1-byte codes.  The code forms of training-mode BatchNorm2d (+ReLU),
slfp_bn_codes_train_supported / _fwd / _bwd of csrc/bn_train.hip, and slfp_conv2d_bwd_codes of csrc/conv_bwd.hip: the exports, the
supported sets and every refusal, all before any device work (fake pointers, no device).  fusion.link_codes_train /
unlink_codes_train on models built on the CPU."""
import copy
import ctypes
import os
import re
import sys

import pytest
import torch
import torch.nn as nn

import _bn_res_blocks as R
from cnns_slfp_quantization_amd import _lib, batchnorm, fusion, layer_specs
from cnns_slfp_quantization_amd import conv2d_func as cf

NEW = ("slfp_bn_codes_train_supported", "slfp_bn_codes_train_fwd", "slfp_bn_codes_train_bwd", "slfp_conv2d_bwd_codes_supported",
       "slfp_conv2d_bwd_codes")
NHWC, NCHW = _lib.LAYOUT_NHWC, _lib.LAYOUT_NCHW
KA = 2.6023073196411133 / 15.5   # a Ka of the reference's MobileNetV1


def test_new_symbols_are_exported_bound_and_declared():
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "slfp.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert hasattr(L, name)
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    doc = header[header.index("the code forms"):]
    for text in ("save_lo[c] = f32(mean - save_mean)", "SLFP_FMT_EXT", "A NaN takes code 0x00", "t > 0 ? gy : 0",
                 "no forward output is read", "ggamma and gbeta may be NULL", "No atomics", "one dword", "not measured"):
        assert text in doc, text
    assert L.slfp_version() == 1   # new exports only


def _sup(shape=(2, 5, 7, 64), layout=NHWC, ka=KA, qbits=8):
    return _lib.load().slfp_bn_codes_train_supported(*shape, layout, ka, qbits)


def test_supported_set():
    L = _lib.load()
    for qbits in (8, 7):
        assert L.slfp_enc_table_ok(KA, _lib.FMT_SFP7 if qbits == 7 else _lib.FMT_ACT8) == 1
        for shape in ((2, 5, 7, 32), (3, 1, 1, 64), (2, 3, 3, 1024), (0, 5, 7, 64), (128, 112, 112, 32)):
            assert L.slfp_bn_train_supported(*shape, NHWC) == 1
            assert _sup(shape, qbits=qbits) == 1, shape
    assert _sup((4, 9, 3, 58)) == 0 and L.slfp_bn_train_supported(4, 9, 3, 58, NHWC) == 1   # c % 4 != 0
    assert _sup((5, 7, 3, 6)) == 0
    assert _sup((1, 1, 1, 64)) == 0                                                         # what the plain form refuses
    assert _sup(layout=NCHW) == 0
    for qbits in (32, 0, 6, 9, -8):
        assert _sup(qbits=qbits) == 0, qbits
    for ka in (0.0, -KA, float("nan"), float("inf"), 1e-38):
        assert _sup(ka=ka) == 0, ka


def _fwd(x=16, gamma=16, beta=16, rm=None, rv=None, relu=1, ka=KA, qbits=8, y=36, sm=16, si=16, lo=16, shape=(2, 5, 7, 64),
         layout=NHWC, ws=16, ws_bytes=1 << 30):
    return _lib.load().slfp_bn_codes_train_fwd(x, gamma, beta, rm, rv, 0.1, 1e-5, relu, ka, qbits, y, sm, si, lo, *shape, layout, ws,
                                               ws_bytes, None)


def _bwd(x=16, gy=48, gamma=16, beta=16, sm=16, si=16, lo=16, relu=1, gx=64, gg=None, gb=None, shape=(2, 5, 7, 64), layout=NHWC,
         ws=16, ws_bytes=1 << 30):
    return _lib.load().slfp_bn_codes_train_bwd(x, gy, gamma, beta, sm, si, lo, relu, gx, gg, gb, *shape, layout, ws, ws_bytes, None)


def test_refused_before_any_device_work():
    # the pointers are never dereferenced and no launch is made: every refusal comes first (this machine may have no GPU)
    need = _lib.load().slfp_bn_train_workspace_bytes(2, 5, 7, 64)
    for call, names in ((_fwd, ("x", "gamma", "beta", "y", "sm", "si", "lo")), (_bwd, ("x", "gy", "gamma", "beta", "sm", "si", "lo", "gx"))):
        for name in names:
            assert call(**{name: None}) == _lib.ERR_BAD_ARG, name
            assert "null pointer" in _lib.last_error()
        assert call(lo=24) == _lib.ERR_ALIGNMENT
        assert call(layout=NCHW) == _lib.ERR_UNSUPPORTED
        assert "slfp_bn_train_supported" in _lib.last_error()
        assert call(shape=(1, 1, 1, 64)) == _lib.ERR_UNSUPPORTED             # M == 1
        assert call(shape=(4, 9, 3, 58)) == _lib.ERR_UNSUPPORTED             # c % 4 != 0
        assert "slfp_bn_codes_train_supported" in _lib.last_error()
        assert call(shape=(5, 7, 3, 6)) == _lib.ERR_UNSUPPORTED
        assert call(layout=7) == _lib.ERR_BAD_ARG
        assert call(relu=2) == _lib.ERR_BAD_ARG
        assert call(shape=(2, 0, 7, 64)) == _lib.ERR_SHAPE
        assert call(x=24) == _lib.ERR_ALIGNMENT
        assert call(ws_bytes=need - 1) == _lib.ERR_BAD_ARG and "workspace" in _lib.last_error()
        assert call(ws=None) == _lib.ERR_BAD_ARG
        assert call(ws=24) == _lib.ERR_BAD_ARG
        assert call(shape=(0, 5, 7, 64), ws=None, ws_bytes=0) == _lib.OK     # n == 0: nothing to do
        # the order of slfp_bn_train_fwd / _bwd: null pointers, the layout, the geometry, what is unsupported, alignment, workspace
        assert call(lo=None, layout=NCHW, ws_bytes=0) == _lib.ERR_BAD_ARG
        assert call(layout=7, shape=(2, 0, 7, 64)) == _lib.ERR_BAD_ARG
        assert call(shape=(2, 0, 7, 58), x=24) == _lib.ERR_SHAPE
        assert call(layout=NCHW, x=24, ws_bytes=0) == _lib.ERR_UNSUPPORTED
        assert call(shape=(4, 9, 3, 58), x=20, ws_bytes=0) == _lib.ERR_UNSUPPORTED
        assert call(x=24, ws_bytes=0) == _lib.ERR_ALIGNMENT
    # the forward's own: the reader's quantizer, y_codes and the running statistics
    for kw in (dict(qbits=32), dict(qbits=0), dict(ka=0.0), dict(ka=-KA), dict(ka=float("nan"))):
        assert _fwd(**kw) == _lib.ERR_UNSUPPORTED, kw
        assert "slfp_bn_codes_train_supported" in _lib.last_error()
        assert _fwd(x=24, ws_bytes=0, **kw) == _lib.ERR_UNSUPPORTED          # ... before alignment and the workspace
        assert _fwd(x=None, **kw) == _lib.ERR_BAD_ARG                        # ... behind the null pointers
    for y in (33, 34, 35, 37):
        assert _fwd(y=y) == _lib.ERR_ALIGNMENT and "y_codes" in _lib.last_error()
        assert _fwd(y=y, ws_bytes=0) == _lib.ERR_ALIGNMENT                   # before the workspace
    assert _fwd(y=36, ws_bytes=0) == _lib.ERR_BAD_ARG                        # 4 bytes are enough for y_codes
    assert _fwd(y=16) == _lib.ERR_BAD_ARG and "alias" in _lib.last_error()
    assert _bwd(gx=16) == _lib.ERR_BAD_ARG and "alias" in _lib.last_error()
    assert _fwd(rm=16) == _lib.ERR_BAD_ARG                                    # running_mean without running_var
    assert _fwd(rm=18, rv=16) == _lib.ERR_ALIGNMENT
    assert _bwd(gg=18) == _lib.ERR_ALIGNMENT


# ---- slfp_conv2d_bwd_codes ----------------------------------------------------------------------------------------------------
DENSE = _lib.BWD_DENSE


def _desc(spec, n=2, x_layout=_lib.LAYOUT_NHWC, y_layout=_lib.LAYOUT_NHWC, qbits=8):
    return _lib.ConvDesc(n=n, c_in=spec.c_in, h=spec.h, w=spec.w, c_out=spec.c_out, kh=spec.k[0], kw=spec.k[1],
                         stride_h=spec.stride[0], stride_w=spec.stride[1], pad_h=spec.pad[0], pad_w=spec.pad[1],
                         dil_h=1, dil_w=1, groups=spec.groups, x_layout=x_layout, y_layout=y_layout, qbits=qbits,
                         ka=float(spec.Ka), kw_scale=float(spec.Kw), mfma_passes=0, reserved=0)


@pytest.mark.parametrize("net", sorted(layer_specs.nets()))
def test_conv_bwd_codes_supported_is_the_ex_query_on_nhwc_dword_layers(net):
    L = _lib.load()
    seen = set()
    for spec in layer_specs.conv_layers(net):
        for flags in (0, DENSE):
            for qbits in (8, 7):
                d = _desc(spec, qbits=qbits)
                ex = L.slfp_conv2d_bwd_supported_ex(ctypes.byref(d), flags)
                got = L.slfp_conv2d_bwd_codes_supported(ctypes.byref(d), flags)
                assert got == (ex if spec.c_in % 4 == 0 else 0), (spec, flags)
                seen.add((got, spec.c_in % 4 == 0))
            nchw = _desc(spec, x_layout=_lib.LAYOUT_NCHW)
            assert L.slfp_conv2d_bwd_codes_supported(ctypes.byref(nchw), flags) == 0
            # gy may still arrive NCHW: only x is codes
            assert L.slfp_conv2d_bwd_codes_supported(ctypes.byref(_desc(spec, y_layout=_lib.LAYOUT_NCHW)), flags) == \
                L.slfp_conv2d_bwd_codes_supported(ctypes.byref(_desc(spec)), flags)
    assert (1, True) in seen and (0, False) in seen   # every net has a C_in = 3 stem and layers the kernels take


def _dense_spec(c_in=16):
    return layer_specs.ConvSpec(c_in, 32, (3, 3), (1, 1), (1, 1), 1, False, 14, 14, 14, 14, 0.2, 0.1)


def test_conv_bwd_codes_refusals_and_the_unknown_flags():
    L = _lib.load()
    fake = 1 << 20                                                   # 16-byte aligned, never touched
    ok = _desc(_dense_spec())
    r = ctypes.byref(ok)
    bwd = L.slfp_conv2d_bwd_codes
    assert L.slfp_conv2d_bwd_codes_supported(r, DENSE) == 1 and L.slfp_conv2d_bwd_codes_supported(r, 0) == 0
    assert L.slfp_conv2d_bwd_codes_supported(None, DENSE) == 0
    for flags in (2, DENSE | 2, 1 << 31):                            # new entry points, not a flag bit
        assert not L.slfp_conv2d_bwd_codes_supported(r, flags)
        assert bwd(r, flags, fake, fake, fake, fake, fake, None, fake, None) == _lib.ERR_BAD_ARG and "flag" in _lib.last_error()
        assert not L.slfp_conv2d_bwd_supported_ex(r, flags)          # ... and flag value 2 is still unknown to the _ex functions
        assert L.slfp_conv2d_bwd_kernel_name_ex(r, flags) == b"composite"
        assert L.slfp_conv2d_bwd_workspace_bytes_ex(r, flags, 1, 1) == 0
        assert L.slfp_conv2d_bwd_ex(r, flags, fake, fake, fake, fake, fake, None, fake, None) == _lib.ERR_BAD_ARG
    assert bwd(None, DENSE, fake, fake, fake, fake, fake, None, fake, None) == _lib.ERR_BAD_ARG
    assert bwd(r, 0, fake, fake, fake, fake, fake, None, fake, None) == _lib.ERR_UNSUPPORTED       # what _ex refuses
    for bad in (_desc(_dense_spec(), x_layout=_lib.LAYOUT_NCHW), _desc(_dense_spec(c_in=6)), _desc(_dense_spec(c_in=3))):
        assert L.slfp_conv2d_bwd_supported_ex(ctypes.byref(bad), DENSE) == 1
        assert L.slfp_conv2d_bwd_codes_supported(ctypes.byref(bad), DENSE) == 0
        assert bwd(ctypes.byref(bad), DENSE, fake, fake, fake, fake, fake, None, fake, None) == _lib.ERR_UNSUPPORTED
        assert "x_codes" in _lib.last_error()
    assert bwd(r, DENSE, fake, fake, None, fake, fake, None, fake, None) == _lib.ERR_BAD_ARG       # no gy
    assert bwd(r, DENSE, None, fake, fake, None, fake, None, fake, None) == _lib.ERR_BAD_ARG       # gw, no x_codes
    assert bwd(r, DENSE, fake, fake, fake, None, None, fake, fake, None) == _lib.ERR_BAD_ARG       # gb, no gw
    for off in (1, 2, 3):
        assert bwd(r, DENSE, fake + off, fake, fake, fake, fake, None, fake, None) == _lib.ERR_ALIGNMENT
        assert "x_codes" in _lib.last_error()
    assert bwd(r, DENSE, fake + 4, fake, fake, fake, fake, None, None, None) == _lib.ERR_BAD_ARG   # 4 bytes are enough for x_codes
    assert "workspace" in _lib.last_error()
    assert bwd(r, DENSE, fake, fake + 4, fake, fake, fake, None, fake, None) == _lib.ERR_ALIGNMENT
    assert bwd(r, DENSE, fake, fake, fake, None, None, None, None, None) == _lib.OK                # nothing requested


# ---- fusion.link_codes_train on models built on the CPU -------------------------------------------------------------------------
def _mobilenet():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import netgen
    scales = [(r["Ka"], r["Kw"]) for r in layer_specs.nets()["mobilenetv1_cifar32"]["layers"]]
    return netgen.fill_parameters(netgen.build_mobilenetv1_cifar(cf.conv2d_Q, cf.linear_Q, 8, scales))


def _convs(model):
    return [m for m in model.modules() if fusion._is_conv_q(m)]


def test_link_finds_the_26_hand_overs_of_mobilenetv1_and_unlink_restores_the_objects():
    model = _mobilenet()
    before = dict(model.named_modules())
    keys = list(model.state_dict().keys())
    ids = [id(p) for p in model.parameters()]
    want = {k: v.clone() for k, v in model.state_dict().items()}
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    assert fusion.link_codes_train(model) == 26
    assert fusion.link_codes_train(model) == 0                             # nothing left to take
    wraps = [m for m in model.modules() if isinstance(m, fusion.TrainBatchNormCodes2d)]
    convs = _convs(model)
    assert len(wraps) == 26 and len(convs) == 27
    assert [w._conv for w in wraps] == convs[1:]                           # a block's last ReLU meets the next block's first conv
    assert all(w._ka == cf._f32(c.Ka) and w._q_bit == 8 and w.min_elements is None for w, c in zip(wraps, convs[1:]))
    seq = model.model
    assert isinstance(seq[0][1], fusion.TrainBatchNormCodes2d) and isinstance(seq[0][2], fusion.FoldedReLU)
    assert seq[0][1]._held == (before["model.0.1"], before["model.0.2"]) and seq[0][2].relu is before["model.0.2"]
    assert isinstance(seq[13][1], fusion.TrainBatchNormCodes2d) and seq[13][4] is before["model.13.4"]   # behind the last conv: a pool
    assert not seq[0][1]._modules                                          # the held modules and the conv sit outside _modules
    assert list(model.state_dict().keys()) == keys
    assert [id(p) for p in model.parameters()] == ids
    assert all(a is b for a, b in zip(opt.param_groups[0]["params"], model.parameters()))
    for k, v in want.items():
        assert torch.equal(model.state_dict()[k], v), k
    model.double()                                                         # buffers are replaced by a cast: unlink re-points them
    assert fusion.unlink_codes_train(model) == 26
    assert dict(model.named_modules()) == before                           # the very same module objects
    assert seq[0][1].running_mean.dtype == torch.float64 and seq[0][1].running_mean is model.state_dict(keep_vars=True)["model.0.1.running_mean"]
    assert fusion.unlink_codes_train(model) == 0


def test_link_leaves_hand_wired_blocks_and_ineligible_runs_alone():
    assert fusion.link_codes_train(R.stack()) == 0                         # Bottlenecks: hand-wired, and plain nn.Conv2d
    conv = cf.conv2d_Q_bias(8, 0.1, 0.2)
    raw = cf.conv2d_Q(8, 0.1, 0.2)
    shared = nn.ReLU()

    def run(bn=None, relu=None, c=None):
        return [bn or nn.BatchNorm2d(8), relu or nn.ReLU(inplace=True), c or conv(8, 8, 1)]

    fused = conv(8, 8, 1); fused._post = (None, None, 1)
    coded = conv(8, 8, 1); coded._code_out = (0.2, 8)
    conv2 = conv(8, 8, 3, padding=1)
    m = nn.Sequential(*run(), *run(c=conv2),                                        # 0..5: two links (a scaled bias is fine)
                      *run(bn=nn.BatchNorm2d(8, affine=False)), *run(bn=nn.BatchNorm2d(8, momentum=None)),
                      *run(relu=nn.ReLU6()), *run(c=raw(8, 8, 1, bias=True)), *run(c=cf.conv2d_Q(32, 0.1, 0.2)(8, 8, 1)),
                      *run(c=fused), *run(c=coded), *run(relu=shared), *run(relu=shared), *run(c=nn.Conv2d(8, 8, 1)),
                      nn.BatchNorm2d(8), nn.Identity(), nn.ReLU(), conv(8, 8, 1),   # not adjacent
                      *run(c=raw(8, 8, 1)))                                          # conv2d_Q without a bias: a link
    before = dict(m.named_modules())
    assert fusion.link_codes_train(m, min_elements=0) == 3
    taken = [i for i, c in enumerate(m) if isinstance(c, fusion.TrainBatchNormCodes2d)]
    assert taken == [0, 3, len(m) - 3] and m[3]._conv is conv2 and m[0].min_elements == 0
    assert fusion.unlink_codes_train(m) == 3 and dict(m.named_modules()) == before


def test_a_nested_sequential_held_twice_is_left_alone():
    """A block in two slots of the root runs in front of two different convs: its last BN + ReLU has no single reader."""
    conv = cf.conv2d_Q_bias(8, 0.1, 0.2)
    twice = nn.Sequential(conv(8, 8, 1), nn.BatchNorm2d(8), nn.ReLU())
    m = nn.Sequential(twice, conv(8, 8, 1), twice, conv(8, 8, 3, padding=1), nn.BatchNorm2d(8), nn.ReLU(), conv(8, 8, 1))
    before = dict(m.named_modules())
    assert fusion.link_codes_train(m, min_elements=0) == 1                 # the run behind the block alone
    assert isinstance(m[4], fusion.TrainBatchNormCodes2d) and m[4]._conv is m[6]
    assert twice[1] is before["0.1"] and twice[2] is before["0.2"]
    inner = nn.Sequential(nn.BatchNorm2d(8), nn.ReLU(), conv(8, 8, 1))      # a whole run inside a block held twice: one successor each,
    assert fusion.link_codes_train(nn.Sequential(inner, inner), min_elements=0) == 0   # but not taken either
    assert fusion.unlink_codes_train(m) == 1 and dict(m.named_modules()) == before


def _small(seed=3):
    torch.manual_seed(seed)
    conv = cf.conv2d_Q_bias(32, 0.1, 0.2)   # q_bit 32: stock ATen on the CPU; never linked, so the BN in front is a plain swap
    m = nn.Sequential(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.BatchNorm2d(8), nn.ReLU(inplace=True)),
                      nn.Sequential(cf.conv2d_Q(8, 0.1, 0.2)(8, 8, 1), nn.BatchNorm2d(8), nn.ReLU(inplace=True),
                                    conv(8, 8, 1), nn.BatchNorm2d(8), nn.ReLU()))
    return R.randomize(m)


@pytest.mark.parametrize("order", ["link_first", "bn_train_first"])
def test_either_order_with_use_device_bn_train(order):
    model = _small()
    before = dict(model.named_modules())
    if order == "link_first":
        assert fusion.link_codes_train(model) == 1
        assert fusion.use_device_bn_train(model) == 2                      # the linked BN is no candidate any more
    else:
        assert fusion.use_device_bn_train(model, min_elements=5) == 3
        assert fusion.link_codes_train(model) == 1
    wrap = model[0][1]
    assert isinstance(wrap, fusion.TrainBatchNormCodes2d) and wrap._conv is model[1][0] and isinstance(model[0][2], fusion.FoldedReLU)
    assert wrap._fallback == ((True, 5) if order == "bn_train_first" else (False, None))
    assert isinstance(model[1][1], fusion.TrainBatchNorm2d) and isinstance(model[1][4], fusion.TrainBatchNorm2d)
    if order == "link_first":
        assert fusion.unlink_codes_train(model) == 1 and fusion.restore_bn_train(model) == 2
    else:
        assert fusion.restore_bn_train(model) == 3                         # takes the links along
    assert dict(model.named_modules()) == before


def test_a_linked_cpu_model_computes_what_the_stock_modules_compute():
    """No device: every call falls back (F.batch_norm + ReLU), in training and in eval mode, through two optimizer steps."""
    torch.manual_seed(1)
    conv = cf.conv2d_Q_bias(32, 0.1, 0.2)
    model = R.randomize(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.BatchNorm2d(8), nn.ReLU(inplace=True), conv(8, 8, 1)))
    model[3].q_bit = 8                                                     # a candidate for the pass ...
    ref = copy.deepcopy(model)
    assert fusion.link_codes_train(model, min_elements=0) == 1
    model[3].q_bit = ref[3].q_bit = 32                                     # ... that computes with stock ATen on the CPU
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
        assert torch.equal(outs[0][0], outs[1][0])
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))
        for k, v in ref.state_dict().items():
            assert torch.equal(model.state_dict()[k], v), k
        assert model[1]._last_kernel == "aten"
    assert int(model[1].num_batches_tracked) == 2


def test_the_default_size_rule_follows_from_the_committed_measurement():
    """batchnorm.CODES_MIN_ELEMENTS admits exactly the size classes the spread rule admits in profiles/bn_codes_train_bench.json."""
    import json
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bn_codes_train_bench.json")
    res = json.load(open(path))
    rows = res["handovers"]
    assert sum(r["layers"] for r in rows) == 26
    classes = sorted({r["elements"] for r in rows}, reverse=True)
    admitted = []
    for e in classes:
        if not all(r["faster_beyond_spread"] for r in rows if r["elements"] == e):
            break
        admitted.append(e)
    assert admitted and res["rule"]["codes_min_elements_by_the_spread_rule"] == admitted[-1]
    floor = batchnorm.CODES_MIN_ELEMENTS
    assert [e for e in classes if e >= floor] == admitted
    for r in rows:   # what a row claims is what its figures say
        other = r[r["better_unlinked_leg"] + "_ms"]
        assert other == min(r["stock_ms"], r["unlinked_ms"])
        assert r["faster_beyond_spread"] == (r["linked_ms"] < other * (1 - r[r["better_unlinked_leg"] + "_spread"]))
