"""GPU: training-mode BatchNorm2d -> layer-output quantizer -> activation on the table forms of csrc/bn_train.hip (DESIGN section
32).  The contract of include/slfp.h is a composition, and it is exact:
  forward    save_mean, save_invstd, running statistics = slfp_bn_train_fwd's; y = F[class of slfp_quantize_layerout_f32(y_plain)]
  backward   gx, ggamma, gbeta = slfp_bn_train_bwd(relu = 0) fed g = gy * D[class], computed by torch in float32
all compared bit for bit (as int32, so a NaN compares by its bits).  F, D: batchnorm.layerout_act_tables.  Cases: _bn_cases.py."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import _bn_cases as B
from _bars import TOL_EXACT
from test_bn_layerout_train_host import CLOSED
from _bn_calls import _bars_ok, _bits, _bwd as _plain_bwd, _fwd as _plain_fwd, _lut_bwd, _lut_fwd, _same, _stream
from cnns_slfp_quantization_amd import _lib, activation_func as af, batchnorm, fusion
from cnns_slfp_quantization_amd import conv2d_func as cf
from cnns_slfp_quantization_amd import layer_specs
from cnns_slfp_quantization_amd.sfp_quant import layerout_quantize_func

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ACTS = {"relu": nn.ReLU, "swish": af.Swish, "gelu": nn.GELU}
NT = _lib.LAYEROUT_TABLE_FLOATS
_cache = {}


def _values():
    """slfp_layerout_lut_values (CPU float32, NT entries) and the number of classes."""
    if "values" not in _cache:
        vals = np.zeros(NT, dtype=np.float32)
        _lib.check(_lib.load().slfp_layerout_lut_values(vals.ctypes.data, NT))
        _cache["values"] = (torch.from_numpy(vals), _lib.load().slfp_layerout_lut_classes())
    return _cache["values"]


def _tables(name):
    if name not in _cache:
        _cache[name] = batchnorm.layerout_act_tables([ACTS[name]()], DEV)
    return _cache[name]


def _quantize(t):
    q = torch.empty_like(t)
    _lib.check(_lib.load().slfp_quantize_layerout_f32(t.data_ptr(), q.data_ptr(), t.numel(), _stream()))
    return q


def _classes(q):
    """The class index of every element of a quantizer output `q`, found through slfp_layerout_lut_values; NaN is class 0."""
    vals, ncls = _values()
    sbits, order = _bits(vals[1:ncls]).to(DEV).sort()
    qb = _bits(q).flatten()
    pos = torch.searchsorted(sbits, qb).clamp_max(sbits.numel() - 1)
    hit = sbits[pos] == qb
    assert bool((hit | torch.isnan(q).flatten()).all()), "a value outside the quantizer's image"
    return torch.where(hit, order[pos] + 1, torch.zeros_like(pos)).view(q.shape)


def _dev(d):
    return d["x"].to(DEV), d["gamma"].to(DEV), d["beta"].to(DEV)


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("case", B.cases(), ids=B.case_id)
def test_forward_and_backward_are_the_composition(case, act):
    shape, offset = case
    d = B.inputs(shape, offset)
    ftab, dtab = _tables(act)
    x, gamma, beta = _dev(d)
    rm0, rv0, rm1, rv1 = d["rm"].to(DEV), d["rv"].to(DEV), d["rm"].to(DEV), d["rv"].to(DEV)
    y_plain, sm0, si0 = _plain_fwd(shape, d, False, rm0, rv0)
    y, sm, si, lo = _lut_fwd(shape, ftab, x, gamma, beta, rm1, rv1)
    torch.cuda.synchronize()
    for a, b in ((sm, sm0), (si, si0), (rm1, rm0), (rv1, rv0)):
        assert torch.equal(a, b)
    # lo = f32(mean - save_mean): at most half a unit in the last place of save_mean
    assert bool((lo.abs().double() <= sm.abs().double() * 2.0 ** -24 + 1e-45).all())
    cls = _classes(_quantize(y_plain))
    assert _same(y, ftab[cls])
    assert y.is_contiguous(memory_format=torch.channels_last)
    for key in ("gy", "gy_sparse"):
        gy = d[key].to(DEV)
        g = gy * dtab[cls]                                            # float32, one multiply
        want = _plain_bwd(shape, d, False, y_plain, sm0, si0, g)
        got = _lut_bwd(shape, dtab, x, gy, gamma, beta, sm, si, lo)
        gx_only = _lut_bwd(shape, dtab, x, gy, gamma, beta, sm, si, lo, params=False)[0]   # ggamma / gbeta NULL
        torch.cuda.synchronize()
        for name, a, b in zip(("gx", "ggamma", "gbeta"), got, want):
            assert _same(a, b), (key, name)
        assert _same(gx_only, got[0]), key


@pytest.mark.parametrize("act", list(ACTS))
def test_every_class(act):
    """gamma = 0 makes t = +-0 + beta = beta exactly: one channel per class, then channels whose beta lies off the grid."""
    from oracle import slfp_oracle
    vals, ncls = _values()
    ftab, _ = _tables(act)
    shape = (2, 1, 1, NT)
    x = torch.randn(2, NT, 1, 1, generator=torch.Generator().manual_seed(11)).to(DEV).contiguous(memory_format=torch.channels_last)
    y = _lut_fwd(shape, ftab, x, torch.zeros(NT, device=DEV), vals.to(DEV))[0]
    torch.cuda.synchronize()
    got = _bits(y).view(2, NT)
    fb = _bits(ftab)
    for r in range(2):
        assert torch.equal(got[r, 1:ncls], fb[1:ncls])              # every class with a nonzero value: both signs, the
        assert bool((got[r, ncls:] == fb[0]).all())                   # denormals, +-248; beta = 0: the NaN class
        assert int(got[r, 0]) == int(fb[0])                           # beta = NaN
    off = np.array([2.0 ** -8 * 1.01, -(2.0 ** -8) * 1.01, 300.0, -300.0, 1e-40, -1e-40, 1.03, 0.0, 247.9, 2.0 ** -8, 3e-39, -1e-44],
                   dtype=np.float32)
    want_q = torch.from_numpy(slfp_oracle.layerout(off))
    cls = _classes(want_q.to(DEV))
    assert int(cls[7]) == 0 and float(want_q[2]) == 248.0 and float(want_q[3]) == -248.0
    shape = (2, 1, 1, off.size)
    x = torch.randn(2, off.size, 1, 1, generator=torch.Generator().manual_seed(12)).to(DEV).contiguous(memory_format=torch.channels_last)
    y = _lut_fwd(shape, ftab, x, torch.zeros(off.size, device=DEV), torch.from_numpy(off).to(DEV))[0]
    torch.cuda.synchronize()
    for r in range(2):
        assert torch.equal(_bits(y).view(2, -1)[r], fb[cls]), r


@pytest.mark.parametrize("act", ["swish", "gelu", "relu"])
@pytest.mark.parametrize("shape", [B.ragged(32), B.ragged(6)], ids=lambda s: "x".join(map(str, s)))
def test_backward_against_float64(shape, act):
    """gx, ggamma, gbeta against _bn_cases.backward64 fed gy * D64[class], D64 the closed-form float64 derivative at the class
    value: TOL_EXACT of max|ref| and of the L2 norm, the bars of test_gpu_bn_train.py."""
    d = B.inputs(shape, False)
    vals, ncls = _values()
    ftab, dtab = _tables(act)
    x, gamma, beta = _dev(d)
    y, sm, si, lo = _lut_fwd(shape, ftab, x, gamma, beta)
    gx, gg, gb = _lut_bwd(shape, dtab, x, d["gy"].to(DEV), gamma, beta, sm, si, lo)
    cls = _classes(_quantize(_plain_fwd(shape, d, False)[0])).cpu()
    torch.cuda.synchronize()
    assert int((cls == 0).sum()) == 0
    d64 = torch.zeros(NT, dtype=torch.float64)
    d64[1:ncls] = CLOSED[act][1](vals[1:ncls].double())
    g64 = B.rows(d["gy"]) * B.rows(d64[cls])
    gx64, gg64, gb64, _, _ = B.backward64(d["x"], g64, d["gamma"])
    assert _bars_ok(B.rows(gx.cpu()), gx64)
    assert _bars_ok(gg.cpu().double().numpy(), gg64)
    assert _bars_ok(gb.cpu().double().numpy(), gb64)


@pytest.mark.parametrize("case", [(B.ragged(32), False), (B.ragged(6), False), ((2, 3, 3, 1024), False)], ids=B.case_id)
def test_deterministic(case):
    shape, offset = case
    d = B.inputs(shape, offset)
    ftab, dtab = _tables("swish")
    x, gamma, beta = _dev(d)
    gy = d["gy"].to(DEV)
    runs = []
    for _ in range(2):
        rm, rv = d["rm"].to(DEV), d["rv"].to(DEV)
        y, sm, si, lo = _lut_fwd(shape, ftab, x, gamma, beta, rm, rv)
        runs.append((y, sm, si, lo, rm, rv) + _lut_bwd(shape, dtab, x, gy, gamma, beta, sm, si, lo))
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert _same(a, b)


@pytest.mark.parametrize("shape", [(2, 5, 7, 32), B.ragged(32), (4, 9, 3, 58)], ids=lambda s: "x".join(map(str, s)))
def test_nan_and_inf_stay_in_their_channel(shape):
    d = B.inputs(shape, False)
    n, h, w, c = shape
    ftab, dtab = _tables("gelu")
    x, gamma, beta = _dev(d)
    gy = d["gy"].to(DEV)
    bad = d["x"].clone()
    bad[n - 1, 3, h - 1, w - 1] = float("nan")    # (the last slab of the ragged shape)
    bad[0, 5, 0, 1] = float("inf")
    bad[1, 2, 1, 0] = -float("inf")
    bad = bad.to(DEV)
    keep = [i for i in range(c) if i not in (2, 3, 5)]
    res = []
    for xi in (x, bad):
        y, sm, si, lo = _lut_fwd(shape, ftab, xi, gamma, beta)
        res.append((y,) + _lut_bwd(shape, dtab, xi, gy, gamma, beta, sm, si, lo))
    torch.cuda.synchronize()
    (y0, gx0, gg0, gb0), (y1, gx1, gg1, gb1) = res
    assert _same(y1[:, keep], y0[:, keep]) and _same(gx1[:, keep], gx0[:, keep])
    assert _same(gg1[keep], gg0[keep]) and _same(gb1[keep], gb0[keep])
    assert bool(torch.isnan(y1[:, [2, 3, 5]]).all())                  # the statistics are NaN: every value is the NaN class


def test_runs_on_the_current_stream():
    """The default stream is held by a sleep; a call on another stream completes meanwhile, with the same bits."""
    shape = B.ragged(32)
    d = B.inputs(shape, False)
    ftab, dtab = _tables("swish")
    x, gamma, beta = _dev(d)
    gy = d["gy"].to(DEV)

    def run():
        y, sm, si, lo = _lut_fwd(shape, ftab, x, gamma, beta)
        return (y, sm, si, lo) + _lut_bwd(shape, dtab, x, gy, gamma, beta, sm, si, lo)

    want = run()
    from test_gpu_headline import _sleep_cycles
    cycles = _sleep_cycles(200)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    held, done = torch.cuda.Event(), torch.cuda.Event()
    torch.cuda._sleep(cycles)               # 0.2 s on the default stream
    held.record()
    with torch.cuda.stream(side):
        got = run()
        done.record()
    done.synchronize()
    still_held = not held.query()
    torch.cuda.synchronize()
    assert still_held, "the side stream's work waited for the default stream (or the sleep was too short to tell)"
    for a, b in zip(got, want):
        assert _same(a, b)


def _stack(acts):
    """[Conv2d_Q, BN, layerout_quantize_func(8), act] x 3 + pool + Linear_Q: the first three layers of test_gpu_backward.py's
    fine-tune model (MobileNetV1-CIFAR) with the tail of the `_swish` / `_gelu` nets, and a 16-class head."""
    from test_gpu_backward import _finetune_model
    stock = _finetune_model()
    layers = []
    for i, act in enumerate(acts):
        layers += [stock[3 * i], stock[3 * i + 1], layerout_quantize_func(8), act]
    fc = [r for r in layer_specs.nets()["mobilenetv1_cifar32"]["layers"] if r["kind"] == "linear"][0]
    layers += [nn.AdaptiveAvgPool2d(1), nn.Flatten(), cf.linear_Q(8, fc["Kw"], fc["Ka"])(64, 16)]
    return nn.Sequential(*layers)


def test_module_level_training_step_matches_the_unfused_kernels():
    """One training step with options.backward = "hip".  The reference is the same model with use_device_bn_train(min_elements=0)
    and the stock quantizer and activation modules: the same BatchNorm bits, so no value crosses a quantizer step, and outputs
    and loss are torch.equal.  The gradients differ only by gy * D[class] against ATen's own activation backward: TOL_EXACT of
    max|ref| per tensor.  Against the fully stock model (MIOpen's BatchNorm) the distances are printed, not asserted: a last-bit
    difference in a BatchNorm output moves a value across a quantizer step."""
    prev = cf.options.backward
    cf.options.backward = "hip"
    try:
        models = {}
        for k in ("lut", "unfused", "stock"):                         # the same initial weights three times
            torch.manual_seed(0)
            models[k] = _stack([af.Swish(), nn.GELU(), nn.ReLU(inplace=True)]).to(DEV).to(memory_format=torch.channels_last).train()
        base = models["stock"]
        x = torch.randn(8, 3, 32, 32).to(DEV).contiguous(memory_format=torch.channels_last)
        tgt = torch.randint(0, 16, (8,)).to(DEV)
        loss_fn = nn.CrossEntropyLoss()
        keys = list(base.state_dict().keys())
        assert fusion.use_device_bn_layerout_train(models["lut"], min_elements=0) == 3
        assert fusion.use_device_bn_train(models["unfused"], min_elements=0) == 3
        assert list(models["lut"].state_dict().keys()) == keys
        res = {}
        taps = {k: [] for k in models}
        for k, m in models.items():
            hooks = [m[i].register_forward_hook(lambda mod, inp, out, k=k: taps[k].append(out.detach().clone())) for i in (3, 7, 11)]
            out = m(x)
            loss = loss_fn(out, tgt)
            loss.backward()
            for hk in hooks:
                hk.remove()
            res[k] = (out.detach(), loss.detach(), [p.grad.detach().clone() for p in m.parameters()], [b.clone() for b in m.buffers()])
        torch.cuda.synchronize()
        assert [models["lut"][i]._last_kernel for i in (1, 5, 9)] == ["bn_lut_train"] * 3
        assert [models["unfused"][i]._last_kernel for i in (1, 5, 9)] == ["bn_train"] * 3
        assert all(isinstance(models["lut"][i], fusion.FoldedTail) for i in (2, 3, 6, 7, 10, 11))
        for a, b in zip(taps["lut"], taps["unfused"]):
            assert _same(a, b)
        assert torch.equal(res["lut"][0], res["unfused"][0]) and torch.equal(res["lut"][1], res["unfused"][1])
        for a, b in zip(res["lut"][3], res["unfused"][3]):            # running statistics and num_batches_tracked
            assert torch.equal(a, b)
        for (name, _), a, b in zip(base.named_parameters(), res["lut"][2], res["unfused"][2]):
            e = ((a - b).abs().max() / b.abs().max()).item()
            print("vs unfused", name, "max|d| / max|ref|", e)
            assert e <= TOL_EXACT, (name, e)
        for a, b in zip(taps["lut"], taps["stock"]):
            print("vs stock: fraction of block outputs that differ", (_bits(a) != _bits(b)).float().mean().item())
        print("vs stock: loss", res["lut"][1].item(), res["stock"][1].item())
        for (name, _), a, b in zip(base.named_parameters(), res["lut"][2], res["stock"][2]):
            print("vs stock", name, "max|d| / max|ref|", ((a - b).abs().max() / b.abs().max()).item())
        m = models["lut"]
        assert fusion.restore_bn_layerout_train(m) == 3 and list(m.state_dict().keys()) == keys
        assert type(m[1]) is nn.BatchNorm2d and type(m[3]) is af.Swish
    finally:
        cf.options.backward = prev


def test_wrapper_falls_back_where_the_kernels_do_not_apply():
    seq = nn.Sequential(nn.BatchNorm2d(8), layerout_quantize_func(8), nn.GELU()).to(DEV).train()
    ref = nn.Sequential(nn.BatchNorm2d(8), layerout_quantize_func(8), nn.GELU()).to(DEV).train()
    assert fusion.use_device_bn_layerout_train(seq, min_elements=0) == 1
    wrap = seq[0]
    x = torch.randn(4, 8, 5, 5, device=DEV)
    assert _same(seq(x), ref(x)) and wrap._last_kernel == "aten"     # contiguous NCHW: not built
    xc = x.contiguous(memory_format=torch.channels_last)
    y = seq(xc)
    assert wrap._last_kernel == "bn_lut_train" and y.shape == xc.shape
    seq.eval(), ref.eval()
    ref.load_state_dict(seq.state_dict())
    assert _same(seq(xc), ref(xc)) and wrap._last_kernel == "aten"
    seq.train()
    default = nn.Sequential(nn.BatchNorm2d(8), layerout_quantize_func(8), nn.GELU()).to(DEV).train()
    assert fusion.use_device_bn_layerout_train(default) == 1
    small = torch.randn(2, 8, 3, 3, device=DEV).contiguous(memory_format=torch.channels_last)
    if small.numel() < batchnorm.LUT_MIN_ELEMENTS:
        default(small)
        assert default[0]._last_kernel == "aten"
    # y is not saved: an in-place change behind the module leaves the backward working
    xi = xc.clone().requires_grad_(True)
    out = seq(xi)
    out += 1.0
    out.sum().backward()
    assert xi.grad is not None and bool(torch.isfinite(xi.grad).all()) and wrap.weight.grad is not None


def test_a_move_between_the_two_passes_keeps_the_arrays_on_the_device():
    """use_device_bn_train on the CPU model, .to(device) (which replaces the buffers on the wrapper alone), then this pass: the
    new module registers the wrapper's device tensors and runs the kernels.  And a module whose running statistics are NOT on the
    input's device never takes the kernel path (it would hand the kernels host addresses): it goes where the stock module goes."""
    seq = nn.Sequential(nn.BatchNorm2d(8), layerout_quantize_func(8), nn.GELU()).train()
    assert fusion.use_device_bn_train(seq, min_elements=0) == 1
    seq.to(DEV)
    assert fusion.use_device_bn_layerout_train(seq, min_elements=0) == 1
    wrap = seq[0]
    sd = seq.state_dict(keep_vars=True)
    for key in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked"):
        t = getattr(wrap, key)
        assert t.is_cuda and t is sd["0." + key] and getattr(wrap._bn, key) is t, key
    x = torch.randn(4, 8, 5, 5, device=DEV).contiguous(memory_format=torch.channels_last)
    y = seq(x)
    torch.cuda.synchronize()
    assert wrap._last_kernel == "bn_lut_train" and bool(torch.isfinite(y).all()) and int(wrap.num_batches_tracked) == 1
    assert not torch.equal(wrap.running_mean, torch.zeros(8, device=DEV))
    wrap._buffers["running_mean"] = wrap.running_mean.cpu()
    with pytest.raises(RuntimeError):                                 # ATen's own device check, as on the stock module
        seq(x)
    assert wrap._last_kernel == "aten"
