"""GPU: training-mode BatchNorm2d (+ReLU) on csrc/bn_train.hip against float64 references computed on the CPU from the same float32
inputs with the textbook formulas.  Cases and bars: _bn_cases.py; test_bn_train_host.py checks on the CPU that
ATen's float32 batch_norm and a NumPy model of the kernel's order hold the statistics bars on these very inputs.
  statistics   mean: |d| <= 2 (M + 1) 2^-24 mean64(|x|); biased variance (from save_invstd): relative 1e-5; the running statistics
               after one and after three calls: the same two bars
  y, gx        max|d| <= 1e-5 max|ref| and ||d||_2 <= 1e-5 ||ref||_2; on the offset case (mu = 1000 sigma) against the centred
               magnitude ref - beta, since x - mean cancels
  ggamma, gbeta   |d| / sum|terms| <= 1e-5 elementwise, L2 <= 1e-6 (the bars of test_gpu_backward.py)
The ReLU mask of the backward reference is the kernel's own y > 0 (y is validated first), so no element is left out."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _bn_cases as B
from _bars import TOL_EXACT
from _bn_calls import _bars_ok, _bwd, _fwd, _sum_bars_ok
from cnns_slfp_quantization_amd import fusion, optimizer as O
from cnns_slfp_quantization_amd import conv2d_func as cf
from cnns_slfp_quantization_amd import layer_specs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("case", B.cases(), ids=B.case_id)
def test_forward_against_float64(case, relu):
    shape, offset = case
    d = B.inputs(shape, offset)
    x = d["x"]
    m = x.numel() // shape[3]
    mean64, var64, y64 = B.forward64(x, d["gamma"], d["beta"], relu)
    rm, rv = d["rm"].to(DEV), d["rv"].to(DEV)
    y, sm, si = _fwd(shape, d, relu, rm, rv)
    torch.cuda.synchronize()
    assert B.mean_bar_ok(sm.cpu().numpy(), mean64, x)
    var = 1.0 / si.cpu().double().numpy() ** 2 - B.EPS
    print("var rel", float((np.abs(var - var64) / var64).max()))
    assert B.var_bar_ok(var, var64, TOL_EXACT)
    # the stated order is the contract: the NumPy model of it gives save_mean's very bits
    km, _ = B.kernel_order_stats(x)
    assert np.array_equal(sm.cpu().numpy(), km.astype(np.float32))
    for calls in (1, 3):
        if calls == 3:
            _fwd(shape, d, relu, rm, rv)
            _fwd(shape, d, relu, rm, rv)
            torch.cuda.synchronize()
        rm64, rv64 = B.running64(d["rm"], d["rv"], mean64, var64, m, calls)
        assert B.mean_bar_ok(rm.cpu().numpy(), rm64, x), calls
        assert B.var_bar_ok(rv.cpu().double().numpy(), rv64, TOL_EXACT), calls
    got = B.rows(y.cpu())
    centred = None
    if offset:   # the bars against the centred magnitude: the pre-ReLU reference minus beta
        centred = B.forward64(x, d["gamma"], d["beta"], False)[2] - d["beta"].double().numpy()
    assert _bars_ok(got, y64, centred)
    if relu:
        assert bool((y >= 0).all())
    assert y.is_contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("case", B.cases(), ids=B.case_id)
def test_backward_against_float64(case, relu, sparse):
    shape, offset = case
    d = B.inputs(shape, offset)
    gy = d["gy_sparse" if sparse else "gy"]
    y, sm, si = _fwd(shape, d, relu)
    gx, gg, gb = _bwd(shape, d, relu, y, sm, si, gy)
    gx_only = _bwd(shape, d, relu, y, sm, si, gy, params=False)[0]   # gamma and beta frozen: the sums still run
    torch.cuda.synchronize()
    g = B.rows(gy)
    if relu:
        g = g * (B.rows(y.cpu()) > 0)
    gx64, gg64, gb64, agg, agb = B.backward64(d["x"], g, d["gamma"])
    for name, got, ref, terms in (("ggamma", gg, gg64, agg), ("gbeta", gb, gb64, agb)):
        assert _sum_bars_ok(name, got.cpu().numpy(), ref, terms), name
    assert _bars_ok(B.rows(gx.cpu()), gx64)
    assert torch.equal(gx_only, gx)


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("case", B.cases(), ids=B.case_id)
def test_results_are_the_stated_order_bit_for_bit(case, relu):
    """The orders of include/slfp.h are the contract: y, gx, ggamma and gbeta are the very bits of the float32 NumPy model of
    them (B.kernel_order_forward / kernel_order_backward), which is handed the device's save_mean and save_invstd (save_invstd
    stays under the variance bar above; the model does not repeat the device's float64 sqrt)."""
    shape, offset = case
    d = B.inputs(shape, offset)
    y, sm, si = _fwd(shape, d, relu)
    gx, gg, gb = _bwd(shape, d, relu, y, sm, si, d["gy"])
    torch.cuda.synchronize()
    sm, si = sm.cpu().numpy(), si.cpu().numpy()
    y = B.rows32(y.cpu())
    want_y = B.kernel_order_forward(d["x"], d["gamma"], d["beta"], sm, si, relu)
    want = B.kernel_order_backward(d["x"], d["gy"], y, d["gamma"], sm, si, relu)
    got = (B.rows32(gx.cpu()), gg.cpu().numpy(), gb.cpu().numpy())
    for name, a, b in zip(("y", "gx", "ggamma", "gbeta"), (y,) + got, (want_y,) + want):
        a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
        print(name, "differing elements", int((a.view(np.uint32) != b.view(np.uint32)).sum()), "of", a.size)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name


@pytest.mark.parametrize("case", [(B.ragged(32), False), (B.ragged(6), False), ((2, 3, 3, 1024), False)], ids=B.case_id)
def test_deterministic(case):
    shape, offset = case
    d = B.inputs(shape, offset)
    runs = []
    for _ in range(2):
        rm, rv = d["rm"].to(DEV), d["rv"].to(DEV)
        y, sm, si = _fwd(shape, d, True, rm, rv)
        runs.append((y, sm, si, rm, rv) + _bwd(shape, d, True, y, sm, si, d["gy"]))
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("shape", [(2, 5, 7, 32), B.ragged(32), (4, 9, 3, 58)], ids=lambda s: "x".join(map(str, s)))
def test_nan_and_inf_stay_in_their_channel(shape):
    """A NaN or an inf in x makes the BatchNorm output of its channel non-finite exactly where the stock module's is (all of
    it: the kernel gives NaN, MIOpen NaN or +-inf), and every other channel keeps its bits.  With the ReLU folded the kernel's
    NaN stays NaN; the stock pair turns the -inf that MIOpen writes on a +inf channel into 0, which is no property to copy."""
    d = B.inputs(shape, False)
    n, h, w, c = shape
    x = d["x"].clone()
    x[n - 1, 3, h - 1, w - 1] = float("nan")    # (the last slab of the ragged shape)
    x[0, 5, 0, 1] = float("inf")
    x[1, 2, 1, 0] = -float("inf")
    xd = x.to(DEV)
    stock = F.batch_norm(xd, None, None, d["gamma"].to(DEV), d["beta"].to(DEV), True, B.MOMENTUM, B.EPS)
    keep = [i for i in range(c) if i not in (2, 3, 5)]
    for relu in (False, True):
        clean = _fwd(shape, d, relu)[0]
        got = _fwd(shape, d, relu, x=xd)[0]
        torch.cuda.synchronize()
        assert torch.equal(torch.isfinite(got), torch.isfinite(stock)), relu
        assert not torch.isfinite(got[:, [2, 3, 5]]).any()
        assert torch.equal(got[:, keep], clean[:, keep])


def test_runs_on_the_current_stream():
    """The default stream is held by a sleep; a call on another stream completes meanwhile, with the same bits."""
    shape = B.ragged(32)
    d = B.inputs(shape, False)
    y0, sm0, si0 = _fwd(shape, d, True)
    gx0, gg0, gb0 = _bwd(shape, d, True, y0, sm0, si0, d["gy"])
    from test_gpu_headline import _sleep_cycles
    cycles = _sleep_cycles(200)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    held, done = torch.cuda.Event(), torch.cuda.Event()
    torch.cuda._sleep(cycles)               # 0.2 s on the default stream
    held.record()
    with torch.cuda.stream(side):
        y, sm, si = _fwd(shape, d, True)
        gx, gg, gb = _bwd(shape, d, True, y, sm, si, d["gy"])
        done.record()
    done.synchronize()
    still_held = not held.query()
    torch.cuda.synchronize()
    assert still_held, "the side stream's work waited for the default stream (or the sleep was too short to tell)"
    for a, b in zip((y, sm, si, gx, gg, gb), (y0, sm0, si0, gx0, gg0, gb0)):
        assert torch.equal(a, b)


def _stack():
    """[Conv2d_Q, BN, ReLU(inplace)] x 3 + pool + Linear_Q: the first three blocks of test_gpu_backward.py's fine-tune model
    (MobileNetV1-CIFAR), their ReLUs in place as the reference nets have them, and a 16-class head."""
    from test_gpu_backward import _finetune_model
    layers = [nn.ReLU(inplace=True) if isinstance(l, nn.ReLU) else l for l in _finetune_model()[:9]]
    fc = [r for r in layer_specs.nets()["mobilenetv1_cifar32"]["layers"] if r["kind"] == "linear"][0]
    layers += [nn.AdaptiveAvgPool2d(1), nn.Flatten(), cf.linear_Q(8, fc["Kw"], fc["Ka"])(64, 16)]
    return nn.Sequential(*layers)


def test_module_level_training_steps_match_the_stock_modules():
    """Three NormalSGD steps with options.backward = "hip".  The control-run rule of test_gpu_backward.py's fine-tune test: at
    every step the stock modules run first ON THE SAME WEIGHTS and BatchNorm state, then the swapped ones; the trajectories are
    never run apart.  After the first step every parameter gradient agrees to rtol 1e-4 with that test's atol (section 12's
    fine-tune bar); the losses of all three steps, which there are bit-identical because the forward is one path, here differ
    by the BN kernels' float32 rounding and are held to the same rtol 1e-4.  The later steps' gradients are printed, not
    asserted: the net is discontinuous in its activations (every Conv2d_Q quantizes its input, every ReLU masks by y > 0), and
    where a last-bit difference in a BatchNorm output moves one activation across a code boundary or across zero, a gradient
    changes by one whole term of its sum -- at the second step the first BatchNorm's weight gradient differed by 1.8 % of its
    largest element (one term among the 2048 of a channel's sum) and the stem's weight gradient by 4e-5 of its largest, at
    the third step every tensor agreed to 7.5e-5 again.  The losses of all three steps were equal to the last digit."""
    torch.manual_seed(0)
    prev = cf.options.backward
    cf.options.backward = "hip"
    try:
        m = _stack().to(DEV).to(memory_format=torch.channels_last).train()
        x = torch.randn(8, 3, 32, 32).to(DEV).contiguous(memory_format=torch.channels_last)
        tgt = torch.randint(0, 16, (8,)).to(DEV)
        loss_fn = nn.CrossEntropyLoss()
        names = [n for n, _ in m.named_parameters()]
        keys = list(m.state_dict().keys())
        opt = O.NormalSGD(m.parameters(), lr=1e-3, momentum=0.9)
        state = [b.clone() for b in m.buffers()]
        for step in range(3):
            grads, loss, after = {}, {}, {}
            for mode in ("stock", "swapped"):
                if mode == "swapped":
                    assert fusion.use_device_bn_train(m, min_elements=0) == 3   # (these tensors are below the measured rule)
                    assert list(m.state_dict().keys()) == keys
                for b, s in zip(m.buffers(), state):   # both passes see the same BatchNorm state
                    b.copy_(s)
                opt.zero_grad(set_to_none=True)
                out = loss_fn(m(x), tgt)
                out.backward()
                grads[mode] = [p.grad.detach().clone() for p in m.parameters()]
                loss[mode] = out.item()
                after[mode] = [b.clone() for b in m.buffers()]
                if mode == "swapped":
                    assert [m[i]._last_kernel for i in (1, 4, 7)] == ["bn_train+relu"] * 3
                    assert all(isinstance(m[i], fusion.FoldedReLU) for i in (2, 5, 8))
                    assert fusion.restore_bn_train(m) == 3
            print("step", step, loss)
            assert abs(loss["swapped"] - loss["stock"]) <= 1e-4 * abs(loss["stock"]), (step, loss)
            for n, a, b in zip(names, grads["swapped"], grads["stock"]):
                if step == 0:
                    atol = (1e-3 if a.dim() == 1 else 1e-5) * b.abs().max().item()
                    torch.testing.assert_close(a, b, rtol=1e-4, atol=atol, msg=lambda s, n=n: f"step 0, {n}: {s}")
                else:
                    print("step", step, n, "max|d| / max|ref|", ((a - b).abs().max() / b.abs().max()).item())
            for a, b in zip(after["swapped"], after["stock"]):   # running statistics and num_batches_tracked
                torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)
            state = after["swapped"]
            opt.step()   # with the swapped model's gradients (the same Parameter objects)
        m.eval()
        assert fusion.use_device_bn_train(m) == 3
        with torch.no_grad():
            y_swapped = m(x)
            assert m[1]._last_kernel == "aten"
            assert fusion.restore_bn_train(m) == 3
            assert torch.equal(y_swapped, m(x))
    finally:
        cf.options.backward = prev


def test_wrapper_falls_back_where_the_kernels_do_not_apply():
    big = nn.Sequential(nn.BatchNorm2d(64), nn.ReLU()).to(DEV).train()
    assert fusion.use_device_bn_train(big) == 1                       # the default: the measured rule, batchnorm.MIN_ELEMENTS
    xb = torch.randn(128, 64, 56, 56, device=DEV).contiguous(memory_format=torch.channels_last)   # 25.7 M elements
    want = torch.relu(F.batch_norm(xb, None, None, big[0].weight, big[0].bias, True, 0.1, big[0].eps))
    torch.testing.assert_close(big(xb), want, rtol=1e-5, atol=1e-5)
    assert big[0]._last_kernel == "bn_train+relu"
    big(xb[:64])                                                      # 12.8 M elements: not reliably faster than stock
    assert big[0]._last_kernel == "aten"
    bn = nn.BatchNorm2d(8).to(DEV).train()
    seq = nn.Sequential(bn, nn.ReLU())
    assert fusion.use_device_bn_train(seq, min_elements=0) == 1
    wrap = seq[0]
    x = torch.randn(4, 8, 5, 5, device=DEV)
    seq(x)                                                            # contiguous NCHW: not built
    assert wrap._last_kernel == "aten"
    seq(x.contiguous(memory_format=torch.channels_last))
    assert wrap._last_kernel == "bn_train+relu"
    with torch.autocast("cuda", dtype=torch.float16):
        seq(x.contiguous(memory_format=torch.channels_last))
    assert wrap._last_kernel == "aten"
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        seq(torch.randn(1, 8, 1, 1, device=DEV))
    assert int(wrap.num_batches_tracked) == 4
    # running statistics that are not float32 on x's device are not handed to the kernels (they write float32): the call does
    # what a stock module holding the same buffers does -- equal output and buffers, or an exception of the same type
    stock = nn.BatchNorm2d(8).to(DEV).train()
    stock.load_state_dict(wrap.state_dict())
    for mod in (wrap, stock):
        mod.running_mean, mod.running_var = mod.running_mean.double(), mod.running_var.double()
    xc = x.contiguous(memory_format=torch.channels_last)
    outs = []
    for mod, tail in ((seq, lambda t: t), (stock, torch.relu)):
        try:
            outs.append(tail(mod(xc)))
        except Exception as e:   # whatever ATen says to such buffers, both say it
            outs.append(type(e))
    assert wrap._last_kernel == "aten"
    assert outs[0] is outs[1] if isinstance(outs[1], type) else torch.equal(outs[0], outs[1])
    for name in ("running_mean", "running_var", "num_batches_tracked"):
        a, b = getattr(wrap, name), getattr(stock, name)
        assert a.dtype == b.dtype and torch.equal(a, b), name
    # parameters that are misaligned views (a flat parameter buffer) are copied for the call, not refused
    flat = torch.randn(17, device=DEV)
    bn.weight = nn.Parameter(flat[1:9])
    bn.bias = nn.Parameter(flat[9:17])
    view = nn.Sequential(bn, nn.ReLU())
    assert bn.weight.data_ptr() % 16 != 0 and fusion.use_device_bn_train(view, min_elements=0) == 1
    xc = x.contiguous(memory_format=torch.channels_last)
    want = torch.relu(F.batch_norm(xc, None, None, bn.weight, bn.bias, True, 0.1, bn.eps))
    out = view(xc)
    assert view[0]._last_kernel == "bn_train+relu"
    torch.testing.assert_close(out, want, rtol=1e-5, atol=1e-5)
    out.sum().backward()
    assert bn.weight.grad is not None and bool(torch.isfinite(bn.weight.grad).all())


class _Residual(nn.Module):
    """A hand-wired block as nets_imgnet/resnet50.py writes it: the BatchNorms sit in named slots, one nn.ReLU(inplace=True) is
    shared, and the last BatchNorm's output is changed in place by `out += identity`."""

    def __init__(self, c):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(c, c, 1, bias=False), nn.BatchNorm2d(c)
        self.conv2, self.bn2 = nn.Conv2d(c, c, 3, padding=1, bias=False), nn.BatchNorm2d(c)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        out += identity
        return self.relu(out)


def test_hand_wired_block_with_in_place_readers_trains_like_stock():
    """Without a folded ReLU the backward does not read the BatchNorm's output, so it is not saved: a shared in-place ReLU and
    `out += identity` behind the swapped module must leave .backward() working, as behind the stock one.  Forward, input and
    parameter gradients against the stock modules (plain float32 convolutions, nothing discontinuous): rtol 1e-4, atol 1e-5 of
    the largest element -- ten times the kernels' own 1e-5 bars, for the two convolutions and the second BatchNorm in between."""
    torch.manual_seed(4)
    blk = _Residual(16).to(DEV).to(memory_format=torch.channels_last).train()
    x = torch.randn(4, 16, 9, 7, device=DEV).contiguous(memory_format=torch.channels_last)
    gy = torch.randn(4, 16, 9, 7, device=DEV).contiguous(memory_format=torch.channels_last)
    state = [b.clone() for b in blk.buffers()]
    res = {}
    for mode in ("stock", "swapped"):
        if mode == "swapped":
            assert fusion.use_device_bn_train(blk, min_elements=0) == 2
            assert type(blk.relu) is nn.ReLU and not blk.bn1._relu and not blk.bn2._relu
        for b, s in zip(blk.buffers(), state):
            b.copy_(s)
        blk.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        out = blk(xi)
        out.backward(gy)
        res[mode] = [out.detach().clone(), xi.grad.clone()] + [p.grad.clone() for p in blk.parameters()]
    assert blk.bn1._last_kernel == "bn_train" and blk.bn2._last_kernel == "bn_train"
    assert fusion.restore_bn_train(blk) == 2
    for a, b in zip(res["swapped"], res["stock"]):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5 * b.abs().max().item())
