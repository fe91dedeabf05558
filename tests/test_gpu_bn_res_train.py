"""GPU: training-mode BatchNorm2d -> residual add -> ReLU on the residual forms of csrc/bn_train.hip.  The
contract of include/slfp.h is a composition, and it is exact:
  forward    save_mean, save_invstd, running statistics = slfp_bn_train_fwd's; y = where(z < 0, 0, z), z = y_plain(relu = 0) + res
  backward   gx, ggamma, gbeta = slfp_bn_train_bwd(relu) given the same x, y, gy; gres = where(y > 0, gy, 0)
all compared bit for bit (as int32, so a NaN compares by its bits), then against float64 with the bars of test_gpu_bn_train.py.
Cases: _bn_cases.py; res = randn from a seeded generator, so max|z| is of the order of max|t|.  The module-level tests run
hand-wired Bottlenecks (_bn_res_blocks.py) through fusion.use_device_bottleneck_train."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import _bn_cases as B
import _bn_res_blocks as R
from _bars import TOL_EXACT
from _bn_calls import _bars_ok, _bits, _bwd as _plain_bwd, _fwd as _plain_fwd, _res_bwd, _res_fwd, _same
from cnns_slfp_quantization_amd import batchnorm, fusion

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@functools.lru_cache(None)
def _res(shape):
    """The residual operand of a case (CPU, channels_last).  Cached: the tests share it and must not write to it."""
    n, h, w, c = shape
    g = torch.Generator().manual_seed(2000 + sum(shape))
    return torch.randn(n, c, h, w, generator=g).contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("case", B.cases(), ids=B.case_id)
def test_forward_and_backward_are_the_composition(case, relu):
    shape, offset = case
    d = B.inputs(shape, offset)
    res = _res(shape).to(DEV)
    rm0, rv0, rm1, rv1 = d["rm"].to(DEV), d["rv"].to(DEV), d["rm"].to(DEV), d["rv"].to(DEV)
    t, sm0, si0 = _plain_fwd(shape, d, False, rm0, rv0)
    y, sm, si = _res_fwd(shape, d, relu, res, rm1, rv1)
    torch.cuda.synchronize()
    for a, b in ((sm, sm0), (si, si0), (rm1, rm0), (rv1, rv0)):
        assert _same(a, b)
    z = t + res                                                       # float32, one add
    assert _same(y, torch.where(z < 0, torch.zeros_like(z), z) if relu else z)
    assert y.is_contiguous(memory_format=torch.channels_last)
    for key in ("gy", "gy_sparse"):
        gy = d[key].to(DEV)
        want = _plain_bwd(shape, d, relu, y, sm0, si0, gy)
        gx, gres, gg, gb = _res_bwd(shape, d, relu, y, sm, si, gy)
        no_gres = _res_bwd(shape, d, relu, y, sm, si, gy, gres=False)
        no_params = _res_bwd(shape, d, relu, y, sm, si, gy, params=False)
        gx_only = _res_bwd(shape, d, relu, y, sm, si, gy, gres=False, params=False)
        torch.cuda.synchronize()
        for name, a, b in zip(("gx", "ggamma", "gbeta"), (gx, gg, gb), want):
            assert _same(a, b), (key, name)
        assert _same(gres, torch.where(y > 0, gy, torch.zeros_like(gy)) if relu else gy), key
        assert _same(no_gres[0], gx) and _same(no_gres[2], gg) and _same(no_gres[3], gb), key
        assert _same(no_params[0], gx) and _same(no_params[1], gres), key
        assert _same(gx_only[0], gx), key


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("case", B.cases(), ids=B.case_id)
def test_forward_against_float64(case, relu):
    """max|d| <= 1e-5 max(max|t64|, max|z64|) and ||d|| <= 1e-5 ||y64||: the add contributes one rounding of z, so the plain
    kernel's bars carry over."""
    shape, offset = case
    d = B.inputs(shape, offset)
    res = _res(shape)
    y = _res_fwd(shape, d, relu, res.to(DEV))[0]
    torch.cuda.synchronize()
    t64 = B.forward64(d["x"], d["gamma"], d["beta"], False)[2]
    z64 = t64 + B.rows(res)
    y64 = np.maximum(z64, 0.0) if relu else z64
    dd = B.rows(y.cpu()) - y64
    e = float(np.abs(dd).max() / max(np.abs(t64).max(), np.abs(z64).max()))
    l2 = float(np.linalg.norm(dd) / np.linalg.norm(y64))
    print("max", e, "l2", l2)
    assert e <= TOL_EXACT and l2 <= TOL_EXACT
    if relu:
        assert bool((y >= 0).all())


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("case", B.cases(), ids=B.case_id)
def test_backward_against_float64(case, relu, sparse):
    """The measures and bars of test_gpu_bn_train.py; the ReLU mask of the reference is the kernel's own y > 0 (y is validated by
    the two tests above).  gres against the float64 masked gy is exact."""
    shape, offset = case
    d = B.inputs(shape, offset)
    gy = d["gy_sparse" if sparse else "gy"]
    y, sm, si = _res_fwd(shape, d, relu, _res(shape).to(DEV))
    gx, gres, gg, gb = _res_bwd(shape, d, relu, y, sm, si, gy)
    torch.cuda.synchronize()
    g = B.rows(gy)
    if relu:
        g = g * (B.rows(y.cpu()) > 0)
    gx64, gg64, gb64, agg, agb = B.backward64(d["x"], g, d["gamma"])
    for name, got, ref, terms in (("ggamma", gg, gg64, agg), ("gbeta", gb, gb64, agb)):
        dd = np.abs(got.cpu().double().numpy() - ref)
        assert (dd[terms == 0] == 0).all(), name
        elem = float((dd[terms > 0] / terms[terms > 0]).max()) if (terms > 0).any() else 0.0
        l2 = float(np.linalg.norm(dd) / max(np.linalg.norm(ref), 1e-300))
        print(name, "elem", elem, "l2", l2)
        assert elem <= 1e-5 and l2 <= 1e-6, (name, elem, l2)
    assert _bars_ok(B.rows(gx.cpu()), gx64)
    assert np.array_equal(B.rows(gres.cpu()), g)


@pytest.mark.parametrize("case", [(B.ragged(32), False), (B.ragged(6), False), ((2, 3, 3, 1024), False)], ids=B.case_id)
def test_deterministic(case):
    shape, offset = case
    d = B.inputs(shape, offset)
    res = _res(shape).to(DEV)
    runs = []
    for _ in range(2):
        rm, rv = d["rm"].to(DEV), d["rv"].to(DEV)
        y, sm, si = _res_fwd(shape, d, True, res, rm, rv)
        runs.append((y, sm, si, rm, rv) + _res_bwd(shape, d, True, y, sm, si, d["gy"]))
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert _same(a, b)


@pytest.mark.parametrize("shape", [(2, 5, 7, 32), B.ragged(32), (4, 9, 3, 58)], ids=lambda s: "x".join(map(str, s)))
def test_nan_and_inf_in_res_stay_in_their_element(shape):
    d = B.inputs(shape, False)
    n, h, w, c = shape
    gy = d["gy"].to(DEV)
    spots = {"nan": (n - 1, 3, h - 1, w - 1), "+inf": (0, 5, 0, 1), "-inf": (1, 2, 1, 0)}   # (nan: the last slab of the ragged shape)
    bad = _res(shape).clone()
    bad[spots["nan"]], bad[spots["+inf"]], bad[spots["-inf"]] = float("nan"), float("inf"), -float("inf")
    out = []
    for r in (_res(shape).to(DEV), bad.to(DEV)):
        y, sm, si = _res_fwd(shape, d, True, r)
        out.append((y,) + _res_bwd(shape, d, True, y, sm, si, gy))
    torch.cuda.synchronize()
    (y0, gx0, gr0, gg0, gb0), (y1, gx1, gr1, gg1, gb1) = out
    hit = torch.zeros(n, c, h, w, dtype=torch.bool, device=DEV)
    for s in spots.values():
        hit[s] = True
    assert torch.equal(_bits(y1)[~hit], _bits(y0)[~hit]) and torch.equal(_bits(gr1)[~hit], _bits(gr0)[~hit])
    assert bool(torch.isnan(y1[spots["nan"]])) and float(y1[spots["+inf"]]) == float("inf") and float(y1[spots["-inf"]]) == 0.0
    assert float(gr1[spots["nan"]]) == 0.0 and float(gr1[spots["-inf"]]) == 0.0       # y > 0 is false for a NaN
    assert float(gr1[spots["+inf"]]) == float(gy[spots["+inf"]])
    keep = [i for i in range(c) if i not in (2, 3, 5)]
    assert _same(gx1[:, keep], gx0[:, keep]) and _same(gg1[keep], gg0[keep]) and _same(gb1[keep], gb0[keep])
    assert bool(torch.isfinite(gx1).all()) and bool(torch.isfinite(gg1).all())        # the statistics never saw res


@pytest.mark.parametrize("shape", [(2, 5, 7, 32), B.ragged(32), (4, 9, 3, 58)], ids=lambda s: "x".join(map(str, s)))
def test_nan_in_x_stays_in_its_channel(shape):
    """As the plain kernels: the channel's statistics are NaN, so all of it is; every other channel keeps its bits."""
    d = B.inputs(shape, False)
    n, h, w, c = shape
    res, gy = _res(shape).to(DEV), d["gy"].to(DEV)
    x = d["x"].clone()
    x[n - 1, 3, h - 1, w - 1] = float("nan")
    out = []
    for xi in (d["x"].to(DEV), x.to(DEV)):
        y, sm, si = _res_fwd(shape, d, True, res, x=xi)
        out.append((y,) + _res_bwd(shape, d, True, y, sm, si, gy, x=xi))
    torch.cuda.synchronize()
    (y0, gx0, gr0, gg0, gb0), (y1, gx1, gr1, gg1, gb1) = out
    keep = [i for i in range(c) if i != 3]
    assert bool(torch.isnan(y1[:, 3]).all())
    assert bool((gr1[:, 3] == 0).all())                               # y > 0 is false everywhere in the channel
    for a, b in ((y1, y0), (gx1, gx0), (gr1, gr0)):
        assert _same(a[:, keep], b[:, keep])
    assert _same(gg1[keep], gg0[keep]) and _same(gb1[keep], gb0[keep])


def test_runs_on_the_current_stream():
    """The default stream is held by a sleep; a call on another stream completes meanwhile, with the same bits."""
    shape = B.ragged(32)
    d = {k: v.to(DEV) for k, v in B.inputs(shape, False).items()}    # on the device beforehand: the side stream copies nothing
    res = _res(shape).to(DEV)

    def run():
        y, sm, si = _res_fwd(shape, d, True, res)
        return (y, sm, si) + _res_bwd(shape, d, True, y, sm, si, d["gy"])

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


def _on_device(m):
    return m.to(DEV).to(memory_format=torch.channels_last).train()


def _step(model, x):
    model.zero_grad(set_to_none=True)
    xi = x.clone().requires_grad_(True)                               # (keeps x's memory format)
    out = model(xi)
    loss = out.square().mean()
    loss.backward()
    torch.cuda.synchronize()
    grads = [torch.zeros((), device=x.device) if p.grad is None else p.grad.detach().clone() for p in model.parameters()]
    return dict(out=out.detach().clone(), loss=loss.detach().clone(), gx=xi.grad.clone(), grads=grads,
                buffers=[b.clone() for b in model.buffers()])


def _bns(blk):
    return [blk.bn1, blk.bn2, blk.bn3]


@pytest.fixture
def deterministic_convs():
    """MIOpen's deterministic algorithms for the duration of a test that compares nn.Conv2d weight gradients exactly."""
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = prev


def test_module_level_training_step_is_exact(deterministic_convs):
    """P: use_device_bn_train alone (bn_train kernels, then ATen's add and ReLU).  Q: the block pass, then use_device_bn_train for
    the downsample's BatchNorm.  The only difference is which kernel applies the add and the ReLU, both exact operations, so
    after one training step everything is torch.equal (+0 and -0 compare equal).  Against the fully stock model: the bars of
    test_hand_wired_block_with_in_place_readers_trains_like_stock.
    The convolutions are plain nn.Conv2d, and MIOpen's default weight-gradient kernels add with atomics: two runs of the fully
    stock model on the same input gave conv weight gradients 0.5e-7 to 1.3e-7 of their largest element apart, with every
    convolution's input and incoming gradient bit-identical.  An exact comparison needs an exact instrument, so the test asks
    MIOpen for its deterministic algorithms (the fixture: torch.backends.cudnn.deterministic) for its duration; with them two runs
    of one model are torch.equal."""
    x = R.example().to(DEV).contiguous(memory_format=torch.channels_last)
    P, Q, S = (_on_device(R.stack()) for _ in range(3))              # the same seed: the same weights three times
    keys = list(S.state_dict().keys())
    assert fusion.use_device_bn_train(P, min_elements=0) == 7
    assert fusion.use_device_bottleneck_train(Q, x, min_elements=0) == 2
    assert fusion.use_device_bn_train(Q, min_elements=0) == 1
    assert list(Q.state_dict().keys()) == keys and Q.training and all(m.training for m in Q.modules())
    for a, b in zip(Q.state_dict().values(), S.state_dict().values()):
        assert torch.equal(a, b)                                      # the verification updated nothing
    p, q, s = _step(P, x), _step(Q, x), _step(S, x)
    for blk in Q:
        assert [bn._last_kernel for bn in _bns(blk)] == ["bn_train+relu", "bn_train+relu", "bn_res_train+relu"]
    assert Q[0].downsample[1]._last_kernel == "bn_train"
    for blk in P:
        assert [bn._last_kernel for bn in _bns(blk)] == ["bn_train"] * 3
    assert torch.equal(q["out"], p["out"]) and torch.equal(q["loss"], p["loss"]) and torch.equal(q["gx"], p["gx"])
    for (name, _), a, b in zip(S.named_parameters(), q["grads"], p["grads"]):
        assert torch.equal(a, b), name
    for (name, _), a, b in zip(S.named_buffers(), q["buffers"], p["buffers"]):
        assert torch.equal(a, b), name
    for name, a, b in [("out", q["out"], s["out"]), ("gx", q["gx"], s["gx"])] + [
            (n, a, b) for (n, _), a, b in zip(S.named_parameters(), q["grads"], s["grads"])]:
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5 * b.abs().max().item(), msg=lambda m, n=name: f"{n}: {m}")
    for a, b in zip(q["buffers"], s["buffers"]):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


def test_look_alikes_are_left_alone():
    model, ref = _on_device(R.mixed()), _on_device(R.mixed())
    before = dict(model.named_modules())
    keys = list(model.state_dict().keys())
    x = R.example32().to(DEV).contiguous(memory_format=torch.channels_last)
    assert fusion.use_device_bottleneck_train(model, x, min_elements=0) == 1
    assert ["forward" in b.__dict__ for b in model] == [False, True, False, False]
    for i in (0, 2, 3):
        assert all(getattr(model[i], k) is before[f"{i}.{k}"] for k in ("bn1", "bn2", "bn3"))
    model(x)
    assert model[1].bn3._last_kernel == "bn_res_train+relu"
    assert fusion.restore_bottleneck_train(model) == 1
    assert dict(model.named_modules()) == before and list(model.state_dict().keys()) == keys
    ref.load_state_dict(model.state_dict())                           # (the training forward above moved the statistics)
    model.eval(), ref.eval()
    with torch.no_grad():
        assert torch.equal(model(x), ref(x))
    # restore_bn_train on a rewritten model leaves it runnable and stock
    model.train()
    assert fusion.use_device_bottleneck_train(model, x, min_elements=0) == 1
    assert fusion.use_device_bn_train(model, min_elements=0) == 9
    fusion.restore_bn_train(model)
    assert dict(model.named_modules()) == before and not any("forward" in b.__dict__ for b in model)
    model.eval()
    with torch.no_grad():
        assert torch.equal(model(x), ref(x))


def test_wrapper_falls_back_where_the_kernels_do_not_apply(deterministic_convs):
    """Where the kernels do not run, the module computes what the stock block computes, with the same ATen calls: everything is
    torch.equal (the convolutions on MIOpen's deterministic algorithms, see above)."""
    torch.manual_seed(8)
    blk = R.randomize(R.Bottleneck(32, 8, 32))
    x = R.example32().to(DEV)

    def pair(min_elements, fmt=torch.channels_last, dtype=torch.float32):
        m = nn.Sequential(copy.deepcopy(blk)).to(DEV, dtype).to(memory_format=fmt).train()
        ref = copy.deepcopy(m)
        xi = x.to(dtype).contiguous(memory_format=fmt)
        assert fusion.use_device_bottleneck_train(m, xi, min_elements=min_elements) == 1
        return m, ref, xi

    m, ref, xc = pair(0)
    m(xc)
    assert [bn._last_kernel for bn in _bns(m[0])] == ["bn_train+relu", "bn_train+relu", "bn_res_train+relu"]
    ref.load_state_dict(m.state_dict())
    m.eval(), ref.eval()
    with torch.no_grad():
        assert torch.equal(m(xc), ref(xc))                            # eval mode
    assert [bn._last_kernel for bn in _bns(m[0])] == ["aten"] * 3
    cases = {"under min_elements": pair(None), "NCHW": pair(0, fmt=torch.contiguous_format), "float64": pair(0, dtype=torch.float64)}
    assert xc.numel() < batchnorm.RES_MIN_ELEMENTS and xc.numel() < batchnorm.MIN_ELEMENTS
    for name, (m, ref, xi) in cases.items():
        a, b = _step(m, xi), _step(ref, xi)
        assert [bn._last_kernel for bn in _bns(m[0])] == ["aten"] * 3, name
        assert torch.equal(a["out"], b["out"]) and torch.equal(a["gx"], b["gx"]), name
        for u, v in zip(a["grads"] + a["buffers"], b["grads"] + b["buffers"]):
            assert torch.equal(u, v), name
    m, ref, xi = pair(0)
    with torch.autocast("cuda", dtype=torch.float16):
        m(xi)
    assert m[0].bn3._last_kernel == "aten"
