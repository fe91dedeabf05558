"""GPU: the fused multi-tensor step of DSGD / SSGD / NormalSGD (slfp_sgd_step_f32) against the reference's recorded
outputs and against the ATen composite of the same step on the same device, bit for bit."""
import copy

import numpy as np
import pytest
import torch

from conftest import GOLDEN, same_bits
from cnns_slfp_quantization_amd import optimizer as O
from cnns_slfp_quantization_amd.conv2d_func import conv2d_Q_bias, linear_Q

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _fused_default():
    O.options.fused = True
    yield
    O.options.fused = True


def _golden():
    return np.load(f"{GOLDEN}/optim_golden.npz")


def _cases():
    z = _golden()
    return sorted({k.rsplit("_p_s", 1)[0] for k in z.files if "_p_s" in k})


@pytest.mark.parametrize("case", _cases())
def test_fused_matches_reference_fixture(case):
    z = _golden()
    rule, q, m = case.split("_")
    q, m = int(q[1:]), int(m[1:]) / 10
    lr = float(z["lr"])
    p = torch.nn.Parameter(torch.from_numpy(z["p0"].copy()).to(DEV))
    opt = O.NormalSGD([p], lr=lr, momentum=m) if rule == "NormalSGD" else getattr(O, rule)([p], q, lr=lr, momentum=m)
    for k in (1, 2, 3):
        p.grad = torch.from_numpy(z[f"g{k}"].copy()).to(DEV)
        opt.step()
        assert same_bits(p.detach().cpu().numpy(), z[f"{case}_p_s{k}"]), (case, k)
        assert same_bits(p.grad.cpu().numpy(), z[f"grad_s{k}"]), (case, k)
        if m:
            assert same_bits(opt.state[p]["momentum_buffer"].cpu().numpy(), z[f"{case}_buf_s{k}"]), (case, k)


def _values(n, gen, scale):
    v = torch.randn(n, generator=gen) * scale
    special = torch.tensor([0.0, -0.0, 1e-45, -1e-40, 0.0625, -0.0625, 0.125, 15.32165, -15.0, 1e-10, np.nan, np.inf, -np.inf])
    k = min(n // 7, special.numel())
    if k:
        idx = torch.randperm(n, generator=gen)[:k]
        v[idx] = special[:k]
    return v


def _tensor_set(gen):
    """(param storage, grad storage) pairs: sizes 1 .. 3 M, views at a 1-float storage offset, channels_last weights, and
    300 small tensors (more than one launch takes)."""
    out = []
    for n in (1, 3, 5, 1023, 4097, 3 * 1024 * 1024 + 7):
        out.append((_values(n, gen, 0.5), _values(n, gen, 0.01)))
    for n in (4096, 1023):   # misaligned views
        pb, gb = _values(n + 1, gen, 0.5), _values(n + 1, gen, 0.01)
        out.append((pb, gb, 1))
    for shape in ((64, 32, 3, 3), (8, 3, 5, 5)):
        p = _values(int(np.prod(shape)), gen, 0.5).view(shape)
        g = _values(int(np.prod(shape)), gen, 0.01).view(shape)
        out.append((p, g, "cl"))
    for i in range(300):
        n = 1 + (i * 37) % 200
        out.append((_values(n, gen, 0.5), _values(n, gen, 0.01)))
    return out


def _make_params(spec):
    ps, gs = [], []
    for item in spec:
        p, g = item[0].to(DEV), item[1].to(DEV)
        if len(item) == 3 and item[2] == 1:
            p, g = p[1:], g[1:]
        elif len(item) == 3 and item[2] == "cl":
            p, g = p.contiguous(memory_format=torch.channels_last), g.contiguous(memory_format=torch.channels_last)
        ps.append(torch.nn.Parameter(p))
        gs.append(g)
    return ps, gs


def _build(rule, q, ps, **hp):
    return O.NormalSGD(ps, **hp) if rule == "NormalSGD" else getattr(O, rule)(ps, q, **hp)


GRID = [dict(lr=0.01, momentum=0.0), dict(lr=0.01, momentum=0.9, weight_decay=5e-4),
        dict(lr=0.03, momentum=0.9, weight_decay=1e-4, dampening=0.1), dict(lr=0.01, momentum=0.9, weight_decay=5e-4, nesterov=True),
        dict(lr=0.02, momentum=0.0, weight_decay=3e-4)]
RULES = [("DSGD", 8), ("DSGD", 7), ("DSGD", 32), ("SSGD", 8), ("NormalSGD", 32)]


@pytest.mark.parametrize("rule,q", RULES)
@pytest.mark.parametrize("hp", range(len(GRID)))
def test_fused_matches_device_composite(rule, q, hp):
    """Same inputs, same GPU, six steps with lr changed between steps; a third of the tensors receive their first
    gradient on step 2, so one launch mixes first-step and later-step tensors."""
    hp = GRID[hp]
    gen = torch.Generator().manual_seed(1234)
    spec = _tensor_set(gen)
    shapes = [p.shape for p in _make_params(spec)[0]]
    steps_grads = [[_values(int(np.prod(sh)), gen, 0.01).view(sh) for sh in shapes] for _ in range(5)]
    runs = []
    for fused in (True, False):
        ps, g0 = _make_params(spec)
        opt = _build(rule, q, ps, **hp)
        O.options.fused = fused
        for s in range(6):
            for i, p in enumerate(ps):
                if s == 0 and i % 3 == 0:
                    p.grad = None
                    continue
                src = g0[i] if s == 0 else steps_grads[s - 1][i].to(DEV)
                g = torch.empty_like(p)   # same strides as p (and the same 1-float offset for the views)
                if p.storage_offset():
                    g = torch.empty(p.numel() + 1, device=DEV)[1:]
                g.copy_(src)
                p.grad = g
            for group in opt.param_groups:
                group["lr"] = hp["lr"] * (1 + s) / 3
            opt.step()
        torch.cuda.synchronize()
        runs.append((ps, opt))
    (pa, oa), (pb, ob) = runs
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert a.stride() == b.stride()
        assert same_bits(a.detach().cpu().numpy(), b.detach().cpu().numpy()), (rule, q, hp, i, a.shape)
        assert same_bits(a.grad.cpu().numpy(), b.grad.cpu().numpy()), (rule, q, hp, i)
        if hp.get("momentum"):
            assert same_bits(oa.state[a]["momentum_buffer"].cpu().numpy(), ob.state[b]["momentum_buffer"].cpu().numpy()), (i,)


def _net(seed):
    torch.manual_seed(seed)
    Conv = conv2d_Q_bias(8, 0.12, 1.0)
    Lin = linear_Q(8, 0.05, 1.0)
    return torch.nn.Sequential(Conv(3, 16, 3, padding=1), torch.nn.BatchNorm2d(16), torch.nn.ReLU(),
                               torch.nn.AdaptiveAvgPool2d(2), torch.nn.Flatten(), Lin(64, 10)).to(DEV)


def _grads(net):
    torch.manual_seed(7)
    x = torch.randn(8, 3, 12, 12, device=DEV)
    net(x).square().mean().backward()
    return [p.grad.detach().clone() for p in net.parameters()]


def _step_n(net, opt, grads, n, sched=None):
    for _ in range(n):
        for p, g in zip(net.parameters(), grads):
            p.grad = g.clone()
        opt.step()
        if sched is not None:
            sched.step()


def test_model_level_fused_equals_composite_and_checkpoints_interchange():
    base = _net(0)
    grads = _grads(base)
    hp = dict(lr=0.05, momentum=0.9, weight_decay=5e-4)
    nets, opts = [], []
    for fused in (True, False):
        O.options.fused = fused
        net = _net(0)   # the same initial weights as `base` (which holds autograd outputs and cannot be deep-copied)
        opt = O.DSGD(net.parameters(), 8, **hp)
        sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[2], gamma=0.1)
        _step_n(net, opt, grads, 4, sched)
        assert opt.param_groups[0]["lr"] == pytest.approx(0.005)
        nets.append(net)
        opts.append(opt)
    for a, b in zip(nets[0].parameters(), nets[1].parameters()):
        assert same_bits(a.detach().cpu().numpy(), b.detach().cpu().numpy())
    sa, sb = opts[0].state_dict(), opts[1].state_dict()
    assert sa["param_groups"] == sb["param_groups"]
    for k in sa["state"]:
        assert same_bits(sa["state"][k]["momentum_buffer"].cpu().numpy(), sb["state"][k]["momentum_buffer"].cpu().numpy())

    # the schedule took effect: without it the weights end elsewhere
    O.options.fused = True
    net_c = _net(0)
    _step_n(net_c, O.DSGD(net_c.parameters(), 8, **hp), grads, 4)
    assert any(not torch.equal(a, c) for a, c in zip(nets[0].parameters(), net_c.parameters()))

    # DSGD -> torch.optim.SGD -> DSGD: the momentum state survives the round trip
    net_a, net_b = copy.deepcopy(nets[0]), copy.deepcopy(nets[0])
    sgd = torch.optim.SGD(net_b.parameters(), lr=0.005, momentum=0.9, weight_decay=5e-4)
    sgd.load_state_dict(copy.deepcopy(opts[0].state_dict()))   # load_state_dict keeps (aliases) same-device tensors
    back = O.DSGD(net_b.parameters(), 8, **hp)
    back.load_state_dict(copy.deepcopy(sgd.state_dict()))
    cont = O.DSGD(net_a.parameters(), 8, **hp)
    cont.load_state_dict(copy.deepcopy(opts[0].state_dict()))
    _step_n(net_a, cont, grads, 1)
    _step_n(net_b, back, grads, 1)
    for a, b in zip(net_a.parameters(), net_b.parameters()):
        assert same_bits(a.detach().cpu().numpy(), b.detach().cpu().numpy())


def test_step_invalidates_conv_inference_cache():
    """A Conv2d_Q kept in eval() under no_grad sees the stepped weights without any eval()/train() call in between."""
    torch.manual_seed(3)
    Conv = conv2d_Q_bias(8, 0.12, 1.0)
    m = Conv(16, 32, 3, padding=1).to(DEV).eval()
    x = torch.randn(2, 16, 10, 10, device=DEV)
    opt = O.DSGD(m.parameters(), 8, lr=0.5, momentum=0.9)
    with torch.no_grad():
        y0 = m(x).clone()
        m(x)   # the prepared weights are cached now
        for p in m.parameters():
            p.grad = torch.randn_like(p)
        opt.step()
        y1 = m(x)
        fresh = Conv(16, 32, 3, padding=1).to(DEV).eval()
        fresh.load_state_dict(m.state_dict())
        y_ref = fresh(x)
    assert not torch.equal(y0, y1)
    assert same_bits(y1.cpu().numpy(), y_ref.cpu().numpy())


def _layouts(gen):
    """(param, grad) pairs on the device in every layout the fast path takes: contiguous (with a vector tail), a view at a
    1-float offset, channels_last, and a depthwise (C, 1, 3, 3) weight whose grad has another stride in the size-1 dim."""
    out = []
    for n in (5, 4097):
        out.append((_values(n, gen, 0.5).to(DEV), _values(n, gen, 0.01).to(DEV)))
    p, g = _values(1025, gen, 0.5).to(DEV), _values(1025, gen, 0.01).to(DEV)
    out.append((p[1:], g[1:]))
    p = _values(64 * 32 * 9, gen, 0.5).view(64, 32, 3, 3).to(DEV).contiguous(memory_format=torch.channels_last)
    g = _values(64 * 32 * 9, gen, 0.01).view(64, 32, 3, 3).to(DEV).contiguous(memory_format=torch.channels_last)
    out.append((p, g))
    p = _values(32 * 9, gen, 0.5).view(32, 1, 3, 3).to(DEV)
    g = torch.empty_strided((32, 1, 3, 3), (9, 1, 3, 1), device=DEV)
    g.copy_(_values(32 * 9, gen, 0.01).view(32, 1, 3, 3))
    out.append((p, g))
    return out


@pytest.mark.parametrize("rule,q", RULES)
def test_fused_path_runs_the_kernel_for_every_dense_layout(rule, q, monkeypatch):
    """With options.fused the composite is never called for these parameters (it raises here), and the kernel's
    result equals the composite's."""
    hp = dict(lr=0.02, momentum=0.9, weight_decay=5e-4)
    gen = torch.Generator().manual_seed(99)
    pairs = _layouts(gen)
    grads = [[(_values(g.numel(), gen, 0.01).view(g.shape)) for _, g in pairs] for _ in range(3)]
    real_composite = O._QuantSGD._composite_step
    results = []
    for fused in (True, False):
        O.options.fused = fused
        if fused:
            def no_composite(self, p, g, group):
                raise AssertionError(f"parameter {tuple(p.shape)} / stride {p.stride()} left the fused path")
            monkeypatch.setattr(O._QuantSGD, "_composite_step", no_composite)
        else:
            monkeypatch.setattr(O._QuantSGD, "_composite_step", real_composite)
        ps = [torch.nn.Parameter(p.clone() if not p.storage_offset() else torch.empty(p.numel() + 1, device=DEV)[1:].copy_(p))
              for p, _ in pairs]
        opt = _build(rule, q, ps, **hp)
        for s in range(3):
            for p, (_, g0), src in zip(ps, pairs, grads[s]):
                g = g0.clone() if not g0.storage_offset() else torch.empty(g0.numel() + 1, device=DEV)[1:]
                if g.stride() != g0.stride():
                    g = torch.empty_strided(g0.shape, g0.stride(), device=DEV)
                g.copy_(src)
                p.grad = g
            opt.step()
        torch.cuda.synchronize()
        results.append((ps, opt))
    (pa, oa), (pb, ob) = results
    for a, b in zip(pa, pb):
        assert same_bits(a.detach().cpu().numpy(), b.detach().cpu().numpy()), (rule, q, tuple(a.shape))
        assert same_bits(a.grad.cpu().numpy(), b.grad.cpu().numpy())
        assert same_bits(oa.state[a]["momentum_buffer"].cpu().numpy(), ob.state[b]["momentum_buffer"].cpu().numpy())


def test_buffer_of_another_shape_never_reaches_the_kernel(monkeypatch):
    """A checkpoint's momentum buffer with fewer elements than the parameter goes to the composite, which raises; the
    kernel entry is replaced by a recorder here, so nothing is launched even if the gate were wrong."""
    seen = []
    monkeypatch.setattr(O._QuantSGD, "_fused_step", lambda self, dev, items, group, qbits: seen.extend(it[0] for it in items))
    a = torch.nn.Parameter(torch.zeros(10, device=DEV))
    b = torch.nn.Parameter(torch.zeros(6, device=DEV))
    opt = O.DSGD([a, b], 8, lr=0.1, momentum=0.9)
    sd = opt.state_dict()
    sd["state"] = {0: {"momentum_buffer": torch.zeros(5, device=DEV)}, 1: {"momentum_buffer": torch.zeros(6, device=DEV)}}
    opt.load_state_dict(sd)
    a.grad, b.grad = torch.ones(10, device=DEV), torch.ones(6, device=DEV)
    with pytest.raises(RuntimeError):
        opt.step()
    assert all(t is not a for t in seen)
