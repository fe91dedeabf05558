"""CPU: the quantization-aware optimizers of utils/optimizer.py (DSGD, SSGD, NormalSGD) -- the drop-in import, the
reference's constructor contract, the ATen composite step against the reference's recorded outputs
(tests/golden/optim_golden.npz, tests/golden/make_golden_optim.py), and argument validation of slfp_sgd_step_f32,
which answers without a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, same_bits
from cnns_slfp_quantization_amd import _lib
from oracle.torch_port import fake_quant


def test_utils_optimizer_resolves_to_this_package():
    import cnns_slfp_quantization_amd.optimizer as mine
    import utils.optimizer as shim
    from utils.optimizer import DSGD, SSGD, NormalSGD
    assert (DSGD, SSGD, NormalSGD) == (mine.DSGD, mine.SSGD, mine.NormalSGD)
    assert os.path.abspath(shim.__file__).startswith(os.path.abspath(ROOT))
    # what `from utils.optimizer import *` gives a reference script (its torchvision import aside)
    for name in ("DSGD", "SSGD", "NormalSGD", "optim", "Optimizer", "required", "torch", "nn", "F", "np",
                 "quantize_weight", "quantize_act", "weight_quantize_func", "act_quantize_func"):
        assert name in shim.__all__, name
    assert "torchvision" not in shim.__all__
    assert shim.optim is torch.optim and shim.Optimizer is torch.optim.Optimizer
    from torch.optim.optimizer import required
    assert shim.required is required


def _param():
    return [torch.nn.Parameter(torch.zeros(3))]


@pytest.mark.parametrize("cls", ["DSGD", "SSGD", "NormalSGD"])
def test_constructor_contract(cls):
    from cnns_slfp_quantization_amd import optimizer as O
    C = getattr(O, cls)
    mk = (lambda **kw: C(_param(), **kw)) if cls == "NormalSGD" else (lambda **kw: C(_param(), 8, **kw))
    for kw, text in ((dict(lr=-0.1), "Invalid learning rate: -0.1"), (dict(lr=0.1, momentum=-1), "Invalid momentum value: -1"),
                     (dict(lr=0.1, weight_decay=-1e-4), "Invalid weight_decay value: -0.0001"),
                     (dict(lr=0.1, nesterov=True), "Nesterov momentum requires a momentum and zero dampening"),
                     (dict(lr=0.1, momentum=0.9, dampening=0.1, nesterov=True), "Nesterov momentum requires")):
        with pytest.raises(ValueError, match=text):
            mk(**kw)
    with pytest.raises(ValueError, match="lr"):   # lr=required and no value in the group
        mk()
    opt = mk(lr=0.1)
    assert opt.defaults == dict(lr=0.1, momentum=0, dampening=0, weight_decay=0, nesterov=False)
    assert isinstance(opt, torch.optim.Optimizer)
    g = opt.param_groups[0]
    del g["nesterov"]
    opt.__setstate__({"state": opt.state, "param_groups": opt.param_groups})
    assert g["nesterov"] is False
    if cls == "NormalSGD":
        assert not hasattr(opt, "quantize_fn")
    else:
        from cnns_slfp_quantization_amd.sfp_quant import weight_quantize_func
        assert isinstance(opt.quantize_fn, weight_quantize_func) and opt.quantize_fn.q_bit == 8
        assert C(_param(), qbit=7, lr=0.1).quantize_fn.q_bit == 7
        with pytest.raises(AssertionError):    # weight_quantize_func asserts q_bit <= 8 or 32
            C(_param(), 16, lr=0.1)


def _golden():
    return np.load(os.path.join(GOLDEN, "optim_golden.npz"))


def _cases(z):
    return sorted({k.rsplit("_p_s", 1)[0] for k in z.files if "_p_s" in k})


def test_fixture_covers_the_grid():
    z = _golden()
    assert len(_cases(z)) == 14
    assert np.isnan(z["g1"]).any() and np.isinf(z["g1"]).any()


@pytest.mark.parametrize("case", _cases(_golden()))
def test_composite_matches_reference_fixture(case):
    """The package's composite step, driven by the CPU port of the reference quantizer, reproduces every recorded step
    bit for bit: p, p.grad and the momentum buffer."""
    from cnns_slfp_quantization_amd import optimizer as O
    z = _golden()
    rule, q, m = case.split("_")
    q, m = int(q[1:]), int(m[1:]) / 10
    lr = float(z["lr"])
    p = torch.nn.Parameter(torch.from_numpy(z["p0"].copy()))
    if rule == "NormalSGD":
        opt = O.NormalSGD([p], lr=lr, momentum=m)
    else:
        opt = getattr(O, rule)([p], q, lr=lr, momentum=m)
        opt.quantize_fn = lambda x: fake_quant(x, q, "weight")
    for k in (1, 2, 3):
        p.grad = torch.from_numpy(z[f"g{k}"].copy())
        opt.step()
        assert same_bits(p.detach().numpy(), z[f"{case}_p_s{k}"]), (case, k)
        assert same_bits(p.grad.numpy(), z[f"grad_s{k}"]), (case, k)
        if m:
            assert same_bits(opt.state[p]["momentum_buffer"].numpy(), z[f"{case}_buf_s{k}"]), (case, k)


def test_cpu_params_use_the_package_quantizer():
    """No CPU compute path for the SLFP quantizers: DSGD q_bit 8 on a CPU tensor raises the package's usual error; q_bit 32
    and SSGD (whose quantizations the reference computes and then ignores) step on the CPU."""
    from cnns_slfp_quantization_amd import optimizer as O
    p = torch.nn.Parameter(torch.ones(4))
    p.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="ROCm"):
        O.DSGD([p], 8, lr=0.1).step()
    O.DSGD([p], 32, lr=0.1).step()
    O.SSGD([p], 8, lr=0.1).step()
    with pytest.raises(UnboundLocalError):      # the reference's quantizer falls off its if/elif for q_bit 5
        O.DSGD([p], 5, lr=0.1).step()


def test_step_bumps_version_and_matches_torch_sgd_state():
    from cnns_slfp_quantization_amd import optimizer as O
    torch.manual_seed(0)
    a = torch.nn.Parameter(torch.randn(10))
    b = torch.nn.Parameter(a.detach().clone())
    oa = O.NormalSGD([a], lr=0.1, momentum=0.9)
    ob = torch.optim.SGD([b], lr=0.1, momentum=0.9)
    for _ in range(2):
        g = torch.randn(10)
        a.grad, b.grad = g.clone(), g.clone()
        v = a._version
        oa.step()
        ob.step()
        assert a._version > v
    assert torch.equal(oa.state[a]["momentum_buffer"], ob.state[b]["momentum_buffer"])
    oc = O.NormalSGD([b], lr=0.1, momentum=0.9)
    oc.load_state_dict(ob.state_dict())
    assert torch.equal(oc.state[b]["momentum_buffer"], oa.state[a]["momentum_buffer"])


def test_sparse_grad_raises():
    from cnns_slfp_quantization_amd import optimizer as O
    p = torch.nn.Parameter(torch.ones(4))
    p.grad = torch.ones(4).to_sparse()
    with pytest.raises(RuntimeError, match="sparse"):
        O.SSGD([p], 8, lr=0.1).step()


def _hp(**kw):
    base = dict(rule=_lib.OPT_DSGD, qbits=8, lr=0.1, momentum=0.9, damp_alpha=1.0, weight_decay=0.0, nesterov=0, reserved=0)
    base.update(kw)
    return _lib.SgdHparams(**base)


def test_sgd_step_abi_validation():
    """Every malformed call returns SLFP_ERR_BAD_ARG before any HIP call (no device is touched here: the pointers are
    never dereferenced)."""
    L = _lib.load()
    assert ctypes.sizeof(_lib.SgdHparams) == 32
    fake = 1 << 20
    P = (ctypes.c_void_p * 2)(fake, fake + 64)
    NUL = (ctypes.c_void_p * 2)(fake, None)
    N = (ctypes.c_int64 * 2)(16, 16)
    F1 = (ctypes.c_uint8 * 2)(1, 0)
    call = lambda h, n=2, p=P, g=P, b=P, num=N, f=F1: L.slfp_sgd_step_f32(None if h is None else ctypes.byref(h), n, p, g, b, num, f, None)
    bad = [
        (lambda: call(None), "null hparams"),
        (lambda: call(_hp(rule=3)), "unknown rule"),
        (lambda: call(_hp(qbits=6)), "qbits"),
        (lambda: call(_hp(qbits=16, rule=_lib.OPT_SGD)), "qbits"),
        (lambda: call(_hp(nesterov=2)), "nesterov"),
        (lambda: call(_hp(momentum=0.0, nesterov=1), b=None), "nesterov"),
        (lambda: call(_hp(), b=None), "momentum_buf"),
        (lambda: call(_hp(momentum=0.0)), "momentum_buf"),
        (lambda: call(_hp(), p=None), "null array"),
        (lambda: call(_hp(), num=None), "null array"),
        (lambda: call(_hp(), f=None), "null array"),
        (lambda: call(_hp(), g=NUL), "null pointer"),
        (lambda: call(_hp(), b=NUL), "null pointer"),
        (lambda: call(_hp(), num=(ctypes.c_int64 * 2)(16, -1)), "out of range"),
    ]
    for fn, text in bad:
        assert fn() == _lib.ERR_BAD_ARG, text
        assert text in _lib.last_error(), (text, _lib.last_error())
    assert call(_hp(), n=0) == _lib.OK   # nothing to do


def test_sgd_step_header_and_binding_agree():
    header = open(os.path.join(ROOT, "include", "slfp.h")).read()
    for name, value in (("SLFP_OPT_SGD", _lib.OPT_SGD), ("SLFP_OPT_DSGD", _lib.OPT_DSGD), ("SLFP_OPT_SSGD", _lib.OPT_SSGD)):
        assert f"#define {name} {value}" in header
    fields = [f for f, _ in _lib.SgdHparams._fields_]
    assert fields == ["rule", "qbits", "lr", "momentum", "damp_alpha", "weight_decay", "nesterov", "reserved"]


def test_fast_path_gate_rejects_a_buffer_of_another_shape():
    """The kernel walks p, grad and the momentum buffer with one index over p.numel(): a buffer of another shape (a
    checkpoint of a slightly different model; load_state_dict does not check shapes) must not reach it."""
    from cnns_slfp_quantization_amd import optimizer as O
    p = torch.zeros(10)
    assert O._dense_like(torch.zeros(10), p)
    assert not O._dense_like(torch.zeros(5), p)
    assert not O._dense_like(torch.zeros(20), p)
    w = torch.zeros(8, 16, 3, 3)
    assert not O._dense_like(torch.zeros(4, 16, 3, 3), w)       # same strides, fewer rows
    assert not O._dense_like(torch.zeros(8, 16, 9), w)
    assert not O._dense_like(torch.zeros(8, 16, 3, 3, dtype=torch.float64), w)
    assert not O._dense_like(w.contiguous(memory_format=torch.channels_last), w)
    # strides of size-1 dims address nothing: a depthwise weight's grad may carry another one there
    dw = torch.zeros(32, 1, 3, 3)
    assert O._dense_like(torch.empty_strided((32, 1, 3, 3), (9, 1, 3, 1)), dw)
    # on the composite, the mismatched buffer raises (as the reference's in-place ops do)
    a = torch.nn.Parameter(torch.zeros(10))
    opt = O.NormalSGD([a], lr=0.1, momentum=0.9)
    sd = opt.state_dict()
    sd["state"] = {0: {"momentum_buffer": torch.zeros(5)}}
    opt.load_state_dict(sd)
    a.grad = torch.ones(10)
    with pytest.raises(RuntimeError):
        opt.step()
