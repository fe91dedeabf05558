"""What tests/test_gpu_backward.py and tests/test_gpu_backward_dense.py share: the inputs that reach every code range, the
float64 reference from the C oracle's quantized operands, the two error measures and the check of one layer against them.
A plain module, imported by name (as _aniso_cases is)."""
import torch

from oracle import slfp_oracle
from cnns_slfp_quantization_amd import conv2d_func as cf
from cnns_slfp_quantization_amd.conv2d_func import conv2d_Q, conv2d_Q_bias

DEV = "cuda"


def _x_values(shape, ka, gen, relu=False):
    """Every code range: below 0.0625*Ka, the log range, above the clamp, negatives, exact zeros."""
    mag = torch.exp2(torch.empty(shape).uniform_(-9, 5, generator=gen)) * ka
    sign = torch.where(torch.rand(shape, generator=gen) < 0.5, -1.0, 1.0) if not relu else 1.0
    x = mag * sign
    x[torch.rand(shape, generator=gen) < 0.05] = 0.0
    return x.float()


def _contractions(xq, wq, gy, mod, x_shape, w_shape):
    """(gx, gw, gb), each with the same contraction over absolute values, in float64."""
    ka, kw = cf._f32(mod.Ka), cf._f32(mod.Kw)
    g = gy.double()
    args = (mod.stride, mod.padding, mod.dilation, mod.groups)
    gx = torch.nn.grad.conv2d_input(x_shape, wq, g, *args) * kw
    ax = torch.nn.grad.conv2d_input(x_shape, wq.abs(), g.abs(), *args) * kw
    gw = torch.nn.grad.conv2d_weight(xq, w_shape, g, *args) * ka
    aw = torch.nn.grad.conv2d_weight(xq.abs(), w_shape, g.abs(), *args) * ka
    return (gx, ax), (gw, aw), (g.sum(dim=(0, 2, 3)), g.abs().sum(dim=(0, 2, 3)))


def _reference(x, w, gy, mod):
    """_contractions of the oracle's quantized operands."""
    q = mod.q_bit
    xq = torch.from_numpy(slfp_oracle.quantize(x.numpy(), cf._f32(mod.Ka), 0 if q == 8 else 2)).double()
    wq = torch.from_numpy(slfp_oracle.quantize(w.numpy(), cf._f32(mod.Kw), 1 if q == 8 else 2)).double()
    return _contractions(xq, wq, gy, mod, x.shape, w.shape)


def _errors(got, ref):
    """(max |g - ref| / abs64 elementwise, tensor-relative L2)."""
    r, a = ref
    d = (got.double().cpu() - r).abs()
    elem = torch.where(a > 0, d / a.clamp_min(1e-300), torch.where(d > 0, torch.inf, 0.0)).max().item()
    l2 = (d.norm() / r.norm().clamp_min(1e-300)).item()
    return elem, l2


def _conv_grads(mod, x, gy, mode, need=(True, True, True)):
    cf.options.backward = mode
    xi = x.detach().clone().requires_grad_(need[0])
    mod.weight.requires_grad_(need[1])
    if mod.bias is not None:
        mod.bias.requires_grad_(need[2])
    mod.zero_grad(set_to_none=True)
    out = mod(xi)
    out.backward(gy)
    gb = mod.bias.grad if mod.bias is not None else None
    return xi.grad, mod.weight.grad, gb, out


def _make(spec, q, scaled, gen, bias=True):
    cls = conv2d_Q_bias if scaled else conv2d_Q
    mod = cls(q, spec.Kw, spec.Ka)(spec.c_in, spec.c_out, spec.k, stride=spec.stride, padding=spec.pad,
                                   groups=spec.groups, bias=bias).to(DEV)
    with torch.no_grad():
        fan = spec.c_in // spec.groups * spec.k[0] * spec.k[1]
        mod.weight.copy_((torch.randn(mod.weight.shape, generator=gen) * (2.0 / fan) ** 0.5).to(DEV))
        if mod.bias is not None:
            mod.bias.copy_((torch.randn(spec.c_out, generator=gen) * 0.1).to(DEV))
    return mod


def _sparse(gy, gen):
    """Two non-zeros per channel."""
    n, c = gy.shape[:2]
    keep = torch.zeros_like(gy, dtype=torch.bool).view(n, c, -1)
    for ch in range(c):
        idx = torch.randperm(n * keep.shape[2], generator=gen)[:2]
        keep[idx // keep.shape[2], ch, idx % keep.shape[2]] = True
    return gy * keep.view_as(gy)


def _check_case(spec, n, q, scaled, gen, channels_last, mode, kernels, sparse=False, label="", composite=True):
    """One layer's backward under `mode` (which must run one of `kernels`) against the float64 reference: elementwise
    <= 1e-5 of the sum of |terms| and tensor-relative L2 <= 1e-6 for gx, gw and (scaled-bias class) gb.  The composite's
    error on the same inputs is printed next to it.  Returns `mode`'s (gx, gw, gb)."""
    mod = _make(spec, q, scaled, gen)
    x = _x_values((n, spec.c_in, spec.h, spec.w), spec.Ka, gen)
    gy = torch.randn((n, spec.c_out, spec.h_out, spec.w_out), generator=gen)
    if sparse:
        gy = _sparse(gy, gen)
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    xd = x.to(DEV).contiguous(memory_format=fmt)
    gyd = gy.to(DEV).contiguous(memory_format=fmt)
    refs = _reference(x, mod.weight.detach().cpu(), gy, mod)
    res, grads = {}, None
    for m in (mode, "composite") if composite else (mode,):
        gx, gw, gb, _ = _conv_grads(mod, xd, gyd, m)
        res[m] = [_errors(gx, refs[0]), _errors(gw, refs[1])]
        if mod.bias is not None and scaled:
            res[m].append(_errors(gb, refs[2]))
        if m == mode:
            grads = (gx, gw, gb)
            assert mod._last_bwd_kernel in kernels, mod._last_bwd_kernel
            assert gx.shape == x.shape and gx.is_contiguous(memory_format=fmt)
            assert gw.shape == mod.weight.shape and gw.is_contiguous()
            if spec.k == (1, 1) and spec.stride == (2, 2) and spec.pad == (0, 0):
                # the three phases no output position reads: exact zeros, and written
                live = torch.zeros(spec.h, spec.w, dtype=torch.bool)
                live[::2, ::2] = True
                assert (gx.cpu()[:, :, ~live] == 0).all()
                assert (gx.cpu()[:, :, live] != 0).any()
    fmt_e = lambda r: [(f"{e:.2e}", f"{l:.2e}") for e, l in r]
    print(f"{label} {spec.c_in}->{spec.c_out} k{spec.k} s{spec.stride} p{spec.pad} g{spec.groups} @{spec.h}x{spec.w} n={n} q{q} "
          f"{'scaled' if scaled else 'raw'} {'nhwc' if channels_last else 'nchw'}: "
          + "  ".join(f"{m} {fmt_e(r)}" for m, r in res.items()))
    for e, l in res[mode]:
        assert e <= 1e-5 and l <= 1e-6, res[mode]
    return grads
