"""Mirror of the reference's utils/optimizer.py: the quantization-aware SGD variants DSGD, SSGD and NormalSGD.

Same names, signatures, ValueErrors, param-group keys and `state[p]['momentum_buffer']` as the reference, so
checkpoints interchange with it and with torch.optim.SGD, and `from utils.optimizer import *` keeps working.  The
step is the reference's op sequence, element for element, in float32:

    g = g + wd * p (p.grad keeps it);  buf = g on the first step, else buf * m + (1 - damp) * g;
    d = g + m * buf (nesterov) | buf | g;  t = (-lr) * d;  wb = Q(p);  p = p + t
    DSGD: s = 2 where |wb - Q(p)| < 1e-4, else 0;  SSGD: s = |p| + 1;  NormalSGD: done
    p = p + t * s

Q is quantize_weight(qbit) at unit scale.  ROCm float32 parameters that are contiguous or channels_last, and whose
grad and momentum buffer have p's shape and strides (strides of size-1 dims aside), are stepped by ONE multi-tensor HIP
kernel per group of up to 48 tensors (slfp_sgd_step_f32), on the current stream of their device and without a host
synchronisation.
Every other parameter goes through `_composite_step`, the same sequence as ATen ops on the tensor's device; it calls
`self.quantize_fn`, so q_bit 8 / 7 on CPU tensors raises this package's usual error, and a test may replace
`quantize_fn` to drive it with another quantizer (the fused path is then not used).  `options.fused = False` sends
every parameter through the composite (A/B runs).

Unlike the reference's `p.data` updates, a step bumps every stepped parameter's version counter, so the inference
weight cache of Conv2d_Q / Linear_Q (keyed on `_version`) sees the new weights.
"""
import ctypes

import torch
import torch.optim as optim
from torch.optim import Optimizer
from torch.optim.optimizer import required

from . import _lib
from .sfp_quant import *  # noqa: F401,F403  (the reference re-exports these: utils/optimizer.py:6)
from .sfp_quant import __all__ as _sfp_all
from .sfp_quant import weight_quantize_func

__all__ = list(_sfp_all) + ["optim", "Optimizer", "required", "DSGD", "SSGD", "NormalSGD"]


class _Options:
    """Process-wide switch of the step (not part of the reference API)."""
    fused = True  # False: every parameter through the ATen composite (A/B runs)


options = _Options()

_THRESH = 1e-4  # utils/optimizer.py: `abs(before - after) > 0.0001`, compared in float32


def _f32(v):
    return ctypes.c_float(float(v)).value


def _check_args(lr, momentum, dampening, weight_decay, nesterov):
    if lr is not required and lr < 0.0:
        raise ValueError("Invalid learning rate: {}".format(lr))
    if momentum < 0.0:
        raise ValueError("Invalid momentum value: {}".format(momentum))
    if weight_decay < 0.0:
        raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
    if nesterov and (momentum <= 0 or dampening != 0):
        raise ValueError("Nesterov momentum requires a momentum and zero dampening")


def _dense_like(t, p):
    """t has p's shape, dtype, device and memory order: the kernel walks both with one linear index over p.numel()
    elements.  Strides of size-1 dims are ignored (they address nothing), so e.g. a depthwise (C, 1, 3, 3) weight whose
    grad carries another stride in dim 1 stays on the kernel.  A shape mismatch (a momentum buffer from another model's
    checkpoint) takes the composite, which raises as the reference does."""
    if t.dtype != torch.float32 or t.device != p.device or t.layout != torch.strided or t.shape != p.shape:
        return False
    return all(a == b for a, b, n in zip(t.stride(), p.stride(), p.shape) if n > 1)


def _fusable(p, g, buf):
    if not (p.is_cuda and p.dtype == torch.float32 and _dense_like(g, p)):
        return False
    if not (p.is_contiguous() or (p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last))):
        return False
    return buf is None or _dense_like(buf, p)


class _QuantSGD(Optimizer):
    """Shared body of DSGD / SSGD / NormalSGD; `_rule` selects the scale term."""
    _rule = _lib.OPT_SGD

    def __init__(self, params, qbit, lr, momentum, dampening, weight_decay, nesterov):
        _check_args(lr, momentum, dampening, weight_decay, nesterov)
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov)
        super().__init__(params, defaults)
        if qbit is not None:
            self.quantize_fn = weight_quantize_func(q_bit=qbit)

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault('nesterov', False)

    def _qbits(self):
        """q_bit of the fused kernel's quantizer, or None when only the composite can run this optimizer."""
        if self._rule == _lib.OPT_SGD:
            return 32
        q = getattr(self, "quantize_fn", None)
        if type(q) is not weight_quantize_func or q.q_bit not in (32, 8, 7):
            return None
        return q.q_bit

    def step(self, closure=None):
        loss = None
        if closure is not None:
            loss = closure()
        qbits = self._qbits()
        if self._rule != _lib.OPT_SGD:
            q = getattr(self.quantize_fn, "q_bit", 32)
            if q not in (32, 8, 7):
                # the reference's quantize_fn falls off its if/elif on the first step (utils/sfp_quant.py:142-147)
                raise UnboundLocalError("q_bit must be 32, 8 or 7 for the SLFP/SFP quantizers")
        with torch.no_grad():
            for group in self.param_groups:
                # the kernel tests float32(momentum) / float32(weight_decay) against 0, the reference the Python values
                group_ok = all((group[k] == 0) == (_f32(group[k]) == 0) for k in ('momentum', 'weight_decay'))
                fused = {}  # device -> [(p, g, buf, first)]
                for p in group['params']:
                    if p.grad is None:
                        continue
                    g = p.grad
                    if g.is_sparse:
                        raise RuntimeError(f"{type(self).__name__} does not support sparse gradients")
                    buf = self.state[p].get('momentum_buffer') if group['momentum'] != 0 else None
                    if options.fused and group_ok and qbits is not None and _fusable(p, g, buf):
                        first = buf is None and group['momentum'] != 0
                        if first:
                            buf = self.state[p]['momentum_buffer'] = torch.empty_like(g)
                        fused.setdefault(p.device, []).append((p, g, buf, first))
                    else:
                        self._composite_step(p, g, group)
                        torch.autograd.graph.increment_version(p)
                for dev, items in fused.items():
                    self._fused_step(dev, items, group, qbits)
                    for p, _, _, _ in items:
                        torch.autograd.graph.increment_version(p)
        return loss

    def _fused_step(self, dev, items, group, qbits):
        live = [it for it in items if it[0].numel() > 0]
        if not live:
            return
        n = len(live)
        ptrs = ctypes.c_void_p * n
        h = _lib.SgdHparams(rule=self._rule, qbits=qbits, lr=_f32(group['lr']), momentum=_f32(group['momentum']),
                            damp_alpha=_f32(1 - group['dampening']), weight_decay=_f32(group['weight_decay']),
                            nesterov=1 if group['nesterov'] else 0, reserved=0)
        mom = group['momentum'] != 0
        P = ptrs(*[it[0].data_ptr() for it in live])
        G = ptrs(*[it[1].data_ptr() for it in live])
        B = ptrs(*[it[2].data_ptr() for it in live]) if mom else None
        N = (ctypes.c_int64 * n)(*[it[0].numel() for it in live])
        F1 = (ctypes.c_uint8 * n)(*[1 if it[3] else 0 for it in live])
        L = _lib.load()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(L.slfp_sgd_step_f32(ctypes.byref(h), n, P, G, B, N, F1, stream))

    def _composite_step(self, p, g, group):
        """The step as ATen ops on p's device (one op per line, each its own float32 rounding)."""
        wd, m, damp, lr = group['weight_decay'], group['momentum'], group['dampening'], group['lr']
        if wd != 0:
            g.add_(p, alpha=wd)
        d = g
        if m != 0:
            state = self.state[p]
            buf = state.get('momentum_buffer')
            if buf is None:
                buf = state['momentum_buffer'] = g.clone()
            else:
                buf.mul_(m).add_(g, alpha=1 - damp)
            d = g.add(buf, alpha=m) if group['nesterov'] else buf
        t = d.mul(-lr)
        if self._rule == _lib.OPT_DSGD:
            before = self.quantize_fn(p.clone())  # Q is the identity for q_bit 32: no alias of p
        p.add_(t)
        if self._rule == _lib.OPT_SGD:
            return
        if self._rule == _lib.OPT_DSGD:
            diff = (before - self.quantize_fn(p)).abs()
            s = torch.where(diff < _THRESH, torch.full_like(p, 2.0), torch.zeros_like(p))
        else:
            s = p.abs().add(1)
        p.add_(t.mul(s))


class DSGD(_QuantSGD):
    """utils/optimizer.py DSGD: the SGD update, doubled where it leaves Q(p) unchanged and undone where it moves it."""
    _rule = _lib.OPT_DSGD

    def __init__(self, params, qbit, lr=required, momentum=0, dampening=0, weight_decay=0, nesterov=False):
        super().__init__(params, qbit, lr, momentum, dampening, weight_decay, nesterov)


class SSGD(_QuantSGD):
    """utils/optimizer.py SSGD: the SGD update, applied once more scaled by |p| + 1."""
    _rule = _lib.OPT_SSGD

    def __init__(self, params, qbit, lr=required, momentum=0, dampening=0, weight_decay=0, nesterov=False):
        super().__init__(params, qbit, lr, momentum, dampening, weight_decay, nesterov)


class NormalSGD(_QuantSGD):
    """utils/optimizer.py NormalSGD: plain SGD with momentum, dampening, weight decay and Nesterov."""
    _rule = _lib.OPT_SGD

    def __init__(self, params, lr=required, momentum=0, dampening=0, weight_decay=0, nesterov=False):
        super().__init__(params, None, lr, momentum, dampening, weight_decay, nesterov)
