"""Training-mode BatchNorm2d (+ReLU) on libslfp_hip's kernels (csrc/bn_train.hip; include/slfp.h states the order of every
sum): the autograd Function behind fusion.TrainBatchNorm2d.  float32 channels_last tensors on the ROCm device only; there is no
fallback in here -- the module decides with bn_train_supported() and otherwise runs ATen's batch_norm itself."""
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .conv2d_func import _on_device, _ptr, _stream_handle, _workspace


# The measured rule of DESIGN section 27 (profiles/bn_train_bench.json): forward + backward of the swapped module was faster
# than the stock modules by more than their run-to-run spread on every shape from 25.7 M elements (N C H W) on, and on none
# of the classes below (12.8 M, 6.4 M, 3.2 M and smaller), where six launches issued from Python set a floor of 0.2 ms.  The
# module leaves smaller tensors to ATen.  The C query slfp_bn_train_supported answers what the kernels CAN run.
MIN_ELEMENTS = 16 << 20


def bn_train_supported(x, min_elements=None):
    """Does the module run libslfp_hip's kernels on the 4-d ROCm float32 tensor `x` as it lies in memory (channels_last, aligned
    as the kernel reads it, at least `min_elements` elements -- None: MIN_ELEMENTS, the measured rule)?  Then
    slfp_bn_train_supported, host only: one value per channel (N H W == 1) is refused, as ATen refuses it."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.numel() > 0):
        return False
    if x.numel() < (MIN_ELEMENTS if min_elements is None else min_elements):
        return False
    if not x.is_contiguous(memory_format=torch.channels_last):
        return False
    n, c, h, w = x.shape
    if x.data_ptr() % (16 if c % 4 == 0 else 4):
        return False
    return bool(_lib.load().slfp_bn_train_supported(n, h, w, c, _lib.LAYOUT_NHWC))


def _nhwc(t):
    """`t` dense in channels_last order at an address the vector kernels can read."""
    if not t.is_contiguous(memory_format=torch.channels_last):
        t = t.contiguous(memory_format=torch.channels_last)
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.channels_last)


def _vec(t):
    """A per-channel array as the kernels read it: dense, and at a 16-byte address (a Parameter may be a view into a flat buffer)."""
    t = t.detach().contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


class hip_bn_train(torch.autograd.Function):
    """y = relu?(batch_norm(x)) with batch statistics; running_mean / running_var (both or neither) are updated in place.
    x: channels_last float32 that bn_train_supported() accepts; weight, bias: float32 [C].  Returns y (channels_last).  The
    output is saved for the backward only with `relu` (the mask is read from it): without, the backward does not read y, and
    the caller may change it in place (`out += identity`, a shared nn.ReLU(inplace=True)) as behind the stock module."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps, relu):
        L = _lib.load()
        n, c, h, w = x.shape
        x = x.detach()
        gamma, beta = _vec(weight), _vec(bias)
        y = torch.empty_like(x)   # keeps the channels_last strides
        save_mean = torch.empty(c, dtype=torch.float32, device=x.device)
        save_invstd = torch.empty(c, dtype=torch.float32, device=x.device)
        with _on_device(x.device):
            nbytes = L.slfp_bn_train_workspace_bytes(n, h, w, c)
            ws = _workspace(x.device, nbytes)
            _lib.check(L.slfp_bn_train_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(running_mean), _ptr(running_var),
                                           float(momentum), float(eps), 1 if relu else 0, y.data_ptr(), save_mean.data_ptr(),
                                           save_invstd.data_ptr(), n, h, w, c, _lib.LAYOUT_NHWC, ws.data_ptr(), nbytes,
                                           _stream_handle(x)))
        ctx.relu = bool(relu)
        if ctx.relu:
            ctx.save_for_backward(x, weight, save_mean, save_invstd, y)
        else:
            ctx.save_for_backward(x, weight, save_mean, save_invstd)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        L = _lib.load()
        x, weight, save_mean, save_invstd = ctx.saved_tensors[:4]
        y = ctx.saved_tensors[4] if ctx.relu else x   # relu == 0: y is not read; any valid pointer stands in
        n, c, h, w = x.shape
        gy = _nhwc(gy)
        gamma = _vec(weight)
        gx = torch.empty_like(x)
        ggamma = torch.empty_like(save_mean) if ctx.needs_input_grad[1] else None
        gbeta = torch.empty_like(save_mean) if ctx.needs_input_grad[2] else None
        with _on_device(x.device):
            nbytes = L.slfp_bn_train_workspace_bytes(n, h, w, c)
            ws = _workspace(x.device, nbytes)
            _lib.check(L.slfp_bn_train_bwd(x.data_ptr(), y.data_ptr(), gy.data_ptr(), gamma.data_ptr(), save_mean.data_ptr(),
                                           save_invstd.data_ptr(), 1 if ctx.relu else 0, gx.data_ptr(), _ptr(ggamma), _ptr(gbeta),
                                           n, h, w, c, _lib.LAYOUT_NHWC, ws.data_ptr(), nbytes, _stream_handle(x)))
        return gx if ctx.needs_input_grad[0] else None, ggamma, gbeta, None, None, None, None, None
