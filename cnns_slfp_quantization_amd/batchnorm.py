"""Training-mode BatchNorm2d (+ReLU) on libslfp_hip's kernels (csrc/bn_train.hip; include/slfp.h states the order of every
sum): the autograd Function behind fusion.TrainBatchNorm2d.  float32 channels_last tensors on the ROCm device only; there is no
fallback in here -- the module decides with bn_train_supported() and otherwise runs ATen's batch_norm itself.  Also the residual,
table and code forms of the same kernels, the Function that spans BatchNorm -> ReLU -> Conv2d_Q (or BatchNorm -> layer-output
quantizer -> activation -> Conv2d_Q) on 1-byte codes, and the pair that puts a Bottleneck's trunk on codes: the tail that writes
them next to float32 and the Conv2d_Q Function that reads them."""
import numpy as np
import torch
import torch.nn as nn
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


def _call(entry, x, *args):
    """One entry point of csrc/bn_train.hip on x's device and stream: `args` in its order (addresses, None for a null pointer,
    numbers; the caller keeps the tensors behind them alive), then the tail every entry point ends with: geometry, layout,
    workspace and stream."""
    L = _lib.load()
    n, c, h, w = x.shape
    with _on_device(x.device):
        nbytes = L.slfp_bn_train_workspace_bytes(n, h, w, c)
        ws = _workspace(x.device, nbytes)
        _lib.check(getattr(L, entry)(*args, n, h, w, c, _lib.LAYOUT_NHWC, ws.data_ptr(), nbytes, _stream_handle(x)))


def _outputs(x, saves):
    """y (x's channels_last strides) and `saves` per-channel float32 arrays for the forward to fill (x is float32)."""
    c = x.shape[1]
    return [torch.empty_like(x)] + [x.new_empty(c) for _ in range(saves)]


def _grads(ctx, x, save_mean, iw):
    """gx, and ggamma / gbeta where the weight (input `iw`) and the bias behind it need them (None: a null pointer)."""
    need = ctx.needs_input_grad
    return torch.empty_like(x), torch.empty_like(save_mean) if need[iw] else None, torch.empty_like(save_mean) if need[iw + 1] else None


class hip_bn_train(torch.autograd.Function):
    """y = relu?(batch_norm(x)) with batch statistics; running_mean / running_var (both or neither) are updated in place.
    x: channels_last float32 that bn_train_supported() accepts; weight, bias: float32 [C].  Returns y (channels_last).  The
    output is saved for the backward only with `relu` (the mask is read from it): without, the backward does not read y, and
    the caller may change it in place (`out += identity`, a shared nn.ReLU(inplace=True)) as behind the stock module."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps, relu):
        x = x.detach()
        gamma, beta = _vec(weight), _vec(bias)
        y, save_mean, save_invstd = _outputs(x, 2)
        _call("slfp_bn_train_fwd", x, x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(running_mean), _ptr(running_var),
              float(momentum), float(eps), 1 if relu else 0, y.data_ptr(), save_mean.data_ptr(), save_invstd.data_ptr())
        ctx.relu = bool(relu)
        ctx.save_for_backward(x, weight, save_mean, save_invstd, *((y,) if ctx.relu else ()))
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, weight, save_mean, save_invstd = ctx.saved_tensors[:4]
        y = ctx.saved_tensors[4] if ctx.relu else x   # relu == 0: y is not read; any valid pointer stands in
        gy, gamma = _nhwc(gy), _vec(weight)
        gx, ggamma, gbeta = _grads(ctx, x, save_mean, 1)
        _call("slfp_bn_train_bwd", x, x.data_ptr(), y.data_ptr(), gy.data_ptr(), gamma.data_ptr(), save_mean.data_ptr(),
              save_invstd.data_ptr(), 1 if ctx.relu else 0, gx.data_ptr(), _ptr(ggamma), _ptr(gbeta))
        return gx if ctx.needs_input_grad[0] else None, ggamma, gbeta, None, None, None, None, None


# ---- BatchNorm2d -> residual add -> ReLU (slfp_bn_res_train_fwd / _bwd) -----------------------------------
# The size rule of the residual form, by the spread rule of sections 27 and 32: the smallest size class from which this class and
# every larger measured one beat the stock tail (BatchNorm, `+=`, ReLU) by more than the stock leg's round-to-round spread.
# Read from profiles/bn_res_train_bench.json (forward + backward of the tail, ResNet-50's trunk shapes at batch 64 and 128):
#   elements (N C H W)   rows                                   stock ms         kernels ms       speed-up     beyond spread
#   98.00 M              128 x 56x56x256                        1.259            0.979            1.29         yes
#   49.00 M              64 x 56x56x256, 128 x 28x28x512        0.638, 0.605     0.540, 0.500     1.18, 1.21   yes, yes
#   24.50 M              64 x 28x28x512, 128 x 14x14x1024       0.264, 0.274     0.235, 0.225     1.12, 1.22   yes, yes
#   12.25 M              64 x 14x14x1024, 128 x 7x7x2048        0.152, 0.176     0.218, 0.121     0.70, 1.46   no, yes
#    6.12 M              64 x 7x7x2048                          0.151            0.218            0.69         no
# (M = 2^20.)  A second run (profiles/bn_res_train_bench_second.json) repeated the three classes from 24.5 M on within 4 % and had
# both 12.25 M rows ahead (1.20x, 1.56x) and 6.12 M behind (0.93x): at 12.25 M and below the six launches issued from Python sit on
# the host's floor, 0.11-0.22 ms from one round to the next, and a class that missed in one run of two stays out.  So the module
# leaves tails of fewer than 24 M elements to ATen unless told otherwise (min_elements=0): of ResNet-50's trunk at batch 64 that
# admits layer1 and layer2, at batch 128 layer3 too.
RES_MIN_ELEMENTS = 24 << 20


class hip_bn_res_train(torch.autograd.Function):
    """y = relu?(batch_norm(x) + res) with batch statistics: the tail of a Bottleneck (bn3, `out += identity`, the shared ReLU) in
    the two passes of hip_bn_train; running_mean / running_var are updated in place.  x, res: float32 of one shape, x channels_last
    as bn_train_supported() accepts it (res is made so).  Saved for the backward: x, weight, save_mean, save_invstd and, with
    `relu`, y (the mask is read from it).  The residual's gradient is g = relu ? (y > 0 ? gy : 0) : gy: with relu it is a second
    store of the dx pass, asked for only if res needs a gradient; without, gy itself is handed on."""

    @staticmethod
    def forward(ctx, x, res, weight, bias, running_mean, running_var, momentum, eps, relu):
        return _bn_res_forward(ctx, "hip_bn_res_train", x, res, weight, bias, running_mean, running_var, momentum, eps, relu)[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        return _bn_res_backward(ctx, gy) + (None,) * 5


def _bn_res_forward(ctx, who, x, res, weight, bias, running_mean, running_var, momentum, eps, relu, quant=None):
    """The forward of the residual form and, with quant = (ka, q_bit), of the residual-and-codes form: the same call with the
    quantizer behind `relu` and the code tensor behind y.  Saves what _bn_res_backward reads; returns (y, codes or None)."""
    if res.shape != x.shape or res.dtype != x.dtype or res.device != x.device:
        raise ValueError(f"{who}: the residual must have x's shape, dtype and device")
    x = x.detach()
    res = _nhwc(res.detach())
    gamma, beta = _vec(weight), _vec(bias)
    y, save_mean, save_invstd = _outputs(x, 2)
    head = (x.data_ptr(), res.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(running_mean), _ptr(running_var), float(momentum),
            float(eps), 1 if relu else 0)
    codes = None
    if quant is None:
        _call("slfp_bn_res_train_fwd", x, *head, y.data_ptr(), save_mean.data_ptr(), save_invstd.data_ptr())
    else:
        codes = torch.empty(x.shape, dtype=torch.uint8, device=x.device, memory_format=torch.channels_last)
        _call("slfp_bn_res_codes_train_fwd", x, *head, float(quant[0]), int(quant[1]), y.data_ptr(), codes.data_ptr(),
              save_mean.data_ptr(), save_invstd.data_ptr())
    ctx.relu = bool(relu)
    ctx.save_for_backward(x, weight, save_mean, save_invstd, *((y,) if ctx.relu else ()))
    return y, codes


def _bn_res_backward(ctx, gy):
    """(gx, gres, ggamma, gbeta) of slfp_bn_res_train_bwd from what hip_bn_res_train.forward saved: the backward of the residual
    form and of the residual-and-codes form, whose inputs both start (x, res, weight, bias)."""
    x, weight, save_mean, save_invstd = ctx.saved_tensors[:4]
    y = ctx.saved_tensors[4] if ctx.relu else x   # relu == 0: y is not read; any valid pointer stands in
    gy, gamma = _nhwc(gy), _vec(weight)
    gx, ggamma, gbeta = _grads(ctx, x, save_mean, 2)
    gres = None
    if ctx.needs_input_grad[1]:
        gres = torch.empty_like(x) if ctx.relu else gy   # relu == 0: g is gy itself, no copy is asked of the kernel
    _call("slfp_bn_res_train_bwd", x, x.data_ptr(), y.data_ptr(), gy.data_ptr(), gamma.data_ptr(), save_mean.data_ptr(),
          save_invstd.data_ptr(), 1 if ctx.relu else 0, gx.data_ptr(), _ptr(gres) if ctx.relu else None, _ptr(ggamma),
          _ptr(gbeta))
    return gx if ctx.needs_input_grad[0] else None, gres, ggamma, gbeta


# ---- BatchNorm2d -> layerout_quantize_func -> activation (slfp_bn_lut_train_fwd / _bwd) -------------------
# The size rule of the table form, read from profiles/bn_layerout_train_bench.json with the spread rule of sections 12 and 27: a
# size class is on the kernels by default only if forward + backward of the swapped block beat the stock modules by more than
# the stock leg's round-to-round spread.  Every shape of 12.25 M elements (N C H W) and more did, by 1.9x to 3.4x.  Below, both
# legs sit on the host's launch floor (0.10 ms for the block's six launches, 0.11-0.26 ms for the stock dozen): the block was
# faster on most shapes (up to 2.4x at 6 M elements), but the floor itself moved between 0.10 and 0.19 ms from one round to
# the next, and over three runs of the benchmark shapes of 0.5, 1, 2, 3, 4 and 8 M elements each missed the rule in one run or
# another (the two earlier runs: profiles/bn_layerout_train_bench_earlier.json).  The module leaves those tensors to ATen unless told otherwise (min_elements=0).
LUT_MIN_ELEMENTS = 12 << 20


def _lut_act_types():
    from . import activation_func as af
    return (nn.ReLU, nn.GELU, nn.SiLU, nn.Sigmoid, af.Swish, af.Sigmoid)


def layerout_act_tables(acts, device):
    """(F, D) for the activation modules `acts` behind a layer-output quantizer: two float32 tensors of _lib.LAYEROUT_TABLE_FLOATS
    entries on `device` (a CPU device too), indexed by layer-output class (slfp_layerout_lut_values; index 0 is NaN).  F is the
    stock modules applied in order to the class values, D the modules' own derivative there: autograd's gradient of F.sum().
    Padding slots are 0 in both.  Accepted, by exact type: nn.ReLU, nn.GELU, nn.SiLU, nn.Sigmoid, activation_func.Swish /
    Sigmoid.  activation_func.STL is refused: its backward is a function of the incoming gradient, not a derivative at the
    input.  As a guard the gradient is taken with ones and with twos upstream; the second must be twice the first wherever both
    are finite, or the modules' backward is no multiplication by a table."""
    acts = list(acts)
    for act in acts:
        if type(act) not in _lut_act_types():
            raise TypeError(f"layerout_act_tables: {type(act).__name__} is not an elementwise activation with a derivative table "
                            "(nn.ReLU, nn.GELU, nn.SiLU, nn.Sigmoid, activation_func.Swish, activation_func.Sigmoid)")
    n = _lib.LAYEROUT_TABLE_FLOATS
    L = _lib.load()
    vals = np.zeros(n, dtype=np.float32)
    _lib.check(L.slfp_layerout_lut_values(vals.ctypes.data, n))
    classes = L.slfp_layerout_lut_classes()
    v = torch.from_numpy(vals).to(device).requires_grad_(True)
    with torch.enable_grad():
        f = v.clone()
        for act in acts:
            f = act(f.clone())   # (an in-place module writes into the copy)
        if not torch.is_tensor(f) or f.shape != (n,) or f.dtype != torch.float32:
            raise RuntimeError("layerout_act_tables: an activation module did not return an elementwise float32 result")
        if acts:
            d1, = torch.autograd.grad(f, v, torch.ones_like(f), retain_graph=True)
            d2, = torch.autograd.grad(f, v, torch.full_like(f, 2.0))
        else:
            d1, d2 = torch.ones_like(f), torch.full_like(f, 2.0)
    both = torch.isfinite(d1) & torch.isfinite(d2)
    if not torch.equal(d2[both], (2.0 * d1)[both]):
        raise RuntimeError("layerout_act_tables: the modules' backward is not linear in the incoming gradient")
    F, D = f.detach().clone(), d1.detach().clone()
    F[classes:] = 0
    D[classes:] = 0
    return F.contiguous(), D.contiguous()


def _layerout_values():
    """(class values as a float32 numpy array of _lib.LAYEROUT_LUT_BYTES entries, padding 0; the number of classes)."""
    n = _lib.LAYEROUT_LUT_BYTES
    L = _lib.load()
    vals = np.zeros(n, dtype=np.float32)
    _lib.check(L.slfp_layerout_lut_values(vals.ctypes.data, n))
    return vals, L.slfp_layerout_lut_classes()


def _layerout_code_bytes(acts, ka, q_bit, device, who, relu_first=False):
    """The one builder of a byte table over the layer-output class (fusion._layerout_table for inference, layerout_code_table for
    training): per slot of slfp_layerout_lut_values the reader's extended code of act_k(... act_1(relu?(value)) ...), the stock
    modules themselves run under no_grad on `device`, then hip_encode (NaN -> 0x00, as everywhere on the code path).  relu_first is
    a ReLU folded in front with the kernels' semantics: fmaxf(NaN, 0) is 0 (torch.relu would keep the NaN).  Padding slots are
    treated as the value 0."""
    from .conv2d_func import _act_fmt
    from .sfp_quant import hip_encode
    vals, _ = _layerout_values()
    with torch.no_grad():
        v = torch.from_numpy(vals).to(device)
        if relu_first:
            v = torch.where(v > 0, v, torch.zeros_like(v))
        for act in acts:
            v = act(v.clone())   # (an in-place module writes into the copy)
        if not torch.is_tensor(v) or v.shape != (len(vals),) or v.dtype != torch.float32:
            raise RuntimeError(f"{who}: an activation module did not return an elementwise float32 result")
        return hip_encode(v.contiguous(), ka, _act_fmt(q_bit))


def layerout_code_table(acts, ka, q_bit, device):
    """The uint8 table of _lib.LAYEROUT_LUT_BYTES entries on the ROCm `device` that slfp_bn_lut_codes_train_fwd indexes by
    layer-output class: the extended code, in the reader's quantizer QA(. / ka) of q_bit 8 or 7, of the stock modules `acts` applied
    in order to the class value (slfp_layerout_lut_values -> the modules under no_grad -> hip_encode).  Index 0, the NaN class, is
    0x00; padding slots are 0.  It accepts exactly the module types layerout_act_tables accepts -- the backward needs the
    derivative table of the same modules -- so activation_func.STL is refused."""
    acts = list(acts)
    for act in acts:
        if type(act) not in _lut_act_types():
            raise TypeError(f"layerout_code_table: {type(act).__name__} is not an elementwise activation with a derivative table "
                            "(nn.ReLU, nn.GELU, nn.SiLU, nn.Sigmoid, activation_func.Swish, activation_func.Sigmoid)")
    if q_bit not in (8, 7):
        raise ValueError(f"layerout_code_table: the reader's q_bit must be 8 or 7, got {q_bit}")
    t = _layerout_code_bytes(acts, ka, q_bit, device, "layerout_code_table")
    t[_layerout_values()[1]:] = 0
    return t


class hip_bn_lut_train(torch.autograd.Function):
    """y = act(layerout(batch_norm(x))) with batch statistics, the activation as the table `ftab` over the layer-output class and
    its derivative as `dtab` (layerout_act_tables, on x's device); running_mean / running_var are updated in place.  x:
    channels_last float32 that bn_train_supported() accepts.  Saved for the backward: x, weight, bias, save_mean, save_invstd and
    save_lo -- never y (the class is recomputed from x), so the caller may change y in place behind the module."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps, ftab, dtab):
        x = x.detach()
        gamma, beta = _vec(weight), _vec(bias)
        y, save_mean, save_invstd, save_lo = _outputs(x, 3)
        _call("slfp_bn_lut_train_fwd", x, x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(running_mean), _ptr(running_var),
              float(momentum), float(eps), ftab.data_ptr(), y.data_ptr(), save_mean.data_ptr(), save_invstd.data_ptr(),
              save_lo.data_ptr())
        ctx.dtab = dtab
        ctx.save_for_backward(x, weight, bias, save_mean, save_invstd, save_lo)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, weight, bias, save_mean, save_invstd, save_lo = ctx.saved_tensors
        gy, gamma, beta = _nhwc(gy), _vec(weight), _vec(bias)
        gx, ggamma, gbeta = _grads(ctx, x, save_mean, 1)
        _call("slfp_bn_lut_train_bwd", x, x.data_ptr(), gy.data_ptr(), gamma.data_ptr(), beta.data_ptr(), save_mean.data_ptr(),
              save_invstd.data_ptr(), save_lo.data_ptr(), ctx.dtab.data_ptr(), gx.data_ptr(), _ptr(ggamma), _ptr(gbeta))
        return gx if ctx.needs_input_grad[0] else None, ggamma, gbeta, None, None, None, None, None, None


# ---- BatchNorm2d (+ReLU) -> the next Conv2d_Q on 1-byte codes, in a training step (slfp_bn_codes_train_fwd / _bwd and
# slfp_conv2d_bwd_codes) --------------------------------------------------------------------------------------
# The size rule of the code form, by the spread rule of DESIGN sections 27 and 32: the smallest size class from which this class and
# every larger measured one beat the better of the two unlinked legs (today's kernels, the stock modules) by more than that leg's
# run-to-run spread.  Read from profiles/bn_codes_train_bench.json and its earlier run (MobileNetV1-224's 26 hand-over shapes at
# batch 128, forward + backward of [BN, ReLU, Conv2d_Q], options.backward = "hip"; M = 2^20 elements of the BatchNorm's tensor):
#   98 M, 49 M            every row ahead in both runs, 1.08-1.35x
#   24.5 M                every row ahead in both runs: by only 1.01-1.12x in the earlier, by 1.11-1.25x in the later
#   12.25 M               the stride-2 depthwise row lost in both runs (0.965x, 0.997x), a 1x1 row in one (0.861x)
#   6.12 M                the 7x7 depthwise row lost to the stock modules in both (0.83x), a 1x1 row in one (0.965x)
#   3.06 M                its one row ahead in both (1.05x), under failing classes
# So hand-overs of fewer than 24 M elements stay float32 unless told otherwise (min_elements=0): of MobileNetV1-224's 26 at batch
# 128 the default links 10.  The whole step was fastest with all 26 linked (12.3 ms against 13.6 with the default and 15.1 without):
# DESIGN section 35.
CODES_MIN_ELEMENTS = 24 << 20


class TrainLink:
    """What a TrainBatchNormCodes2d or a TrainBatchNormLayeroutCodes2d hands its Conv2d_Q next to the code tensor (as the tensor
    attribute `_train_link`): the BN's input with its graph, the BN's operands, the three per-channel arrays the forward saved,
    and the quantizer the codes were written for.  The conv takes it off the tensor before it stashes the codes: a finished step
    must not keep x alive."""
    __slots__ = ("x", "weight", "bias", "save_mean", "save_invstd", "save_lo", "relu", "ka", "q_bit", "conv", "dtab")

    def __init__(self, x, weight, bias, saves, relu, ka, q_bit, conv, dtab=None):
        self.x, self.weight, self.bias = x, weight, bias
        self.save_mean, self.save_invstd, self.save_lo = saves
        self.relu, self.ka, self.q_bit, self.conv = bool(relu), ka, q_bit, conv
        # the table form (TrainBatchNormLayeroutCodes2d): the derivative table of the activation behind the layer-output
        # quantizer, which slfp_bn_lut_train_bwd multiplies by; None: the ReLU form, whose backward is slfp_bn_codes_train_bwd
        self.dtab = dtab

    def made_for(self, conv, codes):
        """Were `codes` written for `conv`, and does it still read them?  Its own clause is the identity; the rest is the reader
        check's host-only half: the wrapper that made this record asked the whole check in this same call, library included."""
        from .conv2d_func import _train_codes_reader_matches
        return conv is self.conv and _train_codes_reader_matches(conv, codes, self.ka, self.q_bit)


def bn_codes_train_supported(x, ka, q_bit, min_elements=None):
    """bn_train_supported under the code form's size rule (None: CODES_MIN_ELEMENTS, which may leave everything out), and
    slfp_bn_codes_train_supported for the reader's quantizer (ka: float32(Ka) as a Python float)."""
    return _codes_form_supported(x, min_elements, CODES_MIN_ELEMENTS, "slfp_bn_codes_train_supported", ka, int(q_bit))


def _codes_form_supported(x, floor, default_floor, query_name, *reader):
    """bn_train_supported under a code form's size rule (floor None: `default_floor`, which may itself be None = never), then the
    form's own library query: with the reader's quantizer (`reader` = ka, q_bit) where the form is told it, without for the table
    form, whose table holds it."""
    floor = default_floor if floor is None else floor
    if floor is None or not bn_train_supported(x, floor):
        return False
    n, c, h, w = x.shape
    return bool(getattr(_lib.load(), query_name)(n, h, w, c, _lib.LAYOUT_NHWC, *reader))


def bn_codes_train_fwd(x, weight, bias, running_mean, running_var, momentum, eps, relu, ka, q_bit):
    """slfp_bn_codes_train_fwd on a tensor bn_codes_train_supported accepts, without recording: (codes, save_mean, save_invstd,
    save_lo), codes a uint8 channels_last tensor of x's shape holding relu?(batch_norm(x)) as the extended codes of QA(. / ka);
    the running statistics are updated in place."""
    x = x.detach()
    gamma, beta = _vec(weight), _vec(bias)
    codes = torch.empty(x.shape, dtype=torch.uint8, device=x.device, memory_format=torch.channels_last)
    saves = [x.new_empty(x.shape[1]) for _ in range(3)]
    _call("slfp_bn_codes_train_fwd", x, x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(running_mean), _ptr(running_var),
          float(momentum), float(eps), 1 if relu else 0, float(ka), int(q_bit), codes.data_ptr(), *(t.data_ptr() for t in saves))
    return (codes, *saves)


# ---- BatchNorm2d -> layerout_quantize_func -> activation -> the next Conv2d_Q on 1-byte codes, in a training step
# (slfp_bn_lut_codes_train_fwd, slfp_conv2d_bwd_codes and slfp_bn_lut_train_bwd) -----------------------------
# The size rule of the table-and-codes form, by the spread rule of DESIGN sections 27, 32 and 35: the smallest size class from which
# this class and every larger measured one beat the better unlinked leg by more than that leg's round-to-round spread, in two runs.
# Read from profiles/bn_lut_codes_train_bench.json and its first run (_first.json): the hand-over shapes of vgg16_cifar32 (GELU,
# "hip_all"), mobilenetv1_cifar32 and mobilenetv1_imagenet224 (Swish, "hip") at batch 128 and 256, forward + backward of [BN,
# layerout, act, Conv2d_Q]; the better unlinked leg was the table kernels (use_device_bn_layerout_train(min_elements=0)) on every
# row; M = 2^20 elements of the BatchNorm's tensor; rows ahead beyond the spread in the first, second run of the rows of the
# class; speed-ups of the second run:
#   196 M             1, 1 of 1      1.22x (the stride-2 depthwise reader of 256 x 112x112x64)
#   98 M              5, 5 of 6      1.05-1.22x; the 1x1 32->64 reader at 112x112 BEHIND in both runs (0.989x, 0.989x)
#   49 M              7, 7 of 9      1.03-1.16x; the 1x1 32->64 and 64->128 readers BEHIND in both (0.987x / 0.989x,
#                                    0.981x / 0.978x)
#   24.5 M            7, 7 of 8      1.05-1.17x; the 1x1 64->128 reader at 56x56 BEHIND in both (0.989x, 0.984x)
#   16 M, 8 M, 3.06 M every row ahead in both runs (1.03-1.05x), under failing classes
#   12.25 M           6, 7 of 7      1.04-1.06x; the 7x7 depthwise row behind in the first run (0.984x)
#   6.12 M            3, 3 of 4      the 7x7 depthwise row at batch 128 BEHIND in both (0.883x, 0.900x)
#   4 M and below     most rows BEHIND in both runs, 0.87-0.95x; a few rows ahead by 1-3 %.  (Both legs are ten launches from
#                     Python there; why the linked one is the slower was not measured.)
# So only hand-overs of 196 M elements and more are linked unless told otherwise (min_elements=0): at batch 128 of the CIFAR nets,
# and of MobileNetV1-224, the default links NOTHING.  What loses in the large classes is one kind of row, the 1x1 reader with 32 or
# 64 input channels, by 1-2 %; every depthwise, dense 3x3 and wider 1x1 reader from 8 M elements on was ahead in both runs but the
# 7x7 depthwise one.  The CIFAR steps at batch 128 (hand-overs of 2 M elements and fewer there, 8 M in VGG): MobileNetV1_swish
# 5.00 -> 5.53 ms with all 26 linked (SLOWER), VGG16_gelu 7.20 -> 7.13 ms with all 8.
LUT_CODES_MIN_ELEMENTS = 196 << 20


def bn_lut_codes_train_supported(x, min_elements=None):
    """bn_train_supported under the table-and-codes form's size rule (None: LUT_CODES_MIN_ELEMENTS, which may be None = never), and
    slfp_bn_lut_codes_train_supported (C % 4 == 0).  The reader's quantizer is in the table, not in the query."""
    return _codes_form_supported(x, min_elements, LUT_CODES_MIN_ELEMENTS, "slfp_bn_lut_codes_train_supported")


def bn_lut_codes_train_fwd(x, weight, bias, running_mean, running_var, momentum, eps, code_table):
    """slfp_bn_lut_codes_train_fwd on a tensor bn_lut_codes_train_supported accepts, without recording: (codes, save_mean,
    save_invstd, save_lo), codes a uint8 channels_last tensor of x's shape holding code_table[class of layerout(batch_norm(x))]
    (code_table: layerout_code_table, on x's device); the running statistics are updated in place."""
    x = x.detach()
    gamma, beta = _vec(weight), _vec(bias)
    codes = torch.empty(x.shape, dtype=torch.uint8, device=x.device, memory_format=torch.channels_last)
    saves = [x.new_empty(x.shape[1]) for _ in range(3)]
    _call("slfp_bn_lut_codes_train_fwd", x, x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(running_mean), _ptr(running_var),
          float(momentum), float(eps), code_table.data_ptr(), codes.data_ptr(), *(t.data_ptr() for t in saves))
    return (codes, *saves)


def _codes_conv_forward(conv, codes, weight, bias, who):
    """Conv2d_Q `conv`'s code-reading forward on training codes, with freshly prepared weights (never the cache): the one
    plan-check-launch of both Functions below and of Conv2d_Q's own call where nothing records.  No kernel is an error here."""
    from .conv2d_func import _launch, _train_codes_plan
    plan = _train_codes_plan(conv, codes)
    if not plan.ok:
        raise RuntimeError(f"{who}: no code-reading forward for this layer (slfp_conv2d_codes_supported); undo the training "
                           "code links (fusion.unlink_codes_train, fusion.unlink_layerout_codes_train, "
                           "fusion.unlink_bottleneck_codes_train)")
    return _launch(conv, plan, codes, weight, bias, cache=False)


class hip_bn_codes_conv_train(torch.autograd.Function):
    """conv(relu?(batch_norm(x))) for a pair linked by fusion.link_codes_train, or conv(act(layerout(batch_norm(x)))) for a block
    linked by fusion.link_layerout_codes_train (the link then carries the activation's derivative table, `dtab`), as ONE Function:
    autograd cannot carry a gradient through the uint8 tensor between the two, and the float32 gradient between their backward
    kernels is a temporary.  The inputs are the BN's x, weight and bias and the conv's weight and (scaled) bias; `codes` and `link`
    (TrainLink) are what the BN wrapper produced already.  The forward runs the conv's code-reading forward with freshly prepared
    weights (never the cache: an optimizer steps `.data` unseen); saved are x, the codes, the three per-channel arrays and the
    weights -- 5 bytes per element where the unlinked pair saves x and y -- and the link's table is kept.  The backward runs
    slfp_conv2d_bwd_codes, then on its gx slfp_bn_codes_train_bwd, or slfp_bn_lut_train_bwd with `dtab` where the link has one."""

    @staticmethod
    def forward(ctx, x, bn_weight, bn_bias, weight, bias, conv, codes, link):
        y = _codes_conv_forward(conv, codes, weight, bias, "hip_bn_codes_conv_train")
        ctx.conv, ctx.relu, ctx.has_bias, ctx.dtab = conv, link.relu, bias is not None, link.dtab
        ctx.save_for_backward(x, codes, bn_weight, bn_bias, link.save_mean, link.save_invstd, link.save_lo, weight)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        from .conv2d_func import _conv_desc, _hip_backward_codes
        x, codes, bn_weight, bn_bias, save_mean, save_invstd, save_lo, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        need_bn = need[0] or need[1] or need[2]
        gy = _nhwc(gy)
        g, gw, gb = _hip_backward_codes(ctx.conv, _conv_desc(ctx.conv, codes.shape, True, True), codes, weight, gy,
                                        (need_bn, need[3], ctx.has_bias and need[4]))
        gx = ggamma = gbeta = None
        if need_bn:
            gamma, beta = _vec(bn_weight), _vec(bn_bias)
            gx, ggamma, gbeta = _grads(ctx, x, save_mean, 1)
            head = (x.data_ptr(), g.data_ptr(), gamma.data_ptr(), beta.data_ptr(), save_mean.data_ptr(), save_invstd.data_ptr(),
                    save_lo.data_ptr())
            if ctx.dtab is not None:   # the table form: the class is recomputed from x, g is multiplied by the derivative there
                _call("slfp_bn_lut_train_bwd", x, *head, ctx.dtab.data_ptr(), gx.data_ptr(), _ptr(ggamma), _ptr(gbeta))
            else:
                _call("slfp_bn_codes_train_bwd", x, *head, 1 if ctx.relu else 0, gx.data_ptr(), _ptr(ggamma), _ptr(gbeta))
        return gx if need[0] else None, ggamma, gbeta, gw, gb, None, None, None


# ---- BatchNorm2d -> residual add -> ReLU that writes the float32 trunk AND its readers' codes (slfp_bn_res_codes_train_fwd;
# DESIGN section 38) ---------------------------------------------------------------------------------------------------------------
# The size rule of the residual-and-codes form, by the spread rule of sections 27-35: the smallest size class from which this class
# and every larger measured one beat the better unlinked leg by more than that leg's round-to-round spread, in two runs.
# Read from profiles/bn_res_codes_train_bench.json and its second run (ResNet-50's trunk shapes at batch 64 and 128, forward +
# backward of [bn3 tail, next conv1 (+ downsample.0)], options.backward = "hip_all"; the better unlinked leg is the residual kernels
# from 24 M elements on and the stock modules below; M = 2^20 elements of the trunk; speed-ups of the first, second run):
#   98 M       both rows ahead in both runs: the boundary row 1.030x, 1.031x, the plain row 1.012x, 1.012x
#   49 M       the two boundary rows ahead (1.008-1.018x), the two plain rows BEHIND in both runs (0.977x, 0.986x; 0.986x, 0.987x)
#   24.5 M     64 x 28x28x512 into conv1 alone behind in both runs (0.991x, 0.994x), the other three rows ahead (1.013-1.028x)
#   12.25 M, 6.12 M   every row ahead (1.045-1.174x) -- against the stock modules, the better unlinked leg there: what wins is
#              mostly the residual kernels the default rule of section 33 leaves out at these sizes -- and under failing classes
# So a trunk of fewer than 98 M elements stays float32 unless told otherwise (min_elements=0): at batch 128 that links the 56 x 56
# trunks of layer1, at batch 64 nothing.  The whole Bottleneck-stack step at batch 64 moved from 15.167 to 15.147 ms with the seven
# trunk links alone and from 14.861 to 14.792 ms on top of the in-block links.
RES_CODES_MIN_ELEMENTS = 98 << 20


def bn_res_codes_train_supported(x, ka, q_bit, min_elements=None):
    """bn_train_supported under the residual-and-codes form's size rule (None: RES_CODES_MIN_ELEMENTS, which may leave everything
    out), and slfp_bn_res_codes_train_supported for the readers' quantizer (ka: float32(Ka) as a Python float)."""
    return _codes_form_supported(x, min_elements, RES_CODES_MIN_ELEMENTS, "slfp_bn_res_codes_train_supported", ka, int(q_bit))


class hip_bn_res_codes_train(torch.autograd.Function):
    """hip_bn_res_train that also returns y as the uint8 channels_last extended codes of QA(y / ka), the quantizer of the Conv2d_Q
    layers that read the trunk (slfp_bn_res_codes_train_fwd): (y, codes), the codes not differentiable.  y is bit for bit
    hip_bn_res_train's and is what the backward reads, so the backward is hip_bn_res_train's own.  Saved for the backward is what
    hip_bn_res_train saves; the codes belong to the readers (hip_trunk_codes_conv_train)."""

    @staticmethod
    def forward(ctx, x, res, weight, bias, running_mean, running_var, momentum, eps, relu, ka, q_bit):
        y, codes = _bn_res_forward(ctx, "hip_bn_res_codes_train", x, res, weight, bias, running_mean, running_var, momentum, eps,
                                   relu, (ka, q_bit))
        ctx.mark_non_differentiable(codes)
        return y, codes

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, _gcodes):
        return _bn_res_backward(ctx, gy) + (None,) * 7


class hip_trunk_codes_conv_train(torch.autograd.Function):
    """conv(trunk) for a Conv2d_Q that reads a trunk linked by fusion.link_bottleneck_codes_train: `codes` are the trunk as the
    extended codes of this conv's own quantizer, written by hip_bn_res_codes_train.  The differentiable inputs are the float32
    trunk (never read), the conv's weight and (scaled) bias.  The forward is the conv's code-reading forward with freshly prepared
    weights (never the cache: an optimizer steps `.data` unseen); saved are the codes and the weight, never the float32 tensor.  The
    backward is slfp_conv2d_bwd_codes; its gx is the trunk's gradient, which autograd adds to the next tail's."""

    @staticmethod
    def forward(ctx, trunk, weight, bias, conv, codes):
        y = _codes_conv_forward(conv, codes, weight, bias, "hip_trunk_codes_conv_train")
        ctx.conv, ctx.has_bias = conv, bias is not None
        ctx.save_for_backward(codes, weight)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        from .conv2d_func import _conv_desc, _hip_backward_codes, _needs
        codes, weight = ctx.saved_tensors
        gx, gw, gb = _hip_backward_codes(ctx.conv, _conv_desc(ctx.conv, codes.shape, True, True), codes, weight, _nhwc(gy), _needs(ctx))
        return gx, gw, gb, None, None
