"""Host-side mirror of the reference's utils/conv2d_func.py on top of the HIP C ABI.

Drop-in operator API (same names, positional order, attributes and state-dict keys):

    conv2d_Q(q_bit, Kw, Ka)       -> class Conv2d_Q(nn.Conv2d)   utils/conv2d_func.py:8-26
    conv2d_Q_bias(q_bit, Kw, Ka)  -> class Conv2d_Q(nn.Conv2d)   utils/conv2d_func.py:28-48
    linear_Q(q_bit, Kw, Ka)       -> class Linear_Q(nn.Linear)   utils/conv2d_func.py:50-66

Where the reference runs  x/Ka -> ~25-pass quantize_act -> w/Kw -> ~25-pass
quantize_weight (every forward) -> fp32 F.conv2d -> *Ka*Kw  (conv2d_func.py:20-25), this
module makes ONE call into libslfp_hip.so (slfp_conv2d_fwd): the SLFP encode is applied
inline on the kernels' load path; `input_q` / `weight_q` -- which the CIFAR nets read back
after every forward (nets_cifar/mobilenetv1.py:88-171) -- are materialised lazily on first
access.

Weights: the reference re-quantizes them on EVERY forward (utils/conv2d_func.py:22).  So does
this module whenever the weights can change under it: in training mode, and whenever autograd
is recording -- the reference's own optimizers update `p.data` in place (utils/optimizer.py:
58-63), which does not bump `weight._version`, so no version key can see it.  Only in
inference (`module.eval()` and `torch.no_grad()`/`inference_mode`) is the kernel-specific
weight blob cached, keyed on storage, `_version`, shape, scales and kernel; every
`module.train(...)` / `.eval()` call and `invalidate()` drop it.

Memory layout: the kernels are NHWC.  A `torch.channels_last` input is consumed and
produced in place (zero copies; BN/ReLU keep the format); an NCHW-contiguous input is
transposed inside the C ABI and, by default, the output comes back NCHW so that code
which `.view()`s NCHW strides (nets_cifar/shufflenet_v2.py:41) keeps working.  Use
`model.to(memory_format=torch.channels_last)` + a channels_last input for the fast path.

There is no CPU compute path here (q_bit 8/7 need a ROCm tensor; q_bit 32 is the
reference's passthrough).  Autograd: forward is always the HIP kernel.  Backward follows
`options.backward`: "composite" (the default) is the reference's STE composite on the GPU
(torch.nn.grad on the quantized operands); "hip" runs the 3x3 depthwise, stride-1 1x1 and
Linear_Q layers through one slfp_conv2d_bwd call each (float32 accumulation, deterministic;
`module._last_bwd_kernel` names what ran) and keeps every other layer on the composite;
"hip_all" is "hip" plus SLFP_BWD_DENSE: every other groups-1, dilation-1 layer (dense k x k,
strided 1x1, the C_in = 3 stems) runs on the implicit-GEMM family `dense_bwd_mfma_f32`, and
only grouped non-depthwise and dilated layers stay on the composite.
"""
import contextlib
import ctypes

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .sfp_quant import *  # noqa: F401,F403  (the reference re-exports these: conv2d_func.py:5)
from .sfp_quant import (_require_gpu_f32, _stream_handle, hip_quantize, hip_encode, hip_decode, weight_quantize_func,
                        act_quantize_func)

__all__ = ["torch", "nn", "F", "np", "conv2d_Q", "conv2d_Q_bias", "linear_Q", "options",
           "quantize_weight", "quantize_act", "quantize_layerout",
           "weight_quantize_func", "act_quantize_func", "layerout_quantize_func"]


class _Options:
    """Process-wide knobs of the HIP path (not part of the reference API)."""
    mfma_passes = _lib.MFMA_DEFAULT  # pointwise MFMA operand precision, see include/slfp.h
    output_layout = "same"           # "same": follow the input's memory format; "nhwc": always channels_last
    eager_stash = False              # True: materialise input_q / weight_q on every forward like the reference
    plan_cache = True                # False: rebuild descriptor / shapes / workspace on every call (host-overhead A/B)
    dwpw_all = False                 # True: fusion.DwPwBlock uses the one-kernel form wherever the library supports it,
                                     # not only where it measured faster than two kernels
    dwpw_pairs = {(32, 1)}           # (depthwise channels, stride) pairs that run as one kernel by default
    dwpw_codes_pairs = set()         # the same for a linked pair on 1-byte codes (slfp_dwpw_fwd_codes): none by default, see the
                                     # measurements of profiles/dwpw_codes_bench.py; dwpw_all forces every supported pair here too
    backward = "composite"           # "composite": the reference's STE composite; "hip": slfp_conv2d_bwd where it covers the layer
                                     # (3x3 depthwise, stride-1 1x1, Linear_Q); "hip_all": also the dense family (SLFP_BWD_DENSE)
    linear_kernel = "pointwise"      # "pointwise": Linear_Q in inference is a 1x1 convolution over the batch (slfp_linear_fwd_prepared);
                                     # "fc": the weight-streaming kernel (slfp_linear_fwd_fc) wherever slfp_linear_fc_supported
                                     # says yes -- the same bits.  A Linear_Q linked by fusion.link_head runs "fc" either way

    def __setattr__(self, name, value):
        if name == "backward" and value not in _BACKWARDS:
            raise ValueError(f"options.backward must be one of {_BACKWARDS}, got {value!r}")
        if name == "linear_kernel" and value not in _LINEAR_KERNELS:
            raise ValueError(f"options.linear_kernel must be one of {_LINEAR_KERNELS}, got {value!r}")
        super().__setattr__(name, value)


_BACKWARDS = ("composite", "hip", "hip_all")
_LINEAR_KERNELS = ("pointwise", "fc")
options = _Options()


def _f32(v):
    """float32(K) as a Python float: the cast ATen applies to the 0-dim float64 scale."""
    return float(np.float32(float(v)))


def _scalar_scale(t, name):
    if t.numel() != 1:
        raise ValueError(f"{name} must be a scalar calibration scale, got a tensor of shape {tuple(t.shape)} "
                         "(pass the per-layer value, as the reference nets do)")
    v = float(t)
    if not v > 0:
        raise ValueError(f"{name} must be > 0, got {v}")
    return v


def _scale_key(t, name):
    """The scale as a Python float for the plan key (validated like _scalar_scale, without its tensor round trip)."""
    if torch.is_tensor(t):
        if t.numel() != 1:
            _scalar_scale(t, name)
        return t.item()
    return float(t)


def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def _act_fmt(q_bit):
    return _lib.FMT_ACT8 if q_bit == 8 else _lib.FMT_SFP7


def _w_fmt(q_bit):
    return _lib.FMT_W8 if q_bit == 8 else _lib.FMT_SFP7


def _conv_desc(mod, shape, nhwc_in=True, nhwc_out=True):
    """The C ABI's descriptor of module `mod` on an input of `shape` (N, C, H, W) in the given layouts: the one place that
    spells the struct's fields.  A Linear_Q is the pointwise geometry (1x1, stride 1, no padding) with H = W = 1."""
    n, c, h, w = shape
    if isinstance(mod, nn.Linear):
        c_out, kh, kw, groups = mod.out_features, 1, 1, 1
        sh = sw = dh = dw = 1
        ph = pw = 0
    else:
        if isinstance(mod.padding, str) or mod.padding_mode != "zeros":
            raise NotImplementedError("Conv2d_Q (HIP): only explicit zero padding is supported")
        c_out, groups = mod.out_channels, mod.groups
        (kh, kw), (sh, sw), (ph, pw), (dh, dw) = mod.kernel_size, _pair(mod.stride), _pair(mod.padding), _pair(mod.dilation)
    return _lib.ConvDesc(n=n, c_in=c, h=h, w=w, c_out=c_out, kh=kh, kw=kw, stride_h=sh, stride_w=sw, pad_h=ph, pad_w=pw,
                         dil_h=dh, dil_w=dw, groups=groups,
                         x_layout=_lib.LAYOUT_NHWC if nhwc_in else _lib.LAYOUT_NCHW,
                         y_layout=_lib.LAYOUT_NHWC if nhwc_out else _lib.LAYOUT_NCHW,
                         qbits=mod.q_bit, ka=_f32(_scalar_scale(mod.Ka, "Ka")), kw_scale=_f32(_scalar_scale(mod.Kw, "Kw")),
                         mfma_passes=options.mfma_passes, reserved=0)


def _conv_io(x_codes, out):
    """slfp_conv2d_fwd_codes' io struct: does the layer read 1-byte codes, and `out` = (Ka, q_bit) of the layer it writes
    codes for (None: float32 out)."""
    return _lib.ConvIo(x_codes=1 if x_codes else 0, y_codes=1 if out is not None else 0,
                       y_ka=_f32(out[0]) if out is not None else 1.0, y_qbits=int(out[1]) if out is not None else 8)


def _ready_event(stream, cache):
    """The event that users of a cached blob on other streams wait on: recorded on the preparing stream right after the
    prepare.  None when the blob is not kept for reuse (cache=False) or was written inside a hipGraph capture (an event
    recorded there cannot be waited on outside it); a hit from another stream then prepares the blob again."""
    if not cache or torch.cuda.is_current_stream_capturing():
        return None
    ev = torch.cuda.Event()
    ev.record(stream)
    return ev


def _hit_from_other_stream(blob, ready, synced, stream):
    """A cache hit on `stream`, which did not prepare `blob`: the stream waits for the prepare, and the blob's memory is
    tied to it (record_stream), once per stream and blob.  Skipped while capturing: GraphedModule warms the cache up
    before the capture and torch.cuda.graph synchronises on entry, so the blob is complete by then."""
    h = stream.cuda_stream
    if h in synced or torch.cuda.is_current_stream_capturing():
        return
    stream.wait_event(ready)
    blob.record_stream(stream)
    synced.add(h)


class _PreparedWeights:
    """Per-module cache of the kernel-specific weight blob (and, for a conv, the OIHW weight_q tensor).  The blob is
    written on the stream that missed the cache; a hit from another stream (streams.forward_image_groups) waits for it
    there.  What fills the blob is the caller's business (_conv_weights, _hip_linear)."""

    def __init__(self):
        self.invalidate()

    def invalidate(self):
        self.key = None       # (device, data_ptr, weight._version, shape, q_bit, Kw, kernel or precision)
        self.blob = None
        self.weight_q = None
        self.stream = None    # handle of the stream that wrote the blob
        self.ready = None     # event recorded there after the prepare (_ready_event)
        self.synced = set()   # handles of the other streams that have waited on `ready`

    @property
    def weight_version(self):
        """`weight._version` of the cached blob (None: nothing cached)."""
        return None if self.key is None else self.key[2]

    def get(self, key, stream, cache, make, want_weight_q=False):
        """The prepared blob for `key`, usable on `stream`.  On a miss -- and always with cache=False -- make(stream handle)
        allocates and fills a new one and returns (blob, weight_q or None)."""
        h = stream.cuda_stream
        if (not cache or key != self.key or self.blob is None or (want_weight_q and self.weight_q is None)
                or (h != self.stream and self.ready is None)):
            blob, wq = make(h)
            self.key, self.blob, self.weight_q = key, blob, wq
            self.stream, self.ready, self.synced = h, _ready_event(stream, cache), set()
        elif h != self.stream:
            _hit_from_other_stream(self.blob, self.ready, self.synced, stream)
        return self.blob


def _conv_weights(mod, desc, weight, stream, cache, kernel=None, want_weight_q=False):
    """Conv2d_Q's prepared weight blob for `desc` on `stream`, through the module's cache."""
    def make(h):
        L = _lib.load()
        w = weight.detach()
        w = w if w.is_contiguous() else w.contiguous()  # OIHW
        blob = torch.empty(L.slfp_conv2d_wprep_bytes(ctypes.byref(desc)), dtype=torch.uint8, device=weight.device)
        wq = torch.empty_like(w) if want_weight_q else None
        _lib.check(L.slfp_conv2d_prepare_weights(ctypes.byref(desc), w.data_ptr(), blob.data_ptr(),
                                                 _ptr(wq), h))
        return blob, wq

    key = (weight.device, weight.data_ptr(), weight._version, weight.shape, desc.qbits, desc.kw_scale,
           kernel if kernel is not None else _lib.load().slfp_conv2d_kernel_name(ctypes.byref(desc)))
    return mod._prep.get(key, stream, cache, make, want_weight_q)


# What a forward can be asked for besides the float32 interface (kind None): kind -> (support query, forward entry point).
_KINDS = {
    None: (None, "slfp_conv2d_fwd_post"),
    "codes": ("slfp_conv2d_codes_supported", "slfp_conv2d_fwd_codes_ws"),          # codes on either side
    "slice": ("slfp_conv2d_codes_slice_supported", "slfp_conv2d_fwd_codes_slice"),  # codes into a channel slice of a wider tensor
    "entry": ("slfp_conv2d_entry_supported", "slfp_conv2d_fwd_entry"),              # float32 in, codes out, pointwise
    "res": ("slfp_conv2d_res_supported", "slfp_conv2d_fwd_res"),                    # a residual operand in the epilogue
    "res_codes": ("slfp_conv2d_res_codes_supported", "slfp_conv2d_fwd_res_codes"),  # the same, and the next block's codes next to y
    "lut": ("slfp_conv2d_codes_lut_supported", "slfp_conv2d_fwd_codes_lut"),        # codes behind the layer-output quantizer: a byte table
    # codes in, float32 out, for a layer whose epilogue ends in the layer-output quantizer (no ReLU behind it): the code kernel runs
    # the affine, slfp_quantize_layerout_f32 the quantizer -- the last layer of a chain linked by fusion.link_layerout
    "codes_lo": ("slfp_conv2d_codes_supported", "slfp_conv2d_fwd_codes_ws"),
    # uint8 pixels + the module's pixel table in (fusion.link_image_u8), float32 or codes out
    "u8": ("slfp_conv2d_u8_supported", "slfp_conv2d_fwd_u8"),
    # codes in, float32 or codes out, for a 1x1 layer in the float32-equivalent mode (options.mfma_passes = 3), which "codes" refuses;
    # tried only on a module fusion.link_codes(x3=True) marked (`_code_x3`)
    "codes_x3": ("slfp_conv2d_codes_x3_supported", "slfp_conv2d_fwd_codes_x3"),
}


def _ptr(t):
    """A tensor's address for the C ABI; None (NULL) for an absent one."""
    return t.data_ptr() if t is not None else None


def _supported(mod, shape, kind, x_codes, out, flags, y_ld=None, desc=None, io=None):
    """Does libslfp_hip run Conv2d_Q `mod` on a channels_last input of `shape` as `kind` (a key of _KINDS): codes in (x_codes) /
    codes out for the layer `out` = (Ka, q_bit) describes (None: float32 out), `flags` in its epilogue ("res": the ReLU behind the
    add), "slice": into a `y_ld`-channel tensor?  desc / io: the structs, where the caller has built them already."""
    d = desc if desc is not None else _conv_desc(mod, shape)
    io = io if io is not None else _conv_io(x_codes, out)
    tail = (int(y_ld),) if kind == "slice" else ()
    query = getattr(_lib.load(), _KINDS[kind][0])
    if kind == "lut":   # the table absorbs the flags; the query takes the pixel stride of the code tensor (C_out: a dense one)
        return bool(query(ctypes.byref(d), ctypes.byref(io), 1 if mod.bias is not None else 0, int(d.c_out)))
    return bool(query(ctypes.byref(d), ctypes.byref(io), 1 if mod.bias is not None else 0, int(flags), *tail))


class _Plan:
    """What one (module, input shape, layout, scales, precision, kind) combination resolves to in the C ABI; for the kinds of
    _KINDS also the io struct and whether libslfp_hip has a kernel for the combination (`ok`)."""
    __slots__ = ("desc", "y_shape", "ws_bytes", "kernel", "kind", "io", "ok", "label", "u8_family")

    def __init__(self, desc, y_shape, ws_bytes, kernel):
        self.desc, self.y_shape, self.ws_bytes, self.kernel = desc, y_shape, ws_bytes, kernel
        self.kind, self.io, self.ok, self.label = None, None, True, kernel   # label: what `_last_kernel` reports
        self.u8_family = None   # kind "u8": the stem family of the byte form ("stem", "small", "rows", "im2row")


def _plan(mod, x, weight, nhwc_in, nhwc_out, codes=None):
    """Everything that depends only on (module geometry, input shape, layouts, scales, precision) is computed once per
    distinct key and kept on the module: descriptor, output shape, workspace size, kernel name.  codes: None for the
    float32 interface, else (kind of _KINDS, does x hold codes, mod._code_out or None, extra) with extra = the channel count of the
    wider tensor for "slice", whether a ReLU follows the add for "res" and "res_codes" (whose `out` is mod._trunk_code_out)."""
    shape = x.shape
    key = (codes, shape, nhwc_in, nhwc_out, _scale_key(mod.Ka, "Ka"), _scale_key(mod.Kw, "Kw"), options.mfma_passes,
           mod.stride, mod.padding, mod.dilation, weight.shape)
    plan = mod._plans.get(key) if options.plan_cache else None
    if plan is None:
        L = _lib.load()
        d = _conv_desc(mod, shape, nhwc_in, nhwc_out)
        if shape[1] != mod.in_channels:
            raise RuntimeError(f"Given groups={mod.groups}, weight of size {list(weight.shape)}, expected input"
                               f"{list(shape)} to have {mod.in_channels} channels, but got {shape[1]} channels instead")
        ho, wo = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(L.slfp_conv2d_out_shape(ctypes.byref(d), ctypes.byref(ho), ctypes.byref(wo)))
        plan = _Plan(d, (d.n, d.c_out, ho.value, wo.value), L.slfp_conv2d_workspace_bytes(ctypes.byref(d)),
                     L.slfp_conv2d_kernel_name(ctypes.byref(d)).decode())
        if codes is not None:
            kind, x_codes, out, extra = codes
            flags = int(mod._post[2]) if mod._post is not None else 0
            plan.kind, plan.io = kind, _conv_io(x_codes, out)
            if kind in ("res", "res_codes"):
                # an epilogue ReLU or layer-output quantizer would sit BEFORE the add: not what the residual kernels compute
                plan.ok = flags == 0 and _supported(mod, shape, kind, x_codes, out, 1 if extra else 0, desc=d, io=plan.io)
            elif kind == "codes_lo":
                # fma(r, scale, shift) from the code kernel, then the quantizer: what the fused float32 epilogue computes, step for step
                plan.ok = flags == 2 and mod._post[0] is not None and _supported(mod, shape, kind, True, None, 0, desc=d, io=plan.io)
            elif kind == "lut":
                # the table stands for layer-output quantizer + activation + the reader's quantizer: the epilogue must carry the former
                plan.ok = bool(flags & 2) and mod._post[0] is not None and _supported(mod, shape, kind, x_codes, out, flags, desc=d, io=plan.io)
            else:
                plan.ok = _supported(mod, shape, kind, x_codes, out, flags, extra, d, plan.io)
            if kind in ("entry", "codes_x3") or (kind == "codes" and not plan.ok):
                plan.ws_bytes = 0   # pointwise: no workspace; refused: the float32 interface's own plan sizes its workspace
            plan.label += (("+codes_in" if x_codes else "") + ("+codes_out" if out is not None and kind != "res_codes" else "")
                           + {"slice": "+slice", "res": "+res", "res_codes": "+res+trunk_codes", "lut": "+lut", "codes_lo": "+layerout_pass",
                              "u8": "+u8", "codes_x3": "+x3"}.get(kind, ""))
            if kind == "u8" and plan.ok:   # what the launch consumes, from the library's own selection
                inst = L.slfp_debug_stem_u8_instance(ctypes.byref(d), ctypes.byref(plan.io), 1 if mod.bias is not None else 0, flags,
                                                     1 if mod._post is not None and mod._post[0] is not None else 0).decode()
                plan.label += ":" + inst
                plan.u8_family = inst.split("/", 1)[0]
        if len(mod._plans) >= 64:   # a net fed ever-changing shapes: do not grow without bound
            mod._plans.clear()
        mod._plans[key] = plan
    return plan


def _epilogue_args(mod, bias, device):
    """(bias or None, post scale, post shift, flags) as the kernels' epilogue takes them on `device`.  mod._post is the
    (scale, shift, flags) set by fusion.fuse_bn_relu: eval-BN (+ layerout) + ReLU in the epilogue; its two vectors are
    moved to the device once."""
    if bias is not None:
        bias = bias.detach()
        bias = bias if bias.is_contiguous() else bias.contiguous()
    if mod._post is None:
        return bias, None, None, 0
    ps, psh, flags = mod._post
    if ps is not None and ps.device != device:
        ps, psh = ps.to(device), psh.to(device)
        mod._post = (ps, psh, flags)
    return bias, ps, psh, int(flags)


_workspaces = {}
_same_device = contextlib.nullcontext()


def _on_device(device):
    """torch.cuda.device(device) only when it is not the current one already (the guard costs ~5 us per call)."""
    return _same_device if device.index == torch.cuda.current_device() else torch.cuda.device(device)


def _workspace(device, nbytes):
    """Scratch for the kernels that need one (the dense path's pre-encoded input), reused across calls: one buffer per
    (device, stream), grown to the largest request.  Calls on one stream are ordered, so consecutive layers can share
    it; a different stream gets its own.  Under hipGraph capture a fresh tensor is taken from the graph's pool instead
    (the captured pointer must stay valid for the graph's lifetime)."""
    if torch.cuda.is_current_stream_capturing() or not options.plan_cache:
        return torch.empty(nbytes, dtype=torch.uint8, device=device)
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _workspaces[key] = buf
    return buf


def _launch(mod, plan, x, weight, bias, y=None, cache=True, res=None, relu=None, y_ld=None):
    """The one call into libslfp_hip of a Conv2d_Q forward: plan.kind's entry point (_KINDS) on input `x`.  y: the output tensor --
    allocated here (channels_last; uint8 where the plan's io writes codes) when None -- or, for "slice", the address of the
    slice's first channel in a y_ld-channel tensor; "res" / "res_codes": + `res`, with `relu` behind the add ("res_codes": y is float32
    and the codes go into a uint8 tensor of their own, returned with y as a pair).  Does the device guard, the
    stream, the module's weight blob (cache: it may come from the module's cache), the epilogue arguments and the workspace, then
    the module's bookkeeping: `_last_kernel`, exactly one of `_last_input` / `_last_codes`, and `_input_q` (stored by the float32
    interface under options.eager_stash, otherwise made on first read).  Returns y."""
    kind, d = plan.kind, plan.desc
    stash = kind is None and options.eager_stash
    with _on_device(x.device):
        stream = torch.cuda.current_stream(x.device)
        # cache the prepared weights only where they cannot change unseen: inference (see the module docstring)
        blob = _conv_weights(mod, d, weight, stream, cache, plan.kernel, want_weight_q=stash)
        if y is None:
            y = torch.empty(plan.y_shape, dtype=torch.uint8 if plan.io.y_codes and kind != "res_codes" else torch.float32,
                            device=x.device, memory_format=torch.channels_last)
        yc = (torch.empty(plan.y_shape, dtype=torch.uint8, device=x.device, memory_format=torch.channels_last)
              if kind == "res_codes" else None)
        ws = _workspace(x.device, plan.ws_bytes) if plan.ws_bytes else None
        b, ps, psh, flags = _epilogue_args(mod, bias, x.device)
        if kind == "codes_lo":
            flags = 0   # the kernel stops behind the affine; the quantizer is the pass below
        xq = torch.empty_like(x) if stash else None
        head = (x.data_ptr(), blob.data_ptr(), _ptr(b), _ptr(ps), _ptr(psh))
        if kind is None:
            args = (ctypes.byref(d),) + head + (flags, y.data_ptr(), _ptr(xq), _ptr(ws))
        elif kind == "slice":
            args = (ctypes.byref(d), ctypes.byref(plan.io)) + head + (flags, y, y_ld, _ptr(ws))
        elif kind == "res":
            args = (ctypes.byref(d), ctypes.byref(plan.io)) + head + (1 if relu else 0, res.data_ptr(), y.data_ptr(), None)
        elif kind == "res_codes":
            args = (ctypes.byref(d), ctypes.byref(plan.io)) + head + (1 if relu else 0, res.data_ptr(), y.data_ptr(), yc.data_ptr(), None)
        elif kind == "u8":   # x: pixel bytes, then the module's pixel table
            args = (ctypes.byref(d), ctypes.byref(plan.io), x.data_ptr(), mod._image_table.data_ptr()) + head[1:] + (flags, y.data_ptr(), _ptr(ws))
        elif kind == "lut":   # no flags: the ReLU bit is part of the table
            args = (ctypes.byref(d), ctypes.byref(plan.io)) + head + (mod._code_lut.data_ptr(), y.data_ptr(), int(d.c_out), _ptr(ws))
        else:   # "codes" takes a workspace, "entry" and "codes_x3" do not
            args = (ctypes.byref(d), ctypes.byref(plan.io)) + head + (flags, y.data_ptr()) + ((_ptr(ws),) if kind not in ("entry", "codes_x3") else ())
        _lib.check(getattr(_lib.load(), _KINDS[kind][1])(*args, stream.cuda_stream))
        if kind == "codes_lo":
            t, y = y, torch.empty_like(y)
            _lib.check(_lib.load().slfp_quantize_layerout_f32(t.data_ptr(), y.data_ptr(), t.numel(), stream.cuda_stream))
    x_codes = x.dtype == torch.uint8 and kind != "u8"
    # plain attributes, written in one go (nn.Module.__setattr__ costs microseconds per name, on every layer of every forward)
    mod.__dict__.update(_last_kernel=plan.label, _last_input=None if x.dtype == torch.uint8 else x.detach(),
                        _last_codes=x.detach() if x_codes else None, _last_pixels=x.detach() if kind == "u8" else None, _input_q=xq)
    return y if yc is None else (y, yc)


def _hip_conv2d(mod, x, weight, bias, cache_ok=False):
    """One slfp_conv2d_fwd call for module `mod` (an nn.Conv2d subclass below).  cache_ok: the prepared weights may
    come from the module's cache (decided by the caller: grad mode is off inside autograd.Function.forward)."""
    _require_gpu_f32(x, "Conv2d_Q")
    if weight.device != x.device:
        raise RuntimeError(f"Conv2d_Q: input is on {x.device} but weight is on {weight.device}")
    squeeze = x.dim() == 3
    if squeeze:
        x = x.unsqueeze(0)
    if x.dim() != 4:
        raise RuntimeError(f"Expected 3D (unbatched) or 4D (batched) input to conv2d, but got input of size: {list(x.shape)}")
    nhwc_in = x.is_contiguous(memory_format=torch.channels_last)
    if not nhwc_in and not x.is_contiguous():
        x = x.contiguous()
    nhwc_out = nhwc_in or options.output_layout == "nhwc"
    plan = _plan(mod, x, weight, nhwc_in, nhwc_out)
    y = torch.empty(plan.y_shape, dtype=torch.float32, device=x.device,
                    memory_format=torch.channels_last if nhwc_out else torch.contiguous_format)
    _launch(mod, plan, x, weight, bias, y, cache=cache_ok)
    return y.squeeze(0) if squeeze else y


def _hip_conv2d_codes(mod, x, weight, bias):
    """Conv2d_Q.forward inside a chain linked by fusion.link_codes: `x` is float32 or the uint8 codes the previous layer
    wrote for THIS module's Ka / q_bit; the result is uint8 codes for the next layer (mod._code_out = (Ka_next, q_bit_next))
    or float32.  One slfp_conv2d_fwd_codes call where libslfp_hip has a kernel for the combination; otherwise the same
    values through the float32 interface plus slfp_encode_f32 / slfp_decode_f32 (always correct, never faster).  A module with
    `_code_entry` set that reads float32 and writes codes asks slfp_conv2d_entry_supported first and, where that says yes, runs
    ONE slfp_conv2d_fwd_entry call (the 1x1 layer at which a chain of codes begins).  A module marked `_code_x3` that reads codes and
    is refused by slfp_conv2d_fwd_codes (a 1x1 layer under options.mfma_passes = 3) asks slfp_conv2d_codes_x3_supported next and runs
    ONE slfp_conv2d_fwd_codes_x3 call."""
    x_codes = x.dtype == torch.uint8
    out = mod._code_out
    if not x_codes:
        _require_gpu_f32(x, "Conv2d_Q")
    elif not x.is_cuda:
        raise RuntimeError("Conv2d_Q: code tensors live on the ROCm device")
    lut = mod._code_lut if out is not None else None
    if lut is not None:
        # a link of fusion.link_layerout: the table holds activation + reader's quantizer of every layer-output class, and the
        # activation modules behind this layer pass codes through.  There is no second way to compute that: no kernel is an error.
        if lut.device != x.device or lut.dtype != torch.uint8 or lut.numel() != _lib.LAYEROUT_LUT_BYTES:
            raise RuntimeError("Conv2d_Q: `_code_lut` must be a uint8 tensor of SLFP_LAYEROUT_LUT_BYTES bytes on the input's device")
        plan = None
        if x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last):
            plan = _plan(mod, x, weight, True, True, ("lut", x_codes, out, None))
        if plan is None or not plan.ok:
            raise RuntimeError("Conv2d_Q: no kernel writes this layer's codes through a layer-output table "
                               "(slfp_conv2d_codes_lut_supported); call fusion.unlink_codes(model)")
        return _launch(mod, plan, x, weight, bias)
    if x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last):   # the code path is NHWC only
        if not x_codes and out is not None and mod._code_entry:
            plan = _plan(mod, x, weight, True, True, ("entry", False, out, None))
            if plan.ok:
                return _launch(mod, plan, x, weight, bias)
        plan = _plan(mod, x, weight, True, True, ("codes", x_codes, out, None))
        if plan.ok:
            return _launch(mod, plan, x, weight, bias)
        if x_codes and mod._code_x3:
            plan = _plan(mod, x, weight, True, True, ("codes_x3", True, out, None))
            if plan.ok:
                return _launch(mod, plan, x, weight, bias)
        if x_codes and out is None and mod._post is not None and int(mod._post[2]) == 2:
            plan = _plan(mod, x, weight, True, True, ("codes_lo", True, None, None))
            if plan.ok:
                return _launch(mod, plan, x, weight, bias)
    # anything else takes the float32 interface
    y = _hip_conv2d(mod, hip_decode(x, _act_fmt(mod.q_bit)) if x_codes else x, weight, bias, cache_ok=True)
    return hip_encode(y, out[0], _act_fmt(out[1])) if out is not None else y


def _hip_conv2d_u8(mod, x, weight, bias, order=None):
    """Conv2d_Q.forward of a stem marked by fusion.link_image_u8 on a uint8 batch: `x` holds PIXELS (never codes), logical (N, C, H, W)
    in channels_last on the weights' device; mod._image_table is the float32 [C][256] table of their values.  In inference, where
    slfp_conv2d_u8_supported says yes (and image_u8_supported keeps the stem's family), ONE slfp_conv2d_fwd_u8 launch: float32 out, or
    the codes mod._code_out describes.  Everywhere else -- training, autograd recording, q_bit 32, a stem without a byte form, a table
    epilogue -- the bytes are expanded on the device (slfp_image_u8_expand_f32) and the module's ordinary forward runs on that float32
    tensor, so gradients and every stash are exactly the float32 path's; `_last_kernel` then reads "u8-expand+<what ran>".  Both give
    the bits of the unlinked module on the expanded tensor."""
    from . import image_u8
    table = mod._image_table
    image_u8.check_pixels(x, table, "Conv2d_Q (image_u8)")
    if weight.device != x.device:
        raise TypeError(f"Conv2d_Q (image_u8): pixels are on {x.device} but the weights on {weight.device}")
    need_grad = torch.is_grad_enabled() and (weight.requires_grad or (mod.bias is not None and mod.bias.requires_grad))
    plan = None
    if (mod.q_bit in (8, 7) and not mod.training and not need_grad and (mod._code_out is None or mod._code_lut is None)
            and (mod.bias is None or mod._scaled_bias) and x.numel()):
        plan = _plan(mod, x, weight, True, True, ("u8", False, mod._code_out, None))
        if not (plan.ok and image_u8_supported(plan.u8_family)):
            plan = None
    if plan is None:
        out = mod.forward(image_u8.expand(x, table), order)
        if mod.q_bit in (8, 7):
            mod.__dict__["_last_kernel"] = "u8-expand+" + str(mod._last_kernel)
        return out
    with torch.no_grad():
        out = _launch(mod, plan, x, weight, bias, cache=not torch.is_grad_enabled())
    mod.output = out
    return out


# Stem families (the first word of slfp_debug_stem_u8_instance's string: "stem", "small", "rows", "im2row") whose byte form the default
# does NOT take: a marked stem of such a family runs "u8-expand" (slfp_image_u8_expand_f32 + the float32 kernel).  Two conditions,
# read from profiles/image_u8_bench.json, both over every row of the family: the rule of DESIGN section 12 -- the byte form (C) is
# below ATen normalisation + the float32 stem (B) by more than B's round-to-round spread -- and the byte form is not slower than the
# library's own expansion path (E) by more than E's spread: of its two ways to read bytes the default takes the faster one.
# Measured on an MI355X: `rows` misses the first (SqueezeNet's stem, float32 out: C 1.10 x B) and the second (C 1.04-1.40 x E);
# `small` misses the second (VGG-16: C 1.09-1.10 x E); `im2row` misses the second with float32 out (C 1.05 x E) and would gain 2 % with
# code out; `stem` (k_stem_fixed) meets both (C 0.84-0.94 x E).  The C query keeps answering what the kernels can run; a test or a benchmark empties this set to run
# every form.
IMAGE_U8_OFF = {"small", "rows", "im2row"}


def image_u8_supported(family):
    """Does the default take the byte form of stem family `family` (_Plan.u8_family)?"""
    return family not in IMAGE_U8_OFF


def _hip_conv2d_slice(mod, x, weight, bias, out_slice):
    """Conv2d_Q.forward_slice(x, (buffer, c_off)) as ONE slfp_conv2d_fwd_codes_slice call: the codes this linked producer
    (mod._code_out) would return go into buffer[:, c_off:c_off + C_out] of a wider uint8 channels_last tensor instead of one of
    their own -- the concat of a Fire module without the copy (fusion.fuse_fire).  Same plan cache and weight blob as the other
    paths.  There is no second way to compute this: a combination without a kernel raises."""
    try:
        buf, c_off = out_slice
        c_off = int(c_off)
    except (TypeError, ValueError):
        raise TypeError("Conv2d_Q: out_slice must be (uint8 channels_last buffer, channel offset)") from None
    x_codes = torch.is_tensor(x) and x.dtype == torch.uint8
    nhwc = torch.channels_last
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and (x_codes or x.dtype == torch.float32)
            and x.is_contiguous(memory_format=nhwc) and weight.device == x.device):
        raise RuntimeError("Conv2d_Q: out_slice needs a 4-d channels_last ROCm input (float32 or uint8 codes) on the weights' device")
    if not (torch.is_tensor(buf) and buf.dtype == torch.uint8 and buf.dim() == 4 and buf.device == x.device
            and buf.is_contiguous(memory_format=nhwc)):
        raise RuntimeError("Conv2d_Q: out_slice's buffer must be a 4-d uint8 channels_last tensor on the input's device")
    ld = buf.shape[1]
    plan = _plan(mod, x, weight, True, True, ("slice", x_codes, mod._code_out, ld))
    n, c_out, ho, wo = plan.y_shape
    if (buf.shape[0], buf.shape[2], buf.shape[3]) != (n, ho, wo) or c_off < 0 or c_off + c_out > ld:
        raise RuntimeError(f"Conv2d_Q: out_slice channels [{c_off}, {c_off + c_out}) of a buffer of shape {list(buf.shape)} do not "
                           f"hold this layer's output {list(plan.y_shape)}")
    if not plan.ok or c_off % 16 or buf.data_ptr() % 16:
        raise RuntimeError(f"Conv2d_Q: no kernel writes this layer's codes into channels {c_off}.. of a {ld}-channel tensor "
                           "(slfp_conv2d_codes_slice_supported; offset and width are multiples of 16)")
    _launch(mod, plan, x, weight, bias, buf.data_ptr() + c_off, y_ld=ld)
    return buf


def _hip_conv2d_res(mod, x, weight, bias, residual, relu, trunk=None):
    """Conv2d_Q.forward(x, residual=r) as ONE slfp_conv2d_fwd_res call: relu?(epilogue(conv(x)) + r), bit-identical to the
    module's ordinary forward followed by torch.add and torch.relu.  `x` is float32 or the uint8 codes a linked producer
    wrote for this module.  Returns None where the library has no residual kernel for the combination (layer geometry,
    layouts, an epilogue ReLU in front of the add): the caller then computes the same values with ATen.
    trunk = (Ka, q_bit) of the Conv2d_Q layers that read the result (mod._trunk_code_out, fusion.link_trunk): where
    slfp_conv2d_res_codes_supported says yes the ONE call is slfp_conv2d_fwd_res_codes, which also writes those readers' codes; the
    float32 tensor returned -- the same bits -- then carries them as `_trunk_codes = (codes, Ka, q_bit)`.  An attribute of that one
    tensor object: whatever an op makes of it has none, and a reader checks the scale before it decodes (Conv2d_Q.forward)."""
    x_codes = x.dtype == torch.uint8
    nhwc = torch.channels_last
    if not (x.is_cuda and x.dim() == 4 and (x_codes or x.dtype == torch.float32) and x.is_contiguous(memory_format=nhwc)
            and weight.device == x.device):
        return None
    plan = _plan(mod, x, weight, True, True, ("res_codes", x_codes, trunk, bool(relu))) if trunk is not None and x_codes else None
    if plan is None or not plan.ok:
        plan = _plan(mod, x, weight, True, True, ("res", x_codes, None, bool(relu)))
    if not plan.ok:
        return None
    r = residual
    if not (torch.is_tensor(r) and r.dtype == torch.float32 and r.device == x.device and tuple(r.shape) == tuple(plan.y_shape)
            and r.is_contiguous(memory_format=nhwc) and r.data_ptr() % 16 == 0):
        return None
    out = _launch(mod, plan, x, weight, bias, res=r, relu=relu)   # the same blob (and cache entry) as the other paths
    if plan.kind == "res_codes":
        out, codes = out
        out._trunk_codes = (codes, trunk[0], trunk[1])
    return out


def _aligned(t):
    """`t` itself if its data is 16-byte aligned (what the C ABI requires), else an aligned copy."""
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _hip_backward(mod, desc, x, w, gy, needs):
    """One slfp_conv2d_bwd_ex call on dense NCHW / NHWC operands (the layouts `desc` names), or None where the library does
    not cover the layer under options.backward's flags ("hip_all": SLFP_BWD_DENSE).  needs = (gx, gw, gb wanted); returns (gx, gw, gb) with None for what was not asked: gx has x's
    memory format, gw is contiguous like `w`."""
    L = _lib.load()
    flags = _lib.BWD_DENSE if options.backward == "hip_all" else 0
    if not L.slfp_conv2d_bwd_supported_ex(ctypes.byref(desc), flags):
        return None
    need_gx, need_gw, need_gb = needs
    x, gy = _aligned(x), _aligned(gy)
    w = w.detach()
    w = _aligned(w if w.is_contiguous() else w.contiguous())   # OIHW
    # the bias sum comes with the weight gradient's pass (a frozen weight with a trainable bias still runs it)
    run_gw = need_gw or need_gb
    gx = torch.empty_like(x) if need_gx else None
    gw = torch.empty(w.shape, dtype=torch.float32, device=x.device) if run_gw else None
    gb = torch.empty(desc.c_out, dtype=torch.float32, device=x.device) if need_gb else None
    with _on_device(x.device):
        nbytes = L.slfp_conv2d_bwd_workspace_bytes_ex(ctypes.byref(desc), flags, int(need_gx), int(run_gw))
        ws = _workspace(x.device, nbytes) if nbytes else None
        _lib.check(L.slfp_conv2d_bwd_ex(ctypes.byref(desc), flags, x.data_ptr(), w.data_ptr(), gy.data_ptr(), _ptr(gx), _ptr(gw),
                                        _ptr(gb), _ptr(ws), _stream_handle(x)))
    mod._last_bwd_kernel = L.slfp_conv2d_bwd_kernel_name_ex(ctypes.byref(desc), flags).decode()
    return gx, gw if need_gw else None, gb


def _bwd_flags():
    """The `flags` word of slfp_conv2d_bwd_*_ex under options.backward, or None where it names no HIP backward ("composite")."""
    return {"hip": 0, "hip_all": _lib.BWD_DENSE}.get(options.backward)


def _bwd_codes_supported(mod, shape):
    """Does slfp_conv2d_bwd_codes cover Conv2d_Q `mod` on a channels_last code tensor of `shape` under options.backward?"""
    flags = _bwd_flags()
    if flags is None:
        return False
    return bool(_lib.load().slfp_conv2d_bwd_codes_supported(ctypes.byref(_conv_desc(mod, shape, True, True)), flags))


def _link_conv_clean(conv):
    """A Conv2d_Q a training link may feed: q_bit 8 or 7, no raw (unscaled) bias, nothing fused or linked onto it."""
    return (conv.q_bit in (8, 7) and (conv.bias is None or conv._scaled_bias) and conv._post is None and conv._code_out is None
            and conv._image_table is None)


def _train_codes_plan(conv, t):
    """The plan of `conv`'s code-reading, float32-writing forward on a channels_last tensor of t's shape: what a training link runs."""
    return _plan(conv, t, conv.weight, True, True, ("codes", True, None, None))


def _train_codes_reader_matches(conv, t, ka, q_bit):
    """The host-only half of _train_codes_reader_ok: `conv` is in training mode, its present quantizer is (ka, q_bit) -- ka as
    _f32(Ka) --, nothing is fused or linked onto it and its weights are on t's device."""
    return (conv.training and conv.q_bit == q_bit and _f32(conv.Ka) == ka and _link_conv_clean(conv)
            and conv.weight.device == t.device)


def _train_codes_reader_ok(conv, t, ka, q_bit):
    """May Conv2d_Q `conv` read training codes of the quantizer (ka, q_bit) in place of the float32 tensor `t` (or: is `t` such a
    code tensor; shape and device are what is read), forward and backward?  The one answer for every producer and reader of a
    training link, the library asked last: _train_codes_reader_matches; a code-reading forward under the current
    options (one cached plan); a backward kernel that reads the codes under options.backward (one query; "composite" has none)."""
    return (_train_codes_reader_matches(conv, t, ka, q_bit) and _train_codes_plan(conv, t).ok
            and _bwd_codes_supported(conv, t.shape))


def _hip_backward_codes(mod, desc, codes, w, gy, needs):
    """_hip_backward with the activation operand as the 1-byte codes the layer read in its forward (slfp_conv2d_bwd_codes; NHWC):
    (gx, gw, gb) for needs = (gx, gw, gb wanted).  The caller has asked _bwd_codes_supported: a layer without the kernel is an
    error here, not a fallback."""
    L = _lib.load()
    flags = _bwd_flags()
    if flags is None or not L.slfp_conv2d_bwd_codes_supported(ctypes.byref(desc), flags):
        raise RuntimeError("Conv2d_Q: no backward kernel reads this layer's codes under options.backward = "
                           f"{options.backward!r} (slfp_conv2d_bwd_codes_supported); call fusion.unlink_codes_train(model)")
    need_gx, need_gw, need_gb = needs
    gy = _aligned(gy)
    w = w.detach()
    w = _aligned(w if w.is_contiguous() else w.contiguous())   # OIHW
    run_gw = need_gw or need_gb
    gx = torch.empty(codes.shape, dtype=torch.float32, device=codes.device, memory_format=torch.channels_last) if need_gx else None
    gw = torch.empty(w.shape, dtype=torch.float32, device=codes.device) if run_gw else None
    gb = torch.empty(desc.c_out, dtype=torch.float32, device=codes.device) if need_gb else None
    with _on_device(codes.device):
        nbytes = L.slfp_conv2d_bwd_workspace_bytes_ex(ctypes.byref(desc), flags, int(need_gx), int(run_gw))
        ws = _workspace(codes.device, nbytes) if nbytes else None
        _lib.check(L.slfp_conv2d_bwd_codes(ctypes.byref(desc), flags, codes.data_ptr(), w.data_ptr(), gy.data_ptr(), _ptr(gx), _ptr(gw),
                                           _ptr(gb), _ptr(ws), torch.cuda.current_stream(codes.device).cuda_stream))
    mod._last_bwd_kernel = L.slfp_conv2d_bwd_kernel_name_ex(ctypes.byref(desc), flags).decode()
    return gx, gw if need_gw else None, gb


def _needs(ctx):
    """(gx, gw, gb) wanted by autograd from a Function whose inputs start with (x, weight, bias)."""
    return ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]


def _conv_backward_hip(ctx, gy):
    """_SlfpConv2dFn.backward on the HIP kernels, or None where slfp_conv2d_bwd does not cover the layer."""
    mod = ctx.mod
    x, weight = ctx.saved_tensors
    squeeze = x.dim() == 3
    if squeeze:
        x, gy = x.unsqueeze(0), gy.unsqueeze(0)
    if x.numel() == 0 or gy.numel() == 0 or not x.is_cuda or isinstance(mod.padding, str):
        return None
    x = x.detach()
    nhwc_x = x.is_contiguous(memory_format=torch.channels_last)
    if not nhwc_x and not x.is_contiguous():
        x = x.contiguous()
    if gy.is_contiguous(memory_format=torch.channels_last):
        nhwc_y = True
    elif gy.is_contiguous():
        nhwc_y = False
    else:   # e.g. the stride-0 gy of out.sum().backward()
        nhwc_y = nhwc_x
        gy = gy.contiguous(memory_format=torch.channels_last if nhwc_y else torch.contiguous_format)
    res = _hip_backward(mod, _conv_desc(mod, x.shape, nhwc_x, nhwc_y), x, weight, gy, _needs(ctx))
    if res is not None and squeeze and res[0] is not None:
        res = (res[0].squeeze(0),) + res[1:]
    return res


class _SlfpConv2dFn(torch.autograd.Function):
    """HIP forward; backward = the reference's composite (STE through both quantizers:
    utils/sfp_quant.py:50-53, :99-102; conv gradients from torch.nn.grad on the GPU), or the HIP kernels of
    slfp_conv2d_bwd with options.backward = "hip" / "hip_all"."""

    @staticmethod
    def forward(ctx, x, weight, bias, mod, scaled_bias):
        ctx.mod = mod
        ctx.scaled_bias = scaled_bias
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return _hip_conv2d(mod, x, weight, bias if scaled_bias else None)

    @staticmethod
    def backward(ctx, gy):
        mod = ctx.mod
        if options.backward in ("hip", "hip_all"):
            res = _conv_backward_hip(ctx, gy)
            if res is not None:
                return res[0], res[1], res[2], None, None
        mod._last_bwd_kernel = "composite"
        x, weight = ctx.saved_tensors
        ka, kw = _f32(mod.Ka), _f32(mod.Kw)
        g = (gy * kw * ka).contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            wq = hip_quantize(weight.detach().contiguous(), kw, _w_fmt(mod.q_bit))
            gx = torch.nn.grad.conv2d_input(x.shape, wq, g, mod.stride, mod.padding, mod.dilation, mod.groups) / ka
        if ctx.needs_input_grad[1]:
            xq = hip_quantize(x.detach().contiguous(), ka, _act_fmt(mod.q_bit))
            gw = torch.nn.grad.conv2d_weight(xq, weight.shape, g, mod.stride, mod.padding, mod.dilation, mod.groups) / kw
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = gy.sum(dim=(0, 2, 3)) if ctx.scaled_bias else g.sum(dim=(0, 2, 3))
        return gx, gw, gb, None, None


def mark_grouped_stash(model):
    """Called by streams.forward_image_groups once all groups have run: every module's stash now holds the last group's
    slice of the batch only, so `input_q` raises until the module's next ordinary forward.  (Reads inside a group's own
    forward, as the reference's CIFAR nets do, see that group's slice.)"""
    for m in model.modules():
        if "_grouped_stash" in m.__dict__:
            m.__dict__["_grouped_stash"] = True


def _check_stash(mod):
    if mod._grouped_stash:
        raise RuntimeError(f"{type(mod).__name__}.input_q: the last forward ran as image groups (streams.forward_image_groups), "
                           "so the stash holds one group's slice of the batch only; run an ordinary forward to read it")


def _apply_post_composite(out, post):
    """The fused epilogue written with stock ATen ops (q_bit == 32 passthrough only)."""
    if post is None:
        return out
    scale, shift, flags = post   # flags: 1 = ReLU (the layer-output quantizer is never fused onto a q_bit 32 conv)
    if scale is not None:
        out = out * scale.to(out.device).view(1, -1, 1, 1) + shift.to(out.device).view(1, -1, 1, 1)
    return torch.relu(out) if (int(flags) & 1) else out


def _conv_class(q_bit, Kw, Ka, bias_default, scaled_bias):
    class Conv2d_Q(nn.Conv2d):
        # Kw, Ka are positional arguments 4 and 5 (utils/conv2d_func.py:10-11, :30)
        def __init__(self, in_channels, out_channels, kernel_size, Kw=Kw, Ka=Ka,
                     stride=1, padding=0, dilation=1, groups=1, bias=bias_default):
            super(Conv2d_Q, self).__init__(in_channels, out_channels, kernel_size, stride,
                                           padding, dilation, groups, bias)
            self.q_bit = q_bit
            self.quantize_weight = weight_quantize_func(q_bit=q_bit)
            self.quantize_act = act_quantize_func(q_bit=q_bit)
            # plain attributes, 0-dim float64, stay on the CPU (utils/conv2d_func.py:17-18)
            self.Kw = torch.tensor(Kw)
            self.Ka = torch.tensor(Ka)
            self._prep = _PreparedWeights()
            self._plans = {}
            self._last_input = None
            self._input_q = None
            self._weight_q32 = None
            self._last_kernel = None
            self._last_bwd_kernel = None   # what the last backward ran: a slfp_conv2d_bwd kernel name or "composite"
            self._post = None  # (scale, shift, relu): fused eval-BN + ReLU epilogue (fusion.fuse_bn_relu)
            self._code_out = None   # (Ka, q_bit) of the next Conv2d_Q: hand it 1-byte codes (fusion.link_codes)
            self._code_entry = False   # with _code_out on a float32 input: ONE slfp_conv2d_fwd_entry launch where the library has it
            self._code_x3 = False   # on a code input that "codes" refuses: slfp_conv2d_fwd_codes_x3 (fusion.link_codes(x3=True))
            # with _code_out behind a layer-output epilogue: the uint8 table of SLFP_LAYEROUT_LUT_BYTES entries that maps a
            # layer-output class to the reader's code (fusion.link_layerout); slfp_conv2d_fwd_codes_lut then runs.  A buffer, so
            # that it follows the module across devices; not persistent: the state dict keeps the reference's keys
            self.register_buffer("_code_lut", None, persistent=False)
            # fusion.link_image_u8: the float32 [C_in][256] table that gives this stem's uint8 input the meaning "pixels"; None: a
            # uint8 input is codes, as ever.  A non-persistent buffer like _code_lut
            self.register_buffer("_image_table", None, persistent=False)
            self._last_pixels = None
            self._trunk_code_out = None   # forward(x, residual=r): (Ka, q_bit) of the Conv2d_Q layers that read the result; it then
                                          # carries their codes (fusion.link_trunk).  Not `_code_out`: the result stays float32
            self._last_codes = None
            self.residual_relu = False   # forward(x, residual=r): a ReLU follows the add (fusion.fuse_residual sets it)
            self._scaled_bias = scaled_bias
            self.output = None
            self._grouped_stash = False   # the stash is one image group's (mark_grouped_stash)

        # -- the reference stores these on every forward (utils/conv2d_func.py:21-22);
        #    here they are computed on first access after a forward.
        @property
        def input_q(self):
            _check_stash(self)
            if self.q_bit == 32:
                return self._input_q
            if self._input_q is None and self._last_input is None and self.__dict__.get("_last_pixels") is not None:
                # a byte-input stem (fusion.link_image_u8): the float32 tensor its pixels stand for, made on first read
                from . import image_u8
                self._last_input = image_u8.expand(self._last_pixels, self._image_table)
            if self._input_q is None and self._last_input is not None:
                self._input_q = hip_quantize(self._last_input, _f32(self.Ka), _act_fmt(self.q_bit))
            elif self._input_q is None and self._last_codes is not None:
                # inside a code chain the input arrived already quantized: input_q = decode(codes), bit for bit
                self._input_q = hip_decode(self._last_codes, _act_fmt(self.q_bit))
            return self._input_q

        @property
        def weight_q(self):
            if self.q_bit == 32:
                return self._weight_q32
            if self._last_input is None and self._last_codes is None and self.__dict__.get("_last_pixels") is None:
                return None
            stale = self._prep.weight_q is None or self._prep.weight_version != self.weight._version
            if stale or self.training or torch.is_grad_enabled():   # p.data updates are invisible to _version
                self._prep.weight_q = hip_quantize(self.weight.detach().contiguous(), _f32(self.Kw), _w_fmt(self.q_bit))
            return self._prep.weight_q

        def invalidate(self):
            """Drop the cached quantized weights (call after changing `weight.data` in place during inference)."""
            self._prep.invalidate()

        def train(self, mode=True):
            self._prep.invalidate()   # weights may have been stepped through `.data` since the last forward
            return super(Conv2d_Q, self).train(mode)

        def _forward_residual(self, input, order, residual):
            out = None
            if (self.q_bit in (8, 7) and not self.training and not torch.is_grad_enabled() and self._code_out is None
                    and (self.bias is None or scaled_bias)):
                if self._grouped_stash:
                    self._grouped_stash = False
                out = _hip_conv2d_res(self, input, self.weight, self.bias, residual, self.residual_relu, self._trunk_code_out)
            if out is None:   # training, NCHW, q_bit 32, a layer without a residual kernel: the same values with ATen
                out = self.forward(input, order) + residual
                if self.residual_relu:
                    out = torch.relu(out)
            self.output = out
            return out

        def _forward_train_codes(self, fn, front, codes, *back):
            """This module on the training codes of a link: fn.apply(*front, weight, bias, self, codes, *back) where one of the
            differentiable inputs (`front`, weight, bias) records, else the bare code-reading forward."""
            from .batchnorm import _codes_conv_forward
            bias = self.bias if scaled_bias else None
            if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (*front, self.weight, bias)):
                out = fn.apply(*front, self.weight, bias, self, codes, *back)
            else:
                with torch.no_grad():
                    out = _codes_conv_forward(self, codes, self.weight, bias, "Conv2d_Q")
            self.output = out
            return out

        def _reads_train_trunk(self, trunk, ttc):
            """Does this module, in training mode, read the codes `ttc` = (codes, float32(Ka), q_bit) that ride on the float32
            `trunk` instead of the tensor itself?  Its own clauses are the code tensor's: the trunk's shape, channels_last."""
            codes, ka, q_bit = ttc
            return (trunk.dtype == torch.float32 and codes.shape == trunk.shape
                    and codes.is_contiguous(memory_format=torch.channels_last) and _train_codes_reader_ok(self, codes, ka, q_bit))

        def forward_slice(self, input, out_slice):
            """`out_slice=(buffer, c_off)`: a linked code producer writes its codes into buffer[:, c_off:c_off + C_out] (uint8,
            channels_last, wider than this layer) in ONE launch (slfp_conv2d_fwd_codes_slice; `_last_kernel` ends in "+slice")
            and returns `buffer`: the concat of a Fire module without the copy (fusion.fuse_fire).  Anything else -- an unlinked
            module, training, a layer without such a kernel -- raises.  A method of its own, not a keyword of forward(): the
            reference's forward surface (and the `residual` keyword beside it) stays as it is.  Like forward() called directly
            it runs no module hooks."""
            if (self._code_out is None or self.q_bit not in (8, 7) or self.training
                    or (self.bias is not None and not scaled_bias)):
                raise RuntimeError("Conv2d_Q: out_slice is for a linked code producer in inference (fusion.link_codes / fuse_fire "
                                   "set `_code_out`; module.eval(); the scaled-bias class)")
            if self._grouped_stash:
                self._grouped_stash = False
            with torch.no_grad():
                self.output = _hip_conv2d_slice(self, input, self.weight, self.bias, out_slice)
            return self.output

        def forward(self, input, order=None, *, residual=None):
            """Conv2d_Q.forward of the reference (utils/conv2d_func.py:20-25).  `residual` (keyword-only, not part of the
            reference's surface): returns relu?(forward(input) + residual), the ReLU if `self.residual_relu` -- the tail of a
            residual block.  In inference on channels_last ROCm tensors, where libslfp_hip has a residual kernel for the
            layer, that is ONE launch (slfp_conv2d_fwd_res; `_last_kernel` then ends in "+res"); otherwise the add and the
            ReLU run as ATen ops after the ordinary forward.  Both give the same bits.  With a residual `self.output` is
            the tensor AFTER the add (and ReLU), not the convolution's own output.  With `_trunk_code_out` set (fusion.link_trunk)
            and code input the launch is slfp_conv2d_fwd_res_codes (`_last_kernel` ends in "+codes_in+res+trunk_codes"): the same
            float32 tensor, which also carries the 1-byte codes of the layers that read it."""
            if residual is not None:
                return self._forward_residual(input, order, residual)
            if self._grouped_stash:
                self._grouped_stash = False
            if self._image_table is not None and torch.is_tensor(input) and input.dtype == torch.uint8:
                # a stem marked by fusion.link_image_u8: uint8 is pixels here, never codes
                self.output = _hip_conv2d_u8(self, input, self.weight, self.bias if scaled_bias else None, order)
                return self.output
            link = input.__dict__.get("_train_link") if type(input) is torch.Tensor and input.dtype == torch.uint8 else None
            if link is not None and link.made_for(self, input):
                # the codes a fusion.TrainBatchNormCodes2d wrote for THIS module's present quantizer, in a training step: BN -> ReLU -> conv
                # as one autograd Function.  The record leaves the tensor first: a finished step must not keep the BN's input alive
                from .batchnorm import hip_bn_codes_conv_train
                del input.__dict__["_train_link"]
                return self._forward_train_codes(hip_bn_codes_conv_train, (link.x, link.weight, link.bias), input, link)
            ttc = input.__dict__.get("_train_trunk_codes") if type(input) is torch.Tensor and self.training else None
            if ttc is not None and self._reads_train_trunk(input, ttc):
                # the float32 trunk of a Bottleneck linked by fusion.link_bottleneck_codes_train carries the codes its bn3 tail wrote
                # for THIS module's present quantizer, in a training step: read those (a stale or foreign scale, a module with
                # something fused onto it or options.backward = "composite" reads the float32 tensor as ever)
                from .batchnorm import hip_trunk_codes_conv_train
                return self._forward_train_codes(hip_trunk_codes_conv_train, (input,), ttc[0])
            tc = input.__dict__.get("_trunk_codes") if type(input) is torch.Tensor else None
            if tc is not None and not self.training and self.q_bit in (8, 7) and tc[1:] == (float(self.Ka), self.q_bit):
                # the float32 trunk of a block linked by fusion.link_trunk carries the codes written for THIS module's present
                # quantizer: read those (a stale or foreign scale is never decoded: the float32 tensor is read instead)
                input = tc[0]
            if self.q_bit == 32:
                # identity quantizers (utils/sfp_quant.py:11-12, :60-61): stock ATen, any device
                self._input_q = input / self.Ka
                self._weight_q32 = self.weight / self.Kw
                b = self.bias
                if b is not None and scaled_bias:
                    b = b / self.Ka / self.Kw
                self.output = F.conv2d(self._input_q, self._weight_q32, b, self.stride, self.padding,
                                       self.dilation, self.groups) * self.Ka * self.Kw
                if self.bias is not None and not scaled_bias:
                    pass  # conv2d_Q hands the raw bias to F.conv2d above (utils/conv2d_func.py:23)
                self.output = _apply_post_composite(self.output, self._post)
                return self.output
            if self.q_bit not in (8, 7):
                raise UnboundLocalError("q_bit must be 32, 8 or 7 (utils/sfp_quant.py:142-147)")
            if input.dtype == torch.uint8 or self._code_out is not None:
                # a link of fusion.link_codes: 1-byte codes on one or both sides (inference only)
                if self.training or self._scaled_bias is False and self.bias is not None:
                    raise RuntimeError("Conv2d_Q: code links (fusion.link_codes) are inference-only and need the scaled bias class; "
                                       "call fusion.unlink_codes(model)")
                with torch.no_grad():
                    self.output = _hip_conv2d_codes(self, input, self.weight, self.bias)
                return self.output
            need_grad = torch.is_grad_enabled() and (input.requires_grad or self.weight.requires_grad or
                                                     (self.bias is not None and self.bias.requires_grad))
            if self._post is not None and (need_grad and self.training):
                raise RuntimeError("Conv2d_Q: a fused BN/ReLU epilogue is inference-only; call fusion.unfuse(model) to train")
            if self._post is not None and self.bias is not None and not scaled_bias:
                raise NotImplementedError("fused epilogue with conv2d_Q's raw (unscaled) bias is not supported")
            if need_grad and self._post is None:
                # conv2d_Q's raw bias is added below, outside the Function: only the scaled one goes through it
                out = _SlfpConv2dFn.apply(input, self.weight, self.bias if scaled_bias else None, self, scaled_bias)
            else:
                out = _hip_conv2d(self, input, self.weight, self.bias if scaled_bias else None,
                                  cache_ok=not self.training and not torch.is_grad_enabled())
            if self.bias is not None and not scaled_bias:
                # conv2d_Q hands the raw bias to F.conv2d (utils/conv2d_func.py:23): (conv + b)*Ka*Kw
                out = out + (self.bias * self.Ka * self.Kw).to(out.dtype).view(1, -1, 1, 1)
            self.output = out
            return out

    return Conv2d_Q


def conv2d_Q(q_bit, Kw, Ka):
    """utils/conv2d_func.py:8-26: bias defaults to False and is NOT rescaled."""
    return _conv_class(q_bit, Kw, Ka, bias_default=False, scaled_bias=False)


def conv2d_Q_bias(q_bit, Kw, Ka):
    """utils/conv2d_func.py:28-48: bias defaults to True, bias_q = bias / Ka / Kw."""
    return _conv_class(q_bit, Kw, Ka, bias_default=True, scaled_bias=True)


def _hip_linear(mod, x, weight, bias, cache_ok=False, fc=False):
    """One Linear_Q forward on libslfp_hip.  fc: run the weight-streaming kernel (slfp_linear_fwd_fc) where the library has it for
    this layer -- the caller asks for it only in inference; `x` may then be the uint8 codes a fusion.link_head producer wrote, and
    mod._code_out / mod._code_relu describe the codes (and the folded ReLU) to write."""
    if x.dtype == torch.uint8 and fc:
        if not x.is_cuda:
            raise RuntimeError("Linear_Q: code tensors live on the ROCm device")
    else:
        _require_gpu_f32(x, "Linear_Q")
    L = _lib.load()
    lead = x.shape[:-1]
    x2 = x.reshape(-1, x.shape[-1])
    x2 = x2 if x2.is_contiguous() else x2.contiguous()
    B, I = x2.shape
    O = weight.shape[0]
    if I != weight.shape[1]:
        raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({B}x{I} and {weight.shape[1]}x{O})")
    w = weight.detach()
    w = w if w.is_contiguous() else w.contiguous()
    b = None
    if bias is not None:
        b = bias.detach()
        b = b if b.is_contiguous() else b.contiguous()
    ka, kw = _f32(_scalar_scale(mod.Ka, "Ka")), _f32(_scalar_scale(mod.Kw, "Kw"))
    x_codes = x2.dtype == torch.uint8
    out, relu = mod._code_out, 1 if mod._code_relu else 0
    fc = (fc and B > 0 and mod.q_bit in (8, 7) and
          bool(L.slfp_linear_fc_supported(B, I, O, mod.q_bit, options.mfma_passes, ctypes.byref(_conv_io(x_codes, out)), 1, relu)))
    if not fc and (x_codes or out is not None or relu):
        # a linked layer without the kernel (F16X3, an empty batch): the float32 interface between slfp_decode_f32 and slfp_encode_f32
        # (never faster).  decode(codes) is input_q = QA(x / Ka), a class value without the scale, and the float32 interface divides
        # by Ka and quantizes again: it is handed input_q * Ka.  QA((q * Ka) / Ka) == q for every class value q: the product and the
        # quotient are each correctly rounded, so the result is within 2 ulp of q, while the quantizer's steps lie midway between
        # classes that are 2^(1/16) (SFP<3,3>: 2^(1/8)) apart; the clamp literal stays above the clamp's threshold, exact zero stays
        # zero, and the "tiny" class stays below the smallest step (should the product underflow to 0, tiny and zero are both the
        # operand +-0).  So the kernel sees the operands the codes stand for: the bits of the unlinked layer in the same mode.
        xf = hip_decode(x2, _act_fmt(mod.q_bit)) * ka if x_codes else x2
        y = _hip_linear_f32(mod, L, xf, w, weight, b, ka, kw, cache_ok)
        y = torch.relu(y) if relu else y
        y = hip_encode(y, out[0], _act_fmt(out[1])) if out is not None else y
    elif fc:
        y = _hip_linear_fc(mod, L, x2, w, weight, b, ka, kw, cache_ok, out, relu)
    else:
        y = _hip_linear_f32(mod, L, x2, w, weight, b, ka, kw, cache_ok)
    return y.reshape(*lead, O)


def _linear_blob(mod, L, w, weight, kw, stream, cache_ok):
    """The prepared weights of a Linear_Q (slfp_linear_prepare_weights): quantized once per weight version (the reference
    re-quantizes on every forward, utils/conv2d_func.py:62: AlexNet's 9216x4096 / VGG-16's 25088x4096 layers make that the dominant
    cost of their classifiers); cached only where cache_ok, see the module docstring.  Both linear kernels read this blob."""
    O, I = w.shape

    def make(h):
        blob = torch.empty(max(L.slfp_linear_workspace_bytes(1, I, O), 16), dtype=torch.uint8, device=w.device)
        _lib.check(L.slfp_linear_prepare_weights(w.data_ptr(), blob.data_ptr(), I, O, kw, mod.q_bit, options.mfma_passes, h))
        return blob, None

    key = (w.device, w.data_ptr(), weight._version, tuple(w.shape), mod.q_bit, kw, options.mfma_passes)
    return mod._prep.get(key, stream, cache_ok, make)


def _hip_linear_f32(mod, L, x2, w, weight, b, ka, kw, cache_ok):
    """slfp_linear_fwd_prepared: the layer as a 1x1 convolution over the rows of x2 (float32, contiguous)."""
    (B, I), O = x2.shape, w.shape[0]
    y = torch.empty((B, O), dtype=torch.float32, device=x2.device)
    with _on_device(x2.device):
        stream = torch.cuda.current_stream(x2.device)
        blob = _linear_blob(mod, L, w, weight, kw, stream, cache_ok)
        _lib.check(L.slfp_linear_fwd_prepared(x2.data_ptr(), blob.data_ptr(), _ptr(b), y.data_ptr(), B, I, O, ka, kw, mod.q_bit,
                                              options.mfma_passes, stream.cuda_stream))
    mod.__dict__["_last_kernel"] = "linear_pointwise"
    return y


def _hip_linear_fc(mod, L, x2, w, weight, b, ka, kw, cache_ok, out, relu):
    """slfp_linear_fwd_fc (the caller has asked slfp_linear_fc_supported): x2 is float32 or the uint8 codes written for this module's
    Ka / q_bit; the result is float32 or, with `out` = (Ka, q_bit) of the Linear_Q that reads it, that layer's codes."""
    (B, I), O = x2.shape, w.shape[0]
    io = _conv_io(x2.dtype == torch.uint8, out)
    y = torch.empty((B, O), dtype=torch.uint8 if out is not None else torch.float32, device=x2.device)
    with _on_device(x2.device):
        stream = torch.cuda.current_stream(x2.device)
        blob = _linear_blob(mod, L, w, weight, kw, stream, cache_ok)
        ws_bytes = L.slfp_linear_fc_workspace_bytes(B, I, O, ctypes.byref(io))
        ws = _workspace(x2.device, ws_bytes) if ws_bytes else None
        _lib.check(L.slfp_linear_fwd_fc(x2.data_ptr(), blob.data_ptr(), _ptr(b), y.data_ptr(), B, I, O, ka, kw, mod.q_bit,
                                        options.mfma_passes, ctypes.byref(io), relu, _ptr(ws), stream.cuda_stream))
    mod.__dict__["_last_kernel"] = "linear_fc" + ("+codes_in" if io.x_codes else "") + ("+codes_out" if io.y_codes else "")
    return y


class _SlfpLinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, mod):
        ctx.mod = mod
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return _hip_linear(mod, x, weight, bias)

    @staticmethod
    def backward(ctx, gy):
        mod = ctx.mod
        x, weight = ctx.saved_tensors
        if options.backward in ("hip", "hip_all") and x.is_cuda and x.numel() > 0:
            # the pointwise kernels with rows = the product of the leading dims and H = W = 1
            I, O = x.shape[-1], weight.shape[0]
            x2, gy2 = x.detach().reshape(-1, I).contiguous(), gy.reshape(-1, O).contiguous()
            res = _hip_backward(mod, _conv_desc(mod, (x2.shape[0], I, 1, 1)), x2, weight, gy2, _needs(ctx))
            if res is not None:
                return (res[0].reshape(x.shape) if res[0] is not None else None), res[1], res[2], None
        mod._last_bwd_kernel = "composite"
        ka, kw = _f32(mod.Ka), _f32(mod.Kw)
        g = gy * kw * ka
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = (g @ hip_quantize(weight.detach().contiguous(), kw, _w_fmt(mod.q_bit))) / ka
        if ctx.needs_input_grad[1]:
            xq = hip_quantize(x.detach().contiguous(), ka, _act_fmt(mod.q_bit))
            gw = (g.reshape(-1, g.shape[-1]).t() @ xq.reshape(-1, xq.shape[-1])) / kw
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = gy.reshape(-1, gy.shape[-1]).sum(0)
        return gx, gw, gb, None


def linear_Q(q_bit, Kw, Ka):
    """utils/conv2d_func.py:50-66 (next-row component: same C ABI, pointwise kernel family)."""
    class Linear_Q(nn.Linear):
        def __init__(self, in_features, out_features, Kw=Kw, Ka=Ka, bias=True):
            super(Linear_Q, self).__init__(in_features, out_features, bias)
            self.q_bit = q_bit
            self.quantize_weight = weight_quantize_func(q_bit=q_bit)
            self.quantize_act = act_quantize_func(q_bit=q_bit)
            self.Kw = torch.tensor(Kw)
            self.Ka = torch.tensor(Ka)
            self._prep = _PreparedWeights()
            self._last_input = None
            self._input_q = None
            self._weight_q = None
            self.bias_q = None
            self._last_kernel = None       # what the last forward ran: "linear_pointwise" or "linear_fc[+codes_in][+codes_out]"
            self._last_bwd_kernel = None
            self._grouped_stash = False   # the stash is one image group's (mark_grouped_stash)
            # fusion.link_head: the classifier head on 1-byte codes (inference only)
            self._code_in = False     # a producer writes this layer's codes: only then is a uint8 input taken as codes
            self._code_out = None     # (Ka, q_bit) of the Linear_Q that reads the result: hand it 1-byte codes
            self._code_relu = False   # the ReLU between this layer and its reader, folded into the epilogue
            self._last_codes = None

        # The reference stores input_q / weight_q / bias_q on every forward (utils/conv2d_func.py:60-64) and its nets
        # read them back afterwards (nets_cifar/mobilenetv1.py:169-170, resnet50.py:353-354, alexnet.py:107-114);
        # here the two quantized tensors are computed on first access after a forward.
        @property
        def input_q(self):
            _check_stash(self)
            if self.q_bit != 32 and self._input_q is None and self._last_input is not None:
                self._input_q = hip_quantize(self._last_input, _f32(self.Ka), _act_fmt(self.q_bit))
            elif self.q_bit != 32 and self._input_q is None and self._last_codes is not None:
                # behind a link the input arrived already quantized: input_q = decode(codes), bit for bit
                self._input_q = hip_decode(self._last_codes, _act_fmt(self.q_bit))
            return self._input_q

        @property
        def weight_q(self):
            if self.q_bit != 32 and self._weight_q is None and (self._last_input is not None or self._last_codes is not None):
                self._weight_q = hip_quantize(self.weight.detach().contiguous(), _f32(self.Kw), _w_fmt(self.q_bit))
            return self._weight_q

        def invalidate(self):
            """Drop the cached quantized weights (call after changing `weight.data` in place during inference)."""
            self._prep.invalidate()

        def train(self, mode=True):
            self.invalidate()
            return super(Linear_Q, self).train(mode)

        def forward(self, input):
            if self._grouped_stash:
                self._grouped_stash = False
            if self.q_bit == 32:
                self._input_q = input / self.Ka
                self._weight_q = self.weight / self.Kw
                # the reference dereferences self.bias unconditionally (utils/conv2d_func.py:63)
                self.bias_q = self.bias / self.Kw / self.Ka
                return F.linear(self._input_q, self._weight_q, self.bias_q) * self.Kw * self.Ka
            if self.q_bit not in (8, 7):
                raise UnboundLocalError("q_bit must be 32, 8 or 7 (utils/sfp_quant.py:142-147)")
            if self.bias is None:
                raise TypeError("unsupported operand type(s) for /: 'NoneType' and 'Tensor'")  # as the reference
            x_codes = input.dtype == torch.uint8
            if x_codes and not self._code_in:
                # only a layer that fusion.link_head marked as a reader takes bytes as codes: anything else (a raw uint8 batch)
                # would be decoded into silently wrong activations
                raise TypeError("Linear_Q: expected float32, got torch.uint8 (1-byte codes are read only by a layer that "
                                "fusion.link_head linked to their producer)")
            self._last_input = None if x_codes else input.detach()
            self._last_codes = input.detach() if x_codes else None
            self._input_q = None
            self._weight_q = None
            self.bias_q = self.bias / self.Kw / self.Ka      # utils/conv2d_func.py:63 (the kernel applies the same two divisions)
            if x_codes or self._code_out is not None or self._code_relu:
                # a link of fusion.link_head: 1-byte codes on one or both sides (inference only)
                if self.training:
                    raise RuntimeError("Linear_Q: code links (fusion.link_head) are inference-only; call fusion.unlink_head(model)")
                with torch.no_grad():
                    return _hip_linear(self, input, self.weight, self.bias, cache_ok=True, fc=True)
            need_grad = torch.is_grad_enabled() and (input.requires_grad or self.weight.requires_grad or
                                                     self.bias.requires_grad)
            if need_grad:
                return _SlfpLinearFn.apply(input, self.weight, self.bias, self)
            inference = not self.training and not torch.is_grad_enabled()
            return _hip_linear(self, input, self.weight, self.bias, cache_ok=inference,
                               fc=inference and options.linear_kernel == "fc")

    return Linear_Q
