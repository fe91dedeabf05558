"""Inference-time rewrites of a model built from Conv2d_Q modules: BatchNorm / ReLU folded into the conv epilogues, layers paired into
one kernel, and activations handed from layer to layer as 1-byte codes.  Call everything AFTER load_state_dict and model.eval().

The passes, in the order a pipeline applies them.  "Needs" = what must have run before; "sets" = the module state it writes; every
undo function restores exactly that state; "also undone by" = the other undo functions that take the pass along.

  pass                             needs                              sets                                          undo / also undone by
  fuse_pair(conv, bn, relu)        --                                 conv._post                                    (set _post = None)
  fuse_bn_relu(model)              --                                 _post, _fused_modules; bn / relu slots        unfuse
                                                                      of an nn.Sequential -> nn.Identity
  fuse_named_bn(model, x)          --                                 _post, _named_bn; the bn<k> slot of a hand-   unfuse_named_bn
                                                                      wired block -> nn.Identity
  fuse_dw_pw(model)                fuse_bn_relu; link_codes first     DwPwBlock (._dw_slot) in the pointwise slot,  unfuse_dw_pw / unfuse
                                   where the blocks are to run on     nn.Identity in the depthwise slot
                                   codes (fuse_bn_relu -> link_codes
                                   -> fuse_dw_pw)
  link_codes(model, x)             fuse_bn_relu                       _code_out (x3=True: _code_x3); pools ->       unlink_codes
                                                                      CodeMaxPool2d
  fuse_residual(model, x)          fuse_named_bn                      block: instance forward, _residual_fused;     unfuse_residual
                                                                      conv3: residual_relu, _in_residual
  fuse_fire(model, x)              --                                 block: instance forward, _fire_fused; its     unfuse_fire
                                                                      convs: _post, _code_out, _code_entry; pools
                                                                      -> CodeMaxPool2d
  link_codes_traced(model, x)      fuse_named_bn / fuse_bn_relu;      _code_out, _code_entry, _post with the ReLU   unlink_codes
                                   before or after fuse_residual      bit, _pre_link_post (x3=True: _code_x3);
                                                                      pools -> CodeMaxPool2d
  link_stem(model, x)              the folds, fuse_fire(entries=True) stem: _code_out, _post, _pre_link_post,       unlink_stem / unlink_codes
                                   or link_codes_traced(entries=      _stem_link; pools -> CodeMaxPool2d, ReLUs
                                   True), fuse_residual               -> CodeReLU
  link_trunk(model, x)             fuse_named_bn, fuse_residual,      conv3: _trunk_code_out, _trunk_link           unlink_trunk / unlink_codes,
                                   link_codes_traced(entries=True)                                                  unfuse_residual
  link_layerout(model, x)          fuse_bn_relu                       _code_out, _code_lut; pools -> CodeMaxPool2d, unlink_codes
                                                                      activation modules -> CodeAct
  link_head(model, x)              fuse_bn_relu / link_codes          Linear_Q: _code_in, _code_out, _code_relu;    unlink_head / unlink_codes
                                                                      last conv: _code_out, _post; _head_link;
                                                                      pools -> CodeMaxPool2d, ReLUs -> CodeReLU,
                                                                      identity avg-pools -> CodePass
  use_device_avgpool(model, x)     --                                 global average pools -> GlobalAvgPool2d,      restore_avgpool
                                                                      (_relu), a ReLU in front -> FoldedReLU("avgpool")
  link_pool_head(model, x)         use_device_avgpool; before         pool: _code_out, _pool_link; Linear_Q:        unlink_pool_head /
                                   link_head                          _code_in                                      restore_avgpool
  the TRAINING passes              fusion_train.py: its header has their rows; the names imported at the end of this file are re-exported

The passes that take an example input share one forward trace (`_Trace`), one rule for "the same tensor" (`_Trace.same`), one
eligibility predicate (`_code_eligible`), one record of wrapped children (`_wrap_children` / `_unwrap_children`) and one
verify-or-roll-back step (`_verified`): DESIGN section 20.  The undo functions that put modules back share one slot walk
(`_restore_slots`); a FoldedReLU names the pass that owns it, and only that pass's undo takes it back.
"""
import collections
import ctypes
import warnings

import torch
import torch.nn as nn


def _is_conv_q(m):
    return isinstance(m, nn.Conv2d) and hasattr(m, "q_bit") and hasattr(m, "Ka") and hasattr(m, "_post")


def fold_bn(bn):
    """(scale, shift) float32 with  bn(x) == x * scale + shift  in eval mode."""
    if bn.training or not bn.track_running_stats or bn.running_mean is None:
        raise RuntimeError("fuse_bn_relu: the BatchNorm2d must be in eval mode with running statistics")
    var = bn.running_var.detach().double()
    mean = bn.running_mean.detach().double()
    gamma = bn.weight.detach().double() if bn.affine else torch.ones_like(var)
    beta = bn.bias.detach().double() if bn.affine else torch.zeros_like(var)
    scale = gamma / torch.sqrt(var + bn.eps)
    shift = beta - mean * scale
    return scale.float().contiguous(), shift.float().contiguous()


def fuse_pair(conv, bn=None, relu=False, layerout=False):
    """Attach bn (eval-mode nn.BatchNorm2d or None), an optional SFP<4,4> layer-output quantizer
    (utils/sfp_quant.py:105-133; needs bn) and an optional ReLU to `conv`'s epilogue, in that order."""
    if not _is_conv_q(conv):
        raise TypeError("fuse_pair: conv must be a Conv2d_Q module of this package")
    if layerout and bn is None:
        raise ValueError("fuse_pair: the layer-output quantizer is fused only together with a BatchNorm2d")
    flags = (1 if relu else 0) | (2 if layerout else 0)   # SLFP_POST_RELU | SLFP_POST_LAYEROUT
    if bn is not None:
        if bn.num_features != conv.out_channels:
            raise ValueError("fuse_pair: BatchNorm2d width does not match the conv's out_channels")
        scale, shift = fold_bn(bn)
        dev = conv.weight.device
        conv._post = (scale.to(dev), shift.to(dev), flags)
    else:
        conv._post = (None, None, flags)
    return conv


def _is_layerout(m):
    """layerout_quantize_func(q_bit <= 8): the SFP<4,4> quantizer module of the `*_swish` / `*_gelu` / ShuffleNetV2 nets."""
    return type(m).__name__ == "layerout_quantize_func" and getattr(m, "q_bit", 32) in (8, 7)


def fuse_bn_relu(model, dw_pw=False):
    """Fuse every [Conv2d_Q, BatchNorm2d(eval), (layerout_quantize_func), (ReLU)] run found in nn.Sequential
    containers (nets_imgnet/mobilenetv1.py:24-41; nets_cifar/mobilenetv1.py:196-231 for the layerout form; a
    Swish / GELU after the quantizer stays a module).  Returns the number of fused convolutions.
    dw_pw=True additionally pairs depthwise and pointwise convs into one kernel where supported (fuse_dw_pw)."""
    n = 0
    for seq in [m for m in model.modules() if isinstance(m, nn.Sequential)]:
        names = list(seq._modules.keys())
        i = 0
        while i < len(names):
            conv = seq._modules[names[i]]
            if _is_conv_q(conv) and conv._post is None and i + 1 < len(names):
                bn = seq._modules[names[i + 1]]
                ok = (isinstance(bn, nn.BatchNorm2d) and not bn.training and bn.num_features == conv.out_channels
                      and (conv.bias is None or getattr(conv, "_scaled_bias", False)))
                if ok:
                    j = i + 2
                    lo = (j < len(names) and _is_layerout(seq._modules[names[j]]) and conv.q_bit in (8, 7))
                    j += 1 if lo else 0
                    relu = j < len(names) and isinstance(seq._modules[names[j]], nn.ReLU)
                    j += 1 if relu else 0
                    fuse_pair(conv, bn, relu, lo)
                    conv._fused_modules = [(names[k], seq._modules[names[k]]) for k in range(i + 1, j)]
                    for k in range(i + 1, j):
                        seq._modules[names[k]] = nn.Identity()
                    n += 1
                    i = j
                    continue
            i += 1
    if dw_pw:
        fuse_dw_pw(model)
    return n


def unfuse(model):
    """Undo fuse_bn_relu (restores the original BatchNorm2d / ReLU modules; un-pairs DwPwBlocks first)."""
    unfuse_dw_pw(model)
    n = 0
    for seq in [m for m in model.modules() if isinstance(m, nn.Sequential)]:
        names = list(seq._modules.keys())
        for i, name in enumerate(names):
            conv = seq._modules[name]
            if _is_conv_q(conv) and conv._post is not None and hasattr(conv, "_fused_modules"):
                for key, mod in conv._fused_modules:
                    seq._modules[key] = mod
                conv._post = None
                del conv._fused_modules
                n += 1
    return n


def fuse_named_bn(model, example_input=None, rtol=None):
    """Blocks that wire conv -> bn by hand in their forward() (the reference's ResNet-50 Bottleneck,
    nets_imgnet/resnet50.py:24-100: self.conv1 / self.bn1 / self.relu ...) cannot be rewritten by position, but they
    follow the torchvision naming: every Conv2d_Q child called `<prefix>conv<suffix>` whose sibling `<prefix>bn<suffix>`
    is an eval-mode BatchNorm2d of matching width gets that BatchNorm folded into its epilogue (the shared ReLU module
    stays where it is: it is also applied after the residual add), and the BatchNorm child becomes nn.Identity.
    Because a name is only a convention, pass `example_input`: one forward records what every BatchNorm is actually fed,
    and a pair is folded only if bn<k>'s input IS conv<k>'s output tensor (the wiring itself is checked, not a numerical
    consequence of it: in a deep quantized net a one-ulp change of an activation flips codes downstream and moves the
    logits by percents -- SURVEY section 7 -- so an output tolerance cannot tell a wrong pairing from rounding).
    `rtol`: optionally ALSO require the model's output to move by at most this much (tensor-relative); on failure
    everything is rolled back and a RuntimeError says so.  Returns the number of folded pairs; `unfuse_named_bn(model)`
    restores the modules."""
    y0 = None
    conv_out, bn_in = {}, {}
    if example_input is not None:
        tr = _Trace(model, example_input)
        y0 = tr.output
        conv_out = {c.mod: c.out for c in tr.calls if _is_conv_q(c.mod)}
        bn_in = {c.mod: c.x for c in tr.calls if isinstance(c.mod, nn.BatchNorm2d)}
        tr.release()
    done = []
    for parent in model.modules():
        if isinstance(parent, nn.Sequential):
            continue   # positional runs are fuse_bn_relu's job
        for name, conv in list(parent._modules.items()):
            if not _is_conv_q(conv) or conv._post is not None or "conv" not in name:
                continue
            bn_name = name.replace("conv", "bn", 1)
            bn = parent._modules.get(bn_name)
            if not isinstance(bn, nn.BatchNorm2d) or bn.training or bn.num_features != conv.out_channels:
                continue
            if conv.bias is not None and not getattr(conv, "_scaled_bias", False):
                continue
            # `is`, not _Trace.same: this pass has no bit-exact verification behind it
            if example_input is not None and (conv not in conv_out or bn_in.get(bn) is not conv_out[conv]):
                continue   # forward() does not apply this bn to this conv's output
            fuse_pair(conv, bn, relu=False)
            conv._named_bn = (parent, bn_name, bn)
            parent._modules[bn_name] = nn.Identity()
            done.append(conv)
    conv_out.clear()
    bn_in.clear()
    if y0 is not None and done and rtol is not None:
        with torch.no_grad():
            y1 = model(example_input)
        err = float((y1 - y0).abs().max() / y0.abs().max().clamp_min(1e-30))
        if not err <= rtol:
            unfuse_named_bn(model)
            raise RuntimeError(f"fuse_named_bn: the model's output moved by {err:.3e} (> {rtol}); nothing was changed")
    return len(done)


def unfuse_named_bn(model):
    """Undo fuse_named_bn."""
    n = 0
    for conv in model.modules():
        if _is_conv_q(conv) and hasattr(conv, "_named_bn"):
            parent, bn_name, bn = conv._named_bn
            parent._modules[bn_name] = bn
            conv._post = None
            del conv._named_bn
            n += 1
    return n


# ------------------------------------------------------------------ depthwise + pointwise in one kernel
class DwPwBlock(nn.Module):
    """[Conv2d_Q 3x3 depthwise, BN, ReLU, Conv2d_Q 1x1, (BN), (ReLU)] as one launch (csrc/conv_dwpw.hip).  Holds the two
    original conv modules (parameters, state-dict keys and scales unchanged: `dw`, `pw`); inference only.  Falls back
    to running them one after the other when the input is not a channels_last ROCm tensor of a supported size.
    A block whose two convs were linked by link_codes BEFORE fuse_dw_pw paired them (the supported order: fuse_bn_relu ->
    link_codes(model, example) -> fuse_dw_pw) reads uint8 codes and runs as one kernel on codes (csrc/conv_dwpw_codes.hip,
    `_forward_codes`) for the pairs in options.dwpw_codes_pairs -- empty by default -- or all supported ones under
    options.dwpw_all; `_last_kernel` then ends in "+codes_in" or "+codes_in+codes_out".  Otherwise its two convs run their
    code kernels."""

    def __init__(self, dw, pw):
        super().__init__()
        self.dw = dw
        self.pw = pw
        self._last_kernel = None

    def forward(self, x):
        from . import _lib
        from .conv2d_func import _conv_desc, _conv_weights, _epilogue_args, _ptr, options
        dw, pw = self.dw, self.pw
        if x.dtype == torch.uint8:
            y = self._forward_codes(x)
            if y is None:
                self._last_kernel = None
                y = pw(dw(x))
            return y
        ok = (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)
              and not self.training and not torch.is_grad_enabled() and options.mfma_passes in (_lib.MFMA_DEFAULT, _lib.MFMA_F16X1)
              and dw.q_bit in (8, 7) and dw._post is not None and dw._post[0] is not None and not (int(dw._post[2]) & 2)
              and pw._post is not None and not (int(pw._post[2]) & 2))
        # measured (profiles/dwpw_bench.py): the one-kernel form only pays on the 32-channel stride-1
        # block; the wider ones run faster as two kernels until the kernel's next version.  options.dwpw_all forces it.
        if ok and not getattr(options, "dwpw_all", False):
            ok = (dw.in_channels, int(dw.stride[0])) in getattr(options, "dwpw_pairs", {(32, 1)})
        if not ok:
            self._last_kernel = None
            return pw(dw(x))
        L = _lib.load()
        N = x.shape[0]
        d1 = _conv_desc(dw, x.shape)
        ho, wo = ctypes.c_int64(), ctypes.c_int64()
        with torch.cuda.device(x.device):
            _lib.check(L.slfp_conv2d_out_shape(ctypes.byref(d1), ctypes.byref(ho), ctypes.byref(wo)))
            d2 = _conv_desc(pw, (N, dw.out_channels, ho.value, wo.value))
            if not L.slfp_dwpw_supported(ctypes.byref(d1), ctypes.byref(d2)):
                self._last_kernel = None
                return pw(dw(x))
            stream = torch.cuda.current_stream(x.device)
            b1 = _conv_weights(dw, d1, dw.weight, stream, True)
            b2 = _conv_weights(pw, d2, pw.weight, stream, True)
            _, s1, h1, f1 = _epilogue_args(dw, None, x.device)
            bias2, s2, h2, f2 = _epilogue_args(pw, pw.bias if getattr(pw, "_scaled_bias", False) else None, x.device)
            if pw.bias is not None and bias2 is None:
                return pw(dw(x))   # conv2d_Q's raw bias is added outside the kernels
            y = torch.empty((N, pw.out_channels, ho.value, wo.value), dtype=torch.float32, device=x.device,
                            memory_format=torch.channels_last)
            _lib.check(L.slfp_dwpw_fwd(ctypes.byref(d1), ctypes.byref(d2), x.data_ptr(), b1.data_ptr(), s1.data_ptr(), h1.data_ptr(),
                                       f1 & 1, b2.data_ptr(), _ptr(bias2), _ptr(s2), _ptr(h2), f2 & 1, y.data_ptr(), stream.cuda_stream))
        self._last_kernel = "dwpw_fused_f16x1" if dw.q_bit == 8 else "dwpw_fused_f16_exact"
        dw._last_input, dw._input_q = x.detach(), None
        pw._last_input, pw._input_q = None, None   # the pointwise input never exists as a tensor
        for m in (dw, pw):
            if m._grouped_stash:
                m._grouped_stash = False
        return y

    def _forward_codes(self, x):
        """The pair inside a chain of codes (link_codes before fuse_dw_pw): `x` holds the depthwise layer's input codes and the
        depthwise layer writes this pointwise layer's codes.  ONE slfp_dwpw_fwd_codes launch (csrc/conv_dwpw_codes.hip) -> the next
        layer's codes (pw._code_out) or float32, bit-identical to the two code kernels; None where the pair does not take it: not
        linked to each other, a layer-output table, a raw bias, a pair outside options.dwpw_codes_pairs (options.dwpw_all: every
        pair), or one slfp_dwpw_codes_supported refuses."""
        from . import _lib
        from .conv2d_func import _conv_desc, _conv_io, _conv_weights, _epilogue_args, _ptr, options
        dw, pw = self.dw, self.pw
        out = pw._code_out
        ok = (x.is_cuda and x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)
              and not self.training and not torch.is_grad_enabled() and dw.q_bit in (8, 7)
              and dw._post is not None and dw._post[0] is not None and dw.bias is None
              and dw._code_out is not None and dw._code_out == _reader_quant(pw)
              and (out is None or (isinstance(out, tuple) and len(out) == 2))
              and dw._code_lut is None and pw._code_lut is None
              and (pw.bias is None or getattr(pw, "_scaled_bias", False)))
        if ok and not getattr(options, "dwpw_all", False):
            ok = (dw.in_channels, int(dw.stride[0])) in options.dwpw_codes_pairs
        if not ok:
            return None
        L = _lib.load()
        N = x.shape[0]
        d1 = _conv_desc(dw, x.shape)
        io = _conv_io(True, out)
        ho, wo = ctypes.c_int64(), ctypes.c_int64()
        with torch.cuda.device(x.device):
            if L.slfp_conv2d_out_shape(ctypes.byref(d1), ctypes.byref(ho), ctypes.byref(wo)) != _lib.OK:
                return None
            d2 = _conv_desc(pw, (N, dw.out_channels, ho.value, wo.value))
            _, s1, h1, f1 = _epilogue_args(dw, None, x.device)
            bias2, s2, h2, f2 = _epilogue_args(pw, pw.bias, x.device)
            if not L.slfp_dwpw_codes_supported(ctypes.byref(d1), ctypes.byref(d2), ctypes.byref(io), 1 if bias2 is not None else 0, f1, f2):
                return None
            stream = torch.cuda.current_stream(x.device)
            b1 = _conv_weights(dw, d1, dw.weight, stream, True)
            b2 = _conv_weights(pw, d2, pw.weight, stream, True)
            y = torch.empty((N, pw.out_channels, ho.value, wo.value), dtype=torch.uint8 if out is not None else torch.float32,
                            device=x.device, memory_format=torch.channels_last)
            _lib.check(L.slfp_dwpw_fwd_codes(ctypes.byref(d1), ctypes.byref(d2), ctypes.byref(io), x.data_ptr(), b1.data_ptr(),
                                             s1.data_ptr(), h1.data_ptr(), f1, b2.data_ptr(), _ptr(bias2), _ptr(s2), _ptr(h2), f2,
                                             y.data_ptr(), stream.cuda_stream))
        self._last_kernel = (("dwpw_fused_f16x1" if dw.q_bit == 8 else "dwpw_fused_f16_exact") + "+codes_in"
                             + ("+codes_out" if out is not None else ""))
        dw.__dict__.update(_last_codes=x.detach(), _last_input=None, _input_q=None)
        pw.__dict__.update(_last_codes=None, _last_input=None, _input_q=None)   # the pointwise input never exists as a tensor
        for m in (dw, pw):
            if m._grouped_stash:
                m._grouped_stash = False
        return y


def _is_dw(m):
    return _is_conv_q(m) and m.groups == m.in_channels == m.out_channels and tuple(m.kernel_size) == (3, 3)


def _is_pw(m):
    return _is_conv_q(m) and m.groups == 1 and tuple(m.kernel_size) == (1, 1) and tuple(m.stride) == (1, 1)


def fuse_dw_pw(model):
    """After fuse_bn_relu: replace every [depthwise Conv2d_Q (+BN+ReLU folded), Identity..., pointwise Conv2d_Q (+BN+ReLU
    folded)] run of an nn.Sequential by one DwPwBlock (the pointwise slot; the depthwise slot becomes nn.Identity).
    Whether a pair really runs as one kernel is decided per call (input layout, size, libslfp_hip's
    slfp_dwpw_supported); otherwise the block runs its two convs as before.  Returns the number of blocks formed.
    With 1-byte codes the supported order is fuse_bn_relu -> link_codes(model, example) -> fuse_dw_pw: the links are made on the
    plain convs, and a block whose depthwise conv writes its pointwise conv's codes may then run as one kernel on codes
    (DwPwBlock._forward_codes; options.dwpw_codes_pairs / dwpw_all).  unfuse_dw_pw and unfuse put the linked convs back as they
    are; unlink_codes reaches blk.dw / blk.pw through model.modules(), and the block then takes float32 again.  link_codes on a
    model that already holds DwPwBlocks does what it did before: it does not look inside them."""
    n = 0
    for seq in [m for m in model.modules() if isinstance(m, nn.Sequential)]:
        names = list(seq._modules.keys())
        i = 0
        while i < len(names):
            dw = seq._modules[names[i]]
            if _is_dw(dw) and dw._post is not None and dw._post[0] is not None:
                j = i + 1
                while j < len(names) and isinstance(seq._modules[names[j]], nn.Identity):
                    j += 1
                if j < len(names) and _is_pw(seq._modules[names[j]]) and seq._modules[names[j]]._post is not None \
                        and seq._modules[names[j]].in_channels == dw.out_channels:
                    pw = seq._modules[names[j]]
                    blk = DwPwBlock(dw, pw)
                    blk.train(dw.training)   # a new module starts in training mode; follow the convs
                    blk._dw_slot = names[i]
                    seq._modules[names[j]] = blk
                    seq._modules[names[i]] = nn.Identity()
                    n += 1
                    i = j + 1
                    continue
            i += 1
    return n


def unfuse_dw_pw(model):
    """Undo fuse_dw_pw."""
    n = 0
    for seq in [m for m in model.modules() if isinstance(m, nn.Sequential)]:
        names = list(seq._modules.keys())
        for j, name in enumerate(names):
            blk = seq._modules[name]
            if isinstance(blk, DwPwBlock):
                seq._modules[blk._dw_slot] = blk.dw
                seq._modules[name] = blk.pw
                n += 1
    return n


# ------------------------------------------------------------------ 1-byte activation codes between layers
class CodeMaxPool2d(nn.Module):
    """An nn.MaxPool2d inside a code chain (link_codes): uint8 codes are pooled as codes (slfp_maxpool2d_codes, or
    slfp_maxpool2d_codes_ex where the pool has ceil_mode=True -- fuse_fire wraps such pools: the class of a
    window's largest input -- bit-identical to pooling the float32 tensor and encoding it), anything else goes to the original
    module, which this wrapper keeps (`pool`; it has no parameters, the state dict does not change)."""

    def __init__(self, pool, q_bit):
        super().__init__()
        self.pool = pool
        self.q_bit = int(q_bit)

    def forward(self, x):
        if x.dtype == torch.uint8:
            from .sfp_quant import hip_maxpool_codes
            p = self.pool
            return hip_maxpool_codes(x, p.kernel_size, p.stride, p.padding, self.q_bit, ceil_mode=bool(p.ceil_mode))
        return self.pool(x)


class CodeReLU(nn.Module):
    """An nn.ReLU behind a stem linked by link_stem: the ReLU is folded into the stem's code quantizer, so on uint8 codes the
    module hands its input through without a launch (torch.relu on codes would be an identity pass over the whole tensor);
    anything else goes to the original module, which this wrapper keeps (`relu`)."""

    def __init__(self, relu):
        super().__init__()
        self.relu = relu

    def forward(self, x):
        return x if x.dtype == torch.uint8 else self.relu(x)


class CodeAct(nn.Module):
    """An elementwise activation module (Swish, nn.GELU, ...) behind a producer linked by link_layerout: the activation is part of
    the producer's byte table, so uint8 codes pass through without a launch; anything else goes to the original module, which this
    wrapper keeps (`act`; the activations have no parameters, the state dict does not change)."""

    def __init__(self, act):
        super().__init__()
        self.act = act

    def forward(self, x):
        return x if x.dtype == torch.uint8 else self.act(x)


def _poolable(m):
    return (isinstance(m, nn.MaxPool2d) and not m.ceil_mode and not m.return_indices
            and (m.dilation == 1 or m.dilation == (1, 1)))


# ------------------------------------------------------------------ what the passes that take an example input share
class _Call(collections.namedtuple("_Call", "mod inp out")):
    """One recorded module call: the module, its positional inputs, its output."""
    __slots__ = ()

    @property
    def x(self):
        """The first positional input, or None."""
        return self.inp[0] if self.inp else None


class _Trace:
    """One no_grad forward of `model` on `example_input`, recorded.  `calls` holds, in execution order, a _Call for every Conv2d_Q
    (not a leaf: it owns its quantizer children), every leaf module and every module in `blocks`; containers only hand their input on.
    `output` is what the model returned.  Every recorded tensor is kept alive until release(), so an address names one tensor: that
    is what `same` rests on.  A pass calls release() before it runs the model again -- a trace holds every activation of the net --
    and keeps `output` for the comparison."""

    def __init__(self, model, example_input, blocks=()):
        self.calls, self._of, self._made, self._read = [], {}, {}, {}
        blocks = set(blocks)
        hooks = [m.register_forward_hook(lambda mod, inp, out: self.calls.append(_Call(mod, inp, out)))
                 for m in model.modules() if _is_conv_q(m) or not m._modules or m in blocks]
        try:
            with torch.no_grad():
                self.output = model(example_input)
        finally:
            for h in hooks:
                h.remove()
        for c in self.calls:
            self._of.setdefault(c.mod, []).append(c)
            if torch.is_tensor(c.out):
                self._made.setdefault(self._key(c.out), []).append(c)
            if torch.is_tensor(c.x):
                self._read.setdefault(self._key(c.x), []).append(c)

    @staticmethod
    def _key(t):
        return (t.data_ptr(), t.shape, t.dtype, t.stride())

    def release(self):
        """Drop every recorded call and with it the recorded tensors; `output` stays."""
        self.calls.clear(); self._of.clear(); self._made.clear(); self._read.clear()

    def same(self, a, b):
        """Is `b` the tensor `a`: the same object, or the same address, shape, dtype and strides (what nn.Identity or an in-place
        ReLU returns; a pooled or computed tensor never is)."""
        return a is b or (torch.is_tensor(a) and torch.is_tensor(b) and self._key(a) == self._key(b))

    def of(self, mod):
        """The recorded calls of `mod`; runs(mod) is their number."""
        return self._of.get(mod, [])

    def runs(self, mod):
        return len(self.of(mod))

    def io(self, mod):
        """(input, output) of `mod`, or None unless it ran exactly once with one positional input, tensor in and tensor out."""
        calls = self.of(mod)
        if len(calls) != 1 or len(calls[0].inp) != 1 or not torch.is_tensor(calls[0].x) or not torch.is_tensor(calls[0].out):
            return None
        return calls[0].x, calls[0].out

    def readers(self, t):
        """The calls whose first input is `t`, in execution order."""
        return self._read.get(self._key(t), []) if torch.is_tensor(t) else []

    def producer(self, t, kind):
        """The first call of a module with kind(module) whose output is `t`, or None.  `kind` is needed because an in-place ReLU
        behind nn.Identity behind a conv makes three calls return one tensor."""
        return next((c for c in (self._made.get(self._key(t), []) if torch.is_tensor(t) else []) if kind(c.mod)), None)


def _post_flags(m):
    """The SLFP_POST_* bits of Conv2d_Q `m`'s epilogue (1 = ReLU, 2 = layer-output quantizer); 0 without one."""
    return int(m._post[2]) if m._post is not None else 0


def _fold_flags(m, flags):
    """Give Conv2d_Q `m`'s epilogue these flag bits, keeping its (scale, shift)."""
    m._post = ((m._post[0], m._post[1]) if m._post is not None else (None, None)) + (flags,)


def _reader_quant(b):
    """(float(Ka), q_bit): the quantizer of Conv2d_Q `b`, which a producer that writes b's codes applies."""
    from .conv2d_func import _scalar_scale
    return float(_scalar_scale(b.Ka, "Ka")), int(b.q_bit)


def _code_eligible(m, producer_side=False):
    """Can Conv2d_Q `m` read codes: 8 / 7 bit, eval mode, numeric padding, no raw bias, no layer-output quantizer.  producer_side: can
    it be given codes to write: also no `_code_out` yet, and not the conv3 of a fuse_residual block."""
    if not _is_conv_q(m) or producer_side and (m._code_out is not None or getattr(m, "_in_residual", False)):
        return False   # _in_residual: the module's output is the block's float32 trunk (conv + identity), not a conv output
    return (m.q_bit in (8, 7) and not m.training and isinstance(m.padding, tuple)
            and (m.bias is None or getattr(m, "_scaled_bias", False)) and not (_post_flags(m) & 2))


def _wrap_children(model, pools, q_bit, relus=(), acts=()):
    """Replace every child slot of `model` that holds one of `pools` / `relus` / `acts` by CodeMaxPool2d(pool, q_bit) / CodeReLU(relu) /
    CodeAct(act).  Returns the (parent, name, original) records that _unwrap_children takes."""
    recs = []
    for parent in [m for m in model.modules() if not isinstance(m, (CodeMaxPool2d, CodeReLU, CodeAct))]:
        for name, child in list(parent._modules.items()):
            if any(child is pm for pm in pools):
                parent._modules[name] = CodeMaxPool2d(child, q_bit)
            elif any(child is rm for rm in relus):
                parent._modules[name] = CodeReLU(child)
            elif any(child is am for am in acts):
                parent._modules[name] = CodeAct(child)
            else:
                continue
            recs.append((parent, name, child))
    return recs


def _unwrap_children(recs):
    """The inverse of _wrap_children; a slot that no longer holds the wrapper of its original is left alone."""
    for parent, name, orig in recs:
        now = parent._modules.get(name)
        if (isinstance(now, CodeMaxPool2d) and now.pool is orig or isinstance(now, CodeReLU) and now.relu is orig
                or isinstance(now, CodeAct) and now.act is orig):
            parent._modules[name] = orig


def _verified(fn, want, undo, reraise=False, warn=None):
    """Run fn() under no_grad and return True if the result is a tensor of `want`'s dtype and shape with torch.equal(result, want)
    (`want`: a tensor, or a function that makes it after fn has run).  Anything else is a refusal: undo() is called and False
    returned -- also for an exception, e.g. a functional op on the tensor that cannot take codes (`warn`: a text with one {} for
    "<type>: <message>", issued as a warning).  reraise: an _lib.SlfpError is not a refusal -- libslfp_hip refused or failed a call
    the support queries had granted, a defect -- and propagates after undo().  DESIGN section 20 lists which pass sets it."""
    from . import _lib
    ok = False
    try:
        with torch.no_grad():
            got = fn()
            ref = want() if callable(want) else want
        ok = torch.is_tensor(got) and got.dtype == ref.dtype and got.shape == ref.shape and torch.equal(got, ref)
    except _lib.SlfpError:
        if reraise:
            undo()
            raise
    except Exception as e:
        if warn is not None:
            warnings.warn(warn.format(f"{type(e).__name__}: {e}"), stacklevel=2)   # the pass is the one that warns
    if not ok:
        undo()
    return ok


def link_codes(model, example_input=None, x3=False):
    """After fuse_bn_relu: wherever a Conv2d_Q's (fused BN + ReLU) output feeds the next Conv2d_Q of an nn.Sequential
    directly (only nn.Identity in between -- nets_imgnet/mobilenetv1.py:24-33 after fusion), link the two: the producer's
    epilogue applies the CONSUMER's quantize_act(. / Ka) (utils/conv2d_func.py:21) and stores 1-byte codes, the consumer
    decodes them (libslfp_hip: slfp_conv2d_fwd_codes).  Same classes, same values: the net's output is bit-identical to
    the unlinked fused net (single-pass MFMA mode / SFP<3,3>), activations cross HBM as 1 B per element instead of 4.
    With `example_input` (a channels_last ROCm batch) only links for which both kernels exist are made (one forward
    records the shapes); without it every candidate is linked and combinations without a kernel run through the float32
    interface plus an encode / decode pass (correct, slower).  Inference only.  Returns the number of links.
    Call it BEFORE fuse_dw_pw (fuse_bn_relu -> link_codes -> fuse_dw_pw): a DwPwBlock is not a Conv2d_Q, so a block formed earlier
    is neither linked to its neighbours nor inside.
    x3=True (options.mfma_passes = 3, the float32-equivalent mode): a side of a candidate link that reads codes and that
    slfp_conv2d_codes_supported refuses -- every 1x1 layer in that mode -- is accepted where slfp_conv2d_codes_x3_supported says yes;
    the module is marked `_code_x3` and runs slfp_conv2d_fwd_codes_x3 (`_last_kernel` ends in "+x3"), bit-identical to the unlinked
    three-pass net.  The default marks nothing and keeps every link count what it was."""
    from .conv2d_func import _supported
    shapes = {}
    if example_input is not None:
        tr = _Trace(model, example_input)
        shapes = {c.mod: tuple(c.x.shape) for c in tr.calls if _is_conv_q(c.mod)}
        tr.release()

    def supported(m, x_codes, out):   # False, or what takes the layer: True ("codes") / "codes_x3"
        if example_input is None:
            return True
        shp = shapes.get(m)
        if shp is None or len(shp) != 4:
            return False
        if _supported(m, shp, "codes", x_codes, out, _post_flags(m)):
            return True
        return "codes_x3" if x3 and x_codes and _supported(m, shp, "codes_x3", True, out, _post_flags(m)) else False

    def mark(m, how):   # without shapes every code reader may try the three-pass entry point ("codes" is asked first)
        if how == "codes_x3" or (x3 and example_input is None):
            m._code_x3 = True

    def flat(seq):   # an nn.Sequential of nn.Sequentials runs its leaves in order (conv_bn / conv_dw blocks of the reference nets)
        for m in seq._modules.values():
            if isinstance(m, nn.Sequential):
                yield from flat(m)
            else:
                yield m

    nested = {c for m in model.modules() if isinstance(m, nn.Sequential) for c in m._modules.values() if isinstance(c, nn.Sequential)}
    n_links = 0
    for seq in [m for m in model.modules() if isinstance(m, nn.Sequential) and m not in nested]:
        allm = [m for m in flat(seq) if not isinstance(m, nn.Identity)]
        # nn.MaxPool2d modules between two convs stay inside the chain (CodeMaxPool2d): drop them from the adjacency list and
        # remember which ones sit behind each conv
        mods, pools_after = [], {}
        for m in allm:
            if _poolable(m) and mods and _code_eligible(mods[-1]):
                pools_after.setdefault(len(mods) - 1, []).append(m)
            else:
                mods.append(m)
        # candidate links: consecutive eligible convs
        cand = [i for i in range(len(mods) - 1) if _code_eligible(mods[i]) and _code_eligible(mods[i + 1])]
        # a conv can consume codes only if its producer link exists; walk left to right and keep links whose two sides have kernels
        linked_in = set()
        for i in cand:
            a, b = mods[i], mods[i + 1]
            out = _reader_quant(b)
            a_in = i in linked_in                       # does `a` itself read codes?
            how_a = supported(a, a_in, out)
            if not how_a:
                # head of a run without a float32 -> codes kernel: enter the chain through one slfp_encode_f32 pass if at least
                # two more layers then run on codes
                if a_in or not (i + 1 in cand and supported(b, True, _reader_quant(mods[i + 2]))):
                    continue
            # b with codes in: it may or may not write codes itself; require the float32-out form here (the code-out form is
            # checked when its own link is made; if that fails b keeps float32 out)
            how_b = supported(b, True, None)
            if not how_b:
                continue
            if pools_after.get(i) and a.out_channels % 4:
                continue   # slfp_maxpool2d_codes needs C % 4 == 0
            if a_in:
                mark(a, how_a)
            mark(b, how_b)
            a._code_out = out
            linked_in.add(i + 1)
            n_links += 1
            _wrap_children(model, pools_after.get(i, ()), b.q_bit)   # the pools between a and b now see codes
    return n_links


def link_codes_traced(model, example_input, entries=False, x3=False):
    """link_codes for blocks that wire their layers by hand in forward() (the reference's ResNet-50 Bottleneck,
    nets_imgnet/resnet50.py:74-100: conv1 -> bn1 -> relu -> conv2 -> bn2 -> relu -> conv3 -> bn3 -> (+ identity) -> relu, with ONE
    shared nn.ReLU).  One forward records the tensors: a Conv2d_Q `b` whose input IS the output of a Conv2d_Q `a` -- directly or
    through nn.Identity (a folded BatchNorm, fuse_named_bn) and / or an nn.ReLU module -- is a candidate; `a` gets the ReLU
    folded into its epilogue (the module's own relu() then runs on the uint8 codes, where it is the identity) and writes `b`'s
    codes.  Links are made only where libslfp_hip has both kernels (slfp_conv2d_codes_supported), never for a producer with
    two consumers, and the whole set is VERIFIED: the linked model must reproduce the unlinked output bit for bit on
    `example_input`, otherwise (a functional use of the tensor that hooks cannot see, e.g. a torch.cat) everything is rolled
    back and 0 is returned.  Inference only; unlink_codes undoes it.  Returns the number of links.
    entries=True: a producer `a` that reads float32 and has no kernel under slfp_conv2d_codes_supported is accepted as well where
    slfp_conv2d_entry_supported says yes (a 1x1 layer: conv1 of every Bottleneck, which reads the float32 trunk); it gets
    `_code_entry = True` and runs slfp_conv2d_fwd_entry.  Everything else -- one consumer only, ReLU folding, pools, verification,
    roll-back -- is the same; the default keeps every link count what it was.
    x3=True: as link_codes(x3=True) -- a code-reading side that slfp_conv2d_codes_supported refuses is accepted where
    slfp_conv2d_codes_x3_supported says yes (the 1x1 layers in the float32-equivalent mode: conv2 -> conv3 of every Bottleneck) and
    marked `_code_x3`; verification and roll-back are the same."""
    from .conv2d_func import _supported
    tr = _Trace(model, example_input)
    y0 = tr.output
    order = [c.mod for c in tr.calls if _is_conv_q(c.mod)]
    if len(order) != len(set(order)):
        return 0   # a module that runs twice per forward has no single producer / consumer

    def x_of(m):
        return tr.of(m)[0].x

    def supported(m, x_codes, out, flags):   # False, or what takes the layer: True ("codes") / "codes_x3"
        if x_of(m).dim() != 4:
            return False
        if _supported(m, x_of(m).shape, "codes", x_codes, out, flags):
            return True
        return "codes_x3" if x3 and x_codes and _supported(m, x_of(m).shape, "codes_x3", True, out, flags) else False

    cand = {}
    for b in order:
        t, via_relu, pools = x_of(b), False, []
        for _ in range(4):   # look back through nn.ReLU / nn.MaxPool2d modules (a ReLU'd tensor pools the same either way)
            relu, pool = tr.producer(t, lambda m: isinstance(m, nn.ReLU)), tr.producer(t, _poolable)
            if relu is not None:
                t, via_relu = relu.x, True
            elif pool is not None and tr.runs(pool.mod) == 1:
                t = pool.x
                pools.append(pool.mod)
            else:
                break
        a = tr.producer(t, _is_conv_q)
        a = a.mod if a is not None else None
        if a is None or a is b or not _code_eligible(a, producer_side=True) or not _code_eligible(b):
            continue
        if x_of(b).dtype == torch.uint8:
            continue   # already linked
        if pools and a.out_channels % 4:
            continue   # slfp_maxpool2d_codes needs C % 4 == 0
        cand.setdefault(a, []).append((b, via_relu, pools))
    made, reads_codes, wrapped, marked = [], set(), [], []
    for a in order:   # execution order: whether `a` itself reads codes is known when its own link is decided
        if a not in cand or len(cand[a]) != 1:
            continue
        b, via_relu, pools = cand[a][0]
        flags = _post_flags(a) | (1 if via_relu else 0)
        out = _reader_quant(b)
        # does `a` itself read codes (an earlier link)?  uint8 into a stem marked by link_image_u8 is pixels, not codes
        a_in = a in reads_codes or (x_of(a).dtype == torch.uint8 and a._image_table is None)
        entry = False
        how_a = supported(a, a_in, out, flags)
        if not how_a:
            entry = (entries and not a_in and x_of(a).dim() == 4
                     and _supported(a, x_of(a).shape, "entry", False, out, flags))
            if not entry:
                continue
        how_b = supported(b, True, b._code_out, _post_flags(b))
        if not how_b:
            continue
        for m, how in ((a, how_a), (b, how_b)):
            if how == "codes_x3" and not m._code_x3:
                m._code_x3 = True
                marked.append(m)
        made.append((a, a._post))
        a._code_entry = entry
        a._pre_link_post = a._post
        _fold_flags(a, flags)
        a._code_out = out
        reads_codes.add(b)
        wrapped += _wrap_children(model, pools, b.q_bit)   # the pools between a and b now see codes
    if not made:
        return 0
    tr.release()

    def undo():
        for a, post in made:
            a._post, a._code_out, a._code_entry = post, None, False
            del a._pre_link_post
        for m in marked:
            m._code_x3 = False
        _unwrap_children(wrapped)

    return len(made) if _verified(lambda: model(example_input), y0, undo) else 0


def unlink_codes(model):
    """Undo link_codes / link_codes_traced / link_stem / link_layerout (and, uncounted, every link of link_trunk: its producers read
    codes)."""
    n = 0
    unlink_trunk(model)
    unlink_head(model)   # (uncounted, as link_trunk's: a head link's producer may be the last conv of a chain)
    for parent in model.modules():
        for name, child in list(parent._modules.items()):
            if isinstance(child, CodeMaxPool2d):
                parent._modules[name] = child.pool
            elif isinstance(child, CodeReLU):
                parent._modules[name] = child.relu
            elif isinstance(child, CodeAct):
                parent._modules[name] = child.act
    for m in model.modules():
        if _is_conv_q(m):
            m._code_x3 = False   # the mark of link_codes(x3=True): also on a chain's last reader, which has no _code_out
        if _is_conv_q(m) and m._code_out is not None:
            m._code_out = None
            m._code_entry = False
            m._code_lut = None   # link_layerout's table
            m.__dict__.pop("_stem_link", None)   # link_stem's record: its pools and ReLUs are unwrapped above
            if hasattr(m, "_pre_link_post"):
                m._post = m._pre_link_post
                del m._pre_link_post
            n += 1
    return n


# ------------------------------------------------------------------ codes behind the layer-output quantizer: the activation as a table
def _lut_act(m):
    """An elementwise activation module link_layerout can put into a producer's table: the stock ones and the reference's mirrors
    (activation_func.py).  Each is a pure per-element function without state."""
    from . import activation_func as af
    return isinstance(m, (nn.ReLU, nn.GELU, nn.SiLU, nn.Sigmoid, af.Swish, af.Sigmoid, af.STL))


def _layerout_producer(m):
    """Can Conv2d_Q `m` be given a table to write codes through: _code_eligible's producer side, WITH the layer-output quantizer
    (and the BatchNorm it needs) in its epilogue."""
    if not _is_conv_q(m) or m._code_out is not None or getattr(m, "_in_residual", False):
        return False
    return (m.q_bit in (8, 7) and not m.training and isinstance(m.padding, tuple) and (m.bias is None or getattr(m, "_scaled_bias", False))
            and bool(_post_flags(m) & 2) and m._post[0] is not None)


def _layerout_table(a, acts, out, device):
    """The uint8 table of producer `a` for the reader `out` = (Ka, q_bit): per layer-output class (slfp_layerout_lut_values) the
    reader's extended code of act_k(... act_1(relu?(value)) ...), computed by the stock modules themselves on `device`.  relu? is
    the ReLU folded into a's epilogue with the kernels' semantics: fmaxf(NaN, 0) is 0 (torch.relu would keep the NaN)."""
    from .batchnorm import _layerout_code_bytes   # the one builder, shared with the training table (batchnorm.layerout_code_table)
    return _layerout_code_bytes(acts, out[0], out[1], device, "link_layerout", bool(_post_flags(a) & 1))


def link_layerout(model, example_input):
    """link_codes_traced for the blocks [Conv2d_Q, BatchNorm2d, layerout_quantize_func, ReLU | Swish | GELU] of MobileNetV1_swish /
    VGG16_gelu (nets_cifar/mobilenetv1.py:196-231, nets_cifar/vgg16.py:186-293), after fuse_bn_relu.  Opt-in.  A producer `a` whose
    epilogue carries the layer-output quantizer is linked to the one Conv2d_Q `b` that reads its output through nothing but
    nn.Identity, elementwise activation modules (_lut_act) and nn.MaxPool2d modules behind them: after the quantizer a value is one
    of a few thousand, so activation and b's quantize_act(. / Ka) become ONE byte table (`a._code_lut`, built by running the modules
    themselves over every value: bit-identical for any of them) that a's kernel indexes (slfp_conv2d_fwd_codes_lut); the
    activation modules then pass the codes through (CodeAct), the pools pool codes (CodeMaxPool2d), b decodes.  The float32
    activation tensor and the activation pass are gone.  Links are made only where `a` has a table kernel for its shape, never
    for a producer with two consumers, and only where `b` can read codes: as the producer of the next link (its table kernel with
    code input) or, the last layer of a chain, through its code kernel with float32 output -- for a layer-output epilogue without a
    folded ReLU that is the code kernel up to the affine and slfp_quantize_layerout_f32 behind it (the same values step for step;
    the older code entry points keep refusing the layer-output bit, and a ReLU behind the quantizer has no such split).  The
    whole set is verified bit for bit against the unlinked output on `example_input` and rolled back otherwise (returns 0).
    Inference only; unlink_codes undoes it.  Returns the number of links."""
    from .conv2d_func import _supported
    tr = _Trace(model, example_input)
    y0 = tr.output
    order = [c.mod for c in tr.calls if _is_conv_q(c.mod)]
    if len(order) != len(set(order)):
        return 0   # a module that runs twice per forward has no single producer / consumer

    def x_of(m):
        return tr.of(m)[0].x

    cand = {}
    for b in order:
        t, acts, pools, seen = x_of(b), [], [], set()
        if not torch.is_tensor(t) or t.dim() != 4 or t.dtype != torch.float32:
            continue
        for _ in range(8):   # back from b: pools first, then the activations (a pool IN FRONT of an activation does not commute with it)
            fresh = lambda m: m not in seen   # noqa: E731
            act = tr.producer(t, lambda m: fresh(m) and _lut_act(m))
            pool = tr.producer(t, lambda m: fresh(m) and _poolable(m)) if not acts else None
            hit = act if act is not None else pool
            if hit is None or tr.runs(hit.mod) != 1 or not torch.is_tensor(hit.x):
                break
            seen.add(hit.mod)
            (acts if hit is act else pools).append(hit.mod)
            t = hit.x
        a = tr.producer(t, _is_conv_q)
        a = a.mod if a is not None else None
        if a is None or a is b or not _layerout_producer(a) or not _code_eligible_reader(b):
            continue
        if pools and a.out_channels % 4:
            continue   # slfp_maxpool2d_codes needs C % 4 == 0
        cand.setdefault(a, []).append((b, acts[::-1], pools))
    link_of = {a: cand[a][0] for a in order if a in cand and len(cand[a]) == 1}

    def table_kernel(a, a_in):
        return x_of(a).dim() == 4 and _supported(a, x_of(a).shape, "lut", a_in, _reader_quant(link_of[a][0]), _post_flags(a))

    def float_out_on_codes(b):   # b with codes in and float32 out
        fl = _post_flags(b)
        if x_of(b).dim() != 4:
            return False
        if fl & 2:
            return fl == 2 and _supported(b, x_of(b).shape, "codes_lo", True, None, 0)
        return _supported(b, x_of(b).shape, "codes", True, None, fl)

    can_read = {}   # can a conv read codes: with float32 out, or as the producer of a link that will be made (decided back to front)
    for m in reversed(order):
        can_read[m] = float_out_on_codes(m) or (m in link_of and table_kernel(m, True) and can_read.get(link_of[m][0], False))
    made, reads_codes, wrapped = [], set(), []
    for a in order:   # execution order: whether `a` itself reads codes is known when its own link is decided
        if a not in link_of:
            continue
        b, acts, pools = link_of[a]
        out = _reader_quant(b)
        if not table_kernel(a, a in reads_codes) or not can_read[b]:
            continue
        a._code_lut = _layerout_table(a, acts, out, x_of(a).device)
        a._code_out = out
        made.append(a)
        reads_codes.add(b)
        wrapped += _wrap_children(model, pools, b.q_bit, acts=acts)
    if not made:
        return 0
    tr.release()

    def undo():
        for a in made:
            a._code_out, a._code_lut = None, None
        _unwrap_children(wrapped)

    return len(made) if _verified(lambda: model(example_input), y0, undo) else 0


def _code_eligible_reader(m):
    """_code_eligible for the consumer of a link_layerout link: its own epilogue may carry the layer-output quantizer (it is then
    the producer of the next link, or the chain's last layer)."""
    return (_is_conv_q(m) and m.q_bit in (8, 7) and not m.training and isinstance(m.padding, tuple)
            and (m.bias is None or getattr(m, "_scaled_bias", False)))


# ------------------------------------------------------------------ the image stem writes the first code tensor of the net
def _restore_stem(stem):
    _unwrap_children(stem.__dict__.pop("_stem_link"))
    stem._post, stem._code_out = stem._pre_link_post, None
    del stem._pre_link_post


def link_stem(model, example_input):
    """The chain of 1-byte codes starts at the image: the large-kernel image stem (7x7 / 11x11, `stem_mfma_*`: ResNet-50,
    SqueezeNet 1.0, AlexNet) writes the codes of the layer(s) behind it instead of its float32 output -- the largest activation
    of these nets.  One traced forward on `example_input` finds the stem (the first-executed Conv2d_Q with in_channels <= 4 and a
    4-d float32 input) and follows its output to every Conv2d_Q that reads it, through nn.Identity (a folded BatchNorm), nn.ReLU
    modules (in place or not) and nn.MaxPool2d in floor or ceil mode (no return_indices, dilation 1, C % 4 == 0, each run once).
    The link is made only if every reader is such a conv and no other module takes the tensor, all readers share (Ka, q_bit) --
    ONE code tensor serves them, as it serves the two expands of a Fire module (ResNet-50's layer1.0.conv1 and
    layer1.0.downsample.0) --, each reader has a code-input kernel in its present state (linked by link_codes_traced, rewritten by
    fuse_fire, or plain) and the stem has the code-output kernel (slfp_conv2d_codes_supported).  The stem then gets the ReLU
    folded, `_code_out` and `_pre_link_post`, the pools become CodeMaxPool2d, the ReLU modules CodeReLU (no pass over the codes), and
    the model must reproduce its recorded output
    with torch.equal; otherwise (a functional use hooks cannot see, e.g. a torch.cat) everything is rolled back.  An exception is a
    refusal too, but an error status of libslfp_hip itself (_lib.SlfpError) is re-raised after the roll-back, as in fuse_fire.
    Run it after fuse_bn_relu / fuse_named_bn, fuse_fire(entries=True), link_codes_traced(entries=True) and fuse_residual; it
    composes with all of them and with graph.GraphedModule.  Inference only.  Returns 1 or 0; unlink_stem undoes exactly this
    link, unlink_codes undoes it as it undoes every link."""
    from .conv2d_func import _supported
    if model.training or not any(_is_conv_q(m) for m in model.modules()):
        return 0
    tr = _Trace(model, example_input)
    y0 = tr.output
    if not torch.is_tensor(y0):
        return 0
    first = next((i for i, c in enumerate(tr.calls) if _is_conv_q(c.mod)), None)
    if first is None:
        return 0
    stem, x_stem, t0 = tr.calls[first].mod, tr.calls[first].x, tr.calls[first].out
    if not (stem.in_channels <= 4 and torch.is_tensor(x_stem) and x_stem.dim() == 4 and x_stem.dtype == torch.float32):
        return 0   # the first-executed Conv2d_Q is no image stem
    if (tr.runs(stem) != 1 or not _code_eligible(stem, producer_side=True) or not torch.is_tensor(t0) or t0.dim() != 4):
        return 0
    # follow the tensor in execution order: live = [tensor, has a ReLU module run on it or on the way to it]
    live, readers, pools, relus = [[t0, False]], [], [], []

    def note(t, relu):
        for e in live:
            if tr.same(e[0], t):   # nn.Identity, an in-place ReLU: the same tensor again
                e[1] = e[1] or relu
                return
        live.append([t, relu])

    for mod, inp, out in tr.calls[first + 1:]:
        xin = inp[0] if inp else None
        src = next((e for e in live if tr.same(e[0], xin)), None)
        if src is None:
            continue
        if tr.runs(mod) != 1 or not torch.is_tensor(out):
            return 0
        if _is_conv_q(mod):
            readers.append((mod, xin, src[1]))
        elif isinstance(mod, nn.Identity):
            note(out, src[1])
        elif isinstance(mod, nn.ReLU):
            relus.append(mod)
            note(out, True)
        elif (isinstance(mod, nn.MaxPool2d) and not mod.return_indices and _pair2(mod.dilation) == (1, 1)
              and stem.out_channels % 4 == 0):
            pools.append(mod)
            note(out, src[1])
        else:
            return 0   # another module takes the tensor
    if not readers or len({r for _, _, r in readers}) != 1:
        return 0   # one code tensor: with the ReLU folded for every reader, or for none
    if len({_reader_quant(b) for b, _, _ in readers}) != 1:
        return 0
    b0, _, via_relu = readers[0]
    out = _reader_quant(b0)
    flags = _post_flags(stem) | (1 if via_relu else 0)
    for b, xin, _ in readers:
        if (not _code_eligible(b) or xin.dtype != torch.float32 or xin.dim() != 4
                or not _supported(b, tuple(xin.shape), "codes", True, b._code_out, _post_flags(b))):
            return 0
    if not _supported(stem, tuple(x_stem.shape), "codes", False, out, flags):
        return 0
    stem._pre_link_post = stem._post
    _fold_flags(stem, flags)
    stem._code_out = out
    # the pools between the stem and its readers now see codes; the ReLUs (each runs once, on this tensor only) are the quantizer's
    stem.__dict__["_stem_link"] = _wrap_children(model, pools, out[1], relus)
    tr.release()
    return int(_verified(lambda: model(example_input), y0, lambda: _restore_stem(stem), reraise=True))


def unlink_stem(model):
    """Undo link_stem."""
    n = 0
    for m in list(model.modules()):
        if "_stem_link" in m.__dict__:
            _restore_stem(m)
            n += 1
    return n


# ------------------------------------------------------------------ the image stem reads uint8 pixels
def _mark_image_stem(stem, table):
    """Give Conv2d_Q `stem` the pixel table (float32 [C_in][256], moved to the weights' device): from now on a uint8 input is pixels."""
    from . import image_u8
    table = image_u8.check_table(table)
    if stem.groups != 1 or stem.in_channels != table.shape[0]:
        raise ValueError(f"link_image_u8: the stem reads {stem.in_channels} channels in {stem.groups} group(s), the table has {table.shape[0]}")
    stem._image_table = table.to(stem.weight.device)   # a registered, non-persistent buffer: the state dict keeps its keys


def _restore_image_stem(stem):
    stem._image_table = None
    stem.__dict__["_last_pixels"] = None


def link_image_u8(model, table, example_input):
    """The net reads uint8 pixels: `table` (image_u8.pixel_table: float32 [C][256], ToTensor + Normalize or any per-channel elementwise
    preprocessing as data) and `example_input`, a uint8 batch of logical shape (N, C, H, W) in channels_last on the model's device.  One
    traced forward on the expanded batch (image_u8.expand) finds the Conv2d_Q that reads the model input; it must run once, have
    groups == 1 and C_in == C.  It gets the table as the non-persistent buffer `_image_table`, which gives uint8 input the meaning
    "pixels" at this one module: in inference, where the library has a byte form of the stem's kernel (slfp_conv2d_u8_supported), one
    slfp_conv2d_fwd_u8 launch reads the bytes -- float32 out or, linked by link_stem / link_codes[_traced], codes out --; in training,
    under autograd, or for a stem without that form the bytes are expanded on the device and the ordinary path runs
    (`_last_kernel`: "u8-expand+..."), so gradients and `input_q` are exactly the float32 path's.  float32 input keeps working as before;
    NCHW-contiguous bytes, CPU bytes or another channel count raise TypeError.  The model must then reproduce, with torch.equal, its
    output on the expanded batch; otherwise the mark is rolled back with a warning.  Run it after the other passes (their example
    input is float32) or before them; it composes with all of them and is undone by unlink_image_u8.  Returns 1 or 0."""
    from . import image_u8
    table = image_u8.check_table(table)
    if not (torch.is_tensor(example_input) and example_input.dtype == torch.uint8 and example_input.dim() == 4):
        raise TypeError("link_image_u8: example_input must be a 4-d torch.uint8 pixel batch")
    if example_input.shape[1] != table.shape[0] or not any(_is_conv_q(m) for m in model.modules()):
        return 0
    if example_input.is_cuda:
        x32 = image_u8.expand(example_input, table.to(example_input.device))
    else:   # no kernel runs on the CPU: only a q_bit 32 model traces there, and the verification below then refuses the link
        x32 = table[torch.arange(table.shape[0]).view(1, -1, 1, 1), example_input.long()].contiguous(memory_format=torch.channels_last)
    tr = _Trace(model, x32)
    y0 = tr.output
    readers = [c for c in tr.readers(x32) if _is_conv_q(c.mod)]
    others = [c for c in tr.readers(x32) if not _is_conv_q(c.mod) and not isinstance(c.mod, nn.Identity)]
    if not torch.is_tensor(y0) or len(readers) != 1 or others or tr.runs(readers[0].mod) != 1:
        return 0   # no single Conv2d_Q takes the image
    stem = readers[0].mod
    if stem.groups != 1 or stem.in_channels != table.shape[0] or stem._image_table is not None:
        return 0
    tr.release()
    _mark_image_stem(stem, table)
    return int(_verified(lambda: model(example_input), y0, lambda: _restore_image_stem(stem), reraise=True,
                         warn="link_image_u8: the model does not take the uint8 batch ({}); rolled back"))


def unlink_image_u8(model):
    """Undo link_image_u8: the stems read float32 only (and uint8 as codes) again.  Returns the number of stems unmarked."""
    n = 0
    for m in model.modules():
        if _is_conv_q(m) and m._image_table is not None:
            _restore_image_stem(m)
            n += 1
    return n


# ------------------------------------------------------------------ residual add + ReLU in the last 1x1 conv's epilogue
_BOTTLENECK_CHILDREN = ("conv1", "bn1", "conv2", "bn2", "conv3", "relu")


def _bottleneck_forward(self, x):
    """The dataflow of the torchvision Bottleneck the reference copies (nets_imgnet/resnet50.py:76-100) with the tail
    relu(bn3(conv3(h)) + identity) handed to conv3 as its residual operand (bn3 is folded already)."""
    out = self.relu(self.bn1(self.conv1(x)))
    out = self.relu(self.bn2(self.conv2(out)))
    identity = x if getattr(self, "downsample", None) is None else self.downsample(x)
    return self.conv3(out, residual=identity)


def _residual_candidate(blk):
    if isinstance(blk, nn.Sequential) or "forward" in blk.__dict__:
        return False
    ch = blk._modules
    if any(ch.get(k) is None for k in _BOTTLENECK_CHILDREN) or "downsample" not in ch and not hasattr(blk, "downsample"):
        return False
    conv3, bn3 = ch["conv3"], ch.get("bn3")
    if not (_is_pw(conv3) and tuple(_pair2(conv3.padding)) == (0, 0) and conv3._code_out is None and isinstance(ch["relu"], nn.ReLU)):
        return False
    if bn3 is not None and not isinstance(bn3, nn.Identity):
        return False   # fold it first (fuse_named_bn): the add follows the BatchNorm
    if conv3._post is not None and (int(conv3._post[2]) & 3):
        return False   # a ReLU / layer-output quantizer in front of the add is another block
    return all(_is_conv_q(ch[k]) for k in ("conv1", "conv2"))


def _pair2(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _restore_block(blk):
    del blk.__dict__["forward"]
    del blk.__dict__["_residual_fused"]
    blk.conv3.residual_relu = False
    del blk.conv3._in_residual
    if "_trunk_link" in blk.conv3.__dict__:   # link_trunk: no trunk consumer outlives the residual route
        _restore_trunk(blk.conv3)


def fuse_residual(model, example_input):
    """After fuse_named_bn: every block that follows the torchvision Bottleneck naming (conv1 / bn1 / conv2 / bn2 / conv3 / bn3 /
    relu / downsample children of a non-Sequential module; conv3 a 1x1 stride-1 Conv2d_Q whose BatchNorm is folded or absent)
    gets an instance-level forward with the same dataflow that ends in conv3(h, residual=identity) with the ReLU folded:
    out = relu(bn3(conv3(h)) + identity) becomes ONE launch (slfp_conv2d_fwd_res) instead of three, 8 B per trunk element
    through HBM instead of 24.  A name is only a convention, so -- the rule link_codes_traced set -- one traced forward on
    `example_input` records every candidate's input and output, each rewritten block must reproduce its recorded output
    bit for bit on its recorded input (otherwise it is restored and not counted), and the rewritten model must reproduce
    the logits bit for bit (otherwise everything is restored and 0 is returned).  Composes with fuse_named_bn,
    link_codes_traced / unlink_codes in either order, and graph.GraphedModule.  Inference only (with grad enabled conv3
    computes the same values with ATen).  Returns the number of blocks rewritten; unfuse_residual undoes it."""
    import types
    cands = [m for m in model.modules() if _residual_candidate(m)]
    if not cands:
        return 0
    tr = _Trace(model, example_input, blocks=cands)
    y0 = tr.output
    done = []
    for blk in cands:
        io = tr.io(blk)
        if io is None:
            continue   # not run, run twice, or not a tensor -> tensor block
        x, want = io
        blk.conv3.residual_relu = True
        blk.conv3._in_residual = True
        blk.__dict__["_residual_fused"] = True
        blk.__dict__["forward"] = types.MethodType(_bottleneck_forward, blk)
        if _verified(lambda: blk(x), want, lambda: _restore_block(blk)):
            done.append(blk)
    tr.release()
    if not done:
        return 0

    def undo():
        for blk in done:
            _restore_block(blk)

    return len(done) if _verified(lambda: model(example_input), y0, undo) else 0


def unfuse_residual(model):
    """Undo fuse_residual."""
    n = 0
    for blk in model.modules():
        if blk.__dict__.get("_residual_fused"):
            _restore_block(blk)
            n += 1
    return n


# ------------------------------------------------------------------ the residual epilogue writes the next block's codes too
def _restore_trunk(conv3):
    conv3.__dict__.pop("_trunk_link", None)
    conv3._trunk_code_out = None


def link_trunk(model, example_input):
    """The trunk of a residual net leaves each block as float32 AND as the next block's 1-byte codes: conv3 of a block rewritten by
    fuse_residual, which reads conv2's codes (link_codes_traced), applies the quantizer of the Conv2d_Q layers that read its result
    -- the next block's conv1, and downsample.0 at a stage boundary -- to the value it holds after the add and the ReLU and
    stores the byte next to the float32 value (slfp_conv2d_fwd_res_codes).  Those readers then take the codes (conv1 keeps
    `_code_entry` and simply receives uint8) and never read the float32 tensor; the next block's residual add, an avgpool or anything
    else still gets the plain float32 tensor, which carries the codes as an attribute (Conv2d_Q.forward).  One traced forward on
    `example_input` finds, for every residual-fused block, the Conv2d_Q layers whose input IS its output.  A link is made only if
    all of them share (float(Ka), q_bit) -- one code tensor serves them --, each has a code-input kernel in its present state, and
    slfp_conv2d_res_codes_supported says yes for conv3.  Each linked block must reproduce its recorded output with torch.equal, hand
    on exactly slfp_encode_f32 of it, and the block that reads it must reproduce its own recorded output from it; then the model
    must reproduce its logits with torch.equal.  A link that fails is taken back alone, a model that fails takes all of them back;
    an error status of libslfp_hip itself (_lib.SlfpError) is re-raised after the roll-back, as in link_stem.  Run it after
    fuse_named_bn, fuse_residual and link_codes_traced(entries=True) (with none of them there is nothing to link: 0); composes with
    link_stem and graph.GraphedModule.  Inference only, never a default.  Returns the number of links; unlink_trunk undoes exactly
    these, unlink_codes and unfuse_residual take them along."""
    from .conv2d_func import _supported, _f32, _act_fmt
    from .sfp_quant import hip_encode
    from . import _lib
    blocks = [m for m in model.modules() if m.__dict__.get("_residual_fused")]
    if model.training or not blocks:
        return 0
    tr = _Trace(model, example_input, blocks=blocks)
    y0 = tr.output
    if not torch.is_tensor(y0):
        return 0
    nhwc = torch.channels_last
    made = []

    def take_back(conv3):
        _restore_trunk(conv3)
        made.remove(conv3)

    def take_all_back():
        while made:
            take_back(made[-1])

    for blk in blocks:
        io = tr.io(blk)
        c3 = blk._modules.get("conv3")
        if io is None or not _is_conv_q(c3) or c3._trunk_code_out is not None or tr.runs(c3) != 1:
            continue
        x_blk, want = io
        if want.dim() != 4 or want.dtype != torch.float32 or not want.is_contiguous(memory_format=nhwc):
            continue
        readers = [c.mod for c in tr.readers(want) if _is_conv_q(c.mod)]
        if not readers or any(tr.runs(b) != 1 or b is c3 for b in readers):
            continue
        scales = {_reader_quant(b) for b in readers}
        if len(scales) != 1:
            continue   # one code tensor serves every reader
        out = next(iter(scales))
        if not all(_code_eligible(b) and _supported(b, tuple(want.shape), "codes", True, b._code_out, _post_flags(b)) for b in readers):
            continue   # a reader without a code-input kernel in its present state
        x3 = tr.of(c3)[0].x
        if (not _code_eligible(c3) or c3._code_out is not None or _post_flags(c3) != 0 or not torch.is_tensor(x3)
                or x3.dtype != torch.uint8 or x3.dim() != 4
                or not _supported(c3, tuple(x3.shape), "res_codes", True, out, 1 if c3.residual_relu else 0)):
            continue
        c3._trunk_code_out = out
        c3.__dict__["_trunk_link"] = True
        made.append(c3)
        nxt = next((b for b in blocks if b is not blk and tr.io(b) is not None and tr.same(tr.io(b)[0], want)), None)

        def relinked():
            """the block's output, or None unless it hands on exactly slfp_encode_f32 of its recorded output and the block that reads
            it reproduces its own recorded output from it"""
            got = blk(x_blk)
            tc = got.__dict__.get("_trunk_codes") if torch.is_tensor(got) else None
            if tc is None or tc[1:] != out or not torch.equal(tc[0], hip_encode(want, _f32(out[0]), _act_fmt(out[1]))):
                return None
            return got if nxt is None or torch.equal(nxt(got), tr.io(nxt)[1]) else None

        try:
            _verified(relinked, want, lambda: take_back(c3), reraise=True)   # a link that fails is taken back alone
        except _lib.SlfpError:
            take_all_back()   # a defect takes back every link
            raise
    tr.release()
    if not made:
        return 0
    return len(made) if _verified(lambda: model(example_input), y0, take_all_back, reraise=True) else 0


def unlink_trunk(model):
    """Undo link_trunk."""
    n = 0
    for m in model.modules():
        if "_trunk_link" in m.__dict__:
            _restore_trunk(m)
            n += 1
    return n


# ------------------------------------------------------------------ SqueezeNet's Fire module on 1-byte codes, without the concat
_FIRE_CHILDREN = ("squeeze", "squeeze_activation", "expand1x1", "expand1x1_activation", "expand3x3", "expand3x3_activation")


def _fire_forward(self, x):
    """The dataflow of the Fire module (nets_imgnet/squeezenet1_0.py:41-46) on codes: the three ReLUs sit in the conv epilogues,
    `squeeze` writes ONE code tensor that both expands read, and the expands write the next layer's codes into the two channel
    halves of one buffer -- what torch.cat([relu(e1), relu(e3)], 1) followed by the consumer's quantizer would hold."""
    from .conv2d_func import _f32, _act_fmt
    from .sfp_quant import hip_encode
    if self.training:
        raise RuntimeError("fuse_fire: a rewritten Fire module is inference-only; call fusion.unfuse_fire(model) to train")
    sq, e1, e3 = self.squeeze, self.expand1x1, self.expand3x3
    with torch.no_grad():
        if x.dtype != torch.uint8:   # head of the chain (the pooled float32 stem output)
            if not x.is_contiguous(memory_format=torch.channels_last):
                x = x.contiguous(memory_format=torch.channels_last)
            if not sq._code_entry:   # one slfp_encode_f32 pass; with _code_entry `squeeze` reads the float32 tensor itself
                x = hip_encode(x, _f32(sq.Ka), _act_fmt(sq.q_bit))
        h = sq(x)
        buf = torch.empty((h.shape[0], e1.out_channels + e3.out_channels, h.shape[2], h.shape[3]), dtype=torch.uint8,
                          device=h.device, memory_format=torch.channels_last)
        e1.forward_slice(h, (buf, 0))
        e3.forward_slice(h, (buf, e1.out_channels))
    return buf


def _fire_candidate(blk):
    if isinstance(blk, nn.Sequential) or "forward" in blk.__dict__ or blk.training:
        return False
    ch = blk._modules
    if any(ch.get(k) is None for k in _FIRE_CHILDREN):
        return False
    sq, e1, e3 = ch["squeeze"], ch["expand1x1"], ch["expand3x3"]
    if not all(isinstance(ch[k + "_activation"], nn.ReLU) for k in ("squeeze", "expand1x1", "expand3x3")):
        return False
    # every leg will write codes; stricter than the shared predicate: no epilogue at all yet (the rewrite puts the ReLU there), dense
    if not all(_code_eligible(c, producer_side=True) and _post_flags(c) == 0 and c.groups == 1 for c in (sq, e1, e3)):
        return False
    same_size = all(tuple(c.stride) == (1, 1) and tuple(_pair2(c.dilation)) == (1, 1)
                    and tuple(k - 1 for k in c.kernel_size) == tuple(2 * p for p in c.padding) for c in (sq, e1, e3))
    return (same_size and e1.in_channels == e3.in_channels == sq.out_channels and e1.out_channels % 16 == 0
            and e3.out_channels % 16 == 0 and float(e1.Ka) == float(e3.Ka) and e1.q_bit == e3.q_bit)   # ONE code tensor serves both


def _restore_fire(blk):
    st = blk.__dict__.pop("_fire_fused")
    del blk.__dict__["forward"]
    for conv, post in st["posts"]:
        conv._post, conv._code_out, conv._code_entry = post, None, False
    _unwrap_children(st["pools"])


def fuse_fire(model, example_input, entries=False):
    """SqueezeNet's Fire modules (nets_imgnet/squeezenet1_0.py:20-46; any non-Sequential block with the six children squeeze /
    squeeze_activation / expand1x1 / expand1x1_activation / expand3x3 / expand3x3_activation, Conv2d_Q and nn.ReLU) on 1-byte
    codes: the block gets an instance-level forward in which the three ReLUs are folded into the conv epilogues, `squeeze` writes
    ONE code tensor for both expands (they must share Ka and q_bit) and both expands write the NEXT consumer's codes into the two
    channel halves of one buffer (Conv2d_Q.forward_slice, slfp_conv2d_fwd_codes_slice): no in-place ReLU passes, no
    torch.cat, 1 B per element where the float32 path moves 24.  The next consumer is found from one traced forward on
    `example_input`: the single Conv2d_Q that reads the block's output, looking through nn.MaxPool2d (floor or ceil mode; wrapped
    in CodeMaxPool2d), nn.Dropout in eval mode and nn.Identity.  A block without such a consumer, or with a leg libslfp_hip has
    no kernel for, is left exactly as it was.  The first block of a chain encodes its float32 input in one pass.  As in
    link_codes_traced / fuse_residual the rewrite verifies itself: every rewritten block must reproduce, code for code,
    slfp_encode_f32 of its recorded output on its recorded input, and the model must reproduce its logits bit for bit -- blocks
    that do not are restored one by one.  An exception while verifying is a refusal too, with a warning that names it -- except an
    error status from libslfp_hip itself (_lib.SlfpError), which restores the blocks and is re-raised: a kernel that fails where the
    support queries said yes must not pass as a skipped block.  Inference only; composes with graph.GraphedModule.  Returns the number of blocks
    rewritten; unfuse_fire undoes it.
    entries=True: a rewritten block whose input arrives as float32 hands it straight to `squeeze` where libslfp_hip has the
    float32 -> codes form of that layer (slfp_conv2d_entry_supported; `squeeze._code_entry`): no slfp_encode_f32 pass at the head of
    the chain.  The verification is the same."""
    import types
    from .conv2d_func import _supported, _f32, _act_fmt
    from .sfp_quant import hip_encode
    from . import _lib
    cands = [m for m in model.modules() if _fire_candidate(m)]
    if not cands or model.training:
        return 0
    tr = _Trace(model, example_input, blocks=cands)
    y0 = tr.output
    conv_in = [c for c in tr.calls if _is_conv_q(c.mod)]
    thru = [c for c in tr.calls if isinstance(c.mod, (nn.MaxPool2d, nn.Dropout, nn.Identity))]

    def consumer_of(t):
        """(the single Conv2d_Q that reads `t`, the pools on the way) or None."""
        found = []
        for c in conv_in:
            cur, pools, ok = c.x, [], False
            for _ in range(6):
                if tr.same(cur, t):
                    ok = True
                    break
                src = [s for s in thru if tr.same(s.out, cur)]
                if len(src) != 1:
                    break
                cur = src[0].x
                if isinstance(src[0].mod, nn.MaxPool2d):
                    pools.append(src[0].mod)
            if ok:
                found.append((c.mod, pools))
        # any other module that takes `t` (or a pooled / passed-through copy) without ending in that conv is a second use
        # (a module that hands its input through -- nn.Dropout in eval mode, nn.Identity -- is not a use of its own)
        direct = sum(1 for s in thru if tr.same(s.x, t) and not tr.same(s.out, t)) + sum(1 for c in conv_in if tr.same(c.x, t))
        if len(found) != 1 or direct != 1:
            return None
        return found[0]

    done = []
    for blk in cands:
        io = tr.io(blk)
        if io is None:
            continue   # not run, run twice, or not a tensor -> tensor block
        x, want = io
        sq, e1, e3 = blk.squeeze, blk.expand1x1, blk.expand3x3
        ld = e1.out_channels + e3.out_channels
        if (x.dim() != 4 or want.dim() != 4 or want.shape[1] != ld or not x.is_cuda
                or not want.is_contiguous(memory_format=torch.channels_last)):
            continue
        cons = consumer_of(want)
        if cons is None:
            continue
        nxt, pools = cons
        # the reader: of _code_eligible only the conditions on the quantizer, the mode and the bias are asked here; a layer-output
        # epilogue is the support query's to refuse, below
        if (nxt.q_bit not in (8, 7) or nxt.training or (nxt.bias is not None and not getattr(nxt, "_scaled_bias", False))
                or any(p.return_indices or _pair2(p.dilation) != (1, 1) or ld % 4 for p in pools)):
            continue
        out_e, out_n = _reader_quant(e1), _reader_quant(nxt)
        hshape = (x.shape[0], sq.out_channels, x.shape[2], x.shape[3])
        nshape = (x.shape[0], nxt.in_channels) + tuple(tr.of(nxt)[0].x.shape[2:])
        if not (_supported(sq, tuple(x.shape), "codes", True, out_e, 1) and _supported(e1, hshape, "slice", True, out_n, 1, ld)
                and _supported(e3, hshape, "slice", True, out_n, 1, ld)
                and _supported(nxt, nshape, "codes", True, None, _post_flags(nxt))):
            continue
        st = {"posts": [(c, c._post) for c in (sq, e1, e3)], "pools": []}
        for c in (sq, e1, e3):
            _fold_flags(c, 1)
        sq._code_out, e1._code_out, e3._code_out = out_e, out_n, out_n
        sq._code_entry = bool(entries and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
                              and _supported(sq, tuple(x.shape), "entry", False, out_e, 1))
        blk.__dict__["_fire_fused"] = st
        blk.__dict__["forward"] = types.MethodType(_fire_forward, blk)
        # e.g. a block whose own forward() does more than the six children say
        if not _verified(lambda: blk(x), lambda: hip_encode(want, _f32(out_n[0]), _act_fmt(out_n[1])), lambda: _restore_fire(blk),
                         reraise=True, warn=f"fuse_fire: {type(blk).__name__} left as it was: its rewritten form raised {{}}"):
            continue
        st["pools"] = _wrap_children(model, pools, nxt.q_bit)   # the pools between the block and its consumer now see codes
        done.append(blk)
    tr.release()
    del conv_in[:], thru[:]
    try:   # restored one by one, last block first, until the logits are the recorded ones again
        while done and not _verified(lambda: model(example_input), y0, lambda: _restore_fire(done.pop()), reraise=True,
                                     warn="fuse_fire: the rewritten model raised {}; restoring the last rewritten block"):
            pass   # e.g. a functional op behind a block that cannot take its codes
    except _lib.SlfpError:
        while done:   # a defect restores every block
            _restore_fire(done.pop())
        raise
    return len(done)


def unfuse_fire(model):
    """Undo fuse_fire."""
    n = 0
    for blk in list(model.modules()):
        if "_fire_fused" in blk.__dict__:
            _restore_fire(blk)
            n += 1
    return n


# ------------------------------------------------------------------ the classifier head on 1-byte codes
class CodePass(nn.Module):
    """A module that is the identity on the tensor link_head follows (an nn.AdaptiveAvgPool2d whose output size equals its input
    size) inside a linked head: uint8 codes pass through without a launch; anything else goes to the original module, which this
    wrapper keeps (`mod`; it has no parameters, the state dict does not change)."""

    def __init__(self, mod):
        super().__init__()
        self.mod = mod

    def forward(self, x):
        return x if x.dtype == torch.uint8 else self.mod(x)


def _is_linear_q(m):
    return isinstance(m, nn.Linear) and hasattr(m, "q_bit") and hasattr(m, "Ka") and hasattr(m, "_code_in")


def _head_eligible(m):
    """Can Linear_Q `m` take part in a head link: 8 / 7 bit, eval mode, a bias (the reference dereferences it)."""
    return _is_linear_q(m) and m.q_bit in (8, 7) and not m.training and m.bias is not None


def _eval_dropout(m):
    return isinstance(m, (nn.Dropout, nn.Dropout2d)) and not m.training


def _restore_head(a):
    """Take back the link whose producer is `a` (a Linear_Q or a Conv2d_Q): every slot and attribute link_head wrote for it."""
    rec = a.__dict__.pop("_head_link")
    for parent, name, orig in rec["slots"]:
        now = parent._modules.get(name)
        if (isinstance(now, CodeMaxPool2d) and now.pool is orig or isinstance(now, CodeReLU) and now.relu is orig
                or isinstance(now, CodePass) and now.mod is orig):
            parent._modules[name] = orig
    a._code_out = None
    if _is_conv_q(a):
        a._post = rec["post"]
    else:
        a._code_relu = False
    rec["reader"]._code_in = False


def _wrap_head(model, pools, relus, passes, q_bit):
    """_wrap_children plus CodePass for `passes`; the records _restore_head takes."""
    recs = _wrap_children(model, pools, q_bit, relus)
    for parent in [m for m in model.modules() if not isinstance(m, (CodeMaxPool2d, CodeReLU, CodeAct, CodePass))]:
        for name, child in list(parent._modules.items()):
            if any(child is pm for pm in passes):
                parent._modules[name] = CodePass(child)
                recs.append((parent, name, child))
    return recs


def link_head(model, example_input):
    """The classifier head on 1-byte codes: after fuse_bn_relu / link_codes, the Linear_Q layers at the end of AlexNet / VGG16_Q
    (utils/conv2d_func.py:50-66) hand their activations on as codes and run the weight-streaming kernel (slfp_linear_fwd_fc).
    One traced forward on `example_input` finds two kinds of link:
      (a) Linear_Q -> Linear_Q with only nn.ReLU, nn.Dropout in eval mode or nn.Identity modules between them (each run once, no
          other module reading the tensor): the producer folds the ReLU (`_code_relu`) and writes the reader's codes (`_code_out`),
          the ReLU slots become CodeReLU, the reader is marked (`_code_in`);
      (b) Conv2d_Q -> the first Linear_Q, where the Linear's recorded input equals, value for value, t.flatten(1) of a recorded 4-d
          tensor t that comes from a code-eligible Conv2d_Q through only its fused ReLU, nn.ReLU modules, floor-mode nn.MaxPool2d
          (-> CodeMaxPool2d), eval Dropout, nn.Identity and an nn.AdaptiveAvgPool2d whose output size equals its input size (-> CodePass);
          nn.Flatten / reshape / flatten between t and the Linear work on the code tensor as they stand.  The conv gets the
          Linear's (Ka, q_bit) as `_code_out`, with the ReLU folded.
    Links are made only where slfp_linear_fc_supported has the reader's (and, for (a), the producer's) kernel.  Each link is verified
    on its own -- the reader's output on the recorded input must be torch.equal to the recorded one -- and a link that fails is
    taken back alone; then the whole model must reproduce its recorded output, or every link is taken back.  Any exception (a
    functional `view` that cannot take a channels_last code tensor, arithmetic on the flattened tensor) is a refusal with a
    warning.  Inference only.  Returns the number of links; unlink_head undoes them (unlink_codes takes them along)."""
    from .conv2d_func import _supported, _conv_io, _scalar_scale, options
    from .sfp_quant import hip_maxpool_codes
    from . import _lib
    if (model.training or not torch.is_tensor(example_input) or not example_input.is_cuda
            or not any(_head_eligible(m) for m in model.modules())):
        return 0
    # (a Linear_Q owns its quantizer children, so it is no leaf: it is recorded as a block)
    tr = _Trace(model, example_input, blocks=[m for m in model.modules() if _is_linear_q(m)])
    y0 = tr.output
    if not torch.is_tensor(y0):
        return 0
    index = {id(c): i for i, c in enumerate(tr.calls)}

    def lin_quant(b):
        return float(_scalar_scale(b.Ka, "Ka")), int(b.q_bit)

    def fc_ok(m, x, x_codes, out, relu):
        rows = x.numel() // x.shape[-1]
        io = _conv_io(x_codes, out)
        return bool(_lib.load().slfp_linear_fc_supported(rows, m.in_features, m.out_features, m.q_bit, options.mfma_passes,
                                                         ctypes.byref(io), 1, 1 if relu else 0))

    lins = [c for c in tr.calls if _is_linear_q(c.mod)]
    plans = []   # (producer, reader, pools, relus, passes, via_relu, x of the producer, x / out of the reader), execution order
    linked_readers = set()
    for cb in lins:
        b = cb.mod
        if (not _head_eligible(b) or tr.runs(b) != 1 or b._code_in or not torch.is_tensor(cb.x) or cb.x.dtype != torch.float32
                or not torch.is_tensor(cb.out)):
            continue
        # walk back from the reader's input through modules that hand the tensor on
        t, via_relu, pools, relus, passes, seen, flat = cb.x, False, [], [], [], {b}, cb.x.dim() == 2
        a, on_the_way = None, []   # every tensor between the producer and the reader
        for _ in range(16):
            on_the_way.append(t)
            made = [c for c in tr._made.get(tr._key(t), []) if c.mod not in seen and index[id(c)] < index[id(cb)]]
            step = next((c for c in reversed(made) if tr.runs(c.mod) == 1 and len(c.inp) == 1 and torch.is_tensor(c.x) and (
                isinstance(c.mod, (nn.ReLU, nn.Identity, nn.Flatten)) or _eval_dropout(c.mod) or
                (t.dim() == 4 and (_poolable(c.mod) or isinstance(c.mod, nn.AdaptiveAvgPool2d) and c.x.shape == c.out.shape)))), None)
            if step is not None:
                seen.add(step.mod)
                if isinstance(step.mod, nn.ReLU):
                    via_relu = True
                    relus.append(step.mod)
                elif isinstance(step.mod, nn.MaxPool2d):
                    pools.append(step.mod)
                elif isinstance(step.mod, nn.AdaptiveAvgPool2d):
                    passes.append(step.mod)
                t = step.x
                continue
            prod = next((c for c in made if _is_linear_q(c.mod) or _is_conv_q(c.mod)), None)
            if prod is not None:
                a = prod
                break
            if t.dim() == 2 and flat:
                # a functional flatten / view / reshape: the latest recorded 4-d tensor with these values
                flat = False
                src = next((c.out for c in reversed(tr.calls[:index[id(cb)]]) if torch.is_tensor(c.out) and c.out.dim() == 4
                            and c.out.dtype == t.dtype and c.out.shape[0] == t.shape[0] and c.out.numel() == t.numel()
                            and torch.equal(c.out.flatten(1), t)), None)
                if src is not None:
                    t = src
                    continue
            break
        if a is None or tr.runs(a.mod) != 1:
            continue
        am = a.mod
        # nothing else may read the tensors on the way: every recorded reader of them is part of the chain
        chain = seen | {am}
        if any(c.mod not in chain for tt in on_the_way + [a.out] for c in tr.readers(tt)):
            continue
        out = lin_quant(b)
        if _is_linear_q(am):
            if (pools or passes or not _head_eligible(am) or am._code_out is not None or a.out.dim() != cb.x.dim()
                    or not torch.is_tensor(a.x)):
                continue
            a_in = am in linked_readers or a.x.dtype == torch.uint8
            if not fc_ok(am, a.x, a_in, out, via_relu) or not fc_ok(b, cb.x, True, None, False):
                continue
        else:
            if (not _code_eligible(am, producer_side=True) or a.out.dim() != 4 or not torch.is_tensor(a.x) or a.x.dim() != 4
                    or (pools and am.out_channels % 4) or not fc_ok(b, cb.x, True, None, False)):
                continue
            flags = _post_flags(am) | (1 if via_relu else 0)
            a_in = a.x.dtype == torch.uint8
            if a_in and not _supported(am, tuple(a.x.shape), "codes", True, out, flags):
                continue   # (a float32 reader without the kernel enters the chain through one slfp_encode_f32 pass, as in link_codes)
        plans.append((am, b, pools[::-1], relus, passes, via_relu, a.x, cb.x, cb.out))
        linked_readers.add(b)
    tr.release()
    if not plans:
        return 0

    made = []

    def take_all_back():
        for am in made:
            _restore_head(am)

    for am, b, pools, relus, passes, via_relu, x_a, x_b, want in plans:
        rec = {"reader": b, "post": am._post if _is_conv_q(am) else None, "slots": _wrap_head(model, pools, relus, passes, b.q_bit)}
        am.__dict__["_head_link"] = rec
        if _is_conv_q(am):
            _fold_flags(am, _post_flags(am) | (1 if via_relu else 0))
        else:
            am._code_relu = via_relu
        am._code_out = lin_quant(b)
        b._code_in = True

        def relinked(am=am, b=b, pools=pools, x_a=x_a, x_b=x_b):
            t = am(x_a)
            for p in pools:
                t = hip_maxpool_codes(t, p.kernel_size, p.stride, p.padding, b.q_bit)
            return b(t.reshape(x_b.shape))

        # b is not a producer yet (execution order): its output is the recorded float32 one
        try:
            ok = _verified(relinked, want, lambda am=am: _restore_head(am), reraise=True)
        except _lib.SlfpError:
            take_all_back()   # the links made so far have not seen the whole-model check: none of them stays
            raise
        if ok:
            made.append(am)
        else:
            warnings.warn("link_head: a link did not reproduce its reader's output and was taken back", stacklevel=2)
    if not made:
        return 0
    if not _verified(lambda: model(example_input), y0, take_all_back, reraise=True):
        # e.g. arithmetic on the flattened tensor, or a functional view that cannot take a channels_last code tensor
        warnings.warn("link_head: the linked model did not reproduce its output on the example input (a functional op between the "
                      "linked layers?); every link was taken back", stacklevel=2)
        return 0
    return len(made)


def unlink_head(model):
    """Undo link_head: every slot and attribute it wrote."""
    n = 0
    for m in list(model.modules()):
        if "_head_link" in m.__dict__:
            _restore_head(m)
            n += 1
    return n


# ------------------------------------------------------------------ the global average pool in front of the classifier
class FoldedReLU(nn.Module):
    """The slot of an nn.ReLU that the wrapper next to it applies: the identity, in the style of CodeReLU.  The original is kept
    (`relu`); it has no parameters, the state dict does not change.  `owner` names the pass that put it there, whose undo function
    alone takes it back: "avgpool" (use_device_avgpool: the GlobalAvgPool2d behind it applies the ReLU), "bn_train"
    (use_device_bn_train: the TrainBatchNorm2d in front of it), "codes_train" (link_codes_train: the TrainBatchNormCodes2d in front)."""

    def __init__(self, relu, owner):
        super().__init__()
        if owner not in ("avgpool", "bn_train", "codes_train"):
            raise ValueError(f"FoldedReLU: owner must be 'avgpool', 'bn_train' or 'codes_train', got {owner!r}")
        self.relu = relu
        self.owner = owner

    def forward(self, x):
        return x


def _avgpool_candidate(m):
    """Is `m` a pooling module that can be a global average pool: nn.AdaptiveAvgPool2d to 1 x 1, or a floor-mode nn.AvgPool2d without
    padding or divisor override (whether its window is the whole map depends on the input: _avgpool_global)."""
    if isinstance(m, nn.AdaptiveAvgPool2d):
        return m.output_size in (1, (1, 1), [1, 1])
    return (isinstance(m, nn.AvgPool2d) and not m.ceil_mode and m.divisor_override is None
            and _pair2(m.padding) == (0, 0))


def _avgpool_global(m, x):
    """Does candidate `m` reduce the 4-d tensor `x` to one window per channel?"""
    if not torch.is_tensor(x) or x.dim() != 4 or x.shape[2] < 1 or x.shape[3] < 1:
        return False
    return isinstance(m, nn.AdaptiveAvgPool2d) or _pair2(m.kernel_size) == (x.shape[2], x.shape[3])


def _avgpool_bound_ok(got, want, x):
    """|got - want| <= 2 (HW + 1) 2^-24 mean64(|x|) per element: two float32 summations of HW terms plus one division each differ by
    at most that, whatever their orders.  `x` is the pooled tensor (after the ReLU, if one is folded)."""
    if not (torch.is_tensor(got) and got.dtype == want.dtype and got.shape == want.shape):
        return False
    hw = x.shape[2] * x.shape[3]
    bound = 2.0 * (hw + 1) * 2.0 ** -24 * x.double().abs().mean(dim=(2, 3), keepdim=True)
    return bool(((got.double() - want.double()).abs() <= bound).all())


class GlobalAvgPool2d(nn.Module):
    """A global average pool (nn.AdaptiveAvgPool2d to 1 x 1, or an nn.AvgPool2d whose window is the whole map) on libslfp_hip's
    kernel (slfp_global_avgpool_f32): float32 sums in one fixed order, so a row of the result does not depend on the batch it
    is computed in.  In eval mode under no_grad, on a ROCm float32 tensor the library takes (channels_last with C a multiple of 4,
    or contiguous NCHW) the kernel runs; anything else -- CPU, grad enabled, training, another window -- goes to the original
    module, which this wrapper keeps (`mod`; it has no parameters, the state dict does not change).
      _relu       use_device_avgpool folded the nn.ReLU in front: the mean of max(x, 0), on either path
      _code_out   (Ka, q_bit) of the Linear_Q that reads the result (link_pool_head): uint8 codes instead of float32
      _last_kernel   "global_avgpool[+relu][+codes_out]", or "aten" """

    def __init__(self, mod):
        super().__init__()
        self.mod = mod
        self.training = mod.training
        self._relu = False
        self._code_out = None
        self._last_kernel = None
        self._asked = {}

    def forward(self, x):
        from .sfp_quant import hip_global_avgpool, global_avgpool_supported, hip_encode
        out = self._code_out
        if (not self.training and not torch.is_grad_enabled() and torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32
                and x.dim() == 4):
            key = (x.shape, x.stride(), out)   # the query is host only, but it is a ctypes call per forward: asked once per geometry
            ok = self._asked.get(key)
            if ok is None:
                if len(self._asked) >= 64:
                    self._asked.clear()
                ok = self._asked[key] = _avgpool_global(self.mod, x) and global_avgpool_supported(x, out)
            if ok:
                self._last_kernel = "global_avgpool" + ("+relu" if self._relu else "") + ("+codes_out" if out is not None else "")
                return hip_global_avgpool(x, relu=self._relu, code_out=out)
        self._last_kernel = "aten"
        y = self.mod(torch.relu(x) if self._relu else x)
        if out is not None:
            if self.training or torch.is_grad_enabled() or not y.is_cuda:
                raise RuntimeError("GlobalAvgPool2d: code links (fusion.link_pool_head) are inference-only on the ROCm device; "
                                   "call fusion.unlink_pool_head(model)")
            from .conv2d_func import _act_fmt
            y = hip_encode(y.contiguous(), out[0], _act_fmt(out[1]))
        return y


def _slots_of(model, child):
    return [(parent, name) for parent in model.modules() for name, c in parent._modules.items() if c is child]


def _restore_slots(model, unwrap, unfold):
    """The slot walk of the undo functions that put modules back: `unwrap(child)` (wrappers) and `unfold(child)` (placeholders)
    return the module to put back, or None for a child that is not their pass's.  Returns the number of distinct wrappers replaced."""
    wrappers = {}   # by identity; holding them keeps an id from being reused within the walk
    for parent in list(model.modules()):
        for name, child in list(parent._modules.items()):
            back = unwrap(child)
            if back is not None:
                wrappers[id(child)] = child
            else:
                back = unfold(child)
            if back is not None:
                parent._modules[name] = back
    return len(wrappers)


def use_device_avgpool(model, example_input):
    """Run the global average pools of `model` on libslfp_hip's kernel: one traced forward on `example_input` finds every module,
    run once, that is an nn.AdaptiveAvgPool2d with output size 1 / (1, 1) or an nn.AvgPool2d whose recorded input is exactly one
    window (kernel == (H, W), no padding, floor mode, no divisor override), on a ROCm float32 tensor the kernel takes, and puts a
    GlobalAvgPool2d wrapper in its slot.  An nn.ReLU directly in front of the pool in the same nn.Sequential is folded into the
    kernel (`_relu`; the ReLU's slot becomes FoldedReLU) where nothing else can read its result: it is run once, and if it is
    in-place its input is a tensor the module in front of it in that nn.Sequential made.  Each swap is checked alone: the
    wrapper's result on the recorded input must lie within 2 (HW + 1) 2^-24 mean64(|x|) of the recorded ATen result (the orders of
    summation differ, so the two are not bit-identical), or the swap is taken back.  Functional F.adaptive_avg_pool2d /
    F.avg_pool2d calls in a forward (ShuffleNetV2) are out of reach of a pass over modules.  Inference only; the default path of
    every module is unchanged.  Returns the number of pools swapped; restore_avgpool undoes them."""
    from .sfp_quant import global_avgpool_supported
    if model.training or not torch.is_tensor(example_input) or not example_input.is_cuda:
        return 0
    if not any(_avgpool_candidate(m) for m in model.modules()):
        return 0
    tr = _Trace(model, example_input)
    plans = []
    for c in tr.calls:
        m = c.mod
        if (not _avgpool_candidate(m) or tr.io(m) is None or c.x.dtype != torch.float32 or not c.x.is_cuda
                or not _avgpool_global(m, c.x) or not global_avgpool_supported(c.x)):
            continue
        relu = None
        for seq in (s for s in model.modules() if isinstance(s, nn.Sequential)):
            kids = list(seq._modules.values())
            i = next((k for k, kid in enumerate(kids) if kid is m), None)
            if i is None or i == 0 or type(kids[i - 1]) is not nn.ReLU:
                continue
            r = kids[i - 1]
            rio = tr.io(r)
            if rio is None or not tr.same(rio[1], c.x) or len(_slots_of(model, r)) != 1 or len(_slots_of(model, m)) != 1:
                continue
            if tr.same(rio[0], rio[1]):   # in place: the tensor must be one the Sequential's previous module made
                pio = tr.io(kids[i - 2]) if i >= 2 else None
                if pio is None or not tr.same(pio[1], rio[0]) or tr.same(pio[0], pio[1]):
                    continue
            relu = r
        plans.append((m, relu, c.x, c.out))
    done = 0
    for m, relu, x, want in plans:
        slots = _slots_of(model, m)
        if not slots:
            continue
        wrap = GlobalAvgPool2d(m)
        wrap._relu = relu is not None   # (x is the ReLU's result: max(., 0) once more changes nothing)
        ok = False
        try:
            with torch.no_grad():
                got = wrap(x)
            ok = wrap._last_kernel != "aten" and _avgpool_bound_ok(got, want, x)
        except Exception as e:
            warnings.warn(f"use_device_avgpool: {type(e).__name__}: {e}", stacklevel=2)
        if not ok:
            warnings.warn("use_device_avgpool: a pool did not reproduce its recorded output within the summation bound and stays "
                          "on ATen", stacklevel=2)
            continue
        for parent, name in slots:
            parent._modules[name] = wrap
        if relu is not None:
            for parent, name in _slots_of(model, relu):
                parent._modules[name] = FoldedReLU(relu, "avgpool")
        done += 1
    tr.release()
    return done


def restore_avgpool(model):
    """Undo use_device_avgpool (and, first, link_pool_head): every slot gets its original module back.  Of the FoldedReLU
    placeholders only this pass's own (owner "avgpool") are taken; those of the training passes stay with their wrappers.  Returns
    the number of pools restored."""
    unlink_pool_head(model)
    return _restore_slots(model, lambda c: c.mod if isinstance(c, GlobalAvgPool2d) else None,
                          lambda c: c.relu if isinstance(c, FoldedReLU) and c.owner == "avgpool" else None)


def _restore_pool_link(pool):
    rec = pool.__dict__.pop("_pool_link")
    pool._code_out = None
    rec["reader"]._code_in = False


def link_pool_head(model, example_input):
    """After use_device_avgpool: where a GlobalAvgPool2d's result reaches a Linear_Q through nn.Flatten, a functional flatten / view /
    reshape, eval-mode Dropout or nn.Identity only, the pool writes that layer's 1-byte codes (`_code_out` = the reader's (Ka,
    q_bit)) and the reader takes them (`_code_in`) and runs the weight-streaming kernel on them (slfp_linear_fwd_fc): ResNet-50's
    and the CIFAR MobileNetV1 nets' avgpool -> flatten -> fc.  One traced forward finds the links: every recorded reader of the
    pooled values (a module input with the pooled tensor's storage and element count) must be such a pass-through module or the
    one Linear_Q, which must be eligible for a head link and have the kernel (slfp_linear_fc_supported with x_codes = 1).  Each
    link is verified alone -- the reader's output on the pool's recorded input must be torch.equal to the recorded one -- then the
    whole model must reproduce the output of the un-linked model (with the device pool) on the example input, or every link is
    taken back with a warning.  link_head may run afterwards: it passes readers that are already linked.  Inference only.
    Returns the number of links; unlink_pool_head undoes them."""
    from .conv2d_func import _conv_io, _scalar_scale, options
    from .sfp_quant import global_avgpool_supported
    from . import _lib
    pools = [m for m in model.modules() if isinstance(m, GlobalAvgPool2d) and m._code_out is None]
    if (model.training or not torch.is_tensor(example_input) or not example_input.is_cuda or not pools
            or not any(_head_eligible(m) for m in model.modules())):
        return 0
    tr = _Trace(model, example_input, blocks=pools + [m for m in model.modules() if _is_linear_q(m)])
    y0 = tr.output
    if not torch.is_tensor(y0):
        return 0
    plans = []
    for i, cp in enumerate(tr.calls):
        p = cp.mod
        if (not isinstance(p, GlobalAvgPool2d) or p not in pools or tr.runs(p) != 1 or p._last_kernel == "aten"
                or not torch.is_tensor(cp.x) or not torch.is_tensor(cp.out) or cp.out.dtype != torch.float32):
            continue
        t = cp.out
        later = [c for c in tr.calls[i + 1:] if torch.is_tensor(c.x) and c.x.data_ptr() == t.data_ptr() and c.x.numel() == t.numel()]
        lins = [c for c in later if _is_linear_q(c.mod)]
        passed = [c for c in later if not _is_linear_q(c.mod)]
        if len(lins) != 1 or any(
                not (isinstance(c.mod, (nn.Flatten, nn.Identity)) or _eval_dropout(c.mod)) or tr.runs(c.mod) != 1
                or not torch.is_tensor(c.out) or c.out.data_ptr() != t.data_ptr() or c.out.numel() != t.numel() for c in passed):
            continue
        cb = lins[0]
        b = cb.mod
        if (not _head_eligible(b) or tr.runs(b) != 1 or b._code_in or cb.x.dim() != 2 or cb.x.dtype != torch.float32
                or cb.x.shape != (t.shape[0], t.shape[1]) or not torch.is_tensor(cb.out)):
            continue
        out = (float(_scalar_scale(b.Ka, "Ka")), int(b.q_bit))
        io = _conv_io(True, None)
        if not _lib.load().slfp_linear_fc_supported(cb.x.shape[0], b.in_features, b.out_features, b.q_bit, options.mfma_passes,
                                                    ctypes.byref(io), 1, 0) or not global_avgpool_supported(cp.x, out):
            continue
        plans.append((p, b, out, cp.x, cb.x.shape, cb.out))
    tr.release()
    made = []

    def take_all_back():
        for p in made:
            _restore_pool_link(p)

    for p, b, out, x_p, shape_b, want in plans:
        p.__dict__["_pool_link"] = {"reader": b}
        p._code_out = out
        b._code_in = True
        try:
            ok = _verified(lambda p=p, b=b, x_p=x_p, shape_b=shape_b: b(p(x_p).reshape(shape_b)), want,
                           lambda p=p: _restore_pool_link(p), reraise=True)
        except _lib.SlfpError:
            take_all_back()
            raise
        if ok:
            made.append(p)
        else:
            warnings.warn("link_pool_head: a link did not reproduce its reader's output and was taken back", stacklevel=2)
    if not made:
        return 0
    if not _verified(lambda: model(example_input), y0, take_all_back, reraise=True):
        warnings.warn("link_pool_head: the linked model did not reproduce its output on the example input (a functional op on the "
                      "pooled tensor?); every link was taken back", stacklevel=2)
        return 0
    return len(made)


def unlink_pool_head(model):
    """Undo link_pool_head: every attribute it wrote."""
    n = 0
    for m in list(model.modules()):
        if "_pool_link" in m.__dict__:
            _restore_pool_link(m)
            n += 1
    return n


# ------------------------------------------------------------------ the training-mode passes: fusion_train.py, reached as fusion.<name>
# (the last statement here, as the import of this module's names is there: whichever is imported first, the other finds its names)
from .fusion_train import (   # noqa: E402,F401
    FoldedTail, TrainBatchNorm2d, TrainBatchNormCodes2d, TrainBatchNormLayerout2d, _bn_bottleneck_candidate,
    use_device_bn_train, restore_bn_train, use_device_bn_layerout_train, restore_bn_layerout_train,
    use_device_bottleneck_train, restore_bottleneck_train, link_codes_train, unlink_codes_train,
    link_bottleneck_codes_train, unlink_bottleneck_codes_train,
    TrainBatchNormLayeroutCodes2d, link_layerout_codes_train, unlink_layerout_codes_train)
