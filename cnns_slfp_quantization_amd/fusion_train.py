"""Training-mode rewrites of a model built from Conv2d_Q modules: the BatchNorm tails of a QAT step on libslfp_hip's kernels, and
the hand-overs from a BatchNorm to the next Conv2d_Q as 1-byte codes.  Opt-in, before or after model.train(); every pass decides
call by call and otherwise runs what the stock modules run.  fusion.py re-exports the public names: `fusion.<name>` reaches them.
The table continues fusion.py's, with its columns; all of these are TRAINING passes and need no other pass unless one is named.

  pass                             needs                              sets                                          undo / also undone by
  use_device_bn_train(model)       --                                 nn.BatchNorm2d -> TrainBatchNorm2d (_relu), a restore_bn_train
                                                                      ReLU behind it -> FoldedReLU("bn_train")
  use_device_bn_layerout_train     -- (before or after                [BN, layerout_quantize_func, activation] ->   restore_bn_layerout_train
    (model)                        use_device_bn_train)               [TrainBatchNormLayerout2d, FoldedTail, FoldedTail]
  link_codes_train(model)          -- (before or after                [BN, ReLU, Conv2d_Q]: the BN slot ->          unlink_codes_train /
                                   use_device_bn_train)               TrainBatchNormCodes2d, a stock ReLU ->        restore_bn_train
                                                                      FoldedReLU("codes_train")
  use_device_bottleneck_train      --                                 block: instance forward, _bn_bottleneck;      restore_bottleneck_train /
    (model, x)                                                        bn1..3 -> TrainBatchNorm2d                    restore_bn_train
  link_bottleneck_codes_train      use_device_bottleneck_train        block: _bn_bottleneck_codes; bn1 / bn2 ->     unlink_bottleneck_codes_train /
    (model, x)                                                        TrainBatchNormCodes2d (_in_bottleneck); bn3   restore_bottleneck_train,
                                                                      wrapper: _trunk                               restore_bn_train
  link_layerout_codes_train(model) -- (before or after                [BN, layerout_quantize_func, activation,      unlink_layerout_codes_train /
                                   use_device_bn_layerout_train,      Conv2d_Q]: the BN slot ->                     restore_bn_layerout_train
                                   use_device_bn_train)               TrainBatchNormLayeroutCodes2d, a stock
                                                                      quantizer / activation ->
                                                                      FoldedTail("layerout_codes_train")

Shared: a placeholder belongs to one pass (FoldedReLU.owner, FoldedTail.owner) and only that pass's undo takes
it back; fusion._restore_slots, _repoint, _eval_mode, _bn_bottleneck_forward are each the one of their kind; "may this Conv2d_Q read
these training codes" is answered by conv2d_func._train_codes_reader_ok.
"""
import contextlib
import types

import torch
import torch.nn as nn

from . import batchnorm as B
from .conv2d_func import _bwd_flags, _f32, _link_conv_clean, _train_codes_reader_ok


# ------------------------------------------------------------------ training-mode BatchNorm2d (+ReLU) on the device kernels
_BN_NAMES = ("running_mean", "running_var", "num_batches_tracked")


class _DeviceBatchNorm(nn.Module):
    """What TrainBatchNorm2d, TrainBatchNormLayerout2d and TrainBatchNormCodes2d share: the stock nn.BatchNorm2d's attributes and the SAME Parameter and
    buffer objects under the same names (the stock module itself is kept outside _modules, `_bn`), the num_batches_tracked tick,
    the rule for when the kernels may run, and the F.batch_norm path on the same buffers for everything else."""
    _version = 2   # nn.BatchNorm2d's state-dict version (num_batches_tracked)

    def __init__(self, bn, min_elements):
        super().__init__()
        object.__setattr__(self, "_bn", bn)
        self.min_elements = min_elements
        self.training = bn.training
        self.num_features, self.eps, self.momentum = bn.num_features, bn.eps, bn.momentum
        self.affine, self.track_running_stats = bn.affine, bn.track_running_stats
        self.register_parameter("weight", bn.weight)
        self.register_parameter("bias", bn.bias)
        for name in _BN_NAMES:
            self.register_buffer(name, getattr(bn, name))
        self._last_kernel = None

    def _begin(self, x):
        """What every call does first: the stock module's refusal of a non-4-d input, and its num_batches_tracked tick."""
        if x.dim() != 4:
            raise ValueError(f"expected 4D input (got {x.dim()}D input)")
        if self.training and self.track_running_stats and self.num_batches_tracked is not None:
            self.num_batches_tracked.add_(1)

    def _kernel_operands(self, x, min_elements):
        """(weight, bias, running_mean, running_var) where the kernels may run this call, else None.  They may in training mode,
        without autocast, on a ROCm float32 tensor batchnorm.bn_train_supported accepts at this size rule, with these four
        float32 on its device: the kernels are handed their addresses and read and write float32 there."""
        if not (self.training and x.is_cuda and x.dtype == torch.float32) or torch.is_autocast_enabled():
            return None
        ops = (self.weight, self.bias, self.running_mean, self.running_var)
        for t in ops:
            if t is None or t.dtype != torch.float32 or t.device != x.device:
                return None
        return ops if B.bn_train_supported(x, min_elements) else None

    def _aten(self, x):
        """F.batch_norm as the stock module calls it, on the same parameters and buffers."""
        self._last_kernel = "aten"
        stats = self.training or (self.running_mean is None and self.running_var is None)
        keep = not self.training or self.track_running_stats
        return torch.nn.functional.batch_norm(x, self.running_mean if keep else None, self.running_var if keep else None,
                                              self.weight, self.bias, stats, self.momentum, self.eps)


class TrainBatchNorm2d(_DeviceBatchNorm):
    """An affine nn.BatchNorm2d (momentum not None) whose training-mode forward and backward run on libslfp_hip's kernels
    (slfp_bn_train_fwd / slfp_bn_train_bwd), with the nn.ReLU behind it folded in (`_relu`).  It registers the
    SAME Parameter and buffer objects under the same names, so state-dict keys do not change and an optimizer built before the swap
    keeps working; the original module is kept outside _modules (`_bn`).  Deliberately not a subclass of nn.BatchNorm2d: the
    eval-mode passes (fuse_bn_relu, fuse_named_bn) match by isinstance and so never fold a BN whose ReLU lives inside it.
    The kernels run in training mode on a ROCm float32 4-d channels_last tensor that slfp_bn_train_supported accepts and that
    has at least `min_elements` elements (None: batchnorm.MIN_ELEMENTS, below which the stock modules measured no slower), with
    weight, bias and the running statistics float32 on its device; eval mode, CPU tensors, autocast, other dtypes or layouts,
    smaller tensors, parameters or buffers of another dtype or device and a module without running-statistics buffers go to
    F.batch_norm with the same buffers (then relu, if folded), which is what the stock modules compute.  The output is saved
    for the backward only with a folded ReLU; without one it may be changed in place behind the module (`out += identity`, a
    shared in-place ReLU), as behind the stock module.
    A block's forward may ask more of one call (use_device_bottleneck_train): forward(x, relu=True) applies a ReLU the module does
    not own, forward(x, residual=identity, relu=True) the tail of a Bottleneck on slfp_bn_res_train_fwd / _bwd;
    where the kernels do not run, that call computes F.batch_norm, `+= residual`, relu with ATen as the stock block does.
    After link_bottleneck_codes_train has told the wrapper the Conv2d_Q layers that read its tail (`_trunk`), a residual call that
    passes _trunk_codes_ok runs slfp_bn_res_codes_train_fwd instead: the same float32 tensor, carrying the readers' 1-byte codes
    as the tensor attribute `_train_trunk_codes` = (codes, Ka, q_bit); every other call runs what it ran.
      _last_kernel   "bn_train[+relu]", "bn_res_train[+relu]", "bn_res_codes_train[+relu]", or "aten" """

    def __init__(self, bn, min_elements=None):
        super().__init__(bn, min_elements)
        self._relu = False
        # link_bottleneck_codes_train: (the Conv2d_Q readers of this tail's output, float32(Ka), q_bit, min_elements) -- a tuple, so
        # that the readers are no children of this module
        self._trunk = None

    def extra_repr(self):
        trunk = "" if self._trunk is None else f", trunk codes for Ka={self._trunk[1]}, q_bit={self._trunk[2]}"
        return f"{self.num_features}, eps={self.eps}, momentum={self.momentum}, relu={self._relu}{trunk}"

    def _trunk_codes_ok(self, x):
        """Does this call write the readers' codes next to the float32 trunk?  options.backward "hip" / "hip_all";
        the size rule and slfp_bn_res_codes_train_supported; every recorded reader may still read codes of the Ka and q_bit the link
        was made for, forward and backward (conv2d_func._train_codes_reader_ok)."""
        readers, ka, q_bit, floor = self._trunk
        return (_bwd_flags() is not None and B.bn_res_codes_train_supported(x, ka, q_bit, floor)
                and all(_train_codes_reader_ok(conv, x, ka, q_bit) for conv in readers))

    def forward(self, x, *, relu=None, residual=None):
        """relu: None -- the module's own folded ReLU (`_relu`); True / False -- what a block's forward asks of this call
        (use_device_bottleneck_train).  residual: a tensor of x's shape added behind the affine map and in front of the ReLU, the
        `out += identity` of a Bottleneck; on the kernels it is slfp_bn_res_train_fwd / _bwd, under a size
        rule of its own (batchnorm.RES_MIN_ELEMENTS where min_elements is None)."""
        self._begin(x)
        relu = self._relu if relu is None else bool(relu)
        floor = self.min_elements
        if floor is None:
            floor = B.MIN_ELEMENTS if residual is None else B.RES_MIN_ELEMENTS
        fits = residual is None or (torch.is_tensor(residual) and residual.shape == x.shape and residual.dtype == x.dtype
                                    and residual.device == x.device)
        if residual is not None and fits and self._trunk is not None:
            # the trunk's readers are known (link_bottleneck_codes_train): under the size rule of that link, the same float32 tensor
            # and, riding on it as `_train_trunk_codes`, (codes, Ka, q_bit) for them (Conv2d_Q.forward)
            cops = self._kernel_operands(x, 0)
            if cops is not None and self._trunk_codes_ok(x):
                _, ka, q_bit, _ = self._trunk
                self._last_kernel = "bn_res_codes_train+relu" if relu else "bn_res_codes_train"
                y, codes = B.hip_bn_res_codes_train.apply(x, residual, *cops, self.momentum, self.eps, relu, ka, q_bit)
                y._train_trunk_codes = (codes, ka, q_bit)
                return y
        ops = self._kernel_operands(x, floor) if fits else None
        if ops is not None:
            if residual is not None:
                self._last_kernel = "bn_res_train+relu" if relu else "bn_res_train"
                return B.hip_bn_res_train.apply(x, residual, *ops, self.momentum, self.eps, relu)
            self._last_kernel = "bn_train+relu" if relu else "bn_train"
            return B.hip_bn_train.apply(x, *ops, self.momentum, self.eps, relu)
        y = self._aten(x)
        if residual is not None:
            y += residual   # the stock block's own statements: out = bn3(out); out += identity; out = relu(out)
        return torch.relu(y) if relu else y


def _bn_train_candidate(m):
    return type(m) is nn.BatchNorm2d and m.affine and m.momentum is not None


def use_device_bn_train(model, min_elements=None):
    """Run the training-mode BatchNorm2d modules of `model` on libslfp_hip's kernels: every affine nn.BatchNorm2d with a momentum
    gets a TrainBatchNorm2d in its slot(s).  Where the module behind it in the same nn.Sequential is a plain nn.ReLU (in place or
    not) and both are held in exactly one slot, the ReLU is folded into the kernels (`_relu`; its slot becomes FoldedReLU).  A
    hand-wired BN (ResNet-50's bn1..3, whose ReLU module is shared) is swapped without a ReLU, and a layerout_quantize_func
    between BN and ReLU keeps the ReLU out.  Opt-in; eval mode and everything the kernels do not take run what the stock
    modules run, and so do tensors of fewer than `min_elements` elements (None: batchnorm.MIN_ELEMENTS, the measured rule of
    DESIGN section 27; 0: every size).  Returns the number of modules swapped; restore_bn_train undoes them."""
    todo = [(m, _slots_of(model, m)) for m in model.modules() if _bn_train_candidate(m)]
    done = 0
    for bn, slots in todo:
        if not slots:   # `model` itself
            continue
        relu = None
        if len(slots) == 1 and isinstance(slots[0][0], nn.Sequential):
            kids = list(slots[0][0]._modules.values())
            i = next(k for k, kid in enumerate(kids) if kid is bn)
            if i + 1 < len(kids) and type(kids[i + 1]) is nn.ReLU and len(_slots_of(model, kids[i + 1])) == 1:
                relu = kids[i + 1]
        wrap = TrainBatchNorm2d(bn, min_elements)
        wrap._relu = relu is not None
        for parent, name in slots:
            parent._modules[name] = wrap
        if relu is not None:
            folded = FoldedReLU(relu, "bn_train")
            for parent, name in _slots_of(model, relu):
                parent._modules[name] = folded
        done += 1
    return done


def restore_bn_train(model):
    """Undo use_device_bn_train: every slot gets its original module back; the originals are pointed at the current parameters
    and buffers (the model may have been moved or cast in between) and take the wrapper's training flag.  Blocks rewritten by
    use_device_bottleneck_train are restored first (restore_bottleneck_train): their instance-level forward calls bn1..3 with
    keywords a stock BatchNorm does not take.  Links of link_codes_train are undone first too (unlink_codes_train): a wrapper of
    theirs would hand the restored nn.ReLU a uint8 tensor."""
    restore_bottleneck_train(model)
    unlink_codes_train(model)
    return _restore_slots(model, lambda c: _repoint(c._bn, c) if isinstance(c, TrainBatchNorm2d) else None,
                          lambda c: c.relu if isinstance(c, FoldedReLU) and c.owner == "bn_train" else None)


# ------------------------------------------------------------------ training-mode Bottleneck tails: BN + ReLU, BN + add + ReLU
_BN_BOTTLENECK_BNS = ("bn1", "bn2", "bn3")


def _bn_tail(bn, t):
    """relu(bn(t)) of a rewritten Bottleneck: a TrainBatchNorm2d is asked for the ReLU, a link's wrapper (TrainBatchNormCodes2d,
    link_bottleneck_codes_train) owns it and may hand on uint8 codes."""
    return bn(t) if isinstance(bn, TrainBatchNormCodes2d) else bn(t, relu=True)


def _bn_bottleneck_forward(self, x):
    """The dataflow of the Bottleneck the reference copies (nets_imgnet/resnet50.py:71-90) with each ReLU, and the add in front of
    the last one, handed to the wrapper in front of it.  The one instance-level forward of a rewritten block, linked or not: it
    asks the module that is in the slot, so a linked bn1 / bn2 hands its codes straight to conv2 / conv3."""
    out = _bn_tail(self.bn1, self.conv1(x))
    out = _bn_tail(self.bn2, self.conv2(out))
    identity = x if getattr(self, "downsample", None) is None else self.downsample(x)
    return self.bn3(self.conv3(out), residual=identity, relu=True)


def _bn_wrappable(m):
    """A BatchNorm a later pass may take: the stock module use_device_bn_train takes, or its wrapper without a folded ReLU."""
    return _bn_train_candidate(m) or (isinstance(m, TrainBatchNorm2d) and not m._relu)


def _bn_bottleneck_candidate(blk):
    if isinstance(blk, nn.Sequential) or "forward" in blk.__dict__:
        return False
    ch = blk._modules
    if any(ch.get(k) is None for k in _BOTTLENECK_CHILDREN + ("bn3",)) or "downsample" not in ch and not hasattr(blk, "downsample"):
        return False
    return type(ch["relu"]) is nn.ReLU and all(_bn_wrappable(ch[k]) for k in _BN_BOTTLENECK_BNS)


def _repoint(held, wrap):
    """`held` -- wrapper `wrap`'s stock BatchNorm (`wrap._bn`) or a TrainBatchNorm2d it stands in for -- pointed at the wrapper's current
    Parameters, buffers and training flag (a move or a cast since the swap replaced them on the wrapper alone).  Returns `held`."""
    for key in ("weight", "bias"):
        held._parameters[key] = wrap._parameters[key]
    for key in _BN_NAMES:
        held._buffers[key] = wrap._buffers[key]
    held.training = wrap.training
    return held


@contextlib.contextmanager
def _eval_mode(model):
    """model.eval() for the span of a trace; every module's training flag is put back on the way out, in every case."""
    flags = [(m, m.training) for m in model.modules()]
    model.eval()
    try:
        yield
    finally:
        for m, t in flags:
            m.training = t


def _restore_bn_bottleneck(blk):
    """Take the instance-level forward off `blk` and put back the stock module wherever this pass created the wrapper.  Links of
    link_bottleneck_codes_train are undone first: they stand in the wrappers' slots."""
    _unlink_bottleneck_codes(blk)
    created = blk.__dict__.pop("_bn_bottleneck")
    del blk.__dict__["forward"]
    for name, wrap in created.items():
        if blk._modules.get(name) is wrap:
            blk._modules[name] = _repoint(wrap._bn, wrap)


def use_device_bottleneck_train(model, example_input, min_elements=None):
    """Run the three tails of every training-mode Bottleneck of `model` on libslfp_hip's kernels: relu(bn1(.)) and relu(bn2(.)) as
    slfp_bn_train_fwd / _bwd with the ReLU folded, and out = bn3(out); out += identity; out = relu(out) as slfp_bn_res_train_fwd /
    _bwd.  A candidate is a non-Sequential module without an instance-level forward that has the children
    conv1 / bn1 / conv2 / bn2 / conv3 / bn3 / relu and a `downsample` attribute (None allowed), bn1..3 each an affine
    nn.BatchNorm2d with a momentum held in that one slot, or a TrainBatchNorm2d without a folded ReLU, and relu a plain nn.ReLU;
    the convolutions may be any module and are not touched.  It gets TrainBatchNorm2d wrappers in the three slots (wrappers that
    are there already are reused) and an instance-level forward with the block's dataflow.  A name is only a convention, so -- the
    rule of fuse_residual -- the pass verifies: it puts the model in eval mode (there every BatchNorm is F.batch_norm with the
    running statistics and nothing is updated, so the rewritten dataflow must equal the stock one exactly), traces one no_grad
    forward on `example_input`, and each rewritten block must reproduce its recorded output bit for bit on its recorded input
    (otherwise it is restored and not counted); then the rewritten model must reproduce the recorded output bit for bit
    (otherwise everything is restored and 0 is returned).  The training flags are put back in every case.  Parameters, buffers
    and state-dict keys do not change.  Composes with use_device_bn_train in either order (a BatchNorm inside `downsample` is that
    pass's).  Tensors of fewer than `min_elements` elements run what the stock block runs (None: batchnorm.MIN_ELEMENTS for
    bn1 / bn2, batchnorm.RES_MIN_ELEMENTS for bn3; 0: every size).  Returns the number of blocks rewritten;
    restore_bottleneck_train undoes them."""
    cands = [m for m in model.modules() if _bn_bottleneck_candidate(m)
             and all(isinstance(m._modules[k], TrainBatchNorm2d) or len(_slots_of(model, m._modules[k])) == 1
                     for k in _BN_BOTTLENECK_BNS)]
    if not cands:
        return 0
    made = []
    try:
        with _eval_mode(model):
            tr = _Trace(model, example_input, blocks=cands)
            y0 = tr.output
            done = []
            for blk in cands:
                io = tr.io(blk)
                if io is None:
                    continue   # not run, run twice, or not a tensor -> tensor block
                x, want = io
                created = {}
                for name in _BN_BOTTLENECK_BNS:
                    bn = blk._modules[name]
                    if not isinstance(bn, TrainBatchNorm2d):
                        created[name] = blk._modules[name] = TrainBatchNorm2d(bn, min_elements)
                made += created.values()
                blk.__dict__["_bn_bottleneck"] = created
                blk.__dict__["forward"] = types.MethodType(_bn_bottleneck_forward, blk)
                if _verified(lambda: blk(x), want, lambda: _restore_bn_bottleneck(blk)):
                    done.append(blk)
            tr.release()
            if not done:
                return 0

            def undo():
                for blk in done:
                    _restore_bn_bottleneck(blk)

            return len(done) if _verified(lambda: model(example_input), y0, undo) else 0
    finally:
        for wrap in made:   # created in eval mode: the stock module's flag, put back by now, is the slot's
            wrap.training = wrap._bn.training


def restore_bottleneck_train(model):
    """Undo use_device_bottleneck_train: the blocks lose their instance-level forward and exactly the wrappers that pass created
    give their slots back to the stock modules (pointed at the current parameters and buffers); wrappers that were there before
    it stay.  Returns the number of blocks restored."""
    n = 0
    for blk in list(model.modules()):
        if "_bn_bottleneck" in blk.__dict__:
            _restore_bn_bottleneck(blk)
            n += 1
    return n


# ------------------------------------------------------------------ training-mode BatchNorm2d -> layer-output quantizer -> activation
class FoldedTail(nn.Module):
    """The slot of a layerout_quantize_func or of an activation module that the wrapper in front of it applies: the identity, in
    the style of FoldedReLU.  The original is kept outside _modules (`mod`); it has no parameters, the state dict does not change.
    `owner` names the pass that put it there, whose undo alone takes it back: "bn_layerout_train" (use_device_bn_layerout_train:
    a TrainBatchNormLayerout2d in front; the default) or "layerout_codes_train" (link_layerout_codes_train: a
    TrainBatchNormLayeroutCodes2d in front, whose uint8 codes pass through)."""

    def __init__(self, mod, owner="bn_layerout_train"):
        super().__init__()
        if owner not in ("bn_layerout_train", "layerout_codes_train"):
            raise ValueError(f"FoldedTail: owner must be 'bn_layerout_train' or 'layerout_codes_train', got {owner!r}")
        object.__setattr__(self, "mod", mod)
        self.owner = owner
        self.training = mod.training

    def extra_repr(self):
        return f"{type(self.mod).__name__}, owner={self.owner}"

    def forward(self, x):
        return x


class TrainBatchNormLayerout2d(_DeviceBatchNorm):
    """The tail [BatchNorm2d, layerout_quantize_func(q_bit 7 or 8), activation(s)] of a training block of MobileNetV1_swish /
    VGG16_gelu on libslfp_hip's kernels (slfp_bn_lut_train_fwd / slfp_bn_lut_train_bwd): behind the quantizer a
    value is one of a few thousand classes, so the activation and its derivative are two float32 tables
    (batchnorm.layerout_act_tables, built by the stock modules themselves, lazily per device).  As TrainBatchNorm2d it registers
    the SAME Parameter and buffer objects under the same names and keeps the original modules outside _modules (`_bn`,
    `_layerout`, `_acts`); it is not an nn.BatchNorm2d subclass.  The kernels run in training mode on a ROCm float32 4-d
    channels_last tensor that slfp_bn_train_supported accepts and that has at least `min_elements` elements (None:
    batchnorm.LUT_MIN_ELEMENTS, the measured rule), with weight, bias and the running statistics float32 on its device.  Eval mode, CPU tensors, autocast, other dtypes or layouts and smaller tensors
    run F.batch_norm on the same buffers, then the kept quantizer module, then the kept activation modules: bit for bit what the
    stock modules compute.  The output is never saved for the backward; it may be changed in place behind the module.
      _last_kernel   "bn_lut_train", or "aten" """

    def __init__(self, bn, layerout, acts, min_elements=None):
        if isinstance(bn, TrainBatchNorm2d):
            if bn._relu:
                raise ValueError("TrainBatchNormLayerout2d: the TrainBatchNorm2d has a ReLU folded in")
            bn = _repoint(bn._bn, bn)   # the wrapper holds the current Parameters and buffers
        acts = tuple(acts)
        for act in acts:
            if type(act) not in B._lut_act_types():
                raise TypeError(f"TrainBatchNormLayerout2d: {type(act).__name__} has no derivative table")
        super().__init__(bn, min_elements)
        object.__setattr__(self, "_layerout", layerout)
        object.__setattr__(self, "_acts", acts)
        self._tables = {}

    def extra_repr(self):
        return (f"{self.num_features}, eps={self.eps}, momentum={self.momentum}, layerout={self._layerout.q_bit}, "
                f"acts={[type(a).__name__ for a in self._acts]}")

    def tables(self, device):
        """(F, D) of batchnorm.layerout_act_tables on `device`, built once per device."""
        key = str(device)
        t = self._tables.get(key)
        if t is None:
            t = self._tables[key] = B.layerout_act_tables(self._acts, device)
        return t

    def forward(self, x):
        self._begin(x)
        ops = self._kernel_operands(x, B.LUT_MIN_ELEMENTS if self.min_elements is None else self.min_elements)
        if ops is not None:
            self._last_kernel = "bn_lut_train"
            return B.hip_bn_lut_train.apply(x, *ops, self.momentum, self.eps, *self.tables(x.device))
        y = self._aten(x)
        y = self._layerout(y)
        for act in self._acts:
            y = act(y)
        return y


def use_device_bn_layerout_train(model, min_elements=None):
    """Run the training blocks [BatchNorm2d, layerout_quantize_func, ReLU | Swish | GELU | ...] of `model` on libslfp_hip's table
    kernels: inside an nn.Sequential, an affine nn.BatchNorm2d with a momentum (or a TrainBatchNorm2d without a folded ReLU, so
    this pass and use_device_bn_train may run in either order), directly followed by a layerout_quantize_func with q_bit 7 or 8
    and by one activation module batchnorm.layerout_act_tables accepts, each held in exactly one slot, becomes a
    TrainBatchNormLayerout2d; the quantizer's and the activation's slots become FoldedTail placeholders.  q_bit == 32 (no
    quantizer: no table), activation_func.STL, a shared module and a hand-wired block are skipped.  Opt-in; eval mode and everything
    the kernels do not take run what the stock modules run, and so do tensors of fewer than `min_elements` elements (None:
    batchnorm.LUT_MIN_ELEMENTS, the measured rule of DESIGN section 32; 0: every size).  Returns the number of blocks taken;
    restore_bn_layerout_train undoes them."""
    done = 0
    for seq in [s for s in model.modules() if isinstance(s, nn.Sequential)]:
        names = list(seq._modules.keys())
        for i in range(len(names) - 2):
            bn, lo, act = (seq._modules[k] for k in names[i:i + 3])
            if not (_bn_wrappable(bn) and _is_layerout(lo) and type(act) in B._lut_act_types()):
                continue
            if any(len(_slots_of(model, m)) != 1 for m in (bn, lo, act)):
                continue
            seq._modules[names[i]] = TrainBatchNormLayerout2d(bn, lo, (act,), min_elements)
            seq._modules[names[i + 1]] = FoldedTail(lo)
            seq._modules[names[i + 2]] = FoldedTail(act)
            done += 1
    return done


def restore_bn_layerout_train(model):
    """Undo use_device_bn_layerout_train: every slot gets its original module back (the stock nn.BatchNorm2d, also where a
    TrainBatchNorm2d stood in the slot); the originals are pointed at the current parameters and buffers (the model may have been
    moved or cast in between) and take the placeholders' training flags.  Links of link_layerout_codes_train are undone first
    (unlink_layerout_codes_train): a wrapper of theirs would hand the restored quantizer a uint8 tensor."""
    unlink_layerout_codes_train(model)
    return _restore_slots(model, lambda c: _repoint(c._bn, c) if isinstance(c, TrainBatchNormLayerout2d) else None,
                          lambda c: _unfold_tail(c, "bn_layerout_train"))


def _unfold_tail(c, owner):
    """The module behind a FoldedTail of `owner`, with the placeholder's training flag; None for any other child."""
    if isinstance(c, FoldedTail) and c.owner == owner:
        c.mod.training = c.training
        return c.mod
    return None


# ------------------------------------------------------------------ training-mode BatchNorm2d + ReLU -> the next Conv2d_Q on 1-byte codes
class TrainBatchNormCodes2d(_DeviceBatchNorm):
    """The BatchNorm2d of a run [BatchNorm2d, ReLU, Conv2d_Q] linked by link_codes_train: in a training step it
    runs slfp_bn_codes_train_fwd without recording and returns relu(batch_norm(x)) as the uint8 channels_last codes of the
    Conv2d_Q's own quantizer; the tensor carries a batchnorm.TrainLink (attribute `_train_link`: x with its graph, the operands,
    the saves), the ReLU slot passes it through and the Conv2d_Q runs BN -> ReLU -> conv as one autograd Function on it
    (batchnorm.hip_bn_codes_conv_train).  As TrainBatchNorm2d it registers the SAME Parameter and buffer objects under the same
    names; what stood in the two slots is kept outside _modules (`_held`).
    The code path is taken per call only where all of this holds: training mode, no autocast, a channels_last float32 ROCm input of
    at least `min_elements` elements (None: batchnorm.CODES_MIN_ELEMENTS) with float32 parameters and buffers on its device;
    slfp_bn_codes_train_supported; a code-reading float32-output forward for the conv under the current options;
    slfp_conv2d_bwd_codes_supported under options.backward "hip" / "hip_all" ("composite" never takes it); and the conv still in
    training mode with the Ka and q_bit the link was made for, nothing fused onto it.  Otherwise the call does what stood in the
    slots does -- a TrainBatchNorm2d with its folded ReLU under its own size rule, or F.batch_norm and a ReLU -- and the conv
    sees float32.
      _last_kernel   "bn_codes_train+relu", or "bn_train+relu" / "aten" """

    def __init__(self, held_bn, held_relu, conv, min_elements=None):
        kernels = isinstance(held_bn, TrainBatchNorm2d)
        super().__init__(_repoint(held_bn._bn, held_bn) if kernels else held_bn, min_elements)
        object.__setattr__(self, "_held", (held_bn, held_relu))
        object.__setattr__(self, "_conv", conv)
        self._fallback = (kernels, held_bn.min_elements if kernels else None)   # what the slot ran: the kernels (+ size rule) or ATen
        self._ka, self._q_bit = _f32(conv.Ka), conv.q_bit

    def extra_repr(self):
        return f"{self.num_features}, eps={self.eps}, momentum={self.momentum}, relu=True, codes for Ka={self._ka}, q_bit={self._q_bit}"

    def _codes_ok(self, x):
        """The code form's own size rule and library query, then the reader check (conv2d_func._train_codes_reader_ok)."""
        return (B.bn_codes_train_supported(x, self._ka, self._q_bit, self.min_elements)
                and _train_codes_reader_ok(self._conv, x, self._ka, self._q_bit))

    def forward(self, x):
        self._begin(x)
        ops = self._kernel_operands(x, 0)
        if ops is not None and self._codes_ok(x):
            codes, *saves = B.bn_codes_train_fwd(x, *ops, self.momentum, self.eps, True, self._ka, self._q_bit)
            codes._train_link = B.TrainLink(x, self.weight, self.bias, saves, True, self._ka, self._q_bit, self._conv)
            self._last_kernel = "bn_codes_train+relu"
            return codes
        kernels, floor = self._fallback
        ops = self._kernel_operands(x, B.MIN_ELEMENTS if floor is None else floor) if kernels else None
        if ops is not None:
            self._last_kernel = "bn_train+relu"
            return B.hip_bn_train.apply(x, *ops, self.momentum, self.eps, True)
        return torch.relu(self._aten(x))


def _flat_slots(seq, model, once=True):
    """(parent, name, module, once) of the leaves of nested nn.Sequentials, in the order they run.  once: every nested Sequential
    around the leaf sits in exactly one slot of `model`, so the leaf appears once in this order and has one successor."""
    for name, m in seq._modules.items():
        if isinstance(m, nn.Sequential):
            yield from _flat_slots(m, model, once and len(_slots_of(model, m)) == 1)
        else:
            yield seq, name, m, once


def link_codes_train(model, min_elements=None):
    """Hand activations from BatchNorm to the next Conv2d_Q as 1-byte codes in a TRAINING step.  Candidates are
    runs [BatchNorm2d | TrainBatchNorm2d with a folded ReLU, ReLU | FoldedReLU, Conv2d_Q] in the flattened leaf order of nested
    nn.Sequentials, so a block's last ReLU meets the next block's first conv (nets_imgnet/mobilenetv1.py:24-41).  ATen is never
    asked to read a uint8 tensor: each of the three sits in exactly one slot (and so does every nested Sequential around it: a
    block held twice has two successors), the BN is affine with a momentum, the conv has q_bit 8
    or 7, no raw bias and nothing fused onto it (_post, _code_out, _image_table).  Hand-wired blocks (Bottleneck, Fire, ShuffleNet
    units) are left alone.  The BN's slot gets a TrainBatchNormCodes2d, a stock ReLU's slot a FoldedReLU; the conv is not touched
    (Conv2d_Q.forward recognises the record on its input).  Opt-in: every call decides for itself (TrainBatchNormCodes2d), and
    tensors of fewer than `min_elements` elements (None: batchnorm.CODES_MIN_ELEMENTS; 0: every size) stay float32.  Composes with
    use_device_bn_train in either order.  Returns the number of links; unlink_codes_train undoes them."""
    nested = {c for m in model.modules() if isinstance(m, nn.Sequential) for c in m._modules.values() if isinstance(c, nn.Sequential)}
    done = 0
    for seq in [m for m in model.modules() if isinstance(m, nn.Sequential) and m not in nested]:
        leaves = list(_flat_slots(seq, model))
        i = 0
        while i + 2 < len(leaves):
            (pb, nb, bn, o1), (pr, nr, relu, o2), (_, _, conv, o3) = leaves[i:i + 3]
            stock = _bn_train_candidate(bn) and type(relu) is nn.ReLU
            swapped = (isinstance(bn, TrainBatchNorm2d) and bn._relu and bn.momentum is not None and isinstance(relu, FoldedReLU)
                       and relu.owner == "bn_train")
            if not ((stock or swapped) and o1 and o2 and o3 and _is_conv_q(conv) and _link_conv_clean(conv)
                    and all(len(_slots_of(model, m)) == 1 for m in (bn, relu, conv))):
                i += 1
                continue
            pb._modules[nb] = TrainBatchNormCodes2d(bn, relu, conv, min_elements)
            if stock:
                pr._modules[nr] = FoldedReLU(relu, "codes_train")
            done += 1
            i += 3
    return done


def _held_bn(wrap):
    """What stood in a TrainBatchNormCodes2d's slot, pointed at the wrapper's current parameters, buffers and training flag."""
    _repoint(wrap._bn, wrap)   # the stock module, which a held TrainBatchNorm2d keeps as its own `_bn`
    return _repoint(wrap._held[0], wrap)


def unlink_codes_train(model):
    """Undo link_codes_train: every slot gets back what it held (the stock modules, or use_device_bn_train's wrappers), pointed at
    the current parameters, buffers and training flag.  The in-block links of link_bottleneck_codes_train are not this pass's and
    stay (unlink_bottleneck_codes_train).  Returns the number of links undone."""
    return _restore_slots(
        model, lambda c: _held_bn(c) if isinstance(c, TrainBatchNormCodes2d) and not c.__dict__.get("_in_bottleneck") else None,
        lambda c: c.relu if isinstance(c, FoldedReLU) and c.owner == "codes_train" else None)


# ------------------------------------------------------------------ training-mode BatchNorm2d -> layer-output quantizer -> activation -> the next Conv2d_Q on 1-byte codes
class TrainBatchNormLayeroutCodes2d(_DeviceBatchNorm):
    """The BatchNorm2d of a run [BatchNorm2d, layerout_quantize_func(q_bit 7 or 8), activation, Conv2d_Q] linked by
    link_layerout_codes_train: in a training step it runs slfp_bn_lut_codes_train_fwd without recording and
    returns act(layerout(batch_norm(x))) as the uint8 channels_last codes of the Conv2d_Q's own quantizer -- behind the layer-output
    quantizer the activation and the reader's quantize_act(. / Ka) are one byte table over the class (batchnorm.layerout_code_table).
    The tensor carries a batchnorm.TrainLink with the activation's derivative table; the two slots behind pass it through and the
    Conv2d_Q runs BN -> quantizer -> activation -> conv as one autograd Function on it (batchnorm.hip_bn_codes_conv_train, whose
    backward is slfp_conv2d_bwd_codes, then slfp_bn_lut_train_bwd).  As the other wrappers it registers the SAME Parameter and buffer
    objects under the same names; what stood in the three slots is kept outside _modules (`_held`), and so are the stock quantizer
    and activation (`_layerout`, `_acts`).  The (F, D) tables and the code table are built lazily per device.
    The code path is taken per call only where all of this holds: training mode, no autocast, a channels_last float32 ROCm input of
    at least `min_elements` elements (None: batchnorm.LUT_CODES_MIN_ELEMENTS, which may be None = never) with float32 parameters and
    buffers on its device; slfp_bn_lut_codes_train_supported (C % 4 == 0); and conv2d_func._train_codes_reader_ok for the conv with
    the Ka and q_bit the link was made for (options.backward = "composite" never takes it).  Otherwise the call does what stood in
    the slots does -- a TrainBatchNormLayerout2d under its own size rule, or F.batch_norm, the kept quantizer, the kept activation
    -- and the conv sees float32.  A layer-output value of exactly zero is the NaN class: the float32 path hands the reader that
    NaN, the code path 0x00, the tiny class (DESIGN sections 21, 35); the BN's own outputs do not differ.
      _last_kernel   "bn_lut_codes_train", or "bn_lut_train" / "aten" """

    def __init__(self, held_bn, held_layerout, held_act, conv, min_elements=None):
        lut = isinstance(held_bn, TrainBatchNormLayerout2d)
        super().__init__(_repoint(held_bn._bn, held_bn) if lut or isinstance(held_bn, TrainBatchNorm2d) else held_bn, min_elements)
        layerout = held_layerout.mod if isinstance(held_layerout, FoldedTail) else held_layerout
        act = held_act.mod if isinstance(held_act, FoldedTail) else held_act
        if type(act) not in B._lut_act_types():
            raise TypeError(f"TrainBatchNormLayeroutCodes2d: {type(act).__name__} has no derivative table")
        # a TrainBatchNorm2d (without a folded ReLU) is taken as the stock module it wraps, as TrainBatchNormLayerout2d takes it
        object.__setattr__(self, "_held", (held_bn if lut else self._bn, held_layerout, held_act))
        object.__setattr__(self, "_layerout", layerout)
        object.__setattr__(self, "_acts", (act,))
        object.__setattr__(self, "_conv", conv)
        self._fallback = (lut, held_bn.min_elements if lut else None)   # what the slots ran: the table kernels (+ size rule) or ATen
        self._ka, self._q_bit = _f32(conv.Ka), conv.q_bit
        self._tables, self._code_tables = {}, {}

    def extra_repr(self):
        return (f"{self.num_features}, eps={self.eps}, momentum={self.momentum}, layerout={self._layerout.q_bit}, "
                f"acts={[type(a).__name__ for a in self._acts]}, codes for Ka={self._ka}, q_bit={self._q_bit}")

    def tables(self, device):
        """(F, D) of batchnorm.layerout_act_tables on `device`, built once per device."""
        key = str(device)
        t = self._tables.get(key)
        if t is None:
            t = self._tables[key] = B.layerout_act_tables(self._acts, device)
        return t

    def code_table(self, device):
        """batchnorm.layerout_code_table for the linked conv's quantizer on `device`, built once per device."""
        key = str(device)
        t = self._code_tables.get(key)
        if t is None:
            t = self._code_tables[key] = B.layerout_code_table(self._acts, self._ka, self._q_bit, device)
        return t

    def _codes_ok(self, x):
        """The form's own size rule and library query, then the reader check (conv2d_func._train_codes_reader_ok)."""
        return B.bn_lut_codes_train_supported(x, self.min_elements) and _train_codes_reader_ok(self._conv, x, self._ka, self._q_bit)

    def forward(self, x):
        self._begin(x)
        ops = self._kernel_operands(x, 0)
        if ops is not None and self._codes_ok(x):
            codes, *saves = B.bn_lut_codes_train_fwd(x, *ops, self.momentum, self.eps, self.code_table(x.device))
            codes._train_link = B.TrainLink(x, self.weight, self.bias, saves, False, self._ka, self._q_bit, self._conv,
                                            self.tables(x.device)[1])
            self._last_kernel = "bn_lut_codes_train"
            return codes
        lut, floor = self._fallback
        ops = self._kernel_operands(x, B.LUT_MIN_ELEMENTS if floor is None else floor) if lut else None
        if ops is not None:
            self._last_kernel = "bn_lut_train"
            return B.hip_bn_lut_train.apply(x, *ops, self.momentum, self.eps, *self.tables(x.device))
        y = self._aten(x)
        y = self._layerout(y)
        for act in self._acts:
            y = act(y)
        return y


def link_layerout_codes_train(model, min_elements=None):
    """Hand activations from a layer-output-quantized block to the next Conv2d_Q as 1-byte codes in a TRAINING step (DESIGN section
    41).  Candidates are runs of four in the flattened leaf order of nested nn.Sequentials (_flat_slots):
    [nn.BatchNorm2d | TrainBatchNorm2d without a folded ReLU | TrainBatchNormLayerout2d, layerout_quantize_func(q_bit 7 or 8) | its
    FoldedTail, one activation batchnorm.layerout_act_tables accepts | its FoldedTail, Conv2d_Q].  Each of the four sits in exactly
    one slot (and so does every nested Sequential around it), the BN is affine with a momentum, the conv has q_bit 8 or 7, no raw
    bias and nothing fused onto it (_link_conv_clean).  The Conv2d_Q must stand DIRECTLY behind the activation: an nn.MaxPool2d in
    between (the last pair of each VGG stage) leaves the pair unlinked, since bit-equal pool gradients need the float32 argmax, whose
    ties differ from ties among codes.  q_bit == 32, activation_func.STL, a shared module, a BN with a folded ReLU and hand-wired
    blocks are skipped.  The BN's slot gets a TrainBatchNormLayeroutCodes2d, a stock quantizer's and activation's slots a
    FoldedTail("layerout_codes_train"); placeholders of use_device_bn_layerout_train stay where they are; the conv is not touched
    (Conv2d_Q.forward recognises the record on its input).  Opt-in: every call decides for itself, and tensors of fewer than
    `min_elements` elements (None: batchnorm.LUT_CODES_MIN_ELEMENTS, which may be None = never; 0: every size) stay float32.
    Composes with use_device_bn_layerout_train and use_device_bn_train in either order.  A TrainBatchNorm2d in the BN's slot is
    taken as the stock module it wraps, as use_device_bn_layerout_train takes it: the wrapper's fallback is then ATen, not the
    plain BatchNorm kernels, and the undo puts the stock nn.BatchNorm2d into the slot.  Returns the number of links;
    unlink_layerout_codes_train undoes them."""
    nested = {c for m in model.modules() if isinstance(m, nn.Sequential) for c in m._modules.values() if isinstance(c, nn.Sequential)}
    done = 0
    for seq in [m for m in model.modules() if isinstance(m, nn.Sequential) and m not in nested]:
        leaves = list(_flat_slots(seq, model))
        i = 0
        while i + 3 < len(leaves):
            (pb, nb, bn, o1), (pl, nl, lo, o2), (pa, na, act, o3), (_, _, conv, o4) = leaves[i:i + 4]
            stock = _bn_wrappable(bn) and _is_layerout(lo) and type(act) in B._lut_act_types()
            swapped = (isinstance(bn, TrainBatchNormLayerout2d) and bn.momentum is not None and len(bn._acts) == 1
                       and all(isinstance(t, FoldedTail) and t.owner == "bn_layerout_train" for t in (lo, act))
                       and lo.mod is bn._layerout and act.mod is bn._acts[0])
            if not ((stock or swapped) and o1 and o2 and o3 and o4 and _is_conv_q(conv) and _link_conv_clean(conv)
                    and all(len(_slots_of(model, m)) == 1 for m in (bn, lo, act, conv))):
                i += 1
                continue
            pb._modules[nb] = TrainBatchNormLayeroutCodes2d(bn, lo, act, conv, min_elements)
            if stock:
                pl._modules[nl] = FoldedTail(lo, "layerout_codes_train")
                pa._modules[na] = FoldedTail(act, "layerout_codes_train")
            done += 1
            i += 3
    return done


def _held_layerout_bn(wrap):
    """What a TrainBatchNormLayeroutCodes2d gives its slot back: the stock BatchNorm or the TrainBatchNormLayerout2d it holds,
    pointed at the wrapper's current parameters, buffers and training flag."""
    _repoint(wrap._bn, wrap)   # the stock module, which a held TrainBatchNormLayerout2d keeps as its own `_bn`
    return _repoint(wrap._held[0], wrap)


def unlink_layerout_codes_train(model):
    """Undo link_layerout_codes_train: every slot gets back what it held (the stock modules, or use_device_bn_layerout_train's
    wrapper, whose placeholders stayed), pointed at the current parameters, buffers and training flags.  One slot does not get
    back what stood in it: where the link found a TrainBatchNorm2d (use_device_bn_train before the link) the slot gets the
    stock nn.BatchNorm2d that wrapper stood for -- what restore_bn_train would have put there, and what
    restore_bn_layerout_train does in the same case; run use_device_bn_train again to have the kernels back.  Returns the
    number of links undone."""
    return _restore_slots(model, lambda c: _held_layerout_bn(c) if isinstance(c, TrainBatchNormLayeroutCodes2d) else None,
                          lambda c: _unfold_tail(c, "layerout_codes_train"))


# ------------------------------------------------------------------ training-mode Bottlenecks on 1-byte codes: in-block links and the trunk
def _unlink_bottleneck_codes(blk):
    """Undo what link_bottleneck_codes_train did to `blk`; returns (in-block links, trunk links) undone."""
    rec = blk.__dict__.pop("_bn_bottleneck_codes", None)
    if rec is None:
        return 0, 0
    n = 0
    for name, wrap in rec["in_block"].items():
        if blk._modules.get(name) is wrap:
            blk._modules[name] = _held_bn(wrap)
            n += 1
    t = 0
    bn3 = rec["trunk"]
    if bn3 is not None and bn3._trunk is not None:
        bn3._trunk = None
        t = 1
    return n, t


def link_bottleneck_codes_train(model, example_input, min_elements=None, *, in_block=True, trunk=True):
    """Put the hand-overs of the training Bottlenecks of `model` on 1-byte codes.  It works on the blocks
    use_device_bottleneck_train has rewritten (those carrying `_bn_bottleneck`); with none it returns (0, 0) and touches nothing.
    In-block links: relu(bn1(.)) -> conv2 and relu(bn2(.)) -> conv3, where the slot holds a TrainBatchNorm2d without a folded ReLU
    and the conv is a Conv2d_Q with q_bit 8 or 7, no raw bias and nothing fused onto it (_link_conv_clean).  The slot gets a
    TrainBatchNormCodes2d made for that conv -- section 35's wrapper, with its per-call decision and fallback --; the block's
    instance-level forward (_bn_bottleneck_forward) asks the module in the slot and hands the uint8 tensor straight on.
    Trunk links: one traced eval-mode forward on `example_input` (_Trace, as link_trunk uses it) finds for each rewritten block the
    Conv2d_Q layers whose input IS its output: the next block's conv1, and downsample.0 at a stage boundary.  A link needs at least
    one reader, every reader run exactly once and clean (_link_conv_clean), and all of them sharing (float32(Ka), q_bit): one code
    tensor serves them.  The block's bn3 wrapper records the readers (`_trunk`); the readers themselves are not modified.  In a
    training step the tail then runs slfp_bn_res_codes_train_fwd, and each reader its code-reading forward and slfp_conv2d_bwd_codes
    (Conv2d_Q.forward; batchnorm.hip_trunk_codes_conv_train), call by call and only where TrainBatchNorm2d._trunk_codes_ok holds.
    Never linked on the trunk: the stem's output into the first block (no rewritten block made it), a last block read only by the
    pool, a boundary whose conv1 and downsample.0 differ in Ka; each costs exactly its own link.  The float32 trunk is still
    written and saved (the ReLU's mask, the next add): a trunk link saves traffic at the readers, not memory.
    min_elements: tensors of fewer elements stay float32 (None: batchnorm.CODES_MIN_ELEMENTS for in-block links and
    batchnorm.RES_CODES_MIN_ELEMENTS for trunk links, either of which may be None = never; 0: every size).  in_block / trunk: make
    only one kind of link (the measurement of section 38 times them apart).  Opt-in, never a default.
    Parameters, buffers, state-dict keys and optimizer bindings do not change; the training flags are put back.  Returns
    (in_block_links, trunk_links); unlink_bottleneck_codes_train undoes exactly these, restore_bottleneck_train and
    restore_bn_train take them along."""
    blocks = [m for m in model.modules() if "_bn_bottleneck" in m.__dict__ and "_bn_bottleneck_codes" not in m.__dict__]
    if not blocks:
        return 0, 0
    with _eval_mode(model):
        tr = _Trace(model, example_input, blocks=blocks)
        readers_of = {}
        for blk in blocks if trunk else ():
            io = tr.io(blk)
            bn3 = blk._modules.get("bn3")
            if io is None or not isinstance(bn3, TrainBatchNorm2d) or bn3._relu or bn3._trunk is not None or tr.runs(bn3) != 1:
                continue
            want = io[1]
            if want.dim() != 4 or want.dtype != torch.float32:
                continue
            readers = [c.mod for c in tr.readers(want) if _is_conv_q(c.mod)]
            if not readers or any(tr.runs(b) != 1 or not _link_conv_clean(b) for b in readers):
                continue
            if len({(_f32(b.Ka), int(b.q_bit)) for b in readers}) != 1:
                continue   # one code tensor serves every reader
            readers_of[blk] = tuple(readers)
        tr.release()
    n_in = n_trunk = 0
    for blk in blocks:
        rec = {"in_block": {}, "trunk": None}
        for bn_name, conv_name in (("bn1", "conv2"), ("bn2", "conv3")) if in_block else ():
            bn, conv = blk._modules.get(bn_name), blk._modules.get(conv_name)
            if (isinstance(bn, TrainBatchNorm2d) and not bn._relu and bn._trunk is None and bn.momentum is not None
                    and _is_conv_q(conv) and _link_conv_clean(conv)
                    and len(_slots_of(model, bn)) == 1 and len(_slots_of(model, conv)) == 1):
                wrap = TrainBatchNormCodes2d(bn, None, conv, min_elements)
                wrap.__dict__["_in_bottleneck"] = True
                rec["in_block"][bn_name] = blk._modules[bn_name] = wrap
        if blk in readers_of:
            bn3 = blk._modules["bn3"]
            ka, q_bit = _f32(readers_of[blk][0].Ka), int(readers_of[blk][0].q_bit)
            bn3._trunk = (readers_of[blk], ka, q_bit, min_elements)
            rec["trunk"] = bn3
        if not rec["in_block"] and rec["trunk"] is None:
            continue
        blk.__dict__["_bn_bottleneck_codes"] = rec
        n_in += len(rec["in_block"])
        n_trunk += rec["trunk"] is not None
    return n_in, n_trunk


def unlink_bottleneck_codes_train(model):
    """Undo link_bottleneck_codes_train: the linked slots get their TrainBatchNorm2d back (pointed at the current parameters,
    buffers and training flag), the bn3 wrappers forget their readers; the blocks keep use_device_bottleneck_train's forward.
    Returns (in_block_links, trunk_links) undone."""
    n = t = 0
    for blk in list(model.modules()):
        a, b = _unlink_bottleneck_codes(blk)
        n, t = n + a, t + b
    return n, t


# The last statement here, as the re-export of this module's names is in fusion.py: whichever is imported first, the other finds
# every name it asks for defined.  All of these are read inside functions only.
from .fusion import (   # noqa: E402
    _BOTTLENECK_CHILDREN, FoldedReLU, _Trace, _is_conv_q, _is_layerout, _restore_slots, _slots_of, _verified)
