"""Shared by test_bn_lut_codes_train_host.py and test_gpu_bn_lut_codes_train.py: small stacks of the blocks
[Conv2d_Q, BatchNorm2d, layerout_quantize_func, Swish | GELU] in the shapes of nets_cifar/mobilenetv1.py:176-250 (MobileNetV1_swish)
and nets_cifar/vgg16.py:186-293 (VGG16_gelu, with its MaxPool2d between stages), built on the CPU, and a checker of the module tree
for fusion.link_layerout_codes_train."""
import torch
import torch.nn as nn

from cnns_slfp_quantization_amd import activation_func as af, fusion, layer_specs
from cnns_slfp_quantization_amd import conv2d_func as cf
from cnns_slfp_quantization_amd.sfp_quant import layerout_quantize_func

_MB = layer_specs.conv_layers("mobilenetv1_imagenet224")   # the reference's Ka / Kw pattern: stem, then (dw, pw) pairs
MOBILENET_LINKS, VGG_LINKS = 4, 2


def _q(spec, c_in, c_out, k, stride, pad, groups=1, q_bit=8):
    return cf.conv2d_Q(q_bit, spec.Kw, spec.Ka)(c_in, c_out, k, stride=stride, padding=pad, groups=groups, bias=False)


def _tail(c, act, q_bit):
    return [nn.BatchNorm2d(c), layerout_quantize_func(q_bit), act()]


def mobilenet_swish_stack(q_bit=8, act=af.Swish):
    """conv_bn(3 -> 32), conv_dw(32 -> 64, stride 1), conv_dw(64 -> 64, stride 2) as nested nn.Sequentials, every BatchNorm followed
    by the layer-output quantizer and Swish, and a 10-class head: five BatchNorms, the first four in front of a Conv2d_Q."""
    def conv_dw(i, inp, oup, s):
        return nn.Sequential(_q(_MB[i], inp, inp, 3, s, 1, inp, q_bit), *_tail(inp, act, q_bit),
                             _q(_MB[i + 1], inp, oup, 1, 1, 0, 1, q_bit), *_tail(oup, act, q_bit))
    torch.manual_seed(4)
    body = nn.Sequential(nn.Sequential(_q(_MB[0], 3, 32, 3, 1, 1, 1, q_bit), *_tail(32, act, q_bit)),
                         conv_dw(1, 32, 64, 1), conv_dw(3, 64, 64, 2))
    return spread(nn.Sequential(body, nn.AdaptiveAvgPool2d(1), nn.Flatten(), cf.linear_Q(q_bit, 0.05, 0.3)(64, 10)))


def vgg_gelu_stack():
    """Two stages of [3x3 conv, BN, layerout, GELU] x 2 + MaxPool2d with scaled-bias convs, and a 10-class head: four BatchNorms, the
    first of each stage in front of a Conv2d_Q, the second in front of the pool."""
    Conv = cf.conv2d_Q_bias(8, 0.06, 0.17)
    torch.manual_seed(6)

    def block(c_in, c_out):
        return [Conv(c_in, c_out, 3, padding=1), *_tail(c_out, nn.GELU, 8)]

    m = nn.Sequential(*block(3, 16), *block(16, 16), nn.MaxPool2d(2, 2), *block(16, 32), *block(32, 32), nn.MaxPool2d(2, 2),
                      nn.AdaptiveAvgPool2d(1), nn.Flatten(), cf.linear_Q(8, 0.05, 0.3)(32, 10))
    return spread(m)


def spread(m):
    """BatchNorm parameters and statistics off their initial values."""
    g = torch.Generator().manual_seed(17)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                c = mod.num_features
                mod.weight.copy_(torch.rand(c, generator=g) + 0.5)
                mod.bias.copy_(torch.randn(c, generator=g) * 0.3)
                mod.running_mean.copy_(torch.randn(c, generator=g) * 0.2)
                mod.running_var.copy_(torch.rand(c, generator=g) + 0.5)
    return m


def convs(m):
    return [c for c in m.modules() if fusion._is_conv_q(c)]


def _leaves(m):
    """The leaf modules in the order they run (nested nn.Sequentials flattened)."""
    for kid in m._modules.values():
        if isinstance(kid, nn.Sequential):
            yield from _leaves(kid)
        else:
            yield kid


def intact(model):
    """None, or the first violation: a code-writing wrapper (TrainBatchNormLayeroutCodes2d) stands directly in front of two
    placeholders for ITS quantizer and activation and of ITS Conv2d_Q -- never in front of a stock module, which would be handed
    uint8 --, and every placeholder stands behind the wrapper of the pass that owns it."""
    leaves = list(_leaves(model))
    for i, kid in enumerate(leaves):
        if isinstance(kid, fusion.TrainBatchNormLayeroutCodes2d):
            nxt = leaves[i + 1:i + 4]
            if len(nxt) < 3 or not all(isinstance(t, fusion.FoldedTail) for t in nxt[:2]):
                return f"a code-writing wrapper in front of {[type(t).__name__ for t in nxt[:2]]}"
            if nxt[0].mod is not kid._layerout or nxt[1].mod is not kid._acts[0] or nxt[2] is not kid._conv:
                return "a code-writing wrapper in front of placeholders or a conv that are not its own"
            lut = isinstance(kid._held[0], fusion.TrainBatchNormLayerout2d)
            if [t.owner for t in nxt[:2]] != ["bn_layerout_train" if lut else "layerout_codes_train"] * 2:
                return f"placeholders of {[t.owner for t in nxt[:2]]} behind a wrapper that holds {type(kid._held[0]).__name__}"
        elif isinstance(kid, fusion.FoldedTail):
            front = [w for w in leaves[max(i - 2, 0):i] if not isinstance(w, fusion.FoldedTail)]
            w = front[-1] if front else None
            if kid.owner == "layerout_codes_train":
                ok = isinstance(w, fusion.TrainBatchNormLayeroutCodes2d) and kid.mod in (w._layerout, *w._acts)
            else:
                ok = (isinstance(w, fusion.TrainBatchNormLayerout2d) and kid.mod in (w._layerout, *w._acts)) or (
                    isinstance(w, fusion.TrainBatchNormLayeroutCodes2d) and isinstance(w._held[0], fusion.TrainBatchNormLayerout2d)
                    and kid in w._held[1:])
            if not ok:
                return f"FoldedTail({type(kid.mod).__name__}, {kid.owner}) behind {type(w).__name__}"
        elif isinstance(kid, fusion.TrainBatchNormLayerout2d):
            if not all(isinstance(t, fusion.FoldedTail) and t.owner == "bn_layerout_train" for t in leaves[i + 1:i + 3]):
                return "TrainBatchNormLayerout2d without its two FoldedTails"
    return None
