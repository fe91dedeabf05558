"""MI355X: fusion.link_layerout on two small nn.Sequential nets built from the blocks of MobileNetV1_swish
(nets_cifar/mobilenetv1.py:196-231) and VGG16_gelu (nets_cifar/vgg16.py:186-293): [Conv2d_Q, BatchNorm2d, layerout_quantize_func,
ReLU | Swish | GELU].  After fuse_bn_relu the pass links every conv -> conv hand-over through a byte table; the logits stay
torch.equal, every linked hand-over is uint8, unlink_codes restores every module slot, link_codes still makes no link, and a model
that uses a hand-over tensor functionally (a torch.cat in a custom forward) is rolled back."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
Q = 8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _mods():
    import utils.conv2d_func as cf
    from utils.activation_func import Swish
    from utils.sfp_quant import layerout_quantize_func
    return cf, Swish, layerout_quantize_func


def _conv(cin, cout, k, ka, stride=1, pad=0, groups=1):
    cf = _mods()[0]
    return cf.conv2d_Q(q_bit=Q, Kw=0.03, Ka=ka)(cin, cout, k, 0.03, ka, stride, pad, groups=groups, bias=False)


def _block(conv, act):
    lo = _mods()[2]
    return [conv, nn.BatchNorm2d(conv.out_channels), lo(q_bit=Q), act]


def _net1():
    """stem 3 -> 32 s2, conv_dw (ReLU) 32 -> 64, conv_dw_swish 64 -> 128 s2, conv_dw_swish 128 -> 128, pool, Linear_Q: 7 convs"""
    cf, Swish, _ = _mods()
    kas = iter([0.17, 0.33, 0.29, 0.27, 0.21, 0.19, 0.23])

    def conv_dw(cin, cout, stride, act):
        return nn.Sequential(*_block(_conv(cin, cin, 3, next(kas), stride, 1, groups=cin), act()),
                             *_block(_conv(cin, cout, 1, next(kas)), act()))

    return nn.Sequential(nn.Sequential(*_block(_conv(3, 32, 3, next(kas), 2, 1), nn.ReLU())),
                         conv_dw(32, 64, 1, nn.ReLU), conv_dw(64, 128, 2, Swish), conv_dw(128, 128, 1, Swish),
                         nn.AdaptiveAvgPool2d(1), nn.Flatten(), cf.linear_Q(q_bit=Q, Kw=0.05, Ka=0.2)(128, 10))


def _net2():
    """3 -> 64, 64 -> 64, MaxPool, 64 -> 128, 128 -> 128, MaxPool, flatten, Linear_Q: 3x3 convs with BN + layerout + nn.GELU()"""
    cf = _mods()[0]
    kas = iter([0.17, 0.12, 0.1, 0.09])

    def c(cin, cout):
        return _block(_conv(cin, cout, 3, next(kas), 1, 1), nn.GELU())

    return nn.Sequential(*c(3, 64), *c(64, 64), nn.MaxPool2d(2), *c(64, 128), *c(128, 128), nn.MaxPool2d(2), nn.Flatten(),
                         cf.linear_Q(q_bit=Q, Kw=0.05, Ka=0.2)(128 * 4 * 4, 10))


class _HiddenCat(nn.Module):
    """the stem's output also goes through a torch.cat that no module hook sees"""

    def __init__(self):
        super().__init__()
        cf = _mods()[0]
        self.stem = nn.Sequential(*_block(_conv(3, 32, 3, 0.17, 2, 1), nn.ReLU()))
        self.block = nn.Sequential(*_block(_conv(32, 32, 3, 0.33, 1, 1, groups=32), nn.ReLU()), *_block(_conv(32, 64, 1, 0.29), nn.ReLU()))
        self.fc = cf.linear_Q(q_bit=Q, Kw=0.05, Ka=0.2)(64 + 64, 10)

    def forward(self, x):
        h = self.stem(x)
        t = self.block(h)
        side = torch.cat([h, h], 1).float().mean((2, 3))
        return self.fc(torch.cat([t.float().mean((2, 3)), side], 1).contiguous())


def _prepare(m, dev, seed):
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.running_mean.copy_(torch.randn(mod.num_features, generator=gen) * 0.05)
                mod.running_var.copy_(0.2 + 0.5 * torch.rand(mod.num_features, generator=gen))
                mod.weight.copy_(0.5 + torch.rand(mod.num_features, generator=gen))
                mod.bias.copy_(torch.randn(mod.num_features, generator=gen) * 0.2)
            elif isinstance(mod, nn.Conv2d):
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=gen) * (2.0 / (mod.weight[0].numel())) ** 0.5)
    x = torch.randn(2, 3, 16, 16, generator=gen)
    m = m.to(dev).eval().to(memory_format=torch.channels_last)
    return m, x.to(dev).contiguous(memory_format=torch.channels_last)


def _slots(m):
    return [(name, id(mod)) for name, mod in m.named_modules()]


def _convs(m):
    from cnns_slfp_quantization_amd import fusion
    return [c for c in m.modules() if fusion._is_conv_q(c)]


@pytest.mark.parametrize("make,n_convs,n_links,n_acts,n_pools", [(_net1, 7, 6, 3, 0), (_net2, 4, 3, 3, 1)], ids=["mobilenet-swish", "vgg-gelu"])
def test_link_layerout_on_a_small_net(dev, make, n_convs, n_links, n_acts, n_pools):
    from cnns_slfp_quantization_amd import fusion
    m, x = _prepare(make(), dev, 31)
    with torch.no_grad():
        assert fusion.fuse_bn_relu(m) == n_convs
        y_fused = m(x)
    assert torch.isfinite(y_fused).all() and y_fused.abs().max() > 0
    convs = _convs(m)
    assert len(convs) == n_convs and all(int(c._post[2]) & 2 for c in convs)
    before = _slots(m)
    assert fusion.link_codes(m, x) == 0           # the threshold-table links refuse the layer-output quantizer
    assert _slots(m) == before and all(c._code_out is None for c in convs)

    assert fusion.link_layerout(m, x) == n_links
    linked = [c for c in convs if c._code_out is not None]
    assert linked == convs[:-1]
    for c in linked:
        assert c._code_lut is not None and c._code_lut.dtype == torch.uint8 and c._code_lut.is_cuda
        assert "_code_lut" not in c.state_dict()
    assert sum(isinstance(k, fusion.CodeAct) for k in m.modules()) == n_acts
    assert sum(isinstance(k, fusion.CodeMaxPool2d) for k in m.modules()) == n_pools
    seen = {}
    hooks = [c.register_forward_hook(lambda mod, inp, out: seen.__setitem__(mod, (inp[0].dtype, out.dtype))) for c in convs]
    with torch.no_grad():
        y_linked = m(x)
    for h in hooks:
        h.remove()
    assert torch.equal(y_linked, y_fused)
    assert seen[convs[0]] == (torch.float32, torch.uint8)
    for c in convs[1:-1]:
        assert seen[c] == (torch.uint8, torch.uint8), c._last_kernel
        assert c._last_kernel.endswith("+codes_in+codes_out+lut"), c._last_kernel
    assert seen[convs[-1]] == (torch.uint8, torch.float32)
    assert convs[-1]._last_kernel.endswith("+codes_in+layerout_pass"), convs[-1]._last_kernel   # the code kernel, then the quantizer
    assert convs[0]._last_kernel.endswith("+codes_out+lut")

    assert fusion.unlink_codes(m) == n_links
    assert _slots(m) == before and all(c._code_out is None and c._code_lut is None for c in convs)
    with torch.no_grad():
        assert torch.equal(m(x), y_fused)
    assert fusion.link_layerout(m, x) == n_links   # and again, from the restored state
    with torch.no_grad():
        assert torch.equal(m(x), y_fused)


def test_a_hidden_cat_is_rolled_back(dev):
    from cnns_slfp_quantization_amd import fusion
    m, x = _prepare(_HiddenCat(), dev, 47)
    with torch.no_grad():
        assert fusion.fuse_bn_relu(m) == 3
        y_fused = m(x)
    before = _slots(m)
    assert fusion.link_layerout(m, x) == 0
    assert _slots(m) == before
    assert all(c._code_out is None and c._code_lut is None for c in _convs(m))
    assert not any(isinstance(k, (fusion.CodeAct, fusion.CodeMaxPool2d)) for k in m.modules())
    with torch.no_grad():
        assert torch.equal(m(x), y_fused)
