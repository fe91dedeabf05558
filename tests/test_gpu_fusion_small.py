"""GPU (MI355X): one tiny hand-wired residual net through the whole fusion pipeline -- fuse_named_bn, fuse_residual,
link_codes_traced(entries=True), link_stem, link_trunk -- the smallest shape at which every shared helper of fusion.py (DESIGN
section 20: the trace, the predicates, the wrap records, the verifier) is on the path of a real link.

2x3x37x45 image -> 7x7 s2 p3 stem 3->32 -> BatchNorm -> in-place ReLU -> MaxPool2d(3, 2, 1) (10x12) -> Bottleneck A (32 -> 32 -> 32 -> 64,
a 1x1 downsample conv; conv1 and downsample.0 share Ka) -> Bottleneck B (64 -> 32 -> 32 -> 64) -> average pool -> nn.Linear.
The logits stay torch.equal after every pass, the passes return what they returned before the helpers were shared, each pass
runs the model as often as it did, and three orders of the undo functions all lead back to the state after fuse_named_bn."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

STATE = ("_code_out", "_code_entry", "_trunk_code_out", "residual_relu")
MARKERS = ("_in_residual", "_pre_link_post", "_stem_link", "_trunk_link", "_fire_fused", "_residual_fused", "_named_bn",
           "_fused_modules", "_dw_slot", "forward")


def _net(q_bit, dev):
    import utils.conv2d_func as cf

    def C(cin, cout, k, ka, stride=1, pad=0):
        return cf.conv2d_Q(q_bit=q_bit, Kw=0.02, Ka=ka)(cin, cout, k, 0.02, ka, stride, pad)

    class Bottleneck(nn.Module):
        def __init__(self, cin, mid, cout, ka, down):
            super().__init__()
            self.conv1, self.bn1 = C(cin, mid, 1, ka[0]), nn.BatchNorm2d(mid)
            self.conv2, self.bn2 = C(mid, mid, 3, ka[1], 1, 1), nn.BatchNorm2d(mid)
            self.conv3, self.bn3 = C(mid, cout, 1, ka[2]), nn.BatchNorm2d(cout)
            self.relu = nn.ReLU(inplace=True)
            self.downsample = nn.Sequential(C(cin, cout, 1, ka[0])) if down else None

        def forward(self, x):
            out = self.relu(self.bn1(self.conv1(x)))
            out = self.relu(self.bn2(self.conv2(out)))
            out = self.bn3(self.conv3(out))
            out += x if self.downsample is None else self.downsample(x)
            return self.relu(out)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1, self.bn1 = C(3, 32, 7, 0.3, 2, 3), nn.BatchNorm2d(32)
            self.relu = nn.ReLU(inplace=True)
            self.maxpool = nn.MaxPool2d(3, 2, 1)
            self.layer1 = nn.Sequential(Bottleneck(32, 32, 64, (0.29, 0.27, 0.25), True),
                                        Bottleneck(64, 32, 64, (0.31, 0.26, 0.24), False))
            self.avgpool = nn.AdaptiveAvgPool2d(1)
            self.fc = nn.Linear(64, 10)

        def forward(self, x):
            x = self.layer1(self.maxpool(self.relu(self.bn1(self.conv1(x)))))
            return self.fc(torch.flatten(self.avgpool(x), 1))

    torch.manual_seed(20)
    m = Net()
    gen = torch.Generator().manual_seed(21)
    with torch.no_grad():
        for bn in [b for b in m.modules() if isinstance(b, nn.BatchNorm2d)]:
            bn.running_mean.copy_(torch.randn(bn.num_features, generator=gen) * 0.1)
            bn.running_var.copy_(0.5 + torch.rand(bn.num_features, generator=gen))
            bn.weight.copy_(0.5 + torch.rand(bn.num_features, generator=gen))
            bn.bias.copy_(torch.randn(bn.num_features, generator=gen) * 0.1)
    x = torch.randn(2, 3, 37, 45, generator=gen)
    m = m.to(dev).eval().to(memory_format=torch.channels_last)
    return m, x.to(dev).contiguous(memory_format=torch.channels_last)


def _snapshot(m):
    rows = []
    for name, mod in m.named_modules():
        post = mod.__dict__.get("_post")
        rows.append((name, id(mod), type(mod).__name__, None if post is None else (id(post[0]), id(post[1]), int(post[2])),
                     tuple(mod.__dict__.get(k) for k in STATE), tuple(k in mod.__dict__ for k in MARKERS)))
    return rows


@pytest.mark.parametrize("q_bit", [8, 7])
def test_the_whole_pipeline_on_a_tiny_residual_net(q_bit):
    from cnns_slfp_quantization_amd import fusion
    assert torch.cuda.is_available(), "these tests need the MI355X"
    m, x = _net(q_bit, torch.device("cuda:0"))
    forwards = []
    m.register_forward_hook(lambda mod, inp, out: forwards.append(1))

    def counted(fn, *a, **k):
        del forwards[:]
        return fn(m, *a, **k), len(forwards)

    passes = [(fusion.fuse_residual, {}), (fusion.link_codes_traced, {"entries": True}), (fusion.link_stem, {}), (fusion.link_trunk, {})]
    undo_orders = {
        "reverse": (fusion.unlink_trunk, fusion.unlink_stem, fusion.unlink_codes, fusion.unfuse_residual),
        "unlink_codes first": (fusion.unlink_codes, fusion.unlink_trunk, fusion.unlink_stem, fusion.unfuse_residual),
        "unfuse_residual first": (fusion.unfuse_residual, fusion.unlink_trunk, fusion.unlink_stem, fusion.unlink_codes),
    }
    with torch.no_grad():
        got = counted(fusion.fuse_named_bn, example_input=x)
        print("fuse_named_bn (pairs, forwards):", got)
        assert got == (7, 1)
        y0 = m(x)
        base = _snapshot(m)
        for order, undos in undo_orders.items():
            for (fn, kw), want in zip(passes, [(2, 2), (4, 2), (1, 2), (1, 2)]):
                got = counted(fn, x, **kw)
                print(f"{fn.__name__} (count, forwards):", got)
                assert got == want, (fn.__name__, got)
                assert torch.equal(m(x), y0), fn.__name__
            kernels = {n: c._last_kernel for n, c in m.named_modules() if hasattr(c, "_trunk_code_out")}
            assert kernels["conv1"].endswith("+codes_out") and kernels["layer1.0.downsample.0"].endswith("+codes_in")
            assert kernels["layer1.0.conv3"].endswith("+codes_in+res+trunk_codes") and kernels["layer1.1.conv3"].endswith("+codes_in+res")
            assert all("+codes_in" in kernels[f"layer1.{i}.conv{k}"] for i in (0, 1) for k in (1, 2, 3))
            assert _snapshot(m) != base
            for undo in undos:
                undo(m)
            assert _snapshot(m) == base, order
            assert torch.equal(m(x), y0), order
