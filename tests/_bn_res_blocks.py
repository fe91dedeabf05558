"""Shared by test_bn_res_train_host.py and test_gpu_bn_res_train.py: hand-wired Bottlenecks with torchvision's Bottleneck.forward,
the dataflow the training nets use (one shared nn.ReLU(), `out += identity`), on plain float32 nn.Conv2d, and look-alikes that
carry the same child names but compute something else.  Everything here is device-agnostic."""
import torch
import torch.nn as nn


class Bottleneck(nn.Module):
    def __init__(self, cin, mid, cout, downsample=False):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, mid, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(mid)
        self.conv2 = nn.Conv2d(mid, mid, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(mid)
        self.conv3 = nn.Conv2d(mid, cout, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(cout)
        self.relu = nn.ReLU()
        self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, bias=False), nn.BatchNorm2d(cout)) if downsample else None

    def forward(self, x):
        identity = x

        out = self.conv1(x)
        out = self.bn1(out)
        out = self.relu(out)

        out = self.conv2(out)
        out = self.bn2(out)
        out = self.relu(out)

        out = self.conv3(out)
        out = self.bn3(out)

        if self.downsample is not None:
            identity = self.downsample(x)

        out += identity
        out = self.relu(out)

        return out


class ScaledIdentity(Bottleneck):
    """The identity enters the add twice."""

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        out = out + 2.0 * x
        return self.relu(out)


class ReluBeforeAdd(Bottleneck):
    """A ReLU in front of the add."""

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = torch.relu(self.bn3(self.conv3(out)))
        out = out + x
        return self.relu(out)


class SkipsBn3(Bottleneck):
    """bn3 is a child but does not run."""

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.conv3(out)
        out = out + x
        return self.relu(out)


LOOKALIKES = (ScaledIdentity, ReluBeforeAdd, SkipsBn3)


def stack(seed=3):
    """Block A 16 -> 8 -> 8 -> 32 with a 1x1 downsample conv + BN, block B 32 -> 8 -> 8 -> 32 plain; the running statistics and
    the affine parameters are moved off their initial values so that an eval-mode forward tells the channels apart."""
    torch.manual_seed(seed)
    m = nn.Sequential(Bottleneck(16, 8, 32, downsample=True), Bottleneck(32, 8, 8 * 4))
    return randomize(m)


def mixed(seed=5):
    """A genuine plain block between the three look-alikes (32 channels throughout)."""
    torch.manual_seed(seed)
    m = nn.Sequential(ScaledIdentity(32, 8, 32), Bottleneck(32, 8, 32), ReluBeforeAdd(32, 8, 32), SkipsBn3(32, 8, 32))
    return randomize(m)


def randomize(m):
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


def example(seed=9):
    """4 x 16 x 9 x 7, channels_last."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(4, 16, 9, 7, generator=g).contiguous(memory_format=torch.channels_last)


def example32(seed=9):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(4, 32, 9, 7, generator=g).contiguous(memory_format=torch.channels_last)
