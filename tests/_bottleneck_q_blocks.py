"""Shared by test_gpu_bn_res_codes_train.py and test_bn_res_codes_train_host.py: _bn_res_blocks.Bottleneck on Conv2d_Q with the
scales of layer_specs' resnet50 rows, and the stack the pass is tested on.
  block A   16 -> 8 -> 8 -> 32, conv2 and the downsample of stride 2 (conv1 and downsample.0 share Ka, as in the net)
  block B   32 -> 8 -> 8 -> 32, plain: conv1 is the one reader of A's trunk
  block C   32 -> 8 -> 8 -> 32 with a downsample whose Ka differs from its conv1's: B's trunk has two readers of two scales
  then the three look-alikes of _bn_res_blocks (plain nn.Conv2d; same child names, another dataflow): C's trunk has no Conv2d_Q reader
Everything here is device-agnostic.  host=True builds the convs from a subclass that computes with stock ATen (q_bit 32) whatever
q_bit says, so that a pass which asks for q_bit 8 can be run on a model that lives on the CPU."""
import torch
import torch.nn as nn

import _bn_res_blocks as R
from cnns_slfp_quantization_amd import conv2d_func as cf
from cnns_slfp_quantization_amd import fusion, layer_specs

ROWS = layer_specs.conv_layers("resnet50_imagenet224")   # 1..4: layer1.0 (conv1..3, downsample.0), 5..7, 8..10, 11..14: layer2.0
GENUINE = 3


def conv_q(row, c_in, c_out, k, stride=1, pad=0, q_bit=8, host=False, ka=None):
    spec = ROWS[row]
    cls = cf.conv2d_Q(q_bit, spec.Kw, spec.Ka if ka is None else ka)
    if host:
        class HostConv(cls):
            def forward(self, input, order=None, **kw):
                keep, self.q_bit = self.q_bit, 32
                try:
                    return super().forward(input, order, **kw)
                finally:
                    self.q_bit = keep
        cls = HostConv
    return cls(c_in, c_out, k, stride=stride, padding=pad, bias=False)


class QBottleneck(R.Bottleneck):
    """_bn_res_blocks.Bottleneck (torchvision's forward) with Conv2d_Q in the four conv slots; rows = the layer_specs rows of conv1,
    conv2, conv3 and downsample.0."""

    def __init__(self, cin, mid, cout, rows, stride=1, downsample=False, q_bit=8, host=False):
        super().__init__(cin, mid, cout, downsample=downsample)
        kw = dict(q_bit=q_bit, host=host)
        self.conv1 = conv_q(rows[0], cin, mid, 1, **kw)
        self.conv2 = conv_q(rows[1], mid, mid, 3, stride, 1, **kw)
        self.conv3 = conv_q(rows[2], mid, cout, 1, **kw)
        if downsample:
            self.downsample = nn.Sequential(conv_q(rows[3], cin, cout, 1, stride, **kw), nn.BatchNorm2d(cout))


def stack(q_bit=8, host=False, seed=3, mid=8):
    """mid: the blocks' inner width.  8 is the stack as described above; libslfp_hip has no code-reading forward for a layer of
    8 input channels, so there the in-block links fall back call by call (conv2 and conv3 read float32) and only the trunk runs on
    codes.  16 is the smallest width at which conv2 and conv3 read codes too."""
    torch.manual_seed(seed)
    assert ROWS[1].Ka == ROWS[4].Ka and ROWS[8].Ka != ROWS[14].Ka
    kw = dict(q_bit=q_bit, host=host)
    m = nn.Sequential(QBottleneck(16, mid, 32, (1, 12, 3, 4), stride=2, downsample=True, **kw),
                      QBottleneck(32, mid, 32, (5, 6, 7), **kw),
                      QBottleneck(32, mid, 32, (8, 9, 10, 14), downsample=True, **kw),
                      *(cls(32, 8, 32) for cls in R.LOOKALIKES))
    return R.randomize(m)


def convs(m):
    return [c for c in m.modules() if fusion._is_conv_q(c)]


def expected_links(m):
    """(in_block, trunk) computed from the stack: two in-block pairs per genuine block; a trunk link where every Conv2d_Q that reads
    a genuine block's output shares one (Ka, q_bit)."""
    blocks = list(m)[:GENUINE]
    trunk = 0
    for blk, nxt in zip(blocks, list(m)[1:GENUINE + 1]):
        readers = [c for c in (getattr(nxt, "conv1", None), nxt.downsample[0] if getattr(nxt, "downsample", None) is not None else None)
                   if c is not None and fusion._is_conv_q(c)]
        if readers and len({(cf._f32(c.Ka), c.q_bit) for c in readers}) == 1:
            trunk += 1
    return 2 * len(blocks), trunk
