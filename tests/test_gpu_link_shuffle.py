"""MI355X: fusion.link_shuffle_units on a two-stage ShuffleNetV2-shaped net built from the project's own unit
(tests/golden/netgen_r3.py): 24 -> 116 -> 232 channels, one stride-2 and two stride-1 units per stage, 16 x 16 pixels, batch 2.  The
linked net must reproduce the unlinked one bit for bit, hand codes over inside every residual branch, and come back on unlink."""
import math
import os
import sys

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_linked_units_equal_the_unlinked_net_and_hand_over_codes():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import netgen_r3 as ng
    import utils.conv2d_func as cf
    import utils.sfp_quant as sq
    from cnns_slfp_quantization_amd import fusion
    dev = torch.device("cuda:0")

    class Factories(ng.Factories):   # Ka for activations of order one, Kw so that three sigma of the He-like weights reach the top class
        def conv(self, name, cin, cout, k, stride=1, pad=0, groups=1):
            self.m[name] = (0.25, 3.0 * math.sqrt(2.0 / (cin // groups * k * k)) / 15.0)
            return super().conv(name, cin, cout, k, stride, pad, groups)

    f = Factories(cf, 7, {}, layerout=sq.layerout_quantize_func)
    units = [ng._ShuffleUnit(f, "s2.0", 24, 116, 2), ng._ShuffleUnit(f, "s2.1", 116, 116, 1), ng._ShuffleUnit(f, "s2.2", 116, 116, 1),
             ng._ShuffleUnit(f, "s3.0", 116, 232, 2), ng._ShuffleUnit(f, "s3.1", 232, 232, 1), ng._ShuffleUnit(f, "s3.2", 232, 232, 1)]
    net = ng.fill_parameters_by_name(nn.Sequential(*units), 77).to(dev).eval().to(memory_format=torch.channels_last)
    x = torch.randn((2, 24, 16, 16), generator=torch.Generator().manual_seed(5)).to(dev).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        assert fusion.fuse_bn_relu(net) == 6 * 3 + 2 * 2
        keys = list(net.state_dict().keys())
        want = net(x)
        assert torch.isfinite(want).all() and len(torch.unique(want)) > 64
        assert fusion.link_shuffle_units(net, x.contiguous()) == 0            # NCHW-contiguous: refused
        assert fusion.link_shuffle_units(net, x) == 6
        got = net(x)
        assert torch.equal(got, want) and got.is_contiguous(memory_format=torch.channels_last)
        for u in units:
            c = u.residual[6].in_channels
            for h in u._shuffle_handover:                                     # the two hand-overs of the branch: uint8 at pitch P
                assert h.dtype == torch.uint8 and h.shape[1] == (c + 31) // 32 * 32 and h.is_contiguous(memory_format=torch.channels_last)
            assert u.residual[0]._last_kernel == "pwr_entry+lut" and u.residual[6]._last_kernel == "pwr_exit+pass"
            assert u.residual[6].input_q.shape[1] == c
        assert list(net.state_dict().keys()) == keys
        assert fusion.unlink_codes(net) == 6
        assert all("forward" not in u.__dict__ for u in units)
        assert torch.equal(net(x), want)
        assert units[1].residual[0]._last_kernel != "pwr_entry+lut"
