#!/usr/bin/env python3
"""The two layer-output-quantized nets of the reference -- MobileNetV1_swish (nets_cifar/mobilenetv1.py:176-250) and VGG16_gelu
(nets_cifar/vgg16.py:186-293) -- as nets of the same shape at 32 x 32, batch 256: fuse_bn_relu alone against fuse_bn_relu +
fusion.link_layerout.

    python profiles/layerout_bench.py [--batch 256] [--out profiles/layerout_bench.json]

The nets are built from the packaged layer tables (cnns_slfp_quantization_amd/data/layer_specs.json: geometry and calibration scales
of mobilenetv1_cifar32 and vgg16_224, the latter run at 32 x 32 with its five 2 x 2 pools); every block is [Conv2d_Q, BatchNorm2d,
layerout_quantize_func, activation] with Swish on the last four depthwise-separable blocks of the MobileNet and nn.GELU() on every
VGG block; weights and BatchNorm statistics are random.  Leg A: fuse_bn_relu.  Leg B: A + link_layerout.  The legs alternate five
times in one process; a leg is 30 forwards after 5 warm-up forwards, timed with HIP events.  The logits of the two legs are
torch.equal."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import utils.conv2d_func as cf  # noqa: E402
from utils.activation_func import Swish  # noqa: E402
from utils.sfp_quant import layerout_quantize_func  # noqa: E402
from cnns_slfp_quantization_amd import fusion, layer_specs  # noqa: E402

ROUNDS, STEPS, WARMUP, Q = 5, 30, 5, 8


def _block(s, act):
    conv = cf.conv2d_Q(q_bit=Q, Kw=s.Kw, Ka=s.Ka)(s.c_in, s.c_out, s.k[0], s.Kw, s.Ka, s.stride[0], s.pad[0], groups=s.groups, bias=False)
    return [conv, nn.BatchNorm2d(s.c_out), layerout_quantize_func(q_bit=Q), act]


def mobilenet_swish():
    specs = layer_specs.conv_layers("mobilenetv1_cifar32")
    assert len(specs) == 27
    mods = []
    for i, s in enumerate(specs):
        mods += _block(s, Swish() if i >= 19 else nn.ReLU())     # conv_dw_swish: the last four blocks = eight convs
    return nn.Sequential(*mods, nn.AdaptiveAvgPool2d(1), nn.Flatten(), cf.linear_Q(q_bit=Q, Kw=0.05, Ka=0.6)(1024, 100))


def vgg_gelu():
    specs = layer_specs.conv_layers("vgg16_224")
    assert len(specs) == 13
    mods = []
    for i, s in enumerate(specs):
        mods += _block(s, nn.GELU())
        if i in (1, 3, 6, 9, 12):
            mods.append(nn.MaxPool2d(2, 2))
    return nn.Sequential(*mods, nn.Flatten(), cf.linear_Q(q_bit=Q, Kw=0.05, Ka=0.6)(512, 100))


def prepare(make, dev, seed):
    torch.manual_seed(seed)   # the Linear_Q head draws from the global generator
    m = make()
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.running_mean.copy_(torch.randn(mod.num_features, generator=gen) * 0.05)
                mod.running_var.copy_(0.5 + torch.rand(mod.num_features, generator=gen))
                mod.weight.copy_(0.5 + torch.rand(mod.num_features, generator=gen))
                mod.bias.copy_(torch.randn(mod.num_features, generator=gen) * 0.2)
            elif isinstance(mod, nn.Conv2d):
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=gen) * (2.0 / mod.weight[0].numel()) ** 0.5)
    return m.to(dev).eval().to(memory_format=torch.channels_last)


def timed(fn, steps=STEPS, warmup=WARMUP):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def run_net(name, make, dev, batch):
    ma, mb = prepare(make, dev, 5), prepare(make, dev, 5)
    x = torch.randn(batch, 3, 32, 32, generator=torch.Generator().manual_seed(6)).to(dev).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        fused = [fusion.fuse_bn_relu(m) for m in (ma, mb)]
        ya = ma(x)
        assert torch.equal(mb(x), ya), "the two legs are not the same net"
        links = fusion.link_layerout(mb, x)
        same = bool(torch.equal(mb(x), ya))
        legs = {"A": [], "B": []}
        for _ in range(ROUNDS):
            legs["A"].append(timed(lambda: ma(x)))
            legs["B"].append(timed(lambda: mb(x)))
    med = {k: statistics.median(v) for k, v in legs.items()}
    convs = [c for c in mb.modules() if fusion._is_conv_q(c)]
    return {"net": name, "batch": batch, "convs": len(convs), "fused": fused[0], "links": links, "logits_bit_identical": same,
            "leg_A_ms": [round(v, 4) for v in legs["A"]], "leg_B_ms": [round(v, 4) for v in legs["B"]],
            "leg_A_median_ms": round(med["A"], 4), "leg_B_median_ms": round(med["B"], 4),
            "leg_A_spread_ms": round(max(legs["A"]) - min(legs["A"]), 4), "speedup": round(med["A"] / med["B"], 4),
            "images_per_s_A": round(batch / med["A"] * 1e3, 1), "images_per_s_B": round(batch / med["B"] * 1e3, 1),
            "kernels_B": [c._last_kernel for c in convs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layerout_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "input": "32 x 32, channels_last", "q_bit": Q,
           "protocol": f"A/B alternated {ROUNDS}x in one process, {STEPS} forwards per leg after {WARMUP} warm-up, HIP events",
           "leg_A": "fuse_bn_relu", "leg_B": "leg A + link_layerout",
           "results": [run_net("MobileNetV1_swish-shaped", mobilenet_swish, dev, args.batch),
                       run_net("VGG16_gelu-shaped", vgg_gelu, dev, args.batch)]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for r in res["results"]:
        print(json.dumps({k: v for k, v in r.items() if k != "kernels_B"}))


if __name__ == "__main__":
    main()
