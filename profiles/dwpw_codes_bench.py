#!/usr/bin/env python3
"""The depthwise -> pointwise block as ONE kernel on 1-byte codes (csrc/conv_dwpw_codes.hip, slfp_dwpw_fwd_codes) against the two
code kernels it replaces (k_dwc then k_pwc_*), on the MI355X.  Writes profiles/dwpw_codes_bench.json (--out: elsewhere).

  pairs      MobileNetV1-224's first four blocks (32@112 -> 64, 64@112 s2 -> 128, 128@56 -> 128, 128@56 s2 -> 256) at batch 128 and
             256, codes in and codes out as inside the linked net.  Leg A = the two Conv2d_Q modules of the linked pair (today's
             path), leg B = fusion.DwPwBlock over the same two modules under options.dwpw_all: the same weights, the same input
             codes, outputs compared byte for byte before anything is timed.
  whole_net  the fixture-shaped MobileNetV1 of bench.py (27 convs, folded BatchNorm / ReLU, pool, classifier), fuse_bn_relu ->
             link_codes; leg A = that net (the parent's two-kernel code path), leg B = the same net after fuse_dw_pw under
             options.dwpw_all (blocks 1-4 as one kernel each; the K >= 256 blocks stay two kernels).

One process.  Every leg is warmed up, then ROUNDS rounds alternate A and B; a round times a window of back-to-back calls between two
device events (steady state: no flush between calls; the tensors of these layers are 26-205 MB).  Reported: the median over the
rounds of each leg, and each leg's own minimum and maximum beside it -- a difference inside leg A's spread is no difference."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import utils.conv2d_func as cf  # noqa: E402
from cnns_slfp_quantization_amd import fusion, layer_specs  # noqa: E402
from cnns_slfp_quantization_amd.sfp_quant import hip_encode  # noqa: E402
from cnns_slfp_quantization_amd import _lib  # noqa: E402

ROUNDS = 7


def window_us(fn, calls):
    """microseconds per call of `calls` back-to-back calls of fn, between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def alternate(leg_a, leg_b, calls, warmup=5):
    ta, tb = [], []
    for _ in range(warmup):
        leg_a()
        leg_b()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        ta.append(window_us(leg_a, calls))
        tb.append(window_us(leg_b, calls))
    return ta, tb


def stats(ts, digits=1):
    return {"median": round(float(np.median(ts)), digits), "min": round(float(min(ts)), digits), "max": round(float(max(ts)), digits)}


def conv(s):
    return cf.conv2d_Q(q_bit=8, Kw=np.float64(s.Kw), Ka=np.float64(s.Ka))(
        s.c_in, s.c_out, s.k[0], np.float64(s.Kw), np.float64(s.Ka), s.stride[0], s.pad[0], groups=s.groups, bias=False)


def randomize_bn(model, g):
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_var.uniform_(0.5, 1.5, generator=g)
                m.weight.uniform_(0.8, 1.6, generator=g)
                m.bias.normal_(0.1, 0.1, generator=g)


def bench_pairs(specs, dev, batches, calls):
    rows = []
    g = torch.Generator(device=dev).manual_seed(3)
    for bi in range(4):
        sd, sp, sn = specs[1 + 2 * bi], specs[2 + 2 * bi], specs[3 + 2 * bi]
        two = nn.Sequential(conv(sd), nn.BatchNorm2d(sd.c_out), nn.ReLU(), conv(sp), nn.BatchNorm2d(sp.c_out), nn.ReLU()).to(dev).eval()
        randomize_bn(two, g)
        two = two.to(memory_format=torch.channels_last)
        fusion.fuse_bn_relu(two)
        assert fusion.link_codes(two) == 1                          # the depthwise conv writes the pointwise conv's codes
        dw, pw = two[0], two[3]
        pw._code_out = (float(np.float64(sn.Ka)), 8)                # ... which writes the next block's, as inside the net
        one = fusion.DwPwBlock(dw, pw).eval()
        for batch in batches:
            x = (torch.randn((batch, sd.c_in, sd.h, sd.w), generator=g, device=dev).abs() * 4 * sd.Ka).contiguous(memory_format=torch.channels_last)
            xc = hip_encode(x, float(sd.Ka), _lib.FMT_ACT8)
            del x
            with torch.no_grad():
                cf.options.dwpw_all = True
                y_two = two(xc)
                y_one = one(xc)
                names = (dw._last_kernel, pw._last_kernel, one._last_kernel)   # the block leaves its convs' records alone
                assert names[0].startswith("dw3x3") and names[1].startswith("pw_mfma") and all("+codes_in" in n for n in names[:2]), names
                assert names[2] and names[2].startswith("dwpw_fused_") and "+codes_in" in names[2], names
                same = bool(y_two.dtype == torch.uint8 and torch.equal(y_two, y_one))
                ta, tb = alternate(lambda: two(xc), lambda: one(xc), calls)
            a, b = stats(ta), stats(tb)
            rows.append({"pair": f"{sd.c_in}@{sd.h} s{sd.stride[0]} -> {sp.c_out}", "batch": batch, "calls_per_window": calls, "rounds": ROUNDS,
                         "two_kernels_us": a, "one_kernel_us": b, "one_over_two": round(b["median"] / a["median"], 3),
                         "bit_identical": same, "kernels_two": list(names[:2]), "kernel_one": names[2]})
            print(rows[-1], flush=True)
            del xc, y_two, y_one
        cf.options.dwpw_all = False
    return rows


def bench_net(specs, dev, batches, steps):
    layers = []
    for s in specs:
        layers += [conv(s), nn.BatchNorm2d(s.c_out), nn.ReLU(inplace=True)]
    model = nn.Sequential(*layers, nn.AvgPool2d(7), nn.Flatten(), nn.Linear(1024, 1000)).to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(3)
    randomize_bn(model, g)
    model = model.to(memory_format=torch.channels_last)
    rows = []
    with torch.no_grad():
        fusion.fuse_bn_relu(model)
        for batch in batches:
            x = torch.randn((batch, 3, 224, 224), device=dev, generator=g).contiguous(memory_format=torch.channels_last)
            links = fusion.link_codes(model, example_input=x)
            y_two = model(x).clone()

            def leg(one_kernel):
                cf.options.dwpw_all = one_kernel
                (fusion.fuse_dw_pw if one_kernel else fusion.unfuse_dw_pw)(model)
                return model

            y_one = leg(True)(x).clone()
            blocks = [m for m in model.modules() if isinstance(m, fusion.DwPwBlock)]
            n_one = sum(1 for b in blocks if b._last_kernel and "+codes_in" in b._last_kernel)
            same = bool(torch.equal(y_one, y_two))
            ta, tb = [], []
            for r in range(ROUNDS + 1):   # round 0 is the warm-up of both legs
                for one_kernel, ts in ((False, ta), (True, tb)):
                    m = leg(one_kernel)
                    m(x)
                    t = window_us(lambda: m(x), steps)
                    if r:
                        ts.append(batch / t * 1e6)
            leg(False)
            fusion.unlink_codes(model)
            rows.append({"batch": batch, "steps_per_window": steps, "rounds": ROUNDS, "code_links": links, "blocks_one_kernel": n_one,
                         "linked_two_kernels_img_s": stats(ta, 0), "linked_dwpw_all_img_s": stats(tb, 0),
                         "one_over_two": round(float(np.median(tb) / np.median(ta)), 3), "bit_identical": same})
            print(rows[-1], flush=True)
            del x
    cf.options.dwpw_all = False
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dwpw_codes_bench.json"))
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    dev = torch.device("cuda", 0)
    specs = layer_specs.conv_layers("mobilenetv1_imagenet224")
    res = {"device": torch.cuda.get_device_name(0), "method": __doc__.split("\n\n")[-1].replace("\n", " "),
           "pairs": bench_pairs(specs, dev, a.batches, a.calls), "whole_net": bench_net(specs, dev, a.batches, a.steps)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
