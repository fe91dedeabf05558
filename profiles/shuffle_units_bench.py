#!/usr/bin/env python3
"""The stride-1 unit shapes of shufflenetv2_224 (widths 116 / 232 / 464 at the spatial sizes of data/layer_specs.json) at batch 128,
SFP<3,3>: fuse_bn_relu alone (leg A) against fuse_bn_relu + fusion.link_shuffle_units (leg B).

    python profiles/shuffle_units_bench.py [--batch 128] [--out profiles/shuffle_units_bench.json]

A unit is tests/golden/netgen_r3.py's _ShuffleUnit with name-seeded random weights and BatchNorm statistics.  The legs alternate
five times in one process; a leg is 30 forwards after 5 warm-up forwards, timed with HIP events; medians and the spread (max - min
over the rounds) are recorded, and the two legs' outputs are torch.equal.  Algorithmic bytes of the linked branch per pixel: the
float32 trunk read once and written once (2 x 8c), the two code hand-overs written and read once each (4 P).  Only single units are
timed here: the whole fixture net and per-kernel rates are not."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]
import netgen_r3 as ng  # noqa: E402
import utils.conv2d_func as cf  # noqa: E402
from utils.sfp_quant import layerout_quantize_func  # noqa: E402
from cnns_slfp_quantization_amd import fusion, layer_specs  # noqa: E402

ROUNDS, STEPS, WARMUP, Q = 5, 30, 5, 7


class Factories(ng.Factories):   # Ka for activations of order one, Kw so that three sigma of the He-like weights reach the top class
    def conv(self, name, cin, cout, k, stride=1, pad=0, groups=1):
        self.m[name] = (0.25, 3.0 * math.sqrt(2.0 / (cin // groups * k * k)) / 15.0)
        return super().conv(name, cin, cout, k, stride, pad, groups)


def leg_ms(unit, x):
    with torch.no_grad():
        for _ in range(WARMUP):
            unit(x)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(STEPS):
            y = unit(x)
        t1.record()
        torch.cuda.synchronize()
    return t0.elapsed_time(t1) / STEPS, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shuffle_units_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    dev = torch.device("cuda:0")
    shapes = sorted({(s.c_in, s.h) for s in layer_specs.conv_layers("shufflenetv2_224")
                     if s.k == (3, 3) and s.groups == s.c_in and s.stride == (1, 1) and s.c_in in (58, 116, 232)})
    rows = []
    for c, h in shapes:
        unit = ng._ShuffleUnit(Factories(cf, Q, {}, layerout=layerout_quantize_func), "u", 2 * c, 2 * c, 1)
        unit = ng.fill_parameters_by_name(unit, 11).to(dev).eval().to(memory_format=torch.channels_last)
        x = torch.randn((a.batch, 2 * c, h, h), generator=torch.Generator().manual_seed(c)).to(dev).contiguous(memory_format=torch.channels_last)
        fusion.fuse_bn_relu(unit)
        ta, tb = [], []
        for _ in range(ROUNDS):
            ms, ya = leg_ms(unit, x)
            ta.append(ms)
            assert fusion.link_shuffle_units(unit, x) == 1
            ms, yb = leg_ms(unit, x)
            tb.append(ms)
            assert torch.equal(ya, yb) and fusion.unlink_codes(unit) == 1
        pitch = (c + 31) // 32 * 32
        gb = a.batch * h * h * (16 * c + 4 * pitch) / 1e9
        ma, mb = statistics.median(ta), statistics.median(tb)
        rows.append({"c": c, "hw": h, "batch": a.batch, "unlinked_ms": round(ma, 4), "unlinked_spread_ms": round(max(ta) - min(ta), 4),
                     "linked_ms": round(mb, 4), "linked_spread_ms": round(max(tb) - min(tb), 4), "linked_over_unlinked": round(mb / ma, 3),
                     "linked_algorithmic_gb_per_s": round(gb / (mb * 1e-3), 1)})
        print(rows[-1], flush=True)
    json.dump({"device": torch.cuda.get_device_name(0), "q_bit": Q, "rounds": ROUNDS, "steps": STEPS, "warmup": WARMUP, "units": rows},
              open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
