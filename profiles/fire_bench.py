#!/usr/bin/env python3
"""SqueezeNet 1.0 (SFP<3,3>, the committed fixture net of tests/golden/netgen_r3.py + nets_r3_golden.npz) with its Fire modules
on 1-byte codes (fusion.fuse_fire) against the best configuration without it.

    python profiles/fire_bench.py [--batches 64 256] [--out profiles/fire_bench.json]

Leg A: fuse_bn_relu + link_codes_traced (both change nothing on this net).  Leg B: A + fuse_fire.  The legs alternate A/B five
times in one process; a leg is 30 forwards after 5 warm-up forwards, timed with HIP events.  Per Fire geometry the fused block
(four launches: squeeze, expand1x1, the 3x3 layer's decode pre-pass and its GEMM, on the codes its predecessor writes; the first one
five, on float32, its encode pass included) is timed against the eight launches it replaces (squeeze, relu_, expand1x1, relu_, the
3x3 layer's encode pre-pass and its GEMM, relu_, cat on float32), and the gain is set against what the removed HBM bytes predict
at the device's copy rate.  The 3x3 layer's pre-pass writes an fp16 copy of the squeeze output padded to 64 channels, which the
GEMM reads back: that traffic stays on both legs and is counted on both."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import netgen_r3 as ng  # noqa: E402
import utils.conv2d_func as cf  # noqa: E402
import utils.sfp_quant as sq  # noqa: E402
from cnns_slfp_quantization_amd import fusion  # noqa: E402
from cnns_slfp_quantization_amd.conv2d_func import _act_fmt, _f32  # noqa: E402
from cnns_slfp_quantization_amd.sfp_quant import hip_encode  # noqa: E402

ROUNDS, STEPS, WARMUP = 5, 30, 5
HBM_TBPS = 6.3   # float4 copy rate of an MI355X (8.0 TB/s peak): what removed bytes are worth at best


def build(dev, batch):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "nets_r3_golden.npz"))
    q, _, in_seed, seed = [int(v) for v in gold["squeezenet:meta"]]
    manifest = json.loads(bytes(gold["squeezenet:manifest"]).decode())
    gains = json.loads(bytes(gold["squeezenet:gains"]).decode())
    m = ng.BUILDERS["squeezenet"](ng.Factories(cf, q, manifest, layerout=sq.layerout_quantize_func))
    ng.fill_parameters_by_name(m, seed, gains)
    m = m.to(dev).eval().to(memory_format=torch.channels_last)
    x = ng.net_input224(batch, in_seed).to(dev).contiguous(memory_format=torch.channels_last)
    return m, x


def timed(fn, steps=STEPS, warmup=WARMUP):
    """milliseconds per call: `steps` calls between two HIP events after `warmup` calls"""
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


def fire_blocks(m):
    return [(n, b) for n, b in m.named_modules() if type(b).__name__ == "_Fire"]


def run_batch(dev, batch):
    ma, x = build(dev, batch)
    mb, _ = build(dev, batch)
    with torch.no_grad():
        for m in (ma, mb):
            assert fusion.fuse_bn_relu(m) == 0 and fusion.link_codes_traced(m, x) == 0
        ya = ma(x)
        n_fused = fusion.fuse_fire(mb, x)
        assert n_fused == 8, n_fused
        assert torch.equal(mb(x), ya), "fuse_fire changed the logits"
        legs = {"A": [], "B": []}
        for _ in range(ROUNDS):
            legs["A"].append(timed(lambda: ma(x)))
            legs["B"].append(timed(lambda: mb(x)))
        # per Fire geometry: the block's recorded float32 input from leg A
        rec = {}
        hooks = [b.register_forward_hook(lambda mod, inp, out, n=n: rec.__setitem__(n, inp[0].detach().clone())) for n, b in fire_blocks(ma)]
        ma(x)
        for h in hooks:
            h.remove()
        fires = []
        blocks_b = dict(fire_blocks(mb))
        for i, (name, blk_a) in enumerate(fire_blocks(ma)):
            blk_b = blocks_b[name]
            xin = rec[name]
            s, e1, e3 = blk_a.squeeze, blk_a.expand1x1, blk_a.expand3x3
            # leg B's block reads what its predecessor writes: codes (the first block: float32, and encodes it itself)
            xb = xin if i == 0 else hip_encode(xin, _f32(blk_b.squeeze.Ka), _act_fmt(blk_b.squeeze.q_bit))
            ta = [timed(lambda: blk_a(xin)) for _ in range(3)]
            tb = [timed(lambda: blk_b(xb)) for _ in range(3)]
            px = batch * xin.shape[2] * xin.shape[3]
            sq_el, out_el, in_el = px * s.out_channels, px * (e1.out_channels + e3.out_channels), px * s.in_channels
            plane = 2 * 2 * px * (-(-s.out_channels // 64) * 64)   # the 3x3 layer's fp16 operand copy (C padded to 64): written, read
            # float32 path: squeeze in 4, squeeze out 4 + relu_ 8 + two loads (expand1x1, the encode pre-pass) 8, block out 4 + relu_ 8 + cat 8
            bytes_a = 4 * in_el + 20 * sq_el + plane + 20 * out_el
            # code path: squeeze in 1 (first block: 4 + 1 + 1 through the encode pass), squeeze out 1 + two loads 2, block out 1
            bytes_b = (6 if i == 0 else 1) * in_el + 3 * sq_el + plane + 1 * out_el
            a_us, b_us = 1e3 * statistics.median(ta), 1e3 * statistics.median(tb)
            fires.append({"block": name, "geometry": f"{s.in_channels}->{s.out_channels}->{e1.out_channels}+{e3.out_channels} @{xin.shape[2]}",
                          "eight_launches_us": round(a_us, 2), "fused_us": round(b_us, 2), "saved_us": round(a_us - b_us, 2),
                          "hbm_bytes_float32_path": int(bytes_a), "hbm_bytes_code_path": int(bytes_b),
                          "predicted_saving_us_at_copy_rate": round((bytes_a - bytes_b) / (HBM_TBPS * 1e12) * 1e6, 2),
                          "three_convs_kernels": [c._last_kernel for c in (blk_b.squeeze, blk_b.expand1x1, blk_b.expand3x3)]})
    med = {k: statistics.median(v) for k, v in legs.items()}
    return {"batch": batch, "fire_blocks_fused": n_fused, "logits_bit_identical": True,
            "leg_A_ms": [round(v, 4) for v in legs["A"]], "leg_B_ms": [round(v, 4) for v in legs["B"]],
            "leg_A_median_ms": round(med["A"], 4), "leg_B_median_ms": round(med["B"], 4),
            "leg_A_spread_ms": round(max(legs["A"]) - min(legs["A"]), 4), "gain_ms": round(med["A"] - med["B"], 4),
            "speedup": round(med["A"] / med["B"], 4), "images_per_s_A": round(batch / med["A"] * 1e3, 1),
            "images_per_s_B": round(batch / med["B"] * 1e3, 1),
            "B_faster_by_more_than_A_spread": bool(max(legs["B"]) < min(legs["A"]) and med["A"] - med["B"] > max(legs["A"]) - min(legs["A"])),
            "fires_saved_us_sum": round(sum(f["saved_us"] for f in fires), 2),
            "fires_predicted_saving_us_sum": round(sum(f["predicted_saving_us_at_copy_rate"] for f in fires), 2),
            "fires": fires}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fire_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"net": "squeezenet1_0 (fixture net, SFP<3,3>, channels_last)", "device": torch.cuda.get_device_name(0),
           "protocol": f"A/B alternated {ROUNDS}x in one process, {STEPS} forwards per leg after {WARMUP} warm-up, HIP events",
           "leg_A": "fuse_bn_relu + link_codes_traced (no change on this net)", "leg_B": "leg A + fuse_fire",
           "hbm_copy_rate_TBps": HBM_TBPS, "results": [run_batch(dev, b) for b in args.batches]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for r in res["results"]:
        print(json.dumps({k: v for k, v in r.items() if k != "fires"}))
        for fr in r["fires"]:
            print("   ", json.dumps({k: v for k, v in fr.items() if k != "three_convs_kernels"}))


if __name__ == "__main__":
    main()
