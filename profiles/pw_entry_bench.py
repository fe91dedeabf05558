#!/usr/bin/env python3
"""What a 1x1 layer that reads float32 and writes 1-byte codes (slfp_conv2d_fwd_entry) is worth.

    python profiles/pw_entry_bench.py [--out profiles/pw_entry_bench.json] [--skip-nets]

1. Per distinct conv1 geometry of ResNet-50 at batch 128 (SLFP<3,4>, BN + ReLU in the epilogue): the pair conv1 + conv2 with a
   float32 hand-over and conv2 writing codes (leg A, today's best) against conv1 writing codes (leg B), and conv1 ALONE in both forms.
2. The fixture ResNet-50 at batches 64 and 128: fuse_named_bn + fuse_residual + link_codes_traced (A) against the same with
   entries=True (B).
3. The fixture SqueezeNet at batch 256: fuse_fire (A) against fuse_fire(entries=True) (B).
The legs alternate A/B five times in one process; a leg is 30 calls after 5 warm-up calls, timed with HIP events; leg A's own
spread (max - min over its rounds) is reported next to every difference.  Outputs are compared bit for bit between the legs."""
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

ROUNDS, STEPS, WARMUP = 5, 30, 5
HBM_TBPS = 6.3   # float4 copy rate of an MI355X: what removed bytes are worth at best
BATCH = 128
# C_in, C_mid, image size at conv1, stride of conv2 (nets_imgnet/resnet50.py: the stride sits on the 3x3 layer)
GEOMS = [(64, 64, 56, 1), (256, 64, 56, 1), (256, 128, 56, 2), (512, 128, 28, 1), (512, 256, 28, 2), (1024, 256, 14, 1),
         (1024, 512, 14, 2), (2048, 512, 7, 1)]


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


def legs(fa, fb):
    a, b = [], []
    for _ in range(ROUNDS):
        a.append(timed(fa))
        b.append(timed(fb))
    ma, mb = statistics.median(a), statistics.median(b)
    spread = max(a) - min(a)
    return {"A_us": [round(1e3 * v, 2) for v in a], "B_us": [round(1e3 * v, 2) for v in b], "A_median_us": round(1e3 * ma, 2),
            "B_median_us": round(1e3 * mb, 2), "A_spread_us": round(1e3 * spread, 2), "gain_us": round(1e3 * (ma - mb), 2),
            "B_slower_by_more_than_A_spread": bool(mb - ma > spread), "B_faster_by_more_than_A_spread": bool(ma - mb > spread)}


def pair(dev, c_in, c_mid, hw, stride2):
    torch.manual_seed(c_in + c_mid + hw)
    ka1, ka2, ka3, kw = 0.45, 0.35, 0.3, 0.03

    def make():
        c1 = cf.conv2d_Q_bias(q_bit=8, Kw=kw, Ka=ka1)(c_in, c_mid, 1, kw, ka1, 1, 0, bias=False)
        c2 = cf.conv2d_Q_bias(q_bit=8, Kw=kw, Ka=ka2)(c_mid, c_mid, 3, kw, ka2, stride2, 1, bias=False)
        return torch.nn.ModuleList([c1, c2]).to(dev).eval().to(memory_format=torch.channels_last)

    A, B = make(), make()
    B.load_state_dict(A.state_dict())
    with torch.no_grad():
        for c in (A[0], A[1]):
            c.weight.mul_(3.0 * (2.0 / (c.in_channels * c.kernel_size[0] ** 2)) ** 0.5 / max(float(c.weight.std()), 1e-9))
        B.load_state_dict(A.state_dict())
        for m in (A, B):   # BN + ReLU in the epilogue, as fuse_named_bn + link_codes_traced leave the layers
            for c in m:
                c._post = (torch.full((c.out_channels,), 0.9, device=dev), torch.full((c.out_channels,), 0.05, device=dev), 1)
            m[1]._code_out = (ka3, 8)
        B[0]._code_out, B[0]._code_entry = (ka2, 8), True
        x = (torch.relu(torch.randn(BATCH, c_in, hw, hw, device=dev)) * 1.2).contiguous(memory_format=torch.channels_last)
        ya, yb = A[1](A[0](x)), B[1](B[0](x))
        assert ya.dtype == torch.uint8 and torch.equal(ya, yb), "the code hand-over changed conv2's output"
        both = legs(lambda: A[1](A[0](x)), lambda: B[1](B[0](x)))
        alone = legs(lambda: A[0](x), lambda: B[0](x))
    el = BATCH * hw * hw * c_mid
    return {"geometry": f"{c_in}->{c_mid} @{hw}, conv2 3x3 stride {stride2}", "conv1_output_elements": el,
            "predicted_saving_us_at_copy_rate": round(6 * el / (HBM_TBPS * 1e12) * 1e6, 2),
            "kernels_A": [A[0]._last_kernel, A[1]._last_kernel], "kernels_B": [B[0]._last_kernel, B[1]._last_kernel],
            "outputs_bit_identical": True, "conv1_plus_conv2": both, "conv1_alone": alone}


def build_net(name, dev, batch):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "nets_r3_golden.npz"))
    q, _, in_seed, seed = [int(v) for v in gold[name + ":meta"]]
    manifest = json.loads(bytes(gold[name + ":manifest"]).decode())
    gains = json.loads(bytes(gold[name + ":gains"]).decode())
    m = ng.BUILDERS[name](ng.Factories(cf, q, manifest, layerout=sq.layerout_quantize_func))
    ng.fill_parameters_by_name(m, seed, gains)
    if name == "resnet50":
        ng.load_bn_stats_by_name_(m, {k[len(name) + 1:]: gold[k] for k in gold.files if k.startswith(name + ":bn:")})
    m = m.to(dev).eval().to(memory_format=torch.channels_last)
    x = ng.net_input224(batch, in_seed).to(dev).contiguous(memory_format=torch.channels_last)
    return m, x


def net(name, dev, batch):
    ma, x = build_net(name, dev, batch)
    mb, _ = build_net(name, dev, batch)
    with torch.no_grad():
        links = []
        for m, entries in ((ma, False), (mb, True)):
            if name == "resnet50":
                fusion.fuse_bn_relu(m)
                assert fusion.fuse_named_bn(m, example_input=x) == 49 and fusion.fuse_residual(m, x) == 16
                links.append(fusion.link_codes_traced(m, x, entries=entries))
            else:
                links.append(fusion.fuse_fire(m, x, entries=entries))
        ya, yb = ma(x), mb(x)
        assert torch.equal(ya.view(torch.int32), yb.view(torch.int32)), "entries=True changed the logits"
        r = legs(lambda: ma(x), lambda: mb(x))
    r.update({"net": name, "batch": batch, "links_or_blocks_A": links[0], "links_or_blocks_B": links[1], "logits_bit_identical": True,
              "images_per_s_A": round(batch / r["A_median_us"] * 1e6, 1), "images_per_s_B": round(batch / r["B_median_us"] * 1e6, 1)})
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pw_entry_bench.json"))
    ap.add_argument("--skip-nets", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0),
           "protocol": f"A/B alternated {ROUNDS}x in one process, {STEPS} calls per leg after {WARMUP} warm-up, HIP events, eager launches",
           "leg_A": "float32 hand-over conv1 -> conv2 (conv2 writes codes) / link_codes_traced / fuse_fire",
           "leg_B": "conv1 writes codes (slfp_conv2d_fwd_entry) / link_codes_traced(entries=True) / fuse_fire(entries=True)",
           "hbm_copy_rate_TBps": HBM_TBPS, "batch_of_the_pairs": BATCH, "pairs": [], "nets": []}

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    for g in GEOMS:
        res["pairs"].append(pair(dev, *g))
        print(json.dumps(res["pairs"][-1]), flush=True)
        flush()
    if not args.skip_nets:
        for name, batch in (("resnet50", 64), ("resnet50", 128), ("squeezenet", 256)):
            res["nets"].append(net(name, dev, batch))
            print(json.dumps(res["nets"][-1]), flush=True)
            flush()


if __name__ == "__main__":
    main()
