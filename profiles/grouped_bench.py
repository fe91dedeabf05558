"""Per-layer A/B of the block-diagonal grouped kernel (SLFP_DESC_GROUPED_MFMA, csrc/conv_grouped.hip) against the float32 direct
kernel the library runs for the same layer by default, through the C ABI on one GPU.

    python profiles/grouped_bench.py [--rounds 7] [--out profiles/grouped_bench.json]

Shapes: the 3x3 conv2 layers of ResNeXt-50 32x4d at a 224 input, and group-width 8 / 64 layers shaped like the first and last
stage of 32x8d; batch 32 and 128, q_bit 8, float32 NHWC on both sides, no bias.  Legs, alternated in one process after a warm-up
round: "direct" (the bit clear) and "mfma" (the bit set), same descriptor otherwise.  Per leg: the median over the rounds of the
mean of `iters` back-to-back launches between two events, and the spread (min, max) of the rounds.  `hbm_fraction`: the bytes the
layer has to move, 4 |x| + 4 |y|, over the mfma leg's time, as a fraction of the 8.0 TB/s roofline (a whole-launch figure, not a
profiler kernel time).  Also recorded: kernel names, the selected variant and the tensor-relative difference between the legs.
`mfma_ahead`: the mfma leg's slowest round beats the direct leg's fastest one."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cnns_slfp_quantization_amd import _lib as lib  # noqa: E402

# (C_in = C_out, groups, H = W of the input, stride)
LAYERS = [(128, 32, 56, 1), (256, 32, 56, 2), (256, 32, 28, 1), (512, 32, 28, 2), (512, 32, 14, 1), (1024, 32, 14, 2), (1024, 32, 7, 1),
          (256, 32, 56, 1), (256, 32, 56, 2), (2048, 32, 14, 2), (2048, 32, 7, 1)]   # group width 8, 8, 64, 64
BATCHES = (32, 128)
ITERS = {"direct": 3, "mfma": 10}
HBM = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "grouped_bench.json"))
    a = ap.parse_args()
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(47)
    ka, kw = 0.21, 0.027
    rows, seen = [], set()
    for c, g, hw, s in LAYERS:
        if (c, g, hw, s) in seen:   # 256 / 32 is both a 32x4d layer and the group-width-8 case
            continue
        seen.add((c, g, hw, s))
        for n in BATCHES:
            ho = (hw + 2 - 3) // s + 1
            x = torch.relu(torch.randn((n, hw, hw, c), generator=gen, device="cuda")) * (5.0 * ka)
            w = torch.randn((c, c // g, 3, 3), generator=gen, device="cuda") * (4.0 * kw)
            y = torch.empty((n, ho, ho, c), device="cuda")
            legs = {}
            for name, bit in (("direct", 0), ("mfma", lib.DESC_GROUPED_MFMA)):
                d = lib.ConvDesc(n=n, c_in=c, h=hw, w=hw, c_out=c, kh=3, kw=3, stride_h=s, stride_w=s, pad_h=1, pad_w=1, dil_h=1, dil_w=1,
                                 groups=g, x_layout=lib.LAYOUT_NHWC, y_layout=lib.LAYOUT_NHWC, qbits=8, ka=ka, kw_scale=kw,
                                 mfma_passes=lib.MFMA_F16X1, reserved=bit)
                blob = torch.empty(L.slfp_conv2d_wprep_bytes(ctypes.byref(d)), dtype=torch.uint8, device="cuda")
                lib.check(L.slfp_conv2d_prepare_weights(ctypes.byref(d), w.data_ptr(), blob.data_ptr(), None, st))
                ws = torch.empty(max(L.slfp_conv2d_workspace_bytes(ctypes.byref(d)), 16), dtype=torch.uint8, device="cuda")
                legs[name] = (d, blob, ws)

            def launch(name):
                d, blob, ws = legs[name]
                lib.check(L.slfp_conv2d_fwd(ctypes.byref(d), x.data_ptr(), blob.data_ptr(), None, y.data_ptr(), None, ws.data_ptr(), st))

            times = {name: [] for name in legs}
            for r in range(a.rounds + 1):   # round 0 warms up
                for name in legs:
                    launch(name)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(ITERS[name]):
                        launch(name)
                    e1.record()
                    e1.synchronize()
                    if r:
                        times[name].append(e0.elapsed_time(e1) * 1000.0 / ITERS[name])
            outs = {}
            for name in legs:
                launch(name)
                outs[name] = y.clone()
            us = {k: round(statistics.median(v), 1) for k, v in times.items()}
            row = {"c": c, "groups": g, "group_width": c // g, "hw": hw, "stride": s, "batch": n,
                   "kernel": {k: L.slfp_conv2d_kernel_name(ctypes.byref(v[0])).decode() for k, v in legs.items()},
                   "variant": L.slfp_debug_grouped_variant(ctypes.byref(legs["mfma"][0])).decode(),
                   "us": us, "us_min_max": {k: [round(min(v), 1), round(max(v), 1)] for k, v in times.items()},
                   "direct_over_mfma": round(us["direct"] / us["mfma"], 2),
                   "mfma_ahead": max(times["mfma"]) < min(times["direct"]),
                   "hbm_fraction": round(4.0 * (x.numel() + y.numel()) / (statistics.median(times["mfma"]) * 1e-6) / HBM, 3),
                   "max_rel_diff_mfma_vs_direct": float((outs["mfma"] - outs["direct"]).abs().max() / outs["direct"].abs().max())}
            rows.append(row)
            print(json.dumps(row), flush=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": ITERS, "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
