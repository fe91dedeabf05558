"""Per-layer A/B of the depthwise k x k kernel (SLFP_DESC_DW_KXK, csrc/conv_dwk.hip) against the float32 direct kernel the library
runs for the same layer by default, through the C ABI on one GPU.

    python profiles/dwk_bench.py [--rounds 7] [--out profiles/dwk_bench.json]

Shapes: the depthwise 5x5 layers of MobileNetV3-Large and EfficientNet-B0 and the 7x7 layers of ConvNeXt-T at a 224 input; batch
32 and 128, q_bit 8, float32 NHWC on both sides, no bias.  Legs, alternated in one process after a warm-up round: "direct" (the
bit clear), "dwk" (the bit set, same descriptor otherwise) and, as a yardstick, "dw3x3": the depthwise 3x3 family on the same
tensor shapes (same channels, map, stride; padding 1), which moves the same bytes.  Per leg: the median over the rounds of the mean
of `iters` back-to-back launches between two events, and the spread (min, max) of the rounds.  `tb_per_s`: the bytes the layer has
to move, 4 |x| + 4 |y|, over the dwk leg's time (a whole-launch figure, not a profiler kernel time).  Every launch of a row reuses
the same x and y, and `mbytes` (x plus y) is below the 256 MiB Infinity Cache on all but two rows: those figures are cache-warm, not
HBM rates.  `dwk_ahead`: the dwk leg's slowest round beats the direct leg's fastest one.  `dwk_over_dw3x3`: how far the longer window
is from the 3x3 family on the same bytes;
reported, not gated.  Also recorded: kernel names, the selected variant and whether the two legs' outputs are the same bits."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cnns_slfp_quantization_amd import _lib as lib  # noqa: E402

# (net, kernel, channels, H = W of the input, stride)
LAYERS = [("mobilenetv3_large", 5, 72, 56, 2), ("mobilenetv3_large", 5, 120, 28, 1), ("mobilenetv3_large", 5, 672, 14, 2),
          ("mobilenetv3_large", 5, 960, 7, 1),
          ("efficientnet_b0", 5, 144, 56, 2), ("efficientnet_b0", 5, 240, 28, 1), ("efficientnet_b0", 5, 480, 14, 1),
          ("efficientnet_b0", 5, 672, 14, 2), ("efficientnet_b0", 5, 1152, 7, 1),
          ("convnext_t", 7, 96, 56, 1), ("convnext_t", 7, 192, 28, 1), ("convnext_t", 7, 384, 14, 1), ("convnext_t", 7, 768, 7, 1)]
BATCHES = (32, 128)
ITERS = {"direct": 5, "dwk": 100, "dw3x3": 100}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "dwk_bench.json"))
    a = ap.parse_args()
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(48)
    ka, kw = 0.21, 0.027
    rows = []
    for net, k, c, hw, s in LAYERS:
        for n in BATCHES:
            ho = (hw + 2 * (k // 2) - k) // s + 1
            x = torch.relu(torch.randn((n, hw, hw, c), generator=gen, device="cuda")) * (5.0 * ka)
            y = torch.empty((n, ho, ho, c), device="cuda")
            legs = {}
            for name, kk, bit in (("direct", k, 0), ("dwk", k, lib.DESC_DW_KXK), ("dw3x3", 3, 0)):
                w = torch.randn((c, 1, kk, kk), generator=torch.Generator(device="cuda").manual_seed(k * 1000 + c), device="cuda") * (4.0 * kw)
                d = lib.ConvDesc(n=n, c_in=c, h=hw, w=hw, c_out=c, kh=kk, kw=kk, stride_h=s, stride_w=s, pad_h=kk // 2, pad_w=kk // 2,
                                 dil_h=1, dil_w=1, groups=c, x_layout=lib.LAYOUT_NHWC, y_layout=lib.LAYOUT_NHWC, qbits=8, ka=ka, kw_scale=kw,
                                 mfma_passes=lib.MFMA_DEFAULT, reserved=bit)
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
            for name in ("direct", "dwk"):
                launch(name)
                outs[name] = y.clone()
            us = {name: round(statistics.median(v), 1) for name, v in times.items()}
            row = {"net": net, "k": k, "c": c, "hw": hw, "stride": s, "batch": n,
                   "kernel": {name: L.slfp_conv2d_kernel_name(ctypes.byref(v[0])).decode() for name, v in legs.items()},
                   "variant": L.slfp_debug_dwk_variant(ctypes.byref(legs["dwk"][0])).decode(),
                   "us": us, "us_min_max": {name: [round(min(v), 1), round(max(v), 1)] for name, v in times.items()},
                   "direct_over_dwk": round(us["direct"] / us["dwk"], 2),
                   "dwk_ahead": max(times["dwk"]) < min(times["direct"]),
                   "dwk_over_dw3x3": round(us["dwk"] / us["dw3x3"], 2),
                   "mbytes": round(4.0 * (x.numel() + y.numel()) / 2**20, 1),
                   "tb_per_s": round(4.0 * (x.numel() + y.numel()) / (statistics.median(times["dwk"]) * 1e-6) / 1e12, 2),
                   "same_bits_as_direct": bool(torch.equal(outs["dwk"].view(torch.int32), outs["direct"].view(torch.int32)))}
            rows.append(row)
            print(json.dumps(row), flush=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": ITERS, "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
