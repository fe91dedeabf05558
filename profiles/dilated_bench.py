"""Per-layer A/B of the phase-tiled dilated dense kernel (SLFP_DESC_DILATED_MFMA, csrc/conv_dense_dil.hip) against the float32
direct kernel the library runs for the same layer by default, through the C ABI on one GPU.

    python profiles/dilated_bench.py [--rounds 7] [--out profiles/dilated_bench.json]

Shapes: the conv2 layers of ResNet50(replace_stride_with_dilation=...) at a 224 input, batch 32 and 128, q_bit 8, float32 NHWC
on both sides, no bias.  Legs, alternated in one process after a warm-up round: "direct" (the bit clear), "mfma" (the bit set)
and, as a yardstick, "dense_d1": the same shape at dilation 1 on dense_mfma_f16x1, which does the same MACs, so mfma / dense_d1
is the price of the phase tiling.  Per leg: the median over the rounds of the mean of `iters` back-to-back launches between two
events (pre-pass included), and the spread (min, max) of the rounds.  Also recorded: the kernel names, the selected variants and
the tensor-relative difference between the two dilated legs.  `mfma_ahead`: the mfma leg's slowest round beats the direct leg's
fastest one."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cnns_slfp_quantization_amd import _lib as lib  # noqa: E402

# (C_in = C_out, H = W, dilation)
LAYERS = [(256, 28, 2), (512, 28, 2), (512, 28, 4), (512, 14, 2)]
BATCHES = (32, 128)
ITERS = {"direct": 3, "mfma": 10, "dense_d1": 10}   # the direct leg runs tens of milliseconds per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "dilated_bench.json"))
    a = ap.parse_args()
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(46)
    ka, kw = 0.21, 0.027
    rows = []
    for c, hw, dil in LAYERS:
        for n in BATCHES:
            x = torch.relu(torch.randn((n, hw, hw, c), generator=gen, device="cuda")) * (5.0 * ka)
            w = torch.randn((c, c, 3, 3), generator=gen, device="cuda") * (4.0 * kw)
            y = torch.empty((n, hw, hw, c), device="cuda")
            legs = {}
            for name, d_, bit in (("direct", dil, 0), ("mfma", dil, lib.DESC_DILATED_MFMA), ("dense_d1", 1, 0)):
                d = lib.ConvDesc(n=n, c_in=c, h=hw, w=hw, c_out=c, kh=3, kw=3, stride_h=1, stride_w=1, pad_h=d_, pad_w=d_, dil_h=d_, dil_w=d_,
                                 groups=1, x_layout=lib.LAYOUT_NHWC, y_layout=lib.LAYOUT_NHWC, qbits=8, ka=ka, kw_scale=kw,
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
            for name in ("direct", "mfma"):
                launch(name)
                outs[name] = y.clone()
            us = {k: round(statistics.median(v), 1) for k, v in times.items()}
            row = {"c": c, "hw": hw, "dilation": dil, "batch": n,
                   "kernel": {k: L.slfp_conv2d_kernel_name(ctypes.byref(v[0])).decode() for k, v in legs.items()},
                   "variant": {"mfma": L.slfp_debug_dense_dil_variant(ctypes.byref(legs["mfma"][0])).decode(),
                               "dense_d1": L.slfp_debug_dense_variant(ctypes.byref(legs["dense_d1"][0]), 0).decode()},
                   "us": us, "us_min_max": {k: [round(min(v), 1), round(max(v), 1)] for k, v in times.items()},
                   "direct_over_mfma": round(us["direct"] / us["mfma"], 2), "mfma_over_dense_d1": round(us["mfma"] / us["dense_d1"], 2),
                   "mfma_ahead": max(times["mfma"]) < min(times["direct"]),
                   "max_rel_diff_mfma_vs_direct": float((outs["mfma"] - outs["direct"]).abs().max() / outs["direct"].abs().max())}
            rows.append(row)
            print(json.dumps(row), flush=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": ITERS, "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
