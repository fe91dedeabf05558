"""Per-layer A/B of the E4M3 pointwise kernel (SLFP_MFMA_FP8, csrc/conv_pw_fp8.hip) against the fp16 code kernel the library runs for
the same layer, through the C ABI on one GPU.

    python profiles/pw_fp8_bench.py [--rounds 7] [--iters 20] [--out profiles/pw_fp8_bench.json]

Shapes: SqueezeNet 1.0's Fire 1x1 layers at batch 256 and MobileNetV1's thirteen pointwise layers at batch 128, q_bit 7; codes -> codes
(ReLU folded) and codes -> float32.  Legs, alternated in one process after a warm-up, medians over the rounds of the mean of `iters`
back-to-back launches between two events: fp16, fp8 as selected, fp8 with PG forced to 1 and to 2 (SLFP_PW8_PG).  Also recorded per
shape: the variant strings and whether the float32 outputs of the two kernels are torch.equal.  Rows where fp16 wins are marked."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cnns_slfp_quantization_amd import _lib as lib  # noqa: E402

# (net, C_in, C_out, H = W, batch)
SQUEEZE = [(96, 16, 54), (16, 64, 54), (128, 16, 54), (128, 32, 54), (32, 128, 54), (256, 32, 27), (256, 48, 27), (48, 192, 27),
           (384, 48, 27), (384, 64, 27), (64, 256, 27), (512, 64, 13), (512, 1000, 13)]
MOBILE = [(32, 64, 112), (64, 128, 56), (128, 128, 56), (128, 256, 28), (256, 256, 28), (256, 512, 14), (512, 512, 14), (512, 1024, 7),
          (1024, 1024, 7)]   # 512 -> 512 runs five times in the net: thirteen layers, nine shapes
SHAPES = [("squeezenet", ci, co, hw, 256) for ci, co, hw in SQUEEZE] + [("mobilenetv1", ci, co, hw, 128) for ci, co, hw in MOBILE]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "pw_fp8_bench.json"))
    a = ap.parse_args()
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(7)
    rows = []

    def switch(pg):
        if pg:
            os.environ["SLFP_PW8_PG"] = str(pg)
        else:
            os.environ.pop("SLFP_PW8_PG", None)
        L.slfp_debug_reload_switches()

    for net, ci, co, hw, n in SHAPES:
        ka, kw = 0.31, 0.02
        x = torch.relu(torch.randn((n, hw, hw, ci), generator=gen, device="cuda")) * (4.0 * ka)
        xc = torch.empty_like(x, dtype=torch.uint8)
        lib.check(L.slfp_encode_f32(x.data_ptr(), xc.data_ptr(), x.numel(), ka, lib.FMT_SFP7 | lib.FMT_EXT, st))
        del x
        w = torch.randn((co, ci, 1, 1), generator=gen, device="cuda") * (3.0 * kw)
        desc, blob = {}, {}
        for mode in (lib.MFMA_F16X1, lib.MFMA_FP8):
            d = lib.ConvDesc(n=n, c_in=ci, h=hw, w=hw, c_out=co, kh=1, kw=1, stride_h=1, stride_w=1, pad_h=0, pad_w=0, dil_h=1, dil_w=1,
                             groups=1, x_layout=lib.LAYOUT_NHWC, y_layout=lib.LAYOUT_NHWC, qbits=7, ka=ka, kw_scale=kw, mfma_passes=mode, reserved=0)
            b = torch.empty(L.slfp_conv2d_wprep_bytes(ctypes.byref(d)), dtype=torch.uint8, device="cuda")
            lib.check(L.slfp_conv2d_prepare_weights(ctypes.byref(d), w.data_ptr(), b.data_ptr(), None, st))
            desc[mode], blob[mode] = d, b
        for y_codes in ([1, 0] if co % 16 == 0 else [0]):
            io = lib.ConvIo(x_codes=1, y_codes=y_codes, y_ka=0.4, y_qbits=7)
            y = torch.empty((n, hw, hw, co), dtype=torch.uint8 if y_codes else torch.float32, device="cuda")
            legs = [("fp16", lib.MFMA_F16X1, 0), ("fp8", lib.MFMA_FP8, 0), ("fp8_pg1", lib.MFMA_FP8, 1), ("fp8_pg2", lib.MFMA_FP8, 2)]

            def launch(mode):
                lib.check(L.slfp_conv2d_fwd_codes(ctypes.byref(desc[mode]), ctypes.byref(io), xc.data_ptr(), blob[mode].data_ptr(), None, None, None,
                                                  1, y.data_ptr(), st))

            times = {name: [] for name, _, _ in legs}
            variant = {}
            for r in range(a.rounds + 1):   # round 0 warms up
                for name, mode, pg in legs:
                    switch(pg)
                    if r == 0:
                        variant[name] = L.slfp_debug_pw_variant(ctypes.byref(desc[mode]), ctypes.byref(io), 0, 0, 0).decode()
                    launch(mode)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        launch(mode)
                    e1.record()
                    e1.synchronize()
                    if r:
                        times[name].append(e0.elapsed_time(e1) * 1000.0 / a.iters)
            switch(0)
            row = {"net": net, "c_in": ci, "c_out": co, "hw": hw, "batch": n, "out": "codes" if y_codes else "f32", "variant": variant,
                   "us": {k: round(statistics.median(v), 2) for k, v in times.items()}}
            if not y_codes:
                outs = {}
                for mode in (lib.MFMA_F16X1, lib.MFMA_FP8):
                    launch(mode)
                    outs[mode] = y.clone()
                row["equal_to_fp16"] = bool(torch.equal(outs[lib.MFMA_F16X1], outs[lib.MFMA_FP8]))
                d = (outs[lib.MFMA_FP8] - outs[lib.MFMA_F16X1]).abs().max() / outs[lib.MFMA_F16X1].abs().max()
                row["max_rel_diff_to_fp16"] = float(d)
            row["fp16_wins"] = row["us"]["fp16"] < row["us"]["fp8"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters, "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
