"""Backward of the dense k x k, strided 1x1 and stem Conv2d_Q layers: the composite (torch.nn.grad on quantized operands,
MIOpen / ATen) against the implicit-GEMM family dense_bwd_mfma_f32 (conv2d_func.options.backward = "hip_all",
SLFP_BWD_DENSE).  DESIGN.md section 12, addendum.

    python profiles/backward_dense_bench.py [--reps 50] [--out profiles/backward_dense_bench.json]
    python profiles/backward_dense_bench.py --nets vgg16_224 --no-steps            (a subset)
    python profiles/backward_dense_bench.py --trace-layer vgg16_224:3 --mode hip_all (one layer, for rocprofv3)

The protocol is profiles/backward_bench.py's: batch 128 (the ResNet-50 side-by-side stack: 64), channels_last, the backward
alone (torch.autograd.grad of a retained graph for x and w; the C_in = 3 stems for w only, as in a real net), HIP events,
`reps` repetitions after warm-up, the two modes alternated twice in one process.  Both legs of each mode are kept: the
composite's own spread between its two legs is the noise a speedup has to clear.  Rates are algorithmic: 2 GEMMs of
2 * MACs FLOP (one for a stem) over the whole hip_all backward (weight re-layout, gx, gw and the reduction launches) against
the 157.3 TF float32-MFMA peak.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cnns_slfp_quantization_amd import layer_specs  # noqa: E402
from cnns_slfp_quantization_amd import conv2d_func as cf  # noqa: E402
from cnns_slfp_quantization_amd.conv2d_func import conv2d_Q  # noqa: E402
from backward_bench import _time, bench_step  # noqa: E402

PEAK_TF = 157.3
NETS = ("vgg16_224", "resnet50_imagenet224", "squeezenet1_0_imagenet224", "alexnet_imagenet224")
MODES = ("composite", "hip_all")


def uncovered(net):
    """(layer index, spec) of every distinct geometry of `net` that options.backward = "hip" leaves on the composite."""
    seen, out = set(), []
    for i, s in enumerate(layer_specs.conv_layers(net)):
        if s.groups != 1 or (s.k == (1, 1) and s.stride == (1, 1) and s.pad == (0, 0)):
            continue
        key = (s.c_in, s.c_out, s.k, s.stride, s.pad, s.h, s.w)
        if key not in seen:
            seen.add(key)
            out.append((i, s))
    return out


def _layer(i, s, batch):
    torch.manual_seed(i)
    mod = conv2d_Q(8, s.Kw, s.Ka)(s.c_in, s.c_out, s.k, stride=s.stride, padding=s.pad, groups=s.groups).cuda()
    x = (torch.randn(batch, s.c_in, s.h, s.w, device="cuda") * s.Ka).contiguous(memory_format=torch.channels_last)
    stem = s.c_in == 3
    x.requires_grad_(not stem)
    gy = torch.randn(batch, s.c_out, s.h_out, s.w_out, device="cuda").contiguous(memory_format=torch.channels_last)
    out = mod(x)
    wanted = (mod.weight,) if stem else (x, mod.weight)
    return mod, stem, lambda: torch.autograd.grad(out, wanted, gy, retain_graph=True)


def bench_layers(net, batch, reps, warmup):
    rows = []
    for i, s in uncovered(net):
        mod, stem, bwd = _layer(i, s, batch)
        for mode in MODES:
            cf.options.backward = mode
            for _ in range(warmup):
                bwd()
        legs = {m: [] for m in MODES}
        for rnd in range(2):
            for mode in MODES:
                cf.options.backward = mode
                legs[mode].append(_time(bwd, reps))
        kern = mod._last_bwd_kernel
        t = {m: min(v) for m, v in legs.items()}
        spread = (max(legs["composite"]) - min(legs["composite"])) / min(legs["composite"])
        flop = (1 if stem else 2) * 2 * batch * s.macs
        row = {"layer": i, "c_in": s.c_in, "c_out": s.c_out, "k": list(s.k), "stride": s.stride[0], "pad": list(s.pad), "hw": s.h,
               "grads": "w" if stem else "x,w", "composite_ms": round(t["composite"], 4), "hip_all_ms": round(t["hip_all"], 4),
               "composite_legs_ms": [round(v, 4) for v in legs["composite"]], "hip_all_legs_ms": [round(v, 4) for v in legs["hip_all"]],
               "composite_spread_pct": round(100 * spread, 2), "speedup": round(t["composite"] / t["hip_all"], 2),
               "faster_beyond_spread": bool(t["hip_all"] < t["composite"] * (1 - spread)),
               "hip_all_kernel": kern, "hip_all_tflops": round(flop / t["hip_all"] / 1e9, 1),
               "pct_f32_mfma_peak": round(100 * flop / t["hip_all"] / 1e9 / PEAK_TF, 1)}
        print(net, json.dumps(row), flush=True)
        rows.append(row)
    cf.options.backward = "composite"
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--nets", nargs="*", default=list(NETS))
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--no-layers", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-layer", default=None, help="NET:LAYER_INDEX: run that layer's backward `reps` times in --mode and exit")
    ap.add_argument("--mode", default="hip_all")
    a = ap.parse_args()
    if a.trace_layer:
        net, idx = a.trace_layer.split(":")
        s = layer_specs.conv_layers(net)[int(idx)]
        _, _, bwd = _layer(int(idx), s, a.batch)
        cf.options.backward = a.mode
        for _ in range(a.reps):
            bwd()
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "batch": a.batch, "peak_tf": PEAK_TF, "layers": {}, "steps": []}
    if not a.no_layers:
        for net in a.nets:
            res["layers"][net] = bench_layers(net, a.batch, a.reps, a.warmup)
    if not a.no_steps:
        steps = max(5, a.reps // 5)
        for net, batch in (("vgg16_224", 128), ("resnet50_imagenet224", 64)):
            if net in a.nets:
                row = bench_step(net, batch, steps, 3, modes=("composite", "hip", "hip_all"))
                row["speedup_hip"] = round(row["composite_ms"] / row["hip_ms"], 2)
                row["speedup_hip_all"] = round(row["composite_ms"] / row["hip_all_ms"], 2)
                print("step", json.dumps(row), flush=True)
                res["steps"].append(row)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
