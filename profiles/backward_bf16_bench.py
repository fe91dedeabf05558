"""Pointwise / Linear_Q backward: the float32-MFMA kernels (slfp_conv2d_bwd_ex) against the bf16 three-way-split kernels
(slfp_conv2d_bwd_bf16, conv2d_func.options.backward_gemm = "bf16x3").  DESIGN.md section 44.

    python profiles/backward_bf16_bench.py [--reps 20] [--rounds 5] [--out profiles/backward_bf16_bench.json]

Per layer: the distinct stride-1 1x1 layers of MobileNetV1-224 and ResNet-50 at batch 128 and the Linear_Q layers of AlexNet / VGG16
/ ResNet-50 (at batch 128, 512 and 2048), through the C ABI on preallocated NHWC operands (gx, gw and gb of one call).  The two legs alternate in one process;
each round times `reps` calls between HIP events after warm-up; reported: the median round and the spread (min .. max).  Rates are
algorithmic: 2 GEMMs of 2*M*Cin*Cout FLOP; bytes = read gy twice and x once, write gx (float32).  Floors: HBM at 8 TB/s; the matrix
unit at 157 TF (float32 MFMA) or 2500 / 6 TF (six bf16 products per float32 product).

Whole step: the MobileNetV1-224 `options.backward = "hip"` step (Conv2d_Q + BN + ReLU stack, NormalSGD) at batch 128 under both
settings, alternated, and the loss after three steps from the same seed for each.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cnns_slfp_quantization_amd import _lib, layer_specs, optimizer as O  # noqa: E402
from cnns_slfp_quantization_amd import conv2d_func as cf  # noqa: E402
from backward_bench import stack_model  # noqa: E402

HBM_TBS, F32_TF, BF16X3_TF = 8.0, 157.0, 2500.0 / 6


def layers(batch):
    """(label, n, h, w, c_in, c_out, Ka, Kw): distinct shapes, in the order met."""
    seen, out = set(), []
    for net in ("mobilenetv1_imagenet224", "resnet50_imagenet224"):
        for s in layer_specs.conv_layers(net):
            key = (s.c_in, s.c_out, s.h, s.w)
            if s.k == (1, 1) and s.groups == 1 and s.stride == (1, 1) and s.pad == (0, 0) and key not in seen:
                seen.add(key)
                out.append((f"{net.split('_')[0]} {s.c_in}->{s.c_out}@{s.h}", batch, s.h, s.w, s.c_in, s.c_out, s.Ka, s.Kw))
    for rows in (batch, 4 * batch, 16 * batch):   # the weight planes cost the same at every batch, the GEMMs' saving grows with it
        for name, ci, co in (("alexnet/vgg16 fc1", 25088, 4096), ("alexnet/vgg16 fc2", 4096, 4096), ("alexnet/vgg16 fc3", 4096, 1000),
                             ("resnet50 fc", 2048, 1000)):
            out.append((f"linear {name} {ci}->{co} x{rows}", rows, 1, 1, ci, co, 0.5, 0.05))
    return out


def _rounds(fn, reps, rounds):
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    return ms


def bench_layer(row, reps, rounds, warmup):
    label, n, h, w, ci, co, ka, kw = row
    L = _lib.load()
    d = _lib.ConvDesc(n=n, c_in=ci, h=h, w=w, c_out=co, kh=1, kw=1, stride_h=1, stride_w=1, pad_h=0, pad_w=0, dil_h=1, dil_w=1, groups=1,
                      x_layout=_lib.LAYOUT_NHWC, y_layout=_lib.LAYOUT_NHWC, qbits=8, ka=float(np.float32(ka)),
                      kw_scale=float(np.float32(kw)), mfma_passes=0, reserved=0)
    if not L.slfp_conv2d_bwd_bf16_supported(ctypes.byref(d), 0, 0):
        return {"layer": label, "bf16x3": "unsupported: " + _lib.last_error()}
    torch.manual_seed(ci + co + h)
    m = n * h * w
    x = torch.randn(m, ci, device="cuda") * ka
    wt = torch.randn(co, ci, device="cuda") * (2.0 / ci) ** 0.5
    gy = torch.randn(m, co, device="cuda")
    gx, gw, gb = torch.empty_like(x), torch.empty_like(wt), torch.empty(co, device="cuda")
    nb = max(L.slfp_conv2d_bwd_workspace_bytes_ex(ctypes.byref(d), 0, 1, 1), L.slfp_conv2d_bwd_bf16_workspace_bytes(ctypes.byref(d), 0, 1, 1))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ptrs = (wt.data_ptr(), gy.data_ptr(), gx.data_ptr(), gw.data_ptr(), gb.data_ptr(), ws.data_ptr(), st)
    legs = {"f32": lambda: _lib.check(L.slfp_conv2d_bwd_ex(ctypes.byref(d), 0, x.data_ptr(), *ptrs)),
            "bf16x3": lambda: _lib.check(L.slfp_conv2d_bwd_bf16(ctypes.byref(d), 0, x.data_ptr(), None, *ptrs))}
    ms = {k: [] for k in legs}
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    for _ in range(rounds):   # alternate the legs
        for k, fn in legs.items():
            ms[k] += _rounds(fn, reps, 1)
    flop = 2 * 2 * m * ci * co
    nbytes = 4 * (2 * m * co + 2 * m * ci)
    out = {"layer": label, "M": m, "c_in": ci, "c_out": co, "instance": L.slfp_debug_bwd_bf16_instance(ctypes.byref(d), 0, 0, 1, 1).decode()}
    for k, peak in (("f32", F32_TF), ("bf16x3", BF16X3_TF)):
        med = statistics.median(ms[k])
        floors = {"hbm": nbytes / HBM_TBS / 1e9, "mfma": flop / peak / 1e9}   # ms
        bound = max(floors, key=floors.get)
        out[k] = {"ms_median": round(med, 4), "ms_min": round(min(ms[k]), 4), "ms_max": round(max(ms[k]), 4),
                  "tflops": round(flop / med / 1e9, 1), "gbs": round(nbytes / med / 1e6, 0), "bound": bound,
                  "pct_of_bound": round(100 * floors[bound] / med, 1)}
    out["speedup_median"] = round(out["f32"]["ms_median"] / out["bf16x3"]["ms_median"], 2)
    # faster by more than the measured spread: the slowest new round beats the fastest float32 round
    out["faster_beyond_spread"] = out["bf16x3"]["ms_max"] < out["f32"]["ms_min"]
    print(json.dumps(out), flush=True)
    return out


def bench_step(batch, reps, rounds, warmup):
    net = "mobilenetv1_imagenet224"
    lf = torch.nn.CrossEntropyLoss()
    res = {"net": net, "batch": batch}
    cf.options.backward = "hip"
    try:
        for gemm in ("f32", "bf16x3"):   # the loss after three NormalSGD steps from one seed
            cf.options.backward_gemm = gemm
            torch.manual_seed(0)
            model, s0 = stack_model(net)
            x = torch.randn(batch, 3, s0.h, s0.w, device="cuda").contiguous(memory_format=torch.channels_last)
            y = torch.randint(0, 10, (batch,), device="cuda")
            opt = O.NormalSGD(model.parameters(), lr=1e-3, momentum=0.9)
            losses = []
            for _ in range(4):
                opt.zero_grad(set_to_none=True)
                loss = lf(model(x), y)
                losses.append(loss.item())
                loss.backward()
                opt.step()
            res[f"{gemm}_losses"] = losses
            res[f"{gemm}_kernels"] = sorted({m._last_bwd_kernel for m in model.modules() if getattr(m, "_last_bwd_kernel", None)})

        def one():
            opt.zero_grad(set_to_none=True)
            lf(model(x), y).backward()
            opt.step()

        ms = {"f32": [], "bf16x3": []}
        for gemm in ms:
            cf.options.backward_gemm = gemm
            for _ in range(warmup):
                one()
        for _ in range(rounds):
            for gemm in ms:
                cf.options.backward_gemm = gemm
                ms[gemm] += _rounds(one, reps, 1)
        for gemm, v in ms.items():
            res[f"{gemm}_ms"] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    finally:
        cf.options.backward, cf.options.backward_gemm = "composite", "f32"
    print("step", json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds, "batch": a.batch,
           "layers": [bench_layer(r, a.reps, a.rounds, a.warmup) for r in layers(a.batch)]}
    if not a.no_step:
        res["step"] = bench_step(a.batch, max(3, a.reps // 4), a.rounds, 2)
    if a.out:
        with open(a.out, "w") as f:
            layer_rows = res.pop("layers")   # one line per layer
            f.write(json.dumps(res)[:-1] + ', "layers": [\n' + ",\n".join(json.dumps(r) for r in layer_rows) + "\n]}\n")


if __name__ == "__main__":
    main()
