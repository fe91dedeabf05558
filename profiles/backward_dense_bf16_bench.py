"""Dense k x k / strided 1x1 backward: the float32-MFMA dense kernels (slfp_conv2d_bwd_ex with SLFP_BWD_DENSE) against the bf16
three-way-split kernels (slfp_conv2d_bwd_dense_bf16, conv2d_func.options.backward_gemm = "bf16x3_all").  DESIGN.md section 45.

    python profiles/backward_dense_bf16_bench.py [--reps 20] [--rounds 5] [--out profiles/backward_dense_bf16_bench.json]

Per layer: the distinct dense layers of VGG-16, ResNet-50 (conv2 at stride 1 and 2, the strided 1x1 downsamples), SqueezeNet 1.0
(expand 3x3) and AlexNet (3x3 / 5x5) whose widths are multiples of 8, at batch 128, through the C ABI on preallocated NHWC operands
(gx, gw and gb of one call).  The two legs alternate in one process; each round times `reps` calls between HIP events after warm-up;
reported: the median round and the spread (min .. max).  Rates are algorithmic: 2 GEMMs of 2*M*taps*Cin*Cout FLOP (M = N*Ho*Wo);
bytes = read gy twice and x once, write gx (float32).  Floors: HBM at 8 TB/s; the matrix unit at 157 TF (float32 MFMA) or 2500 / 6
TF (six bf16 products per float32 product).  The rule: a layer counts as faster only if the bf16x3 median is
below the float32 leg's minimum and the float32 median is above the bf16x3 leg's maximum.

Whole step: a VGG-16-shaped Conv2d_Q + BN + ReLU stack (NormalSGD, --step-batch) and the Bottleneck stack of
profiles/bn_res_train_bench.py (DSGD, batch 128) under options.backward = "hip_all", "f32" against "bf16x3_all", alternated.
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
from backward_bf16_bench import BF16X3_TF, F32_TF, HBM_TBS, _rounds  # noqa: E402
import bn_res_train_bench  # noqa: E402

NETS = ("vgg16_224", "resnet50_imagenet224", "squeezenet1_0_imagenet224", "alexnet_imagenet224")


def layers():
    """ConvSpec rows with a label: the distinct dense geometries, in the order met."""
    seen, out = set(), []
    for net in NETS:
        for s in layer_specs.conv_layers(net):
            key = (s.c_in, s.c_out, s.h, s.w, s.k, s.stride, s.pad)
            pw = s.k == (1, 1) and s.stride == (1, 1) and s.pad == (0, 0)
            if s.groups == 1 and not pw and s.c_in % 8 == 0 and s.c_out % 8 == 0 and key not in seen:
                seen.add(key)
                out.append((f"{net.split('_')[0]} {s.c_in}->{s.c_out} k{s.k[0]}x{s.k[1]} s{s.stride[0]} @{s.h}", s))
    return out


def bench_layer(label, s, n, reps, rounds, warmup):
    L, flags = _lib.load(), _lib.BWD_DENSE
    d = _lib.ConvDesc(n=n, c_in=s.c_in, h=s.h, w=s.w, c_out=s.c_out, kh=s.k[0], kw=s.k[1], stride_h=s.stride[0], stride_w=s.stride[1],
                      pad_h=s.pad[0], pad_w=s.pad[1], dil_h=1, dil_w=1, groups=1, x_layout=_lib.LAYOUT_NHWC, y_layout=_lib.LAYOUT_NHWC,
                      qbits=8, ka=float(np.float32(s.Ka)), kw_scale=float(np.float32(s.Kw)), mfma_passes=0, reserved=0)
    if not L.slfp_conv2d_bwd_dense_bf16_supported(ctypes.byref(d), flags, 0):
        return {"layer": label, "bf16x3": "unsupported: " + _lib.last_error()}
    torch.manual_seed(s.c_in + s.c_out + s.h)
    taps, m = s.k[0] * s.k[1], n * s.h_out * s.w_out
    x = torch.randn(n, s.h, s.w, s.c_in, device="cuda") * s.Ka
    wt = torch.randn(s.c_out, s.c_in, *s.k, device="cuda") * (2.0 / (s.c_in * taps)) ** 0.5
    gy = torch.randn(n, s.h_out, s.w_out, s.c_out, device="cuda")
    gx, gw, gb = torch.empty_like(x), torch.empty_like(wt), torch.empty(s.c_out, device="cuda")
    nb = max(L.slfp_conv2d_bwd_workspace_bytes_ex(ctypes.byref(d), flags, 1, 1),
             L.slfp_conv2d_bwd_dense_bf16_workspace_bytes(ctypes.byref(d), flags, 1, 1))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    ptrs = (wt.data_ptr(), gy.data_ptr(), gx.data_ptr(), gw.data_ptr(), gb.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    legs = {"f32": lambda: _lib.check(L.slfp_conv2d_bwd_ex(ctypes.byref(d), flags, x.data_ptr(), *ptrs)),
            "bf16x3": lambda: _lib.check(L.slfp_conv2d_bwd_dense_bf16(ctypes.byref(d), flags, x.data_ptr(), None, *ptrs))}
    ms = {k: [] for k in legs}
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    for _ in range(rounds):   # alternate the legs
        for k, fn in legs.items():
            ms[k] += _rounds(fn, reps, 1)
    flop = 2 * 2 * m * taps * s.c_in * s.c_out
    nbytes = 4 * (2 * gy.numel() + 2 * x.numel())
    out = {"layer": label, "batch": n, "M": m, "taps": taps, "c_in": s.c_in, "c_out": s.c_out,
           "instance": L.slfp_debug_bwd_dense_bf16_instance(ctypes.byref(d), flags, 0, 1, 1).decode()}
    for k, peak in (("f32", F32_TF), ("bf16x3", BF16X3_TF)):
        med = statistics.median(ms[k])
        floors = {"hbm": nbytes / HBM_TBS / 1e9, "mfma": flop / peak / 1e9}   # ms
        bound = max(floors, key=floors.get)
        out[k] = {"ms_median": round(med, 4), "ms_min": round(min(ms[k]), 4), "ms_max": round(max(ms[k]), 4),
                  "tflops": round(flop / med / 1e9, 1), "gbs": round(nbytes / med / 1e6, 0), "bound": bound,
                  "pct_of_bound": round(100 * floors[bound] / med, 1)}
    out["speedup_median"] = round(out["f32"]["ms_median"] / out["bf16x3"]["ms_median"], 2)
    out["faster_beyond_spread"] = (out["bf16x3"]["ms_median"] < out["f32"]["ms_min"] and out["f32"]["ms_median"] > out["bf16x3"]["ms_max"])
    print(json.dumps(out), flush=True)
    return out


def bench_step(name, model, x, y, opt, reps, rounds, warmup):
    lf = torch.nn.CrossEntropyLoss()

    def one():
        opt.zero_grad(set_to_none=True)
        lf(model(x), y).backward()
        opt.step()

    res = {"stack": name, "batch": x.shape[0]}
    cf.options.backward = "hip_all"
    try:
        ms = {"f32": [], "bf16x3_all": []}
        for gemm in ms:
            cf.options.backward_gemm = gemm
            for _ in range(warmup):
                one()
            res[f"{gemm}_kernels"] = sorted({m._last_bwd_kernel for m in model.modules() if getattr(m, "_last_bwd_kernel", None)})
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
    ap.add_argument("--step-batch", type=int, default=64, help="batch of the VGG-16-shaped whole step")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds, "batch": a.batch,
           "layers": [bench_layer(label, s, a.batch, a.reps, a.rounds, a.warmup) for label, s in layers()]}
    if not a.no_step:
        torch.manual_seed(0)
        vgg, s0 = stack_model("vgg16_224")
        x = torch.randn(a.step_batch, 3, s0.h, s0.w, device="cuda").contiguous(memory_format=torch.channels_last)
        y = torch.randint(0, 10, (a.step_batch,), device="cuda")
        res["steps"] = [bench_step("vgg16-shaped", vgg, x, y, O.NormalSGD(vgg.parameters(), lr=1e-3, momentum=0.9), 3, a.rounds, 2)]
        del vgg, x
        torch.cuda.empty_cache()
        bott = bn_res_train_bench.stack_model().train()
        x = torch.randn(a.batch, bn_res_train_bench.STAGES[0][0], 56, 56, device="cuda").contiguous(memory_format=torch.channels_last)
        y = torch.randint(0, 100, (a.batch,), device="cuda")
        res["steps"].append(bench_step("bottleneck", bott, x, y, O.DSGD(bott.parameters(), 8, lr=1e-4, momentum=0.9, weight_decay=5e-4),
                                       5, a.rounds, 2))
    if a.out:
        with open(a.out, "w") as f:
            layer_rows = res.pop("layers")   # one line per layer
            f.write(json.dumps(res)[:-1] + ', "layers": [\n' + ",\n".join(json.dumps(r) for r in layer_rows) + "\n]}\n")


if __name__ == "__main__":
    main()
