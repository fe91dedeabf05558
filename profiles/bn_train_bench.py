"""Training-mode BatchNorm2d + ReLU: the stock modules (MIOpen's BatchNorm kernels and ATen's ReLU passes) against
fusion.TrainBatchNorm2d on csrc/bn_train.hip.  DESIGN.md section 27.

    python profiles/bn_train_bench.py [--reps 30] [--out profiles/bn_train_bench.json] [--no-steps]

Per BN shape of mobilenetv1_imagenet224 and mobilenetv1_cifar32 (layer_specs) at batch 128, channels_last: forward + backward of
[BatchNorm2d, ReLU] (gradients for x, gamma and beta), timed with HIP events after warm-up, the two legs alternated twice in one
process; each leg's time is the better of its two rounds and `stock_spread` is the stock leg's round-to-round difference
relative to its best -- a difference between the legs below it is noise.  GB/s is algorithmic: 12 B/element forward (read x,
write y; the statistics pass reads x once more) + 28 B/element backward (x, gy, y; then x, gy, y again and gx) against 8 TB/s.
The per-shape legs force every size onto the kernels (min_elements=0); `module_default` says what the module does on its own
(batchnorm.MIN_ELEMENTS, the rule read from this table).
Whole step: forward + backward + DSGD of backward_bench.py's Conv2d_Q + BN + ReLU stack with options.backward = "hip", the
BatchNorms stock or swapped (fusion.use_device_bn_train with its default rule), alternated the same way.
"""
import argparse
import collections
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import backward_bench  # noqa: E402
from backward_bench import _time  # noqa: E402
from cnns_slfp_quantization_amd import batchnorm, fusion, layer_specs, optimizer as O  # noqa: E402
from cnns_slfp_quantization_amd import conv2d_func as cf  # noqa: E402

PEAK_TBS = 8.0
BYTES_PER_ELEMENT = 12 + 28


def _alternate(legs, reps, warmup):
    """legs: {name: fn}.  Warm every leg, then two rounds of all legs in turn: ({name: best ms}, {name: spread})."""
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    rounds = {name: [] for name in legs}
    for _ in range(2):
        for name, fn in legs.items():
            rounds[name].append(_time(fn, reps))
    best = {name: min(v) for name, v in rounds.items()}
    spread = {name: (max(v) - min(v)) / min(v) for name, v in rounds.items()}
    return best, spread


def bench_shapes(net, batch, reps, warmup):
    shapes = collections.Counter((s.h_out, s.w_out, s.c_out) for s in layer_specs.conv_layers(net))
    rows = []
    for (h, w, c), count in shapes.items():
        torch.manual_seed(c + h)
        x = torch.randn(batch, c, h, w, device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_(True)
        gy = torch.randn(batch, c, h, w, device="cuda").contiguous(memory_format=torch.channels_last)
        stock = torch.nn.Sequential(torch.nn.BatchNorm2d(c), torch.nn.ReLU(inplace=True)).cuda().train()
        ours = torch.nn.Sequential(torch.nn.BatchNorm2d(c), torch.nn.ReLU(inplace=True)).cuda().train()
        assert fusion.use_device_bn_train(ours, min_elements=0) == 1   # every size on the kernels: this run is what the rule is read from

        def leg(model):
            def run():
                out = model(x)
                torch.autograd.grad(out, (x, model[0].weight, model[0].bias), gy)
            return run

        best, spread = _alternate({"stock": leg(stock), "hip": leg(ours)}, reps, warmup)
        assert ours[0]._last_kernel == "bn_train+relu", ours[0]._last_kernel
        nbytes = BYTES_PER_ELEMENT * batch * c * h * w
        row = {"net": net, "h": h, "w": w, "c": c, "layers": count, "elements": batch * c * h * w,
               "module_default": "bn_train" if batch * c * h * w >= batchnorm.MIN_ELEMENTS else "aten", "stock_ms": round(best["stock"], 4),
               "hip_ms": round(best["hip"], 4), "speedup": round(best["stock"] / best["hip"], 2),
               "stock_spread": round(spread["stock"], 3), "hip_spread": round(spread["hip"], 3),
               "hip_gbs": round(nbytes / best["hip"] / 1e6), "pct_hbm": round(100 * nbytes / best["hip"] / 1e9 / PEAK_TBS, 1),
               "faster_beyond_spread": bool(best["hip"] < best["stock"] * (1 - spread["stock"]))}
        print("shape", json.dumps(row), flush=True)
        rows.append(row)
        del x, gy, stock, ours
        torch.cuda.empty_cache()
    return rows


def bench_step(net, batch, reps, warmup):
    torch.manual_seed(0)
    model, s0 = backward_bench.stack_model(net)
    model.train()
    x = torch.randn(batch, 3, s0.h, s0.w, device="cuda").contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 10, (batch,), device="cuda")
    lf = torch.nn.CrossEntropyLoss()
    opt = O.DSGD(model.parameters(), 8, lr=1e-4, momentum=0.9, weight_decay=5e-4)
    cf.options.backward = "hip"

    def one():
        opt.zero_grad(set_to_none=True)
        lf(model(x), y).backward()
        opt.step()

    # the swap itself is outside the timed region
    rounds = {"stock": [], "bn_train": []}
    for name, prep in (("stock", fusion.restore_bn_train), ("bn_train", fusion.use_device_bn_train)):
        prep(model)
        for _ in range(warmup):
            one()
    for _ in range(2):
        for name, prep in (("stock", fusion.restore_bn_train), ("bn_train", fusion.use_device_bn_train)):
            prep(model)
            torch.cuda.synchronize()
            rounds[name].append(_time(one, reps))
    on_kernels = sum(getattr(m, "_last_kernel", "") in ("bn_train", "bn_train+relu") for m in model.modules())
    swapped_n = sum(isinstance(m, fusion.TrainBatchNorm2d) for m in model.modules())
    fusion.restore_bn_train(model)
    cf.options.backward = "composite"
    row = {"net": net, "batch": batch, "backward": "hip", "bn_swapped": swapped_n, "bn_on_kernels": on_kernels,
           "stock_bn_ms": round(min(rounds["stock"]), 3), "bn_train_ms": round(min(rounds["bn_train"]), 3),
           "speedup": round(min(rounds["stock"]) / min(rounds["bn_train"]), 2),
           "stock_spread": round((max(rounds["stock"]) - min(rounds["stock"])) / min(rounds["stock"]), 3)}
    print("step", json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "bn_train_bench.json"))
    a = ap.parse_args()
    nets = ("mobilenetv1_imagenet224", "mobilenetv1_cifar32")
    res = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "reps": a.reps,
           "bytes_per_element": {"forward": 12, "backward": 28}, "shapes": [], "steps": []}
    for net in nets:
        res["shapes"] += bench_shapes(net, a.batch, a.reps, a.warmup)
    if not a.no_steps:
        for net in nets:
            res["steps"].append(bench_step(net, a.batch, max(5, a.reps // 3), 3))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
