"""Training-mode [BatchNorm2d, layerout_quantize_func, Swish | GELU]: the stock modules (MIOpen's BatchNorm, the quantizer pass,
ATen's activation passes) against fusion.TrainBatchNormLayerout2d on the table forms of csrc/bn_train.hip.  DESIGN.md section 32.

    python profiles/bn_layerout_train_bench.py [--reps 20 (at least)] [--out profiles/bn_layerout_train_bench.json] [--no-steps]

Shapes (layer_specs): vgg16_cifar32 (GELU) -- the conv outputs of vgg16_224 at 1/7 of the side, which is VGG16_gelu on CIFAR;
mobilenetv1_cifar32 (Swish); mobilenetv1_imagenet224 (Swish), for scale.  Batch 128 and 256, channels_last: forward + backward
of the block (gradients for x, gamma and beta), timed with HIP events after warm-up (and a second of unrelated work before the first
window), every window at least 150 ms long (`reps`), the two legs alternated twice in one process; each leg's time is the better of its two rounds and `stock_spread` is the stock leg's round-to-round difference relative
to its best -- a difference between the legs below it is noise (the method of bn_train_bench.py).  GB/s is algorithmic: 12
B/element forward (the statistics pass reads x, the apply reads x and writes y) + 20 B/element backward (x, gy; then x, gy and
gx) against 8 TB/s.  The per-shape legs force every size onto the kernels (min_elements=0); `module_default` says what the
module does on its own (batchnorm.LUT_MIN_ELEMENTS, the rule read from this table).
Whole step: forward + backward + DSGD of a [Conv2d_Q, BN, layerout, act] stack with the nets' conv shapes at batch 128 with
options.backward = "hip", the tails stock or swapped at min_elements=0, alternated the same way.
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
from backward_bench import _time  # noqa: E402
from bn_train_bench import _alternate  # noqa: E402
from cnns_slfp_quantization_amd import activation_func as af, batchnorm, fusion, layer_specs, optimizer as O  # noqa: E402
from cnns_slfp_quantization_amd import conv2d_func as cf  # noqa: E402
from cnns_slfp_quantization_amd.sfp_quant import layerout_quantize_func  # noqa: E402

PEAK_TBS = 8.0
BYTES_PER_ELEMENT = 12 + 20
WINDOW_MS = 150.0
MAX_REPS = 2000
NETS = {"vgg16_cifar32": ("vgg16_224", 7, torch.nn.GELU), "mobilenetv1_cifar32": ("mobilenetv1_cifar32", 1, af.Swish),
        "mobilenetv1_imagenet224": ("mobilenetv1_imagenet224", 1, af.Swish)}


def _specs(net):
    """(ConvSpec, h_in, h_out) per layer of `net`; vgg16_cifar32 is vgg16_224 with every side divided by 7."""
    table, div, _ = NETS[net]
    return [(s, s.h // div, s.h_out // div) for s in layer_specs.conv_layers(table)]


def _tail(c, act):
    return [torch.nn.BatchNorm2d(c), layerout_quantize_func(8), act()]


def bench_shapes(net, batch, reps, warmup):
    act = NETS[net][2]
    shapes = collections.Counter((ho, ho * s.w_out // s.h_out, s.c_out) for s, _, ho in _specs(net))
    rows = []
    for (h, w, c), count in shapes.items():
        torch.manual_seed(c + h)
        x = torch.randn(batch, c, h, w, device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_(True)
        gy = torch.randn(batch, c, h, w, device="cuda").contiguous(memory_format=torch.channels_last)
        stock = torch.nn.Sequential(*_tail(c, act)).cuda().train()
        ours = torch.nn.Sequential(*_tail(c, act)).cuda().train()
        assert fusion.use_device_bn_layerout_train(ours, min_elements=0) == 1   # every size on the kernels: the rule is read from this run

        def leg(model):
            def run():
                out = model(x)
                torch.autograd.grad(out, (x, model[0].weight, model[0].bias), gy)
            return run

        legs = {"stock": leg(stock), "hip": leg(ours)}
        for fn in legs.values():
            for _ in range(warmup):
                fn()
        # a timed window of WINDOW_MS at least: a window of a few milliseconds measures the clock and the scheduler, not the legs
        n_reps = max(reps, min(MAX_REPS, int(WINDOW_MS / max(_time(legs["stock"], 10), 1e-3))))
        best, spread = _alternate(legs, n_reps, warmup)
        assert ours[0]._last_kernel == "bn_lut_train", ours[0]._last_kernel
        elements = batch * c * h * w
        nbytes = BYTES_PER_ELEMENT * elements
        row = {"net": net, "act": act.__name__, "batch": batch, "h": h, "w": w, "c": c, "layers": count, "elements": elements, "reps": n_reps,
               "module_default": "bn_lut_train" if elements >= batchnorm.LUT_MIN_ELEMENTS else "aten",
               "stock_ms": round(best["stock"], 4), "hip_ms": round(best["hip"], 4), "speedup": round(best["stock"] / best["hip"], 2),
               "stock_spread": round(spread["stock"], 3), "hip_spread": round(spread["hip"], 3),
               "hip_gbs": round(nbytes / best["hip"] / 1e6), "pct_hbm": round(100 * nbytes / best["hip"] / 1e9 / PEAK_TBS, 1),
               "faster_beyond_spread": bool(best["hip"] < best["stock"] * (1 - spread["stock"]))}
        print("shape", json.dumps(row), flush=True)
        rows.append(row)
        del x, gy, stock, ours
        torch.cuda.empty_cache()
    return rows


def stack_model(net):
    """[Conv2d_Q, BN, layerout, act] per conv layer of `net` (a 2 x 2 max pool where the table's side halves between two layers),
    then pool, flatten and a 100-way Linear_Q with nominal scales."""
    act = NETS[net][2]
    layers, side = [], None
    for s, h_in, h_out in _specs(net):
        if side is not None and h_in * 2 == side:
            layers.append(torch.nn.MaxPool2d(2))
        Conv = cf.conv2d_Q(8, s.Kw, s.Ka)
        layers += [Conv(s.c_in, s.c_out, s.k, stride=s.stride, padding=s.pad, groups=s.groups)] + _tail(s.c_out, act)
        side = h_out
    first = _specs(net)[0]
    layers += [torch.nn.AdaptiveAvgPool2d(1), torch.nn.Flatten(), cf.linear_Q(8, 0.05, 0.5)(_specs(net)[-1][0].c_out, 100)]
    return torch.nn.Sequential(*layers).cuda().to(memory_format=torch.channels_last), first[1]


def bench_step(net, batch, reps, warmup):
    torch.manual_seed(0)
    model, side = stack_model(net)
    model.train()
    x = torch.randn(batch, 3, side, side, device="cuda").contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 100, (batch,), device="cuda")
    lf = torch.nn.CrossEntropyLoss()
    opt = O.DSGD(model.parameters(), 8, lr=1e-4, momentum=0.9, weight_decay=5e-4)
    prev = cf.options.backward
    cf.options.backward = "hip"

    def one():
        opt.zero_grad(set_to_none=True)
        lf(model(x), y).backward()
        opt.step()

    def swap(m):
        fusion.use_device_bn_layerout_train(m, min_elements=0)

    # the swap itself is outside the timed region
    legs = (("stock", fusion.restore_bn_layerout_train), ("bn_lut_train", swap))
    rounds = {name: [] for name, _ in legs}
    try:
        for name, prep in legs:
            prep(model)
            for _ in range(warmup):
                one()
        for _ in range(2):
            for name, prep in legs:
                prep(model)
                torch.cuda.synchronize()
                rounds[name].append(_time(one, reps))
        on_kernels = sum(getattr(m, "_last_kernel", "") == "bn_lut_train" for m in model.modules())
        swapped_n = sum(isinstance(m, fusion.TrainBatchNormLayerout2d) for m in model.modules())
    finally:
        fusion.restore_bn_layerout_train(model)
        cf.options.backward = prev
    row = {"net": net, "batch": batch, "backward": "hip", "blocks_swapped": swapped_n, "blocks_on_kernels": on_kernels,
           "stock_ms": round(min(rounds["stock"]), 3), "bn_lut_train_ms": round(min(rounds["bn_lut_train"]), 3),
           "speedup": round(min(rounds["stock"]) / min(rounds["bn_lut_train"]), 2),
           "stock_spread": round((max(rounds["stock"]) - min(rounds["stock"])) / min(rounds["stock"]), 3)}
    print("step", json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "bn_layerout_train_bench.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "batches": a.batches, "reps": a.reps,
           "bytes_per_element": {"forward": 12, "backward": 20}, "lut_min_elements": batchnorm.LUT_MIN_ELEMENTS, "shapes": [], "steps": []}
    spin = torch.randn(4096, 4096, device="cuda")   # a second of work before the first window: clocks up, code objects loaded
    for _ in range(200):
        spin = torch.tanh(spin @ spin * 1e-4)
    torch.cuda.synchronize()
    del spin
    for batch in a.batches:
        for net in NETS:
            res["shapes"] += bench_shapes(net, batch, a.reps, a.warmup)
    if not a.no_steps:
        for net in ("vgg16_cifar32", "mobilenetv1_cifar32"):
            try:
                res["steps"].append(bench_step(net, 128, 30, 5))
            except Exception as e:   # a step row that cannot run is recorded, not dropped
                res["steps"].append({"net": net, "batch": 128, "error": f"{type(e).__name__}: {e}"})
                print("step", json.dumps(res["steps"][-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
