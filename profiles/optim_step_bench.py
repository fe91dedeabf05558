#!/usr/bin/env python3
"""Step time of the quantization-aware optimizers: the fused multi-tensor HIP step vs the ATen composite
(cnns_slfp_quantization_amd.optimizer.options.fused), on the parameter sets of the reference nets.

    python profiles/optim_step_bench.py [--steps 50] [--warmup 5] [--out FILE]

Prints one JSON line (and writes it to --out).  Rows:
  * sets: MobileNetV1-224 (4.2 M parameters), ResNet-50 (25.6 M), VGG-16 (138 M).  Conv weights (and conv biases) come from
    data/layer_specs.json; every conv gets a BatchNorm weight and bias; the fully-connected layers are the ImageNet ones
    (MobileNetV1 1024x1000, ResNet-50 2048x1000, VGG-16 25088x4096, 4096x4096, 4096x1000: the table's VGG-16 rows are
    CIFAR-sized).  DSGD, q_bit 8, momentum 0.9, weight_decay 5e-4 (the reference harness's setting): 24 B per element.
  * warm: K back-to-back steps between two HIP events, after W warm-up steps -> ms/step, GB/s = 24 B * numel / time.
  * cold: the same, with a 512 MiB buffer written before every step (outside the timed events) so that neither the
    parameters nor the state start in the 256 MiB Infinity Cache.
  * launches/step: device kernels of one step, counted with torch.profiler (null where the profiler is unavailable).
  * finetune: forward + backward + step of mobilenetv1_cifar32-shaped Conv2d_Q layers (+ BN, ReLU, pool, Linear_Q), batch 128.
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from cnns_slfp_quantization_amd import layer_specs, optimizer as O  # noqa: E402
from cnns_slfp_quantization_amd.conv2d_func import conv2d_Q, linear_Q  # noqa: E402

BYTES_PER_ELEM = 24
FC = {"mobilenetv1_imagenet224": [(1000, 1024)], "resnet50_imagenet224": [(1000, 2048)],
      "vgg16_224": [(4096, 25088), (4096, 4096), (1000, 4096)]}
NAMES = {"mobilenetv1_imagenet224": "MobileNetV1-224", "resnet50_imagenet224": "ResNet-50", "vgg16_224": "VGG-16"}


def param_shapes(net):
    shapes = []
    for l in layer_specs.conv_layers(net):
        shapes.append((l.c_out, l.c_in // l.groups, l.k[0], l.k[1]))
        if l.bias:
            shapes.append((l.c_out,))
        shapes += [(l.c_out,), (l.c_out,)]   # BatchNorm weight, bias
    for o, i in FC[net]:
        shapes += [(o, i), (o,)]
    return shapes


def make_params(shapes, gen):
    ps = []
    for s in shapes:
        p = torch.nn.Parameter(torch.randn(s, device="cuda", generator=gen) * 0.1)
        p.grad = torch.randn(s, device="cuda", generator=gen) * 0.01
        ps.append(p)
    return ps


def time_steps(opt, steps, flush=None):
    """ms per step over `steps` steps; with `flush`, the buffer is rewritten before every step, outside the events."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps if flush is not None else 1)]
    if flush is None:
        ev[0][0].record()
        for _ in range(steps):
            opt.step()
        ev[0][1].record()
        torch.cuda.synchronize()
        return ev[0][0].elapsed_time(ev[0][1]) / steps
    for a, b in ev:
        flush.add_(1.0)
        a.record()
        opt.step()
        b.record()
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in ev) / steps


def count_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception:  # noqa: BLE001  (the profiler is optional here)
        return None


def bench_set(net, args, flush):
    gen = torch.Generator(device="cuda").manual_seed(0)
    shapes = param_shapes(net)
    ps = make_params(shapes, gen)
    numel = sum(math.prod(s) for s in shapes)
    opt = O.DSGD(ps, 8, lr=0.01, momentum=0.9, weight_decay=5e-4)
    row = {"set": NAMES[net], "tensors": len(shapes), "numel": numel, "gb_per_step": numel * BYTES_PER_ELEM / 1e9}
    for mode in ("fused", "composite"):
        O.options.fused = mode == "fused"
        for _ in range(args.warmup):
            opt.step()
        ms = time_steps(opt, args.steps)
        row[mode] = {"ms_per_step": ms, "gb_per_s": numel * BYTES_PER_ELEM / ms / 1e6,
                     "launches_per_step": count_launches(opt.step)}
        if mode == "fused" or net != "vgg16_224":
            msc = time_steps(opt, args.steps, flush)
            row[mode]["cold_ms_per_step"] = msc
            row[mode]["cold_gb_per_s"] = numel * BYTES_PER_ELEM / msc / 1e6
    O.options.fused = True
    row["speedup_warm"] = row["composite"]["ms_per_step"] / row["fused"]["ms_per_step"]
    del opt, ps
    torch.cuda.empty_cache()
    return row


def finetune_model():
    layers = []
    for l in layer_specs.conv_layers("mobilenetv1_cifar32"):
        Conv = conv2d_Q(8, l.Kw, l.Ka)
        layers += [Conv(l.c_in, l.c_out, l.k, stride=l.stride, padding=l.pad, groups=l.groups),
                   torch.nn.BatchNorm2d(l.c_out), torch.nn.ReLU()]
    fc = [r for r in layer_specs.nets()["mobilenetv1_cifar32"]["layers"] if r["kind"] == "linear"][0]
    layers += [torch.nn.AdaptiveAvgPool2d(1), torch.nn.Flatten(), linear_Q(8, fc["Kw"], fc["Ka"])(fc["c_in"], fc["c_out"])]
    return torch.nn.Sequential(*layers).cuda()


def bench_finetune(args, batch=128):
    torch.manual_seed(0)
    model = finetune_model()
    x = torch.randn(batch, 3, 32, 32, device="cuda")
    y = torch.randint(0, 100, (batch,), device="cuda")
    opt = O.DSGD(model.parameters(), 8, lr=0.01, momentum=0.9, weight_decay=5e-4)
    loss_fn = torch.nn.CrossEntropyLoss()

    def one():
        opt.zero_grad(set_to_none=True)
        loss_fn(model(x), y).backward()
        opt.step()

    row = {"net": "mobilenetv1_cifar32 Conv2d_Q layers", "batch": batch,
           "params": sum(p.numel() for p in model.parameters())}
    for mode in ("fused", "composite"):
        O.options.fused = mode == "fused"
        for _ in range(args.warmup):
            one()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.steps):
            one()
        b.record()
        torch.cuda.synchronize()
        row[f"{mode}_ms_per_step"] = a.elapsed_time(b) / args.steps
    O.options.fused = True
    row["speedup"] = row["composite_ms_per_step"] / row["fused_ms_per_step"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_step_bench.py needs a GPU")
    flush = torch.empty(512 * 1024 * 1024 // 4, device="cuda")
    result = {"bench": "optim_step", "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
              "rule": "DSGD q_bit 8, momentum 0.9, weight_decay 5e-4", "bytes_per_elem": BYTES_PER_ELEM,
              "sets": [bench_set(n, args, flush) for n in ("mobilenetv1_imagenet224", "resnet50_imagenet224", "vgg16_224")]}
    del flush
    torch.cuda.empty_cache()
    result["finetune"] = bench_finetune(args)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
