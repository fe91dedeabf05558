"""Training-mode tail of a ResNet-50 Bottleneck, out = bn3(out); out += identity; out = relu(out): the stock modules (MIOpen's
BatchNorm, ATen's in-place add, ATen's ReLU) against fusion.TrainBatchNorm2d(x, residual=identity, relu=True) on the residual
forms of csrc/bn_train.hip.  DESIGN.md section 33.

    python profiles/bn_res_train_bench.py [--reps 20 (at least)] [--out profiles/bn_res_train_bench.json] [--no-steps]

(a) `tails`: the trunk shapes of ResNet-50, (56,56,256), (28,28,512), (14,14,1024), (7,7,2048), batch 64 and 128, channels_last:
forward + backward of the tail (gradients for x, identity, gamma and beta), timed with HIP events after warm-up (and a second of
unrelated work before the first window), every window at least 150 ms long (`reps`), the two legs alternated twice in one
process; each leg's time is the better of its two rounds and `stock_spread` is the stock leg's round-to-round difference relative
to its best -- a difference between the legs below it is noise (the method of bn_train_bench.py).  GB/s is algorithmic: 16
B/element forward (the statistics pass reads x; the apply reads x and identity and writes y) + 32 B/element backward (the reduce
reads x, gy, y; the dx pass reads them again and writes gx and the identity's gradient) against 8 TB/s.  The legs force every
size onto the kernels (min_elements=0); `module_default` says what the module does on its own (batchnorm.RES_MIN_ELEMENTS).
(b) `bn_relu`: the same for [BatchNorm2d, ReLU] at the bn1 / bn2 shapes, stock against use_device_bn_train(min_elements=0), as a
reference row (12 + 24 B/element).
(c) `steps`: forward + backward + DSGD at batch 64 with options.backward = "hip_all" of a stack with one downsample Bottleneck and
one plain Bottleneck per stage (the real channel counts and strides, Conv2d_Q with nominal scales), three legs alternated the same
way: stock tails, use_device_bn_train, and use_device_bottleneck_train on top (both at min_elements=0).
`rule`: the smallest size class (N C H W elements) from which this class and every larger measured class beat the stock leg by
more than the stock leg's spread on every row, which is what batchnorm.RES_MIN_ELEMENTS is read from.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from backward_bench import _time  # noqa: E402
from bn_train_bench import _alternate  # noqa: E402
from cnns_slfp_quantization_amd import batchnorm, fusion, optimizer as O  # noqa: E402
from cnns_slfp_quantization_amd import conv2d_func as cf  # noqa: E402

PEAK_TBS = 8.0
WINDOW_MS = 150.0
MAX_REPS = 2000
TRUNK = ((56, 56, 256), (28, 28, 512), (14, 14, 1024), (7, 7, 2048))
INNER = ((56, 56, 64), (28, 28, 128), (14, 14, 256), (7, 7, 512))
STAGES = ((64, 64, 256, 1), (256, 128, 512, 2), (512, 256, 1024, 2), (1024, 512, 2048, 2))   # (in, width, out, stride)


class StockTail(nn.Module):
    """The three statements of the stock block."""

    def __init__(self, c):
        super().__init__()
        self.bn3, self.relu = nn.BatchNorm2d(c), nn.ReLU()

    def forward(self, out, identity):
        out = self.bn3(out)
        out += identity
        return self.relu(out)


class HipTail(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.bn3 = fusion.TrainBatchNorm2d(nn.BatchNorm2d(c), 0)   # every size on the kernels: the rule is read from this run

    def forward(self, out, identity):
        return self.bn3(out, residual=identity, relu=True)


def _row(kind, batch, h, w, c, n_reps, best, spread, bytes_per_element, default_floor, kernel):
    elements = batch * c * h * w
    nbytes = bytes_per_element * elements
    return {"kind": kind, "batch": batch, "h": h, "w": w, "c": c, "elements": elements, "reps": n_reps,
            "module_default": kernel if elements >= default_floor else "aten",
            "stock_ms": round(best["stock"], 4), "hip_ms": round(best["hip"], 4), "speedup": round(best["stock"] / best["hip"], 2),
            "stock_spread": round(spread["stock"], 3), "hip_spread": round(spread["hip"], 3),
            "hip_gbs": round(nbytes / best["hip"] / 1e6), "pct_hbm": round(100 * nbytes / best["hip"] / 1e9 / PEAK_TBS, 1),
            "faster_beyond_spread": bool(best["hip"] < best["stock"] * (1 - spread["stock"]))}


def _measure(legs, reps, warmup):
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    # a timed window of WINDOW_MS at least: a window of a few milliseconds measures the clock and the scheduler, not the legs
    n_reps = max(reps, min(MAX_REPS, int(WINDOW_MS / max(_time(legs["stock"], 10), 1e-3))))
    return (n_reps,) + _alternate(legs, n_reps, warmup)


def bench_tails(batch, reps, warmup):
    rows = []
    for h, w, c in TRUNK:
        torch.manual_seed(c + h)
        x, idt = (torch.randn(batch, c, h, w, device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_(True)
                  for _ in range(2))
        gy = torch.randn(batch, c, h, w, device="cuda").contiguous(memory_format=torch.channels_last)
        stock, ours = StockTail(c).cuda().train(), HipTail(c).cuda().train()

        def leg(model):
            def run():
                out = model(x, idt)
                torch.autograd.grad(out, (x, idt, model.bn3.weight, model.bn3.bias), gy)
            return run

        n_reps, best, spread = _measure({"stock": leg(stock), "hip": leg(ours)}, reps, warmup)
        assert ours.bn3._last_kernel == "bn_res_train+relu", ours.bn3._last_kernel
        row = _row("bn_add_relu", batch, h, w, c, n_reps, best, spread, 16 + 32, batchnorm.RES_MIN_ELEMENTS, "bn_res_train+relu")
        print("tail", json.dumps(row), flush=True)
        rows.append(row)
        del x, idt, gy, stock, ours
        torch.cuda.empty_cache()
    return rows


def bench_bn_relu(batch, reps, warmup):
    rows = []
    for h, w, c in INNER:
        torch.manual_seed(c + h)
        x = torch.randn(batch, c, h, w, device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_(True)
        gy = torch.randn(batch, c, h, w, device="cuda").contiguous(memory_format=torch.channels_last)
        stock = nn.Sequential(nn.BatchNorm2d(c), nn.ReLU()).cuda().train()
        ours = nn.Sequential(nn.BatchNorm2d(c), nn.ReLU()).cuda().train()
        assert fusion.use_device_bn_train(ours, min_elements=0) == 1

        def leg(model):
            def run():
                out = model(x)
                torch.autograd.grad(out, (x, model[0].weight, model[0].bias), gy)
            return run

        n_reps, best, spread = _measure({"stock": leg(stock), "hip": leg(ours)}, reps, warmup)
        assert ours[0]._last_kernel == "bn_train+relu", ours[0]._last_kernel
        row = _row("bn_relu", batch, h, w, c, n_reps, best, spread, 12 + 24, batchnorm.MIN_ELEMENTS, "bn_train+relu")
        print("bn_relu", json.dumps(row), flush=True)
        rows.append(row)
        del x, gy, stock, ours
        torch.cuda.empty_cache()
    return rows


class Bottleneck(nn.Module):
    """The hand-wired block of the training net: one shared ReLU, `out += identity`."""

    def __init__(self, cin, width, cout, stride, downsample):
        super().__init__()
        C = cf.conv2d_Q(8, 0.05, 0.25)
        self.conv1, self.bn1 = C(cin, width, 1), nn.BatchNorm2d(width)
        self.conv2, self.bn2 = C(width, width, 3, stride=stride, padding=1), nn.BatchNorm2d(width)
        self.conv3, self.bn3 = C(width, cout, 1), nn.BatchNorm2d(cout)
        self.relu = nn.ReLU()
        self.downsample = nn.Sequential(C(cin, cout, 1, stride=stride), nn.BatchNorm2d(cout)) if downsample else None

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        out += identity
        return self.relu(out)


def stack_model():
    layers = []
    for cin, width, cout, stride in STAGES:
        layers += [Bottleneck(cin, width, cout, stride, True), Bottleneck(cout, width, cout, 1, False)]
    layers += [nn.AdaptiveAvgPool2d(1), nn.Flatten(), cf.linear_Q(8, 0.05, 0.5)(STAGES[-1][2], 100)]
    return nn.Sequential(*layers).cuda().to(memory_format=torch.channels_last)


def bench_step(batch, reps, warmup):
    torch.manual_seed(0)
    model = stack_model().train()
    x = torch.randn(batch, STAGES[0][0], 56, 56, device="cuda").contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 100, (batch,), device="cuda")
    lf = nn.CrossEntropyLoss()
    opt = O.DSGD(model.parameters(), 8, lr=1e-4, momentum=0.9, weight_decay=5e-4)
    prev = cf.options.backward
    cf.options.backward = "hip_all"
    taken = {}

    def one():
        opt.zero_grad(set_to_none=True)
        lf(model(x), y).backward()
        opt.step()

    def stock(m):
        fusion.restore_bn_train(m)

    def bn_train(m):
        fusion.restore_bn_train(m)
        taken["bn_train"] = fusion.use_device_bn_train(m, min_elements=0)

    def bottleneck(m):
        fusion.restore_bn_train(m)
        taken["bottleneck_blocks"] = fusion.use_device_bottleneck_train(m, x, min_elements=0)
        taken["bottleneck_bn_train"] = fusion.use_device_bn_train(m, min_elements=0)

    # the swaps themselves are outside the timed region
    legs = (("stock", stock), ("bn_train", bn_train), ("bottleneck", bottleneck))
    rounds = {name: [] for name, _ in legs}
    kernels = {}
    try:
        for name, prep in legs:
            prep(model)
            for _ in range(warmup):
                one()
        for _ in range(2):
            for name, prep in legs:
                prep(model)
                one()
                torch.cuda.synchronize()
                rounds[name].append(_time(one, reps))
                kinds = [m._last_kernel for m in model.modules() if isinstance(m, fusion.TrainBatchNorm2d)]
                kernels[name] = {k: kinds.count(k) for k in sorted(set(kinds))}
    finally:
        fusion.restore_bn_train(model)
        cf.options.backward = prev
    best = {name: min(v) for name, v in rounds.items()}
    row = {"batch": batch, "backward": "hip_all", "blocks": 2 * len(STAGES), "taken": taken, "kernels": kernels, "reps": reps,
           "stock_ms": round(best["stock"], 3), "bn_train_ms": round(best["bn_train"], 3), "bottleneck_ms": round(best["bottleneck"], 3),
           "speedup_vs_stock": round(best["stock"] / best["bottleneck"], 3),
           "speedup_vs_bn_train": round(best["bn_train"] / best["bottleneck"], 3),
           "stock_spread": round((max(rounds["stock"]) - best["stock"]) / best["stock"], 3),
           "bn_train_spread": round((max(rounds["bn_train"]) - best["bn_train"]) / best["bn_train"], 3)}
    print("step", json.dumps(row), flush=True)
    return row


def rule(rows):
    """The smallest size class from which this class and every larger one passed on every row; None if the largest did not."""
    classes = sorted({r["elements"] for r in rows}, reverse=True)
    floor = None
    for e in classes:
        if not all(r["faster_beyond_spread"] for r in rows if r["elements"] == e):
            break
        floor = e
    return floor


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "bn_res_train_bench.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "batches": a.batches, "reps": a.reps,
           "bytes_per_element": {"bn_add_relu": {"forward": 16, "backward": 32}, "bn_relu": {"forward": 12, "backward": 24}},
           "res_min_elements": batchnorm.RES_MIN_ELEMENTS, "tails": [], "bn_relu": [], "steps": []}
    spin = torch.randn(4096, 4096, device="cuda")   # a second of work before the first window: clocks up, code objects loaded
    for _ in range(200):
        spin = torch.tanh(spin @ spin * 1e-4)
    torch.cuda.synchronize()
    del spin
    for batch in a.batches:
        res["tails"] += bench_tails(batch, a.reps, a.warmup)
    for batch in a.batches:
        res["bn_relu"] += bench_bn_relu(batch, a.reps, a.warmup)
    res["rule"] = {"smallest_passing_class_elements": rule(res["tails"]),
                   "classes": sorted({r["elements"] for r in res["tails"]})}
    print("rule", json.dumps(res["rule"]), flush=True)
    if not a.no_steps:
        try:
            res["steps"].append(bench_step(64, 20, 5))
        except Exception as e:   # a step row that cannot run is recorded, not dropped
            res["steps"].append({"batch": 64, "error": f"{type(e).__name__}: {e}"})
            print("step", json.dumps(res["steps"][-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
