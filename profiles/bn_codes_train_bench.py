"""A QAT step's hand-over BatchNorm2d -> ReLU -> Conv2d_Q on 1-byte codes (fusion.link_codes_train) against the same three
modules on today's kernels and against the stock modules.  DESIGN.md section 35.

    python profiles/bn_codes_train_bench.py [--reps 20] [--out profiles/bn_codes_train_bench.json] [--no-steps]

Per hand-over shape of mobilenetv1_imagenet224 (the 26 Conv2d_Q layers behind a BatchNorm + ReLU; equal shapes once, `layers` counts
them) at batch 128, channels_last, options.backward = "hip": forward + backward of [BatchNorm2d, ReLU, Conv2d_Q] with gradients for
x, gamma, beta and the conv weight, timed with HIP events after warm-up, the three legs alternated twice in one process:
    linked     fusion.link_codes_train(min_elements=0): slfp_bn_codes_train_fwd, the conv's code-reading forward,
               slfp_conv2d_bwd_codes, slfp_bn_codes_train_bwd
    unlinked   fusion.use_device_bn_train(min_elements=0): slfp_bn_train_fwd / _bwd, the float32 conv forward, slfp_conv2d_bwd_ex
    stock      nn.BatchNorm2d and nn.ReLU (MIOpen, ATen) around the same Conv2d_Q
Each leg's time is the better of its two rounds, its spread the round-to-round difference relative to that.  A row is
`faster_beyond_spread` if the linked leg is below the BETTER of the other two by more than that leg's spread.  `rule` applies the
spread rule of DESIGN sections 27 / 32 to the rows: the smallest size class (elements of the BatchNorm's tensor) from which this
class and every larger one has only such rows; null if no class does.
Whole step: forward + backward + DSGD of backward_bench.py's Conv2d_Q + BN + ReLU stack, options.backward = "hip", batch 128:
the parent's best configuration (fusion.use_device_bn_train with its default rule) against the same with all 26 hand-overs linked
(min_elements=0) and with the default rule (batchnorm.CODES_MIN_ELEMENTS), with torch.cuda.max_memory_allocated of each.
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
from bn_train_bench import _alternate  # noqa: E402
from cnns_slfp_quantization_amd import batchnorm, fusion, layer_specs, optimizer as O  # noqa: E402
from cnns_slfp_quantization_amd import conv2d_func as cf  # noqa: E402

NET = "mobilenetv1_imagenet224"
LINKED = "bn_codes_train+relu"


def _block(s):
    conv = cf.conv2d_Q(8, s.Kw, s.Ka)(s.c_in, s.c_out, s.k, stride=s.stride, padding=s.pad, groups=s.groups)
    return torch.nn.Sequential(torch.nn.BatchNorm2d(s.c_in), torch.nn.ReLU(inplace=True), conv).cuda().train()


def bench_handovers(batch, reps, warmup):
    specs = layer_specs.conv_layers(NET)[1:]   # every conv but the stem reads a BatchNorm + ReLU
    geometry = lambda s: (s.c_in, s.c_out, s.h, s.w, s.k, s.stride, s.groups)
    shapes = collections.Counter(geometry(s) for s in specs)
    first = {}
    for s in specs:
        first.setdefault(geometry(s), s)   # equal shapes once, with the scales of the first such layer
    rows = []
    for key, count in shapes.items():
        s = first[key]
        torch.manual_seed(s.c_in + s.h)
        x = torch.randn(batch, s.c_in, s.h, s.w, device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_(True)
        gy = torch.randn(batch, s.c_out, s.h_out, s.w_out, device="cuda").contiguous(memory_format=torch.channels_last)
        stock, unlinked, linked = _block(s), _block(s), _block(s)
        for m in (unlinked, linked):
            m.load_state_dict(stock.state_dict())
        assert fusion.use_device_bn_train(unlinked, min_elements=0) == 1
        assert fusion.link_codes_train(linked, min_elements=0) == 1

        def leg(model):
            bn, conv = model[0], model[2]

            def run():
                out = model(x)
                torch.autograd.grad(out, (x, bn.weight, bn.bias, conv.weight), gy)
            return run

        best, spread = _alternate({"stock": leg(stock), "unlinked": leg(unlinked), "linked": leg(linked)}, reps, warmup)
        assert linked[0]._last_kernel == LINKED and "+codes_in" in linked[2]._last_kernel, (linked[0]._last_kernel, linked[2]._last_kernel)
        assert unlinked[0]._last_kernel == "bn_train+relu" and linked[2]._last_bwd_kernel == unlinked[2]._last_bwd_kernel != "composite"
        other = min(("unlinked", "stock"), key=lambda k: best[k])
        elements = batch * s.c_in * s.h * s.w
        row = {"c_in": s.c_in, "c_out": s.c_out, "h": s.h, "w": s.w, "k": s.k[0], "stride": s.stride[0], "groups": s.groups,
               "layers": count, "elements": elements, "fwd_kernel": linked[2]._last_kernel, "bwd_kernel": linked[2]._last_bwd_kernel,
               "stock_ms": round(best["stock"], 4), "unlinked_ms": round(best["unlinked"], 4), "linked_ms": round(best["linked"], 4),
               "stock_spread": round(spread["stock"], 3), "unlinked_spread": round(spread["unlinked"], 3),
               "linked_spread": round(spread["linked"], 3), "better_unlinked_leg": other,
               "speedup_vs_better": round(best[other] / best["linked"], 3),
               "faster_beyond_spread": bool(best["linked"] < best[other] * (1 - spread[other]))}
        print("handover", json.dumps(row), flush=True)
        rows.append(row)
        del x, gy, stock, unlinked, linked
        torch.cuda.empty_cache()
    return rows


def spread_rule(rows):
    """The smallest size class from which this class and every larger measured one has only rows faster beyond the spread."""
    classes = sorted({r["elements"] for r in rows}, reverse=True)
    rule = None
    for e in classes:
        if not all(r["faster_beyond_spread"] for r in rows if r["elements"] == e):
            break
        rule = e
    return rule


def bench_step(batch, reps, warmup):
    torch.manual_seed(0)
    model, s0 = backward_bench.stack_model(NET)
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

    def parent_best(m):
        fusion.restore_bn_train(m)   # takes the links along
        fusion.use_device_bn_train(m)

    def linked(floor):
        def prep(m):
            parent_best(m)
            fusion.link_codes_train(m, min_elements=floor)
        return prep

    legs = {"parent_best": parent_best, "linked_all": linked(0), "linked_default": linked(None)}
    rounds, peak, on_codes = {k: [] for k in legs}, {}, {}
    for name, prep in legs.items():   # the swaps are outside the timed region
        prep(model)
        for _ in range(warmup):
            one()
    for _ in range(2):
        for name, prep in legs.items():
            prep(model)
            one()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            rounds[name].append(_time(one, reps))
            peak[name] = torch.cuda.max_memory_allocated()
            on_codes[name] = sum(getattr(m, "_last_kernel", "") == LINKED for m in model.modules())
    fusion.restore_bn_train(model)
    cf.options.backward = "composite"
    best = {k: min(v) for k, v in rounds.items()}
    row = {"net": NET, "batch": batch, "backward": "hip", "handovers_on_codes": on_codes,
           "ms": {k: round(v, 3) for k, v in best.items()},
           "spread": {k: round((max(v) - min(v)) / min(v), 3) for k, v in rounds.items()},
           "max_memory_allocated_mib": {k: round(v / 2 ** 20, 1) for k, v in peak.items()},
           "speedup_linked_all": round(best["parent_best"] / best["linked_all"], 3),
           "speedup_linked_default": round(best["parent_best"] / best["linked_default"], 3)}
    print("step", json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "bn_codes_train_bench.json"))
    a = ap.parse_args()
    cf.options.backward = "hip"
    res = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "reps": a.reps, "backward": "hip",
           "algorithmic_bytes_per_element_not_measured": {"bn_forward": [12, 9], "reader_forward_read": [4, 1], "reader_gw_read": [4, 1],
                                                          "bn_backward": [28, 20], "saved_for_backward": [8, 5]},
           "codes_min_elements_in_effect": batchnorm.CODES_MIN_ELEMENTS}
    res["handovers"] = bench_handovers(a.batch, a.reps, a.warmup)
    res["rule"] = {"codes_min_elements_by_the_spread_rule": spread_rule(res["handovers"]),
                   "rows_faster_beyond_spread": sum(r["faster_beyond_spread"] for r in res["handovers"]), "rows": len(res["handovers"])}
    print("rule", json.dumps(res["rule"]), flush=True)
    res["steps"] = [] if a.no_steps else [bench_step(a.batch, max(5, a.reps // 2), 3)]
    cf.options.backward = "composite"
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
