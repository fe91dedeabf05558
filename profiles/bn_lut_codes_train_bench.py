"""A QAT step's hand-over BatchNorm2d -> layerout_quantize_func -> Swish | GELU -> Conv2d_Q on 1-byte codes
(fusion.link_layerout_codes_train) against the same four modules on today's table kernels and against the stock modules.
DESIGN.md section 41.

    python profiles/bn_lut_codes_train_bench.py [--reps 20] [--out profiles/bn_lut_codes_train_bench.json] [--no-steps]

Per hand-over shape of bn_layerout_train_bench.py's shape set (vgg16_cifar32 with GELU, mobilenetv1_cifar32 and
mobilenetv1_imagenet224 with Swish; batch 128 and 256) that has a Conv2d_Q reader directly behind the activation -- every layer but
the last of a net and, in VGG, but the last of a stage, whose reader stands behind a MaxPool2d --, the reader taken from that net
(equal shapes once, `layers` counts them), channels_last: forward + backward of [BatchNorm2d, layerout_quantize_func, act, Conv2d_Q]
with gradients for x, gamma, beta and the conv weight, timed with HIP events after warm-up, every window at least WINDOW_MS long, the
three legs alternated twice in one process:
    linked     fusion.link_layerout_codes_train(min_elements=0): slfp_bn_lut_codes_train_fwd, the conv's code-reading forward,
               slfp_conv2d_bwd_codes, slfp_bn_lut_train_bwd
    unlinked   fusion.use_device_bn_layerout_train(min_elements=0): slfp_bn_lut_train_fwd / _bwd, the float32 conv forward,
               slfp_conv2d_bwd_ex
    stock      nn.BatchNorm2d, the quantizer and the activation modules (MIOpen, ATen) around the same Conv2d_Q
options.backward is "hip" for the MobileNets and "hip_all" for VGG (its dense 3 x 3 readers have a backward kernel only there).
Each leg's time is the better of its two rounds, its spread the round-to-round difference relative to that.  A row is
`faster_beyond_spread` if the linked leg is below the BETTER of the other two by more than that leg's spread.  `rule` applies the
spread rule of DESIGN sections 27 / 32 / 35 to the rows: the smallest size class (elements of the BatchNorm's tensor) from which this
class and every larger one has only such rows; null if no class does.  The benchmark is run twice and the constant
batchnorm.LUT_CODES_MIN_ELEMENTS admits a class only if it passes in both files.
Whole step: forward + backward + DSGD of bn_layerout_train_bench.py's [Conv2d_Q, BN, layerout, act] stacks at batch 128,
mobilenetv1_cifar32 under options.backward = "hip" and vgg16_cifar32 under "hip_all": the parent's configurations
(fusion.use_device_bn_layerout_train with its default rule and with min_elements=0; the better is `parent_best`) against the
min_elements=0 one plus the links under the default rule (batchnorm.LUT_CODES_MIN_ELEMENTS) and plus all links (min_elements=0),
with torch.cuda.max_memory_allocated of each.
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
import bn_layerout_train_bench as LB  # noqa: E402
from backward_bench import _time  # noqa: E402
from bn_train_bench import _alternate  # noqa: E402
from cnns_slfp_quantization_amd import batchnorm, fusion, optimizer as O  # noqa: E402
from cnns_slfp_quantization_amd import conv2d_func as cf  # noqa: E402

LINKED = "bn_lut_codes_train"
WINDOW_MS = 40.0
MAX_REPS = 400
BACKWARD = {"vgg16_cifar32": "hip_all", "mobilenetv1_cifar32": "hip", "mobilenetv1_imagenet224": "hip"}


def handovers(net):
    """(producer ConvSpec, reader ConvSpec, h, w of the tensor between them) for every layer of `net` whose output is read by the
    next Conv2d_Q directly: the reader's input side equals the producer's output side (otherwise a pool stands between them)."""
    specs = LB._specs(net)
    out = []
    for (s, _, ho), (r, r_hin, _) in zip(specs, specs[1:]):
        if r_hin == ho and r.c_in == s.c_out:
            out.append((s, r, ho, ho * s.w_out // s.h_out))
    return out


def _block(net, c, reader):
    conv = cf.conv2d_Q(8, reader.Kw, reader.Ka)(reader.c_in, reader.c_out, reader.k, stride=reader.stride, padding=reader.pad,
                                                 groups=reader.groups)
    return torch.nn.Sequential(*LB._tail(c, LB.NETS[net][2]), conv).cuda().train()


def bench_handovers(net, batch, reps, warmup):
    cf.options.backward = BACKWARD[net]
    geometry = lambda h: (h[2], h[3], h[1].c_in, h[1].c_out, h[1].k, h[1].stride, h[1].groups)
    found = handovers(net)
    shapes = collections.Counter(geometry(h) for h in found)
    first = {}
    for h in found:
        first.setdefault(geometry(h), h)   # equal shapes once, with the scales of the first such reader
    rows = []
    for key, count in shapes.items():
        _, r, h, w = first[key]
        c = r.c_in
        torch.manual_seed(c + h)
        x = torch.randn(batch, c, h, w, device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_(True)
        stock, unlinked, linked = _block(net, c, r), _block(net, c, r), _block(net, c, r)
        for m in (unlinked, linked):
            m.load_state_dict(stock.state_dict())
        assert fusion.use_device_bn_layerout_train(unlinked, min_elements=0) == 1
        assert fusion.link_layerout_codes_train(linked, min_elements=0) == 1
        with torch.no_grad():
            gy = torch.randn_like(stock(x.detach()))

        def leg(model):
            bn, conv = model[0], model[3]

            def run():
                out = model(x)
                torch.autograd.grad(out, (x, bn.weight, bn.bias, conv.weight), gy)
            return run

        legs = {"stock": leg(stock), "unlinked": leg(unlinked), "linked": leg(linked)}
        for fn in legs.values():
            for _ in range(warmup):
                fn()
        # a timed window of WINDOW_MS at least: a window of a few milliseconds measures the clock and the scheduler, not the legs
        n_reps = max(reps, min(MAX_REPS, int(WINDOW_MS / max(_time(legs["unlinked"], 5), 1e-3))))
        best, spread = _alternate(legs, n_reps, warmup)
        assert linked[0]._last_kernel == LINKED and "+codes_in" in linked[3]._last_kernel, (linked[0]._last_kernel, linked[3]._last_kernel)
        assert unlinked[0]._last_kernel == "bn_lut_train" and linked[3]._last_bwd_kernel == unlinked[3]._last_bwd_kernel != "composite"
        other = min(("unlinked", "stock"), key=lambda k: best[k])
        elements = batch * c * h * w
        row = {"net": net, "act": LB.NETS[net][2].__name__, "batch": batch, "backward": BACKWARD[net], "c_in": c, "c_out": r.c_out,
               "h": h, "w": w, "k": r.k[0], "stride": r.stride[0], "groups": r.groups, "layers": count, "elements": elements,
               "reps": n_reps, "fwd_kernel": linked[3]._last_kernel, "bwd_kernel": linked[3]._last_bwd_kernel,
               "stock_ms": round(best["stock"], 4), "unlinked_ms": round(best["unlinked"], 4), "linked_ms": round(best["linked"], 4),
               "stock_spread": round(spread["stock"], 3), "unlinked_spread": round(spread["unlinked"], 3),
               "linked_spread": round(spread["linked"], 3), "better_unlinked_leg": other,
               "speedup_vs_better": round(best[other] / best["linked"], 3),
               "faster_beyond_spread": bool(round(best["linked"], 4) < round(best[other], 4) * (1 - round(spread[other], 3)))}
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


def bench_step(net, batch, reps, warmup):
    torch.manual_seed(0)
    model, side = LB.stack_model(net)
    model.train()
    x = torch.randn(batch, 3, side, side, device="cuda").contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 100, (batch,), device="cuda")
    lf = torch.nn.CrossEntropyLoss()
    opt = O.DSGD(model.parameters(), 8, lr=1e-4, momentum=0.9, weight_decay=5e-4)
    cf.options.backward = BACKWARD[net]

    def one():
        opt.zero_grad(set_to_none=True)
        lf(model(x), y).backward()
        opt.step()

    def parent(floor):
        def prep(m):
            fusion.restore_bn_layerout_train(m)   # takes the links along
            fusion.use_device_bn_layerout_train(m, min_elements=floor)
        return prep

    def linked(floor):
        def prep(m):
            parent(0)(m)
            fusion.link_layerout_codes_train(m, min_elements=floor)
        return prep

    # the parent's two configurations (the table kernels under their default size rule, and at every size); the links on the latter
    legs = {"parent_default": parent(None), "parent_all": parent(0), "linked_default": linked(None), "linked_all": linked(0)}
    rounds, peak, on_codes, links = {k: [] for k in legs}, {}, {}, {}
    try:
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
                links[name] = sum(isinstance(m, fusion.TrainBatchNormLayeroutCodes2d) for m in model.modules())
    finally:
        fusion.restore_bn_layerout_train(model)
        cf.options.backward = "composite"
    best = {k: min(v) for k, v in rounds.items()}
    best["parent_best"] = min(best["parent_default"], best["parent_all"])
    row = {"net": net, "batch": batch, "backward": BACKWARD[net], "links": links,
           "parent_best_is": min(("parent_default", "parent_all"), key=lambda k: best[k]), "handovers_on_codes": on_codes,
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
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "bn_lut_codes_train_bench.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "batches": a.batches, "reps": a.reps, "backward": BACKWARD,
           "algorithmic_bytes_per_element_not_measured": {"bn_forward": [12, 9], "reader_forward_read": [4, 1], "reader_gw_read": [4, 1],
                                                          "bn_backward": [20, 20], "saved_for_backward": [8, 5]},
           "lut_codes_min_elements_in_effect": batchnorm.LUT_CODES_MIN_ELEMENTS, "handovers": [], "steps": []}
    spin = torch.randn(4096, 4096, device="cuda")   # a second of work before the first window: clocks up, code objects loaded
    for _ in range(200):
        spin = torch.tanh(spin @ spin * 1e-4)
    torch.cuda.synchronize()
    del spin
    for batch in a.batches:
        for net in LB.NETS:
            res["handovers"] += bench_handovers(net, batch, a.reps, a.warmup)
    res["rule"] = {"lut_codes_min_elements_by_the_spread_rule": spread_rule(res["handovers"]),
                   "rows_faster_beyond_spread": sum(r["faster_beyond_spread"] for r in res["handovers"]), "rows": len(res["handovers"])}
    print("rule", json.dumps(res["rule"]), flush=True)
    if not a.no_steps:
        for net in ("mobilenetv1_cifar32", "vgg16_cifar32"):
            try:
                res["steps"].append(bench_step(net, 128, 30, 5))
            except Exception as e:   # a step row that cannot run is recorded, not dropped
                res["steps"].append({"net": net, "batch": 128, "error": f"{type(e).__name__}: {e}"})
                print("step", json.dumps(res["steps"][-1]), flush=True)
    cf.options.backward = "composite"
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
