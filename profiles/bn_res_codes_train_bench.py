"""A QAT step's trunk hand-over of ResNet-50 on 1-byte codes: the bn3 tail of a Bottleneck that writes the float32 trunk AND its
readers' codes (slfp_bn_res_codes_train_fwd), read by the next block's conv1 (and downsample.0) through their code-reading forward
and slfp_conv2d_bwd_codes, against the same modules unlinked.  DESIGN.md section 38.

    python profiles/bn_res_codes_train_bench.py [--reps 20 (at least)] [--out profiles/bn_res_codes_train_bench.json] [--no-steps]

(a) `trunks`: the trunk shapes of ResNet-50 at batch 64 and 128, channels_last, options.backward = "hip_all": forward + backward of
[bn3 tail, next conv1] ("plain": conv1 C -> C/4) and, for the three shapes in front of a stage boundary, of [bn3 tail, next conv1,
downsample.0] ("boundary": conv1 C -> C/2, downsample.0 C -> 2C of stride 2), with gradients for the tail's x, identity, gamma and
beta and for the conv weights.  Timed with HIP events after warm-up, every window at least 150 ms long, the three legs alternated
twice in one process (the method of bn_res_train_bench.py):
    linked     slfp_bn_res_codes_train_fwd, the readers' code forward, slfp_conv2d_bwd_codes, slfp_bn_res_train_bwd (every size)
    unlinked   fusion.TrainBatchNorm2d(residual=, relu=True) with its default rule (batchnorm.RES_MIN_ELEMENTS: the residual kernels
               from 24 M elements on, ATen below), float32 readers, slfp_conv2d_bwd_ex: what use_device_bottleneck_train leaves
    stock      nn.BatchNorm2d, `+=`, nn.ReLU around the same Conv2d_Q readers
Each leg's time is the better of its two rounds, its spread the round-to-round difference relative to that.  A row is
`faster_beyond_spread` if the linked leg is below the BETTER of the other two by more than that leg's spread.  `rule` applies the
spread rule of DESIGN sections 27-35: the smallest size class (elements of the trunk) from which this class and every larger one
has only such rows; null if no class does.  batchnorm.RES_CODES_MIN_ELEMENTS is what two runs of this script agree on.
(b) `steps`: forward + backward + DSGD of bn_res_train_bench.py's Bottleneck stack at batch 64, options.backward = "hip_all", with
torch.cuda.max_memory_allocated, under unlinked / in-block links only / trunk links only / both, each with the default rules
(min_elements=None) and with every size on the kernels (min_elements=0).
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
from bn_res_train_bench import STAGES, TRUNK, StockTail, _measure, stack_model  # noqa: E402
from cnns_slfp_quantization_amd import batchnorm, fusion, optimizer as O  # noqa: E402
from cnns_slfp_quantization_amd import conv2d_func as cf  # noqa: E402

KA, KW = 0.25, 0.05   # the nominal scales of bn_res_train_bench.py's stack
# ((h, w, c) of the trunk, ((c_out, stride) of each reader))
PLAIN = tuple(((h, w, c), ((c // 4, 1),)) for h, w, c in TRUNK)
BOUNDARY = tuple(((h, w, c), ((c // 2, 1), (2 * c, 2))) for h, w, c in TRUNK[:3])


class Trunk(nn.Module):
    """A tail and the Conv2d_Q layers that read its output.  kind: "stock" | "unlinked" | "linked"."""

    def __init__(self, c, readers, kind):
        super().__init__()
        C = cf.conv2d_Q(8, KW, KA)
        self.readers = nn.ModuleList(C(c, c_out, 1, stride=stride) for c_out, stride in readers)
        self.kind = kind
        if kind == "stock":
            self.tail = StockTail(c)
        else:
            self.bn3 = fusion.TrainBatchNorm2d(nn.BatchNorm2d(c), 0 if kind == "linked" else None)
            if kind == "linked":   # what link_bottleneck_codes_train(min_elements=0) records on a block's bn3
                self.bn3._trunk = (tuple(self.readers), cf._f32(self.readers[0].Ka), 8, 0)

    @property
    def bn(self):
        return self.tail.bn3 if self.kind == "stock" else self.bn3

    def forward(self, out, identity):
        t = self.tail(out, identity) if self.kind == "stock" else self.bn3(out, residual=identity, relu=True)
        return [r(t) for r in self.readers]


def bench_trunks(batch, reps, warmup):
    rows = []
    for where, shapes in (("plain", PLAIN), ("boundary", BOUNDARY)):
        for (h, w, c), readers in shapes:
            torch.manual_seed(c + h)
            x, idt = (torch.randn(batch, c, h, w, device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_(True)
                      for _ in range(2))
            models = {k: Trunk(c, readers, k).cuda().train() for k in ("stock", "unlinked", "linked")}
            for m in models.values():
                m.load_state_dict(models["stock"].state_dict(), strict=False)
            with torch.no_grad():
                gys = [torch.randn_like(o) for o in models["stock"](x, idt)]

            def leg(model):
                params = (x, idt, model.bn.weight, model.bn.bias) + tuple(r.weight for r in model.readers)

                def run():
                    torch.autograd.grad(model(x, idt), params, gys)
                return run

            n_reps, best, spread = _measure({k: leg(m) for k, m in models.items()}, reps, warmup)
            linked, unlinked = models["linked"], models["unlinked"]
            assert linked.bn3._last_kernel == "bn_res_codes_train+relu", linked.bn3._last_kernel
            assert all("+codes_in" in r._last_kernel and r._last_bwd_kernel != "composite" for r in linked.readers)
            assert [r._last_bwd_kernel for r in linked.readers] == [r._last_bwd_kernel for r in unlinked.readers]
            best = {k: round(v, 5) for k, v in best.items()}       # the row's flag is a function of the figures it prints
            spread = {k: round(v, 4) for k, v in spread.items()}
            other = min(("unlinked", "stock"), key=lambda k: best[k])
            elements = batch * c * h * w
            row = {"where": where, "batch": batch, "h": h, "w": w, "c": c, "readers": [list(r) for r in readers], "elements": elements,
                   "reps": n_reps, "unlinked_tail": unlinked.bn3._last_kernel, "bwd_kernels": [r._last_bwd_kernel for r in linked.readers],
                   "stock_ms": best["stock"], "unlinked_ms": best["unlinked"], "linked_ms": best["linked"],
                   "stock_spread": spread["stock"], "unlinked_spread": spread["unlinked"], "linked_spread": spread["linked"],
                   "better_unlinked_leg": other,
                   "speedup_vs_better": round(best[other] / best["linked"], 3),
                   "faster_beyond_spread": bool(best["linked"] < best[other] * (1 - spread[other]))}
            print("trunk", json.dumps(row), flush=True)
            rows.append(row)
            del x, idt, gys, models
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
    model = stack_model().train()
    x = torch.randn(batch, STAGES[0][0], 56, 56, device="cuda").contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 100, (batch,), device="cuda")
    lf = nn.CrossEntropyLoss()
    opt = O.DSGD(model.parameters(), 8, lr=1e-4, momentum=0.9, weight_decay=5e-4)
    prev = cf.options.backward
    cf.options.backward = "hip_all"
    links = {}

    def one():
        opt.zero_grad(set_to_none=True)
        lf(model(x), y).backward()
        opt.step()

    def setting(name, floor, in_block, trunk):
        def prep(m):
            fusion.restore_bn_train(m)   # takes blocks and links along
            assert fusion.use_device_bottleneck_train(m, x, min_elements=floor) == 2 * len(STAGES)
            fusion.use_device_bn_train(m, min_elements=floor)
            if in_block or trunk:
                links[name] = list(fusion.link_bottleneck_codes_train(m, x, min_elements=floor, in_block=in_block, trunk=trunk))
        return prep

    legs = {}
    for rule, floor in (("default", None), ("all", 0)):
        for name, in_block, trunk in (("unlinked", False, False), ("in_block", True, False), ("trunk", False, True), ("both", True, True)):
            legs[f"{name}_{rule}"] = setting(f"{name}_{rule}", floor, in_block, trunk)
    rounds, peak, on_codes = {k: [] for k in legs}, {}, {}
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
                kinds = [getattr(m, "_last_kernel", None) for m in model.modules()]
                on_codes[name] = {"in_block": kinds.count("bn_codes_train+relu"), "trunk": kinds.count("bn_res_codes_train+relu")}
    finally:
        fusion.restore_bn_train(model)
        cf.options.backward = prev
    best = {k: min(v) for k, v in rounds.items()}
    row = {"batch": batch, "backward": "hip_all", "blocks": 2 * len(STAGES), "reps": reps, "links_made": links, "on_codes": on_codes,
           "ms": {k: round(v, 3) for k, v in best.items()},
           "spread": {k: round((max(v) - min(v)) / min(v), 3) for k, v in rounds.items()},
           "max_memory_allocated_mib": {k: round(v / 2 ** 20, 1) for k, v in peak.items()}}
    print("step", json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "bn_res_codes_train_bench.json"))
    a = ap.parse_args()
    prev = cf.options.backward
    cf.options.backward = "hip_all"
    res = {"device": torch.cuda.get_device_name(0), "batches": a.batches, "reps": a.reps, "backward": "hip_all",
           "algorithmic_bytes_per_element_not_measured": {"bn3_tail_forward": [16, 17], "reader_forward_read": [4, 1],
                                                          "reader_gw_read": [4, 1], "bn3_tail_backward": [32, 32],
                                                          "saved_for_backward_trunk": [8, 9]},
           "res_codes_min_elements_in_effect": batchnorm.RES_CODES_MIN_ELEMENTS, "trunks": [], "steps": []}
    spin = torch.randn(4096, 4096, device="cuda")   # a second of work before the first window: clocks up, code objects loaded
    for _ in range(200):
        spin = torch.tanh(spin @ spin * 1e-4)
    torch.cuda.synchronize()
    del spin
    for batch in a.batches:
        res["trunks"] += bench_trunks(batch, a.reps, a.warmup)
    res["rule"] = {"res_codes_min_elements_by_the_spread_rule": spread_rule(res["trunks"]),
                   "rows_faster_beyond_spread": sum(r["faster_beyond_spread"] for r in res["trunks"]), "rows": len(res["trunks"])}
    print("rule", json.dumps(res["rule"]), flush=True)
    cf.options.backward = prev
    if not a.no_steps:
        try:
            res["steps"].append(bench_step(64, 10, 3))
        except Exception as e:   # a step row that cannot run is recorded, not dropped
            res["steps"].append({"batch": 64, "error": f"{type(e).__name__}: {e}"})
            print("step", json.dumps(res["steps"][-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
