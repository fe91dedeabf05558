#!/usr/bin/env python3
"""Residual add + ReLU in the 1x1 conv's epilogue (slfp_conv2d_fwd_res / fusion.fuse_residual) against the three launches it
replaces.   python profiles/residual_bench.py [--reps 60] [--out profiles/residual_bench.json]

Per layer: conv3 of ResNet-50's four stages (64->256 @56, 128->512 @28, 256->1024 @14, 512->2048 @7) at batch 128 with float32
and with code input, HIP-event times of
    fused    one slfp_conv2d_fwd_res launch
    unfused  slfp_conv2d_fwd_post / slfp_conv2d_fwd_codes (ReLU off) + torch.add + torch.relu   (the parent's code path)
    conv     the conv launch of the unfused sequence alone
alternated in one process, --reps repetitions after warm-up (median and min), and the bytes/s each reaches on its ALGORITHMIC
bytes (computed here from the shapes: X once, W once, every elementwise operand once).
Whole net: the ResNet-50 fixture net (tests/golden/netgen_r3.py) at batch 64 and 128, fuse_bn_relu + fuse_named_bn +
link_codes_traced (A: the parent's best configuration) against the same + fuse_residual (B), legs alternated A/B/A/B in one
process; the spread of the repeated A legs is the yardstick for B - A."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from cnns_slfp_quantization_amd import _lib, fusion, layer_specs  # noqa: E402

dev = torch.device("cuda", 0)
BATCH = 128


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Layer:
    def __init__(self, s, n, gen):
        L = _lib.load()
        self.s, self.n = s, n
        self.d = _lib.ConvDesc(n=n, c_in=s.c_in, h=s.h, w=s.w, c_out=s.c_out, kh=1, kw=1, stride_h=1, stride_w=1, pad_h=0, pad_w=0,
                               dil_h=1, dil_w=1, groups=1, x_layout=_lib.LAYOUT_NHWC, y_layout=_lib.LAYOUT_NHWC, qbits=8,
                               ka=float(np.float32(s.Ka)), kw_scale=float(np.float32(s.Kw)), mfma_passes=_lib.MFMA_F16X1, reserved=0)
        w = torch.randn((s.c_out, s.c_in, 1, 1), generator=gen, device=dev) * (2.0 / s.c_in) ** 0.5
        self.blob = torch.empty(L.slfp_conv2d_wprep_bytes(ctypes.byref(self.d)), dtype=torch.uint8, device=dev)
        _lib.check(L.slfp_conv2d_prepare_weights(ctypes.byref(self.d), w.data_ptr(), self.blob.data_ptr(), None, _stream()))
        self.scale = torch.rand(s.c_out, generator=gen, device=dev) + 0.5
        self.shift = torch.randn(s.c_out, generator=gen, device=dev) * 0.3
        self.xf = torch.relu(torch.randn((n, s.h, s.w, s.c_in), generator=gen, device=dev)) * (6.0 * s.Ka)
        self.xc = torch.empty(self.xf.shape, dtype=torch.uint8, device=dev)
        _lib.check(L.slfp_encode_f32(self.xf.data_ptr(), self.xc.data_ptr(), self.xf.numel(), self.d.ka, _lib.FMT_ACT8 | _lib.FMT_EXT, _stream()))
        self.res = torch.randn((n, s.h, s.w, s.c_out), generator=gen, device=dev)
        self.y = torch.empty_like(self.res)
        self.t = torch.empty_like(self.res)
        self.io = {c: _lib.ConvIo(x_codes=int(c), y_codes=0, y_ka=1.0, y_qbits=8) for c in (False, True)}

    def conv(self, codes):
        L = _lib.load()
        if codes:
            _lib.check(L.slfp_conv2d_fwd_codes(ctypes.byref(self.d), ctypes.byref(self.io[True]), self.xc.data_ptr(), self.blob.data_ptr(), None,
                                               self.scale.data_ptr(), self.shift.data_ptr(), 0, self.y.data_ptr(), _stream()))
        else:
            _lib.check(L.slfp_conv2d_fwd_post(ctypes.byref(self.d), self.xf.data_ptr(), self.blob.data_ptr(), None, self.scale.data_ptr(),
                                              self.shift.data_ptr(), 0, self.y.data_ptr(), None, None, _stream()))

    def unfused(self, codes):
        self.conv(codes)
        return torch.relu(self.y + self.res)   # nn.ReLU() of these blocks is not in place: two new tensors, as in the net

    def fused(self, codes):
        x = self.xc if codes else self.xf
        _lib.check(_lib.load().slfp_conv2d_fwd_res(ctypes.byref(self.d), ctypes.byref(self.io[codes]), x.data_ptr(), self.blob.data_ptr(), None,
                                                   self.scale.data_ptr(), self.shift.data_ptr(), 1, self.res.data_ptr(), self.t.data_ptr(),
                                                   None, _stream()))
        return self.t


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)   # us
    return out


def layer_table(reps):
    gen = torch.Generator(device=dev).manual_seed(11)
    rows = []
    for c_in, hw in ((64, 56), (128, 28), (256, 14), (512, 7)):
        s = next(s for s in layer_specs.conv_layers("resnet50_imagenet224")
                 if s.k == (1, 1) and s.stride == (1, 1) and s.c_in == c_in and s.c_out == 4 * c_in and s.h == hw)
        lay = Layer(s, BATCH, gen)
        px = BATCH * s.h * s.w
        for codes in (False, True):
            assert torch.equal(lay.fused(codes), lay.unfused(codes))
            legs = {"fused": [], "unfused": [], "conv": []}
            fns = {"fused": lambda: lay.fused(codes), "unfused": lambda: lay.unfused(codes), "conv": lambda: lay.conv(codes)}
            for k in fns:
                timed(fns[k], 3)
            for _ in range(reps):   # alternated: one repetition of each leg per round
                for k in ("fused", "unfused", "conv"):
                    legs[k] += timed(fns[k], 1, warm=0)
            xb = px * s.c_in * (1 if codes else 4)
            wb = s.c_in * s.c_out * 2
            yb = px * s.c_out * 4
            alg = {"fused": xb + wb + 2 * yb, "unfused": xb + wb + yb + 3 * yb + 2 * yb, "conv": xb + wb + yb}
            row = {"layer": f"{s.c_in}->{s.c_out}@{s.h}", "batch": BATCH, "codes_in": codes, "reps": reps}
            for k, v in legs.items():
                med = statistics.median(v)
                row[k + "_us_median"], row[k + "_us_min"] = round(med, 2), round(min(v), 2)
                row[k + "_alg_bytes"] = alg[k]
                row[k + "_TBps"] = round(alg[k] / med / 1e6, 3)
            row["fused_vs_unfused"] = round(row["fused_us_median"] / row["unfused_us_median"], 3)
            row["fused_vs_conv"] = round(row["fused_us_median"] / row["conv_us_median"], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del lay
        torch.cuda.empty_cache()
    return rows


def build_net(batch):
    import netgen_r3 as ng
    import utils.conv2d_func as cf
    import utils.sfp_quant as sq
    gold = np.load(os.path.join(ROOT, "tests", "golden", "nets_r3_golden.npz"))
    q, _, in_seed, seed = [int(v) for v in gold["resnet50:meta"]]
    manifest = json.loads(bytes(gold["resnet50:manifest"]).decode())
    gains = json.loads(bytes(gold["resnet50:gains"]).decode())
    m = ng.BUILDERS["resnet50"](ng.Factories(cf, q, manifest, layerout=sq.layerout_quantize_func))
    ng.fill_parameters_by_name(m, seed, gains)
    ng.load_bn_stats_by_name_(m, {k[len("resnet50") + 1:]: gold[k] for k in gold.files if k.startswith("resnet50:bn:")})
    x = ng.net_input224(4, in_seed).repeat((batch + 3) // 4, 1, 1, 1)[:batch]
    return m.to(dev).eval().to(memory_format=torch.channels_last), x.to(dev).contiguous(memory_format=torch.channels_last)


def net_rate(m, x, steps, warm=3):
    with torch.no_grad():
        for _ in range(warm):
            m(x)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            m(x)
        b.record()
        b.synchronize()
    return x.shape[0] * steps / (a.elapsed_time(b) * 1e-3)


def whole_net(batch, rounds, steps):
    m, x = build_net(batch)
    with torch.no_grad():
        n_f = fusion.fuse_bn_relu(m) + fusion.fuse_named_bn(m, example_input=x)
        y0 = m(x)
        n_l = fusion.link_codes_traced(m, x)
        legs = {"A": [], "B": []}
        same = True
        for _ in range(rounds):
            legs["A"].append(net_rate(m, x, steps))                 # the parent's best configuration
            n_r = fusion.fuse_residual(m, x)
            same = same and bool(torch.equal(m(x), y0))
            legs["B"].append(net_rate(m, x, steps))                 # + fuse_residual
            assert fusion.unfuse_residual(m) == n_r
    a, b = statistics.median(legs["A"]), statistics.median(legs["B"])
    row = {"net": "resnet50 (fixture)", "batch": batch, "bn_pairs": n_f, "code_links": n_l, "residual_blocks": n_r, "steps": steps,
           "A_images_per_s": [round(v, 1) for v in legs["A"]], "B_images_per_s": [round(v, 1) for v in legs["B"]],
           "A_median": round(a, 1), "B_median": round(b, 1), "A_spread": round(max(legs["A"]) - min(legs["A"]), 1),
           "gain": round(b / a - 1.0, 4), "B_beats_A_by_more_than_the_spread": bool(min(legs["B"]) - max(legs["A"]) > 0 and b - a > max(legs["A"]) - min(legs["A"])),
           "logits_bit_identical": same,
           # what the removed traffic predicts: 16 B x 5 519 360 trunk elements per image at the HBM rate the elementwise kernels reach
           "removed_bytes_per_image": 16 * 5519360}
    print(json.dumps(row), flush=True)
    del m
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--skip-layers", action="store_true", help="whole-net legs only (cache-policy A/Bs of two builds)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "residual_bench.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "layers": [] if a.skip_layers else layer_table(a.reps),
           "whole_net": [whole_net(b, a.rounds, a.steps) for b in (64, 128)]}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
