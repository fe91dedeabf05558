#!/usr/bin/env python3
"""The global average pool kernel (csrc/pool_avg.hip, slfp_global_avgpool_f32) against the ATen pool it can replace, on the MI355X.
Writes profiles/avgpool_bench.json (--out: elsewhere).

  pool    the pool alone at ResNet-50's 7 x 7 x 2048, MobileNetV1's 7 x 7 x 1024 and SqueezeNet's 13 x 13 x 1000, batch 1, 8, 64 and
          256, channels_last, and at batch 64 also contiguous NCHW.  Leg A = F.adaptive_avg_pool2d on the tensor (what the nets run
          without fusion.use_device_avgpool); SqueezeNet: also leg A' = its separate torch.relu pass + the pool, against the kernel
          with relu = 1.  Leg B = the kernel, float32 out; leg C = the kernel, codes out.  Before anything is timed B is compared
          with A under the bound 2 (HW + 1) 2^-24 mean64(|x|) and C with slfp_encode_f32 of B.
  head    ResNet-50's avgpool -> flatten -> fc (2048 -> 1000) under options.linear_kernel = "fc": the ATen pool + the float32
          weight-streaming Linear_Q against the pair linked by fusion.use_device_avgpool + fusion.link_pool_head.  Through eager
          modules both legs are bound by the host at every batch (the same time from batch 1 to 256), so
  head_c_abi   the same head as calls of the C ABI: ATen pool + slfp_linear_fwd_fc (float32 in), the kernel (float32 out) + the same,
          and the linked pair (the kernel writes fc's codes, slfp_linear_fwd_fc reads them).

GB/s = the algorithmic bytes (4 N H W C read + 4 N C or N C written) over the median time, next to the 8.0 TB/s peak of the part.

One process.  Every leg is warmed up, then ROUNDS rounds alternate the legs; a round times a window of back-to-back calls between two
device events.  A window holds as many calls as fill --window-ms (50 ms) of device time, counted per leg from a 20-call probe.  The
calls are asynchronous, but at batch 1 and 8 the kernels are shorter than one enqueue from Python: those rows measure the launch path
of each leg (ctypes for the kernel, the ATen dispatcher for leg A), not the device.  Reported: the median over the rounds of each
leg, and each leg's own minimum and maximum beside it -- a difference inside leg A's spread is no difference."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cnns_slfp_quantization_amd import conv2d_func as cf  # noqa: E402
from cnns_slfp_quantization_amd import fusion  # noqa: E402
from cnns_slfp_quantization_amd import _lib  # noqa: E402

ROUNDS = 5
PEAK_GB_S = 8000.0
KA, KW = 0.25, 0.02
SHAPES = [("resnet50", 7, 7, 2048, False), ("mobilenetv1", 7, 7, 1024, False), ("squeezenet", 13, 13, 1000, True)]


def window_us(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def calls_for(fn, window_ms):
    """calls per timed window: enough for `window_ms` of device time, from a 20-call probe (which also warms the leg up)"""
    return max(20, int(np.ceil(window_ms * 1e3 / window_us(fn, 20))))


def alternate(legs, window_ms):
    """ROUNDS rounds over the legs in turn; each leg's window holds its own number of calls.  Returns (times, calls) per leg."""
    for leg in legs:
        leg()
    torch.cuda.synchronize()
    calls = [calls_for(leg, window_ms) for leg in legs]
    ts = [[] for _ in legs]
    for _ in range(ROUNDS):
        for t, leg, n in zip(ts, legs, calls):
            t.append(window_us(leg, n))
    return ts, calls


def stats(ts, digits=2):
    return {"median": round(float(np.median(ts)), digits), "min": round(float(min(ts)), digits), "max": round(float(max(ts)), digits)}


def within_bound(got, want, x_nchw):
    hw = x_nchw.shape[2] * x_nchw.shape[3]
    bound = 2.0 * (hw + 1) * 2.0 ** -24 * x_nchw.double().abs().mean(dim=(2, 3))
    return bool(((got.double() - want.double()).abs() <= bound).all())


def bench_pool(dev, batches, window_ms):
    L = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev).manual_seed(3)
    rows = []
    for name, H, W, C, has_relu in SHAPES:
        for N, nhwc in [(n, True) for n in batches] + [(64, False)]:
            x = torch.randn((N, C, H, W), generator=g, device=dev) * (4 * KA)   # signed: SqueezeNet's ReLU has work to do
            x = x.contiguous(memory_format=torch.channels_last) if nhwc else x.contiguous()
            layout = _lib.LAYOUT_NHWC if nhwc else _lib.LAYOUT_NCHW
            yb = torch.empty((N, C), device=dev)
            yc = torch.empty((N, C), dtype=torch.uint8, device=dev)
            io_f = _lib.ConvIo(x_codes=0, y_codes=0, y_ka=1.0, y_qbits=8)
            io_c = _lib.ConvIo(x_codes=0, y_codes=1, y_ka=KA, y_qbits=8)
            relu = 1 if has_relu else 0

            def leg_a():
                return F.adaptive_avg_pool2d(x, 1)

            def leg_a_relu():
                return F.adaptive_avg_pool2d(torch.relu(x), 1)

            def leg_b():
                _lib.check(L.slfp_global_avgpool_f32(x.data_ptr(), yb.data_ptr(), N, H, W, C, layout, relu, ctypes.byref(io_f), st))

            def leg_c():
                _lib.check(L.slfp_global_avgpool_f32(x.data_ptr(), yc.data_ptr(), N, H, W, C, layout, relu, ctypes.byref(io_c), st))

            ref = (leg_a_relu() if has_relu else leg_a()).reshape(N, C)
            leg_b(); leg_c()
            torch.cuda.synchronize()
            ok = within_bound(yb, ref, torch.relu(x) if has_relu else x)
            wc = torch.empty((N, C), dtype=torch.uint8, device=dev)
            _lib.check(L.slfp_encode_f32(yb.data_ptr(), wc.data_ptr(), yb.numel(), KA, _lib.FMT_ACT8 | _lib.FMT_EXT, st))
            ok = ok and bool(torch.equal(yc, wc))
            legs = [leg_a, leg_b, leg_c] + ([leg_a_relu] if has_relu else [])
            ts, calls = alternate(legs, window_ms)
            a, b, c = stats(ts[0]), stats(ts[1]), stats(ts[2])
            yard = stats(ts[3]) if has_relu else a   # what the kernel replaces: with relu = 1 that is the ReLU pass + the pool
            rd = 4.0 * N * H * W * C
            row = {"net": name, "H": H, "W": W, "C": C, "batch": N, "layout": "NHWC" if nhwc else "NCHW", "kernel_relu": relu,
                   "window_ms": window_ms, "calls_per_window": calls, "rounds": ROUNDS,
                   "aten_pool_us": a, "kernel_f32_us": b, "kernel_codes_us": c,
                   "f32_over_aten": round(b["median"] / yard["median"], 3), "codes_over_aten": round(c["median"] / yard["median"], 3),
                   "outside_aten_spread": {"f32": not (yard["min"] <= b["median"] <= yard["max"]),
                                           "codes": not (yard["min"] <= c["median"] <= yard["max"])},
                   "gb_s": {"aten": round((rd + 4.0 * N * C) / yard["median"] * 1e-3, 1), "kernel_f32": round((rd + 4.0 * N * C) / b["median"] * 1e-3, 1),
                            "kernel_codes": round((rd + 1.0 * N * C) / c["median"] * 1e-3, 1), "peak": PEAK_GB_S},
                   "results_agree": ok}
            if has_relu:
                row["aten_relu_pool_us"] = yard
                row["f32_over_aten_pool_without_relu"] = round(b["median"] / a["median"], 3)
            rows.append(row)
            print(row, flush=True)
            del x, yb, yc
    return rows


class _Head(nn.Module):
    """nets_imgnet/resnet50.py:146-147, 244-245: avgpool -> flatten -> fc"""

    def __init__(self):
        super().__init__()
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = cf.linear_Q(8, KW, KA)(2048, 1000)

    def forward(self, x):
        return self.fc(torch.flatten(self.avgpool(x), 1))


def bench_head(dev, batches, window_ms):
    torch.manual_seed(5)
    head = _Head().to(dev).eval()
    rows = []
    g = torch.Generator(device=dev).manual_seed(7)
    cf.options.linear_kernel = "fc"
    try:
        with torch.no_grad():
            for N in batches:
                x = (torch.randn((N, 2048, 7, 7), generator=g, device=dev).abs() * (4 * KA)).contiguous(memory_format=torch.channels_last)
                linked = _Head().to(dev).eval()
                linked.load_state_dict(head.state_dict())
                swapped = fusion.use_device_avgpool(linked, x)
                y_dev = linked(x)
                links = fusion.link_pool_head(linked, x)
                same = bool(torch.equal(linked(x), y_dev))
                (ta, tb), calls = alternate([lambda: head(x), lambda: linked(x)], window_ms)
                a, b = stats(ta), stats(tb)
                rows.append({"batch": N, "pools_swapped": swapped, "links": links, "calls_per_window": calls, "rounds": ROUNDS,
                             "aten_pool_fc_f32_us": a, "linked_us": b, "kernels": [linked.avgpool._last_kernel, linked.fc._last_kernel],
                             "linked_over_aten": round(b["median"] / a["median"], 3),
                             "linked_equals_unlinked_device_pool": same})
                print(rows[-1], flush=True)
                del linked, x
    finally:
        cf.options.linear_kernel = "pointwise"
    return rows


def bench_head_abi(dev, batches, window_ms):
    """The same head as calls of the C ABI (no module, no pass): what the device does once the launch path is out of the way."""
    L = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev).manual_seed(11)
    K, N, H, W = 2048, 1000, 7, 7
    w = torch.randn((N, K), generator=g, device=dev) * (KW * 3)
    b = torch.randn((N,), generator=g, device=dev) * 0.5
    blob = torch.empty(L.slfp_linear_workspace_bytes(1, K, N), dtype=torch.uint8, device=dev)
    _lib.check(L.slfp_linear_prepare_weights(w.data_ptr(), blob.data_ptr(), K, N, KW, 8, 0, st))
    rows = []
    for M in batches:
        x = (torch.randn((M, K, H, W), generator=g, device=dev).abs() * (4 * KA)).contiguous(memory_format=torch.channels_last)
        io_ff = _lib.ConvIo(x_codes=0, y_codes=0, y_ka=1.0, y_qbits=8)
        io_pool = _lib.ConvIo(x_codes=0, y_codes=1, y_ka=KA, y_qbits=8)
        io_fc = _lib.ConvIo(x_codes=1, y_codes=0, y_ka=1.0, y_qbits=8)
        ws = torch.empty(max(L.slfp_linear_fc_workspace_bytes(M, K, N, ctypes.byref(io_ff)), 16), dtype=torch.uint8, device=dev)
        pf, pc = torch.empty((M, K), device=dev), torch.empty((M, K), dtype=torch.uint8, device=dev)
        ya, yb, yc = torch.empty((M, N), device=dev), torch.empty((M, N), device=dev), torch.empty((M, N), device=dev)

        def fc_f32(p, y):
            _lib.check(L.slfp_linear_fwd_fc(p.data_ptr(), blob.data_ptr(), b.data_ptr(), y.data_ptr(), M, K, N, KA, KW, 8, 0,
                                            ctypes.byref(io_ff), 0, ws.data_ptr(), st))

        def leg_a():   # the ATen pool, then the float32 fc (its encode pass included)
            fc_f32(F.adaptive_avg_pool2d(x, 1), ya)

        def leg_b():   # the kernel with float32 out, then the float32 fc: the un-linked device pool
            _lib.check(L.slfp_global_avgpool_f32(x.data_ptr(), pf.data_ptr(), M, H, W, K, _lib.LAYOUT_NHWC, 0, ctypes.byref(io_ff), st))
            fc_f32(pf, yb)

        def leg_c():   # the linked pair: the kernel writes fc's codes, fc reads them
            _lib.check(L.slfp_global_avgpool_f32(x.data_ptr(), pc.data_ptr(), M, H, W, K, _lib.LAYOUT_NHWC, 0, ctypes.byref(io_pool), st))
            _lib.check(L.slfp_linear_fwd_fc(pc.data_ptr(), blob.data_ptr(), b.data_ptr(), yc.data_ptr(), M, K, N, KA, KW, 8, 0,
                                            ctypes.byref(io_fc), 0, None, st))

        leg_a(); leg_b(); leg_c()
        torch.cuda.synchronize()
        same = bool(torch.equal(yb, yc))
        (ta, tb, tc), calls = alternate([leg_a, leg_b, leg_c], window_ms)
        a, bb, c = stats(ta), stats(tb), stats(tc)
        rows.append({"batch": M, "calls_per_window": calls, "rounds": ROUNDS, "aten_pool_fc_f32_us": a, "kernel_pool_fc_f32_us": bb,
                     "linked_us": c, "linked_over_aten": round(c["median"] / a["median"], 3),
                     "unlinked_kernel_over_aten": round(bb["median"] / a["median"], 3), "linked_equals_unlinked_device_pool": same})
        print(rows[-1], flush=True)
        del x
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "avgpool_bench.json"))
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64, 256])
    ap.add_argument("--window-ms", type=float, default=50.0, help="device time per timed window; the calls per window follow from it")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "method": __doc__.split("\n\n")[-1].replace("\n", " "),
           "pool": bench_pool(dev, a.batches, a.window_ms), "head": bench_head(dev, a.batches, a.window_ms),
           "head_c_abi": bench_head_abi(dev, a.batches, a.window_ms)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
