#!/usr/bin/env python3
"""Linear_Q on the weight-streaming kernel (csrc/linear_fc.hip, slfp_linear_fwd_fc) against the pointwise path it can replace
(slfp_linear_fwd_prepared: the layer as a 1x1 convolution over the batch), on the MI355X.  Writes profiles/linear_fc_bench.json
(--out: elsewhere).

  layers     the classifier layers of AlexNet (9216 -> 4096 -> 4096 -> 1000), VGG16_Q (25088 -> 4096 -> 4096 -> 1000) and ResNet-50
             (2048 -> 1000) at batch 1, 8, 64 and 256, q_bit 8, single-pass mode.  Leg A = slfp_linear_fwd_prepared (float32 in and
             out), leg B = slfp_linear_fwd_fc with float32 in and out (the encode pass into the workspace included), leg C = the same
             with codes in and codes out (float32 out where N is not whole 16-channel tiles: the 1000-class layers).  The outputs
             are compared bit for bit before anything is timed.
  tiles      per (layer, batch): leg C under every forced (n-tiles, row-tiles) per workgroup (slfp_debug_linear_fc_tiles) next to the
             rule's own choice: the measurements behind fc_select.
  cold       legs A and C again with 512 MiB written to another buffer before every call (each call between its own two events): W
             then comes from HBM, not from the 256 MiB Infinity Cache that back-to-back replays of a 75-205 MB layer partly hit.
  head       a three-layer AlexNet head (Dropout, Linear_Q, ReLU, Dropout, Linear_Q, ReLU, Linear_Q on a [batch, 9216] float32 input):
             unlinked on the pointwise path, unlinked under options.linear_kernel = "fc", and linked by fusion.link_head.

One process.  Every leg is warmed up, then ROUNDS rounds alternate the legs; a round times a window of back-to-back calls between two
device events.  A window holds as many calls as fill --window-ms (50 ms) of device time, counted per leg from a 20-call probe
("calls_per_window": 83 ... 5 109 in the committed run), so that the clock and the scheduler are small beside it.  The calls are asynchronous: the host
only has to enqueue faster than the device runs, which it does down to the 10 us layers (a leg that became host-bound would show the
same time at every batch and tiling).  Reported: the median over the rounds of each leg, and each leg's own minimum and maximum
beside it -- a difference inside leg A's spread is no difference."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import utils.conv2d_func as cf  # noqa: E402
from cnns_slfp_quantization_amd import fusion  # noqa: E402
from cnns_slfp_quantization_amd import _lib  # noqa: E402

ROUNDS = 5
KA, KW = 0.25, 0.02
LAYERS = [("alexnet.fc1", 9216, 4096), ("alexnet.fc2 / vgg16.fc2", 4096, 4096), ("alexnet.fc3 / vgg16.fc3", 4096, 1000),
          ("vgg16.fc1", 25088, 4096), ("resnet50.fc", 2048, 1000)]


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


def cold_us(fn, flush, calls):
    """mean microseconds of `calls` calls, each behind a 512 MiB write to another buffer and between its own two events"""
    tot = 0.0
    for _ in range(calls):
        flush.fill_(1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        tot += e0.elapsed_time(e1) * 1e3
    return tot / calls


def stats(ts, digits=1):
    return {"median": round(float(np.median(ts)), digits), "min": round(float(min(ts)), digits), "max": round(float(max(ts)), digits)}


def bench_layers(dev, batches, window_ms):
    L = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev).manual_seed(3)
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    rows = []
    for name, K, N in LAYERS:
        w = torch.randn((N, K), generator=g, device=dev) * (KW * 3)
        b = torch.randn((N,), generator=g, device=dev) * 0.5
        blob = torch.empty(L.slfp_linear_workspace_bytes(1, K, N), dtype=torch.uint8, device=dev)
        _lib.check(L.slfp_linear_prepare_weights(w.data_ptr(), blob.data_ptr(), K, N, KW, 8, 0, st))
        del w
        codes_out = N % 16 == 0
        for M in batches:
            x = torch.randn((M, K), generator=g, device=dev).abs() * (4 * KA)
            xc = torch.empty((M, K), dtype=torch.uint8, device=dev)
            _lib.check(L.slfp_encode_f32(x.data_ptr(), xc.data_ptr(), x.numel(), KA, _lib.FMT_ACT8 | _lib.FMT_EXT, st))
            ya, yb = torch.empty((M, N), device=dev), torch.empty((M, N), device=dev)
            yc = torch.empty((M, N), dtype=torch.uint8 if codes_out else torch.float32, device=dev)
            io_f = _lib.ConvIo(x_codes=0, y_codes=0, y_ka=1.0, y_qbits=8)
            io_c = _lib.ConvIo(x_codes=1, y_codes=1 if codes_out else 0, y_ka=0.37, y_qbits=8)
            ws = torch.empty(max(L.slfp_linear_fc_workspace_bytes(M, K, N, ctypes.byref(io_f)), 16), dtype=torch.uint8, device=dev)

            def leg_a():
                _lib.check(L.slfp_linear_fwd_prepared(x.data_ptr(), blob.data_ptr(), b.data_ptr(), ya.data_ptr(), M, K, N, KA, KW, 8, 0, st))

            def leg_b():
                _lib.check(L.slfp_linear_fwd_fc(x.data_ptr(), blob.data_ptr(), b.data_ptr(), yb.data_ptr(), M, K, N, KA, KW, 8, 0,
                                                ctypes.byref(io_f), 0, ws.data_ptr(), st))

            def leg_c():
                _lib.check(L.slfp_linear_fwd_fc(xc.data_ptr(), blob.data_ptr(), b.data_ptr(), yc.data_ptr(), M, K, N, KA, KW, 8, 0,
                                                ctypes.byref(io_c), 1, None, st))

            leg_a(); leg_b(); leg_c()
            torch.cuda.synchronize()
            same = bool(torch.equal(ya, yb))
            want = torch.relu(ya)
            if codes_out:
                wc = torch.empty((M, N), dtype=torch.uint8, device=dev)
                _lib.check(L.slfp_encode_f32(want.data_ptr(), wc.data_ptr(), want.numel(), 0.37, _lib.FMT_ACT8 | _lib.FMT_EXT, st))
                want = wc
            same = same and bool(torch.equal(yc, want))
            (ta, tb, tc), calls = alternate([leg_a, leg_b, leg_c], window_ms)
            tiles = {}
            for ntw in (1, 2, 4):
                for mt in (1, 2, 4):
                    if mt > 1 and M <= 16 * (mt // 2):
                        continue   # more row tiles than the batch has rows for: the narrower one does the same work
                    assert L.slfp_debug_linear_fc_tiles(ntw, mt) == 0
                    leg_c()
                    torch.cuda.synchronize()
                    assert torch.equal(yc, want), (ntw, mt)
                    n = calls_for(leg_c, window_ms)
                    tiles[f"{ntw}x{mt}"] = round(float(np.median([window_us(leg_c, n) for _ in range(3)])), 1)
            assert L.slfp_debug_linear_fc_tiles(0, 0) == 0
            cold = {"pointwise_us": round(cold_us(leg_a, flush, 6), 1), "fc_codes_us": round(cold_us(leg_c, flush, 6), 1)}
            a, bb, c = stats(ta), stats(tb), stats(tc)
            rows.append({"layer": name, "K": K, "N": N, "batch": M, "window_ms": window_ms, "calls_per_window": calls, "rounds": ROUNDS,
                         "pointwise_f32_us": a, "fc_f32_us": bb, "fc_codes_us": c, "fc_codes_writes": "codes" if codes_out else "float32",
                         "fc_f32_over_pointwise": round(bb["median"] / a["median"], 3), "fc_codes_over_pointwise": round(c["median"] / a["median"], 3),
                         "w_gb_s_fc_codes": round(2.0 * K * N / c["median"] * 1e-3, 1), "bit_identical": same,
                         "forced_tiles_us (n-tiles x row-tiles)": tiles, "cold": cold})
            print(rows[-1], flush=True)
            del x, xc, ya, yb, yc
        del blob
    return rows


def bench_head(dev, batches, window_ms):
    Lin = cf.linear_Q(8, KW, KA)

    def make():
        return nn.Sequential(nn.Dropout(), Lin(9216, 4096), nn.ReLU(), nn.Dropout(), Lin(4096, 4096), nn.ReLU(), Lin(4096, 1000)).to(dev).eval()

    torch.manual_seed(5)
    head = make()
    rows = []
    g = torch.Generator(device=dev).manual_seed(7)
    with torch.no_grad():
        for M in batches:
            x = torch.randn((M, 9216), generator=g, device=dev).abs() * (4 * KA)
            linked = make()
            linked.load_state_dict(head.state_dict())
            y0 = head(x)
            links = fusion.link_head(linked, x)

            def leg_fc():
                cf.options.linear_kernel = "fc"
                y = head(x)
                cf.options.linear_kernel = "pointwise"
                return y

            same = bool(torch.equal(leg_fc(), y0) and torch.equal(linked(x), y0))
            (ta, tb, tc), calls = alternate([lambda: head(x), leg_fc, lambda: linked(x)], window_ms)
            a, b, c = stats(ta), stats(tb), stats(tc)
            rows.append({"batch": M, "links": links, "calls_per_window": calls, "rounds": ROUNDS, "unlinked_pointwise_us": a,
                         "unlinked_fc_us": b, "linked_us": c, "fc_over_pointwise": round(b["median"] / a["median"], 3),
                         "linked_over_pointwise": round(c["median"] / a["median"], 3), "bit_identical": same})
            print(rows[-1], flush=True)
            del linked, x
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_fc_bench.json"))
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64, 256])
    ap.add_argument("--window-ms", type=float, default=50.0, help="device time per timed window; the calls per window follow from it")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "method": __doc__.split("\n\n")[-1].replace("\n", " "),
           "layers": bench_layers(dev, a.batches, a.window_ms), "head": bench_head(dev, a.batches, a.window_ms)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
