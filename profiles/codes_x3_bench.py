#!/usr/bin/env python3
"""The pointwise (1x1) kernels on 1-byte codes in the float32-equivalent (three-pass) mode (csrc/conv_pw_codes.hip with PASSES = 3,
slfp_conv2d_fwd_codes_x3) against the float32-interface three-pass launch they replace inside a linked net, on the MI355X.  Writes
profiles/codes_x3_bench.json (--out: elsewhere).

  layers     the 13 pointwise layers of MobileNetV1-224 at batch 128, straight through the C ABI with the epilogue of the fused net
             (post scale / shift + ReLU), one prepared three-pass blob per layer.  Leg A = slfp_conv2d_fwd_post on float32 (what this
             change does not touch), leg B = slfp_conv2d_fwd_codes_x3 codes -> float32, leg C = codes -> codes.  B is compared with A
             bit for bit, C with slfp_encode_f32 of A byte for byte, before anything is timed.
  whole_net  the fixture-shaped MobileNetV1 of bench.py (27 convs, folded BatchNorm / ReLU, pool, classifier) under
             options.mfma_passes = 3 after fuse_bn_relu: leg A = unlinked, leg B = the same weights after link_codes(x3=True).

One process.  Every leg is warmed up, then ROUNDS rounds alternate the legs; a round times a window of back-to-back calls between two
device events (steady state: no flush between calls; the tensors of these layers are 6-820 MB).  Reported: the median over the
rounds of each leg, and each leg's own minimum and maximum beside it -- a difference inside leg A's spread is no difference."""
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
from cnns_slfp_quantization_amd import fusion, layer_specs  # noqa: E402
from cnns_slfp_quantization_amd import _lib  # noqa: E402

ROUNDS = 7


def window_us(fn, calls):
    """microseconds per call of `calls` back-to-back calls of fn, between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def alternate(legs, calls, warmup=5):
    ts = [[] for _ in legs]
    for _ in range(warmup):
        for leg in legs:
            leg()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for t, leg in zip(ts, legs):
            t.append(window_us(leg, calls))
    return ts


def stats(ts, digits=1):
    return {"median": round(float(np.median(ts)), digits), "min": round(float(min(ts)), digits), "max": round(float(max(ts)), digits)}


def bench_layers(specs, dev, batch, calls):
    L = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev).manual_seed(3)
    rows = []
    pw = [(i, s) for i, s in enumerate(specs) if tuple(s.k) == (1, 1) and s.groups == 1]
    assert len(pw) == 13
    for i, s in pw:
        ka_next = float(np.float32(specs[i + 1].Ka)) if i + 1 < len(specs) else 0.25
        d = _lib.ConvDesc(n=batch, c_in=s.c_in, h=s.h, w=s.w, c_out=s.c_out, kh=1, kw=1, stride_h=1, stride_w=1, pad_h=0, pad_w=0, dil_h=1,
                          dil_w=1, groups=1, x_layout=_lib.LAYOUT_NHWC, y_layout=_lib.LAYOUT_NHWC, qbits=8, ka=float(np.float32(s.Ka)),
                          kw_scale=float(np.float32(s.Kw)), mfma_passes=_lib.MFMA_F16X3, reserved=0)
        dp = ctypes.byref(d)
        io_f, io_c = _lib.ConvIo(x_codes=1, y_codes=0, y_ka=1.0, y_qbits=8), _lib.ConvIo(x_codes=1, y_codes=1, y_ka=ka_next, y_qbits=8)
        assert L.slfp_conv2d_codes_x3_supported(dp, ctypes.byref(io_f), 0, 1) == 1 and L.slfp_conv2d_codes_x3_supported(dp, ctypes.byref(io_c), 0, 1) == 1
        names = (L.slfp_debug_pw_variant(dp, None, 0, 0, 0).decode(), L.slfp_debug_pwc_x3_variant(dp, ctypes.byref(io_f)).decode(),
                 L.slfp_debug_pwc_x3_variant(dp, ctypes.byref(io_c)).decode())
        x = torch.randn((batch, s.h, s.w, s.c_in), generator=g, device=dev).abs_() * (2.0 * s.Ka)
        xc = torch.empty(x.shape, dtype=torch.uint8, device=dev)
        fmt = _lib.FMT_ACT8 | _lib.FMT_EXT
        _lib.check(L.slfp_encode_f32(x.data_ptr(), xc.data_ptr(), x.numel(), d.ka, fmt, st))
        w = torch.randn((s.c_out, s.c_in, 1, 1), generator=g, device=dev) * float(np.sqrt(2.0 / s.c_in))
        scale = torch.rand(s.c_out, generator=g, device=dev) + 0.5
        shift = torch.randn(s.c_out, generator=g, device=dev) * 0.1
        blob = torch.empty(L.slfp_conv2d_wprep_bytes(dp), dtype=torch.uint8, device=dev)
        _lib.check(L.slfp_conv2d_prepare_weights(dp, w.data_ptr(), blob.data_ptr(), None, st))
        out = (batch, s.h, s.w, s.c_out)
        ya, yb = torch.empty(out, device=dev), torch.empty(out, device=dev)
        yc, want = torch.empty(out, dtype=torch.uint8, device=dev), torch.empty(out, dtype=torch.uint8, device=dev)
        args = (blob.data_ptr(), None, scale.data_ptr(), shift.data_ptr(), 1)

        def leg_a():
            _lib.check(L.slfp_conv2d_fwd_post(dp, x.data_ptr(), *args, ya.data_ptr(), None, None, st))

        def leg_b():
            _lib.check(L.slfp_conv2d_fwd_codes_x3(dp, ctypes.byref(io_f), xc.data_ptr(), *args, yb.data_ptr(), st))

        def leg_c():
            _lib.check(L.slfp_conv2d_fwd_codes_x3(dp, ctypes.byref(io_c), xc.data_ptr(), *args, yc.data_ptr(), st))

        leg_a(), leg_b(), leg_c()
        _lib.check(L.slfp_encode_f32(ya.data_ptr(), want.data_ptr(), ya.numel(), ka_next, fmt, st))
        same = bool(torch.equal(ya.view(torch.int32), yb.view(torch.int32))) and bool(torch.equal(yc, want))
        ta, tb, tc = alternate((leg_a, leg_b, leg_c), calls)
        a, b, c = stats(ta), stats(tb), stats(tc)
        rows.append({"layer": f"{s.c_in}@{s.h} -> {s.c_out}", "batch": batch, "calls_per_window": calls, "rounds": ROUNDS,
                     "f32_x3_us": a, "codes_to_f32_x3_us": b, "codes_to_codes_x3_us": c,
                     "codes_to_f32_over_f32": round(b["median"] / a["median"], 3), "codes_to_codes_over_f32": round(c["median"] / a["median"], 3),
                     "bit_identical": same, "kernels": list(names)})
        print(rows[-1], flush=True)
        del x, xc, ya, yb, yc, want
    return rows


def conv(s):
    return cf.conv2d_Q(q_bit=8, Kw=np.float64(s.Kw), Ka=np.float64(s.Ka))(
        s.c_in, s.c_out, s.k[0], np.float64(s.Kw), np.float64(s.Ka), s.stride[0], s.pad[0], groups=s.groups, bias=False)


def build_net(specs, dev):
    torch.manual_seed(3)
    layers = []
    for s in specs:
        layers += [conv(s), nn.BatchNorm2d(s.c_out), nn.ReLU(inplace=True)]
    model = nn.Sequential(*layers, nn.AvgPool2d(7), nn.Flatten(), nn.Linear(1024, 1000))
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_var.uniform_(0.5, 1.5, generator=g)
                m.weight.uniform_(0.8, 1.6, generator=g)
                m.bias.normal_(0.1, 0.1, generator=g)
    model = model.to(dev).eval().to(memory_format=torch.channels_last)
    fusion.fuse_bn_relu(model)
    return model


def bench_net(specs, dev, batch, steps):
    prev = cf.options.mfma_passes
    cf.options.mfma_passes = 3
    try:
        with torch.no_grad():
            plain, linked = build_net(specs, dev), build_net(specs, dev)
            g = torch.Generator(device=dev).manual_seed(4)
            x = torch.randn((batch, 3, 224, 224), device=dev, generator=g).contiguous(memory_format=torch.channels_last)
            links = fusion.link_codes(linked, example_input=x, x3=True)
            y_a, y_b = plain(x).clone(), linked(x).clone()
            pw = [m for m in linked.modules() if isinstance(m, nn.Conv2d) and tuple(m.kernel_size) == (1, 1)]
            n_x3 = sum(1 for m in pw if m._last_kernel and m._last_kernel.endswith("+x3"))
            same = bool(torch.equal(y_a, y_b))
            ta, tb = alternate((lambda: plain(x), lambda: linked(x)), steps, warmup=3)
        ia, ib = [batch / t * 1e6 for t in ta], [batch / t * 1e6 for t in tb]
        row = {"batch": batch, "steps_per_window": steps, "rounds": ROUNDS, "code_links": links, "pointwise_layers_on_x3": n_x3,
               "unlinked_x3_img_s": stats(ia, 0), "linked_x3_img_s": stats(ib, 0),
               "linked_over_unlinked": round(float(np.median(ib) / np.median(ia)), 3), "bit_identical": same}
        print(row, flush=True)
        return [row]
    finally:
        cf.options.mfma_passes = prev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codes_x3_bench.json"))
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    dev = torch.device("cuda", 0)
    specs = layer_specs.conv_layers("mobilenetv1_imagenet224")
    res = {"device": torch.cuda.get_device_name(0), "method": __doc__.split("\n\n")[-1].replace("\n", " "),
           "layers": bench_layers(specs, dev, a.batch, a.calls), "whole_net": bench_net(specs, dev, a.batch, a.steps)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
