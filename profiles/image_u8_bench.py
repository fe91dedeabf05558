"""Image stems on uint8 pixels (slfp_conv2d_fwd_u8) against what a caller with bytes does today.  DESIGN.md section 31.

    python profiles/image_u8_bench.py [--reps 30] [--out profiles/image_u8_bench.json] [--no-net]

Per first layer of the seven reference nets (layer_specs) at its benchmark batch (256 for the two MobileNetV1, 128 otherwise),
through the C ABI, with bias as the net has it, a BatchNorm-like affine and the ReLU in the epilogue, float32 out and code out:
  A  the float32 stem on a pre-normalised float32 tensor (the input already in device memory: no caller with bytes has it for free)
  B  normalisation on the device from bytes with ATen (x.float().div_(255).sub_(mean).div_(std), channels_last) + the float32 stem:
     what a caller with bytes does today
  C  the byte-input stem (slfp_conv2d_fwd_u8) on the bytes and the pixel table
  E  slfp_image_u8_expand_f32 + the float32 stem: the library's own path for a stem without a byte form
Timed with HIP events after warm-up, the legs alternated twice in one process; a leg's time is the better of its two rounds and
`b_spread` is leg B's round-to-round difference relative to its best.  The rule of DESIGN section 12: a stem family whose C is not
below B by more than B's spread in every one of its rows is taken out of the default of fusion.link_image_u8
(conv2d_func.IMAGE_U8_OFF); so is a family whose C is slower than E, the library's own other way to read bytes, by more than E's spread
in any row.  C against A is reported next to it and decides nothing.
Whole nets, BatchNorm folded and code-linked, images/s with B in front, with C (IMAGE_U8_OFF emptied) and with the default
(IMAGE_U8_OFF as committed): MobileNetV1-224 as bench.py builds it at batch 256, and ResNet-50 (the fixture net of
tests/golden/netgen_r3.py, as profiles/residual_bench.py builds it) at batch 128 after fuse_named_bn, link_codes_traced(entries=True)
and link_stem.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests", "golden"))
from cnns_slfp_quantization_amd import _lib, fusion, image_u8, layer_specs  # noqa: E402
from cnns_slfp_quantization_amd import conv2d_func as cf  # noqa: E402

NETS = (("mobilenetv1_imagenet224", 256), ("mobilenetv1_cifar32", 256), ("vgg16_224", 128), ("shufflenetv2_224", 128),
        ("resnet50_imagenet224", 128), ("squeezenet1_0_imagenet224", 128), ("alexnet_imagenet224", 128))
KA_NEXT = 0.25


def _time(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def _alternate(legs, reps, warmup):
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    rounds = {name: [] for name in legs}
    for _ in range(2):
        for name, fn in legs.items():
            rounds[name].append(_time(fn, reps))
    return {n: min(v) for n, v in rounds.items()}, {n: (max(v) - min(v)) / min(v) for n, v in rounds.items()}


def _constants(net):
    return (image_u8.CIFAR_MEAN, image_u8.CIFAR_STD) if "cifar" in net else (image_u8.IMAGENET_MEAN, image_u8.IMAGENET_STD)


def bench_stem(net, batch, reps, warmup):
    L = _lib.load()
    s = layer_specs.conv_layers(net)[0]
    dev = torch.device("cuda:0")
    d = _lib.ConvDesc(n=batch, c_in=s.c_in, h=s.h, w=s.w, c_out=s.c_out, kh=s.k[0], kw=s.k[1], stride_h=s.stride[0], stride_w=s.stride[1],
                      pad_h=s.pad[0], pad_w=s.pad[1], dil_h=1, dil_w=1, groups=1, x_layout=_lib.LAYOUT_NHWC, y_layout=_lib.LAYOUT_NHWC, qbits=8,
                      ka=float(np.float32(s.Ka)), kw_scale=float(np.float32(s.Kw)), mfma_passes=0, reserved=0)
    dp = ctypes.byref(d)
    gen = torch.Generator().manual_seed(1)
    mean, std = _constants(net)
    table = image_u8.pixel_table(mean, std).to(dev)
    mean_t, std_t = torch.tensor(mean, device=dev).view(1, 3, 1, 1), torch.tensor(std, device=dev).view(1, 3, 1, 1)
    x8 = torch.randint(0, 256, (batch, 3, s.h, s.w), dtype=torch.uint8, generator=gen).to(dev).contiguous(memory_format=torch.channels_last)
    x32 = image_u8.expand(x8, table)
    w = (torch.randn((s.c_out, s.c_in) + tuple(s.k), generator=gen) * (3.0 * s.Kw)).to(dev)
    bias = (torch.randn(s.c_out, generator=gen) * 0.1).to(dev) if s.bias else None
    ps, psh = (0.5 + torch.rand(s.c_out, generator=gen)).to(dev), (torch.randn(s.c_out, generator=gen) * 0.1).to(dev)
    blob = torch.empty(L.slfp_conv2d_wprep_bytes(dp), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(L.slfp_conv2d_prepare_weights(dp, w.data_ptr(), blob.data_ptr(), None, st))
    nws = L.slfp_conv2d_workspace_bytes(dp)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev) if nws else None
    wsp, bp = (ws.data_ptr() if ws is not None else None), (bias.data_ptr() if bias is not None else None)
    tmp = torch.empty_like(x32)
    rows = []
    for out in ("f32", "codes"):
        io = _lib.ConvIo(x_codes=0, y_codes=1 if out == "codes" else 0, y_ka=KA_NEXT, y_qbits=8)
        iop = ctypes.byref(io)
        y = torch.empty((batch, s.h_out, s.w_out, s.c_out), dtype=torch.uint8 if out == "codes" else torch.float32, device=dev)
        has_b = 1 if s.bias else 0
        if out == "codes" and not L.slfp_conv2d_codes_supported(dp, iop, has_b, 1):
            continue
        assert L.slfp_conv2d_u8_supported(dp, iop, has_b, 1) == 1, (net, out)
        inst = L.slfp_debug_stem_u8_instance(dp, iop, has_b, 1, 1).decode()
        f32_inst = L.slfp_debug_stem_instance(dp, iop if out == "codes" else None, has_b, 1, 1).decode()

        def stem(xp):
            if out == "codes":
                _lib.check(L.slfp_conv2d_fwd_codes_ws(dp, iop, xp, blob.data_ptr(), bp, ps.data_ptr(), psh.data_ptr(), 1, y.data_ptr(), wsp, st))
            else:
                _lib.check(L.slfp_conv2d_fwd_post(dp, xp, blob.data_ptr(), bp, ps.data_ptr(), psh.data_ptr(), 1, y.data_ptr(), None, wsp, st))

        def leg_a():
            stem(x32.data_ptr())

        def leg_b():
            xn = x8.float().div_(255).sub_(mean_t).div_(std_t)
            stem(xn.data_ptr())

        def leg_c():
            _lib.check(L.slfp_conv2d_fwd_u8(dp, iop, x8.data_ptr(), table.data_ptr(), blob.data_ptr(), bp, ps.data_ptr(), psh.data_ptr(), 1,
                                            y.data_ptr(), wsp, st))

        def leg_e():
            _lib.check(L.slfp_image_u8_expand_f32(x8.data_ptr(), table.data_ptr(), tmp.data_ptr(), batch * s.h * s.w, 3, st))
            stem(tmp.data_ptr())

        leg_a(); ya = y.clone(); leg_c()
        same = bool(torch.equal(ya, y))
        best, spread = _alternate({"A": leg_a, "B": leg_b, "C": leg_c, "E": leg_e}, reps, warmup)
        row = {"net": net, "batch": batch, "out": out, "instance": inst, "f32_instance": f32_inst, "family": inst.split("/")[0],
               "c_equals_a_bits": same, "a_ms": round(best["A"], 4), "b_ms": round(best["B"], 4), "c_ms": round(best["C"], 4),
               "e_ms": round(best["E"], 4), "b_spread": round(spread["B"], 3), "a_spread": round(spread["A"], 3),
               "c_spread": round(spread["C"], 3), "e_spread": round(spread["E"], 3), "c_over_b": round(best["C"] / best["B"], 3),
               "c_over_a": round(best["C"] / best["A"], 3), "c_over_e": round(best["C"] / best["E"], 3),
               "c_below_b_beyond_spread": bool(best["C"] < best["B"] * (1 - spread["B"])),
               "c_not_above_e_beyond_spread": bool(best["C"] <= best["E"] * (1 + spread["E"]))}
        print("stem", json.dumps(row), flush=True)
        rows.append(row)
    return rows


def build_mobilenet(dev):
    """MobileNetV1-224 as bench.py's whole_net builds it, BatchNorm + ReLU folded, code-linked."""
    import torch.nn as nn
    import utils.conv2d_func as ucf
    net = "mobilenetv1_imagenet224"
    layers = []
    for s in layer_specs.conv_layers(net):
        conv = ucf.conv2d_Q(q_bit=8, Kw=np.float64(s.Kw), Ka=np.float64(s.Ka))(
            s.c_in, s.c_out, s.k[0], np.float64(s.Kw), np.float64(s.Ka), s.stride[0], s.pad[0], groups=s.groups, bias=False)
        layers += [conv, nn.BatchNorm2d(s.c_out), nn.ReLU(inplace=True)]
    model = nn.Sequential(*layers, nn.AvgPool2d(7), nn.Flatten(), nn.Linear(1024, 1000)).to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(3)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_var.uniform_(0.5, 1.5, generator=g)
                m.weight.uniform_(0.8, 1.6, generator=g)
                m.bias.normal_(0.1, 0.1, generator=g)
    model = model.to(memory_format=torch.channels_last)

    def link(x32):
        fusion.fuse_bn_relu(model)
        return {"code_links": fusion.link_codes(model, example_input=x32)}

    return net, model, model[0], link


def build_resnet50(dev):
    """The ResNet-50 fixture net (tests/golden/netgen_r3.py + nets_r3_golden.npz), as profiles/residual_bench.py builds it."""
    import netgen_r3 as ng
    import utils.conv2d_func as ucf
    import utils.sfp_quant as sq
    gold = np.load(os.path.join(os.path.dirname(HERE), "tests", "golden", "nets_r3_golden.npz"))
    q, _, _, seed = [int(v) for v in gold["resnet50:meta"]]
    manifest = json.loads(bytes(gold["resnet50:manifest"]).decode())
    gains = json.loads(bytes(gold["resnet50:gains"]).decode())
    m = ng.BUILDERS["resnet50"](ng.Factories(ucf, q, manifest, layerout=sq.layerout_quantize_func))
    ng.fill_parameters_by_name(m, seed, gains)
    ng.load_bn_stats_by_name_(m, {k[len("resnet50") + 1:]: gold[k] for k in gold.files if k.startswith("resnet50:bn:")})
    m = m.to(dev).eval().to(memory_format=torch.channels_last)

    def link(x32):
        out = {"bn_pairs": fusion.fuse_bn_relu(m) + fusion.fuse_named_bn(m, example_input=x32)}
        out["code_links"] = fusion.link_codes_traced(m, x32, entries=True)
        out["stem_links"] = fusion.link_stem(m, x32)
        return out

    return "resnet50 (fixture)", m, dict(m.named_modules())["conv1"], link


def bench_net(build, batch, steps):
    """images/s of a whole code-linked net with bytes in front: B (ATen normalisation + the float32 stem), C (the byte stem,
    IMAGE_U8_OFF emptied) and D (the default: IMAGE_U8_OFF as committed), alternated twice, best of two."""
    dev = torch.device("cuda:0")
    net, model, stem, link = build(dev)
    mean, std = _constants(net)
    table = image_u8.pixel_table(mean, std)
    mean_t, std_t = torch.tensor(mean, device=dev).view(1, 3, 1, 1), torch.tensor(std, device=dev).view(1, 3, 1, 1)
    x8 = torch.randint(0, 256, (batch, 3, 224, 224), dtype=torch.uint8).to(dev).contiguous(memory_format=torch.channels_last)
    out = {"net": net, "batch": batch, "steps": steps}
    default_off = set(cf.IMAGE_U8_OFF)
    out["image_u8_off"] = sorted(default_off)
    try:
        with torch.no_grad():
            x32 = image_u8.expand(x8, table.to(dev))
            out.update(link(x32))
            y_b = model(x8.float().div_(255).sub_(mean_t).div_(std_t))
            y_32 = model(x32)
            out["image_u8_links"] = fusion.link_image_u8(model, table, x8)
            cf.IMAGE_U8_OFF.clear()
            y_c = model(x8)
            out["c_stem_kernel"] = stem._last_kernel
            out["c_equals_expand_bits"] = bool(torch.equal(y_c, y_32))
            cf.IMAGE_U8_OFF.update(default_off)
            y_d = model(x8)
            out["default_stem_kernel"] = stem._last_kernel
            out["default_equals_expand_bits"] = bool(torch.equal(y_d, y_32))
            out["b_max_abs_diff_to_c"] = float((y_b - y_c).abs().max())   # ATen's device division is not the table's function

            def run_b():
                model(x8.float().div_(255).sub_(mean_t).div_(std_t))

            def run_c():
                cf.IMAGE_U8_OFF.clear()
                model(x8)

            def run_d():
                cf.IMAGE_U8_OFF.clear()
                cf.IMAGE_U8_OFF.update(default_off)
                model(x8)

            legs = (("B", run_b), ("C", run_c), ("D", run_d))
            rates = {name: [] for name, _ in legs}
            for _, fn in legs:
                for _ in range(3):
                    fn()
            for _ in range(2):
                for name, fn in legs:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        fn()
                    torch.cuda.synchronize()
                    rates[name].append(batch * steps / (time.perf_counter() - t0))
            for name, key in (("B", "b"), ("C", "c"), ("D", "default")):
                out[key + "_images_per_s"] = round(max(rates[name]), 1)
                out[key + "_spread"] = round((max(rates[name]) - min(rates[name])) / max(rates[name]), 3)
            out["c_over_b_rate"] = round(max(rates["C"]) / max(rates["B"]), 3)
            out["default_over_b_rate"] = round(max(rates["D"]) / max(rates["B"]), 3)
            out["default_over_c_rate"] = round(max(rates["D"]) / max(rates["C"]), 3)
    finally:
        cf.IMAGE_U8_OFF.clear()
        cf.IMAGE_U8_OFF.update(default_off)
    print("net", json.dumps(out), flush=True)
    del model
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-net", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "image_u8_bench.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "legs": {"A": "float32 stem on a pre-normalised tensor",
           "B": "ATen normalisation from bytes + float32 stem", "C": "slfp_conv2d_fwd_u8", "E": "slfp_image_u8_expand_f32 + float32 stem"},
           "stems": [], "families": {}, "nets": []}
    for net, batch in NETS:
        res["stems"] += bench_stem(net, batch, a.reps, a.warmup)
        torch.cuda.empty_cache()
    for fam in sorted({r["family"] for r in res["stems"]}):
        rows = [r for r in res["stems"] if r["family"] == fam]
        res["families"][fam] = {"rows": len(rows), "c_below_b_in_every_row": all(r["c_below_b_beyond_spread"] for r in rows),
                                "c_not_above_e_in_every_row": all(r["c_not_above_e_beyond_spread"] for r in rows),
                                "default": all(r["c_below_b_beyond_spread"] and r["c_not_above_e_beyond_spread"] for r in rows),
                                "worst_c_over_b": max(r["c_over_b"] for r in rows), "worst_c_over_e": max(r["c_over_e"] for r in rows),
                                "worst_c_over_a": max(r["c_over_a"] for r in rows)}
    res["image_u8_off"] = sorted(f for f, v in res["families"].items() if not v["default"])
    res["image_u8_off_committed"] = sorted(cf.IMAGE_U8_OFF)
    if not a.no_net:
        res["nets"].append(bench_net(build_mobilenet, 256, a.steps))
        res["nets"].append(bench_net(build_resnet50, 128, a.steps))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
