#!/usr/bin/env python3
"""bench.py -- images/sec of the SLFP<3,4>-quantized conv2d hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W            (N = 1)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W     (N > 1, one rank per GPU over RCCL)

Workload (BASELINE.json, configs[1]): MobileNetV1 ImageNet 224x224, SLFP<3,4> (Qbits 8),
batch 256 PER GPU (weak scaling).  One "step" = one batch through ALL 27 Conv2d_Q layers of
the net -- the hot-path operator utils/conv2d_func.py:20-25 and nothing else --
each layer reading its own synthetic post-ReLU-like NHWC input that is already resident in
HBM, through the C ABI (slfp_conv2d_fwd), with weights prepared once (quantize-once cache).
Layer geometry and the per-layer Ka/Kw come from the reference's own tables
(cnns_slfp_quantization_amd/data/layer_specs.json).  Random-init weights, synthetic data.

Prints ONE JSON line on rank 0 (see README/DESIGN.md for the field meanings).  A plain run sets up, warms up, times
exactly K steps and reports them (`value`, `ms_per_step`); `--full` adds every secondary measurement (per-kernel and
roofline figures, the single-stream and float32-equivalent timings, the code path, BASELINE configs 3-5, the codec, the
whole net, the CPU baseline).  `--dump-outputs DIR` writes the layer outputs of the last timed step to DIR/*.npy.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cnns_slfp_quantization_amd import _lib, layer_specs, sharding  # noqa: E402

HBM_PEAK_GBS = 8000.0       # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
HBM_COPY_GBS = 6290.0       # measured float4-copy ceiling from the same guide
MFMA_F16_PEAK_TFLOPS = 2500.0  # dense fp16/bf16 MFMA peak (same guide; never the 2:1-sparsity figure)
DUMP_BUDGET_BYTES = 48 << 20   # --dump-outputs: all layers' outputs (or samples of them) together


class Layer:
    """One Conv2d_Q layer of the workload, bound to device buffers."""

    def __init__(self, L, spec, batch, dev, passes, gen, qbits=8, post=False):
        self.spec = spec
        self.batch = batch
        s = spec
        self.desc = _lib.ConvDesc(n=batch, c_in=s.c_in, h=s.h, w=s.w, c_out=s.c_out, kh=s.k[0], kw=s.k[1],
                                  stride_h=s.stride[0], stride_w=s.stride[1], pad_h=s.pad[0], pad_w=s.pad[1],
                                  dil_h=1, dil_w=1, groups=s.groups, x_layout=_lib.LAYOUT_NHWC,
                                  y_layout=_lib.LAYOUT_NHWC, qbits=qbits, ka=float(np.float32(s.Ka)),
                                  kw_scale=float(np.float32(s.Kw)), mfma_passes=passes, reserved=0)
        self.kernel = L.slfp_conv2d_kernel_name(ctypes.byref(self.desc)).decode()
        # synthetic post-ReLU-like activation spanning all 7 binades and both clamps;
        # the image stem gets a signed N(0,1)-like input
        x = torch.randn((batch, s.h, s.w, s.c_in), generator=gen, device=dev)
        x = x if s.c_in == 3 else x.abs_()
        self.x = x.mul_(4.0 * s.Ka)
        self.y = torch.empty((batch, s.h_out, s.w_out, s.c_out), device=dev)
        fan = (s.c_in // s.groups) * s.k[0] * s.k[1]
        self.w = torch.randn((s.c_out, s.c_in // s.groups, s.k[0], s.k[1]), generator=gen, device=dev)
        self.w.mul_(min(5.0 * s.Kw, 3.0 * (2.0 / fan) ** 0.5 + 2.0 * s.Kw))
        self.bias = torch.randn(s.c_out, generator=gen, device=dev) * 0.1 if s.bias else None
        self.blob = torch.empty(L.slfp_conv2d_wprep_bytes(ctypes.byref(self.desc)), dtype=torch.uint8, device=dev)
        ws = L.slfp_conv2d_workspace_bytes(ctypes.byref(self.desc))  # dense k x k layers: input encoded once to fp16
        self.ws = torch.empty(ws, dtype=torch.uint8, device=dev) if ws else None
        self.bytes = spec.algorithmic_bytes(batch)
        # --post: the fused eval-BN + ReLU epilogue (slfp_conv2d_fwd_post) on every layer, to price it
        self.post = (torch.rand(s.c_out, generator=gen, device=dev) + 0.5,
                     torch.randn(s.c_out, generator=gen, device=dev) * 0.1) if post else None

    def set_passes(self, L, stream, passes):
        """Switch the MFMA precision mode.  The prepared blob is specific to the kernel family the
        descriptor selects (a dense k x k layer is an fp16 fragment blob in single-pass mode and a
        float32 HWIO blob in float32-equivalent mode), so it is rebuilt when the family changes."""
        self.desc.mfma_passes = passes
        kernel = L.slfp_conv2d_kernel_name(ctypes.byref(self.desc)).decode()
        if kernel != self.kernel:
            self.kernel = kernel
            self.blob = torch.empty(L.slfp_conv2d_wprep_bytes(ctypes.byref(self.desc)), dtype=torch.uint8, device=self.x.device)
            ws = L.slfp_conv2d_workspace_bytes(ctypes.byref(self.desc))
            self.ws = torch.empty(ws, dtype=torch.uint8, device=self.x.device) if ws else None
            self.prepare(L, stream)

    def prepare(self, L, stream):
        _lib.check(L.slfp_conv2d_prepare_weights(ctypes.byref(self.desc), self.w.data_ptr(), self.blob.data_ptr(),
                                                 None, stream))

    def encode_codes(self, L, stream):
        """u8 codes of QW(w / Kw) (1 B per weight, extended code points): what travels between ranks."""
        fmt = (_lib.FMT_W8 if self.desc.qbits == 8 else _lib.FMT_SFP7) | _lib.FMT_EXT
        codes = torch.empty(self.w.numel(), dtype=torch.uint8, device=self.w.device)
        _lib.check(L.slfp_encode_f32(self.w.data_ptr(), codes.data_ptr(), self.w.numel(), float(self.desc.kw_scale), fmt, stream))
        return codes

    def prepare_from_codes(self, L, stream, codes):
        _lib.check(L.slfp_conv2d_prepare_weights_codes(ctypes.byref(self.desc), codes.data_ptr(), self.blob.data_ptr(), None, stream))

    def run(self, L, stream):
        if self.post is not None:
            rc = L.slfp_conv2d_fwd_post(ctypes.byref(self.desc), self.x.data_ptr(), self.blob.data_ptr(),
                                        self.bias.data_ptr() if self.bias is not None else None,
                                        self.post[0].data_ptr(), self.post[1].data_ptr(), 1, self.y.data_ptr(),
                                        None, self.ws.data_ptr() if self.ws is not None else None, stream)
            if rc != 0:
                _lib.check(rc)
            return
        rc = L.slfp_conv2d_fwd(ctypes.byref(self.desc), self.x.data_ptr(), self.blob.data_ptr(),
                               self.bias.data_ptr() if self.bias is not None else None, self.y.data_ptr(),
                               None, self.ws.data_ptr() if self.ws is not None else None, stream)
        if rc != 0:
            _lib.check(rc)


FAMILY_KERNELS = {"dw3x3_nhwc": ("k_dw3x3",), "stem_nhwc": ("k_stem", "k_stem_fixed"), "direct_nhwc": ("k_direct",),
                  "pw_mfma_f16x1": ("k_pw_stream", "k_pw_tiled"), "pw_mfma_f16x3": ("k_pw_stream", "k_pw_tiled"),
                  "pw_mfma_f16_exact": ("k_pw_stream", "k_pw_tiled"),
                  "dense_mfma_f16x1": ("k_dense_mfma", "k_dense3x3", "k_dense3x3_res", "k_dense_encode"), "dense_mfma_f16x3": ("k_dense_mfma", "k_dense_encode"),
                  "dense_mfma_f16_exact": ("k_dense_mfma", "k_dense3x3", "k_dense3x3_res", "k_dense_encode"),
                  "stem_mfma_f16x1": ("k_stem_mfma", "k_stem_im2row"), "stem_mfma_f16_exact": ("k_stem_mfma", "k_stem_im2row"),
                  "stem_small_mfma_f16x1": ("k_stem_small",), "stem_small_mfma_f16_exact": ("k_stem_small",),
                  # the code path (run_codes_config): families of slfp_conv2d_fwd_codes
                  "stem_codes": ("k_stem_mx", "k_stem_fixed"), "dw3x3_codes": ("k_dwc",),
                  "pw_mfma_codes": ("k_pwc_stream", "k_pwc_tiled", "k_pwc_slice"),
                  "dense_mfma_codes": ("k_dense_mfma", "k_dense3x3", "k_dense_decode", "k_dense_encode")}


PREPASS_KERNELS = ("k_dense_encode", "k_dense_decode", "k_stem_im2row")


def pmc_traffic(family, net, batch):
    """HBM bytes per launch of `family` from the newest committed rocprofv3 PMC summary of THIS workload
    (profiles/index.json lists tag -> net, batch, oldest first; profiles/<tag>_summary.json holds
    FETCH_SIZE x 2 (gfx950 correction) + WRITE_SIZE from separate --pmc passes of this same bench
    command).  Returns (bytes_per_launch, tag) or (None, None)."""
    try:
        index = json.load(open(os.path.join(ROOT, "profiles", "index.json")))
    except OSError:
        return None, None
    for ent in reversed(index):
        if ent["net"] != net or ent["batch"] != batch:
            continue
        path = os.path.join(ROOT, "profiles", ent["tag"] + "_summary.json")
        if not os.path.exists(path):
            continue
        tot = n = 0
        launches = None
        for r in json.load(open(path)):
            if r["kernel"].split("<")[0] in FAMILY_KERNELS.get(family, ()) and "hbm_read_MB" in r and "hbm_write_MB" in r:
                tot += (r["hbm_read_MB"] + r["hbm_write_MB"]) * 1e6 * r["launches"]
                if r["kernel"].split("<")[0] not in PREPASS_KERNELS:
                    n += r["launches"]   # a pre-pass kernel adds bytes to its layer's launch, not a launch
        if n:
            return int(tot / n), ent["tag"]
    return None, None


def whole_net(specs, net, batch, dev, steps):
    """Secondary, clearly labelled number: the whole MobileNetV1 through this repo's
    drop-in modules INCLUDING the stock nn.BatchNorm2d / nn.ReLU / AvgPool2d / Linear between
    and after the convs (nets_imgnet/mobilenetv1.py:43-61), channels_last, eval, no_grad -- and
    the same net after fusion.fuse_bn_relu (eval-BN + ReLU folded into the conv epilogues)."""
    import torch.nn as nn
    import utils.conv2d_func as cf
    from cnns_slfp_quantization_amd import fusion
    if net != "mobilenetv1_imagenet224":
        return None
    layers = []
    for s in specs:
        conv = cf.conv2d_Q(q_bit=8, Kw=np.float64(s.Kw), Ka=np.float64(s.Ka))(
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
    x = torch.randn((batch, 3, 224, 224), device=dev, generator=g).contiguous(memory_format=torch.channels_last)
    out = {}
    with torch.no_grad():
        for tag in ("stock_bn_relu", "fused_bn_relu", "fused_dw_pw"):   # then "fused_codes" below
            if tag == "fused_bn_relu":
                fusion.fuse_bn_relu(model)
            if tag == "fused_dw_pw":   # MobileNet blocks as ONE kernel each where libslfp_hip supports the pair (csrc/conv_dwpw.hip)
                out["dw_pw_blocks_formed"] = fusion.fuse_dw_pw(model)
            for _ in range(2):
                model(x)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                model(x)
            torch.cuda.synchronize()
            out[tag] = round(batch * steps / (time.perf_counter() - t0), 1)
        out["dw_pw_blocks_one_kernel"] = sum(1 for m in model.modules() if isinstance(m, fusion.DwPwBlock) and m._last_kernel)
        # later measurements in one process run a little faster (clocks / allocator warm): measure the two-kernel net again
        # AFTER the paired one so that the comparison is not an ordering artefact, and keep its better number
        fusion.unfuse_dw_pw(model)
        for _ in range(2):
            model(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            model(x)
        torch.cuda.synchronize()
        out["fused_bn_relu"] = max(out["fused_bn_relu"], round(batch * steps / (time.perf_counter() - t0), 1))
        # the fused net with every conv -> conv hand-over as 1-byte SLFP codes (fusion.link_codes; bit-identical logits)
        try:
            y_fused = model(x)
            out["code_links"] = fusion.link_codes(model, example_input=x)
            for _ in range(2):
                y_codes = model(x)
            out["fused_codes_matches_fused"] = bool(torch.equal(y_codes, y_fused))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                model(x)
            torch.cuda.synchronize()
            out["fused_codes"] = round(batch * steps / (time.perf_counter() - t0), 1)
        except Exception as e:  # secondary number
            out["fused_codes"] = None
            out["fused_codes_error"] = str(e)[:200]
        best = max((out.get("fused_codes") or 0, "fused_codes"), (out["fused_bn_relu"], "fused_bn_relu"), (out["fused_dw_pw"], "fused_dw_pw"))[1]
        if best != "fused_codes":
            fusion.unlink_codes(model)
        if best == "fused_dw_pw":
            fusion.fuse_dw_pw(model)
        out["hipgraph_net"] = best
        # the fused net replayed as ONE hipGraph (all launches go to the capture stream through the C ABI):
        # removes the per-layer Python/launch latency and the inter-kernel gaps
        try:
            static_x = x.clone()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    model(static_x)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                static_y = model(static_x)
            graph.replay()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                graph.replay()
            torch.cuda.synchronize()
            out["fused_hipgraph"] = round(batch * steps / (time.perf_counter() - t0), 1)
            ref_y = model(static_x)
            out["hipgraph_matches_eager"] = bool(torch.equal(ref_y, static_y))
        except Exception as e:  # graph capture is an optimisation of the secondary number only
            out["fused_hipgraph"] = None
            out["hipgraph_error"] = str(e)[:200]
    # small batch: host- and launch-bound eager vs graph.GraphedModule (one hipGraph per input signature)
    try:
        from cnns_slfp_quantization_amd.graph import GraphedModule
        xs = x[:8].contiguous(memory_format=torch.channels_last)
        fast = GraphedModule(model)
        small = {}
        with torch.no_grad():
            for tag, fn in (("eager", model), ("hipgraph", fast)):
                for _ in range(3):
                    fn(xs)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(50):
                    fn(xs)
                torch.cuda.synchronize()
                small[tag] = round(8 * 50 / (time.perf_counter() - t0), 1)
            small["hipgraph_matches_eager"] = bool(torch.equal(fast(xs), model(xs)))
        out["batch8"] = small
    except Exception as e:  # secondary number only
        out["batch8"] = {"error": str(e)[:200]}
    out["unit"] = "images/sec"
    out["note"] = ("whole MobileNetV1-224 incl. BN/ReLU/pool/fc through the drop-in modules, 1 GPU, batch %d; fused_dw_pw = "
                   "fused_bn_relu + the depthwise/pointwise pairs run as ONE kernel where that measured at least as fast as two (the "
                   "32-channel stride-1 block; options.dwpw_all forces every supported pair; bit-identical either way, DESIGN.md "
                   "section 4); fused_hipgraph = the faster net replayed as one hipGraph" % batch)
    return out


def cpu_baseline(specs, sample_batch, iters):
    """The reference's CPU path re-stated with the same ATen op sequence (oracle/torch_port.py,
    proven bit-identical to the reference in the build container), timed on this box's
    host cores on a bounded sample of the same workload."""
    from oracle import torch_port as tp
    # the GPU box gives one GPU a 16-core CPU share; os.cpu_count() reports the whole host
    try:
        ncpu = len(os.sched_getaffinity(0))
    except AttributeError:
        ncpu = os.cpu_count() or 1
    torch.set_num_threads(max(1, min(ncpu, 16)))
    g = torch.Generator().manual_seed(0)
    data = []
    for s in specs:
        x = torch.randn((sample_batch, s.c_in, s.h, s.w), generator=g)
        x = (x if s.c_in == 3 else x.abs()) * (4.0 * s.Ka)
        w = torch.randn((s.c_out, s.c_in // s.groups, s.k[0], s.k[1]), generator=g) * (5.0 * s.Kw)
        b = torch.randn(s.c_out, generator=g) * 0.1 if s.bias else None
        data.append((s, x, w, b))

    def one_pass():
        with torch.no_grad():
            for s, x, w, b in data:
                tp.conv2d_q(x, w, b, s.stride, s.pad, 1, s.groups, np.float64(s.Ka), np.float64(s.Kw), 8)

    t0 = time.perf_counter()
    one_pass()  # warm-up, also sizes the sample: about 10 s of CPU work
    t_pass = time.perf_counter() - t0
    iters = max(iters, min(40, int(10.0 / max(t_pass, 1e-3))))
    t0 = time.perf_counter()
    for _ in range(iters):
        one_pass()
    dt = time.perf_counter() - t0
    return {"value": round(sample_batch * iters / dt, 3), "unit": "images/sec", "cores": torch.get_num_threads(),
            "kind": "port",
            "sample": f"{iters} x batch {sample_batch} through the same {len(specs)} Conv2d_Q layers, "
                      f"oracle/torch_port.py (the reference's ATen op sequence minus its three .clone() passes per "
                      f"quantizer: ~1.7x faster than the reference's own modules on the same layer, i.e. a conservative "
                      f"baseline) on PyTorch-CPU, no_grad"}


def pmc_field(family, net, batch, field):
    """Launch-weighted mean of a derived field (e.g. mfma_busy_frac) of `family` in the newest committed PMC summary."""
    try:
        index = json.load(open(os.path.join(ROOT, "profiles", "index.json")))
    except OSError:
        return None
    for ent in reversed(index):
        if ent["net"] != net or ent["batch"] != batch:
            continue
        path = os.path.join(ROOT, "profiles", ent["tag"] + "_summary.json")
        if not os.path.exists(path):
            continue
        tot = n = 0.0
        for r in json.load(open(path)):
            if r["kernel"].split("<")[0] in FAMILY_KERNELS.get(family, ()) and field in r:
                w = r["launches"] * r.get("avg_us", 1.0)
                tot += r[field] * w
                n += w
        if n:
            return round(tot / n, 4)
    return None


def timed_steps(step, steps, world, dev):
    """EXACTLY `steps` steps between barrier + synchronize on both sides; returns this rank's seconds."""
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


_GROUP_STREAMS = {}


def group_stream(dev, g):
    """The HIP stream of image group g: created once per process and reused by every measurement.  (HIP maps streams to a few
    hardware queues; two streams that land on the same queue serialise -- profiles/two_streams.py measured 110 k images/s on a
    freshly created SECOND pair of streams against 129 k on the first pair -- so the streams are kept for the process, and
    run_config tries the pairs among the first four once and keeps one that overlaps.)"""
    key = (dev.index, g)
    if key not in _GROUP_STREAMS:
        _GROUP_STREAMS[key] = torch.cuda.Stream(device=dev)
    return _GROUP_STREAMS[key]


def sample_outputs(layer_ys, seed=0, budget_bytes=DUMP_BUDGET_BYTES):
    """What a caller of the timed path receives from one step: every layer's float32 output over the whole batch.
    layer_ys[i] lists layer i's output tensors in batch order (one per image group).  A layer's output is returned whole
    (NHWC) when it fits its share of `budget_bytes`, else as a fixed sample of its elements: the same flat positions of
    the whole-batch NHWC tensor on every run, chosen by a generator seeded with (seed, layer index), in ascending order."""
    cap = max(1, budget_bytes // 4 // len(layer_ys))
    out = {}
    for i, ys in enumerate(layer_ys):
        per = ys[0].numel()
        n = per * len(ys)
        if n <= cap:
            y = torch.cat([t.reshape(-1) for t in ys]).view(len(ys) * ys[0].shape[0], *ys[0].shape[1:])
        else:
            idx = torch.from_numpy(np.sort(np.random.default_rng([seed, i]).choice(n, size=cap, replace=False))).to(ys[0].device)
            y = torch.empty(cap, dtype=ys[0].dtype, device=ys[0].device)
            for g, t in enumerate(ys):
                sel = (idx >= g * per) & (idx < (g + 1) * per)
                y[sel] = t.reshape(-1)[idx[sel] - g * per]
        out[f"layer{i:02d}_y"] = y.float().cpu().numpy()
    return out


def run_config(L, net, batch, qbits, passes, steps, warmup, dev, rank, world, post=False, per_layer=False, exact_too=False,
               image_groups=1, full=True, dump=None):
    """One workload: every Conv2d_Q layer of `net` at `batch` images on this rank.  Returns (result dict, per-rank seconds).
    image_groups = G > 1: the timed steps run the batch as G groups of batch / G images, each group on its own HIP stream
    through all the layers (images are independent units of this path -- SURVEY 8e -- so the groups never synchronise: while
    one group's kernel drains its last workgroups, another group's kernel fills the CUs; the per-launch gap of one stream is
    the other's work).  Same weights (one prepared blob per layer), same images per step; the per-kernel figures of the
    result are measured on whole-batch launches in a separate single-stream pass, which is also reported.
    full=False times the headline steps and nothing else: no single-stream timing next to the image groups, no per-kernel
    pass (no `roofline` / `kernels`; per_layer still runs that pass), no float32-equivalent or north-star-scope timing.
    dump: a dict that receives sample_outputs() of the timed path right after its timed steps."""
    specs = layer_specs.conv_layers(net)
    gen = torch.Generator(device=dev).manual_seed(1234 + rank)
    layers = [Layer(L, s, batch, dev, passes, gen, qbits, post) for s in specs]
    stream = torch.cuda.current_stream().cuda_stream
    # Quantized weights: rank 0 encodes them ONCE to u8 codes (1 B per weight), the codes of all layers travel as one
    # bucket (the only collective of the whole path: RCCL broadcast over xGMI, sharding.py), and every rank lays them
    # out for its own kernels (slfp_conv2d_prepare_weights_codes: identical to preparing from the weights).
    if world > 1:
        codes = [l.encode_codes(L, stream) if rank == 0 else torch.empty(l.w.numel(), dtype=torch.uint8, device=dev) for l in layers]
        torch.cuda.synchronize()
        sharding.broadcast_blobs(codes, src=0)
        for l, c in zip(layers, codes):
            l.prepare_from_codes(L, stream, c)
        del codes
    else:
        for l in layers:
            l.prepare(L, stream)
    torch.cuda.synchronize()

    def step():
        for l in layers:
            l.run(L, stream)

    grouped = image_groups > 1 and batch % image_groups == 0
    single = None
    if full or not grouped:
        for _ in range(warmup):
            step()
        dt_rank = timed_steps(step, steps, world, dev)
        rank_dts = sharding.rank_times(dt_rank, device=dev)   # every rank's seconds; the job's time is the slowest rank's
        dt = max(rank_dts)
        if grouped:
            single = {"value": round(batch * world * steps / dt, 1), "ms_per_step": round(dt / steps * 1e3, 4)}
        elif dump is not None:
            dump.update(sample_outputs([[l.y] for l in layers]))
    if grouped:
        groups = []
        for g in range(image_groups):
            st = group_stream(dev, g)
            gl = [Layer(L, s, batch // image_groups, dev, passes, gen, qbits, post) for s in specs]
            for a, b in zip(gl, layers):
                a.blob = b.blob            # ONE prepared weight blob per layer, shared by the groups
            groups.append([st.cuda_stream, gl])
        torch.cuda.synchronize()

        def gstep():
            for i in range(len(specs)):    # the groups' launches interleaved layer by layer; the streams run free
                for sh, gl in groups:
                    gl[i].run(L, sh)

        if image_groups == 2 and (dev.index, "pair") not in _GROUP_STREAMS:
            # two streams that HIP placed on one hardware queue serialise (profiles/stream_pairs.py): try the pairs among four
            # candidate streams for a few steps each, once per process, and keep the pair that overlaps
            cand = [group_stream(dev, g) for g in range(4)]
            best = None
            for a, b in ((0, 1), (2, 3), (0, 2), (1, 3), (0, 3), (1, 2)):
                groups[0][0], groups[1][0] = cand[a].cuda_stream, cand[b].cuda_stream
                gstep()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(4):
                    gstep()
                torch.cuda.synchronize()
                t = time.perf_counter() - t0
                if best is None or t < best[0]:
                    best = (t, a, b)
            _GROUP_STREAMS[(dev.index, "pair")] = (cand[best[1]], cand[best[2]])
        if image_groups == 2:
            pa, pb = _GROUP_STREAMS[(dev.index, "pair")]
            groups[0][0], groups[1][0] = pa.cuda_stream, pb.cuda_stream

        for _ in range(warmup):
            gstep()
        dt_rank = timed_steps(gstep, steps, world, dev)
        rank_dts = sharding.rank_times(dt_rank, device=dev)
        dt = max(rank_dts)
        if dump is not None:
            dump.update(sample_outputs([[gl[i].y for _, gl in groups] for i in range(len(specs))]))
        del groups

    imgs = batch * world * steps
    value = imgs / dt
    bytes_img = layer_specs.algorithmic_bytes_per_image(net, batch)
    whole_gbs = bytes_img * value / 1e9 / world  # per GPU
    res = {"value": round(value, 1), "ms_per_step": round(dt / steps * 1e3, 4),
           "hbm_roofline_frac_whole_path": round(whole_gbs / HBM_PEAK_GBS, 4),
           "algorithmic_bytes_per_image": int(bytes_img),
           "pointwise_mfma": next((l.kernel for l in layers if l.kernel.startswith("pw_")), None),
           "n_layers": len(layers)}
    if grouped:
        res["image_groups"] = image_groups
    if not (full or per_layer):
        del layers
        torch.cuda.empty_cache()
        return res, rank_dts

    # ---- per-kernel timing with HIP events on the launch stream (separate pass, same step order: cold caches)
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in layers] for _ in range(steps)]
    for k in range(steps):
        for i, l in enumerate(layers):
            ev[k][i][0].record()
            l.run(L, stream)
            ev[k][i][1].record()
    torch.cuda.synchronize()
    layer_ms = [float(np.mean([ev[k][i][0].elapsed_time(ev[k][i][1]) for k in range(steps)])) for i in range(len(layers))]
    fam = {}
    for l, ms in zip(layers, layer_ms):
        f = fam.setdefault(l.kernel, {"ms": 0.0, "bytes": 0, "launches": 0, "flops": 0})
        f["ms"] += ms
        f["bytes"] += l.bytes
        f["flops"] += 2 * l.spec.macs * l.batch
        f["launches"] += 1
    dominant = max(fam, key=lambda k: fam[k]["ms"])
    dom = fam[dominant]
    dom_gbs = dom["bytes"] / (dom["ms"] * 1e-3) / 1e9

    exact_value = None
    if exact_too and full and passes == 0 and qbits == 8:   # the float32-equivalent mode (fp16 hi/lo split, 3 MFMA passes), same buffers
        for l in layers:
            l.set_passes(L, stream, _lib.MFMA_F16X3)
        step()
        dte = max(sharding.rank_times(timed_steps(step, steps, world, dev), device=dev))
        exact_value = batch * world * steps / dte
        for l in layers:
            l.set_passes(L, stream, passes)

    # the north-star scope by itself (BASELINE.json: "3x3 depthwise + 1x1 pointwise"): the same steps WITHOUT the image stem, by
    # the wall clock -- the per-family HIP-event sums above carry ~2 us of event overhead per launch that a step does not have
    scope = None
    if exact_too and full and world == 1:
        sub = [l for l in layers if l.spec.c_in > 4]
        if len(sub) != len(layers) and sub:
            def sub_step():
                for l in sub:
                    l.run(L, stream)
            for _ in range(max(1, warmup // 4)):
                sub_step()
            dts = timed_steps(sub_step, steps, 1, dev)
            sub_bytes = sum(l.bytes for l in sub)
            scope = {"layers": len(sub), "ms_per_step": round(dts / steps * 1e3, 4),
                     "achieved_GB/s": round(sub_bytes * steps / dts / 1e9, 1),
                     "hbm_roofline_frac": round(sub_bytes * steps / dts / 1e9 / HBM_PEAK_GBS, 4),
                     "note": "depthwise + pointwise layers only (no stem), wall clock over the same number of steps"}

    res.update({
        "roofline": {"bound": "hbm", "kernel": dominant, "achieved": round(dom_gbs, 1), "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": round(dom_gbs / HBM_PEAK_GBS, 4),
                     "frac_of_measured_copy_ceiling": round(dom_gbs / HBM_COPY_GBS, 4),
                     "traffic": pmc_traffic(dominant, net, batch)[0],
                     "traffic_profile": pmc_traffic(dominant, net, batch)[1],
                     "mfma_busy_frac": pmc_field(dominant, net, batch, "mfma_busy_frac"),
                     "launches_per_step": dom["launches"], "avg_launch_ms": round(dom["ms"] / dom["launches"], 4),
                     "algorithmic_bytes_per_launch": int(dom["bytes"] / dom["launches"])},
        "kernels": {k: {"ms_per_step": round(v["ms"], 4), "GB/s": round(v["bytes"] / (v["ms"] * 1e-3) / 1e9, 1),
                        "TFLOP/s": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1), "launches": v["launches"]}
                    for k, v in fam.items()},
    })
    if dominant.startswith(("dense_mfma", "stem_mfma_")):
        # compute-bound families (VGG-16 / ResNet-50 3x3, large stems): price against the matrix cores.
        # achieved = algorithmic flops (2 * MACs of the layers) / measured time incl. the fp16 encode pre-pass
        tf = dom["flops"] / (dom["ms"] * 1e-3) / 1e12
        res["roofline"] = {"bound": "mfma", "kernel": dominant, "achieved": round(tf, 1), "peak": MFMA_F16_PEAK_TFLOPS,
                           "unit": "TFLOP/s", "frac": round(tf / MFMA_F16_PEAK_TFLOPS, 4), "traffic": None,
                           "mfma_busy_frac": pmc_field(dominant, net, batch, "mfma_busy_frac"),
                           "launches_per_step": dom["launches"], "avg_launch_ms": round(dom["ms"] / dom["launches"], 4),
                           "algorithmic_flops_per_launch": int(dom["flops"] / dom["launches"])}
    if exact_value is not None:
        res["value_pointwise_f16x3_float32_equivalent"] = round(exact_value, 1)
    if scope is not None:
        res["dw_pw_scope"] = scope
    if single is not None:
        single["hbm_roofline_frac_whole_path"] = round(bytes_img * single["value"] / 1e9 / world / HBM_PEAK_GBS, 4)
        res["single_stream"] = single
    if per_layer and rank == 0:
        for l, ms in zip(layers, layer_ms):
            sp = l.spec
            print(f"  {l.kernel:18s} {sp.c_in:4d}->{sp.c_out:4d} k{sp.k[0]} s{sp.stride[0]} {sp.h:3d}->{sp.h_out:3d}  "
                  f"{ms:8.4f} ms  {l.bytes / ms / 1e6:8.1f} GB/s", file=sys.stderr)
    del layers
    torch.cuda.empty_cache()
    return res, rank_dts


def run_codes_config(L, net, batch, qbits, steps, warmup, dev, image_groups=1):
    """The same conv layers with 1-byte activation codes on every hand-over fusion.link_codes can make (SURVEY 8f rank 1,
    second half; slfp_conv2d_fwd_codes_ws): every layer with the fused BatchNorm + ReLU epilogue; MobileNetV1: ONE chain, the stem
    reading float32 images and writing the next layer's codes, every other layer reading codes (of its own synthetic input,
    resident in HBM) and writing codes, the last one writing float32; VGG-16: the conv -> conv hand-overs inside a stage.  Algorithmic bytes: 1 B per activation element on a code side, 4 B on a float32 side, weights once
    per batch.  Bit-identical to the float32 interface (tests/test_gpu_codes.py); single-pass MFMA mode."""
    specs = layer_specs.conv_layers(net)
    gen = torch.Generator(device=dev).manual_seed(4321)
    stream = torch.cuda.current_stream().cuda_stream
    fmt = (_lib.FMT_ACT8 if qbits == 8 else _lib.FMT_SFP7) | _lib.FMT_EXT

    def direct(i):
        """Does layer i's (fused BN + ReLU) output feed layer i+1 directly, as fusion.link_codes requires?  MobileNetV1: always
        (nets_imgnet/mobilenetv1.py:43-57); VGG-16: inside a stage, and from one stage to the next through its MaxPool2d, which
        pools the codes (slfp_maxpool2d_codes; nets_cifar/vgg16.py:30-92) -- the pool itself is outside the conv path on either
        interface."""
        if i < 0 or i + 1 >= len(specs):
            return False
        a, b = specs[i], specs[i + 1]
        same = a.h_out == b.h and a.w_out == b.w
        pooled = net.startswith("vgg16") and a.h_out == 2 * b.h and a.w_out == 2 * b.w
        return a.c_out == b.c_in and (same or pooled)

    # a hand-over becomes codes where both kernels exist: decided left to right, as link_codes does
    x_codes = [False] * len(specs)
    y_codes = [False] * len(specs)
    descs = []
    for s in specs:
        descs.append(_lib.ConvDesc(n=batch, c_in=s.c_in, h=s.h, w=s.w, c_out=s.c_out, kh=s.k[0], kw=s.k[1], stride_h=s.stride[0],
                                   stride_w=s.stride[1], pad_h=s.pad[0], pad_w=s.pad[1], dil_h=1, dil_w=1, groups=s.groups,
                                   x_layout=_lib.LAYOUT_NHWC, y_layout=_lib.LAYOUT_NHWC, qbits=qbits, ka=float(np.float32(s.Ka)),
                                   kw_scale=float(np.float32(s.Kw)), mfma_passes=_lib.MFMA_F16X1, reserved=0))

    def ok(i, xin, yout):
        io = _lib.ConvIo(x_codes=1 if xin else 0, y_codes=1 if yout else 0,
                         y_ka=float(np.float32(specs[i + 1].Ka)) if yout else 1.0, y_qbits=qbits)
        return bool(L.slfp_conv2d_codes_supported(ctypes.byref(descs[i]), ctypes.byref(io), 0, 1))

    for i in range(len(specs) - 1):
        if direct(i) and ok(i, x_codes[i], True) and ok(i + 1, True, False):
            y_codes[i] = x_codes[i + 1] = True
    if not any(y_codes):
        return None
    def make_layers(nb, share=None):
        out_layers = []
        for i, s in enumerate(specs):
            l = Layer(L, s, nb, dev, _lib.MFMA_F16X1, gen, qbits, post=True)
            if share is not None:
                l.blob, l.post, l.bias = share[i].blob, share[i].post, share[i].bias   # one set of weights / BN vectors
            else:
                l.prepare(L, stream)
            _finish_layer(l, i, s, nb)
            out_layers.append(l)
        return out_layers

    def _finish_layer(l, i, s, nb):
        l.io = _lib.ConvIo(x_codes=1 if x_codes[i] else 0, y_codes=1 if y_codes[i] else 0,
                           y_ka=float(np.float32(specs[i + 1].Ka)) if y_codes[i] else 1.0, y_qbits=qbits)
        l.on_codes = x_codes[i] or y_codes[i]
        if x_codes[i]:
            xc = torch.empty(l.x.shape, dtype=torch.uint8, device=dev)
            _lib.check(L.slfp_encode_f32(l.x.data_ptr(), xc.data_ptr(), l.x.numel(), float(l.desc.ka), fmt, stream))
            l.x = xc
        if y_codes[i]:
            l.y = torch.empty(l.y.shape, dtype=torch.uint8, device=dev)
        l.cbytes = nb * (s.in_elems * (1 if x_codes[i] else 4) + s.out_elems * (1 if y_codes[i] else 4)) + 4 * s.w_elems
        base = "stem" if s.c_in == 3 else ("dw3x3" if s.groups > 1 else ("pw_mfma" if s.k == (1, 1) else "dense_mfma"))
        l.family = base + ("_codes" if l.on_codes else "_float32")

    layers = make_layers(batch)
    torch.cuda.synchronize()

    def run(l, sh=None):
        sh = stream if sh is None else sh
        if not l.on_codes:   # a layer with float32 on both sides: the float32 interface
            l.run(L, sh)
            return
        rc = L.slfp_conv2d_fwd_codes_ws(ctypes.byref(l.desc), ctypes.byref(l.io), l.x.data_ptr(), l.blob.data_ptr(),
                                        l.bias.data_ptr() if l.bias is not None else None,
                                        l.post[0].data_ptr(), l.post[1].data_ptr(), 1, l.y.data_ptr(),
                                        l.ws.data_ptr() if l.ws is not None else None, sh)
        if rc != 0:
            _lib.check(rc)

    def step():
        for l in layers:
            run(l)

    for _ in range(warmup):
        step()
    dt = timed_steps(step, steps, 1, dev)
    single = None
    if image_groups > 1 and batch % image_groups == 0:   # the batch as independent image groups on as many HIP streams (run_config)
        single = {"value": round(batch * steps / dt, 1), "ms_per_step": round(dt / steps * 1e3, 4)}
        groups = [(group_stream(dev, g).cuda_stream, make_layers(batch // image_groups, share=layers)) for g in range(image_groups)]
        torch.cuda.synchronize()

        def gstep():
            for i in range(len(specs)):
                for sh, gl in groups:
                    run(gl[i], sh)

        for _ in range(warmup):
            gstep()
        dt = timed_steps(gstep, steps, 1, dev)
        del groups
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in layers] for _ in range(steps)]
    for k in range(steps):
        for i, l in enumerate(layers):
            ev[k][i][0].record()
            run(l)
            ev[k][i][1].record()
    torch.cuda.synchronize()
    layer_ms = [float(np.mean([ev[k][i][0].elapsed_time(ev[k][i][1]) for k in range(steps)])) for i in range(len(layers))]
    fam = {}
    for l, ms in zip(layers, layer_ms):
        f = fam.setdefault(l.family, {"ms": 0.0, "bytes": 0, "launches": 0})
        f["ms"] += ms
        f["bytes"] += l.cbytes
        f["launches"] += 1
    dominant = max(fam, key=lambda k: fam[k]["ms"])
    dom = fam[dominant]
    dom_gbs = dom["bytes"] / (dom["ms"] * 1e-3) / 1e9
    value = batch * steps / dt
    bytes_img = sum(l.cbytes for l in layers) / batch
    f32_bytes_img = layer_specs.algorithmic_bytes_per_image(net, batch)
    res = {"value": round(value, 1), "unit": "images/sec", "ms_per_step": round(dt / steps * 1e3, 4),
           "image_groups": image_groups if single is not None else 1, "single_stream": single,
           "algorithmic_bytes_per_image": int(bytes_img),
           "hbm_roofline_frac_whole_path": round(bytes_img * value / 1e9 / HBM_PEAK_GBS, 4),
           "float32_interface_bytes_equivalent_frac": round(f32_bytes_img * value / 1e9 / HBM_PEAK_GBS, 4),
           "roofline": {"bound": "hbm", "kernel": dominant, "achieved": round(dom_gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": round(dom_gbs / HBM_PEAK_GBS, 4), "traffic": pmc_traffic(dominant, net + "+codes", batch)[0],
                        "launches_per_step": dom["launches"], "avg_launch_ms": round(dom["ms"] / dom["launches"], 4),
                        "algorithmic_bytes_per_launch": int(dom["bytes"] / dom["launches"])},
           "kernels": {k: {"ms_per_step": round(v["ms"], 4), "GB/s": round(v["bytes"] / (v["ms"] * 1e-3) / 1e9, 1), "launches": v["launches"]}
                       for k, v in fam.items()},
           "note": "every layer with the fused BN + ReLU epilogue; activations between layers as 1-byte SLFP codes (1 B/elem "
                   "algorithmic); bit-identical to the float32 interface; these kernels are VALU-issue-bound, not HBM-bound "
                   "(profiles/r03c*): `float32_interface_bytes_equivalent_frac` prices the same images/s with the float32 "
                   "interface's bytes"}
    del layers
    torch.cuda.empty_cache()
    return res


def codec_bench(L, dev, n=1 << 28, reps=5):
    """the standalone codec as a bandwidth kernel -- slfp_quantize_f32 (4 B in + 4 B out per
    element) and slfp_encode_f32 (4 B in + 1 B out) on 1 GiB of float32, HIP events on the launch stream."""
    x = torch.randn(n, device=dev).abs_().mul_(2.0)
    y = torch.empty_like(x)
    c = torch.empty(n, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    out = {"elements": n}
    for name, fn, bpe in (("quantize_act8", lambda: L.slfp_quantize_f32(x.data_ptr(), y.data_ptr(), n, 0.17, _lib.FMT_ACT8, stream), 8),
                          ("encode_act8", lambda: L.slfp_encode_f32(x.data_ptr(), c.data_ptr(), n, 0.17, _lib.FMT_ACT8, stream), 5),
                          ("quantize_sfp7", lambda: L.slfp_quantize_f32(x.data_ptr(), y.data_ptr(), n, 0.17, _lib.FMT_SFP7, stream), 8)):
        _lib.check(fn())
        torch.cuda.synchronize()
        best = 1e9
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); _lib.check(fn()); e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1))
        gbs = n * bpe / (best * 1e-3) / 1e9
        out[name] = {"GB/s": round(gbs, 1), "frac_of_8TBs": round(gbs / HBM_PEAK_GBS, 4), "ms": round(best, 4), "bytes_per_element": bpe}
    del x, y, c
    torch.cuda.empty_cache()
    return out


# BASELINE.json configs 3-5 at their named batch sizes (config 4: the per-GPU slice of global batch 1024 on 8 GPUs)
OTHER_CONFIGS = (("vgg16_224", 128, 8), ("resnet50_imagenet224", 128, 8), ("squeezenet1_0_imagenet224", 256, 7),
                 ("shufflenetv2_224", 256, 7))


def _positive(s):
    v = int(s)
    if v < 1:
        raise argparse.ArgumentTypeError("must be at least 1")
    return v


def _non_negative(s):
    v = int(s)
    if v < 0:
        raise argparse.ArgumentTypeError("must be at least 0")
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # 200 timed steps after 100 warm-up steps (0.65 s of GPU time): the step time settles ~1.3 % below what 20 steps after 5 show
    # (clocks and the Infinity Cache reach their steady state) and repeats within +-0.1 % on one box (profiles/ab_env_long.sh)
    ap.add_argument("--steps", type=_positive, default=200)
    ap.add_argument("--warmup", type=_non_negative, default=100)
    ap.add_argument("--full", action="store_true",
                    help="also run every secondary measurement: the single-stream timing next to the image groups, the "
                         "per-kernel pass (roofline, kernels), the float32-equivalent mode, the north-star scope, the code "
                         "path, BASELINE configs 3-5 and the codec, the whole net and the CPU baseline (the --no-* options "
                         "leave some out)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write every layer's output of the last timed step (float32; a fixed "
                         "sample of a large one) to DIR/layer<i>_y.npy")
    ap.add_argument("--net", default="mobilenetv1_imagenet224")
    ap.add_argument("--batch", type=int, default=256, help="images per GPU per step (weak scaling)")
    ap.add_argument("--global-batch", type=int, default=0,
                    help="strong scaling: this many images per step in total, sharded over the ranks on the batch axis "
                         "(BASELINE config 4: --net resnet50_imagenet224 --global-batch 1024)")
    ap.add_argument("--passes", type=int, default=0, choices=[0, 1, 3], help="pointwise MFMA precision (0 = library default)")
    ap.add_argument("--qbits", type=int, default=8, choices=[8, 7], help="8 = SLFP<3,4> (headline), 7 = SFP<3,3> (BASELINE config 5)")
    ap.add_argument("--post", action="store_true", help="run every layer with the fused BN+ReLU epilogue (secondary measurement)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-whole-net", action="store_true", help="with --full: skip the whole-net measurements")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="with --full: skip the short runs of BASELINE configs 3-5 and the codec")
    ap.add_argument("--cpu-sample-batch", type=int, default=16)
    ap.add_argument("--per-layer", action="store_true", help="also run the per-kernel pass and print a per-layer table to stderr")
    ap.add_argument("--image-groups", type=int, default=2,
                    help="run a step's batch as this many independent image groups on as many HIP streams (1 = one stream)")
    args = ap.parse_args()

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("--gpus N > 1 must be launched with torch.distributed.run (one rank per GPU)")
    L = _lib.load()  # raises if the HIP extension is missing: no fallback
    assert torch.cuda.is_available(), "bench.py needs an MI355X"
    # rehearsal knobs (1-GPU box): SLFP_BENCH_SHARE_GPU=1 puts every rank on cuda:0 and SLFP_BENCH_BACKEND=gloo
    # replaces RCCL (which refuses two ranks on one device), so the N > 1 control flow can be exercised
    share = os.environ.get("SLFP_BENCH_SHARE_GPU") == "1"
    backend = os.environ.get("SLFP_BENCH_BACKEND", "nccl")
    dev_index = 0 if share else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)  # RCCL over xGMI
        else:
            dist.init_process_group(backend)

    lo, hi, strong = sharding.per_rank_batch(args.batch, args.global_batch, rank, world)   # this rank's slice of the batch
    batch = hi - lo
    if strong and batch * world != args.global_batch:
        raise SystemExit("--global-batch must divide evenly over the ranks (the bench reports one per-rank batch)")

    dump = {} if args.dump_outputs and rank == 0 else None
    res, rank_dts = run_config(L, args.net, batch, args.qbits, args.passes, args.steps, args.warmup, dev, rank, world,
                               post=args.post, per_layer=args.per_layer, exact_too=True, image_groups=args.image_groups,
                               full=args.full, dump=dump)
    if dump is not None:
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, a in dump.items():
            np.save(os.path.join(args.dump_outputs, name + ".npy"), a)

    if rank == 0:
        out = {
            "metric": "images/sec at batch 256, MobileNetV1 SLFP<3,4> ImageNet-224; % HBM roofline",
            "value": res["value"], "unit": "images/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": res["ms_per_step"], "higher_is_better": True, "scaling": "strong" if strong else "weak",
            "vs_baseline": None, "dtype": "f32 (1x1 contraction: fp16 MFMA operands, f32 accumulate)", "data": "synthetic",
            "config": {"workload": f"{args.net}: all {res['n_layers']} Conv2d_Q layers, "
                                   f"{'SLFP<3,4> Qbits=8' if args.qbits == 8 else 'SFP<3,3> Qbits=7'}, NHWC, "
                                   f"batch {batch} per GPU"
                                   + (f" as {res['image_groups']} concurrent image groups of {batch // res['image_groups']} on "
                                      f"{res['image_groups']} HIP streams" if res.get("image_groups", 1) > 1 else "")
                                   + ", inputs resident in HBM",
                       "batch_per_gpu": batch, "global_batch": batch * world,
                       "parallelism": f"batch-sharded x{world}, one-time RCCL broadcast of the u8 weight codes",
                       "pointwise_mfma": res["pointwise_mfma"]},
            "hbm_roofline_frac_whole_path": res["hbm_roofline_frac_whole_path"],
            "algorithmic_bytes_per_image": res["algorithmic_bytes_per_image"],
            "rank_ms_per_step": [round(d / args.steps * 1e3, 4) for d in rank_dts],
        }
        if "roofline" in res:   # the per-kernel pass (--full, --per-layer)
            out["roofline"], out["kernels"] = res["roofline"], res["kernels"]
        if "value_pointwise_f16x3_float32_equivalent" in res:
            out["value_pointwise_f16x3_float32_equivalent"] = res["value_pointwise_f16x3_float32_equivalent"]
        if "dw_pw_scope" in res:
            out["dw_pw_scope"] = res["dw_pw_scope"]
        if "single_stream" in res:
            out["single_stream"] = res["single_stream"]   # the same steps as 27 whole-batch launches on one stream
        if "image_groups" in res:
            out["image_groups"] = res["image_groups"]
    if args.full and world == 1 and rank == 0:
        if not args.no_other_configs:
            # BASELINE configs 3-5 at their named batch sizes: short runs (3 steps), each with its own roofline object
            other = {}
            for net, b, q in OTHER_CONFIGS:
                try:
                    r, _ = run_config(L, net, b, q, 0, 3, 1, dev, 0, 1, image_groups=args.image_groups)
                    other[net] = {"batch": b, "qbits": q, "value": r["value"], "unit": "images/sec", "ms_per_step": r["ms_per_step"],
                                  "image_groups": r.get("image_groups", 1), "single_stream": r.get("single_stream"),
                                  "hbm_roofline_frac_whole_path": r["hbm_roofline_frac_whole_path"], "roofline": r["roofline"],
                                  "kernels": r["kernels"]}
                    if net == "vgg16_224":   # the conv -> conv hand-overs inside VGG-16's stages as 1-byte codes (dense kernels)
                        cp = run_codes_config(L, net, b, q, 3, 1, dev)
                        if cp:
                            other[net]["codes_path"] = {k: cp[k] for k in ("value", "unit", "ms_per_step", "image_groups", "single_stream",
                                                                           "algorithmic_bytes_per_image", "kernels")}
                except Exception as e:  # a secondary measurement must not take the headline line down
                    other[net] = {"batch": b, "qbits": q, "error": str(e)[:200]}
            out["other_configs"] = other
            out["codec"] = codec_bench(L, dev)
        if args.net in ("mobilenetv1_imagenet224", "vgg16_224") and args.passes in (0, 1) and not args.post:
            try:   # secondary measurement: the same layers chained through 1-byte codes
                # (one stream: the code kernels' persistent grids already fill the device; two image groups measured 180 k vs 206 k)
                cp = run_codes_config(L, args.net, batch, args.qbits, args.steps, args.warmup, dev)
                if cp:
                    out["codes_path"] = cp
            except Exception as e:
                out["codes_path"] = {"error": str(e)[:200]}
        if not args.no_whole_net:
            wn = whole_net(layer_specs.conv_layers(args.net), args.net, batch, dev, max(3, args.steps // 2))
            if wn:
                out["whole_net"] = wn
        if not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(layer_specs.conv_layers(args.net), args.cpu_sample_batch, 1)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
