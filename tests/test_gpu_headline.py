"""GPU (MI355X): the launches bench.py times, checked at the size it times them; and the product's grouped entry point.

bench.py's headline step runs the 27 Conv2d_Q layers of MobileNetV1-224 through `bench.Layer`: NHWC in and out, each layer's
own calibrated Ka / Kw, inputs |randn| * 4 Ka (the stem's signed), as two image groups of 128 on two HIP streams sharing one
prepared weight blob per layer; `--full` adds whole-batch launches of 256 and the float32-equivalent mode (mfma_passes = 3,
switched with `Layer.set_passes`).  Every layer here is a `bench.Layer`, so the launches under test are the timed ones:
  * each layer at N = 128 and N = 256, both modes: sampled images (the group boundary included) against the CPU oracle;
  * batch-size invariance: the N = 256 output equals N = 128 launches on its halves and N = 1 launches, bit for bit (the
    path has no split-K and no atomics, so an image's outputs cannot depend on the other images);
  * run_config's grouped step (two streams, shared blobs, interleaved launches, no synchronisation) equals the
    single-stream launches on the same inputs, bit for bit.
Then streams.forward_image_groups on a model whose prepared-weight caches are cold or just invalidated, its arguments, and
the `input_q` stash after a grouped forward.
"""
import itertools

import pytest
import torch
import torch.nn as nn

import bench
from _bars import ELEM_MIN, elem_frac_bar, tol
from cnns_slfp_quantization_amd import _lib, fusion, layer_specs, streams
from cnns_slfp_quantization_amd import optimizer as O
from cnns_slfp_quantization_amd.conv2d_func import conv2d_Q, linear_Q
from conftest import elem_exceed_frac, note_elem_stats, rel_errors
from oracle import slfp_oracle as so

pytestmark = pytest.mark.gpu

SPECS = layer_specs.conv_layers("mobilenetv1_imagenet224")
MODES = (_lib.MFMA_DEFAULT, _lib.MFMA_F16X3)   # the headline's mode and --full's float32-equivalent one
IDS = [f"{i:02d}-{s.c_in}x{s.c_out}k{s.k[0]}s{s.stride[0]}@{s.h}" for i, s in enumerate(SPECS)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L():
    lib = _lib.load()   # raises if libslfp_hip.so is missing: no fallback
    assert lib.slfp_device_count() >= 1
    return lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _family(s, passes):
    """The kernel family the launch of layer `s` must reach (conv_abi.hip make_plan_core)."""
    if s.c_in == 3:
        return "stem_nhwc"   # the 3x3 s2 3->32 stem keeps its exact fp32 kernel in both modes
    if s.groups > 1:
        return "dw3x3_nhwc"
    return "pw_mfma_f16x3" if passes == _lib.MFMA_F16X3 else "pw_mfma_f16x1"


def _layer(L, i, batch, dev, seed):
    """Layer i at `batch` images in the headline mode, built and prepared as run_config does (a generator of its own, so a
    failing case reruns alone)."""
    gen = torch.Generator(device=dev).manual_seed(seed + 1000 * i + batch)
    layer = bench.Layer(L, SPECS[i], batch, dev, MODES[0], gen)
    layer.prepare(L, _stream())
    return layer


def _part(L, big, lo, hi, dev):
    """A launch of `big`'s layer on images lo:hi: a bench.Layer of hi - lo images given the whole-batch layer's input
    slice, weights and prepared blob (one blob shared across batch sizes, as run_config's image groups share it)."""
    part = bench.Layer(L, big.spec, hi - lo, dev, big.desc.mfma_passes, torch.Generator(device=dev).manual_seed(0))
    part.x, part.w, part.bias, part.blob = big.x[lo:hi], big.w, big.bias, big.blob
    part.y.fill_(float("nan"))
    return part


def _run(L, layer):
    layer.y.fill_(float("nan"))   # an output the kernel leaves unwritten cannot pass as a stale result
    layer.run(L, _stream())


# ------------------------------------------------------------------ 1. every layer at N = 128 and 256 against the oracle
@pytest.mark.parametrize("i", range(len(SPECS)), ids=IDS)
def test_headline_layer_vs_oracle_at_size(L, dev, i):
    s = SPECS[i]
    for batch in (128, 256):
        layer = _layer(L, i, batch, dev, seed=11)
        idx = [0, 1, 64, batch - 1] + ([127, 128] if batch == 256 else [])   # 127 | 128: the image-group boundary
        xs = layer.x[idx].permute(0, 3, 1, 2).contiguous().cpu().numpy()
        ref = so.conv2d(xs, layer.w.cpu().numpy(), None if layer.bias is None else layer.bias.cpu().numpy(), s.stride, s.pad,
                        1, s.groups, layer.desc.ka, layer.desc.kw_scale, 8)
        for passes in MODES:
            layer.set_passes(L, _stream(), passes)   # what --full does between the two modes: same buffers
            kern = layer.kernel
            assert kern == _family(s, passes), (i, batch, passes, kern)
            _run(L, layer)
            got = layer.y[idx].permute(0, 3, 1, 2).contiguous().cpu().numpy()
            emax, el2 = rel_errors(got, ref)
            frac = elem_exceed_frac(got, ref)
            note_elem_stats(kern, got, ref)
            print(f"layer {i:2d} N={batch} {kern}: emax {emax:.2e} el2 {el2:.2e} frac {frac:.4f}")
            assert emax <= tol(kern) and el2 <= tol(kern), (i, batch, kern, emax, el2)
            if got.size >= ELEM_MIN:
                assert frac <= elem_frac_bar(kern), (i, batch, kern, frac)
        del layer, xs, ref


# ------------------------------------------------------------------ 2. batch-size invariance, every image
@pytest.mark.parametrize("i", range(len(SPECS)), ids=IDS)
def test_headline_layer_is_batch_size_invariant(L, dev, i):
    big = _layer(L, i, 256, dev, seed=22)
    for passes in MODES:
        big.set_passes(L, _stream(), passes)
        _run(L, big)
        for lo, hi in ((0, 128), (128, 256), (77, 78), (255, 256)):
            part = _part(L, big, lo, hi, dev)
            part.run(L, _stream())
            same = torch.equal(part.y, big.y[lo:hi])
            assert same, (i, big.kernel, (lo, hi), int((part.y != big.y[lo:hi]).sum()))
            del part


# ------------------------------------------------------------------ 3. two image groups on two streams, as timed
@pytest.mark.parametrize("passes", MODES, ids=["f16x1", "f16x3"])
def test_two_image_groups_as_timed_equal_single_stream_launches(L, dev, passes):
    """run_config's grouped step: two groups of 128, each layer's blob prepared once (for the whole-batch descriptor) and
    shared, separate inputs, outputs and workspaces, the groups' launches interleaved layer by layer on two streams with no
    synchronisation until the end; three steps back to back, as the timed loop runs them."""
    gen = torch.Generator(device=dev).manual_seed(1234)
    groups = [[], []]
    for s in SPECS:
        whole = bench.Layer(L, s, 256, dev, passes, gen)
        whole.prepare(L, _stream())
        for gl in groups:
            gl.append(bench.Layer(L, s, 128, dev, passes, gen))
            gl[-1].blob = whole.blob
        del whole
    refs = []
    for gl in groups:
        refs.append([])
        for layer in gl:
            _run(L, layer)
            refs[-1].append(layer.y.clone())
            layer.y.fill_(float("nan"))
    pair = [torch.cuda.Stream(device=dev) for _ in groups]
    for st in pair:
        st.wait_stream(torch.cuda.current_stream())
    handles = [st.cuda_stream for st in pair]
    for _ in range(3):
        for i in range(len(SPECS)):
            for h, gl in zip(handles, groups):
                gl[i].run(L, h)
    torch.cuda.synchronize()
    for g, gl in enumerate(groups):
        for i, layer in enumerate(gl):
            assert torch.equal(layer.y, refs[g][i]), (g, i, layer.kernel, int((layer.y != refs[g][i]).sum()))


# ------------------------------------------------------------------ streams.forward_image_groups
def _cifar_net(seed):
    """MobileNetV1-CIFAR from its layer table with a Linear_Q classifier (as test_gpu_backward builds it)."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        layers = []
        for s in layer_specs.conv_layers("mobilenetv1_cifar32"):
            layers += [conv2d_Q(8, s.Kw, s.Ka)(s.c_in, s.c_out, s.k, stride=s.stride, padding=s.pad, groups=s.groups),
                       nn.BatchNorm2d(s.c_out), nn.ReLU()]
        fc = [r for r in layer_specs.nets()["mobilenetv1_cifar32"]["layers"] if r["kind"] == "linear"][0]
        layers += [nn.AdaptiveAvgPool2d(1), nn.Flatten(), linear_Q(8, fc["Kw"], fc["Ka"])(fc["c_in"], fc["c_out"])]
        net = nn.Sequential(*layers)
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_var.uniform_(0.5, 1.5)
                m.weight.data.uniform_(0.8, 1.6)
                m.bias.data.normal_(0.1, 0.1)
    return net


def _fresh_pair(dev):
    """Two identical BN-fused nets in eval mode that have never run: every prepared-weight cache is cold."""
    nets = []
    for _ in range(2):
        net = _cifar_net(5).to(dev).eval().to(memory_format=torch.channels_last)
        assert fusion.fuse_bn_relu(net) == len(layer_specs.conv_layers("mobilenetv1_cifar32"))
        nets.append(net)
    x = torch.randn((16, 3, 32, 32), generator=torch.Generator(device=dev).manual_seed(6), device=dev)
    return nets[0], nets[1], x.contiguous(memory_format=torch.channels_last)


def _sleep_cycles(ms):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(1_000_000)
    b.record()
    b.synchronize()
    return int(min(1_000_000 / max(a.elapsed_time(b), 1e-3), 5e6) * ms)


def _concurrent_streams(dev, cycles):
    """Two streams on which work runs side by side (HIP puts streams on a few hardware queues, and two streams that share
    one serialise, which would hide the race these tests provoke): the first pair of four where a sleep on one does not
    hold up the other."""
    cand = [torch.cuda.Stream(device=dev) for _ in range(4)]
    for a, b in itertools.combinations(cand, 2):
        with torch.cuda.stream(a):
            torch.cuda._sleep(cycles)
        a_done, b_done = torch.cuda.Event(), torch.cuda.Event()
        a_done.record(a)
        b_done.record(b)
        b_done.synchronize()
        overlap = not a_done.query()
        torch.cuda.synchronize()
        if overlap:
            return [a, b]
    pytest.fail("no two of four streams run concurrently")


def _grouped_with_group0_late(net, x, pair, cycles):
    """forward_image_groups with group 0's stream held up by a sleep: group 0 misses the caches and prepares the blobs on its
    stream behind the sleep, group 1 takes the cache hits and launches on its own stream while those blobs are unwritten."""
    with torch.cuda.stream(pair[0]):
        torch.cuda._sleep(cycles)
    y = streams.forward_image_groups(net, x, groups=2, streams=pair)
    torch.cuda.synchronize()
    return y


def test_grouped_forward_on_cold_and_invalidated_weight_caches(dev):
    """A prepared blob (weight values only: no offsets or indices) read before its prepare has landed gives wrong numbers;
    the cache makes a hit from another stream wait for the prepare.  Cold caches (a net that never ran), then caches
    invalidated by a DSGD step (new weight versions): both equal one ordinary forward of an identical net, bit for bit."""
    a, b, x = _fresh_pair(dev)
    cycles = _sleep_cycles(50)
    pair = _concurrent_streams(dev, cycles)
    with torch.no_grad():
        want = b(x)
        got = _grouped_with_group0_late(a, x, pair, cycles)
        assert torch.equal(got, want), int((got != want).sum())
        g = torch.Generator(device=dev).manual_seed(7)
        grads = [torch.randn(p.shape, generator=g, device=dev) * 1e-2 for p in a.parameters()]
        for net in (a, b):
            for p, gr in zip(net.parameters(), grads):
                p.grad = gr.clone()
            O.DSGD(net.parameters(), 8, lr=0.5, momentum=0.9).step()
        assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
        want = b(x)
        got = _grouped_with_group0_late(a, x, pair, cycles)
        assert torch.equal(got, want), int((got != want).sum())


class _ReadsStash(nn.Module):
    """Reads layers' input_q at the end of its own forward, as the reference's CIFAR nets do (nets_cifar/mobilenetv1.py:88)."""

    def __init__(self, net, taps):
        super().__init__()
        self.net = net
        self.taps = taps
        self.seen = []

    def forward(self, x):
        y = self.net(x)
        self.seen.append([self.net[t].input_q.clone() for t in self.taps])
        return y


def test_grouped_forward_arguments_and_input_q_stash(dev):
    a, _, x = _fresh_pair(dev)
    convs = [i for i, m in enumerate(a) if isinstance(m, nn.Conv2d)]
    taps = [convs[0], convs[5], len(a) - 1]   # the stem, a depthwise layer and the Linear_Q classifier
    net = _ReadsStash(a, taps)
    pair = [torch.cuda.Stream(device=dev) for _ in range(3)]
    with torch.no_grad():
        want = net(x)
        stash = net.seen.pop()
        assert a[convs[0]]._prep.synced == set()   # hits on the stream that prepared the blob add no event work
        with pytest.raises(ValueError, match="3 streams"):
            streams.forward_image_groups(net, x, groups=3, streams=pair[:2])
        got = streams.forward_image_groups(net, x, groups=2, streams=pair)   # a stream more than needed goes unused
        torch.cuda.synchronize()
        assert torch.equal(got, want)
        # inside each group's forward the stash is that group's slice
        assert len(net.seen) == 2
        for t in range(len(taps)):
            assert torch.equal(torch.cat([net.seen[0][t], net.seen[1][t]]), stash[t]), taps[t]
        for t in taps:
            with pytest.raises(RuntimeError, match="forward_image_groups"):
                a[t].input_q
        net.seen.clear()
        assert torch.equal(net(x), want)
        for t, ref in zip(taps, stash):
            assert torch.equal(a[t].input_q, ref)
