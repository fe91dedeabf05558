"""Cases of tests/test_gpu_dw_rows.py, and the worker that runs them in a process of its own.

The depthwise kernel is chosen by a switch the library reads once, when it is loaded (SLFP_DW_ROWS, csrc/slfp_host.hpp).  The
test compares the register-window kernel (csrc/conv_dw3.hip) with the tile kernel (csrc/conv_dw2.hip) on the same seeded
inputs, so the tile kernel's outputs come from a fresh process started with SLFP_DW_ROWS=0:

    SLFP_DW_ROWS=0 python tests/_dw_rows_worker.py OUTDIR tile

runs every case, checks that the library reports the expected kernel for it, and writes OUTDIR/<case id>.npy."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from cnns_slfp_quantization_amd import _lib  # noqa: E402

KA, KW = 2.6023073196411133 / 15.5, 1.9635683298110962 / 15.5

# every stride-2 depthwise geometry of MobileNetV1 (nets_imgnet/mobilenetv1.py:43-57): (C, H = W), pad 1
NET_GEOMS = [(64, 112), (128, 56), (256, 28), (512, 14)]
# (tag, N, C, H, W, pad, post, specials)
NET_CASES = [(f"net_c{c}_h{h}_n{n}_{'post' if post else 'plain'}", n, c, h, h, 1, post, None)
             for (c, h) in NET_GEOMS for n in (128, 256) for post in (False, True)]
# shapes the net does not have but the dispatch admits: ragged tiles, pad 0 / 1 / 2, C = 32 / 96, N = 1 / 3, images smaller
# than one wave's tasks; each with clean inputs and with NaN, +-inf, +-0 and values on and beyond both clamps
ODD_GEOMS = [(1, 32, 57, 30, 1), (3, 96, 15, 57, 0), (3, 32, 30, 15, 1), (1, 96, 57, 57, 0), (3, 32, 3, 3, 1), (5, 32, 5, 4, 0),
             (2, 64, 20, 9, 2)]
ODD_CASES = [(f"odd_n{n}_c{c}_h{h}_w{w}_p{p}_{'post' if post else 'plain'}_{sp}", n, c, h, w, p, post, sp)
             for (n, c, h, w, p) in ODD_GEOMS for post in (False, True) for sp in ("finite", "nonfinite")]
CASES = NET_CASES + ODD_CASES


def specials(kind):
    """Values written over seeded positions of the input: both zeros, the clamps of QA(x / Ka) (2^-5 and 15.5 in units of
    Ka) from both sides and far beyond, and -- `nonfinite` -- NaN and both infinities."""
    v = [0.0, -0.0, KA * 2.0 ** -5, -KA * 2.0 ** -5, KA * 2.0 ** -6, KA * 2.0 ** -4.9, KA * 15.5, -KA * 15.5, KA * 15.4, KA * 16.0,
         KA * 1e4, -KA * 1e4, KA * 1e-9, -KA * 1e-30]
    if kind == "nonfinite":
        v += [float("nan"), float("inf"), float("-inf"), -float("nan")]
    return v


class Case:
    def __init__(self, case, dev):
        self.tag, n, c, h, w, pad, self.post, sp = case
        L = _lib.load()
        self.d = _lib.ConvDesc(n=n, c_in=c, h=h, w=w, c_out=c, kh=3, kw=3, stride_h=2, stride_w=2, pad_h=pad, pad_w=pad,
                               dil_h=1, dil_w=1, groups=c, x_layout=_lib.LAYOUT_NHWC, y_layout=_lib.LAYOUT_NHWC, qbits=8,
                               ka=float(np.float32(KA)), kw_scale=float(np.float32(KW)), mfma_passes=0, reserved=0)
        seed = ((((n * 1009 + c) * 1009 + h) * 1009 + w) * 7 + pad) * 3 + (0 if sp is None else 1 + (sp == "nonfinite"))   # plain / post share inputs
        gen = torch.Generator(device=dev).manual_seed(seed)
        x = torch.randn((n, h, w, c), generator=gen, device=dev)
        self.x = (x.abs_() if sp is None else x).mul_(4.0 * KA)   # net cases: post-ReLU-like, as bench.py; odd cases: signed
        self.w = torch.randn((c, 1, 3, 3), generator=gen, device=dev) * (5.0 * KW)
        self.scale = torch.rand(c, generator=gen, device=dev) + 0.5
        self.shift = torch.randn(c, generator=gen, device=dev) * 0.3
        if sp is not None:
            vals = torch.tensor(specials(sp), dtype=torch.float32, device=dev)
            k = min(self.x.numel(), 4 * len(vals) + 3)
            pos = torch.randperm(self.x.numel(), generator=gen, device=dev)[:k]
            self.x.view(-1)[pos] = vals[torch.arange(k, device=dev) % len(vals)]
        ho, wo = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(L.slfp_conv2d_out_shape(ctypes.byref(self.d), ctypes.byref(ho), ctypes.byref(wo)))
        self.out_shape = (n, ho.value, wo.value, c)
        self.blob = torch.empty(L.slfp_conv2d_wprep_bytes(ctypes.byref(self.d)), dtype=torch.uint8, device=dev)
        _lib.check(L.slfp_conv2d_prepare_weights(ctypes.byref(self.d), self.w.data_ptr(), self.blob.data_ptr(), None, _stream()))

    def variant(self):
        return _lib.load().slfp_debug_dw3x3_variant(ctypes.byref(self.d), 1 if self.post else 0).decode()

    def run(self):
        """slfp_conv2d_fwd, or slfp_conv2d_fwd_post with the scale / shift vectors and the ReLU"""
        L = _lib.load()
        y = torch.full(self.out_shape, float("nan"), device=self.x.device)   # an element the kernel skips stays NaN
        if self.post:
            _lib.check(L.slfp_conv2d_fwd_post(ctypes.byref(self.d), self.x.data_ptr(), self.blob.data_ptr(), None, self.scale.data_ptr(),
                                              self.shift.data_ptr(), 1, y.data_ptr(), None, None, _stream()))
        else:
            _lib.check(L.slfp_conv2d_fwd(ctypes.byref(self.d), self.x.data_ptr(), self.blob.data_ptr(), None, y.data_ptr(), None, None,
                                         _stream()))
        torch.cuda.synchronize()
        return y


def _stream():
    return torch.cuda.current_stream().cuda_stream


def main():
    outdir, expect = sys.argv[1], sys.argv[2]
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    for case in CASES:
        c = Case(case, dev)
        assert c.variant() == expect, (c.tag, c.variant(), expect)
        np.save(os.path.join(outdir, c.tag + ".npy"), c.run().cpu().numpy())
        del c
    print("dw rows worker ok", flush=True)


if __name__ == "__main__":
    main()
