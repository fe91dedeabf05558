"""GPU (MI355X): every instance of the two one-kernel depthwise -> pointwise block kernels (csrc/conv_dwpw.hip: k_dwpw<S, KS, NT>;
csrc/conv_dwpw_codes.hip: k_dwpw_codes<S, KS, NT, FMT, YC>) at the small ragged shapes of tests/_dwpw_variants.py, straight through the
C ABI.  The feature tests reach five of the eighteen (S, KS, NT) of each kernel, at whole-layer shapes and against the device's own
two-kernel sequence only.  Here each row names its instance (slfp_debug_dwpw_instance says which one runs) and is held

  1. to the specification, BIT FOR BIT: include/slfp.h defines the one-kernel forms as the two launches -- slfp_conv2d_fwd_post(dw) then
     slfp_conv2d_fwd_post(pw) on the float32 interface, slfp_conv2d_fwd_codes_ws(dw -> codes for Ka_pw) then
     slfp_conv2d_fwd_codes_ws(pw) on codes.  float32 is compared as int32, codes as bytes.  On the special-value rows NaN positions must
     agree, everything else bit for bit, and the NaN must reach the output (float32 input) or be patched to the fp16 zero exactly as
     k_dwc's code 0x00 is (a NaN in post1_shift);
  2. to a CPU reference with no device in it (float32 and codes -> float32 rows without special values): the depthwise stage by the
     bit-exact restatement oracle/slfp_oracle.c: slfp_oracle_dw3x3_f32 -- the device's depthwise-alone output must equal it bit for bit,
     so no quantizer flip separates the two sides -- then the pointwise contraction in double (slfp_oracle_conv2d), post2 and the ReLU
     in float64, under the pointwise family's bars of tests/_bars.py.  No tolerance of this file's own;
  3. code output to the oracle's encoder applied to the same row's one-kernel float32 output (ReLU folded, or signed codes);
  4. to memory discipline: the output ends at the last byte of a dedicated allocation in the first launch and lies between two 64-byte
     0xA5 guards in the second; the guards stay, the two launches give the same bytes.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

from _bars import ELEM_MIN, elem_frac_bar, tol as _tol
from _dwpw_variants import (KA_DW, KA_NEXT, KA_PW, KW_DW, KW_PW, NAN_CHANNEL, ROWS, geom_key, instance, make_descs, make_input,
                            make_io, make_params, out_hw, reader_qbits)
from conftest import elem_exceed_frac, rel_errors, same_bits
from oracle import slfp_oracle as so

pytestmark = pytest.mark.gpu

GUARD = 64
RAN = set()      # reporter strings of the one-kernel launches this file made
WORST = {}       # q_bit -> [max-rel, l2, fraction]: the largest CPU-reference errors seen (printed by the closing test)
_INPUTS = {}     # geom_key -> _Input
_PARAMS = {}     # (C, N) -> _Params
_BLOBS = {}      # (C, N, stride, pad, h, w, batch, qbits) -> (dw blob, pw blob)
_REFS = {}       # the CPU reference of a computation, shared by the float32 and the codes row of the same block
_MIDS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from cnns_slfp_quantization_amd import _lib
    L = _lib.load()  # raises if libslfp_hip.so is missing: no fallback
    assert L.slfp_device_count() >= 1
    return _lib


@pytest.fixture(scope="module")
def arena(dev):
    """A device allocation of its own (32 MiB: a whole number of 2 MiB pages that the caching allocator hands to the device as it
    is, once its free blocks are released): outputs are placed at its very end, so nothing lies behind their last byte."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return torch.empty(32 << 20, dtype=torch.uint8, device=dev)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _fmt(qbits):
    return (so.FMT_ACT8 if qbits == 8 else so.FMT_SFP7) | so.FMT_EXT


def _ptr(t):
    return t.data_ptr() if t is not None else None


class _Input:
    """The input of a geometry key on the host and the device: float32 (clean, and with the special values planted) and the codes of
    QA(x / Ka_dw) in both formats, by the oracle's encoder.  Built once, never written again."""

    def __init__(self, row, dev):
        self.x_np, self.xs_np = make_input(row)
        self.x, self.xs = torch.from_numpy(self.x_np).to(dev), torch.from_numpy(self.xs_np).to(dev)
        self.codes_np = {q: so.encode(self.x_np, np.float32(KA_DW), _fmt(q)) for q in (8, 7)}
        self.codes = {q: torch.from_numpy(c).to(dev) for q, c in self.codes_np.items()}


class _Params:
    def __init__(self, c, n_out, dev):
        self.np = make_params(c, n_out)
        for k, v in self.np.items():
            setattr(self, k, torch.from_numpy(v).to(dev))
        self.sh1_nan_np = self.np["sh1"].copy()
        self.sh1_nan_np[NAN_CHANNEL] = float("nan")
        self.sh1_nan = torch.from_numpy(self.sh1_nan_np).to(dev)


def _input(row, dev):
    k = geom_key(row)
    if k not in _INPUTS:
        _INPUTS[k] = _Input(row, dev)
    return _INPUTS[k]


def _params(row, dev):
    k = (row.c, row.n_out)
    if k not in _PARAMS:
        _PARAMS[k] = _Params(row.c, row.n_out, dev)
    return _PARAMS[k]


def _blobs(lib, row, dw, pw, P, dev):
    k = (row.c, row.n_out, row.stride, row.pad, row.h, row.w, row.batch, row.qbits)
    if k not in _BLOBS:
        L = lib.load()
        out = []
        for d, w in ((dw, P.w_dw), (pw, P.w_pw)):
            blob = torch.empty(L.slfp_conv2d_wprep_bytes(ctypes.byref(d)), dtype=torch.uint8, device=dev)
            lib.check(L.slfp_conv2d_prepare_weights(ctypes.byref(d), w.data_ptr(), blob.data_ptr(), None, _stream()))
            out.append(blob)
        _BLOBS[k] = tuple(out)
    return _BLOBS[k]


class _Call:
    """One row's operands on the device, and its launches."""

    def __init__(self, lib, row, dev):
        self.lib, self.row, self.dev = lib, row, dev
        self.P = _params(row, dev)
        self.X = _input(row, dev)
        self.dw, self.pw = make_descs(lib, row)
        self.blob1, self.blob2 = _blobs(lib, row, self.dw, self.pw, self.P, dev)
        self.sh1 = self.P.sh1_nan if row.special == "shift_nan" else self.P.sh1
        self.bias = self.P.bias2 if row.bias else None
        self.sc2, self.sh2 = (self.P.sc2, self.P.sh2) if row.post2 else (None, None)
        if row.iface == "f32":
            self.x = self.X.xs if row.special == "values" else self.X.x
        else:
            self.x = self.X.codes[row.qbits]
        self.shape = (row.batch,) + out_hw(row) + (row.n_out,)

    def one_kernel(self, y_ptr, io="row"):
        """slfp_dwpw_fwd / slfp_dwpw_fwd_codes into y_ptr; io: the row's, or another slfp_conv2d_io of the code interface"""
        lib, L, r = self.lib, self.lib.load(), self.row
        d1, d2 = ctypes.byref(self.dw), ctypes.byref(self.pw)
        if io == "row":
            io = make_io(lib, r)
        name = instance(lib, r, self.dw, self.pw, io)
        assert name != "none", r
        if io is None:
            assert L.slfp_dwpw_supported(d1, d2) == 1, r
            rc = L.slfp_dwpw_fwd(d1, d2, self.x.data_ptr(), self.blob1.data_ptr(), self.P.sc1.data_ptr(), self.sh1.data_ptr(), r.relu1,
                                 self.blob2.data_ptr(), _ptr(self.bias), _ptr(self.sc2), _ptr(self.sh2), r.relu2, y_ptr, _stream())
        else:
            assert L.slfp_dwpw_codes_supported(d1, d2, ctypes.byref(io), int(r.bias), r.relu1, r.relu2) == 1, r
            rc = L.slfp_dwpw_fwd_codes(d1, d2, ctypes.byref(io), self.x.data_ptr(), self.blob1.data_ptr(), self.P.sc1.data_ptr(),
                                       self.sh1.data_ptr(), r.relu1, self.blob2.data_ptr(), _ptr(self.bias), _ptr(self.sc2), _ptr(self.sh2),
                                       r.relu2, y_ptr, _stream())
        assert rc == lib.OK, (r, rc, lib.last_error())
        RAN.add(name)
        return name

    def _mid(self, dtype):
        ho, wo = out_hw(self.row)
        return torch.empty((self.row.batch, ho, wo, self.row.c), dtype=dtype, device=self.dev)

    def _y(self, codes):
        return torch.empty(self.shape, dtype=torch.uint8 if codes else torch.float32, device=self.dev)

    def depthwise_alone_f32(self):
        """the depthwise layer by itself, float32 out: slfp_conv2d_fwd_post, or slfp_conv2d_fwd_codes_ws on the codes"""
        lib, L, r = self.lib, self.lib.load(), self.row
        mid = self._mid(torch.float32)
        if r.iface == "f32":
            lib.check(L.slfp_conv2d_fwd_post(ctypes.byref(self.dw), self.x.data_ptr(), self.blob1.data_ptr(), None, self.P.sc1.data_ptr(),
                                             self.sh1.data_ptr(), r.relu1, mid.data_ptr(), None, None, _stream()))
        else:
            io = lib.ConvIo(x_codes=1, y_codes=0, y_ka=1.0, y_qbits=8)
            assert L.slfp_conv2d_codes_supported(ctypes.byref(self.dw), ctypes.byref(io), 0, r.relu1) == 1
            lib.check(L.slfp_conv2d_fwd_codes_ws(ctypes.byref(self.dw), ctypes.byref(io), self.x.data_ptr(), self.blob1.data_ptr(), None,
                                                 self.P.sc1.data_ptr(), self.sh1.data_ptr(), r.relu1, mid.data_ptr(), None, _stream()))
        return mid

    def two_kernels(self):
        """The specification: the two layers one after the other.  Returns (intermediate: float32 or codes for Ka_pw, y)."""
        lib, L, r = self.lib, self.lib.load(), self.row
        d1, d2 = ctypes.byref(self.dw), ctypes.byref(self.pw)
        if r.iface == "f32":
            mid = self.depthwise_alone_f32()
            y = self._y(False)
            nws = L.slfp_conv2d_workspace_bytes(d2)
            ws = torch.empty(nws, dtype=torch.uint8, device=self.dev) if nws else None
            lib.check(L.slfp_conv2d_fwd_post(d2, mid.data_ptr(), self.blob2.data_ptr(), _ptr(self.bias), _ptr(self.sc2), _ptr(self.sh2),
                                             r.relu2, y.data_ptr(), None, _ptr(ws), _stream()))
            return mid, y
        io1 = lib.ConvIo(x_codes=1, y_codes=1, y_ka=float(np.float32(KA_PW)), y_qbits=r.qbits)
        io2 = make_io(lib, r)
        assert L.slfp_conv2d_codes_supported(d1, ctypes.byref(io1), 0, r.relu1) == 1
        assert L.slfp_conv2d_codes_supported(d2, ctypes.byref(io2), int(r.bias), r.relu2) == 1
        mid = self._mid(torch.uint8)
        y = self._y(bool(io2.y_codes))
        lib.check(L.slfp_conv2d_fwd_codes_ws(d1, ctypes.byref(io1), self.x.data_ptr(), self.blob1.data_ptr(), None, self.P.sc1.data_ptr(),
                                             self.sh1.data_ptr(), r.relu1, mid.data_ptr(), None, _stream()))
        lib.check(L.slfp_conv2d_fwd_codes_ws(d2, ctypes.byref(io2), mid.data_ptr(), self.blob2.data_ptr(), _ptr(self.bias), _ptr(self.sc2),
                                             _ptr(self.sh2), r.relu2, y.data_ptr(), None, _stream()))
        return mid, y


def _cpu_reference(row, X, P):
    """(depthwise stage by the bit-exact restatement, block output in float64) -- no device in it.  The restatement quantizes a float32
    input to the values the codes decode to, so the float32 and the codes row of one block share the result."""
    km = (row.c, row.n_out, row.stride, row.pad, row.h, row.w, row.batch, row.qbits, row.relu1)   # the weights are per (C, N) pair
    if km not in _MIDS:
        _MIDS[km] = so.dw3x3_f32(X.x_np, P.np["w_dw"], None, row.stride, row.pad, KA_DW, KW_DW, row.qbits, scale=P.np["sc1"],
                                 shift=P.np["sh1"], relu=bool(row.relu1))
        on_codes = so.dw3x3_f32(X.codes_np[row.qbits], P.np["w_dw"], None, row.stride, row.pad, KA_DW, KW_DW, row.qbits, scale=P.np["sc1"],
                                shift=P.np["sh1"], relu=bool(row.relu1))
        assert same_bits(_MIDS[km], on_codes), "the restatement on the codes and on the float32 input behind them"
    mid = _MIDS[km]
    kr = km + (row.bias, row.post2, row.relu2)
    if kr not in _REFS:
        ref = so.conv2d(np.ascontiguousarray(mid.transpose(0, 3, 1, 2)), P.np["w_pw"], P.np["bias2"] if row.bias else None, 1, 0, 1, 1, KA_PW,
                        KW_PW, row.qbits).transpose(0, 2, 3, 1).astype(np.float64)
        if row.post2:
            ref = ref * P.np["sc2"].astype(np.float64) + P.np["sh2"].astype(np.float64)
        if row.relu2:
            ref = np.maximum(ref, 0.0)
        _REFS[kr] = ref
    return mid, _REFS[kr]


def _first_diff(got, want):
    bad = np.argwhere(got != want)
    at = tuple(bad[0]) if len(bad) else None
    return f"{len(bad)} of {got.size} differ; first at (image, row, column, channel) {at}: got {got[at]:#x}, want {want[at]:#x}" if at else "NaN placement"


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_dwpw_variant(lib, dev, arena, row):
    L = lib.load()
    call = _Call(lib, row, dev)
    assert instance(lib, row, call.dw, call.pw) == row.instance, row
    codes_out = reader_qbits(row) is not None
    n_el = int(np.prod(call.shape))
    nbytes = n_el * (1 if codes_out else 4)
    assert nbytes % 16 == 0 and 2 * nbytes + 4 * GUARD <= arena.numel()

    # ---- 4. the output at the very end of its allocation, then between two guards; twice the same bytes
    end = arena.numel()
    last = arena[end - nbytes - GUARD:]
    last.fill_(0xA5)
    at = end - 2 * nbytes - 4 * GUARD
    mid_buf = arena[at:at + nbytes + 2 * GUARD]
    mid_buf.fill_(0xA5)
    assert (last.data_ptr() + GUARD) % 16 == 0 and (mid_buf.data_ptr() + GUARD) % 16 == 0
    assert call.one_kernel(last.data_ptr() + GUARD) == row.instance
    call.one_kernel(mid_buf.data_ptr() + GUARD)
    torch.cuda.synchronize()
    assert bool((last[:GUARD] == 0xA5).all()), (row, "guard in front of the output written")
    assert bool((mid_buf[:GUARD] == 0xA5).all()) and bool((mid_buf[GUARD + nbytes:] == 0xA5).all()), (row, "guard band written")
    assert torch.equal(last[GUARD:], mid_buf[GUARD:GUARD + nbytes]), (row, "run to run")
    got_bytes = last[GUARD:].cpu().numpy().copy()
    got = got_bytes.reshape(call.shape) if codes_out else got_bytes.view(np.uint32).reshape(call.shape)

    # ---- 1. the specification: the two launches, bit for bit
    mid_dev, want_dev = call.two_kernels()
    torch.cuda.synchronize()
    want = want_dev.cpu().numpy()
    want = want if codes_out else want.view(np.uint32)
    if codes_out:
        assert np.array_equal(got, want), (row, _first_diff(got, want))
    else:
        assert same_bits(got, want), (row, _first_diff(got, want))
        isn = np.isnan(got.view(np.float32))
        if row.special == "values":
            assert isn.any() and not isn.all(), (row, "the planted NaN must reach the output", int(isn.sum()))
            assert np.array_equal(isn, np.isnan(want.view(np.float32)))
        else:
            assert not isn.any(), (row, "NaN in the output of clean input: a read outside the tensor, or an element never written")
    if row.special == "shift_nan":
        # the depthwise result of that channel is NaN everywhere: k_dwc writes 0x00 for it, the one-kernel form patches the operand to
        # the same fp16 zero -- no NaN may come out, and the bits above are the two-kernel sequence's
        assert bool((mid_dev[..., NAN_CHANNEL] == 0).all()) and not bool((mid_dev[..., NAN_CHANNEL + 1] == 0).all())
        assert bool(torch.isnan(call.depthwise_alone_f32()[..., NAN_CHANNEL]).all())

    # ---- 2. a CPU reference with no device in it
    if row.special is None and row.iface in ("f32", "cin"):
        mid_ref, ref = _cpu_reference(row, call.X, call.P)
        mid_got = (mid_dev if row.iface == "f32" else call.depthwise_alone_f32()).cpu().numpy()
        assert same_bits(mid_got, mid_ref), (row, "the device's depthwise stage against the restatement",
                                             _first_diff(mid_got.view(np.uint32), mid_ref.view(np.uint32)))
        if row.iface == "cin":   # ... and the codes the two-kernel sequence hands over are the oracle's of that float32
            assert np.array_equal(mid_dev.cpu().numpy(), so.encode(mid_ref, np.float32(KA_PW), _fmt(row.qbits))), row
        kern = L.slfp_conv2d_kernel_name(ctypes.byref(call.pw)).decode()
        assert kern.startswith("pw_mfma_f16"), kern
        yf = got.view(np.float32)
        emax, el2 = rel_errors(yf, ref)
        big = n_el >= ELEM_MIN
        frac = elem_exceed_frac(yf, ref) if big else float("nan")
        print(f"{row.name}: {row.instance} [{kern}] max-rel {emax:.3e} l2 {el2:.3e} " +
              (f"elementwise fraction {frac:.4f}" if big else f"elementwise fraction skipped ({n_el} < {ELEM_MIN} elements)"))
        w = WORST.setdefault(row.qbits, [0.0, 0.0, 0.0])
        w[0], w[1], w[2] = max(w[0], emax), max(w[1], el2), max(w[2], frac if big else 0.0)
        assert emax <= _tol(kern) and el2 <= _tol(kern), (row, kern, emax, el2)
        if big:
            assert frac <= elem_frac_bar(kern), (row, kern, frac)

    # ---- 3. code output: the oracle's encoder on the same row's one-kernel float32 output
    if codes_out:
        y32_dev = torch.empty(call.shape, dtype=torch.float32, device=dev)
        call.one_kernel(y32_dev.data_ptr(), io=lib.ConvIo(x_codes=1, y_codes=0, y_ka=1.0, y_qbits=8))
        torch.cuda.synchronize()
        y32 = y32_dev.cpu().numpy()
        assert not np.isnan(y32).any(), row
        src = np.maximum(y32, np.float32(0.0)) if row.relu2 else y32   # the ReLU is folded into the quantizer
        want_codes = so.encode(src, np.float32(KA_NEXT), _fmt(reader_qbits(row)))
        assert np.array_equal(got, want_codes), (row, _first_diff(got, want_codes))
        neg = float((so.decode(got, _fmt(reader_qbits(row))) < 0).mean())
        if row.relu2:
            assert neg == 0.0, (row, neg)
        else:
            assert neg > 0.05, (row, "signed codes expected", neg)
    elif not row.relu2 and row.special is None:
        assert float((got.view(np.float32) < 0).mean()) > 0.05, row   # both signs reach the float32 output


def _block(stride, dev):
    """A 32 -> 256 block -- the pair slfp_dwpw_supported took and slfp_dwpw_fwd had no instance for -- with BatchNorm and ReLU"""
    from cnns_slfp_quantization_amd import conv2d_func as cf
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(3200 + stride)
        dw = cf.conv2d_Q(8, 0.06, 0.2)(32, 32, 3, stride=stride, padding=1, groups=32, bias=False)
        pw = cf.conv2d_Q(8, 0.02, 0.25)(32, 256, 1, bias=False)
        m = nn.Sequential(dw, nn.BatchNorm2d(32), nn.ReLU(inplace=True), pw, nn.BatchNorm2d(256), nn.ReLU(inplace=True))
        g = torch.Generator().manual_seed(78 + stride)
        with torch.no_grad():
            for bn in (m[1], m[4]):
                bn.running_mean.normal_(0.0, 0.2, generator=g)
                bn.running_var.uniform_(0.5, 1.5, generator=g)
                bn.weight.uniform_(0.8, 1.6, generator=g)
                bn.bias.normal_(0.1, 0.2, generator=g)
            dw.weight.mul_(3.0)
        x = torch.randn((3, 32, 15, 17), generator=g)
    return m.to(dev).eval().to(memory_format=torch.channels_last), x.to(dev).contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("stride", [1, 2])
def test_module_level_32_to_256_block_runs_as_one_kernel(dev, stride):
    """fusion.fuse_bn_relu + fuse_dw_pw under options.dwpw_all: the block is ONE launch and returns the bits of its two convs."""
    from cnns_slfp_quantization_amd import conv2d_func as cf, fusion
    m, x = _block(stride, dev)
    try:
        with torch.no_grad():
            assert fusion.fuse_bn_relu(m) == 2
            y_two = m(x).clone()
            cf.options.dwpw_all = True
            assert fusion.fuse_dw_pw(m) == 1
            blk = [b for b in m if isinstance(b, fusion.DwPwBlock)][0]
            y_one = m(x).clone()
            assert blk._last_kernel == "dwpw_fused_f16x1", blk._last_kernel
            assert tuple(y_one.shape) == (3, 256, (15 - 1) // stride + 1, (17 - 1) // stride + 1)
            assert torch.equal(y_one, y_two), float((y_one - y_two).abs().max())
            assert float((y_one > 0).float().mean()) > 0.05
    finally:
        cf.options.dwpw_all = False


def test_zz_every_instance_of_the_table_ran():
    """Closes the file: what the row tests launched, by the reporter's own account, is the table's set of instances; and the largest
    CPU-reference errors of check 2, per q_bit (DESIGN.md records them)."""
    for q in sorted(WORST):
        print(f"q_bit {q}: largest max-rel {WORST[q][0]:.3e}, l2 {WORST[q][1]:.3e}, elementwise fraction {WORST[q][2]:.4f}")
    assert RAN == {r.instance for r in ROWS}, RAN ^ {r.instance for r in ROWS}
