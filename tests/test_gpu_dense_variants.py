"""GPU (MI355X): every dense k x k kernel variant (csrc/conv_dense.hip) at the small ragged shapes of tests/_dense_variants.py,
straight through the C ABI.  The six tilings, the general / unrolled / weights-resident bodies and their NWB / NSLOT / plane
specialisations each carry their own hand-counted waits, halo staging plan and epilogue unroll; the workloads reach the wide
ones only at full batch.  Here each row forces its variant (slfp_debug_dense_variant says which one runs) and is held

  * to the CPU oracle, by the bars of tests/_bars.py;
  * to the layer's unforced launch, bit for bit: every output element accumulates chunk -> tap -> k-step in the same order in
    every tiling and body, NaN inputs included;
  * on the code interface (rows with C_out % 16 == 0): codes in == float32 in; codes out == slfp_encode_f32(float32 out),
    with and without ReLU, dense and into a channel slice of a wider tensor;
  * to itself: a second launch gives the same bits (a fragment read before its DMA landed shows here).
"""
import ctypes

import numpy as np
import pytest
import torch

from _bars import ELEM_MIN, elem_frac_bar, tol as _tol
from _dense_variants import ROWS, desc_key, make_desc, set_switches
from conftest import elem_exceed_frac, rel_errors, same_bits
from oracle import slfp_oracle as so

pytestmark = pytest.mark.gpu

KA, KW, KA_NEXT = 0.21, 0.027, 0.2345
RAN = set()      # reporter strings of the launches the row tests made
_LAYERS = {}     # desc_key -> _Layer


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


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


class _Layer:
    """One descriptor of the table: seeded input (clean and with NaNs planted), weights, bias, post vectors, the prepared blob, and --
    computed once, shared by the rows of this descriptor, never written again -- the oracle's output and the unforced launches'."""

    def __init__(self, lib, row, dev):
        L = lib.load()
        self.lib, self.L, self.row = lib, L, row
        self.d = make_desc(lib, row, KA, KW)
        gen = torch.Generator(device=dev).manual_seed(4000 + sum(desc_key(row)[:11]))
        self.x = torch.relu(torch.randn((row.n, row.h, row.w, row.c_in), generator=gen, device=dev)) * (5.0 * KA)
        self.x_nan = self.x.clone()
        self.x_nan.view(-1)[13::1009] = float("nan")
        self.w = torch.randn((row.c_out, row.c_in, row.kh, row.kw), generator=gen, device=dev) * (4.0 * KW)
        self.bias = torch.randn(row.c_out, generator=gen, device=dev) * 0.3
        self.scale = torch.rand(row.c_out, generator=gen, device=dev) + 0.5
        self.shift = torch.randn(row.c_out, generator=gen, device=dev) * 0.3
        ho, wo = ctypes.c_int64(), ctypes.c_int64()
        lib.check(L.slfp_conv2d_out_shape(ctypes.byref(self.d), ctypes.byref(ho), ctypes.byref(wo)))
        self.out_shape = (row.n, ho.value, wo.value, row.c_out)
        self.kern = L.slfp_conv2d_kernel_name(ctypes.byref(self.d)).decode()
        assert self.kern.startswith("dense_mfma"), self.kern
        self.blob = torch.empty(L.slfp_conv2d_wprep_bytes(ctypes.byref(self.d)), dtype=torch.uint8, device=dev)
        lib.check(L.slfp_conv2d_prepare_weights(ctypes.byref(self.d), self.w.data_ptr(), self.blob.data_ptr(), None, _stream()))
        self.ws = torch.empty(L.slfp_conv2d_workspace_bytes(ctypes.byref(self.d)), dtype=torch.uint8, device=dev)
        self.fmt = (lib.FMT_ACT8 if row.qbits == 8 else lib.FMT_SFP7) | lib.FMT_EXT
        self.xc = self.encode(self.x, KA)
        set_switches(L, None)
        self.base = self.fwd(self.x).cpu().numpy()
        self.base_nan = self.fwd(self.x_nan).cpu().numpy()
        assert np.isnan(self.base_nan).any() and not np.isnan(self.base).any()
        self.ref = so.conv2d(self.x.permute(0, 3, 1, 2).contiguous().cpu().numpy(), self.w.cpu().numpy(), self.bias.cpu().numpy(),
                             row.stride, (row.pad_h, row.pad_w), 1, 1, KA, KW, row.qbits)

    def variant(self, x_codes=0):
        return self.L.slfp_debug_dense_variant(ctypes.byref(self.d), x_codes).decode()

    def encode(self, t, ka):
        c = torch.empty(t.shape, dtype=torch.uint8, device=t.device)
        self.lib.check(self.L.slfp_encode_f32(t.data_ptr(), c.data_ptr(), t.numel(), float(np.float32(ka)), self.fmt, _stream()))
        return c

    def fwd(self, x):
        """slfp_conv2d_fwd: float32 in, float32 out, bias, no post-op"""
        y = torch.empty(self.out_shape, device=x.device)
        self.lib.check(self.L.slfp_conv2d_fwd(ctypes.byref(self.d), x.data_ptr(), self.blob.data_ptr(), self.bias.data_ptr(), y.data_ptr(),
                                              None, self.ws.data_ptr(), _stream()))
        return y

    def fwd_post(self, x, relu):
        """slfp_conv2d_fwd_post: float32 in, float32 out, bias and scale / shift (+ ReLU)"""
        y = torch.empty(self.out_shape, device=x.device)
        self.lib.check(self.L.slfp_conv2d_fwd_post(ctypes.byref(self.d), x.data_ptr(), self.blob.data_ptr(), self.bias.data_ptr(),
                                                   self.scale.data_ptr(), self.shift.data_ptr(), relu, y.data_ptr(), None,
                                                   self.ws.data_ptr(), _stream()))
        return y

    def fwd_codes(self, x, x_codes, y_codes, relu, y=None, y_ld=0):
        """slfp_conv2d_fwd_codes_ws, or slfp_conv2d_fwd_codes_slice into `y` with pixel stride y_ld; the same bias and post vectors"""
        lib, L = self.lib, self.L
        io = lib.ConvIo(x_codes=int(x_codes), y_codes=int(y_codes), y_ka=float(np.float32(KA_NEXT if y_codes else 1.0)), y_qbits=self.row.qbits)
        args = (x.data_ptr(), self.blob.data_ptr(), self.bias.data_ptr(), self.scale.data_ptr(), self.shift.data_ptr(), relu)
        if y_ld:
            assert L.slfp_conv2d_codes_slice_supported(ctypes.byref(self.d), ctypes.byref(io), 1, relu, y_ld) == 1
            lib.check(L.slfp_conv2d_fwd_codes_slice(ctypes.byref(self.d), ctypes.byref(io), *args, y.data_ptr(), y_ld, self.ws.data_ptr(), _stream()))
            return y
        assert L.slfp_conv2d_codes_supported(ctypes.byref(self.d), ctypes.byref(io), 1, relu) == 1, (self.row, x_codes, y_codes)
        y = torch.empty(self.out_shape, dtype=torch.uint8 if y_codes else torch.float32, device=x.device)
        lib.check(L.slfp_conv2d_fwd_codes_ws(ctypes.byref(self.d), ctypes.byref(io), *args, y.data_ptr(), self.ws.data_ptr(), _stream()))
        return y


def _layer(lib, row, dev):
    key = desc_key(row)
    if key not in _LAYERS:
        _LAYERS[key] = _Layer(lib, row, dev)
    return _LAYERS[key]


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_dense_variant(lib, dev, row):
    L = lib.load()
    try:
        lay = _layer(lib, row, dev)   # (leaves the switches unset)
        set_switches(L, row.env)
        assert lay.variant() == row.variant, (row, lay.variant())
        ran = {lay.variant()}

        # ---- against the oracle, all images
        y = lay.fwd(lay.x)
        got = y.permute(0, 3, 1, 2).contiguous().cpu().numpy()
        emax, el2 = rel_errors(got, lay.ref)
        frac = elem_exceed_frac(got, lay.ref)
        print(f"{row.name}: {row.variant} {lay.kern} max-rel {emax:.3e} l2 {el2:.3e} elem-frac {frac:.4f}")
        assert emax <= _tol(lay.kern) and el2 <= _tol(lay.kern), (row, emax, el2)
        assert got.size >= ELEM_MIN
        assert frac <= elem_frac_bar(lay.kern), (row, frac)

        # ---- across tilings and bodies: the bits of the unforced launch, NaN inputs included
        assert same_bits(y.cpu().numpy(), lay.base), row
        y_nan = lay.fwd(lay.x_nan)
        assert same_bits(y_nan.cpu().numpy(), lay.base_nan), row

        # ---- run to run
        y2 = lay.fwd(lay.x)
        assert torch.equal(_bits(y2), _bits(y)), row

        # ---- the code interface on this variant
        if row.c_out % 16 == 0:
            ran.add(lay.variant(1))
            for relu in (1, 0):
                y_ref = lay.fwd_post(lay.x, relu)
                codes_ref = lay.encode(y_ref, KA_NEXT)
                yc = lay.fwd_codes(lay.xc, True, False, relu)                 # codes in, float32 out
                assert torch.equal(_bits(yc), _bits(y_ref)), (row, relu, "codes in")
                for src, is_codes in ((lay.x, False), (lay.xc, True)):        # float32 / codes in, codes out
                    c = lay.fwd_codes(src, is_codes, True, relu)
                    bad = int((c != codes_ref).sum())
                    assert bad == 0, (row, relu, is_codes, bad, c.numel())
                    c2 = lay.fwd_codes(src, is_codes, True, relu)
                    assert torch.equal(c2, c), (row, relu, is_codes, "run to run")
                # into the upper half of a tensor twice as wide: exactly those bytes, nothing else touched
                n, ho, wo, co = lay.out_shape
                wide = torch.full((n, ho, wo, 2 * co), 0xA5, dtype=torch.uint8, device=dev)
                lay.fwd_codes(lay.xc, True, True, relu, y=wide[..., co:], y_ld=2 * co)
                assert wide[..., co:].data_ptr() == wide.data_ptr() + co
                assert torch.equal(wide[..., co:], codes_ref), (row, relu, "slice")
                assert bool((wide[..., :co] == 0xA5).all()), (row, relu, "outside the slice")
        RAN.update(ran)
    finally:
        set_switches(L, None)


def test_zz_every_variant_of_the_table_ran():
    """Closes the file: what the row tests launched, by the reporter's own account, is the table's set of variants."""
    assert RAN == {r.variant for r in ROWS}, RAN ^ {r.variant for r in ROWS}
