"""GPU (MI355X): every depthwise 3x3 kernel instance (csrc/conv_dw.hip, conv_dw2.hip, conv_dw3.hip, conv_dwc.hip) at the small ragged
shapes of tests/_dw_variants.py, straight through the C ABI.  The four launchers pick among about a hundred template instances; the
feature tests reach them at the nets' geometries and hold float32 results to a 1e-5 tensor-relative bar.  Here each row forces its
instance (slfp_debug_dw3x3_instance says which one runs) and is held

  * to the CPU restatement of the family's stated arithmetic (include/slfp.h; oracle/slfp_oracle.c: slfp_oracle_dw3x3_f32) BIT FOR
    BIT, a NaN equal to a NaN: float32 outputs directly (code input: the restatement on the decoded codes); code outputs as
    slfp_oracle_encode of the restatement's float32, ReLU folded or signed; the table epilogue as the byte table applied on the host to
    the restatement's layer-output value.  A window, a halo column or a tail that is one off cannot hide below a tolerance;
  * to the double-accumulating oracle under the bars of tests/_bars.py (float32 outputs; independent of the restatement);
  * to a NaN placement worked out from the input alone: NaNs planted at scattered pixels (one whose predecessor is clean, pixel 0 of
    the second image, the last channel of the last pixel) come out on exactly the output pixels whose window samples them, in exactly
    that channel -- as 0 behind the float32 ReLU, as the zero code 0x01 behind the folded ReLU, as 0x00 in signed codes;
  * inside guard bands: every tensor a launch reads or writes is a view into an arena with 4 KiB on each side -- NaN around float32
    inputs, weights and per-channel vectors, 0xA5 around code inputs and all outputs; outputs are prefilled (NaN / 0xA5), the output
    guards must be untouched and clean input must give NaN-free output;
  * to the other rows of the same layer (kernel against kernel, switch against switch, codes in against float32 in) and to itself
    on a second launch: the same bits.
"""
import ctypes

import numpy as np
import pytest
import torch

from _bars import ELEM_MIN, elem_frac_bar, tol as _tol
from _dw_variants import (KA, KA_NEXT, KW, LAYEROUT, RELU, ROWS, geom_key, instance, layer_key, make_desc, make_inputs, make_io, out_hw,
                          set_switches)
from conftest import elem_exceed_frac, rel_errors, same_bits
from oracle import slfp_oracle as so

pytestmark = pytest.mark.gpu

GUARD = 4096     # bytes on each side of every tensor
RAN = set()      # reporter strings of the launches the row tests made
_GEOMS = {}      # geom_key -> _Geom
_BLOBS = {}      # (geom_key, qbits) -> prepared weights
_SAME = {}       # layer_key -> (row name, float32 output of the clean input, of the NaN input)
_LUTS = {}       # y_qbits -> (device table, host table)


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


class _Arena:
    """A tensor as a view into a byte buffer with GUARD bytes in front of and behind it.  fill: NaN (float32 inputs) or a byte."""

    def __init__(self, shape, dtype, dev, fill, src=None):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.nbytes = n
        pad = (-n) % 16
        if fill != fill:
            self.buf = torch.full(((2 * GUARD + n + pad) // 4,), float("nan"), dtype=torch.float32, device=dev).view(torch.uint8)
            self.fill = None
        else:
            self.buf = torch.full((2 * GUARD + n + pad,), fill, dtype=torch.uint8, device=dev)
            self.fill = fill
        self.t = self.buf[GUARD:GUARD + n].view(dtype).view(shape)
        assert self.t.data_ptr() % 16 == 0
        if src is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(src)) if isinstance(src, np.ndarray) else src)

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        return bool((self.buf[:GUARD] == self.fill).all()) and bool((self.buf[GUARD + self.nbytes:] == self.fill).all())


def _fmt(qbits):
    return (so.FMT_ACT8 if qbits == 8 else so.FMT_SFP7) | so.FMT_EXT


class _Geom:
    """The inputs of one geometry key, on the host and in guarded arenas: built once, shared by its rows, never written again."""

    def __init__(self, row, dev):
        nan = float("nan")
        self.x_np, self.x_nan_np, self.w_np, self.bias_np, self.scale_np, self.shift_np = make_inputs(row)
        self.x = {False: _Arena(self.x_np.shape, torch.float32, dev, nan, self.x_np),
                  True: _Arena(self.x_np.shape, torch.float32, dev, nan, self.x_nan_np)}
        self.codes_np, self.codes = {}, {}
        for q in (8, 7):   # the codes of QA(x / Ka), by the oracle
            for planted, x in ((False, self.x_np), (True, self.x_nan_np)):
                c = so.encode(x, np.float32(KA), _fmt(q))
                self.codes_np[q, planted] = c
                self.codes[q, planted] = _Arena(c.shape, torch.uint8, dev, 0xA5, c)
        self.w = _Arena(self.w_np.shape, torch.float32, dev, nan, self.w_np)
        self.bias = _Arena((row.c,), torch.float32, dev, nan, self.bias_np)
        self.scale = _Arena((row.c,), torch.float32, dev, nan, self.scale_np)
        self.shift = _Arena((row.c,), torch.float32, dev, nan, self.shift_np)
        self.shift_nan_np = self.shift_np.copy()   # third pass: a NaN that arises in the epilogue (channel 2 of the affine's shift)
        self.shift_nan_np[2] = nan
        self.shift_nan = _Arena((row.c,), torch.float32, dev, nan, self.shift_nan_np)
        # where a NaN of the planted input is sampled, per stride and padding: from the input alone
        self.isnan = np.isnan(self.x_nan_np)
        self.planted = self.x_nan_np.view(np.uint32) != self.x_np.view(np.uint32)   # the NaNs and the infinities
        assert 2 <= int(self.isnan.sum()) <= 3 and int(self.planted.sum()) <= 5

    def window_map(self, row, sites):
        """the outputs whose window samples one of `sites` (a mask over the input), in that site's channel"""
        ho, wo = out_hw(row)
        p = np.pad(sites, ((0, 0), (row.pad, row.pad), (row.pad, row.pad), (0, 0)))
        m = np.zeros((row.n, ho, wo, row.c), dtype=bool)
        for kh in range(3):
            for kw in range(3):
                m |= p[:, kh:kh + (ho - 1) * row.stride + 1:row.stride, kw:kw + (wo - 1) * row.stride + 1:row.stride, :]
        return m


def _geom(row, dev):
    k = geom_key(row)
    if k not in _GEOMS:
        _GEOMS[k] = _Geom(row, dev)
    return _GEOMS[k]


def _blob(lib, row, d, g, dev):
    k = (geom_key(row), row.qbits)
    if k not in _BLOBS:
        L = lib.load()
        n = L.slfp_conv2d_wprep_bytes(ctypes.byref(d))
        assert n % 4 == 0 and L.slfp_conv2d_workspace_bytes(ctypes.byref(d)) == 0
        b = _Arena((n // 4,), torch.float32, dev, float("nan"))   # what prepare does not write stays NaN
        lib.check(L.slfp_conv2d_prepare_weights(ctypes.byref(d), g.w.ptr(), b.ptr(), None, _stream()))
        _BLOBS[k] = b
    return _BLOBS[k]


def _act(v):
    """the activation behind the table epilogue of these rows: x cos(3 x), elementwise and far from monotone"""
    with np.errstate(invalid="ignore"):
        return (v * np.cos(np.float32(3.0) * v)).astype(np.float32)


def _lut(lib, y_qbits, dev):
    """The byte table of the layer-output classes for the reader (KA_NEXT, y_qbits), built as tests/test_gpu_layerout_lut.py builds it:
    the class values from slfp_layerout_lut_values, the activation, the reader's encoder (here the oracle's)."""
    if y_qbits not in _LUTS:
        L = lib.load()
        n = lib.LAYEROUT_LUT_BYTES
        v = np.zeros(n, dtype=np.float32)
        lib.check(L.slfp_layerout_lut_values(v.ctypes.data, n))
        classes = L.slfp_layerout_lut_classes()
        table = so.encode(_act(v), np.float32(KA_NEXT), _fmt(y_qbits))
        _LUTS[y_qbits] = (_Arena((n,), torch.uint8, dev, 0xA5, table), table, v[:classes].view(np.uint32).copy())
    return _LUTS[y_qbits]


def _lut_apply(table, class_bits, q):
    """table[class of q] for layer-output values q (NaN: class 0)"""
    qb = q.view(np.uint32).ravel()
    isn = (qb & 0x7FFFFFFF) > 0x7F800000
    order = np.argsort(class_bits[1:], kind="stable")
    pos = np.clip(np.searchsorted(class_bits[1:][order], qb), 0, len(order) - 1)
    idx = order[pos] + 1
    assert np.array_equal(class_bits[idx][~isn], qb[~isn]), "a layer-output value without a class"
    idx[isn] = 0
    return table[idx].reshape(q.shape)


def _run(lib, row, d, g, blob, planted, dev, shift_nan=False):
    """One launch of the row through its interface; returns the output as a numpy array (uint32 bits of float32, or code bytes)."""
    L = lib.load()
    codes_out = row.iface in ("cout", "lut")
    shape = (row.n,) + out_hw(row) + (row.c,)
    y = _Arena(shape, torch.uint8 if codes_out else torch.float32, dev, 0xA5)
    if codes_out:
        assert bool((y.t == 0xA5).all())
    else:
        y.t.fill_(float("nan"))   # an element the kernel skips stays NaN
    dp = ctypes.byref(d)
    bias = g.bias.ptr() if row.bias else None
    sc, sh = (g.scale.ptr(), (g.shift_nan if shift_nan else g.shift).ptr()) if row.post else (None, None)
    if row.iface == "f32":
        lib.check(L.slfp_conv2d_fwd(dp, g.x[planted].ptr(), blob.ptr(), bias, y.ptr(), None, None, _stream()))
    elif row.iface == "post":
        lib.check(L.slfp_conv2d_fwd_post(dp, g.x[planted].ptr(), blob.ptr(), bias, sc, sh, row.flags, y.ptr(), None, None, _stream()))
    else:
        io = make_io(lib, row.iface, row.y_qbits, KA_NEXT)
        xc = g.codes[row.qbits, planted]
        if row.iface == "lut":
            assert L.slfp_conv2d_codes_lut_supported(dp, ctypes.byref(io), 0, row.c) == 1, row
            lib.check(L.slfp_conv2d_fwd_codes_lut(dp, ctypes.byref(io), xc.ptr(), blob.ptr(), None, sc, sh, _lut(lib, row.y_qbits, dev)[0].ptr(),
                                                  y.ptr(), row.c, None, _stream()))
        else:
            assert L.slfp_conv2d_codes_supported(dp, ctypes.byref(io), 0, row.flags) == 1, row
            lib.check(L.slfp_conv2d_fwd_codes(dp, ctypes.byref(io), xc.ptr(), blob.ptr(), None, sc, sh, row.flags, y.ptr(), _stream()))
    torch.cuda.synchronize()
    assert y.guards_intact(), (row, "guard band of the output written")
    out = y.t.cpu().numpy()
    return out if codes_out else out.view(np.uint32)


def _want(lib, row, g, planted, dev, shift_nan=False):
    """What the row must write, from the restatement alone."""
    x = g.codes_np[row.qbits, planted] if row.iface in ("cin", "cout", "lut") else (g.x_nan_np if planted else g.x_np)
    t = so.dw3x3_f32(x, g.w_np, g.bias_np if row.bias else None, row.stride, row.pad, KA, KW, row.qbits,
                     g.scale_np if row.post else None, (g.shift_nan_np if shift_nan else g.shift_np) if row.post else None, bool(row.flags & LAYEROUT), bool(row.flags & RELU))
    if row.iface == "cout":
        return so.encode(t, np.float32(KA_NEXT), _fmt(row.y_qbits))
    if row.iface == "lut":
        _, table, class_bits = _lut(lib, row.y_qbits, dev)
        return _lut_apply(table, class_bits, t)
    return t.view(np.uint32)


def _equal(got, want, codes_out):
    return np.array_equal(got, want) if codes_out else same_bits(got, want)


def _first_diff(got, want):
    bad = np.argwhere(got != want)
    at = tuple(bad[0]) if len(bad) else None
    return f"{len(bad)} of {got.size} differ; first at (image, row, column, channel) {at}: got {got[at]:#x}, want {want[at]:#x}" if at else "NaN placement"


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_dw_variant(lib, dev, row):
    L = lib.load()
    try:
        set_switches(L, None)
        g = _geom(row, dev)
        d = make_desc(lib, row, KA, KW)
        blob = _blob(lib, row, d, g, dev)
        set_switches(L, row.env)
        got_v = instance(lib, d, row.iface, row.bias, row.post, row.flags, row.y_qbits, KA_NEXT)
        assert got_v == row.variant, (row, got_v)
        codes_out = row.iface in ("cout", "lut")
        lo = bool(row.flags & LAYEROUT)

        # ---- clean input: the restatement's bits; no NaN unless the layer-output quantizer makes one of an exact zero
        y = _run(lib, row, d, g, blob, False, dev)
        want = _want(lib, row, g, False, dev)
        assert _equal(y, want, codes_out), (row, "clean input", _first_diff(y, want))
        if not codes_out and not lo:
            yf = y.view(np.float32)
            assert not np.isnan(yf).any(), (row, "NaN in the output of clean input: a read outside the tensor")
            # ... and the double-accumulating oracle under the family's bars (independent of the restatement)
            ref = so.conv2d(g.x_np.transpose(0, 3, 1, 2), g.w_np, g.bias_np if row.bias else None, row.stride, row.pad, 1, row.c, KA, KW,
                            row.qbits).transpose(0, 2, 3, 1).astype(np.float64)
            if row.post:
                ref = ref * g.scale_np.astype(np.float64) + g.shift_np.astype(np.float64)
            if row.flags & RELU:
                ref = np.maximum(ref, 0.0)
            emax, el2 = rel_errors(yf, ref)
            print(f"{row.name}: {got_v} max-rel {emax:.3e} l2 {el2:.3e}")
            assert emax <= _tol("dw3x3_nhwc") and el2 <= _tol("dw3x3_nhwc"), (row, emax, el2)
            if not row.post and yf.size >= ELEM_MIN:
                assert elem_exceed_frac(yf, ref) <= elem_frac_bar("dw3x3_nhwc"), row

        # ---- NaN and +-inf planted: the restatement's bits, and the placement from the input alone
        y_nan = _run(lib, row, d, g, blob, True, dev)
        want_nan = _want(lib, row, g, True, dev)
        assert _equal(y_nan, want_nan, codes_out), (row, "NaN input", _first_diff(y_nan, want_nan))
        if not lo:
            # (code input: slfp_encode_f32 gives a NaN the code 0x00, which decodes to the tiny class -- no NaN enters the kernel)
            m = g.window_map(row, g.isnan) if row.iface in ("f32", "post") else np.zeros(y.shape, dtype=bool)
            assert int(m.sum()) <= 27 and (m.any() or row.iface not in ("f32", "post"))
            clean = ~g.window_map(row, g.planted)   # outputs that sample neither a NaN nor an infinity: as of the clean input
            if codes_out:
                at_nan = 0x01 if (row.flags & RELU) else 0x00
                assert (y_nan[m] == at_nan).all(), (row, "code of a NaN", np.unique(y_nan[m]).tolist())
                assert np.array_equal(y_nan[clean], y[clean]), (row, "a planted value reaches an output whose window does not sample it")
            else:
                isn = np.isnan(y_nan.view(np.float32))
                if row.flags & RELU:
                    assert not isn.any() and (y_nan[m] == 0).all(), (row, "fmaxf(NaN, 0) is +0")
                else:
                    assert np.array_equal(isn, m), (row, f"{int(isn.sum())} NaN outputs, {int(m.sum())} expected",
                                                    np.argwhere(isn != m)[:6].tolist())
                assert np.array_equal(y_nan[clean], y[clean]), (row, "a planted value reaches an output whose window does not sample it")

        # ---- a NaN that arises in the epilogue (the affine's shift of channel 2): NaN in float32 and in the layer-output class, +0
        # behind the float32 ReLU, the zero code behind the folded ReLU (as the float32 form's fmaxf(NaN, 0)), 0x00 in signed codes
        if row.post:
            y_sh = _run(lib, row, d, g, blob, False, dev, shift_nan=True)
            want_sh = _want(lib, row, g, False, dev, shift_nan=True)
            assert _equal(y_sh, want_sh, codes_out), (row, "NaN in post_shift", _first_diff(y_sh, want_sh))
            if row.iface == "cout":
                assert (y_sh[..., 2] == (0x01 if (row.flags & RELU) else 0x00)).all(), (row, np.unique(y_sh[..., 2]).tolist())
            others = np.arange(row.c) != 2
            assert np.array_equal(y_sh[..., others], y[..., others]), (row, "the NaN of channel 2 reaches another channel")

        # ---- the same bits on a second launch, and from every other row of the same layer
        assert np.array_equal(_run(lib, row, d, g, blob, False, dev), y), (row, "run to run")
        if not codes_out:
            kind = row.iface in ("f32", "post")
            first = _SAME.setdefault((layer_key(row), kind), (row.name, y, y_nan))
            assert same_bits(first[1], y) and same_bits(first[2], y_nan), (row.name, "differs from the same layer's row", first[0])
            other = _SAME.get((layer_key(row), not kind))   # codes in against float32 in: the clean input
            assert other is None or same_bits(other[1], y), (row.name, "differs from the same layer's row", other[0])
        RAN.add(got_v)
    finally:
        set_switches(L, None)


def test_zz_every_instance_of_the_table_ran():
    """Closes the file: what the row tests launched, by the reporter's own account, is the table's set of instances."""
    assert RAN == {r.variant for r in ROWS}, RAN ^ {r.variant for r in ROWS}
