"""GPU (MI355X): every image-stem and direct kernel instance (csrc/conv_direct.hip, conv_stem_small.hip, conv_stem_mfma.hip) at the small
ragged shapes of tests/_stem_variants.py, straight through the C ABI.  The four launchers pick among about forty template instances
and their runtime forms; the feature tests reach them at the nets' geometries under tensor-relative bars.  Here each row forces its
instance (slfp_debug_stem_instance says which one runs) and is held

  * float32 kernels (direct, stem/gen, stem/fixed, stem/mx): to the CPU restatement of their stated arithmetic (include/slfp.h;
    oracle/slfp_oracle.c: slfp_oracle_conv_f32) BIT FOR BIT, a NaN equal to a NaN: float32 outputs directly; code outputs as
    slfp_oracle_encode of the restatement's float32, ReLU folded or signed; the table epilogue as the byte table applied on the host to
    the restatement's layer-output value.  A window or a halo column that is one off cannot hide below a tolerance.  And to the
    double-accumulating oracle under the bars of tests/_bars.py (independent of the restatement);
  * fp16 matrix-core kernels (small, rows, im2row): to the operand-level reference of _stem_variants.f16_reference within
    2 (K + 4) 2^-24 sum|terms| per element (derived, not measured: f16_bound; the host test shows the reference itself inside the bars),
    and to the double-accumulating oracle under the unchanged bars; code output and the table epilogue to the oracle's encoding / the
    host byte table of the same layer's float32 output by the same kernel, bit for bit;
  * to a NaN placement worked out from the input alone: NaNs planted at scattered pixels (one in the first image, pixel 0 of the
    second, the last channel of the last pixel) come out on exactly the output pixels whose window samples them, in every output
    channel of that group -- as 0 behind the float32 ReLU, as each kernel's documented code behind the folded ReLU ("NaN in
    front of a folded ReLU"), as 0x00 in signed codes; outputs whose window samples no planted value keep the clean input's bits;
  * inside guard bands: every tensor a launch reads or writes is a view into an arena with 4 KiB on each side -- NaN around float32
    inputs, weights and per-channel vectors, 0xA5 around outputs and the workspace; outputs are prefilled (NaN / 0xA5), the output and
    workspace guards must be untouched and clean input must give NaN-free output;
  * to the other rows of the same layer (k_stem_mx against k_stem_fixed, k_stem_rows against the two-kernel form, the table against
    the long-form quantizer) and to itself on a second launch: the same bits.
"""
import ctypes
import time

import numpy as np
import pytest
import torch

from _bars import ELEM_MIN, elem_frac_bar, tol as _tol
from _stem_variants import (F16_KINDS, KA, KA_NEXT, KW, LAYEROUT, RELU, ROWS, chunk, f16_bound, f16_reference, geom_key, instance, kind, layer_key,
                            make_desc, make_inputs, make_io, out_hw, set_switches)
from conftest import elem_exceed_frac, rel_errors, same_bits
from oracle import slfp_oracle as so

pytestmark = pytest.mark.gpu

GUARD = 4096     # bytes on each side of every tensor
RAN = set()      # reporter strings of the launches the row tests made
TIMES = {}       # row name -> seconds
RATIO = {}       # fp16 kernel -> largest |y - reference| / bound seen
_GEOMS = {}      # geom_key -> _Geom
_BLOBS = {}      # (geom_key, qbits, passes, family) -> prepared weights
_SAME = {}       # (layer_key, arithmetic, output form) -> (row name, output of the clean input, of the NaN input)
_LUTS = {}       # y_qbits -> (device table, host table, class bits)


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
        self.w = _Arena(self.w_np.shape, torch.float32, dev, nan, self.w_np)
        self.bias = _Arena((row.c_out,), torch.float32, dev, nan, self.bias_np)
        self.scale = _Arena((row.c_out,), torch.float32, dev, nan, self.scale_np)
        self.shift = _Arena((row.c_out,), torch.float32, dev, nan, self.shift_np)
        self.isnan = np.isnan(self.x_nan_np)
        self.planted = self.x_nan_np.view(np.uint32) != self.x_np.view(np.uint32)   # the NaNs and the infinities
        assert 2 <= int(self.isnan.sum()) <= 3 and int(self.planted.sum()) <= 5
        self.cache = {}   # host references shared by the rows of a layer

    def window_map(self, row, sites):
        """the outputs whose window samples one of `sites` (a mask over the input): every output channel of the site's group"""
        ho, wo = out_hw(row)
        (ph, pw), (sh, sw), (dh, dw) = row.pad, row.stride, row.dil
        cg, og = row.c_in // row.groups, row.c_out // row.groups
        m = np.zeros((row.n, ho, wo, row.c_out), dtype=bool)
        for g in range(row.groups):
            s = sites[..., g * cg:(g + 1) * cg].any(axis=-1)
            p = np.pad(s, ((0, 0), (ph, ph), (pw, pw)))
            hit = np.zeros((row.n, ho, wo), dtype=bool)
            for kh in range(row.k[0]):
                for kw in range(row.k[1]):
                    hit |= p[:, kh * dh:kh * dh + (ho - 1) * sh + 1:sh, kw * dw:kw * dw + (wo - 1) * sw + 1:sw]
            m[..., g * og:(g + 1) * og] = hit[..., None]
        return m


def _geom(row, dev):
    k = geom_key(row)
    if k not in _GEOMS:
        _GEOMS[k] = _Geom(row, dev)
    return _GEOMS[k]


def _blob(lib, row, d, g, dev):
    """prepared weights and the workspace of the descriptor's family (the blob's layout depends on the family, not on the switches)"""
    L = lib.load()
    fam = L.slfp_conv2d_kernel_name(ctypes.byref(d)).decode()
    k = (geom_key(row), row.stride, row.qbits, fam)
    if k not in _BLOBS:
        n = L.slfp_conv2d_wprep_bytes(ctypes.byref(d))
        assert n > 0 and n % 4 == 0
        b = _Arena((n // 4,), torch.float32, dev, float("nan"))   # what prepare does not write stays NaN
        lib.check(L.slfp_conv2d_prepare_weights(ctypes.byref(d), g.w.ptr(), b.ptr(), None, _stream()))
        _BLOBS[k] = b
    return _BLOBS[k]


def _workspace(lib, d, dev):
    n = lib.load().slfp_conv2d_workspace_bytes(ctypes.byref(d))
    return _Arena((n,), torch.uint8, dev, 0xA5) if n else None


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
    qb = np.ascontiguousarray(q).view(np.uint32).ravel()
    isn = (qb & 0x7FFFFFFF) > 0x7F800000
    order = np.argsort(class_bits[1:], kind="stable")
    pos = np.clip(np.searchsorted(class_bits[1:][order], qb), 0, len(order) - 1)
    idx = order[pos] + 1
    assert np.array_equal(class_bits[idx][~isn], qb[~isn]), "a layer-output value without a class"
    idx[isn] = 0
    return table[idx].reshape(q.shape)


def _run(lib, row, d, g, blob, planted, dev, iface=None, flags=None):
    """One launch of the row's layer through `iface` (default: the row's); returns the output as a numpy array (uint32 bits of float32,
    or code bytes)."""
    L = lib.load()
    iface = iface or row.iface
    flags = row.flags if flags is None else flags
    codes_out = iface in ("cout", "lut")
    shape = (row.n,) + out_hw(row) + (row.c_out,)
    y = _Arena(shape, torch.uint8 if codes_out else torch.float32, dev, 0xA5)
    if not codes_out:
        y.t.fill_(float("nan"))   # an element the kernel skips stays NaN
    ws = _workspace(lib, d, dev)
    wsp = ws.ptr() if ws is not None else None
    dp = ctypes.byref(d)
    bias = g.bias.ptr() if row.bias else None
    sc, sh = (g.scale.ptr(), g.shift.ptr()) if row.post else (None, None)
    x = g.x[planted].ptr()
    if iface == "f32":
        lib.check(L.slfp_conv2d_fwd(dp, x, blob.ptr(), bias, y.ptr(), None, wsp, _stream()))
    elif iface == "post":
        lib.check(L.slfp_conv2d_fwd_post(dp, x, blob.ptr(), bias, sc, sh, flags, y.ptr(), None, wsp, _stream()))
    else:
        io = make_io(lib, iface, row.y_qbits, KA_NEXT)
        if iface == "lut":
            assert L.slfp_conv2d_codes_lut_supported(dp, ctypes.byref(io), int(row.bias), row.c_out) == 1, row
            lib.check(L.slfp_conv2d_fwd_codes_lut(dp, ctypes.byref(io), x, blob.ptr(), bias, sc, sh, _lut(lib, row.y_qbits, dev)[0].ptr(),
                                                  y.ptr(), row.c_out, wsp, _stream()))
        else:
            assert L.slfp_conv2d_codes_supported(dp, ctypes.byref(io), int(row.bias), flags) == 1, row
            lib.check(L.slfp_conv2d_fwd_codes_ws(dp, ctypes.byref(io), x, blob.ptr(), bias, sc, sh, flags, y.ptr(), wsp, _stream()))
    torch.cuda.synchronize()
    assert y.guards_intact(), (row, "guard band of the output written")
    assert ws is None or ws.guards_intact(), (row, "guard band of the workspace written")
    out = y.t.cpu().numpy()
    return out if codes_out else out.view(np.uint32)


def _nan_code(row):
    """the code a NaN gets ("NaN in front of a folded ReLU"): the zero code from k_stem_rows / k_stem_mfma behind a folded
    ReLU; 0x00 from the other kernels, in signed codes, and wherever slfp_encode_f32 codes a NaN"""
    return 0x01 if (row.flags & RELU) and kind(row) in ("rows", "im2row") else 0x00


def _codes_of(lib, row, t, dev, m_nan):
    """the bytes a code-writing row must store for the float32 result t of its layer (cout: t before the ReLU, which the quantizer folds
    in; lut: the layer-output value); m_nan: where a NaN input is sampled"""
    if row.iface == "lut":
        _, table, class_bits = _lut(lib, row.y_qbits, dev)
        return _lut_apply(table, class_bits, t)
    tf = t.view(np.float32)
    isn = np.isnan(tf)
    if row.flags & RELU:
        with np.errstate(invalid="ignore"):
            tf = np.where(isn, np.float32(0.0), np.maximum(tf, np.float32(0.0))).astype(np.float32)
    c = so.encode(tf, np.float32(KA_NEXT), _fmt(row.y_qbits))
    c[isn | m_nan] = _nan_code(row)
    return c


def _restatement(row, g, planted, layerout, relu):
    key = ("f32", layer_key(row)[len(geom_key(row)):], chunk(row), planted, layerout, relu)
    if key not in g.cache:
        g.cache[key] = so.conv_f32(g.x_nan_np if planted else g.x_np, g.w_np, g.bias_np if row.bias else None, row.stride, row.pad, row.dil,
                                   row.groups, KA, KW, row.qbits, chunk(row), g.scale_np if row.post else None,
                                   g.shift_np if row.post else None, layerout, relu)
    return g.cache[key]


def _oracle(row, g):
    """the double-accumulating oracle of the clean input with the affine and the ReLU in float64, NHWC"""
    key = ("f64", layer_key(row)[len(geom_key(row)):])
    if key not in g.cache:
        ref = so.conv2d(g.x_np.transpose(0, 3, 1, 2), g.w_np, g.bias_np if row.bias else None, row.stride, row.pad, row.dil, row.groups, KA,
                        KW, row.qbits).transpose(0, 2, 3, 1).astype(np.float64)
        if row.post:
            ref = ref * g.scale_np.astype(np.float64) + g.shift_np.astype(np.float64)
        if row.flags & RELU:
            ref = np.maximum(ref, 0.0)
        g.cache[key] = ref
    return g.cache[key]


def _first_diff(got, want):
    bad = np.argwhere(got != want)
    at = tuple(bad[0]) if len(bad) else None
    return f"{len(bad)} of {got.size} differ; first at (image, row, column, channel) {at}: got {got[at]:#x}, want {want[at]:#x}" if at else "NaN placement"


def _bars(row, yf, ref, name, got_v):
    emax, el2 = rel_errors(yf, ref)
    print(f"{row.name}: {got_v} max-rel {emax:.3e} l2 {el2:.3e}")
    assert emax <= _tol(name) and el2 <= _tol(name), (row, emax, el2)
    if not row.post and yf.size >= ELEM_MIN:
        assert elem_exceed_frac(yf, ref) <= elem_frac_bar(name), row


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_stem_variant(lib, dev, row):
    L = lib.load()
    t0 = time.perf_counter()
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
        f16 = kind(row) in F16_KINDS
        equal = np.array_equal if codes_out else same_bits
        m = g.window_map(row, g.isnan)            # outputs that sample a NaN
        clean = ~g.window_map(row, g.planted)     # outputs that sample neither a NaN nor an infinity: as of the clean input
        assert m.any() and clean.any()
        none = np.zeros(m.shape, dtype=bool)

        y = _run(lib, row, d, g, blob, False, dev)
        y_nan = _run(lib, row, d, g, blob, True, dev)
        if not f16:
            # ---- float32 kernels: the restatement's bits, clean and with NaN and +-inf planted
            for planted, got, mm in ((False, y, none), (True, y_nan, m)):
                if codes_out:
                    want = _codes_of(lib, row, _restatement(row, g, planted, lo, False).view(np.uint32), dev, mm)
                else:
                    want = _restatement(row, g, planted, lo, bool(row.flags & RELU)).view(np.uint32)
                assert equal(got, want), (row, "NaN input" if planted else "clean input", _first_diff(got, want))
            if not codes_out and not lo:   # ... and the double-accumulating oracle under the family's bars
                _bars(row, y.view(np.float32), _oracle(row, g), "direct_nhwc", got_v)
        elif not codes_out:
            # ---- fp16 kernels, float32 out: the operand-level reference within the derived bound; the oracle under the bars
            yf = y.view(np.float32).astype(np.float64)
            key = ("f16", layer_key(row)[len(geom_key(row)):])
            if key not in g.cache:
                g.cache[key] = f16_reference(row, g.x_np, g.w_np, g.bias_np, g.scale_np, g.shift_np, so)
            ref16, mag = g.cache[key]
            bound = f16_bound(row, mag)
            err = np.abs(yf - ref16)
            ratio = float((err / np.maximum(bound, 1e-300)).max())
            RATIO[kind(row)] = max(RATIO.get(kind(row), 0.0), ratio)
            print(f"{row.name}: {got_v} max |y - operand-level reference| / bound {ratio:.4f}")
            assert (err <= bound).all(), (row, ratio, np.argwhere(err > bound)[:4].tolist())
            _bars(row, y.view(np.float32), _oracle(row, g), "stem_mfma_f16x1" if row.qbits == 8 else "stem_mfma_f16_exact", got_v)
        else:
            # ---- fp16 kernels, codes out: the oracle's encoding / the host byte table of the same kernel's float32 output
            tw_flags = row.flags & ~RELU   # the ReLU is the quantizer's: code the value in front of it
            for planted, got, mm in ((False, y, none), (True, y_nan, m)):
                twin = _run(lib, row, d, g, blob, planted, dev, iface="post", flags=tw_flags)
                want = _codes_of(lib, row, twin, dev, mm)
                assert equal(got, want), (row, "NaN input" if planted else "clean input", _first_diff(got, want))
            # ... and that kernel's float32 output of the bare layer (bias and affine as the row's, no quantizer, no ReLU) within the
            # derived bound of the operand-level reference: a code row's window is checked as a float32 row's is
            bare = row._replace(flags=0, iface="post")
            yb = _run(lib, bare, d, g, blob, False, dev).view(np.float32).astype(np.float64)
            ref16, mag = f16_reference(bare, g.x_np, g.w_np, g.bias_np, g.scale_np, g.shift_np, so)
            err, bound = np.abs(yb - ref16), f16_bound(bare, mag)
            assert (err <= bound).all(), (row, "float32 output of the same layer", float((err / np.maximum(bound, 1e-300)).max()))

        # ---- clean input gives NaN-free output; the NaN placement from the input alone
        if not lo:
            if codes_out:
                assert (y_nan[m] == _nan_code(row)).all(), (row, "code of a NaN", np.unique(y_nan[m]).tolist())
            else:
                assert not np.isnan(y.view(np.float32)).any(), (row, "NaN in the output of clean input: a read outside the tensor")
                isn = np.isnan(y_nan.view(np.float32))
                if row.flags & RELU:
                    assert not isn.any() and (y_nan[m] == 0).all(), (row, "fmaxf(NaN, 0) is +0")
                else:
                    assert np.array_equal(isn, m), (row, f"{int(isn.sum())} NaN outputs, {int(m.sum())} expected",
                                                    np.argwhere(isn != m)[:6].tolist())
            assert np.array_equal(y_nan[clean], y[clean]), (row, "a planted value reaches an output whose window does not sample it")

        # ---- the same bits on a second launch, and from every other row of the same layer with the same arithmetic
        assert np.array_equal(_run(lib, row, d, g, blob, False, dev), y), (row, "run to run")
        arith = "f16" if f16 else ("direct", chunk(row)) if kind(row) == "direct" else "stem"
        form = (row.iface, row.y_qbits) if codes_out else "f32"
        first = _SAME.setdefault((layer_key(row), arith, form), (row.name, y, y_nan))
        assert equal(first[1], y) and equal(first[2], y_nan), (row.name, "differs from the same layer's row", first[0])
        RAN.add(got_v)
    finally:
        set_switches(L, None)
        TIMES[row.name] = time.perf_counter() - t0


def test_zz_every_instance_of_the_table_ran():
    """Closes the file: what the row tests launched, by the reporter's own account, is the table's set of instances."""
    if TIMES:
        slow = max(TIMES, key=TIMES.get)
        print(f"\n{len(TIMES)} rows in {sum(TIMES.values()):.1f} s; slowest {slow}: {TIMES[slow]:.2f} s")
    for k in sorted(RATIO):
        print(f"{k}: largest |y - operand-level reference| / bound {RATIO[k]:.4f}")
    assert RAN == {r.variant for r in ROWS}, RAN ^ {r.variant for r in ROWS}
