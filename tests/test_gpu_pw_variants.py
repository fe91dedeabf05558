"""GPU (MI355X): every pointwise (1x1) kernel instance (csrc/conv_pw.hip, csrc/conv_pw_codes.hip) at the small ragged shapes of
tests/_pw_variants.py, straight through the C ABI.  The launchers pick among well over a hundred template instances; the
feature tests reach them at the workloads' channel counts and mostly compare a fused launch with an unfused one that runs the
same kernel body.  Here each row forces its instance (slfp_debug_pw_variant says which one runs) and is held

  * to the CPU oracle, by the bars of tests/_bars.py (float32 outputs directly; code outputs through the layer's unforced
    float32 launch, which is held to the oracle when the layer is built);
  * to the layer's unforced float32-interface launches, bit for bit: stream against tiled, table against long form, staged against
    direct stores, capped against uncapped grid, codes in against float32 in;
  * to a NaN placement worked out without any kernel: NaNs planted at scattered input pixels (one whose predecessor is clean,
    pixel 0 of the second image) must come out on exactly the output pixels that sample them, in all channels;
  * inside guard bands: every tensor a launch reads or writes is a view into an arena with 4 KiB on each side -- NaN around the
    float32 inputs (a read past the end that feeds the result shows as a NaN in the output of clean input), 0xA5 around the
    outputs (must be untouched);
  * on its interface: codes out == slfp_encode_f32(float32 out) with and without ReLU; residual == relu?(post(conv) + res) built
    in torch; second output == the codes of the first; a slice store writes exactly the slice's bytes;
  * to itself: a second launch gives the same bits.
"""
import ctypes

import numpy as np
import pytest
import torch

from _bars import ELEM_MIN, elem_frac_bar, tol as _tol
from _pw_variants import ROWS, desc_key, make_desc, set_switches, variant as _variant
from conftest import elem_exceed_frac, rel_errors, same_bits
from oracle import slfp_oracle as so

pytestmark = pytest.mark.gpu

KA, KW, KA_NEXT = 0.21, 0.027, 0.2345
GUARD = 4096     # bytes on each side of every tensor
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


class _Arena:
    """A tensor as a view into a byte buffer with GUARD bytes in front of and behind it."""

    def __init__(self, shape, dtype, dev, fill, src=None):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.nbytes = n
        if dtype == torch.float32 and fill != fill:   # NaN guards around a float32 input
            self.buf = torch.full(((2 * GUARD + n) // 4,), float("nan"), dtype=torch.float32, device=dev).view(torch.uint8)
            self.fill = None
        else:
            self.buf = torch.full((2 * GUARD + n,), fill, dtype=torch.uint8, device=dev)
            self.fill = fill
        self.t = self.buf[GUARD:GUARD + n].view(dtype).view(shape)
        assert self.t.data_ptr() % 16 == 0
        if src is not None:
            self.t.copy_(src)

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        return bool((self.buf[:GUARD] == self.fill).all()) and bool((self.buf[GUARD + self.nbytes:] == self.fill).all())


def _nan_in(t, dev):
    return _Arena(t.shape, torch.float32, dev, float("nan"), t)


class _Layer:
    """One descriptor of the table: seeded inputs (clean and with NaNs planted, as float32 and as codes) in guarded arenas, weights,
    bias, post vectors, residual, the prepared blob, and -- computed once, shared by the rows of this descriptor, never written
    again -- the oracle's output, the NaN placement, and the unforced float32-interface launches."""

    def __init__(self, lib, row, dev):
        L = lib.load()
        self.lib, self.L, self.row, self.dev = lib, L, row, dev
        self.d = make_desc(lib, row, KA, KW)
        gen = torch.Generator(device=dev).manual_seed(7000 + sum(desc_key(row)))
        x = torch.randn((row.n, row.h, row.w, row.c_in), generator=gen, device=dev) * (2.5 * KA)
        x.view(-1)[::97] = 17.0 * KA    # beyond the clamp
        x.view(-1)[5::193] = 0.0        # exact zeros
        # NaNs at scattered input pixels: (image, row, column, channel).  (0, 0, 6): its predecessor is clean, and channel 3 is one that
        # the predecessor would pick up if it read a k-step past its own row; (1, 0, 0): pixel 0 of the second image; one in the last
        # channel; two at an odd row or column, which stride 2 does not sample
        x_nan = x.clone()
        for img, r, c, ch in ((0, 0, 6, 3), (1, 0, 0, 1), (1, 4, 8, row.c_in - 1), (0, 3, 5, row.c_in // 2), (1, row.h - 1, row.w - 2, 0)):
            x_nan[img, r, c, ch] = float("nan")
        self.x, self.x_nan = _nan_in(x, dev), _nan_in(x_nan, dev)
        self.w = torch.randn((row.c_out, row.c_in, 1, 1), generator=gen, device=dev) * (4.0 * KW)
        self.bias = torch.randn(row.c_out, generator=gen, device=dev) * 0.3
        self.scale = torch.rand(row.c_out, generator=gen, device=dev) + 0.5
        self.shift = torch.randn(row.c_out, generator=gen, device=dev) * 0.3
        ho, wo = ctypes.c_int64(), ctypes.c_int64()
        lib.check(L.slfp_conv2d_out_shape(ctypes.byref(self.d), ctypes.byref(ho), ctypes.byref(wo)))
        self.out_shape = (row.n, ho.value, wo.value, row.c_out)
        self.res = _nan_in(torch.randn(self.out_shape, generator=gen, device=dev) * 0.8, dev)
        self.res0 = _nan_in(torch.zeros(self.out_shape, device=dev), dev)
        self.kern = L.slfp_conv2d_kernel_name(ctypes.byref(self.d)).decode()
        assert self.kern.startswith("pw_mfma"), self.kern
        self.blob = torch.empty(L.slfp_conv2d_wprep_bytes(ctypes.byref(self.d)), dtype=torch.uint8, device=dev)
        lib.check(L.slfp_conv2d_prepare_weights(ctypes.byref(self.d), self.w.data_ptr(), self.blob.data_ptr(), None, _stream()))
        assert L.slfp_conv2d_workspace_bytes(ctypes.byref(self.d)) == 0
        self.fmt = (lib.FMT_ACT8 if row.qbits == 8 else lib.FMT_SFP7) | lib.FMT_EXT
        self.xc = _Arena(x.shape, torch.uint8, dev, 0x7F, self.encode(x, KA))
        # the placement of NaNs, from the input alone: an output pixel is NaN iff the input pixel it samples holds one
        nan_px = torch.isnan(x_nan).any(dim=-1)[:, ::row.stride, ::row.stride].cpu().numpy()
        assert nan_px.shape == self.out_shape[:3] and 3 <= nan_px.sum() <= 5
        self.nan_px = nan_px
        # the oracle, and the unforced launches every row of this descriptor is compared with
        self.ref = so.conv2d(x.permute(0, 3, 1, 2).contiguous().cpu().numpy(), self.w.cpu().numpy(), self.bias.cpu().numpy(),
                             row.stride, 0, 1, 1, KA, KW, row.qbits)
        set_switches(L, None)
        self.base = self.f32(self.x)
        self.check_oracle(self.base, "unforced")
        self.base_nan = self.f32(self.x_nan)
        self.check_nan_placement(self.base_nan, "unforced")
        self.post = {relu: self.f32(self.x, post=True, relu=relu) for relu in (0, 1)}

    # ---- helpers
    def variant(self, iface):
        return _variant(self.lib, self.d, iface, self.row.qbits, KA_NEXT)

    def encode(self, t, ka):
        c = torch.empty(t.shape, dtype=torch.uint8, device=t.device)
        self.lib.check(self.L.slfp_encode_f32(t.contiguous().data_ptr(), c.data_ptr(), t.numel(), float(np.float32(ka)), self.fmt, _stream()))
        return c

    def io(self, x_codes, y_codes):
        return self.lib.ConvIo(x_codes=int(x_codes), y_codes=int(y_codes), y_ka=float(np.float32(KA_NEXT if y_codes else 1.0)), y_qbits=self.row.qbits)

    def _vecs(self, post):
        return (self.bias.data_ptr(), self.scale.data_ptr() if post else None, self.shift.data_ptr() if post else None)

    def _out(self, dtype=torch.float32):
        return _Arena(self.out_shape, dtype, self.dev, 0xA5)

    def _done(self, *outs):
        for o in outs:
            assert o.guards_intact(), (self.row, "guard band written")
        return outs[0].t if len(outs) == 1 else tuple(o.t for o in outs)

    # ---- the entry points (all with the bias; post: scale / shift as well)
    def f32(self, x, post=False, relu=0):
        y = self._out()
        d, (b, sc, sh) = ctypes.byref(self.d), self._vecs(post)
        self.lib.check(self.L.slfp_conv2d_fwd_post(d, x.ptr(), self.blob.data_ptr(), b, sc, sh, relu, y.ptr(), None, None, _stream()))
        return self._done(y)

    def codes(self, x, y_codes, post=False, relu=0):
        y = self._out(torch.uint8 if y_codes else torch.float32)
        d, io, (b, sc, sh) = ctypes.byref(self.d), self.io(True, y_codes), self._vecs(post)
        assert self.L.slfp_conv2d_codes_supported(d, ctypes.byref(io), 1, relu) == 1, self.row
        self.lib.check(self.L.slfp_conv2d_fwd_codes(d, ctypes.byref(io), x.ptr(), self.blob.data_ptr(), b, sc, sh, relu, y.ptr(), _stream()))
        return self._done(y)

    def entry(self, x, post=False, relu=0):
        y = self._out(torch.uint8)
        d, io, (b, sc, sh) = ctypes.byref(self.d), self.io(False, True), self._vecs(post)
        assert self.L.slfp_conv2d_entry_supported(d, ctypes.byref(io), 1, relu) == 1, self.row
        self.lib.check(self.L.slfp_conv2d_fwd_entry(d, ctypes.byref(io), x.ptr(), self.blob.data_ptr(), b, sc, sh, relu, y.ptr(), _stream()))
        return self._done(y)

    def resid(self, x, x_codes, res, post=False, relu=0):
        y = self._out()
        d, io, (b, sc, sh) = ctypes.byref(self.d), self.io(x_codes, False), self._vecs(post)
        assert self.L.slfp_conv2d_res_supported(d, ctypes.byref(io), 1, relu) == 1, self.row
        self.lib.check(self.L.slfp_conv2d_fwd_res(d, ctypes.byref(io), x.ptr(), self.blob.data_ptr(), b, sc, sh, relu, res.ptr(), y.ptr(), None, _stream()))
        return self._done(y)

    def dual(self, x, res, post=False, relu=0):
        y, c = self._out(), self._out(torch.uint8)
        d, io, (b, sc, sh) = ctypes.byref(self.d), self.io(True, True), self._vecs(post)
        assert self.L.slfp_conv2d_res_codes_supported(d, ctypes.byref(io), 1, relu) == 1, self.row
        self.lib.check(self.L.slfp_conv2d_fwd_res_codes(d, ctypes.byref(io), x.ptr(), self.blob.data_ptr(), b, sc, sh, relu, res.ptr(), y.ptr(), c.ptr(),
                                                        None, _stream()))
        return self._done(y, c)

    def slice_(self, x, post=False, relu=0):
        """into the upper half of a tensor twice as wide: returns (the slice, the lower half)"""
        n, ho, wo, co = self.out_shape
        wide = _Arena((n, ho, wo, 2 * co), torch.uint8, self.dev, 0xA5)
        d, io, (b, sc, sh) = ctypes.byref(self.d), self.io(True, True), self._vecs(post)
        assert self.L.slfp_conv2d_codes_slice_supported(d, ctypes.byref(io), 1, relu, 2 * co) == 1, self.row
        self.lib.check(self.L.slfp_conv2d_fwd_codes_slice(d, ctypes.byref(io), x.ptr(), self.blob.data_ptr(), b, sc, sh, relu, wide.ptr() + co, 2 * co,
                                                          None, _stream()))
        self._done(wide)
        return wide.t[..., co:], wide.t[..., :co]

    # ---- checks
    def check_oracle(self, y, what):
        """float32 NHWC output of conv + bias on the clean input: NaN-free (nothing past a tensor's end fed it), within the bars"""
        assert not bool(torch.isnan(y).any()), (self.row, what, "NaN in the output of clean input: a read outside the tensor")
        got = y.permute(0, 3, 1, 2).contiguous().cpu().numpy()
        emax, el2 = rel_errors(got, self.ref)
        frac = elem_exceed_frac(got, self.ref)
        print(f"{self.row.name}: {what} {self.kern} max-rel {emax:.3e} l2 {el2:.3e} elem-frac {frac:.4f}")
        assert emax <= _tol(self.kern) and el2 <= _tol(self.kern), (self.row, what, emax, el2)
        assert got.size >= ELEM_MIN
        assert frac <= elem_frac_bar(self.kern), (self.row, what, frac)

    def check_nan_placement(self, y, what):
        isn = torch.isnan(y).cpu().numpy()
        want = np.broadcast_to(self.nan_px[..., None], isn.shape)
        if not np.array_equal(isn, want):
            extra = np.argwhere(isn.all(-1) & ~self.nan_px)[:6].tolist()
            missing = np.argwhere(~isn.all(-1) & self.nan_px)[:6].tolist()
            raise AssertionError((self.row, what, f"{int(isn.sum())} NaN outputs, {int(want.sum())} expected; NaN pixels that sample no NaN "
                                  f"(image, row, column): {extra}; pixels that should be NaN in all channels and are not: {missing}"))
        assert bool(torch.isfinite(y[~torch.from_numpy(self.nan_px).to(y.device)]).all()), (self.row, what)

    def want_res(self, relu):
        want = torch.add(self.post[0], self.res.t)
        return torch.relu(want) if relu else want


def _layer(lib, row, dev):
    key = desc_key(row)
    if key not in _LAYERS:
        _LAYERS[key] = _Layer(lib, row, dev)
    return _LAYERS[key]


def _bits(t):
    return t.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _codes_equal(got, want_f32, lay, what):
    want = lay.encode(want_f32, KA_NEXT)
    bad = int((got != want).sum())
    assert bad == 0, (lay.row, what, bad, got.numel())


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_pw_variant(lib, dev, row):
    L = lib.load()
    try:
        lay = _layer(lib, row, dev)   # (leaves the switches unset)
        set_switches(L, row.env)
        got_v = lay.variant(row.iface)
        assert got_v == row.variant, (row, got_v)
        print(f"{row.name}: {row.iface} -> {got_v}")
        ok_px = torch.from_numpy(~lay.nan_px).to(dev)
        i = row.iface

        if i == "f32":
            y = lay.f32(lay.x)
            lay.check_oracle(y, row.variant)
            assert same_bits(y.cpu().numpy(), lay.base.cpu().numpy()), (row, "differs from the unforced launch")
            y_nan = lay.f32(lay.x_nan)
            lay.check_nan_placement(y_nan, row.variant)
            assert same_bits(y_nan.cpu().numpy(), lay.base_nan.cpu().numpy()), (row, "NaN input: differs from the unforced launch")
            for relu in (0, 1):
                assert _same(lay.f32(lay.x, post=True, relu=relu), lay.post[relu]), (row, relu, "post-op launch")
            assert _same(lay.f32(lay.x), y), (row, "run to run")
        elif i == "cin":
            y = lay.codes(lay.xc, False)
            lay.check_oracle(y, row.variant)
            assert _same(y, lay.base), (row, "codes in differs from float32 in")
            for relu in (0, 1):
                assert _same(lay.codes(lay.xc, False, post=True, relu=relu), lay.post[relu]), (row, relu, "post-op launch")
            assert _same(lay.codes(lay.xc, False), y), (row, "run to run")
        elif i in ("entry", "cout", "slice"):
            def run(**kw):
                if i == "entry":
                    return lay.entry(lay.x, **kw)
                if i == "cout":
                    return lay.codes(lay.xc, True, **kw)
                c, below = lay.slice_(lay.xc, **kw)
                assert bool((below == 0xA5).all()), (row, "outside the slice")
                return c
            c = run()
            _codes_equal(c, lay.base, lay, "codes of conv + bias")        # base is held to the oracle
            for relu in (1, 0):
                _codes_equal(run(post=True, relu=relu), lay.post[relu], lay, f"post-op, relu {relu}")
            if i == "entry":   # NaN input: every pixel that samples no NaN keeps the codes of the float32 launch
                c_nan = lay.entry(lay.x_nan)
                want = lay.encode(lay.base_nan, KA_NEXT)
                assert torch.equal(c_nan[ok_px], want[ok_px]), (row, "NaN input reaches pixels that sample none")
            assert torch.equal(run(), c), (row, "run to run")
        elif i in ("res", "cres"):
            xin, xc = (lay.xc, True) if i == "cres" else (lay.x, False)
            y0 = lay.resid(xin, xc, lay.res0)                              # + 0: the plain result
            lay.check_oracle(y0, row.variant)
            for relu in (0, 1):
                y = lay.resid(xin, xc, lay.res, post=True, relu=relu)
                assert not bool(torch.isnan(y).any()), (row, relu)
                assert torch.equal(y, lay.want_res(relu)), (row, relu, int((y != lay.want_res(relu)).sum()))
            if i == "res":
                lay.check_nan_placement(lay.resid(lay.x_nan, False, lay.res, post=True, relu=0), row.variant)
            assert _same(lay.resid(xin, xc, lay.res, post=True, relu=1), y), (row, "run to run")
        else:
            assert i == "cdual"
            y0, c0 = lay.dual(lay.xc, lay.res0)
            lay.check_oracle(y0, row.variant)
            _codes_equal(c0, y0, lay, "codes of the plain result")
            for relu in (0, 1):
                y, c = lay.dual(lay.xc, lay.res, post=True, relu=relu)
                assert torch.equal(y, lay.want_res(relu)), (row, relu, int((y != lay.want_res(relu)).sum()))
                _codes_equal(c, y, lay, f"second output, relu {relu}")
            y2, c2 = lay.dual(lay.xc, lay.res, post=True, relu=1)
            assert _same(y2, y) and torch.equal(c2, c), (row, "run to run")
        RAN.add(got_v)
    finally:
        set_switches(L, None)


def test_zz_every_variant_of_the_table_ran():
    """Closes the file: what the row tests launched, by the reporter's own account, is the table's set of variants."""
    assert RAN == {r.variant for r in ROWS}, RAN ^ {r.variant for r in ROWS}
