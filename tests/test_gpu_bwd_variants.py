"""GPU (MI355X): every backward kernel instance of csrc/conv_bwd.hip at the small ragged shapes of tests/_bwd_variants.py, straight
through the C ABI (slfp_conv2d_bwd_ex / slfp_conv2d_bwd_codes).  slfp_debug_bwd_instance says which instances a row launches; each row
is held

  * to the float64 reference of tests/_bwd_cases.py (torch.nn.grad contractions of the C oracle's quantized operands) by the
    project's bars: elementwise |d| / sum|terms| <= 1e-5 and tensor-relative L2 <= 1e-6 for gx, gw and gb;
  * to the table-encode float32 launch of the same layer, bit for bit: the long form and the codes rows (whose decoded codes are first
    shown to be the oracle's quantize(x) bit for bit);
  * inside guard bands: x, w and gy are views with 4 KiB of NaN (codes: 0x7F) on each side, so a read past an end that feeds the result
    shows in the output of clean input; gx, gw, gb and a workspace of exactly slfp_conv2d_bwd_workspace_bytes_ex bytes have 0xA5 bands
    that must be untouched;
  * on every `need` subset the ABI allows: the outputs asked for equal the full run's, the others keep their fill;
  * (float32 rows) to a NaN placement worked out from the geometry alone: with NaNs and an infinity planted in x, gw is NaN on exactly
    the (channel, tap) elements whose taps sample those pixels and within the bars elsewhere; gx and gb, which never read x, keep
    their bits;
  * to itself: a second launch gives the same bits.
The last test shows that the launches made are the set of instances the launchers can select."""
import ctypes

import numpy as np
import pytest
import torch

import _bwd_variants as V
from _bwd_cases import _errors
from _bwd_variants import KA, ROWS
from oracle import slfp_oracle

pytestmark = pytest.mark.gpu

GUARD = 4096     # bytes on each side of every tensor
NEEDS = ((1, 1, 1), (1, 1, 0), (0, 1, 1), (0, 1, 0), (1, 0, 0))   # (gx, gw, gb): gb is computed together with gw
RAN = set()      # reporter strings (split numbers stripped) of the launches the row tests made
_LAYERS = {}     # layer key -> _Layer


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
    """A tensor as a view into a byte buffer with GUARD bytes in front of and behind it (`off` more bytes in front: a view that is
    4-byte but not 16-byte aligned)."""

    def __init__(self, shape, dtype, dev, fill, src=None, off=0):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.nbytes, self.off = n, off
        if dtype == torch.float32 and fill != fill:   # NaN guards around a float32 input
            self.buf = torch.full(((2 * GUARD + n) // 4,), float("nan"), dtype=torch.float32, device=dev).view(torch.uint8)
            self.fill = None
        else:
            self.buf = torch.full((2 * GUARD + n + off,), fill, dtype=torch.uint8, device=dev)
            self.fill = fill
        assert self.buf.data_ptr() % 16 == 0
        self.t = self.buf[GUARD + off:GUARD + off + n].view(dtype).view(shape)
        if src is not None:
            self.t.copy_(src)

    def ptr(self):
        return self.buf.data_ptr() + GUARD + self.off

    def guards_intact(self):
        return bool((self.buf[:GUARD + self.off] == self.fill).all()) and bool((self.buf[GUARD + self.off + self.nbytes:] == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())


def _nan_in(t, dev):
    return _Arena(t.shape, torch.float32, dev, float("nan"), t)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


class _Layer:
    """One layer of the table: its seeded inputs in guarded arenas (NHWC; x clean and with nan_sites planted), and -- made once, shared
    by the rows of the layer, never written again -- the codes of x and the table-encode float32 launch."""

    def __init__(self, lib, row, dev):
        self.lib, self.L, self.row, self.dev = lib, lib.load(), row, dev
        x, w, gy = V.inputs(row)
        nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()   # noqa: E731
        self.x = _nan_in(nhwc(x).to(dev), dev)
        self.x_nan = _nan_in(nhwc(V.plant(row, x)).to(dev), dev)
        self.w = _nan_in(w.contiguous().to(dev), dev)
        self.gy = _nan_in(nhwc(gy).to(dev), dev)
        self.xq = slfp_oracle.quantize(nhwc(x).numpy(), float(np.float32(KA)), 0 if row.qbits == 8 else 2)
        self._codes, self._base = {}, None

    def codes(self, off):
        """x as the extended codes of QA(x / Ka), `off` bytes past a 16-byte boundary; decode(codes) is the oracle's xq bit for bit."""
        if off not in self._codes:
            lib, L, row = self.lib, self.L, self.row
            fmt = (lib.FMT_ACT8 if row.qbits == 8 else lib.FMT_SFP7) | lib.FMT_EXT
            c = torch.empty(self.x.t.shape, dtype=torch.uint8, device=self.dev)
            lib.check(L.slfp_encode_f32(self.x.ptr(), c.data_ptr(), c.numel(), float(np.float32(KA)), fmt, _stream()))
            back = torch.empty(self.x.t.shape, dtype=torch.float32, device=self.dev)
            lib.check(L.slfp_decode_f32(c.data_ptr(), back.data_ptr(), c.numel(), fmt, _stream()))
            torch.cuda.synchronize()
            assert np.array_equal(back.cpu().numpy().view(np.int32), self.xq.view(np.int32)), "decode(encode(x)) != quantize(x)"
            a = _Arena(c.shape, torch.uint8, self.dev, 0x7F, c, off=off)
            assert a.ptr() % 4 == 0 and a.ptr() % 16 == off
            self._codes[off] = a
        return self._codes[off]

    def launch(self, row, need, x=None):
        """One call of the row's entry point under the switches now set: {name: tensor} of the outputs asked for.  Every output sits
        in a 0xA5 arena, the workspace is exactly the stated size inside one; all bands must be untouched afterwards."""
        lib, L, dev = self.lib, self.L, self.dev
        d = V.make_desc(lib, row)
        r = ctypes.byref(d)
        shapes = {"gx": self.x.t.shape, "gw": self.w.t.shape, "gb": (row.c_out,)}
        outs = {k: _Arena(s, torch.float32, dev, 0xA5) for k, s in shapes.items()}
        nbytes = L.slfp_conv2d_bwd_workspace_bytes_ex(r, row.flags, need[0], need[1])
        ws = _Arena((nbytes,), torch.uint8, dev, 0xA5)
        ptr = lambda k, on: outs[k].ptr() if on else None   # noqa: E731
        if row.operand == "codes":
            xa = self.codes(row.align) if x is None else x
            rc = L.slfp_conv2d_bwd_codes(r, row.flags, xa.ptr(), self.w.ptr(), self.gy.ptr(), ptr("gx", need[0]), ptr("gw", need[1]),
                                         ptr("gb", need[2]), ws.ptr(), _stream())
        else:
            xa = self.x if x is None else x
            rc = L.slfp_conv2d_bwd_ex(r, row.flags, xa.ptr(), self.w.ptr(), self.gy.ptr(), ptr("gx", need[0]), ptr("gw", need[1]),
                                      ptr("gb", need[2]), ws.ptr(), _stream())
        lib.check(rc)
        torch.cuda.synchronize()
        assert ws.guards_intact(), (row.name, need, "workspace", nbytes)
        got = {}
        for (k, a), on in zip(outs.items(), need):
            if on:
                assert a.guards_intact(), (row.name, need, k)
                got[k] = a.t.clone()
            else:
                assert a.untouched(), (row.name, need, k)
        return got

    def base(self):
        """The float32-operand launch on the threshold table (no switch set): what every other form of the layer must equal."""
        if self._base is None:
            row = self.row._replace(operand="f32", env=(), align=0)
            V.set_switches(self.L, None)
            assert "/tab/" in V.instance(self.lib, V.make_desc(self.lib, row), row.flags, 0)
            self._base = self.launch(row, (1, 1, 1))
        return self._base


def _layer(lib, row, dev):
    key = V.layer_key(row)
    if key not in _LAYERS:
        _LAYERS[key] = _Layer(lib, row, dev)
    return _LAYERS[key]


def _nchw(gx):
    return gx.permute(0, 3, 1, 2)


def _check_bars(row, got, refs, what=""):
    for (name, g), ref in zip((("gx", _nchw(got["gx"])), ("gw", got["gw"]), ("gb", got["gb"])), refs):
        assert bool(torch.isfinite(g).all()), (row.name, what, name)
        elem, l2 = _errors(g, ref)
        print(f"{row.name} {what} {name}: elem {elem:.2e} l2 {l2:.2e}")
        assert elem <= 1e-5 and l2 <= 1e-6, (row.name, what, name, elem, l2)


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_bwd_variant(lib, dev, row):
    L = lib.load()
    lay = _layer(lib, row, dev)
    try:
        base = lay.base() if (row.operand == "codes" or row.env) else None
        V.set_switches(L, row.env)
        said = V.instance(lib, V.make_desc(lib, row), row.flags, row.operand == "codes")
        assert V.strip(said) == row.variant, (row.name, said)
        full = lay.launch(row, (1, 1, 1))
        RAN.update(V.strip(said).split("+"))
        _check_bars(row, full, V.reference(row), said)
        if base is not None:   # codes against the float32 operand, the long form against the table: the same sums in the same order
            for k in ("gx", "gw", "gb"):
                assert torch.equal(full[k], base[k]), (row.name, k)
        for need in NEEDS[1:]:
            part = lay.launch(row, need)
            assert set(part) == {k for k, on in zip(("gx", "gw", "gb"), need) if on}
            for k, g in part.items():
                assert torch.equal(g, full[k]), (row.name, need, k)
        again = lay.launch(row, (1, 1, 1))
        for k in ("gx", "gw", "gb"):
            assert _same(again[k], full[k]), (row.name, "second launch", k)
        if row.operand == "f32":
            # NaN and +inf planted in x: the infinity is clamped by the quantizer, a NaN reaches exactly the taps that sample it
            bad = lay.launch(row, (1, 1, 1), x=lay.x_nan)
            assert _same(bad["gx"], full["gx"]) and _same(bad["gb"], full["gb"]), row.name
            mask = V.nan_mask(row)
            gw = bad["gw"].cpu()
            assert torch.equal(torch.isnan(gw), mask), (row.name, int(torch.isnan(gw).sum()), int(mask.sum()))
            r, a = V.reference(row, planted=True)[1]
            elem, l2 = _errors(gw[~mask], (r[~mask], a[~mask]))
            assert elem <= 1e-5 and l2 <= 1e-6, (row.name, "gw beside the NaNs", elem, l2)
    finally:
        V.set_switches(L, None)


def test_zz_every_instance_of_the_table_ran():
    """After the row tests: the reporter strings of the launches made are the set the launchers can select."""
    print(f"\nbackward variants: {len(ROWS)} rows on {len(_LAYERS)} layers")
    want = V.reachable()
    assert not want - RAN, f"instances no launch ran: {sorted(want - RAN)}"
    assert not RAN - want, f"launches outside the reachable set: {sorted(RAN - want)}"
