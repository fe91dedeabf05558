"""GPU (MI355X): image stems that read uint8 pixels (slfp_conv2d_fwd_u8) at the rows of tests/_image_u8_cases.py.

Each row makes two passes: (a) the normalisation table of the ImageNet constants at Ka = 0.1, over bytes in which every value occurs
in every channel and 0 / 255 alternate along the borders (a padded tap read as table[c][0] instead of the operand +0 shows);
(b) a synthetic table with the quantizer's special values, a NaN and both infinities among its entries.  The reference is the same
interface's float32 entry point (slfp_conv2d_fwd_post / slfp_conv2d_fwd_codes_ws) on x32 = P[c, x] expanded by numpy on the host:
outputs must be BYTE-EQUAL (a NaN equals a NaN).  The fixed/tab rows are also held to the CPU restatement slfp_oracle_conv_f32 bit for
bit, which ties the byte path to the oracle independently of the float32 kernels.  The byte batch is a view at byte offset 1 of a
larger allocation, outputs and the workspace lie between guard bands, and every call is made twice.

Then slfp_image_u8_expand_f32 against numpy, and fusion.link_image_u8 on small module stacks."""
import ctypes

import numpy as np
import pytest
import torch

from _image_u8_cases import (IMAGENET_MEAN, IMAGENET_STD, KA_NORM, ROWS, expand_np, io_of, norm_table, pixels, synth_table, u8_instance,
                             u8_supported)
from _stem_variants import KA, KA_NEXT, KW, LAYEROUT, RELU, geom_key, make_desc, make_inputs, out_hw, set_switches
from conftest import same_bits
from oracle import slfp_oracle as so

pytestmark = pytest.mark.gpu

GUARD = 4096
_GEOMS, _BLOBS = {}, {}


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
    """A tensor as a view into a byte buffer of 0xA5 with GUARD bytes in front of and behind it; off: extra bytes in front (1: the
    tensor starts at an odd address)."""

    def __init__(self, shape, dtype, dev, src=None, off=0):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.nbytes, self.off = n, off
        self.buf = torch.full((2 * GUARD + off + n + (-(n + off)) % 16,), 0xA5, dtype=torch.uint8, device=dev)
        self.t = self.buf[GUARD + off:GUARD + off + n].view(dtype).view(shape)
        assert self.t.data_ptr() % 16 == off
        if src is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(src)))

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        return bool((self.buf[:GUARD + self.off] == 0xA5).all()) and bool((self.buf[GUARD + self.off + self.nbytes:] == 0xA5).all())


class _Geom:
    """Pixels, weights and per-channel vectors of one geometry, on the host and the device: built once, shared, never written again."""

    def __init__(self, row, dev):
        _, _, self.w_np, self.bias_np, self.scale_np, self.shift_np = make_inputs(row)
        self.x_np = pixels(row)
        self.x = _Arena(self.x_np.shape, torch.uint8, dev, self.x_np, off=1)     # byte offset 1 inside a larger allocation
        self.w = _Arena(self.w_np.shape, torch.float32, dev, self.w_np)
        self.bias = _Arena((row.c_out,), torch.float32, dev, self.bias_np)
        self.scale = _Arena((row.c_out,), torch.float32, dev, self.scale_np)
        self.shift = _Arena((row.c_out,), torch.float32, dev, self.shift_np)
        self.tables = {}   # pass -> (host table, device table, host x32, device x32)


def _geom(row, dev):
    k = geom_key(row)
    if k not in _GEOMS:
        _GEOMS[k] = _Geom(row, dev)
    return _GEOMS[k]


def _pass(g, row, which, dev):
    if which not in g.tables:
        t = norm_table(row.c_in) if which == "a" else synth_table(row, KA)
        x32 = expand_np(g.x_np, t)
        g.tables[which] = (t, _Arena(t.shape, torch.float32, dev, t), x32, _Arena(x32.shape, torch.float32, dev, x32))
    return g.tables[which]


def _blob(lib, row, d, g, dev):
    L = lib.load()
    k = (geom_key(row), row.stride, row.qbits, L.slfp_conv2d_kernel_name(ctypes.byref(d)).decode())
    if k not in _BLOBS:
        n = L.slfp_conv2d_wprep_bytes(ctypes.byref(d))
        b = _Arena((n,), torch.uint8, dev)
        lib.check(L.slfp_conv2d_prepare_weights(ctypes.byref(d), g.w.ptr(), b.ptr(), None, _stream()))
        _BLOBS[k] = b
    return _BLOBS[k]


def _run(lib, row, d, g, blob, dev, x_ptr, pix_ptr=None):
    """One launch of the row's layer: the byte entry point (pix_ptr given) or the float32 entry point of the same interface."""
    L = lib.load()
    codes_out = row.iface == "cout"
    y = _Arena((row.n,) + out_hw(row) + (row.c_out,), torch.uint8 if codes_out else torch.float32, dev)
    nws = L.slfp_conv2d_workspace_bytes(ctypes.byref(d))
    ws = _Arena((nws,), torch.uint8, dev) if nws else None
    wsp = ws.ptr() if ws is not None else None
    dp = ctypes.byref(d)
    bias = g.bias.ptr() if row.bias else None
    sc, sh = (g.scale.ptr(), g.shift.ptr()) if row.post else (None, None)
    io = io_of(lib, row, KA_NEXT)
    iop = ctypes.byref(io) if io is not None else None
    if pix_ptr is not None:
        lib.check(L.slfp_conv2d_fwd_u8(dp, iop, x_ptr, pix_ptr, blob.ptr(), bias, sc, sh, row.flags, y.ptr(), wsp, _stream()))
    elif codes_out:
        lib.check(L.slfp_conv2d_fwd_codes_ws(dp, iop, x_ptr, blob.ptr(), bias, sc, sh, row.flags, y.ptr(), wsp, _stream()))
    else:
        lib.check(L.slfp_conv2d_fwd_post(dp, x_ptr, blob.ptr(), bias, sc, sh, row.flags, y.ptr(), None, wsp, _stream()))
    torch.cuda.synchronize()
    assert y.guards_intact(), (row, "guard band of the output written")
    assert ws is None or ws.guards_intact(), (row, "guard band of the workspace written")
    out = y.t.cpu().numpy()
    return out if codes_out else out.view(np.uint32)


def _first_diff(got, want):
    bad = np.argwhere(got != want)
    at = tuple(bad[0]) if len(bad) else None
    return f"{len(bad)} of {got.size} differ; first at (image, row, column, channel) {at}: got {got[at]:#x}, want {want[at]:#x}" if at else "NaN placement"


def _restatement(row, g, x32, ka):
    """the CPU restatement of the float32 stems' arithmetic on the expanded tensor; code rows: its float32 value coded on the host"""
    codes_out = row.iface == "cout"
    t = so.conv_f32(x32, g.w_np, g.bias_np if row.bias else None, row.stride, row.pad, row.dil, row.groups, ka, KW, row.qbits, 0,
                    g.scale_np if row.post else None, g.shift_np if row.post else None, bool(row.flags & LAYEROUT),
                    bool(row.flags & RELU) and not codes_out)
    if not codes_out:
        return t.view(np.uint32)
    isn = np.isnan(t)
    if row.flags & RELU:   # folded into the quantizer
        with np.errstate(invalid="ignore"):
            t = np.where(isn, np.float32(0.0), np.maximum(t, np.float32(0.0))).astype(np.float32)
    c = so.encode(t, np.float32(KA_NEXT), (so.FMT_ACT8 if row.y_qbits == 8 else so.FMT_SFP7) | so.FMT_EXT)
    c[isn] = 0x00   # the stems' code of a NaN ("NaN in front of a folded ReLU")
    return c


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_row_equals_the_float32_entry_point_on_the_expanded_tensor(lib, dev, row):
    L = lib.load()
    try:
        set_switches(L, None)
        g = _geom(row, dev)
        codes_out = row.iface == "cout"
        equal = np.array_equal if codes_out else same_bits
        if row.n * row.h * row.w >= 256:   # every byte value in every channel, on the pixels behind the border
            assert all(len(np.unique(g.x_np[:, 1:-1, 1:-1, c])) == 256 for c in range(row.c_in)), row
        assert (g.x_np[:, 0, 0, :] == 0).all() and (g.x_np[:, -1, -1, :] == 255).all() and set(np.unique(g.x_np[:, 0, :, :])) == {0, 255}
        for which, ka in (("a", KA_NORM), ("b", KA)):
            set_switches(L, None)
            d = make_desc(lib, row, ka, KW)
            blob = _blob(lib, row, d, g, dev)
            table, table_dev, x32, x32_dev = _pass(g, row, which, dev)
            if which == "a":
                assert np.abs(table / np.float32(ka)).max() > 15.5 and table.min() < 0 < table.max()   # both clamps are passed
            else:   # the NaN and both infinities are drawn by planted pixels
                assert np.isnan(x32).any() and np.isposinf(x32).any() and np.isneginf(x32).any(), row
            set_switches(L, row.env)
            assert u8_supported(lib, d, row, KA_NEXT) == 1 and u8_instance(lib, d, row, KA_NEXT) == row.variant, row
            y = _run(lib, row, d, g, blob, dev, g.x.ptr(), table_dev.ptr())
            ref = _run(lib, row, d, g, blob, dev, x32_dev.ptr())
            assert equal(y, ref), (row, which, _first_diff(y, ref))
            if not codes_out and which == "a":
                assert not np.isnan(y.view(np.float32)).any(), (row, "NaN from finite pixels: a read outside the tensor")
            if row.variant.startswith("stem/fixed/tab"):   # ... and the CPU restatement, independently of the float32 kernels
                want = _restatement(row, g, x32, ka)
                assert equal(y, want), (row, which, "restatement", _first_diff(y, want))
            y2 = _run(lib, row, d, g, blob, dev, g.x.ptr(), table_dev.ptr())
            assert np.array_equal(y2, y), (row, which, "run to run")
            assert g.x.guards_intact() and table_dev.guards_intact()
    finally:
        set_switches(L, None)


@pytest.mark.parametrize("c", (1, 3, 4))
@pytest.mark.parametrize("npx", (1, 15, 3465))
def test_expand_equals_numpy(lib, dev, c, npx):
    L = lib.load()
    rng = np.random.default_rng(31 * c + npx)
    table = (rng.standard_normal((c, 256)) * 3.0).astype(np.float32)
    table[0, 5], table[c - 1, 200] = np.float32("nan"), np.float32("-inf")
    x = rng.integers(0, 256, (npx, c), dtype=np.uint8)
    x[0, 0] = 5
    xa, ta = _Arena(x.shape, torch.uint8, dev, x, off=1), _Arena(table.shape, torch.float32, dev, table)
    for _ in range(2):
        ya = _Arena((npx, c), torch.float32, dev)
        lib.check(L.slfp_image_u8_expand_f32(xa.ptr(), ta.ptr(), ya.t.data_ptr(), npx, c, _stream()))
        torch.cuda.synchronize()
        assert ya.guards_intact()
        assert np.array_equal(ya.t.cpu().numpy().view(np.uint32), expand_np(x, table).view(np.uint32))
    assert L.slfp_image_u8_expand_f32(xa.ptr(), ta.ptr(), ya.ptr(), npx, 5, _stream()) == lib.ERR_SHAPE
    assert L.slfp_image_u8_expand_f32(xa.ptr(), ta.ptr(), ya.ptr() + 4, npx, c, _stream()) == lib.ERR_ALIGNMENT
    assert L.slfp_image_u8_expand_f32(None, ta.ptr(), ya.ptr(), npx, c, _stream()) == lib.ERR_BAD_ARG


# ---------------------------------------------------------------------------------------------------------------- modules
def _i32(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _bytes(dev, n, h, w, c=3, seed=5):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (n, c, h, w), dtype=torch.uint8, generator=g)
    x[:, :, 0, :], x[:, :, -1, :], x[:, :, :, 0], x[:, :, :, -1] = 0, 255, 255, 0
    return x.to(dev).contiguous(memory_format=torch.channels_last)


def _table(dev=None):
    from cnns_slfp_quantization_amd import image_u8
    t = image_u8.pixel_table(IMAGENET_MEAN, IMAGENET_STD)
    return t if dev is None else t.to(dev)


def _bn(c, gen):
    bn = torch.nn.BatchNorm2d(c)
    with torch.no_grad():
        bn.weight.copy_(0.5 + torch.rand(c, generator=gen)); bn.bias.copy_(torch.randn(c, generator=gen) * 0.1)
        bn.running_mean.copy_(torch.randn(c, generator=gen) * 0.1); bn.running_var.copy_(0.5 + torch.rand(c, generator=gen))
    return bn


def _mobilenet_head(dev, stride=2):
    """stem (3x3, 3 -> 32) + depthwise + pointwise, each with BatchNorm and ReLU"""
    import utils.conv2d_func as cf
    gen = torch.Generator().manual_seed(11)
    C = cf.conv2d_Q(q_bit=8, Kw=0.02, Ka=0.3)
    m = torch.nn.Sequential(C(3, 32, 3, 0.02, 0.3, stride, 1), _bn(32, gen), torch.nn.ReLU(),
                            C(32, 32, 3, 0.05, 0.4, 1, 1, groups=32), _bn(32, gen), torch.nn.ReLU(),
                            C(32, 64, 1, 0.03, 0.5, 1, 0), _bn(64, gen), torch.nn.ReLU())
    return m.to(dev).eval().to(memory_format=torch.channels_last)


def test_mobilenet_head_reads_bytes_and_writes_codes(dev):
    from cnns_slfp_quantization_amd import fusion, image_u8, streams
    m, x, table = _mobilenet_head(dev), _bytes(dev, 3, 33, 36), _table()
    with torch.no_grad():
        x32 = image_u8.expand(x, table.to(dev))
        assert torch.equal(x32.cpu(), table[torch.arange(3).view(1, 3, 1, 1), x.cpu().long()])
        y0 = m(x32)
        assert fusion.fuse_bn_relu(m) == 3
        assert fusion.link_image_u8(m, table, x) == 1 and fusion.link_image_u8(m, table, x) == 0
        y32 = m(x32)
        y1 = m(x)
        assert torch.equal(_i32(y1), _i32(y32))
        assert m[0]._last_kernel == "stem_nhwc+u8:stem/fixed/tab/u8/f32", m[0]._last_kernel
        links = fusion.link_codes_traced(m, x)
        assert links >= 1 and m[0]._code_out is not None      # the stem writes the depthwise layer's codes
        y2 = m(x)
        assert m[0]._last_kernel == "stem_nhwc+codes_out+u8:stem/fixed/tab/u8/yc", m[0]._last_kernel
        assert "+codes_in" in m[3]._last_kernel
        assert torch.equal(_i32(y2), _i32(y1))
        # float32 input into the linked stem: unchanged
        assert torch.equal(_i32(m(x32)), _i32(y1)) and m[0]._last_kernel == "stem_nhwc+codes_out"
        # input_q of the byte-input stem is the float32 path's
        m(x)
        q_u8 = m[0].input_q.clone()
        m(x32)
        assert torch.equal(_i32(q_u8), _i32(m[0].input_q))
        # image groups on two streams: the same bits
        assert torch.equal(_i32(streams.forward_image_groups(m, x, groups=2)), _i32(y1))
        # anything but dense NHWC bytes on the device with the table's channel count is a TypeError
        for bad in (x.contiguous(), x.cpu(), x[:, :2].contiguous(memory_format=torch.channels_last)):
            with pytest.raises(TypeError):
                m(bad)
        assert fusion.unlink_codes(m) == links and fusion.unlink_image_u8(m) == 1 and fusion.unlink_image_u8(m) == 0
        fusion.unfuse(m)
        assert torch.equal(_i32(m(x32)), _i32(y0))
    # the unlinked model is back to what it did before: uint8 is codes again (a float32-only first layer decodes them)
    assert m[0]._image_table is None


def test_large_kernel_stem_after_link_stem(dev, monkeypatch):
    import utils.conv2d_func as cf
    from cnns_slfp_quantization_amd import fusion, image_u8, conv2d_func
    C = cf.conv2d_Q_bias(q_bit=8, Kw=0.02, Ka=0.3)
    torch.manual_seed(3)
    m = torch.nn.Sequential(C(3, 64, 7, 0.02, 0.3, 2, 3), torch.nn.ReLU(inplace=True), torch.nn.MaxPool2d(3, 2, 1),
                            C(64, 64, 1, 0.03, 0.6, 1, 0)).to(dev).eval().to(memory_format=torch.channels_last)
    x, table = _bytes(dev, 2, 20, 70), _table()
    with torch.no_grad():
        m[0].weight.mul_(0.5)
        x32 = image_u8.expand(x, table.to(dev))
        y0 = m(x32)
        assert fusion.link_stem(m, x32) == 1
        assert fusion.link_image_u8(m, table, x) == 1
        if "rows" in conv2d_func.IMAGE_U8_OFF:   # the measured default keeps this family on the expansion: same bits
            assert torch.equal(_i32(m(x)), _i32(y0)) and m[0]._last_kernel.startswith("u8-expand+stem_mfma_f16x1+codes_out"), m[0]._last_kernel
        monkeypatch.setattr(conv2d_func, "IMAGE_U8_OFF", set())   # the kernel itself
        y1 = m(x)
        assert torch.equal(_i32(y1), _i32(y0))
        assert m[0]._last_kernel.startswith("stem_mfma_f16x1+codes_out+u8:rows/nt4/act8/u8/yc"), m[0]._last_kernel
        assert "+codes_in" in m[3]._last_kernel
        assert fusion.unlink_image_u8(m) == 1 and fusion.unlink_stem(m) == 1
        assert torch.equal(_i32(m(x32)), _i32(y0))


def test_a_stem_without_a_byte_form_expands(dev):
    """stride 3: the generic k_stem on the float32 interface; the linked module expands the bytes and runs it"""
    from cnns_slfp_quantization_amd import fusion, image_u8, _lib
    import utils.conv2d_func as cf
    prev = cf.options.mfma_passes
    try:
        cf.options.mfma_passes = _lib.MFMA_F16X3     # keeps the 3x3 layer off the fp16 stems: k_stem
        m, x, table = _mobilenet_head(dev, stride=3), _bytes(dev, 2, 33, 36), _table()
        with torch.no_grad():
            x32 = image_u8.expand(x, table.to(dev))
            y0 = m(x32)
            assert fusion.link_image_u8(m, table, x) == 1
            assert torch.equal(_i32(m(x)), _i32(y0))
            assert m[0]._last_kernel == "u8-expand+stem_nhwc", m[0]._last_kernel
            assert fusion.unlink_image_u8(m) == 1
    finally:
        cf.options.mfma_passes = prev


def test_default_rule_can_take_a_family_out(dev, monkeypatch):
    """conv2d_func.IMAGE_U8_OFF (the rule of DESIGN section 12 in Python): a family listed there expands instead; the same bits"""
    from cnns_slfp_quantization_amd import fusion, conv2d_func
    m, x, table = _mobilenet_head(dev), _bytes(dev, 2, 33, 36), _table()
    with torch.no_grad():
        monkeypatch.setattr(conv2d_func, "IMAGE_U8_OFF", set())
        assert fusion.link_image_u8(m, table, x) == 1
        y = m(x)
        assert "+u8:" in m[0]._last_kernel
        monkeypatch.setattr(conv2d_func, "IMAGE_U8_OFF", {"stem"})
        assert torch.equal(_i32(m(x)), _i32(y)) and m[0]._last_kernel.startswith("u8-expand+"), m[0]._last_kernel


def test_training_on_bytes_gives_the_expanded_batch_gradients(dev):
    from cnns_slfp_quantization_amd import fusion, image_u8
    import utils.conv2d_func as cf
    prev = cf.options.backward
    try:
        cf.options.backward = "hip_all"
        m, x, table = _mobilenet_head(dev), _bytes(dev, 2, 33, 36), _table()
        with torch.no_grad():
            assert fusion.link_image_u8(m, table, x) == 1
        stem = m[0].train()
        x32 = image_u8.expand(x, table.to(dev))
        grads = []
        for inp in (x, x32):
            stem.zero_grad()
            out = stem(inp)
            out.backward(torch.ones_like(out) * 0.25)
            grads.append(stem.weight.grad.clone())
        assert stem._last_bwd_kernel is not None
        assert torch.equal(_i32(grads[0]), _i32(grads[1])) and float(grads[0].abs().max()) > 0
        stem(x)
        assert stem._last_kernel.startswith("u8-expand+"), stem._last_kernel
    finally:
        cf.options.backward = prev
