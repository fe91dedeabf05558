"""GPU (MI355X): every kernel family on non-square geometry against the CPU oracle.

Every other parity test builds its input as [N, H, H, C] with one scalar each for kernel size, stride and padding, where
`row * W + col` and `row * H + col` are the same number.  The rows of tests/_aniso_cases.py have H != W and, where the family
takes them, kh != kw, pad_h != pad_w, stride_h != stride_w, dil_h != dil_w; tests/test_aniso_host.py pins where they
dispatch.  Bars: tests/_bars.py, as everywhere else."""
import ctypes

import numpy as np
import pytest
import torch

import _aniso_cases as ac
from _bars import ELEM_MIN, elem_frac_bar, tol as _tol
from conftest import elem_exceed_frac, note_elem_stats, rel_errors, same_bits
from oracle import slfp_oracle as so

pytestmark = pytest.mark.gpu

N_TABLE = 3


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


def _raw_conv(lib, dev, c, x, w_oihw, bias, qbits, passes, nchw=False):
    """Straight through the C ABI (no torch module).  nchw=False: x is [N, H, W, C], slfp_conv2d_fwd, NHWC out.  nchw=True:
    x is [N, C, H, W], slfp_conv2d_fwd_post without an epilogue and with both layouts NCHW: the in-ABI transposes and the
    workspace carve-up behind them.  Returns the output as [N, O, Ho, Wo] and the kernel name."""
    L = lib.load()
    N = x.shape[0]
    assert tuple(x.shape) == ((N, c.C, c.H, c.W) if nchw else (N, c.H, c.W, c.C)) and tuple(w_oihw.shape) == (c.O, c.C // c.g, c.kh, c.kw)
    lay = lib.LAYOUT_NCHW if nchw else lib.LAYOUT_NHWC
    d = ac.desc(lib, c, N, qbits, passes, lay, lay)
    ho, wo = ctypes.c_int64(), ctypes.c_int64()
    lib.check(L.slfp_conv2d_out_shape(ctypes.byref(d), ctypes.byref(ho), ctypes.byref(wo)))
    assert (ho.value, wo.value) == ac.out_hw(c)
    blob = torch.empty(L.slfp_conv2d_wprep_bytes(ctypes.byref(d)), dtype=torch.uint8, device=dev)
    lib.check(L.slfp_conv2d_prepare_weights(ctypes.byref(d), w_oihw.data_ptr(), blob.data_ptr(), None, _stream()))
    shape = (N, c.O, ho.value, wo.value) if nchw else (N, ho.value, wo.value, c.O)
    y = torch.full(shape, float("nan"), dtype=torch.float32, device=dev)   # an element nobody writes fails the comparison
    ws_bytes = L.slfp_conv2d_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
    bp = bias.data_ptr() if bias is not None else None
    wsp = ws.data_ptr() if ws is not None else None
    if nchw:
        lib.check(L.slfp_conv2d_fwd_post(ctypes.byref(d), x.data_ptr(), blob.data_ptr(), bp, None, None, 0, y.data_ptr(), None, wsp, _stream()))
    else:
        lib.check(L.slfp_conv2d_fwd(ctypes.byref(d), x.data_ptr(), blob.data_ptr(), bp, y.data_ptr(), None, wsp, _stream()))
    return (y if nchw else y.permute(0, 3, 1, 2)).contiguous(), L.slfp_conv2d_kernel_name(ctypes.byref(d)).decode()


_INPUTS = {}
_REFS = {}


def _inputs(c, N, seed, bias):
    """Seeded operands of a case, NCHW / OIHW on the host: post-ReLU-like except for image stems.  Made once per case."""
    key = (c[1:14], N, seed, bias)
    if key not in _INPUTS:
        gen = torch.Generator(device="cpu").manual_seed(seed)
        w = torch.randn((c.O, c.C // c.g, c.kh, c.kw), generator=gen) * (5.0 * ac.KW)
        b = torch.randn(c.O, generator=gen) * 0.5 if bias else None
        x = torch.randn((N, c.C, c.H, c.W), generator=gen) * (6.0 * ac.KA)
        x = torch.relu(x) if c.C > 4 else x
        _INPUTS[key] = (x, w, b)
    return _INPUTS[key]


def _reference(c, N, seed, bias, qbits):
    """The oracle's output for a case: computed once, shared by the operand modes and the NCHW run, never written to."""
    key = (c[1:14], N, seed, bias, qbits)
    if key not in _REFS:
        x, w, b = _inputs(c, N, seed, bias)
        ref = so.conv2d(x.numpy(), w.numpy(), None if b is None else b.numpy(), (c.sh, c.sw), (c.ph, c.pw), (c.dh, c.dw), c.g,
                        ac.KA, ac.KW, qbits)
        ref.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def _check_against_oracle(lib, dev, c, N, qbits, passes, seed, bias, nchw=False):
    x, w, b = _inputs(c, N, seed, bias)
    ref = _reference(c, N, seed, bias, qbits)
    xd = (x if nchw else x.permute(0, 2, 3, 1)).contiguous().to(dev)
    got, kern = _raw_conv(lib, dev, c, xd, w.to(dev), None if b is None else b.to(dev), qbits, passes, nchw)
    got = got.cpu().numpy()
    assert got.shape == ref.shape, (kern, c, got.shape, ref.shape)
    tol = _tol(kern)
    emax, el2 = rel_errors(got, ref)
    assert emax <= tol and el2 <= tol, (kern, "nchw" if nchw else "nhwc", c, (qbits, passes), emax, el2)
    frac = elem_exceed_frac(got, ref)
    note_elem_stats(kern, got, ref)
    if got.size >= ELEM_MIN:
        assert frac <= elem_frac_bar(kern), (kern, c, (qbits, passes), frac)
    return kern


def _family(fam):
    return [(c, tw, i) for c, tw, i in ac.all_cases() if c.fam == fam]


@pytest.mark.parametrize("qbits, passes", ac.MODES)
@pytest.mark.parametrize("fam", ac.FAMILIES)
def test_table_rows_and_twins_vs_oracle(lib, dev, fam, qbits, passes):
    """Every row of the table and its transposed twin, float32 NHWC interface, the kernel the host test pins."""
    mode = ac.MODES.index((qbits, passes))
    rows = _family(fam)
    assert rows
    for c, tw, i in rows:
        kern = _check_against_oracle(lib, dev, c, N_TABLE, qbits, passes, seed=9000 + 2 * i + tw, bias=bool(i & 1))
        assert kern == c.names[mode], (c, kern)


@pytest.mark.parametrize("fam", ac.FAMILIES)
def test_table_rows_nchw_interface_vs_oracle(lib, dev, fam):
    """Each row and twin once through slfp_conv2d_fwd_post with x_layout = y_layout = NCHW (the operand mode cycles with the
    row): the transposes inside the ABI with H != W, and the workspace shared between them and the kernel's own scratch."""
    for c, tw, i in _family(fam):
        mode = (i + tw) % len(ac.MODES)
        qbits, passes = ac.MODES[mode]
        kern = _check_against_oracle(lib, dev, c, N_TABLE, qbits, passes, seed=9000 + 2 * i + tw, bias=bool(i & 1), nchw=True)
        assert kern == c.names[mode], (c, kern)


def test_randomized_rectangular_geometries_vs_oracle(lib, dev):
    """tests/test_gpu_parity.py's random sweep with H and W (and, where the family takes a pair, kernel sides and paddings)
    drawn independently: _aniso_cases.sweep_draws, whose dispatch and skip count tests/test_aniso_host.py checks."""
    kinds = {}
    skipped = 0
    draws = ac.sweep_draws()
    for i, (c, N, qbits, passes, bias) in enumerate(draws):
        if ac.degenerate(c):
            skipped += 1
            continue
        kern = _check_against_oracle(lib, dev, c, N, qbits, passes, seed=14000 + i, bias=bias)
        kinds[kern] = kinds.get(kern, 0) + 1
    assert skipped <= len(draws) // 20
    for fam in ac.SWEEP_FAMILIES:   # the sweep must actually reach the families it is meant to cover
        assert kinds.get(fam, 0) > 0, (fam, kinds)


# one table row per family, through the drop-in modules with tuple arguments
MODULE_ROWS = [4, 12, 18, 32, 37]   # dw rows kernel 29x14 s2; 1x1 s2 at 23x5; dense 3x5 p(1,2); stem 7x5 s2 p(3,1); direct g3 d(2,3)


@pytest.mark.parametrize("row", MODULE_ROWS)
@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
def test_modules_with_tuple_arguments_vs_oracle(dev, row, layout):
    """conv2d_Q(...) and conv2d_Q_bias(...) built with tuple kernel_size / stride / padding / dilation (conv2d_func._conv_desc
    and the plan key), NCHW and channels_last inputs: output, input_q and weight_q against the oracle."""
    import utils.conv2d_func as cf
    c = ac.ROWS[row]
    for qbits, with_bias in ((8, False), (8, True), (7, True)):
        x, w, b = _inputs(c, 2, 9500 + row, with_bias)
        factory = cf.conv2d_Q_bias if with_bias else cf.conv2d_Q
        Conv = factory(q_bit=qbits, Kw=np.float64(ac.KW), Ka=np.float64(ac.KA))
        m = Conv(c.C, c.O, (c.kh, c.kw), np.float64(ac.KW), np.float64(ac.KA), (c.sh, c.sw), (c.ph, c.pw), (c.dh, c.dw),
                 groups=c.g, bias=with_bias).to(dev).eval()
        xd = x.to(dev)
        if layout == "channels_last":
            xd = xd.contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            m.weight.copy_(w)
            if with_bias:
                m.bias.copy_(b)
            y = m(xd)
            xq, wq = m.input_q.cpu().numpy(), m.weight_q.cpu().numpy()
        assert y.is_contiguous(memory_format=torch.channels_last if layout == "channels_last" else torch.contiguous_format)
        ref, xqo, wqo = so.conv2d(x.numpy(), w.numpy(), None if b is None else b.numpy(), (c.sh, c.sw), (c.ph, c.pw), (c.dh, c.dw),
                                  c.g, ac.KA, ac.KW, qbits, want_q=True)
        assert m._last_kernel == c.names[0 if qbits == 8 else 2], (c, m._last_kernel)
        assert tuple(y.shape) == ref.shape
        emax, el2 = rel_errors(y.cpu().numpy(), ref)
        assert emax <= _tol(m._last_kernel) and el2 <= _tol(m._last_kernel), (c, layout, qbits, m._last_kernel, emax, el2)
        assert same_bits(xq, xqo), (c, layout, qbits, "input_q")
        assert same_bits(wq, wqo), (c, layout, qbits, "weight_q")
