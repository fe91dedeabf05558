"""Host side of the non-square geometry table (tests/_aniso_cases.py): where every row and its transposed twin dispatches.
tests/test_gpu_aniso.py checks what the kernels compute on these rows; if a dispatch change moved a row to another family,
that test would silently check the other family instead.  This one says so.  No device is touched."""
import ctypes

import pytest

import _aniso_cases as ac
from cnns_slfp_quantization_amd import _lib

CASES = ac.all_cases()
IDS = [f"{c.fam}{i}{'t' if tw else ''}" for c, tw, i in CASES]


def test_table_is_what_it_claims():
    assert len(ac.ROWS) >= 40 and len(CASES) > len(ac.ROWS)
    for c, tw, i in CASES:
        assert c.H != c.W and c.fam in ac.FAMILIES and len(c.names) == len(ac.MODES)
        assert ac.twin(ac.twin(c)) == c
    rows = [c for c, tw, _ in CASES if not tw]
    assert any(c.kh != c.kw for c in rows) and any(c.ph != c.pw for c in rows) and any(c.sh != c.sw for c in rows)
    assert any(c.dh != c.dw for c in rows) and any(1 < c.g < c.C for c in rows)
    assert any(c.H < c.W for c in rows) and any(c.H > c.W for c in rows)


@pytest.mark.parametrize("c, is_twin, row", CASES, ids=IDS)
def test_dispatch_of_row(c, is_twin, row):
    L = _lib.load()
    for (qbits, passes), want in zip(ac.MODES, c.names):
        d = ac.desc(_lib, c, 3, qbits, passes)
        ho, wo = ctypes.c_int64(), ctypes.c_int64()
        assert L.slfp_conv2d_out_shape(ctypes.byref(d), ctypes.byref(ho), ctypes.byref(wo)) == _lib.OK
        assert (ho.value, wo.value) == ac.out_hw(c), (c, qbits, passes)
        kern = L.slfp_conv2d_kernel_name(ctypes.byref(d)).decode()
        assert kern == want, (c, qbits, passes, kern)
        # every family reads its weights from the prepared blob; the matrix-core families of compute-bound layers encode
        # the input once into the workspace, and the channel-padded copies live there
        assert L.slfp_conv2d_wprep_bytes(ctypes.byref(d)) > 0, (c, kern)
        ws = L.slfp_conv2d_workspace_bytes(ctypes.byref(d))
        needs_ws = kern.startswith(("dense_mfma", "stem_mfma", "repad+"))
        assert (ws > 0) == needs_ws, (c, kern, ws)
        # the NCHW interface converts through the workspace on top of that
        dn = ac.desc(_lib, c, 3, qbits, passes, _lib.LAYOUT_NCHW, _lib.LAYOUT_NCHW)
        assert L.slfp_conv2d_kernel_name(ctypes.byref(dn)).decode() == want
        hoN, woN = ac.out_hw(c)
        assert L.slfp_conv2d_workspace_bytes(ctypes.byref(dn)) >= ws + 4 * 3 * (c.C * c.H * c.W + c.O * hoN * woN), (c, kern)
        if c.variant is not None:
            for has_post in (0, 1):
                assert L.slfp_debug_dw3x3_variant(ctypes.byref(d), has_post).decode() == c.variant, (c, qbits, passes)
        else:
            assert L.slfp_debug_dw3x3_variant(ctypes.byref(d), 0).decode() == "none", c


def test_random_sweep_reaches_every_family_and_skips_nothing():
    """The generator of the GPU sweep, on the host: no degenerate draw, H != W and independent pairs actually drawn, and
    the dispatch sends the draws to every family the square sweep of tests/test_gpu_parity.py asserts."""
    L = _lib.load()
    draws = ac.sweep_draws()
    assert len(draws) == ac.SWEEP_DRAWS
    assert sum(ac.degenerate(c) for c, *_ in draws) == 0
    kinds = {}
    for c, n, qbits, passes, bias in draws:
        d = ac.desc(_lib, c, n, qbits, passes)
        ho, wo = ctypes.c_int64(), ctypes.c_int64()
        assert L.slfp_conv2d_out_shape(ctypes.byref(d), ctypes.byref(ho), ctypes.byref(wo)) == _lib.OK, c
        assert (ho.value, wo.value) == ac.out_hw(c) and ho.value > 0 and wo.value > 0, c
        kern = L.slfp_conv2d_kernel_name(ctypes.byref(d)).decode()
        kinds[kern] = kinds.get(kern, 0) + 1
    for fam in ac.SWEEP_FAMILIES:
        assert kinds.get(fam, 0) > 0, (fam, kinds)
    cs = [c for c, *_ in draws]
    assert sum(c.H != c.W for c in cs) > 0.9 * len(cs)
    assert any(c.kh != c.kw for c in cs) and any(c.ph != c.pw for c in cs)
    assert 0 < sum(c.sh != c.sw for c in cs) <= len(cs) // 5 + 10 and 0 < sum(c.dh != c.dw for c in cs) <= len(cs) // 5 + 10
    # a rectangular draw on a fast family is the point: most draws must not end on the direct kernel
    assert kinds["direct_nhwc"] < 0.6 * len(cs), kinds
    print(kinds)
