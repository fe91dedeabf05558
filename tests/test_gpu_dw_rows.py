"""The register-window depthwise kernel (csrc/conv_dw3.hip, k_dw3x3_rows) against the tile kernel (csrc/conv_dw2.hip) and the
CPU oracle.

Both kernels run the same arithmetic in the same order, so their outputs must agree byte for byte: every stride-2 depthwise
geometry of MobileNetV1 at N = 128 and N = 256, with and without the fused scale / shift + ReLU, and shapes the net does not
have (ragged tiles, pad 0 / 1 / 2, C = 32 / 96, N = 1 / 3 / 5, NaN, +-inf, +-0, values on both clamps).  All elements are
compared, without a tolerance.  The tile kernel's outputs come from a fresh child process started with SLFP_DW_ROWS=0
(tests/_dw_rows_worker.py) before this process runs a depthwise layer; this process runs k_dw3x3_rows on every case (the
switch forced to every size class, so that the comparison does not depend on the measured dispatch rule)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import elem_exceed_frac, rel_errors
from _bars import ELEM_MIN, elem_frac_bar, tol
from _dw_rows_worker import CASES, KA, KW, NET_GEOMS, ODD_CASES, Case
from oracle import slfp_oracle as so

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tile_outputs(tmp_path_factory):
    """Directory of <case>.npy written by the tile kernel in a child process (a child, never an exec of this process)."""
    out = tmp_path_factory.mktemp("dw_tile")
    env = dict(os.environ, SLFP_DW_ROWS="0", PYTHONDONTWRITEBYTECODE="1")
    p = subprocess.run([sys.executable, os.path.join(HERE, "_dw_rows_worker.py"), str(out), "tile"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode == 0 and "dw rows worker ok" in p.stdout, p.stdout[-3000:]
    return out


@pytest.fixture(scope="module")
def rows_forced(tile_outputs):
    """This process on k_dw3x3_rows for every size class (after the child has finished)."""
    from cnns_slfp_quantization_amd import _lib
    L = _lib.load()
    old = os.environ.get("SLFP_DW_ROWS")
    os.environ["SLFP_DW_ROWS"] = "15"
    L.slfp_debug_reload_switches()
    yield L
    if old is None:
        os.environ.pop("SLFP_DW_ROWS", None)
    else:
        os.environ["SLFP_DW_ROWS"] = old
    L.slfp_debug_reload_switches()


def _same_bytes(a, b):
    return a.shape == b.shape and bool(np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_rows_kernel_is_byte_equal_to_the_tile_kernel(dev, tile_outputs, rows_forced, case):
    c = Case(case, dev)
    assert c.variant() == "rows", (c.tag, c.variant())
    got = c.run().cpu().numpy()
    ref = np.load(os.path.join(str(tile_outputs), c.tag + ".npy"))
    if case[7] == "nonfinite" and not c.post:   # (the fused ReLU is fmaxf(u, 0): it turns a NaN into 0 in both kernels)
        assert np.isnan(ref).any() and not np.isnan(ref).all()
    if case[7] != "nonfinite":
        assert np.isfinite(ref).all()
    assert _same_bytes(got, ref), (c.tag, int((got.view(np.uint32) != ref.view(np.uint32)).sum()), got.size)


def _oracle(c, images):
    xs = c.x[images].permute(0, 3, 1, 2).contiguous().cpu().numpy()
    ref = so.conv2d(xs, c.w.cpu().numpy(), None, 2, c.d.pad_h, 1, c.d.c_in, KA, KW, 8)
    if c.post:   # eval-mode BatchNorm as one float32 FMA per element, then the ReLU
        sc = c.scale.cpu().numpy().astype(np.float64)[None, :, None, None]
        sh = c.shift.cpu().numpy().astype(np.float64)[None, :, None, None]
        ref = np.maximum((ref.astype(np.float64) * sc + sh).astype(np.float32), 0.0)
    return ref


def _check_oracle(c, images):
    got = c.run()[images].permute(0, 3, 1, 2).contiguous().cpu().numpy()
    ref = _oracle(c, images)
    emax, el2 = rel_errors(got, ref)
    assert emax <= tol("dw3x3_nhwc") and el2 <= tol("dw3x3_nhwc"), (c.tag, emax, el2)
    if got.size >= ELEM_MIN:
        assert elem_exceed_frac(got, ref) <= elem_frac_bar("dw3x3_nhwc"), (c.tag, elem_exceed_frac(got, ref))


@pytest.mark.parametrize("case", [c for c in ODD_CASES if c[7] == "finite"], ids=[c[0] for c in ODD_CASES if c[7] == "finite"])
def test_rows_kernel_odd_shapes_vs_oracle(dev, rows_forced, case):
    c = Case(case, dev)
    assert c.variant() == "rows"
    _check_oracle(c, list(range(case[1])))


@pytest.mark.parametrize("geom", NET_GEOMS, ids=[f"c{c}_h{h}" for c, h in NET_GEOMS])
@pytest.mark.parametrize("post", [False, True], ids=["plain", "post"])
def test_rows_kernel_net_shapes_vs_oracle(dev, rows_forced, geom, post):
    """Sampled images of a batch whose waves straddle image boundaries (N = 5: first, middle, last)."""
    ch, h = geom
    c = Case((f"oracle_c{ch}_h{h}", 5, ch, h, h, 1, post, "finite"), dev)
    assert c.variant() == "rows"
    _check_oracle(c, [0, 2, 4])
