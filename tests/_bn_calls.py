"""Shared by the three GPU BatchNorm test files (and, for the bars, by test_bn_train_host.py): the raw calls of the six entry
points of csrc/bn_train.hip on the current stream, bit-for-bit comparison, and the float64 bars of test_gpu_bn_train.py."""
import numpy as np
import torch

import _bn_cases as B
from _bars import TOL_EXACT
from cnns_slfp_quantization_amd import _lib

DEV = torch.device("cuda:0")
NHWC = _lib.LAYOUT_NHWC


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ws(shape):
    n, h, w, c = shape
    nbytes = _lib.load().slfp_bn_train_workspace_bytes(n, h, w, c)
    return torch.empty(nbytes, dtype=torch.uint8, device=DEV), nbytes


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _fwd(shape, d, relu, rm=None, rv=None, x=None):
    """slfp_bn_train_fwd on the current stream: y, save_mean, save_invstd (rm / rv updated in place)."""
    n, h, w, c = shape
    x = d["x"].to(DEV) if x is None else x
    gamma, beta = d["gamma"].to(DEV), d["beta"].to(DEV)
    y = torch.empty_like(x)
    sm, si = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
    ws, nbytes = _ws(shape)
    _lib.check(_lib.load().slfp_bn_train_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(rm), _ptr(rv), B.MOMENTUM, B.EPS,
                                             int(relu), y.data_ptr(), sm.data_ptr(), si.data_ptr(), n, h, w, c, NHWC, ws.data_ptr(),
                                             nbytes, _stream()))
    return y, sm, si


def _bwd(shape, d, relu, y, sm, si, gy, params=True):
    n, h, w, c = shape
    x, gamma, gy = d["x"].to(DEV), d["gamma"].to(DEV), gy.to(DEV)
    gx = torch.empty_like(x)
    gg, gb = (torch.empty(c, device=DEV), torch.empty(c, device=DEV)) if params else (None, None)
    ws, nbytes = _ws(shape)
    _lib.check(_lib.load().slfp_bn_train_bwd(x.data_ptr(), y.data_ptr(), gy.data_ptr(), gamma.data_ptr(), sm.data_ptr(), si.data_ptr(),
                                             int(relu), gx.data_ptr(), _ptr(gg), _ptr(gb), n, h, w, c, NHWC, ws.data_ptr(), nbytes,
                                             _stream()))
    return gx, gg, gb


def _res_fwd(shape, d, relu, res, rm=None, rv=None, x=None):
    """slfp_bn_res_train_fwd on the current stream: y, save_mean, save_invstd (rm / rv updated in place)."""
    n, h, w, c = shape
    x = d["x"].to(DEV) if x is None else x
    gamma, beta = d["gamma"].to(DEV), d["beta"].to(DEV)
    y = torch.empty_like(x)
    sm, si = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
    ws, nbytes = _ws(shape)
    _lib.check(_lib.load().slfp_bn_res_train_fwd(x.data_ptr(), res.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(rm), _ptr(rv),
                                                 B.MOMENTUM, B.EPS, int(relu), y.data_ptr(), sm.data_ptr(), si.data_ptr(), n, h, w, c,
                                                 NHWC, ws.data_ptr(), nbytes, _stream()))
    return y, sm, si


def _res_bwd(shape, d, relu, y, sm, si, gy, gres=True, params=True, x=None):
    """slfp_bn_res_train_bwd: gx, gres, ggamma, gbeta (None where not asked for)."""
    n, h, w, c = shape
    x = d["x"].to(DEV) if x is None else x
    gamma, gy = d["gamma"].to(DEV), gy.to(DEV)
    gx = torch.empty_like(x)
    gr = torch.empty_like(x) if gres else None
    gg, gb = (torch.empty(c, device=DEV), torch.empty(c, device=DEV)) if params else (None, None)
    ws, nbytes = _ws(shape)
    _lib.check(_lib.load().slfp_bn_res_train_bwd(x.data_ptr(), y.data_ptr(), gy.data_ptr(), gamma.data_ptr(), sm.data_ptr(),
                                                 si.data_ptr(), int(relu), gx.data_ptr(), _ptr(gr), _ptr(gg), _ptr(gb), n, h, w, c,
                                                 NHWC, ws.data_ptr(), nbytes, _stream()))
    return gx, gr, gg, gb


def _lut_fwd(shape, ftab, x, gamma, beta, rm=None, rv=None):
    """slfp_bn_lut_train_fwd on the current stream: y, save_mean, save_invstd, save_lo (rm / rv updated in place)."""
    n, h, w, c = shape
    y = torch.empty_like(x)
    sm, si, lo = (torch.empty(c, device=DEV) for _ in range(3))
    ws, nbytes = _ws(shape)
    _lib.check(_lib.load().slfp_bn_lut_train_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(rm), _ptr(rv), B.MOMENTUM, B.EPS,
                                                 ftab.data_ptr(), y.data_ptr(), sm.data_ptr(), si.data_ptr(), lo.data_ptr(), n, h, w, c,
                                                 NHWC, ws.data_ptr(), nbytes, _stream()))
    return y, sm, si, lo


def _lut_bwd(shape, dtab, x, gy, gamma, beta, sm, si, lo, params=True):
    n, h, w, c = shape
    gx = torch.empty_like(x)
    gg, gb = (torch.empty(c, device=DEV), torch.empty(c, device=DEV)) if params else (None, None)
    ws, nbytes = _ws(shape)
    _lib.check(_lib.load().slfp_bn_lut_train_bwd(x.data_ptr(), gy.data_ptr(), gamma.data_ptr(), beta.data_ptr(), sm.data_ptr(),
                                                 si.data_ptr(), lo.data_ptr(), dtab.data_ptr(), gx.data_ptr(), _ptr(gg), _ptr(gb), n, h,
                                                 w, c, NHWC, ws.data_ptr(), nbytes, _stream()))
    return gx, gg, gb


def _bars_ok(got, ref, scale=None):
    """(max|d| / max|scale|, ||d|| / ||scale||) both <= 1e-5; scale defaults to ref."""
    scale = ref if scale is None else scale
    dd = np.asarray(got, dtype=np.float64) - ref
    e = float(np.abs(dd).max() / np.abs(scale).max())
    l = float(np.linalg.norm(dd) / np.linalg.norm(scale))
    print("max", e, "l2", l)
    return e <= TOL_EXACT and l <= TOL_EXACT


def _sum_bars_ok(name, got, ref, terms):
    """ggamma / gbeta: exactly 0 where every term is 0; |d| / sum|terms| <= 1e-5 elementwise and L2 <= 1e-6."""
    dd = np.abs(np.asarray(got, dtype=np.float64) - ref)
    elem = float((dd[terms > 0] / terms[terms > 0]).max()) if (terms > 0).any() else 0.0
    l2 = float(np.linalg.norm(dd) / max(np.linalg.norm(ref), 1e-300))
    print(name, "elem", elem, "l2", l2)
    return bool((dd[terms == 0] == 0).all()) and elem <= 1e-5 and l2 <= 1e-6
