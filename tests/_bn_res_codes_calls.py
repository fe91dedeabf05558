"""Shared by test_gpu_bn_res_codes_train.py: the raw call of slfp_bn_res_codes_train_fwd on the current stream, the library's
encoder and decoder on extended codes, the residual that spreads a tail's output over the reader's classes, and guarded buffers."""
import torch

import _bn_cases as B
from _bn_calls import DEV, NHWC, _ptr, _stream, _ws
from cnns_slfp_quantization_amd import _lib

GUARD = 256


def fmt(qbits):
    return _lib.FMT_SFP7 if qbits == 7 else _lib.FMT_ACT8


def res_codes_fwd_raw(shape, x, res, gamma, beta, relu, ka, qbits, y, codes, sm, si, rm=None, rv=None, ws=None):
    """The status of slfp_bn_res_codes_train_fwd on the given addresses (tensors, or integers for y / codes)."""
    n, h, w, c = shape
    buf, nbytes = _ws(shape) if ws is None else ws
    p = lambda t: t if isinstance(t, int) else t.data_ptr()
    return _lib.load().slfp_bn_res_codes_train_fwd(x.data_ptr(), res.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(rm), _ptr(rv),
                                                   B.MOMENTUM, B.EPS, int(relu), ka, qbits, p(y), p(codes), sm.data_ptr(), si.data_ptr(),
                                                   n, h, w, c, NHWC, buf.data_ptr(), nbytes, _stream())


def res_codes_fwd(shape, d, relu, res, ka, qbits, rm=None, rv=None, x=None):
    """slfp_bn_res_codes_train_fwd on the current stream: y, y_codes (uint8, channels_last), save_mean, save_invstd."""
    n, h, w, c = shape
    x = d["x"].to(DEV) if x is None else x
    gamma, beta = d["gamma"].to(DEV), d["beta"].to(DEV)
    y = torch.full_like(x, 7.0)
    codes = torch.full((n, c, h, w), 0xEE, dtype=torch.uint8, device=DEV).contiguous(memory_format=torch.channels_last)
    sm, si = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
    assert _lib.load().slfp_bn_res_codes_train_supported(n, h, w, c, NHWC, ka, qbits) == 1
    _lib.check(res_codes_fwd_raw(shape, x, res, gamma, beta, relu, ka, qbits, y, codes, sm, si, rm, rv))
    return y, codes, sm, si


def encode(y, ka, qbits):
    out = torch.empty(y.shape, dtype=torch.uint8, device=DEV).contiguous(memory_format=torch.channels_last)
    _lib.check(_lib.load().slfp_encode_f32(y.data_ptr(), out.data_ptr(), y.numel(), ka, fmt(qbits) | _lib.FMT_EXT, _stream()))
    return out


def decode(codes, qbits):
    out = torch.empty(codes.shape, dtype=torch.float32, device=DEV).contiguous(memory_format=torch.channels_last)
    _lib.check(_lib.load().slfp_decode_f32(codes.data_ptr(), out.data_ptr(), codes.numel(), fmt(qbits) | _lib.FMT_EXT, _stream()))
    return out


def targets(numel, ka, gen):
    """`numel` float32 values spread over the classes of a quantizer with scale `ka` (in memory order): both signs over eleven
    binades, and at fixed strides the clamp, the top regular class, the tiny class and exact zero."""
    e = torch.rand(numel, generator=gen) * 11.0 - 7.0
    t = ka * torch.exp2(e) * torch.where(torch.rand(numel, generator=gen) < 0.3, -1.0, 1.0)
    t[::97] = 17.0 * ka      # beyond the clamp
    t[3::101] = 15.0 * ka    # the top regular class of both formats
    t[5::103] = 0.01 * ka    # the tiny class
    t[6::109] = -0.01 * ka   # ... and its negative
    t[7::107] = 0.0          # exact zero, with and without the ReLU
    return t


def residual(y0, ka, gen):
    """res = target - y0 (y0: the plain BatchNorm's output, channels_last), so that y0 + res lands on targets(): where the
    subtraction is exact the sum is the target itself (always for target 0: res = -y0), elsewhere within an ulp of it."""
    flat = y0.permute(0, 2, 3, 1).reshape(-1)                      # memory order of a channels_last tensor
    res = targets(flat.numel(), ka, gen).to(y0.device) - flat
    n, c, h, w = y0.shape
    return res.view(n, h, w, c).permute(0, 3, 1, 2)                # channels_last strides, no copy


def guarded(nbytes, tail=True):
    """A uint8 buffer of 0xA5 with GUARD bytes in front of `nbytes` payload bytes and (tail) behind them; the payload is 16-byte
    aligned.  Without the tail the payload ends at the last byte of the allocation."""
    buf = torch.full((GUARD + nbytes + (GUARD if tail else 0),), 0xA5, dtype=torch.uint8, device=DEV)
    assert (buf.data_ptr() + GUARD) % 16 == 0
    return buf


def guards_ok(buf, nbytes):
    return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + nbytes:] == 0xA5).all())
