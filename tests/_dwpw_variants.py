"""Small ragged cases for every instance of the two one-kernel depthwise -> pointwise block kernels (csrc/conv_dwpw.hip: k_dwpw<S, KS,
NT>, float32 in and out; csrc/conv_dwpw_codes.hip: k_dwpw_codes<S, KS, NT, FMT, YC>, 1-byte codes in, float32 or codes out), shared by
tests/test_dwpw_variants_host.py (the table reaches what it claims, spans what the launchers can select and what the queries accept)
and tests/test_gpu_dwpw_variants.py (each row bit for bit against the two-kernel sequence, against a CPU reference, inside guards).

A row = the block's geometry, the interface it is called through, the epilogue's operands and flags, and the string
slfp_debug_dwpw_instance must then report (include/slfp.h; one word per template argument a launcher chooses):

    f32/s<1|2>/k<1|2|4>/n<4|8|16>                          k_dwpw<S, KS, NT>             (KS = C / 32, NT = N / 16)
    codes/s<1|2>/k<1|2|4>/n<4|8|16>/<act8|sfp7>/<f32|yc>   k_dwpw_codes<S, KS, NT, FMT, YC>

Interfaces: "f32" slfp_dwpw_fwd; "cin" slfp_dwpw_fwd_codes with float32 output; "cio8" / "cio7" with code output for a q_bit 8 / 7
reader (the reader's q_bit is its own: both appear behind both input formats).

Shapes, and the edge each one hits (a workgroup = one image x one 14 x 14 (stride 1) / 7 x 7 (stride 2) tile of depthwise outputs):
    base, stride 1   15 x 17 pad 1 -> 15 x 17   2 x 2 tiles, a 1-row last row tile and a 3-column last column tile
    base, stride 2   16 x 19 pad 1 -> 8 x 10    2 x 2 tiles of 7, a 1-row and a 3-column remainder
                     batch 3: 12 workgroups (>= 8, no multiple of 8: the tail of xcd_remap), tile indices crossing an image
    stride 1 pad 0   14 x 14 -> 12 x 12         the smallest stride-1 input: one tile, ragged both ways; batch 1: a grid below 8
    stride 1 pad 2   14 x 16 -> 16 x 18         2 x 2 tiles, two padding rows / columns in the halo
    stride 2 pad 0   15 x 20 -> 7 x 9           an exactly full tile down, a 2-column remainder across
    stride 2 pad 1   15 x 20 -> 8 x 10          odd height, even width: a bottom padding row but no right-hand padding column
    stride 2 pad 2   17 x 15 -> 10 x 9
    tiny, stride 2   5 x 9 pad 0 -> 2 x 4; 2 x 2 pad 1 -> 1 x 1 (batch 2): images far smaller than a tile, at K = 32 and K = 128
Every (S, KS, NT) of both kernels, and every (FMT, YC) of the codes kernel, runs at its stride's base shape with signed inputs,
relu1 = 1, relu2 = 0, a pointwise bias and post2 vectors.  One instance per stride then takes the other epilogue branches (post2 NULL
with and without the bias -- has_vec false --, the ReLU pairs (0, 0), (0, 1), (1, 1)); each (S, KS) -- phase 1's template arguments --
takes pad 0 and pad 2 on both kernels; the special-value rows plant NaN / +inf / -inf / -0.0 in the float32 input ("values") or a NaN
in one channel of post1_shift with relu1 = 0 ("shift_nan": the depthwise result is NaN, which the code path patches to the fp16 zero)."""
from collections import namedtuple

Row = namedtuple("Row", "name c n_out stride pad h w batch qbits iface bias post2 relu1 relu2 special instance")

IFACES = ("f32", "cin", "cio8", "cio7")
KA_DW, KW_DW, KA_PW, KW_PW, KA_NEXT = 0.17, 0.11, 0.33, 0.07, 0.29   # tests/test_gpu_dwpw_codes.py's scales
STRIDES, KSS, NTS = (1, 2), (1, 2, 4), (4, 8, 16)
BASE = {1: (15, 17), 2: (16, 19)}   # stride -> (h, w) at pad 1
NAN_CHANNEL = 5                      # the channel of post1_shift a "shift_nan" row sets to NaN

ROWS = []


def _fmt(qbits):
    return "act8" if qbits == 8 else "sfp7"


def instance_name(iface, stride, ks, nt, qbits):
    if iface == "f32":
        return f"f32/s{stride}/k{ks}/n{nt}"
    return f"codes/s{stride}/k{ks}/n{nt}/{_fmt(qbits)}/{'f32' if iface == 'cin' else 'yc'}"


def _add(name, iface, stride, ks, nt, h=None, w=None, pad=1, batch=3, qbits=8, bias=True, post2=True, relu1=1, relu2=0, special=None):
    assert iface in IFACES and special in (None, "values", "shift_nan")
    assert special != "values" or iface == "f32"
    assert special != "shift_nan" or (iface != "f32" and relu1 == 0)
    if h is None:
        h, w = BASE[stride]
    ROWS.append(Row(name, 32 * ks, 16 * nt, stride, pad, h, w, batch, qbits, iface, bool(bias), bool(post2), relu1, relu2, special,
                    instance_name(iface, stride, ks, nt, qbits)))


# =============================================================================== every instance, at the base shape
_k = 0
for _s in STRIDES:
    for _ks in KSS:
        for _nt in NTS:
            _add(f"all-f32-s{_s}k{_ks}n{_nt}", "f32", _s, _ks, _nt, qbits=8 if _k % 2 == 0 else 7)
            for _q in (8, 7):
                _add(f"all-cin-s{_s}k{_ks}n{_nt}-{_fmt(_q)}", "cin", _s, _ks, _nt, qbits=_q)
                _reader = 8 if (_k % 2 == 0) == (_q == 8) else 7   # both readers behind both input formats
                _add(f"all-cio{_reader}-s{_s}k{_ks}n{_nt}-{_fmt(_q)}", f"cio{_reader}", _s, _ks, _nt, qbits=_q)
            _k += 1

# =============================================================================== the epilogue's branches, one instance per stride
for _s, _ks, _nt in ((1, 1, 4), (2, 2, 8)):
    for _i in ("f32", "cin", "cio8"):
        _t = f"{_i}-s{_s}k{_ks}n{_nt}"
        _add(f"ep-{_t}-bias-nopost2", _i, _s, _ks, _nt, post2=False)                # sc2 == nullptr, has_vec by the bias
        _add(f"ep-{_t}-nobias-nopost2", _i, _s, _ks, _nt, bias=False, post2=False)   # has_vec false
        _add(f"ep-{_t}-nobias", _i, _s, _ks, _nt, bias=False)                        # has_vec by post2 alone: the bias row of ep is zeros
        for _r1, _r2 in ((0, 0), (0, 1), (1, 1)):
            _add(f"ep-{_t}-relu{_r1}{_r2}", _i, _s, _ks, _nt, relu1=_r1, relu2=_r2)

# =============================================================================== padding: every (S, KS) of phase 1, both kernels
_PADS = {1: ((0, 14, 14, 1), (2, 14, 16, 3)), 2: ((0, 15, 20, 3), (1, 15, 20, 3), (2, 17, 15, 2))}   # stride -> (pad, h, w, batch)
_k = 0
for _s in STRIDES:
    for _ks in KSS:
        for _p, _h, _w, _b in _PADS[_s]:
            _nt = NTS[_k % 3]
            _q = 8 if _k % 2 == 0 else 7
            _add(f"pad-f32-s{_s}k{_ks}n{_nt}-{_h}x{_w}p{_p}", "f32", _s, _ks, _nt, _h, _w, _p, _b, qbits=_q)
            _i = ("cin", "cio8", "cio7")[_k % 3]
            _add(f"pad-{_i}-s{_s}k{_ks}n{_nt}-{_h}x{_w}p{_p}-{_fmt(_q)}", _i, _s, _ks, _nt, _h, _w, _p, _b, qbits=_q)
            _k += 1

# =============================================================================== stride-2 images far smaller than a tile
for _ks, _nt in ((1, 4), (4, 16)):
    for _p, _h, _w, _b in ((0, 5, 9, 1), (1, 2, 2, 2)):
        _add(f"tiny-f32-k{_ks}n{_nt}-{_h}x{_w}p{_p}", "f32", 2, _ks, _nt, _h, _w, _p, _b)
        _i = "cin" if _p == 0 else "cio8"
        _add(f"tiny-{_i}-k{_ks}n{_nt}-{_h}x{_w}p{_p}", _i, 2, _ks, _nt, _h, _w, _p, _b, qbits=8 if _ks == 1 else 7)

# =============================================================================== special values
for _s, _ks, _nt in ((1, 2, 8), (2, 4, 4)):
    _add(f"nan-f32-s{_s}k{_ks}n{_nt}", "f32", _s, _ks, _nt, relu1=0, relu2=0, special="values")
    _add(f"nan-cin-s{_s}k{_ks}n{_nt}", "cin", _s, _ks, _nt, relu1=0, relu2=0, special="shift_nan")
    _add(f"nan-cio8-s{_s}k{_ks}n{_nt}", "cio8", _s, _ks, _nt, relu1=0, relu2=1, special="shift_nan", qbits=7)

del _k, _s, _ks, _nt, _q, _reader, _i, _t, _r1, _r2, _p, _h, _w, _b


def selectable():
    """Every instance the two launchers can select, from the grammar: 18 + 72."""
    out = set()
    for s in STRIDES:
        for ks in KSS:
            for nt in NTS:
                out.add(f"f32/s{s}/k{ks}/n{nt}")
                out |= {f"codes/s{s}/k{ks}/n{nt}/{f}/{o}" for f in ("act8", "sfp7") for o in ("f32", "yc")}
    return out


def out_hw(r):
    return (r.h + 2 * r.pad - 3) // r.stride + 1, (r.w + 2 * r.pad - 3) // r.stride + 1


def workgroups(r):
    """Workgroups of the row's launch: images x tiles of 14 x 14 (stride 1) / 7 x 7 (stride 2) depthwise outputs."""
    ho, wo = out_hw(r)
    t = 7 if r.stride == 2 else 14
    return r.batch * (-(-ho // t)) * (-(-wo // t))


def kernel_of(r):
    return "k_dwpw" if r.iface == "f32" else "k_dwpw_codes"


def reader_qbits(r):
    """q_bit of the layer that reads the row's code output (None: float32 output)"""
    return {"cio8": 8, "cio7": 7}.get(r.iface)


def geom_key(r):
    """Rows with the same key share the input tensor."""
    return (r.c, r.batch, r.h, r.w)


def make_descs(lib, r):
    """The two layers' descriptors (NHWC, single-pass mode), as tests/test_gpu_dwpw_codes.py::_Block builds them."""
    import numpy as np
    ho, wo = out_hw(r)
    common = dict(dil_h=1, dil_w=1, x_layout=lib.LAYOUT_NHWC, y_layout=lib.LAYOUT_NHWC, qbits=r.qbits, mfma_passes=lib.MFMA_F16X1, reserved=0)
    dw = lib.ConvDesc(n=r.batch, c_in=r.c, h=r.h, w=r.w, c_out=r.c, kh=3, kw=3, stride_h=r.stride, stride_w=r.stride, pad_h=r.pad,
                      pad_w=r.pad, groups=r.c, ka=float(np.float32(KA_DW)), kw_scale=float(np.float32(KW_DW)), **common)
    pw = lib.ConvDesc(n=r.batch, c_in=r.c, h=ho, w=wo, c_out=r.n_out, kh=1, kw=1, stride_h=1, stride_w=1, pad_h=0, pad_w=0, groups=1,
                      ka=float(np.float32(KA_PW)), kw_scale=float(np.float32(KW_PW)), **common)
    return dw, pw


def make_io(lib, r):
    """slfp_conv2d_io of the row's one-kernel call (None: the float32 interface)"""
    import numpy as np
    if r.iface == "f32":
        return None
    out = reader_qbits(r)
    return lib.ConvIo(x_codes=1, y_codes=0 if out is None else 1, y_ka=float(np.float32(KA_NEXT)) if out is not None else 1.0,
                      y_qbits=out if out is not None else 8)


def instance(lib, r, dw=None, pw=None, io="row", relu1=None, relu2=None):
    """slfp_debug_dwpw_instance for the row (or for the descriptors / io / flags given in its place)"""
    import ctypes
    if dw is None:
        dw, pw = make_descs(lib, r)
    if io == "row":
        io = make_io(lib, r)
    return lib.load().slfp_debug_dwpw_instance(ctypes.byref(dw), ctypes.byref(pw), ctypes.byref(io) if io is not None else None, int(r.bias),
                                               r.relu1 if relu1 is None else relu1, r.relu2 if relu2 is None else relu2).decode()


def special_sites(r):
    """(image, row, column, channel, value) a "values" row plants: a NaN, +inf, -inf and -0.0 pixel inside the first image (one value per
    channel of that pixel, in turn) and a NaN in the last channel of the last image's last pixel."""
    nan, inf = float("nan"), float("inf")
    vals = (nan, inf, -inf, -0.0)
    sites = [(0, r.h // 2, r.w // 2, ch, vals[ch % 4]) for ch in range(r.c)]
    return sites + [(r.batch - 1, r.h - 1, r.w - 1, r.c - 1, nan)]


def make_input(r):
    """Seeded float32 NHWC input of a geometry key, as tests/test_gpu_dwpw_codes.py::_Block.input builds it, with both signs: all binades,
    both clamps from both sides, the tiny class, exact zeros of both signs.  Returns (x, x with special_sites planted)."""
    import numpy as np
    rng = np.random.default_rng(7000 + 13 * r.c + 101 * r.batch + 17 * r.h + r.w)
    x = (rng.standard_normal((r.batch, r.h, r.w, r.c)) * (6.0 * KA_DW)).astype(np.float32)
    x[..., 0::3] *= np.float32(2.0) ** rng.integers(-7, 1, size=x[..., 0::3].shape).astype(np.float32)   # the low binades too
    f = x.reshape(-1)
    f[::97] = 17.0 * KA_DW           # beyond the clamp
    f[3::101] = -17.0 * KA_DW
    f[5::193] = 0.05 * KA_DW         # the "tiny" class
    f[11::211] = -0.05 * KA_DW
    f[7::89] = 0.0
    f[13::223] = -0.0
    xs = x.copy()
    for img, row, col, ch, v in special_sites(r):
        xs[img, row, col, ch] = v
    return x, xs


def make_inputs(r):
    """Everything a row's launches read, as numpy arrays: x, x_special (make_input) and the pair's weights and vectors (make_params)."""
    x, xs = make_input(r)
    return dict(x=x, x_special=xs, **make_params(r.c, r.n_out))


def make_params(c, n_out):
    """Seeded weights and per-channel vectors of a (C, N) pair: w_dw [C, 1, 3, 3], w_pw [N, C, 1, 1], sc1, sh1 [C], bias2, sc2, sh2 [N].
    Every row of the pair uses the same arrays; sc2 alternates in sign, so the output carries both signs whatever the ReLUs in front."""
    import numpy as np
    rng = np.random.default_rng(500 + 3 * c + n_out)
    w_dw = (rng.standard_normal((c, 1, 3, 3)) * (4.0 * KW_DW)).astype(np.float32)
    w_pw = (rng.standard_normal((n_out, c, 1, 1)) * min(5.0 * KW_PW, 3.0 * (2.0 / c) ** 0.5 + 2.0 * KW_PW)).astype(np.float32)
    sc1 = (rng.random(c) + 0.5).astype(np.float32)
    sh1 = (rng.standard_normal(c) * 0.3).astype(np.float32)
    bias2 = (rng.standard_normal(n_out) * 0.2).astype(np.float32)
    sc2 = (rng.random(n_out) + 0.5).astype(np.float32)
    sc2[1::2] *= -1.0
    sh2 = (rng.standard_normal(n_out) * 0.3).astype(np.float32)
    return dict(w_dw=w_dw, w_pw=w_pw, sc1=sc1, sh1=sh1, bias2=bias2, sc2=sc2, sh2=sh2)
