"""Small ragged cases for every image-stem and direct kernel instance (csrc/conv_direct.hip: k_direct, k_stem, k_stem_fixed, k_stem_mx;
conv_stem_small.hip: k_stem_small; conv_stem_mfma.hip: k_stem_rows, k_stem_im2row + k_stem_mfma), shared by
tests/test_stem_variants_host.py (the table reaches what it claims and spans what the launchers can select; the nets' first layers are
covered by it; the CPU restatement and the fp16 operand-level reference against the double-accumulating oracle) and
tests/test_gpu_stem_variants.py (each row against its reference, guard bands, NaN placement, twice).

A row = the descriptor fields, the interface the layer is called through, bias / post vectors / flags, mfma_passes, the switches to
set, and the string slfp_debug_stem_instance must then report.  The grammar (include/slfp.h):

    direct/<act8|sfp7>/cc<CC>/oc<chunks>/<vec|scalar|mixed>     k_direct<FMT>
    stem/gen/<act8|sfp7>/p<2|4|8>                               k_stem<FMT>
    stem/fixed/<act8|sfp7>/long                                 k_stem_fixed<FMT, 3, 3, 3, 2, 32>
    stem/fixed/tab/<f32|yc|yc-signed|lut>                       k_stem_fixed<Act8, 3, 3, 3, 2, 32, TAB, 16, YC, LUTQ>
    stem/mx/<f32|yc|yc-signed|lut>                              k_stem_mx<YC, LUTQ>
    small/nt<1|2|3|4>/<act8|sfp7>/<f32|yc|yc-signed|lut>        k_stem_small<FMT, NT, LUTQ>
    rows/nt<4|6>/<act8|sfp7>/<f32|yc|yc-signed>                 k_stem_rows<FMT, NT, YC>
    im2row/nt<4|6>/<act8|sfp7>/<f32|yc|yc-signed>               k_stem_im2row<FMT> + k_stem_mfma<NT, 8, YC>

Interfaces: "f32" slfp_conv2d_fwd (no post vectors, no flags); "post" slfp_conv2d_fwd_post; "cout" slfp_conv2d_fwd_codes_ws (float32
in, codes out); "lut" slfp_conv2d_fwd_codes_lut.  flags: 1 = SLFP_POST_RELU, 2 = SLFP_POST_LAYEROUT.  passes: the descriptor's
mfma_passes (3 = SLFP_MFMA_F16X3 keeps a qbits-8 layer off the fp16 stems).

Shapes, and the edge each one hits (n = 2 or 3 throughout, so tiles cross the image boundary).

k_stem_mx / k_stem_fixed<TAB, 16> (16 x 16 output tiles; 3x3 s2 3 -> 32):
    33 x 36 pad 1 -> 17 x 18    both axes ragged, 2 x 2 tiles; W * 3 = 108: a multiple of 4, pad_w = 1: k_stem_mx
    35 x 36 pad 0, 31 x 32 pad 2 -> 17 x 17   the paddings at which k_stem_mx's aligned float4 loads are off by one or two floats:
                                the selection must keep them on stem/fixed/tab, and the bits must be the restatement's
    33 x 36 pad (1, 0) and (0, 1)   pad_h != pad_w: only pad_w decides (the second one is k_stem_mx)
    33 x 35 pad 1               W * 3 = 105: no multiple of 4, stem/fixed/tab by itself
    7 x 8 pad 1 -> 4 x 4        an image smaller than a tile: 2 workgroups
    each of them takes f32, yc (ReLU folded), yc-signed and lut in turn; SLFP_STEM_OLD twins of the pad-1 rows;
    stem/fixed/<fmt>/long (8 x 16 tiles) under SLFP_LONG_ENCODE, at both formats (qbits 7 has a threshold table too: it runs the table
    kernels, see "sfp7" rows)
k_stem (8 x 16 tiles; reached with mfma_passes = 3 at qbits 8, or where neither fp16 stem applies: K > 32 with kh * kw < 25):
    O = 16 / 32 / 64 (P = 2 / 4 / 8); 3x3 s1 c3 at 9 x 17 pad 1 (2 x 2 ragged tiles); 2x2 c1 s1 (IWC = 17: step_h = 15, step_j = 1);
    7x7 c4 s4 O = 16 (IWC = 268 > 256: step_h = 0); kernels 1x3 and 3x1; stride 3; pad 0 and pad >= k / 2 + 1; bias, affine, ReLU
k_direct (8 x 8 tiles, 64-channel output chunks, CC <= 32), at 10 x 11 (2 x 2 ragged tiles) and one at 3 x 3:
    groups 3 with C = 9 -> O = 9 (scalar lanes, partial n_o); C = 5 -> O = 3; C = 4 -> O = 12 in 2 groups (mixed lanes); dilation 2;
    stride (2, 1); kernel 2x3; Cg = 40 (chunks of 32 + 8); Og = 72 (a second output chunk with 8 live channels and idle threads);
    dilation 8 with k = 3 (the LDS budget cuts CC below Cg); both formats
k_stem_small (8 x 32 tiles, one k-step of 32):
    K = 27 (3x3x3), K = 32 exactly (4x4x2 and 2x4x4: no zero slot in use), K = 25 (5x5x1), K = 2 (1x2x1); c_out 4 / 24 / 40 / 64 (NT
    1..4 with dead channels in the last tile); stride 1 at 9 x 35 and stride 2 at 17 x 67 (both 2 x 2 ragged); pads 0 / 1 / 2 and
    pad_h != pad_w; the c_out = 64 rows take yc, yc-signed and lut; both formats
k_stem_rows (8 x 32 tiles):
    7x7 s2 c3 -> 64 (nt4), -> 96 (nt6), -> 16 (dead tiles) at 20 x 70 pad 3 and 21 x 69 pad 0; 5x5 s1 c4; 7x7 s1 c2; 3x9 s2 c4
    (kw * c_in = 36: ksub = 2); yc and yc-signed where c_out % 16 == 0; both formats
k_stem_im2row + k_stem_mfma:
    odd stride * c_in (7x7 s1 c3, 6x6 s1 c1, 7x7 s3 c3); LDS overflow of the rows form (11x11 s4 c3 at 35 x 51); SLFP_STEM_IM2ROW
    twins of the rows-form rows; nt 4 and 6; yc forms
xcd_remap: every kernel has a row with fewer than 8 workgroups and one with a count >= 8 that is no multiple of 8 (the host test
recomputes the counts; k_stem_mfma's grid is persistent and capped by the device, so its unit count stands in)."""
from collections import namedtuple

Row = namedtuple("Row", "name c_in c_out k stride pad dil groups n h w qbits iface bias post flags passes env y_qbits variant")

IFACES = ("f32", "post", "cout", "lut")
RELU, LAYEROUT = 1, 2
SWITCHES = ("SLFP_STEM_OLD", "SLFP_STEM_IM2ROW", "SLFP_LONG_ENCODE")
OLD, IM2ROW, LONG = {"SLFP_STEM_OLD": "1"}, {"SLFP_STEM_IM2ROW": "1"}, {"SLFP_LONG_ENCODE": "1"}
F32_KINDS = ("direct", "stem")                # float32 arithmetic: held to the restatement bit for bit
F16_KINDS = ("small", "rows", "im2row")       # fp16 matrix-core stems: held to the operand-level reference

ROWS = []


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _add(name, variant, c_in, c_out, k, h, w, pad=0, stride=1, dil=1, groups=1, n=2, iface="f32", bias=False, post=False, flags=0,
         passes=0, env=None, qbits=8, y_qbits=None):
    assert iface in IFACES and (iface != "f32" or (not post and not flags))
    ROWS.append(Row(name, c_in, c_out, _pair(k), _pair(stride), _pair(pad), _pair(dil), groups, n, h, w, qbits, iface, bool(bias),
                    bool(post), flags, passes, tuple(sorted((env or {}).items())), y_qbits or qbits, variant))


def _fmt(qbits):
    return "act8" if qbits == 8 else "sfp7"


# output form -> (interface, post vectors, flags)
FORMS = {"f32": ("post", True, RELU), "yc": ("cout", True, RELU), "yc-signed": ("cout", True, 0), "lut": ("lut", True, LAYEROUT)}

# =============================================================================== k_stem_mx / k_stem_fixed (3x3 s2 3 -> 32)
# (tag, h, w, pad, n, kernel without a switch)
_MB = (("33x36p1", 33, 36, 1, 3, "mx"), ("35x36p0", 35, 36, 0, 2, "fixed/tab"), ("31x32p2", 31, 32, 2, 2, "fixed/tab"),
       ("33x36p10", 33, 36, (1, 0), 2, "fixed/tab"), ("33x36p01", 33, 36, (0, 1), 2, "mx"), ("33x35p1", 33, 35, 1, 2, "fixed/tab"),
       ("7x8p1", 7, 8, 1, 2, "mx"))
for _t, _h, _w, _p, _n, _kern in _MB:
    _add(f"mb-{_t}-plain", f"stem/{_kern}/f32", 3, 32, 3, _h, _w, _p, 2, n=_n)                                  # no bias, no post: raw acc
    for _form, (_i, _post, _fl) in FORMS.items():
        _add(f"mb-{_t}-{_form}", f"stem/{_kern}/{_form}", 3, 32, 3, _h, _w, _p, 2, n=_n, iface=_i, post=_post, flags=_fl,
             bias=(_form in ("f32", "yc-signed")))
        if _kern == "mx":   # the vector kernel on the same layer: the same bits
            _add(f"mb-{_t}-{_form}-old", f"stem/fixed/tab/{_form}", 3, 32, 3, _h, _w, _p, 2, n=_n, iface=_i, post=_post, flags=_fl,
                 bias=(_form in ("f32", "yc-signed")), env=OLD)
_add("mb-33x36p1-plain-old", "stem/fixed/tab/f32", 3, 32, 3, 33, 36, 1, 2, n=3, env=OLD)
_add("mb-33x36p1-lo", "stem/mx/f32", 3, 32, 3, 33, 36, 1, 2, n=3, iface="post", post=True, flags=LAYEROUT | RELU)   # the float32 layer-output quantizer
_add("mb-35x36p0-lo", "stem/fixed/tab/f32", 3, 32, 3, 35, 36, 0, 2, iface="post", post=True, flags=LAYEROUT)
_add("mb-33x36p1-yc-to-sfp7", "stem/mx/yc", 3, 32, 3, 33, 36, 1, 2, n=3, iface="cout", post=True, flags=RELU, y_qbits=7)
_add("mb-35x36p0-signed-to-sfp7", "stem/fixed/tab/yc-signed", 3, 32, 3, 35, 36, 0, 2, iface="cout", post=True, y_qbits=7)
_add("mb-33x36p1-sfp7", "stem/mx/f32", 3, 32, 3, 33, 36, 1, 2, n=3, qbits=7)                                      # SFP<3,3> has a threshold table too
_add("mb-35x36p0-sfp7", "stem/fixed/tab/f32", 3, 32, 3, 35, 36, 0, 2, qbits=7, iface="post", post=True, flags=RELU)
for _q in (8, 7):
    _add(f"mb-33x36p1-long-{_fmt(_q)}", f"stem/fixed/{_fmt(_q)}/long", 3, 32, 3, 33, 36, 1, 2, n=3, env=LONG, qbits=_q)
    _add(f"mb-35x36p0-long-{_fmt(_q)}", f"stem/fixed/{_fmt(_q)}/long", 3, 32, 3, 35, 36, 0, 2, env=LONG, qbits=_q, iface="post",
         post=True, flags=RELU, bias=True)

# =============================================================================== k_stem
_X3 = 3   # mfma_passes = SLFP_MFMA_F16X3
_add("gen-3x3c3-o64", "stem/gen/act8/p8", 3, 64, 3, 9, 17, 1, n=3, passes=_X3)                                # 2 x 2 ragged tiles, 12 workgroups
_add("gen-3x3c3-o32-post", "stem/gen/act8/p4", 3, 32, 3, 9, 17, 1, n=3, passes=_X3, iface="post", bias=True, post=True, flags=RELU)
_add("gen-3x3c3-o16", "stem/gen/act8/p2", 3, 16, 3, 9, 17, 1, n=3, passes=_X3, bias=True)
_add("gen-2x2c1", "stem/gen/act8/p8", 1, 64, 2, 9, 17, 0, passes=_X3)                                          # IWC = 17
_add("gen-7x7c4s4", "stem/gen/act8/p2", 4, 16, 7, 35, 70, 3, 4, passes=_X3, iface="post", post=True)          # IWC = 268: step_h = 0
_add("gen-1x3c3", "stem/gen/act8/p4", 3, 32, (1, 3), 9, 18, (0, 2), passes=_X3, iface="post", flags=RELU)     # pad_w = k / 2 + 1
_add("gen-3x1c2", "stem/gen/act8/p8", 2, 64, (3, 1), 10, 17, (2, 0), passes=_X3)                               # pad_h = k / 2 + 1
_add("gen-3x3c3s3", "stem/gen/act8/p4", 3, 32, 3, 25, 50, 0, 3, passes=_X3, bias=True)                         # stride 3: 8 x 16 exactly
_add("gen-5x5c4-p3", "stem/gen/act8/p8", 4, 64, 5, 8, 15, 3, n=3, passes=_X3, iface="post", post=True, flags=LAYEROUT | RELU)   # pad 3
_add("gen-4x4c3-sfp7", "stem/gen/sfp7/p4", 3, 32, 4, 10, 19, 1, qbits=7)                                       # K = 48 > 32, kh * kw < 25: no fp16 stem
_add("gen-4x4c3-sfp7-o16", "stem/gen/sfp7/p2", 3, 16, 4, 10, 19, 1, qbits=7, iface="post", bias=True, post=True, flags=RELU)
_add("gen-4x4c3-sfp7-o64", "stem/gen/sfp7/p8", 3, 64, 4, 10, 19, 1, n=3, qbits=7, bias=True)
_add("gen-3x3s2c3-o32-long", "stem/gen/act8/p4", 3, 32, 3, 17, 33, 1, 1, passes=_X3, env=LONG)                # stride 1: not the MobileNet stem

# =============================================================================== k_direct
_add("dir-g3c9", "direct/act8/cc3/oc1/scalar", 9, 9, 3, 10, 11, 1, groups=3, n=2)                              # Og = 3: partial n_o
_add("dir-c5o3", "direct/act8/cc5/oc1/scalar", 5, 3, 3, 10, 11, 1, iface="post", bias=True, post=True, flags=RELU)
_add("dir-c4o12g2", "direct/act8/cc2/oc1/mixed", 4, 12, 3, 10, 11, 1, groups=2, bias=True)                     # Og = 6: a vector and a scalar thread per group
_add("dir-dil2", "direct/act8/cc8/oc1/vec", 8, 8, 3, 10, 11, 2, dil=2, n=3)
_add("dir-s21", "direct/act8/cc8/oc1/vec", 8, 16, 3, 10, 11, 1, stride=(2, 1), iface="post", post=True)
_add("dir-2x3", "direct/sfp7/cc8/oc1/vec", 8, 8, (2, 3), 10, 11, (0, 1), qbits=7, bias=True)
_add("dir-cg40", "direct/act8/cc32/oc1/vec", 80, 8, 3, 10, 11, 1, groups=2)                                    # Cg = 40: chunks of 32 + 8
_add("dir-cg40-sfp7", "direct/sfp7/cc32/oc1/vec", 80, 16, (2, 3), 10, 11, 1, groups=2, qbits=7, iface="post", post=True, flags=RELU)
_add("dir-og72", "direct/act8/cc8/oc2/vec", 8, 72, (2, 3), 10, 11, 1, bias=True)                                # second output chunk: 8 live channels
_add("dir-dil8", "direct/act8/cc21/oc1/vec", 48, 8, 3, 20, 22, 8, dil=8, groups=2)                              # IH = IW = 24: 12288 / 576 = 21 < Cg = 24
_add("dir-3x3img", "direct/act8/cc5/oc1/scalar", 5, 6, 3, 3, 3, 1, n=3)                                         # one tile per image
_add("dir-lo", "direct/act8/cc8/oc1/vec", 8, 8, 3, 10, 11, 2, dil=2, n=3, iface="post", post=True, flags=LAYEROUT)

# =============================================================================== k_stem_small
# (tag, c_in, c_out, k, stride, h, w, pad, n)
_SM = (("k27-o64-s1", 3, 64, 3, 1, 9, 35, 1, 3), ("k27-o24-s2", 3, 24, 3, 2, 17, 67, 1, 2), ("k32-4x4x2-o40", 2, 40, 4, 1, 9, 35, 2, 2),
       ("k32-2x4x4-o4", 4, 4, (2, 4), 2, 17, 67, (0, 1), 3), ("k25-o64-s2", 1, 64, 5, 2, 17, 67, 2, 2), ("k2-o24", 1, 24, (1, 2), 1, 9, 35, 0, 2),
       ("k27-o40-p0", 3, 40, 3, 1, 9, 35, 0, 3), ("k27-o4-p21", 3, 4, 3, 1, 9, 35, (2, 1), 2))
for _t, _ci, _co, _k, _s, _h, _w, _p, _n in _SM:
    _nt = (_co + 15) // 16
    for _q in (8, 7):
        _pl = _q == 8
        _add(f"small-{_t}-{_fmt(_q)}", f"small/nt{_nt}/{_fmt(_q)}/f32", _ci, _co, _k, _h, _w, _p, _s, n=_n, qbits=_q,
             iface="f32" if _pl else "post", bias=not _pl, post=not _pl, flags=0 if _pl else RELU)
        if _co == 64:
            for _form in ("yc", "yc-signed", "lut"):
                _i, _post, _fl = FORMS[_form]
                _add(f"small-{_t}-{_form}-{_fmt(_q)}", f"small/nt4/{_fmt(_q)}/{_form}", _ci, _co, _k, _h, _w, _p, _s, n=_n, qbits=_q,
                     iface=_i, post=_post, flags=_fl, bias=(_form == "yc"))
_add("small-k27-o64-s1-affine", "small/nt4/act8/f32", 3, 64, 3, 9, 35, 1, n=3, iface="post", post=True)              # the affine alone

# =============================================================================== k_stem_rows and the two-kernel form
# (tag, c_in, c_out, k, stride, h, w, pad, n): stride * c_in even, the rows form fits LDS
_RW = (("7x7s2-o64", 3, 64, 7, 2, 20, 70, 3, 2), ("7x7s2-o96", 3, 96, 7, 2, 21, 69, 0, 2), ("7x7s2-o16", 3, 16, 7, 2, 20, 70, 3, 3),
       ("5x5s1c4-o64", 4, 64, 5, 1, 10, 35, 2, 2), ("7x7s1c2-o32", 2, 32, 7, 1, 11, 36, 3, 2),
       ("3x9s2c4-o64", 4, 64, (3, 9), 2, 17, 70, (1, 4), 2))
for _t, _ci, _co, _k, _s, _h, _w, _p, _n in _RW:
    _nt = 4 if _co <= 64 else 6
    for _q in (8, 7):
        for _kern, _env in (("rows", None), ("im2row", IM2ROW)):
            _pl = _q == 8
            _add(f"{_kern}-{_t}-{_fmt(_q)}", f"{_kern}/nt{_nt}/{_fmt(_q)}/f32", _ci, _co, _k, _h, _w, _p, _s, n=_n, qbits=_q, env=_env,
                 iface="f32" if _pl else "post", bias=not _pl, post=not _pl, flags=0 if _pl else RELU)
            if _co % 16 == 0 and _q == 8 or _t in ("7x7s2-o96", "5x5s1c4-o64"):
                for _form in ("yc", "yc-signed"):
                    _i, _post, _fl = FORMS[_form]
                    _add(f"{_kern}-{_t}-{_form}-{_fmt(_q)}", f"{_kern}/nt{_nt}/{_fmt(_q)}/{_form}", _ci, _co, _k, _h, _w, _p, _s, n=_n,
                         qbits=_q, env=_env, iface=_i, post=_post, flags=_fl, bias=(_form == "yc"))
# odd stride * c_in and the LDS overflow: the two-kernel form without a switch
_IM = (("7x7s1c3-o64", 3, 64, 7, 1, 10, 35, 3, 2), ("6x6s1c1-o96", 1, 96, 6, 1, 11, 36, 2, 2), ("7x7s3c3-o32", 3, 32, 7, 3, 25, 70, 3, 3),
       ("11x11s4c3-o64", 3, 64, 11, 4, 35, 51, 2, 2))
for _t, _ci, _co, _k, _s, _h, _w, _p, _n in _IM:
    _nt = 4 if _co <= 64 else 6
    _add(f"im2row-{_t}", f"im2row/nt{_nt}/act8/f32", _ci, _co, _k, _h, _w, _p, _s, n=_n, iface="post", bias=True, post=True, flags=RELU)
    _add(f"im2row-{_t}-yc", f"im2row/nt{_nt}/act8/yc", _ci, _co, _k, _h, _w, _p, _s, n=_n, iface="cout", bias=True, post=True, flags=RELU)
    _add(f"im2row-{_t}-sfp7", f"im2row/nt{_nt}/sfp7/f32", _ci, _co, _k, _h, _w, _p, _s, n=_n, qbits=7)

del _t, _h, _w, _p, _n, _kern, _form, _i, _post, _fl, _q, _ci, _co, _k, _s, _nt, _pl, _env


def kind(r):
    return r.variant.split("/")[0]


def out_hw(r):
    return ((r.h + 2 * r.pad[0] - r.dil[0] * (r.k[0] - 1) - 1) // r.stride[0] + 1,
            (r.w + 2 * r.pad[1] - r.dil[1] * (r.k[1] - 1) - 1) // r.stride[1] + 1)


def taps(r):
    """multiply-adds of one output element, padded ones included"""
    return r.k[0] * r.k[1] * (r.c_in // r.groups)


def chunk(r):
    """k_direct's channel chunk CC, from the reporter string (0 for the stems: one chunk)"""
    return int(r.variant.split("/")[2][2:]) if kind(r) == "direct" else 0


def geom_key(r):
    """Rows with the same geometry key share inputs, weights and per-channel vectors."""
    return (r.c_in, r.c_out, r.k, r.groups, r.n, r.h, r.w)


def layer_key(r):
    """Rows with the same layer key describe the same computation on the same inputs."""
    return geom_key(r) + (r.stride, r.pad, r.dil, r.qbits, r.bias, r.post, r.flags)


def workgroups(r):
    """Workgroups of the row's launch, from the launchers' geometry (k_stem_mfma: its units of 16 pixels per wave, 8 waves a workgroup,
    before the device's cap on the persistent grid)."""
    ho, wo = out_hw(r)
    cdiv = lambda a, b: -(-a // b)   # noqa: E731
    v = r.variant.split("/")
    if v[0] == "direct":
        return r.n * cdiv(ho, 8) * cdiv(wo, 8) * r.groups * cdiv(r.c_out // r.groups, 64)
    if v[0] == "stem":
        th = 16 if v[1] == "mx" or v[2] == "tab" else 8
        return r.n * cdiv(ho, th) * cdiv(wo, 16)
    if v[0] == "im2row":
        return cdiv(r.n * ho * cdiv(wo, 16), 8)
    return r.n * cdiv(ho, 8) * cdiv(wo, 32)


KA, KW, KA_NEXT = 0.21, 0.027, 0.2345


def specials(ka=KA):
    """Values written over seeded positions of the input: both zeros, the clamps of QA(x / Ka) from both sides, the tiny class, and
    values far beyond the clamp."""
    return [0.0, -0.0, ka * 2.0 ** -5, -ka * 2.0 ** -5, ka * 2.0 ** -6, ka * 2.0 ** -4.9, ka * 15.5, -ka * 15.5, ka * 15.4, ka * 16.0,
            ka * 1e4, -ka * 1e4, ka * 1e-9, -ka * 1e-30]


def nan_sites(r):
    """(image, row, column, channel, value) planted in the second pass: a NaN in the first image, one at pixel 0 of the second image,
    one in the last channel of the last pixel, and both infinities (which the quantizer clamps: no NaN from them)."""
    nan, inf = float("nan"), float("inf")
    return ((0, min(1, r.h - 1), min(5, r.w - 1), 1 % r.c_in, nan), (1, 0, 0, 0, nan), (r.n - 1, r.h - 1, r.w - 1, r.c_in - 1, -nan),
            (0, r.h // 2, r.w // 2, 0, inf), (1, r.h - 1, 0, r.c_in // 2, -inf))


def make_inputs(r):
    """Seeded numpy inputs of a geometry key: x (NHWC, signed, the specials scattered over it), x_nan (x with nan_sites planted),
    w [O, C / groups, KH, KW], bias, scale, shift [O].  Every row of the same geometry gets the same arrays."""
    import numpy as np
    rng = np.random.default_rng(7000 + 7 * r.c_in + 131 * r.n + 17 * r.h + r.w + 1009 * r.c_out + 13 * r.k[0] + r.k[1])
    x = (rng.standard_normal((r.n, r.h, r.w, r.c_in)) * (4.0 * KA)).astype(np.float32)
    vals = np.array(specials(), dtype=np.float32)
    k = min(x.size // 4, 4 * len(vals) + 3)
    pos = rng.permutation(x.size)[:k]
    x.reshape(-1)[pos] = vals[np.arange(k) % len(vals)]
    x_nan = x.copy()
    for img, row, col, ch, v in nan_sites(r):
        x_nan[img, row, col, ch] = v
    w = (rng.standard_normal((r.c_out, r.c_in // r.groups) + r.k) * (5.0 * KW)).astype(np.float32)
    bias = (rng.standard_normal(r.c_out) * 0.3).astype(np.float32)
    scale = (rng.random(r.c_out) + 0.5).astype(np.float32)
    scale[1::2] *= -1.0
    shift = (rng.standard_normal(r.c_out) * 0.3).astype(np.float32)
    return x, x_nan, w, bias, scale, shift


def make_desc(lib, r, ka=KA, kw_scale=KW):
    import numpy as np
    return lib.ConvDesc(n=r.n, c_in=r.c_in, h=r.h, w=r.w, c_out=r.c_out, kh=r.k[0], kw=r.k[1], stride_h=r.stride[0], stride_w=r.stride[1],
                        pad_h=r.pad[0], pad_w=r.pad[1], dil_h=r.dil[0], dil_w=r.dil[1], groups=r.groups, x_layout=lib.LAYOUT_NHWC,
                        y_layout=lib.LAYOUT_NHWC, qbits=r.qbits, ka=float(np.float32(ka)), kw_scale=float(np.float32(kw_scale)),
                        mfma_passes=r.passes, reserved=0)


def make_io(lib, iface, y_qbits, y_ka=KA_NEXT):
    import numpy as np
    if iface in ("f32", "post"):
        return None
    return lib.ConvIo(x_codes=0, y_codes=1, y_ka=float(np.float32(y_ka)), y_qbits=y_qbits)


def instance(lib, d, iface, bias, post, flags, y_qbits, y_ka=KA_NEXT):
    """slfp_debug_stem_instance for descriptor `d` called through interface `iface`"""
    import ctypes
    io = make_io(lib, iface, y_qbits, y_ka)
    return lib.load().slfp_debug_stem_instance(ctypes.byref(d), ctypes.byref(io) if io is not None else None, int(bias), int(flags),
                                               int(post)).decode()


def set_switches(L, env):
    """Leave exactly `env` (a dict or a tuple of pairs; None: nothing) of the stem switches set and have the library re-read them."""
    import os
    for k in SWITCHES:
        os.environ.pop(k, None)
    for k, v in dict(env or ()).items():
        assert k in SWITCHES, k
        os.environ[k] = v
    L.slfp_debug_reload_switches()


def f16_reference(r, x, w, bias, scale, shift, so):
    """The fp16 kernels' operand-level reference, in numpy from the oracle's quantizers: x16 = float16(16 QA(x / Ka)), w16 =
    float16(16 QW(w / Kw)), contracted in float64, divided by 256, then the stated epilogue in float64 -- ((acc + (bias / Ka) / Kw) Ka)
    Kw, the affine, the ReLU (no layer-output quantizer: a discontinuity).  x: NHWC; returns (reference, sum of |terms|), NHWC
    float64: the terms are the products, the bias term and the affine's shift, each at the magnitude it has in the result."""
    import numpy as np
    fa, fw = (so.FMT_ACT8, so.FMT_W8) if r.qbits == 8 else (so.FMT_SFP7, so.FMT_SFP7)
    with np.errstate(invalid="ignore", over="ignore"):
        x16 = (so.quantize(x, np.float32(KA), fa) * np.float32(16.0)).astype(np.float16).astype(np.float64)
        w16 = (so.quantize(w, np.float32(KW), fw) * np.float32(16.0)).astype(np.float16).astype(np.float64)
    ho, wo = out_hw(r)
    (kh_, kw_), (sh, sw), (ph, pw) = r.k, r.stride, r.pad
    assert r.groups == 1 and r.dil == (1, 1)
    xp = np.pad(x16, ((0, 0), (ph, ph), (pw, pw), (0, 0)))
    acc = np.zeros((r.n, ho, wo, r.c_out))
    mag = np.zeros((r.n, ho, wo, r.c_out))
    with np.errstate(invalid="ignore"):
        for kh in range(kh_):
            for kw in range(kw_):
                win = xp[:, kh:kh + (ho - 1) * sh + 1:sh, kw:kw + (wo - 1) * sw + 1:sw, :]
                wk = w16[:, :, kh, kw].T   # [C, O]
                acc += win @ wk
                mag += np.abs(win) @ np.abs(wk)
    acc /= 256.0
    mag /= 256.0
    ka, kws = float(np.float32(KA)), float(np.float32(KW))
    if r.bias:
        bq = ((bias / np.float32(KA)) / np.float32(KW)).astype(np.float64)
        acc, mag = acc + bq, mag + np.abs(bq)
    t, mag = (acc * ka) * kws, mag * (ka * kws)
    if r.post:
        t, mag = t * scale.astype(np.float64) + shift.astype(np.float64), mag * np.abs(scale.astype(np.float64)) + np.abs(shift.astype(np.float64))
    if r.flags & RELU:
        with np.errstate(invalid="ignore"):
            t = np.where(np.isnan(t), 0.0, np.maximum(t, 0.0))   # fmaxf(NaN, 0) = 0; 1-Lipschitz: the bound carries over
    return t, mag


def f16_bound(r, mag):
    """2 (K + 4) 2^-24 sum|terms| per element: K products accumulated in float32, the bias addition, two rescales and the affine's fma
    make K + 4 roundings, each at most 2^-24 of a partial result that the sum of |terms| bounds; the factor 2 because the matrix
    cores' internal additions are not specified to round to nearest."""
    return 2.0 * (taps(r) + 4) * 2.0 ** -24 * mag
