"""Small ragged cases for every backward kernel instance of csrc/conv_bwd.hip, shared by tests/test_bwd_variants_host.py (the table
reaches what it claims, is exactly the set the launchers can select, covers the census of layer_specs, every named edge is recomputed
from the reporter's numbers, the float64 reference of every row is usable) and tests/test_gpu_bwd_variants.py (each row through the
C ABI against that reference, codes and the long form bit for bit against the table launch, guard bands, every `need` subset, NaN
placement, twice).

A row = the descriptor fields, n, qbits, the operand form ("f32": slfp_conv2d_bwd_ex, "codes": slfp_conv2d_bwd_codes), the switches
to set (SLFP_LONG_ENCODE), the flags, the byte offset of the code tensor past a 16-byte boundary, the string slfp_debug_bwd_instance
must report for gx + gw with the split numbers stripped (strip()), and the edges the row hits, each named in a word.  The grammar
(include/slfp.h; one word per template argument a launcher chooses, then the runtime split):

    dw/s<1|2>/<tab|long|codes>/<act8|sfp7>/b<blocks>                              k_dw3x3_bwd<S, AF>
    pw/gx/tm<1|2>tn<1|2>/<v4|v1>                                                  k_gemm_f32<TM, TN, false, kNoEnc, VEC>
    pw/gw/tm<1|2>tn<1|2>/<v4|v1>/<tab|long|codes>/<act8|sfp7>/p<splits>k<kps>     k_gemm_f32<TM, TN, true, AF, VEC>
    dense/gx/tn<1|2>/<v4|v1>                                                      k_dense_gx<TN, VEC>
    dense/gw/tm<1|2>tn<1|2>/<v4|v1>/<tab|long|codes>/<act8|sfp7>/p<splits>k<kps>  k_dense_gw<TM, TN, AF, VEC>

What the launchers can select (reachable()): the depthwise kernel 2 strides x 5 encodes = 10 instances; pointwise gx TM x TN x VEC = 8
and gw the same x 5 encodes = 40; dense gx 3 (the scalar form exists at TN = 1 only) and gw 4 x 5 vector + 5 scalar = 25.  The `tab`
instance serves both formats with different table contents, so the strings carry the format there too: 12 + 8 + 48 + 3 + 30 strings.
Codes need C_in % 4 == 0, so a scalar (v1) codes instance has C_out % 4 != 0.

Shapes, and the edges they hit (edge_holds() below holds the predicate of every word; the host test evaluates it on the reported p, k, b).

Pointwise, one layer per (tm_w, tn_w, vec) in all six forms; tm_w = 1 layers at M = 126 (tm_x = 1), tm_w = 2 at M = 130 (tm_x = 2):
    68 -> 124, 124 -> 132, 132 -> 68, 132 -> 140           one past / short of a 64 or 128 tile on each GEMM side; float4 loads
    8 -> 10, 68 -> 130, 132 -> 10, 132 -> 130              C_out % 4 != 0: scalar gy loads next to the dword code load
  edges: 6 -> 10 and 130 -> 6 (C_in % 4 != 0); 68 -> 124 at M = 2*17*17 = 578 (two splits, a short last one, a partial last k-step,
    kb off the 64-row tile), float32 and codes; 8 -> 8 at M = 2*55*163 (P >= 65, P % 64 != 0); 6 -> 10 at M = 2*50*53 (16 <= P < 64,
    the reduction's columns no multiple of 16); 68 -> 124 and 132 -> 10 at h = w = 1, n = 5 (Linear_Q's form); codes 4 bytes past a
    16-byte boundary.
Dense, one layer per (tm_w, tn_w) in all six forms, and the scalar layer 8 -> 10:
    12 -> 20 3x3 s1 p1 @7x6       C_out % 16 != 0: a tap seam inside a 16-deep chunk of k_dense_gx
    12 -> 132 3x3 s2 p1 @7x9      stride-2 phases of odd extents
    16 -> 24 3x3 s3 p1 @11x8      stride-3 phases; ncol = 144: tn_w = 2 with one ragged tile
    132 -> 132 3x3 s1 p1 @5x6     tn_x = 2; both GEMM sides one past a 128 tile
  edges: 6 -> 10 (scalar x gather); 1x1 stride 2 at 7x6 (three empty phases: gx there is exact zeros by design, rows marked `zeros`),
    float32 and codes; the 7x7 stride-2 stem 3 -> 16 @17x15; 5x5 pad 2; (2, 1) strides; 68 -> 132 @5x4 (ragged tiles); 6 -> 10 and
    8 -> 12 @17x17 (M = 578: two splits through the OIHW scatter of k_reduce_parts, ragged columns), float32 and codes; 4 -> 4
    3x3 @50x53 (16 <= P < 64) and 4 -> 4 1x1 stride 2 @110x326 (P >= 65, P % 64 != 0); codes 4 and 8 bytes past a 16-byte boundary.
Depthwise, C = 36 (36 * 7 = 252 lanes: idle lanes) @7x5 at both strides in all six forms:
  edges: C in {3, 6, 36, 64, 100, 116} (idle lanes; dead channels in the last blockIdx.y) on float32 and, where C % 4 == 0, codes;
    Ho % 4 and Wo % 8 non-zero; 3 x 5 (smaller than a unit); stride 2 at even / odd H and W independently; H = 1 (the kh = 0 and
    kh = 2 taps only ever meet padding: exact zeros, `zeros`); C = 64 @5x3 with n = 2050 (units > gridDim.x * rows: the grid-stride
    walk; 1024 partials through the reduction); C = 8 @9x17 n = 70 (16 <= P < 64) and n = 249 (P >= 65, P % 64 != 0)."""
import functools
import re
from collections import namedtuple
from types import SimpleNamespace

Row = namedtuple("Row", "name kind c_in c_out k stride pad n h w qbits operand env flags align variant edges zeros")

SWITCHES = ("SLFP_LONG_ENCODE",)
LONG = (("SLFP_LONG_ENCODE", "1"),)
DENSE = 1   # SLFP_BWD_DENSE
FORMS = ("tab", "long", "codes")
KA, KW = 0.2, 0.1
ROWS = []


def _fmt(qbits):
    return "act8" if qbits == 8 else "sfp7"


def _two(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _add(name, kind, c_in, c_out, k, stride, pad, n, h, w, gx, gw, form="tab", qbits=8, edges=("instance",), align=0, zeros=False):
    """gx / gw: the instance words the row claims ("tm1tn1/v4"; dw: the stride word alone)."""
    assert form in FORMS and kind in ("dw", "pw", "dense")
    enc = f"{form}/{_fmt(qbits)}"
    if kind == "dw":
        variant = f"dw/{gw}/{enc}"
    else:
        variant = f"{kind}/gx/{gx}+{kind}/gw/{gw}/{enc}"
    ROWS.append(Row(name, kind, c_in, c_out, _two(k), _two(stride), _two(pad), n, h, w, qbits, "codes" if form == "codes" else "f32",
                    LONG if form == "long" else (), DENSE if kind == "dense" else 0, align, variant, tuple(edges), zeros))


def _six(name, *args, edges=("instance",), **kw):
    """The layer in all six activation forms: table, long form and codes, in both formats."""
    for form in FORMS:
        for q in (8, 7):
            _add(f"{name}-{form}-{_fmt(q)}", *args, form=form, qbits=q, edges=edges, **kw)


def _tt(tm, tn, vec):
    return f"tm{tm}tn{tn}/{'v4' if vec else 'v1'}"


# =============================================================================== pointwise / Linear_Q
# (c_in, c_out, n, h, w): tm_w = 1 layers at M = 126, tm_w = 2 layers at M = 130, so that tm_x takes both values for every (tn, vec)
_PW_BASE = {(1, 1, True): (68, 124), (2, 1, True): (124, 132), (1, 2, True): (132, 68), (2, 2, True): (132, 140),
            (1, 1, False): (8, 10), (2, 1, False): (68, 130), (1, 2, False): (132, 10), (2, 2, False): (132, 130)}
for (_tm, _tn, _v), (_ci, _co) in _PW_BASE.items():
    _n, _h, _w = (3, 6, 7) if _tm == 1 else (2, 5, 13)
    _six(f"pw-{_ci}x{_co}", "pw", _ci, _co, 1, 1, 0, _n, _h, _w, _tt(_tm, _tn, _v), _tt(_tm, _tn, _v),
         edges=("ragged-co", "ragged-ci", "m-under-128" if _tm == 1 else "m-over-128", "red-gb-ragged"))
_add("pw-6x10", "pw", 6, 10, 1, 1, 0, 3, 6, 7, _tt(1, 1, False), _tt(1, 1, False), edges=("cin-scalar", "m-under-128"))
_add("pw-130x6", "pw", 130, 6, 1, 1, 0, 2, 5, 13, _tt(2, 2, False), _tt(1, 2, False), edges=("cin-scalar", "ragged-ci", "m-over-128"))
_add("pw-6x10-sfp7-long", "pw", 6, 10, 1, 1, 0, 2, 5, 13, _tt(2, 1, False), _tt(1, 1, False), form="long", qbits=7, edges=("cin-scalar",))
for _form, _q in (("tab", 8), ("codes", 8), ("codes", 7), ("long", 7)):
    _add(f"pw-68x124-m578-{_form}-{_fmt(_q)}", "pw", 68, 124, 1, 1, 0, 2, 17, 17, _tt(2, 1, True), _tt(1, 1, True), form=_form, qbits=_q,
         edges=("short-split", "partial-kstep", "kb-off-tile", "red-p<16", "ragged-rows"))
_add("pw-132x130-m578-codes", "pw", 132, 130, 1, 1, 0, 2, 17, 17, _tt(2, 2, False), _tt(2, 2, False), form="codes",
     edges=("short-split", "partial-kstep", "red-ncols-ragged"))
_add("pw-8x8-p65", "pw", 8, 8, 1, 1, 0, 2, 55, 163, _tt(2, 1, True), _tt(1, 1, True), edges=("red-p65+", "short-split", "partial-kstep"))
_add("pw-8x8-p65-codes", "pw", 8, 8, 1, 1, 0, 2, 55, 163, _tt(2, 1, True), _tt(1, 1, True), form="codes", qbits=7, edges=("red-p65+",))
_add("pw-6x10-p20", "pw", 6, 10, 1, 1, 0, 2, 50, 53, _tt(2, 1, False), _tt(1, 1, False), edges=("red-p16-63", "red-ncols-ragged"))
_add("pw-8x10-p20-codes", "pw", 8, 10, 1, 1, 0, 2, 50, 53, _tt(2, 1, False), _tt(1, 1, False), form="codes", edges=("red-p16-63",))
_add("pw-linear-68x124", "pw", 68, 124, 1, 1, 0, 5, 1, 1, _tt(1, 1, True), _tt(1, 1, True), edges=("linear", "partial-kstep"))
_add("pw-linear-132x10-codes", "pw", 132, 10, 1, 1, 0, 5, 1, 1, _tt(1, 2, False), _tt(1, 2, False), form="codes", edges=("linear",))
_add("pw-linear-132x140-sfp7", "pw", 132, 140, 1, 1, 0, 5, 1, 1, _tt(1, 2, True), _tt(2, 2, True), qbits=7, edges=("linear", "ragged-co"))
_add("pw-68x124-codes-off4", "pw", 68, 124, 1, 1, 0, 3, 6, 7, _tt(1, 1, True), _tt(1, 1, True), form="codes", align=4, edges=("codes-off4",))
_add("pw-132x130-codes-off12", "pw", 132, 130, 1, 1, 0, 2, 5, 13, _tt(2, 2, False), _tt(2, 2, False), form="codes", qbits=7, align=12,
     edges=("codes-off4",))

# =============================================================================== dense
# (tm_w, tn_w) -> (c_in, c_out, stride, n, h, w), all 3x3 pad 1
_DENSE_BASE = {(1, 1): (12, 20, 1, 3, 7, 6), (2, 1): (12, 132, 2, 2, 7, 9), (1, 2): (16, 24, 3, 2, 11, 8), (2, 2): (132, 132, 1, 2, 5, 6)}
for (_tm, _tn), (_ci, _co, _s, _n, _h, _w) in _DENSE_BASE.items():
    _six(f"dense-{_ci}x{_co}-s{_s}", "dense", _ci, _co, 3, _s, 1, _n, _h, _w, f"tn{2 if _ci >= 128 else 1}/v4", _tt(_tm, _tn, True),
         edges=("ragged-co", "ragged-ci") + (("tap-seam",) if _co % 16 else ()) + (("odd-phases",) if _s > 1 else ()))
_six("dense-8x10-scalar", "dense", 8, 10, 3, 1, 1, 3, 7, 6, "tn1/v1", _tt(1, 1, False), edges=("tap-seam", "ragged-co"))
_add("dense-6x10", "dense", 6, 10, 3, 1, 1, 3, 7, 6, "tn1/v1", _tt(1, 1, False), edges=("cin-scalar", "tap-seam"))
_add("dense-6x10-s2-long-sfp7", "dense", 6, 10, 3, 2, 1, 2, 9, 7, "tn1/v1", _tt(1, 1, False), form="long", qbits=7, edges=("cin-scalar", "odd-phases"))
for _form, _q in (("tab", 8), ("codes", 8), ("codes", 7)):
    _add(f"dense-1x1s2-8x12-{_form}-{_fmt(_q)}", "dense", 8, 12, 1, 2, 0, 3, 7, 6, "tn1/v4", _tt(1, 1, True), form=_form, qbits=_q,
         edges=("empty-phases", "tap-seam"), zeros=True)
_add("dense-1x1s2-6x10-odd", "dense", 6, 10, 1, 2, 0, 2, 7, 9, "tn1/v1", _tt(1, 1, False), edges=("empty-phases", "cin-scalar"), zeros=True)
_add("dense-stem7x7-3x16", "dense", 3, 16, 7, 2, 3, 2, 17, 15, "tn1/v1", _tt(1, 1, False), edges=("stem", "odd-phases", "cin-scalar"))
_add("dense-stem7x7-3x16-sfp7", "dense", 3, 16, 7, 2, 3, 2, 17, 15, "tn1/v1", _tt(1, 1, False), qbits=7, edges=("stem",))
_add("dense-5x5p2-8x12", "dense", 8, 12, 5, 1, 2, 2, 6, 7, "tn1/v4", _tt(1, 2, True), edges=("tap-seam", "ragged-ci"))
_add("dense-3x3s21-12x20", "dense", 12, 20, 3, (2, 1), (1, 1), 2, 9, 6, "tn1/v4", _tt(1, 1, True), edges=("odd-phases", "tap-seam"))
_add("dense-3x3s3-16x16-odd", "dense", 16, 16, 3, 3, 1, 2, 11, 13, "tn1/v4", _tt(1, 2, True), edges=("odd-phases",))
_add("dense-68x132", "dense", 68, 132, 3, 1, 1, 2, 5, 4, "tn1/v4", _tt(2, 2, True), edges=("ragged-co", "ragged-ci", "tap-seam"))
_add("dense-68x132-codes", "dense", 68, 132, 3, 1, 1, 2, 5, 4, "tn1/v4", _tt(2, 2, True), form="codes", edges=("ragged-co", "ragged-ci"))
_add("dense-6x10-m578", "dense", 6, 10, 3, 1, 1, 2, 17, 17, "tn1/v1", _tt(1, 1, False),
     edges=("short-split", "partial-kstep", "kb-off-tile", "red-p<16", "red-ncols-ragged", "ragged-rows"))
_add("dense-8x12-m578-codes", "dense", 8, 12, 3, 1, 1, 2, 17, 17, "tn1/v4", _tt(1, 1, True), form="codes", edges=("short-split", "partial-kstep"))
_add("dense-8x10-m578-codes-sfp7", "dense", 8, 10, 3, 1, 1, 2, 17, 17, "tn1/v1", _tt(1, 1, False), form="codes", qbits=7,
     edges=("short-split", "partial-kstep", "tap-seam"))
_add("dense-4x4-p20", "dense", 4, 4, 3, 1, 1, 2, 50, 53, "tn1/v4", _tt(1, 1, True), edges=("red-p16-63",))
_add("dense-4x4-1x1s2-p65", "dense", 4, 4, 1, 2, 0, 2, 110, 326, "tn1/v4", _tt(1, 1, True), edges=("red-p65+", "empty-phases"), zeros=True)
_add("dense-12x20-codes-off4", "dense", 12, 20, 3, 1, 1, 3, 7, 6, "tn1/v4", _tt(1, 1, True), form="codes", align=4, edges=("codes-off4",))
_add("dense-8x10-codes-off8", "dense", 8, 10, 3, 1, 1, 3, 7, 6, "tn1/v1", _tt(1, 1, False), form="codes", qbits=7, align=8, edges=("codes-off4",))

# =============================================================================== depthwise 3x3, pad 1
for _s in (1, 2):
    _six(f"dw-c36-s{_s}", "dw", 36, 36, 3, _s, 1, 3, 7, 5, None, f"s{_s}", edges=("idle-lanes",) + (("unit-ragged",) if _s == 1 else ()))
_DW_GEOMS = ((3, 7, 5), (2, 3, 5), (3, 6, 7), (2, 7, 6), (2, 6, 6), (3, 7, 7), (2, 1, 9), (2, 9, 13))   # (n, h, w)
_k = 0
for _c in (3, 6, 36, 64, 100, 116):
    for _s in (1, 2):
        for _j in range(2):
            _n, _h, _w = _DW_GEOMS[_k % len(_DW_GEOMS)]
            _k += 1
            _e = (("idle-lanes",) if 256 // min(_c, 64) * min(_c, 64) < 256 else ()) + (("dead-channels",) if _c > 64 else ())
            _e += (("small-image",) if (_h, _w) == (3, 5) else ()) + (("h1",) if _h == 1 else ())
            _e += (("unit-ragged",) if (_h, _w) in ((7, 5), (9, 13)) and _s == 1 else ())
            _add(f"dw-c{_c}-s{_s}-{_h}x{_w}", "dw", _c, _c, 3, _s, 1, _n, _h, _w, None, f"s{_s}", qbits=8 if _j == 0 else 7,
                 edges=_e or ("channels",), zeros=_h == 1)
for _c, _s, _q, _al in ((100, 1, 8, 0), (116, 2, 7, 0), (64, 2, 8, 0), (100, 2, 8, 4), (36, 1, 7, 12)):
    _add(f"dw-c{_c}-s{_s}-codes-{_fmt(_q)}-off{_al}", "dw", _c, _c, 3, _s, 1, 2, 6, 7, None, f"s{_s}", form="codes", qbits=_q, align=_al,
         edges=(("dead-channels",) if _c > 64 else ()) + (("codes-off4",) if _al else ()) or ("channels",))
for _s in (1, 2):   # stride 2 with H and W even / odd independently; stride 1 on the same images
    for _h, _w in ((6, 8), (6, 9), (7, 8), (7, 9)):
        _add(f"dw-c8-s{_s}-{_h}x{_w}", "dw", 8, 8, 3, _s, 1, 2, _h, _w, None, f"s{_s}", edges=("parity",))
_add("dw-c64-5x3-n2050", "dw", 64, 64, 3, 1, 1, 2050, 5, 3, None, "s1", edges=("units>slots", "red-p65+x64"))
_add("dw-c64-5x3-n2050-codes", "dw", 64, 64, 3, 1, 1, 2050, 5, 3, None, "s1", form="codes", edges=("units>slots",))
_add("dw-c8-9x17-n70", "dw", 8, 8, 3, 1, 1, 70, 9, 17, None, "s1", edges=("red-p16-63", "unit-ragged"))
_add("dw-c8-9x17-n249", "dw", 8, 8, 3, 1, 1, 249, 9, 17, None, "s1", qbits=7, edges=("red-p65+",))

del _tm, _tn, _v, _ci, _co, _n, _h, _w, _s, _form, _q, _c, _j, _k, _e, _al


# =============================================================================== geometry, reporter, reachable set
def out_hw(r):
    return tuple((e + 2 * p - k) // s + 1 for e, p, k, s in zip((r.h, r.w), r.pad, r.k, r.stride))


def layer_key(r):
    """Rows with the same layer key share inputs and the float64 reference; every form of the layer must give the same bits."""
    return (r.kind, r.c_in, r.c_out, r.k, r.stride, r.pad, r.n, r.h, r.w, r.qbits)


def make_desc(lib, r):
    import numpy as np
    return lib.ConvDesc(n=r.n, c_in=r.c_in, h=r.h, w=r.w, c_out=r.c_out, kh=r.k[0], kw=r.k[1], stride_h=r.stride[0], stride_w=r.stride[1],
                        pad_h=r.pad[0], pad_w=r.pad[1], dil_h=1, dil_w=1, groups=r.c_in if r.kind == "dw" else 1,
                        x_layout=lib.LAYOUT_NHWC, y_layout=lib.LAYOUT_NHWC, qbits=r.qbits, ka=float(np.float32(KA)),
                        kw_scale=float(np.float32(KW)), mfma_passes=0, reserved=0)


def instance(lib, d, flags, x_codes, need_gx=1, need_gw=1):
    import ctypes
    return lib.load().slfp_debug_bwd_instance(ctypes.byref(d), flags, int(x_codes), int(need_gx), int(need_gw)).decode()


_NUM = re.compile(r"/(?:p\d+k\d+|b\d+)$")


def strip(s):
    """The instance words of a reporter string: every part without its /p<splits>k<kps> or /b<blocks>."""
    return "+".join(_NUM.sub("", part) for part in s.split("+"))


def numbers(s):
    """{'p': splits, 'k': kps} or {'b': blocks} of a reporter string."""
    m = re.search(r"/(?:p(\d+)k(\d+)|b(\d+))$", s)
    return {"b": int(m.group(3))} if m.group(3) else {"p": int(m.group(1)), "k": int(m.group(2))}


def reachable():
    """Every kernel string (split numbers stripped) the launchers of csrc/conv_bwd.hip can select, from the grammar and the rules of
    pw_shape / dense_shape / with_act_enc: the scalar dense forms exist at tn_x = 1 and tm_w = tn_w = 1 only."""
    encs = [f"{f}/{q}" for f in FORMS for q in ("act8", "sfp7")]
    tiles = [(tm, tn) for tm in (1, 2) for tn in (1, 2)]
    out = {f"dw/s{s}/{e}" for s in (1, 2) for e in encs}
    out |= {f"pw/gx/tm{tm}tn{tn}/{v}" for tm, tn in tiles for v in ("v4", "v1")}
    out |= {f"pw/gw/tm{tm}tn{tn}/{v}/{e}" for tm, tn in tiles for v in ("v4", "v1") for e in encs}
    out |= {"dense/gx/tn1/v4", "dense/gx/tn2/v4", "dense/gx/tn1/v1"}
    out |= {f"dense/gw/tm{tm}tn{tn}/v4/{e}" for tm, tn in tiles for e in encs}
    out |= {f"dense/gw/tm1tn1/v1/{e}" for e in encs}
    return out


def set_switches(L, env):
    """Leave exactly `env` (a dict or a tuple of pairs; None: nothing) of the switches set and have the library re-read them."""
    import os
    for k in SWITCHES:
        os.environ.pop(k, None)
    for k, v in dict(env or ()).items():
        assert k in SWITCHES, k
        os.environ[k] = v
    L.slfp_debug_reload_switches()


# =============================================================================== the edges, recomputed
def _cdiv(a, b):
    return -(-a // b)


def _tiles(r):
    """(tm_x, tn_x, tm_w, tn_w) as the row's claimed strings say."""
    gx, gw = r.variant.split("+")
    mx = re.search(r"(?:tm(\d))?tn(\d)", gx)
    mw = re.search(r"tm(\d)tn(\d)", gw)
    return int(mx.group(1) or 2), int(mx.group(2)), int(mw.group(1)), int(mw.group(2))   # k_dense_gx: TM = 2


def edge_holds(r, word, nums):
    """Whether row `r` hits the edge `word`, from its descriptor fields and the numbers the reporter gave (p, k / b)."""
    ho, wo = out_hw(r)
    if r.kind == "dw":
        c, b = r.c_in, nums["b"]
        cw = min(c, 64)
        rows = 256 // cw
        units = r.n * _cdiv(ho, 4) * _cdiv(wo, 8)
        P = b
        pred = {
            "idle-lanes": cw * rows < 256, "dead-channels": c > 64 and c % 64 != 0, "channels": True, "parity": True,
            "unit-ragged": ho % 4 != 0 and wo % 8 != 0, "small-image": r.h < 4 and r.w < 8, "h1": r.h == 1,
            "units>slots": units > b * rows, "codes-off4": r.align % 4 == 0 and r.align % 16 != 0 and r.operand == "codes",
            "red-p16-63": 16 <= P < 64, "red-p65+": P >= 65 and P % 64 != 0, "red-p65+x64": P >= 65, "instance": True,
        }
        return pred[word]
    p, k = nums["p"], nums["k"]
    tm_x, tn_x, tm_w, tn_w = _tiles(r)
    m_x = r.n * r.h * r.w                       # gx rows
    m_w = r.n * ho * wo                         # rows the gw contraction runs over
    ncol = r.k[0] * r.k[1] * r.c_in
    last = m_w - (p - 1) * k                    # rows of the last split
    pred = {
        "instance": True, "ragged-co": r.c_out % (64 * tm_w) != 0, "ragged-ci": ncol % (64 * tn_w) != 0 and r.c_in % (64 * tn_x) != 0,
        "ragged-rows": m_x % (64 * tm_x) != 0, "m-under-128": 64 < m_x < 128, "m-over-128": 128 < m_x < 192,
        "short-split": p > 1 and 0 < last < k, "partial-kstep": last % 16 != 0, "kb-off-tile": p > 1 and k % 64 != 0,
        "red-p<16": 1 < p < 16, "red-p16-63": 16 <= p < 64, "red-p65+": p >= 65 and p % 64 != 0,
        "red-ncols-ragged": p > 1 and (r.c_out * ncol) % 16 != 0, "red-gb-ragged": r.c_out % 16 != 0,
        "cin-scalar": r.c_in % 4 != 0, "linear": r.h == 1 and r.w == 1 and r.kind == "pw", "tap-seam": r.c_out % 16 != 0,
        "odd-phases": max(r.stride) > 1 and any(e % s != 0 for e, s in zip((r.h, r.w), r.stride) if s > 1),
        "empty-phases": r.k == (1, 1) and r.stride == (2, 2), "stem": r.c_in == 3 and r.k == (7, 7),
        "codes-off4": r.align % 4 == 0 and r.align % 16 != 0 and r.operand == "codes",
    }
    return pred[word]


# =============================================================================== inputs and the float64 reference
def module_of(r):
    """What _bwd_cases._reference reads of a module."""
    return SimpleNamespace(q_bit=r.qbits, Ka=KA, Kw=KW, stride=r.stride, padding=r.pad, dilation=(1, 1),
                           groups=r.c_in if r.kind == "dw" else 1)


@functools.lru_cache(maxsize=None)
def _layer_inputs(key):
    import torch
    from _bwd_cases import _x_values
    kind, c_in, c_out, k, stride, pad, n, h, w, qbits = key
    ho, wo = ((e + 2 * p - kk) // s + 1 for e, p, kk, s in zip((h, w), pad, k, stride))
    gen = torch.Generator().manual_seed(4200 + 131 * c_in + 17 * c_out + 7 * n + 3 * h + w + qbits + 1000 * k[0] + 11 * stride[0])
    x = _x_values((n, c_in, h, w), KA, gen)
    fan = (1 if kind == "dw" else c_in) * k[0] * k[1]
    wt = torch.randn((c_out, 1 if kind == "dw" else c_in, k[0], k[1]), generator=gen) * (2.0 / fan) ** 0.5
    gy = torch.randn((n, c_out, ho, wo), generator=gen)
    return x, wt, gy


def inputs(r):
    """Seeded CPU inputs of the row's layer, NCHW: (x, w, gy).  x reaches every code range (_bwd_cases._x_values).  Never written."""
    return _layer_inputs(layer_key(r))


@functools.lru_cache(maxsize=None)
def _layer_reference(key, planted):
    import torch
    from _bwd_cases import _reference
    r = next(row for row in ROWS if layer_key(row) == key)
    x, wt, gy = inputs(r)
    if planted:
        x = plant(r, x)
        x = torch.where(torch.isnan(x), torch.zeros_like(x), x)
    return _reference(x, wt, gy, module_of(r))


def reference(r, planted=False):
    """((gx, |gx| terms), (gw, ...), (gb, ...)) in float64, computed once per layer.  planted: of the inputs of plant() with each NaN
    replaced by zero, which is the reference of every gw element the NaNs do not reach."""
    return _layer_reference(layer_key(r), bool(planted))


def nan_sites(r):
    """(image, channel, row, column, value): a NaN in the last channel of the last pixel, one at pixel 0 of the second image, and an
    infinity (which the quantizer clamps: no NaN from it) in the middle of the first."""
    nan, inf = float("nan"), float("inf")
    return ((r.n - 1, r.c_in - 1, r.h - 1, r.w - 1, nan), (1, min(1, r.c_in - 1), 0, 0, nan), (0, r.c_in // 2, r.h // 2, r.w // 2, inf))


def plant(r, x):
    x = x.clone()
    for img, ch, row, col, v in nan_sites(r):
        x[img, ch, row, col] = v
    return x


def nan_mask(r):
    """The gw elements (OIHW) a NaN of nan_sites reaches, from the geometry alone: tap (kh, kw) of input channel ci samples input pixel
    (hi, wi) iff some output position (ho, wo) has ho * stride - pad + kh == hi (and the columns alike)."""
    import torch
    ho, wo = out_hw(r)
    mask = torch.zeros((r.c_out, 1 if r.kind == "dw" else r.c_in, r.k[0], r.k[1]), dtype=torch.bool)
    for _, ch, hi, wi, v in nan_sites(r):
        if v == v:
            continue
        for kh in range(r.k[0]):
            for kw in range(r.k[1]):
                th, tw = hi + r.pad[0] - kh, wi + r.pad[1] - kw
                if th % r.stride[0] or tw % r.stride[1] or not 0 <= th // r.stride[0] < ho or not 0 <= tw // r.stride[1] < wo:
                    continue
                if r.kind == "dw":
                    mask[ch, 0, kh, kw] = True
                else:
                    mask[:, ch, kh, kw] = True
    return mask
