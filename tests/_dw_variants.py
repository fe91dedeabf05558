"""Small ragged cases for every depthwise 3x3 kernel instance (csrc/conv_dw.hip, conv_dw2.hip, conv_dw3.hip, conv_dwc.hip), shared
by tests/test_dw_variants_host.py (the table reaches what it claims and spans what the launchers can select; the workloads' census is
covered by it; the CPU restatement against the double-accumulating oracle) and tests/test_gpu_dw_variants.py (each row bit for bit
against the restatement, guard bands, NaN placement, twice).

A row = the descriptor fields, the interface the layer is called through, bias / post vectors / flags, the switches to set, and the
string slfp_debug_dw3x3_instance must then report.  The grammar (include/slfp.h; one word per template argument a launcher chooses):

    general/s<1|2>/<cb32iw16|cb64iw9|cb32iw15|gen>/v<4|2>/<tab|long>/<act8|sfp7>[/lo]      k_dw3x3<FMT, S, CBT, IWT, V, LO, TAB>
    tile/s<1|2>/<plain|post>                                                              k_dw3x3_tile<S, TH, TW, POST>
    rows/<plain|post>                                                                     k_dw3x3_rows<7, POST>
    dwc/s<1|2>/lc<3|4|5>/<f32|yc|yc-signed|lut>/<plain|post>/<act8|sfp7>                   k_dwc<S, LCS, TH, TW, YC, POST, SIGNED, LUTQ>

Interfaces: "f32" slfp_conv2d_fwd (no post vectors, no flags); "post" slfp_conv2d_fwd_post; "cin" / "cout" slfp_conv2d_fwd_codes with
float32 / code output; "lut" slfp_conv2d_fwd_codes_lut.  flags: 1 = SLFP_POST_RELU, 2 = SLFP_POST_LAYEROUT.

Shapes, and the edge each one hits (n = 2 or 3 throughout, so tiles, tasks and waves cross the image boundary).

k_dw3x3_tile, stride 1 (14 x 14 tiles, 32-channel groups; refuses Ho <= 7 and Wo <= 7 together):
    15 x 17 pad 1 -> 15 x 17   2 x 2 tiles with a 1-row and a 3-column remainder (both axes ragged); n = 3: 12 workgroups
    17 x 16 pad 0 -> 15 x 14   an exactly full tile across, a 1-row remainder down; C = 64: two channel groups
    12 x 13 pad 2 -> 14 x 15   pad 2; exactly full down, a 1-column remainder across
    8 x 3 pad 1 -> 8 x 3       just over the rule on one axis only; one tile per image: 2 workgroups
    10 x 16 pad 1, C = 96      three channel groups; 12 workgroups
k_dw3x3_tile, stride 2 (SLFP_DW_ROWS=0; 7 x 7 tiles):
    15 x 29 pad 1 -> 8 x 15    a 1-row and a 1-column remainder (2 x 3 tiles)
    15 x 15 pad 0 -> 7 x 7     exactly one tile
    9 x 12 pad 2 -> 6 x 7      pad 2, a short tile down
k_dw3x3_rows: four of _dw_rows_worker.ODD_GEOMS (ragged tiles, pad 0 / 1 / 2, C = 32 / 64 / 96, an image smaller than a tile, idle
    waves in the last workgroup), unswitched and under SLFP_DW_ROWS=15.
k_dw3x3 (the channel-group rule of dw_select: CB = the largest power-of-two multiple of 4 up to 64 dividing C, 32 with a ragged last
group when that is below 32, halved while the halo tile exceeds 40 KiB; TH / TW = min(Ho / Wo, 14 | 7); IW = (TW - 1) S + 3):
    cb32iw16   C = 32 at 15 x 17 under SLFP_DW_OLD (the tile row's layer: 2 x 2 ragged tiles); C = 96 with a bias and no switch;
               C = 64 at 11 x 16 (Ho >= 9: the 40 KiB cap halves the group); C = 24 and 116 unswitched (c_live false in masked lanes)
    cb64iw9    C = 128 at 5 x 7 pad 1 (Wo == 7, Ho <= 7), unswitched: 4 workgroups
    cb32iw15   stride 2, C = 32 / 96 at Wo >= 7 under SLFP_DW_OLD / with a bias; C = 24 unswitched
    gen        C = 64 at 8 x 14 (CB stays 64 with IW = 16: no specialised instance); C = 64 at 5 x 3 (TW = 3); C = 4, 8, 20;
               stride 2 with TW = 4 and 5 (IW is always odd at stride 2: what alternates is the parity of IWh, the offset of the odd
               de-interleaved columns)
    v2         C = 58 at Wo = 15 (1,32,16,2) and at Wo = 4; C = 6; stride 2
    long / sfp7 / lo   every geometry form under SLFP_LONG_ENCODE and at qbits 7; SLFP_POST_LAYEROUT with the affine for v4 and v2,
               stride 1 and 2, table and long form, both formats
k_dwc (stride 1: a lane walks 7 rows x 2 columns; stride 2: 4 x 1; a block holds 32 / 16 / 8 tasks for C = 32 / 64 / >= 128):
    s1  5 x 5 pad 1, n = 2     6 tasks (12 at C = 256): below one block, most lanes have valid == false; Ho = 5 < TH, Wo odd
    s1  9 x 11 pad 0, n = 3    7 x 9: 15 tasks (no multiple of 32, 16 or 8), Wo odd
    s1  16 x 13 pad 2, n = 3   18 x 15: 72 tasks: 3 / 5 / 9 workgroups (C = 256: 18), Ho = 2 * 7 + 4, Wo odd
    s2  9 x 7 pad 1, n = 2     5 x 4: 16 tasks, Ho = 4 + 1
    s2  11 x 11 pad 0, n = 3   5 x 5: 30 tasks
    s2  13 x 20 pad 2, n = 2   8 x 11: 44 tasks (C = 256: 88 = 11 workgroups)
  each (stride, lane count, output form, input format) takes one of its stride's three shapes in turn; lc5 alternates C = 128 and 256.
xcd_remap: every kernel has a row with fewer than 8 workgroups and one with a count >= 8 that is no multiple of 8 (WORKGROUPS below
names them; the host test recomputes the counts)."""
from collections import namedtuple

Row = namedtuple("Row", "name c stride pad n h w qbits iface bias post flags env y_qbits variant")

IFACES = ("f32", "post", "cin", "cout", "lut")
RELU, LAYEROUT = 1, 2
SWITCHES = ("SLFP_DW_OLD", "SLFP_DW_ROWS", "SLFP_LONG_ENCODE")
OLD, LONG, ROWS0, ROWS15 = {"SLFP_DW_OLD": "1"}, {"SLFP_LONG_ENCODE": "1"}, {"SLFP_DW_ROWS": "0"}, {"SLFP_DW_ROWS": "15"}

ROWS = []


def _add(name, variant, c, h, w, pad=1, stride=1, n=2, iface="f32", bias=False, post=False, flags=0, env=None, qbits=8, y_qbits=None):
    assert iface in IFACES and (iface != "f32" or (not post and not flags))
    ROWS.append(Row(name, c, stride, pad, n, h, w, qbits, iface, bool(bias), bool(post), flags, tuple(sorted((env or {}).items())),
                    y_qbits or qbits, variant))


def _env(*parts):
    out = {}
    for p in parts:
        out.update(p)
    return out


def _fmt(qbits):
    return "act8" if qbits == 8 else "sfp7"


# =============================================================================== k_dw3x3_tile
_TILE_S1 = (("15x17", 32, 15, 17, 1, 3), ("17x16p0", 64, 17, 16, 0, 2), ("12x13p2", 32, 12, 13, 2, 2), ("8x3", 32, 8, 3, 1, 2),
            ("10x16c96", 96, 10, 16, 1, 2))
for _t, _c, _h, _w, _p, _n in _TILE_S1:
    _add(f"tile-s1-{_t}", "tile/s1/plain", _c, _h, _w, _p, n=_n)
    _add(f"tile-s1-{_t}-post", "tile/s1/post", _c, _h, _w, _p, n=_n, iface="post", post=True, flags=RELU)
_add("tile-s1-15x17-relu", "tile/s1/plain", 32, 15, 17, n=3, iface="post", flags=RELU)      # the ReLU alone: a runtime flag
_add("tile-s1-15x17-affine", "tile/s1/post", 32, 15, 17, n=3, iface="post", post=True)      # the affine alone
_add("tile-s1-15x17-sfp7", "tile/s1/plain", 32, 15, 17, n=3, qbits=7)
_TILE_S2 = (("15x29", 32, 15, 29, 1, 2), ("15x15p0", 64, 15, 15, 0, 3), ("9x12p2", 96, 9, 12, 2, 2))
for _t, _c, _h, _w, _p, _n in _TILE_S2:
    _add(f"tile-s2-{_t}", "tile/s2/plain", _c, _h, _w, _p, 2, n=_n, env=ROWS0)
    _add(f"tile-s2-{_t}-post", "tile/s2/post", _c, _h, _w, _p, 2, n=_n, iface="post", post=True, flags=RELU, env=ROWS0)
_add("tile-s2-15x29-sfp7", "tile/s2/post", 32, 15, 29, 1, 2, iface="post", post=True, env=ROWS0, qbits=7)

# =============================================================================== k_dw3x3_rows
_ROWS = ((3, 96, 15, 57, 0), (3, 32, 3, 3, 1), (2, 64, 20, 9, 2), (5, 32, 5, 4, 0))   # of _dw_rows_worker.ODD_GEOMS: (n, c, h, w, pad)
for _n, _c, _h, _w, _p in _ROWS:
    _add(f"rows-n{_n}c{_c}-{_h}x{_w}p{_p}", "rows/plain", _c, _h, _w, _p, 2, n=_n)
    _add(f"rows-n{_n}c{_c}-{_h}x{_w}p{_p}-post", "rows/post", _c, _h, _w, _p, 2, n=_n, iface="post", post=True, flags=RELU)
_add("rows-15x29", "rows/plain", 32, 15, 29, 1, 2)                                              # the stride-2 tile row's layer
_add("rows-15x29-mask15", "rows/plain", 32, 15, 29, 1, 2, env=ROWS15)
_add("rows-15x15p0-mask15-post", "rows/post", 64, 15, 15, 0, 2, n=3, iface="post", post=True, flags=RELU, env=ROWS15)
_add("rows-15x29-sfp7", "rows/post", 32, 15, 29, 1, 2, iface="post", post=True, qbits=7)

# =============================================================================== k_dw3x3
# ---- every instance once: geometry form x lane width, table and long form, both formats.  (c, h, w, pad, stride, n, switch that
# keeps a multiple-of-32 layer off the tile / rows kernels when the table form is wanted; the long form keeps it off by itself)
_GEN_BASE = {
    "s1/cb32iw16/v4": (32, 15, 17, 1, 1, 3, OLD),
    "s1/cb64iw9/v4": (128, 5, 7, 1, 1, 2, None),
    "s2/cb32iw15/v4": (32, 15, 17, 1, 2, 3, OLD),
    "s1/gen/v4": (64, 5, 3, 1, 1, 2, None),
    "s2/gen/v4": (20, 9, 8, 1, 2, 2, None),
    "s1/cb32iw16/v2": (58, 6, 15, 1, 1, 2, None),
    "s1/gen/v2": (58, 7, 6, 0, 1, 3, None),
    "s2/gen/v2": (58, 9, 11, 1, 2, 2, None),
}
for _g, (_c, _h, _w, _p, _s, _n, _sw) in _GEN_BASE.items():
    for _q in (8, 7):
        _add(f"gen-{_g}-tab-{_fmt(_q)}", f"general/{_g}/tab/{_fmt(_q)}", _c, _h, _w, _p, _s, n=_n, env=_sw, qbits=_q)
        _add(f"gen-{_g}-long-{_fmt(_q)}", f"general/{_g}/long/{_fmt(_q)}", _c, _h, _w, _p, _s, n=_n, env=LONG, qbits=_q,
             iface="post", post=True, flags=RELU)
# ---- the fused layer-output quantizer: always the generic geometry, also where the plain launch is specialised (C = 58 at Wo = 15)
_LO_BASE = {"s1/gen/v4": (32, 9, 10, 1, 1, 2), "s1/gen/v2": (58, 6, 15, 1, 1, 2), "s2/gen/v4": (96, 9, 15, 1, 2, 2), "s2/gen/v2": (6, 7, 9, 0, 2, 3)}
for _g, (_c, _h, _w, _p, _s, _n) in _LO_BASE.items():
    for _q in (8, 7):
        _add(f"lo-{_g}-tab-{_fmt(_q)}", f"general/{_g}/tab/{_fmt(_q)}/lo", _c, _h, _w, _p, _s, n=_n, iface="post", post=True,
             flags=LAYEROUT | (RELU if _q == 7 else 0), qbits=_q)
        _add(f"lo-{_g}-long-{_fmt(_q)}", f"general/{_g}/long/{_fmt(_q)}/lo", _c, _h, _w, _p, _s, n=_n, iface="post", post=True,
             flags=LAYEROUT | (RELU if _q == 8 else 0), env=LONG, qbits=_q, bias=(_q == 8))
# ---- the other ways into each geometry form
_add("gen-cb32iw16-c96-bias", "general/s1/cb32iw16/v4/tab/act8", 96, 17, 16, 0, bias=True)                       # 12 workgroups
_add("gen-cb32iw16-c32-bias-post", "general/s1/cb32iw16/v4/tab/act8", 32, 15, 17, n=3, iface="post", bias=True, post=True, flags=RELU)
_add("gen-cb32iw16-c64-cap", "general/s1/cb32iw16/v4/tab/act8", 64, 11, 16, bias=True)                            # Ho = 11: CB 64 -> 32
_add("gen-cb32iw16-c64-cap-old", "general/s1/cb32iw16/v4/tab/act8", 64, 11, 16, env=OLD)
_add("gen-cb32iw16-c24", "general/s1/cb32iw16/v4/tab/act8", 24, 9, 14)                                             # ragged only group
_add("gen-cb32iw16-c116", "general/s1/cb32iw16/v4/tab/act8", 116, 3, 16, n=3)                                      # 3 full groups + 20 channels
_add("gen-cb32iw16-c116-post", "general/s1/cb32iw16/v4/tab/act8", 116, 3, 16, n=3, iface="post", post=True, flags=RELU)
_add("gen-cb64iw9-bias", "general/s1/cb64iw9/v4/tab/act8", 64, 9, 7, bias=True, n=3)                               # Ho = 9: one 9 x 7 tile, IH = 11
_add("gen-cb32iw15-c96-bias", "general/s2/cb32iw15/v4/tab/act8", 96, 13, 15, 0, 2, bias=True)
_add("gen-cb32iw15-c96-old", "general/s2/cb32iw15/v4/tab/act8", 96, 13, 15, 0, 2, env=OLD)
_add("gen-cb32iw15-c24", "general/s2/cb32iw15/v4/tab/act8", 24, 13, 14, 1, 2)
_add("gen-gen-c64-8x14", "general/s1/gen/v4/tab/act8", 64, 8, 14, bias=True)                                       # CB = 64, IW = 16
_add("gen-gen-c64-8x14-old", "general/s1/gen/v4/tab/act8", 64, 8, 14, env=OLD)
for _c in (4, 8, 20):
    _add(f"gen-gen-c{_c}", "general/s1/gen/v4/tab/act8", _c, 6, 7, n=3)
    _add(f"gen-gen-c{_c}-s2", "general/s2/gen/v4/tab/act8", _c, 9, 10, 1, 2, n=3, iface="post", post=True, flags=RELU)   # TW = 5
_add("gen-gen-c64-s2-tw3", "general/s2/gen/v4/tab/act8", 64, 7, 5, 1, 2, bias=True)
_add("gen-gen-c8-s2-tw4-p2", "general/s2/gen/v4/tab/act8", 8, 6, 5, 2, 2)                                          # pad 2: (5 + 4 - 3) / 2 + 1 = 4
_add("gen-v2-c58-wo15-bias", "general/s1/cb32iw16/v2/tab/act8", 58, 6, 15, bias=True, iface="post", post=True)
_add("gen-v2-c6", "general/s1/gen/v2/tab/act8", 6, 5, 9, n=3)
_add("gen-v2-c6-s2", "general/s2/gen/v2/tab/act8", 6, 9, 9, 1, 2, n=3)
_add("gen-v2-c58-p2", "general/s1/gen/v2/tab/act8", 58, 4, 5, 2)
_add("gen-tile-15x17-old-post", "general/s1/cb32iw16/v4/tab/act8", 32, 15, 17, n=3, iface="post", post=True, flags=RELU, env=OLD)
_add("gen-rows-15x29-old", "general/s2/cb32iw15/v4/tab/act8", 32, 15, 29, 1, 2, env=OLD)                           # the rows / tile rows' layer

# =============================================================================== k_dwc
_DWC_SHAPES = {1: ((5, 5, 1, 2), (9, 11, 0, 3), (16, 13, 2, 3)), 2: ((9, 7, 1, 2), (11, 11, 0, 3), (13, 20, 2, 2))}   # (h, w, pad, n)
# output form -> (interface, post vectors, flags)
_DWC_FORMS = (("f32/plain", "cin", False, 0), ("f32/post", "cin", True, RELU), ("yc/plain", "cout", False, RELU), ("yc/post", "cout", True, RELU),
              ("yc-signed/plain", "cout", False, 0), ("yc-signed/post", "cout", True, 0), ("lut/post", "lut", True, LAYEROUT))
_k = 0
for _s in (1, 2):
    for _lc, _cs in ((3, (32, 32)), (4, (64, 64)), (5, (128, 256))):
        for _q in (8, 7):
            for _form, _i, _post, _fl in _DWC_FORMS:
                _h, _w, _p, _n = _DWC_SHAPES[_s][_k % 3]
                _c = _cs[(_k // 3) % 2]
                _add(f"dwc-s{_s}-lc{_lc}-{_form.replace('/', '-')}-{_fmt(_q)}", f"dwc/s{_s}/lc{_lc}/{_form}/{_fmt(_q)}", _c, _h, _w, _p, _s,
                     n=_n, iface=_i, post=_post, flags=_fl, qbits=_q)
                _k += 1
# ---- the runtime words the strings do not carry: the ReLU of the float32 form, the reader's format differing from the layer's
_add("dwc-s1-lc3-f32-relu", "dwc/s1/lc3/f32/plain/act8", 32, 16, 13, 2, n=3, iface="cin", flags=RELU)
_add("dwc-s2-lc5-f32-affine", "dwc/s2/lc5/f32/post/act8", 256, 13, 20, 2, 2, iface="cin", post=True)
_add("dwc-s1-lc5-c256-yc", "dwc/s1/lc5/yc/post/act8", 256, 16, 13, 2, n=3, iface="cout", post=True, flags=RELU)         # 18 workgroups
_add("dwc-s1-lc4-yc-to-sfp7", "dwc/s1/lc4/yc/post/act8", 64, 9, 11, 0, n=3, iface="cout", post=True, flags=RELU, y_qbits=7)
_add("dwc-s1-lc3-signed-to-sfp7", "dwc/s1/lc3/yc-signed/post/act8", 32, 16, 13, 2, n=3, iface="cout", post=True, y_qbits=7)
_add("dwc-s2-lc5-signed-sfp7-to-act8", "dwc/s2/lc5/yc-signed/plain/sfp7", 128, 11, 11, 0, 2, n=3, iface="cout", qbits=7, y_qbits=8)
_add("dwc-s2-lc4-lut-to-sfp7", "dwc/s2/lc4/lut/post/act8", 64, 13, 20, 2, 2, iface="lut", post=True, flags=LAYEROUT, y_qbits=7)
# ---- the layers of the float32-interface rows above, on codes: the same bits
_add("dwc-tile-15x17", "dwc/s1/lc3/f32/plain/act8", 32, 15, 17, n=3, iface="cin")
_add("dwc-tile-15x17-post", "dwc/s1/lc3/f32/post/act8", 32, 15, 17, n=3, iface="cin", post=True, flags=RELU)
_add("dwc-rows-15x29", "dwc/s2/lc3/f32/plain/act8", 32, 15, 29, 1, 2, iface="cin")
_add("dwc-cb64iw9-5x7", "dwc/s1/lc5/f32/plain/act8", 128, 5, 7, iface="cin")

del _t, _c, _h, _w, _p, _n, _g, _q, _s, _sw, _lc, _cs, _form, _i, _post, _fl, _k


def out_hw(r):
    return (r.h + 2 * r.pad - 3) // r.stride + 1, (r.w + 2 * r.pad - 3) // r.stride + 1


def geom_key(r):
    """Rows with the same geometry key share inputs, weights and per-channel vectors."""
    return (r.c, r.n, r.h, r.w)


def layer_key(r):
    """Rows with the same layer key and a float32 output describe the same computation: every kernel, interface and switch must give it
    the same bits."""
    return (r.c, r.stride, r.pad, r.n, r.h, r.w, r.qbits, r.bias, r.post, r.flags)


def workgroups(r):
    """Workgroups the row's launch has, from the launchers' geometry (dw_select, launch_dw3x3_tile, launch_dw3x3_rows, launch_dwc)."""
    ho, wo = out_hw(r)
    kind = r.variant.split("/")[0]
    cdiv = lambda a, b: -(-a // b)   # noqa: E731
    if kind == "tile":
        t = 7 if r.stride == 2 else 14
        return r.n * cdiv(ho, t) * cdiv(wo, t) * (r.c // 32)
    if kind == "rows":
        return cdiv(r.n * cdiv(ho, 7) * cdiv(wo, 7) * (r.c // 32), 4)
    if kind == "dwc":
        lcs = 5 if r.c >= 128 else (4 if r.c == 64 else 3)
        th, tw = (4, 1) if r.stride == 2 else (7, 2)
        return cdiv(r.n * cdiv(ho, th) * cdiv(wo, tw) * (r.c // (4 << lcs)), 256 >> lcs)
    cb = 4
    while cb < 64 and r.c % (cb * 2) == 0:
        cb *= 2
    if cb < 32:
        cb = 4
        while cb < 32 and cb < r.c:
            cb *= 2
    tmax = 14 if r.stride == 1 else 7
    th, tw = min(ho, tmax), min(wo, tmax)
    ih, iw = (th - 1) * r.stride + 3, (tw - 1) * r.stride + 3
    while cb > 4 and ih * iw * cb * 4 > 40 * 1024:
        cb //= 2
    return r.n * cdiv(ho, th) * cdiv(wo, tw) * cdiv(r.c, cb)


KA, KW, KA_NEXT = 0.21, 0.027, 0.2345


def specials(ka=KA):
    """Values written over seeded positions of the input (as _dw_rows_worker.specials): both zeros, the clamps of QA(x / Ka) from both
    sides, the tiny class, and values far beyond the clamp."""
    return [0.0, -0.0, ka * 2.0 ** -5, -ka * 2.0 ** -5, ka * 2.0 ** -6, ka * 2.0 ** -4.9, ka * 15.5, -ka * 15.5, ka * 15.4, ka * 16.0,
            ka * 1e4, -ka * 1e4, ka * 1e-9, -ka * 1e-30]


def nan_sites(r):
    """(image, row, column, channel, value) planted in the second pass: one NaN whose predecessor pixel is clean, one at pixel 0 of the
    second image, one in the last channel of the last pixel, and both infinities (which the quantizer clamps: no NaN from them)."""
    nan, inf = float("nan"), float("inf")
    return ((0, 0, min(2, r.w - 1), 3 % r.c, nan), (1, 0, 0, 1, nan), (r.n - 1, r.h - 1, r.w - 1, r.c - 1, -nan),
            (0, r.h // 2, r.w // 2, 0, inf), (1, r.h - 1, 0, r.c // 2, -inf))


def make_inputs(r):
    """Seeded numpy inputs of a geometry key: x (NHWC, signed, the specials scattered over it), x_nan (x with nan_sites planted),
    w [C, 1, 3, 3], bias, scale, shift [C].  Every row of the same geometry gets the same arrays."""
    import numpy as np
    rng = np.random.default_rng(9000 + 7 * r.c + 131 * r.n + 17 * r.h + r.w)
    x = (rng.standard_normal((r.n, r.h, r.w, r.c)) * (4.0 * KA)).astype(np.float32)
    vals = np.array(specials(), dtype=np.float32)
    k = min(x.size, 4 * len(vals) + 3)
    pos = rng.permutation(x.size)[:k]
    x.reshape(-1)[pos] = vals[np.arange(k) % len(vals)]
    x_nan = x.copy()
    for img, row, col, ch, v in nan_sites(r):
        x_nan[img, row, col, ch] = v
    w = (rng.standard_normal((r.c, 1, 3, 3)) * (5.0 * KW)).astype(np.float32)
    bias = (rng.standard_normal(r.c) * 0.3).astype(np.float32)
    scale = (rng.random(r.c) + 0.5).astype(np.float32)
    scale[1::2] *= -1.0
    shift = (rng.standard_normal(r.c) * 0.3).astype(np.float32)
    return x, x_nan, w, bias, scale, shift


def make_desc(lib, r, ka=KA, kw_scale=KW):
    import numpy as np
    return lib.ConvDesc(n=r.n, c_in=r.c, h=r.h, w=r.w, c_out=r.c, kh=3, kw=3, stride_h=r.stride, stride_w=r.stride,
                        pad_h=r.pad, pad_w=r.pad, dil_h=1, dil_w=1, groups=r.c, x_layout=lib.LAYOUT_NHWC, y_layout=lib.LAYOUT_NHWC,
                        qbits=r.qbits, ka=float(np.float32(ka)), kw_scale=float(np.float32(kw_scale)), mfma_passes=0, reserved=0)


def make_io(lib, iface, y_qbits, y_ka=0.2345):
    import numpy as np
    if iface in ("f32", "post"):
        return None
    y_codes = iface in ("cout", "lut")
    return lib.ConvIo(x_codes=1, y_codes=int(y_codes), y_ka=float(np.float32(y_ka if y_codes else 1.0)), y_qbits=y_qbits)


def instance(lib, d, iface, bias, post, flags, y_qbits, y_ka=0.2345):
    """slfp_debug_dw3x3_instance for descriptor `d` called through interface `iface`"""
    import ctypes
    io = make_io(lib, iface, y_qbits, y_ka)
    return lib.load().slfp_debug_dw3x3_instance(ctypes.byref(d), ctypes.byref(io) if io is not None else None, int(bias), int(flags),
                                                int(post)).decode()


def set_switches(L, env):
    """Leave exactly `env` (a dict or a tuple of pairs; None: nothing) of the depthwise switches set and have the library re-read them."""
    import os
    for k in SWITCHES:
        os.environ.pop(k, None)
    for k, v in dict(env or ()).items():
        assert k in SWITCHES, k
        os.environ[k] = v
    L.slfp_debug_reload_switches()
