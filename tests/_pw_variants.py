"""Small ragged cases for every pointwise (1x1) kernel instance (csrc/conv_pw.hip, csrc/conv_pw_codes.hip), shared by
tests/test_pw_variants_host.py (the table reaches what it claims; the workloads' census is covered by it) and
tests/test_gpu_pw_variants.py (each row against the oracle, across variants, NaN placement, guard bands, twice).

A row = the descriptor fields, the interface the layer is called through, the switches to set, and the string
slfp_debug_pw_variant must then report.  The grammar (one word per template argument the launcher chooses):

    stream/ks<N>/<kfull|kpart|a8>/<tab|long>/<stg|dir>/p<1|3>/<act8|sfp7>[/res|/yc][/grid<n>]      k_pw_stream
    tiled/<wm><wn><mt>/<kfull|kpart>/<tab|long>/<stg|dir>/p<1|3>/<act8|sfp7>[/res|/yc]             k_pw_tiled (NT = 4)
    pwc-stream/ks<N>/<xw|dw|half>/<act8|sfp7>/<f32|yc|res|res/dual>[/grid<n>]                      k_pwc_stream
    slice/nts<4|8>/<act8|sfp7>/<f32|yc|res|res/dual>[/grid<n>]                                     k_pwc_slice
    pwc-tiled/<wm><wn><mt>/<act8|sfp7>/<f32|yc|res|res/dual>                                       k_pwc_tiled

    ks<N>     the KS instance (stream: 1, 2, 3, 4, 6 for five or six k-steps, 8 for seven or eight)
    kfull     stream: K == 32 * KS (unguarded loads); tiled: K % 64 == 0.  kpart: the guarded K tail.  a8: the 8-byte access form
    tab/long  threshold-table quantizer / long form (SLFP_PW_NOTAB, SLFP_LONG_ENCODE)
    stg/dir   LDS-staged whole-line stores / direct stores (SLFP_PW_NOSTG, SLFP_PW_STG_MAXKS; KS 6 is direct by default)
    p<N>      MFMA passes; act8 / sfp7: the activation format (qbits 8 / 7)
    xw/dw     16-byte code loads + transpose (K % 64 == 0) / dword loads; half: K = 16 or 48, a half-live last k-step
    f32 / yc / res / res/dual     float32 out / code out / residual operand / residual operand and a second, code output
    /grid<n>  SLFP_PW_GRID caps the persistent grid at n workgroups (k_pwc_slice: n rank groups)

Interfaces: "f32" slfp_conv2d_fwd; "entry" slfp_conv2d_fwd_entry (float32 in, codes out); "res" slfp_conv2d_fwd_res on float32;
"cin" / "cout" slfp_conv2d_fwd_codes with codes in and float32 / codes out; "cres" slfp_conv2d_fwd_res on codes; "cdual"
slfp_conv2d_fwd_res_codes; "slice" slfp_conv2d_fwd_codes_slice (pixel stride twice C_out).

Shapes.  Pixels: n = 2, 9 x 11, so M = 198 = 12 units of 16 pixels + 6 rows = three 64-pixel blocks of the tiled kernels + a 6-row
one, 99 pixels per image: units and blocks cross the image boundary.  Stride-2 rows sample the same image (5 x 6 outputs, M = 60;
the strided kernels index pixels through W).  k_pwc_slice with one rank group strides by 64 units: its capped rows use n = 2,
23 x 29 (M = 1334 = 84 units: a second, ragged trip, with the cross-unit prefetch).  Channels: C_out = 40 / 72 / 136 / 264 sit just
above a tile or the previous tiling's width, so channel tiles and whole waves are partly or wholly empty; code rows need
C_out % 16 == 0 (48 / 80 / 144 / 272).  C_in walks every KS instance at both ends of its range and with a K tail."""
from collections import namedtuple

Row = namedtuple("Row", "name c_in c_out stride n h w qbits passes iface env variant")

IFACES = ("f32", "entry", "res", "cin", "cout", "cres", "cdual", "slice")
_FORM = {"cin": "f32", "cout": "yc", "cres": "res", "cdual": "res/dual", "slice": "yc"}

ROWS = []


def _add(name, variant, c_in, c_out, iface="f32", env=None, stride=1, n=2, h=9, w=11, qbits=8, passes=1):
    assert iface in IFACES
    ROWS.append(Row(name, c_in, c_out, stride, n, h, w, qbits, passes, iface, tuple(sorted((env or {}).items())), variant))


def _env(*parts):
    out = {}
    for p in parts:
        out.update(p)
    return out


STREAM = {"SLFP_PW_STREAM_MAX_KB": "128"}   # the float32-interface stream kernel up to its capacity (default: 30 KiB of W)
TILED = {"SLFP_PW_STREAM_MAX_KB": "0"}      # every multiple-of-4 layer on the tiled kernel
NOTAB, NOSTG, LONG = {"SLFP_PW_NOTAB": "1"}, {"SLFP_PW_NOSTG": "1"}, {"SLFP_LONG_ENCODE": "1"}


def _grid(n):
    return {"SLFP_PW_GRID": str(n)}


def _ks(k):
    steps = (k + 31) // 32
    return steps if steps <= 4 else (6 if steps <= 6 else 8)


def _stream(k, kform=None, tab="tab", stg=None, p=1, fmt="act8", tail=""):
    """the string of a k_pw_stream row: K form and store form by the default rule unless given"""
    ks = _ks(k)
    kform = kform or ("kfull" if k == 32 * ks else "kpart")
    stg = stg or ("stg" if (ks <= 4 or ks == 8) and tab == "tab" and kform != "a8" else "dir")
    return f"stream/ks{ks}/{kform}/{tab}/{stg}/p{p}/{fmt}{tail}"


def _tiled(t, k, tab="tab", stg="stg", p=1, fmt="act8", tail=""):
    return f"tiled/{t}/{'kfull' if k % 64 == 0 else 'kpart'}/{tab}/{stg}/p{p}/{fmt}{tail}"


# =============================================================================== k_pw_stream, float32 interface
# ---- every KS instance, KFULL at both ends of the KS = 6 and KS = 8 ranges (160 and 224 fill five of six / seven of eight k-steps:
# the guarded form), and K tails; C_out = 40: the third channel tile is half empty, the fourth (the blob's padding) wholly
for _k in (32, 64, 96, 128, 160, 192, 224, 256, 40, 72, 100, 136, 200, 232):
    _add(f"st-k{_k}", _stream(_k), _k, 40, env=STREAM)
# ---- C_out = 72: five tiles of eight
for _k in (64, 160):
    _add(f"st-k{_k}-n72", _stream(_k), _k, 72, env=STREAM)
# ---- even channel counts that are no multiple of 4 (8-byte accesses): KS 2, 1, 4 and 6 (the instance for five k-steps).  (116 is a
# multiple of 4: ShuffleNetV2's 116 -> 116 layers are 32 KiB of W and run, by the default rule, on the tiled kernel -- the row below.)
for _k, _n in ((58, 58), (24, 58), (114, 58), (138, 58)):
    _add(f"st-a8-{_k}-{_n}", _stream(_k, "a8"), _k, _n)
# ---- the long-form quantizer, direct stores where the rule stages, staged stores where the rule does not
_add("st-k64-notab", _stream(64, tab="long"), 64, 40, env=_env(STREAM, NOTAB))
_add("st-k100-notab", _stream(100, tab="long"), 100, 40, env=_env(STREAM, NOTAB))
_add("st-k160-notab", _stream(160, tab="long"), 160, 40, env=_env(STREAM, NOTAB))
_add("st-a8-58-58-notab", _stream(58, "a8", tab="long"), 58, 58, env=NOTAB)
_add("st-k128-long", _stream(128, tab="long"), 128, 40, env=_env(STREAM, LONG))
_add("st-k256-long", _stream(256, tab="long"), 256, 40, env=_env(STREAM, LONG))
_add("st-k64-nostg", _stream(64, stg="dir"), 64, 40, env=_env(STREAM, NOSTG))
_add("st-k232-nostg", _stream(232, stg="dir"), 232, 40, env=_env(STREAM, NOSTG))
_add("st-k32-maxks0", _stream(32, stg="dir"), 32, 40, env=_env(STREAM, {"SLFP_PW_STG_MAXKS": "0"}))
_add("st-k96-maxks0", _stream(96, stg="dir"), 96, 40, env=_env(STREAM, {"SLFP_PW_STG_MAXKS": "0"}))
_add("st-k192-maxks8", _stream(192, stg="stg"), 192, 40, env=_env(STREAM, {"SLFP_PW_STG_MAXKS": "8"}))
_add("st-k136-maxks8", _stream(136, stg="stg"), 136, 40, env=_env(STREAM, {"SLFP_PW_STG_MAXKS": "8"}))
_add("st-k160-maxks8", _stream(160, stg="stg"), 160, 72, env=_env(STREAM, {"SLFP_PW_STG_MAXKS": "8"}))
# ---- three passes and SFP<3,3>
for _k in (64, 100, 96, 160, 192, 224, 256):
    _add(f"st-k{_k}-f16x3", _stream(_k, p=3), _k, 40, env=STREAM, passes=3)
_add("st-a8-58-58-f16x3", _stream(58, "a8", p=3), 58, 58, passes=3)
_add("st-k64-f16x3-notab", _stream(64, tab="long", p=3), 64, 40, env=_env(STREAM, NOTAB), passes=3)
for _k in (32, 64, 100, 128, 160, 256):
    _add(f"st-k{_k}-sfp7", _stream(_k, fmt="sfp7"), _k, 40, env=STREAM, qbits=7)
_add("st-a8-58-58-sfp7", _stream(58, "a8", fmt="sfp7"), 58, 58, qbits=7)
_add("st-k64-sfp7-notab", _stream(64, tab="long", fmt="sfp7"), 64, 40, env=_env(STREAM, NOTAB), qbits=7)
# ---- what the workloads add to that (the census of tests/test_pw_variants_host.py): SqueezeNet's 16-, 48- and 96-channel and
# ShuffleNetV2's 24-channel inputs in every mode they are run in
_add("st-k24", _stream(24), 24, 40, env=STREAM)
_add("st-k24-sfp7", _stream(24, fmt="sfp7"), 24, 40, env=STREAM, qbits=7)
_add("st-k24-f16x3", _stream(24, p=3), 24, 40, env=STREAM, passes=3)
_add("st-k32-f16x3", _stream(32, p=3), 32, 40, env=STREAM, passes=3)
_add("st-k40-sfp7", _stream(40, fmt="sfp7"), 40, 40, env=STREAM, qbits=7)
_add("st-k40-f16x3", _stream(40, p=3), 40, 40, env=STREAM, passes=3)
_add("st-k96-sfp7", _stream(96, fmt="sfp7"), 96, 40, env=STREAM, qbits=7)
_add("st-k128-f16x3", _stream(128, p=3), 128, 40, env=STREAM, passes=3)
_add("st-a8-24-58-sfp7", _stream(24, "a8", fmt="sfp7"), 24, 58, qbits=7)
_add("st-a8-24-58-f16x3", _stream(24, "a8", p=3), 24, 58, passes=3)
# ---- the capacity limit: 256 -> 256 is 128 KiB of W, 16 channel tiles
_add("st-k256-n256", _stream(256), 256, 256, env=STREAM)
# ---- stride 2
_add("st-k64-s2", _stream(64), 64, 40, env=STREAM, stride=2)
_add("st-k100-s2", _stream(100), 100, 40, env=STREAM, stride=2)
_add("st-k160-s2", _stream(160), 160, 40, env=STREAM, stride=2)
# ---- residual operand: staged and direct as the default rule has it, K tails, the other modes
for _k in (64, 100, 160, 192, 256):
    _add(f"st-k{_k}-res", _stream(_k, tail="/res"), _k, 40, "res", env=STREAM)
_add("st-k64-res-f16x3", _stream(64, p=3, tail="/res"), 64, 40, "res", env=STREAM, passes=3)
_add("st-k160-res-f16x3", _stream(160, p=3, tail="/res"), 160, 40, "res", env=STREAM, passes=3)
_add("st-k64-res-sfp7", _stream(64, fmt="sfp7", tail="/res"), 64, 40, "res", env=STREAM, qbits=7)
# ---- code output (no staging): C_out a multiple of 16
for _k, _n in ((32, 80), (64, 48), (72, 48), (96, 16), (100, 48), (128, 48), (160, 48), (192, 48), (224, 48), (256, 64)):
    _add(f"st-k{_k}-n{_n}-yc", _stream(_k, stg="dir", tail="/yc"), _k, _n, "entry", env=STREAM)
_add("st-k16-n48-yc", _stream(16, stg="dir", tail="/yc"), 16, 48, "entry", env=STREAM)
_add("st-k48-n48-yc", _stream(48, stg="dir", tail="/yc"), 48, 48, "entry", env=STREAM)
for _k, _n in ((32, 80), (16, 48), (48, 48), (96, 16), (128, 48)):
    _add(f"st-k{_k}-n{_n}-yc-sfp7", _stream(_k, stg="dir", fmt="sfp7", tail="/yc"), _k, _n, "entry", env=STREAM, qbits=7)
_add("st-k64-yc-sfp7", _stream(64, stg="dir", fmt="sfp7", tail="/yc"), 64, 48, "entry", env=STREAM, qbits=7)
_add("st-k160-yc-sfp7", _stream(160, stg="dir", fmt="sfp7", tail="/yc"), 160, 48, "entry", env=STREAM, qbits=7)
# ---- the persistent loop's second and third trips: 13 units over 8 waves (one workgroup) and over 24 (three)
for _g in (1, 3):
    _add(f"st-k64-grid{_g}", _stream(64) + f"/grid{_g}", 64, 40, env=_env(STREAM, _grid(_g)))
    _add(f"st-k160-grid{_g}", _stream(160) + f"/grid{_g}", 160, 40, env=_env(STREAM, _grid(_g)))
_add("st-a8-58-58-grid1", _stream(58, "a8") + "/grid1", 58, 58, env=_grid(1))
_add("st-k64-f16x3-grid1", _stream(64, p=3) + "/grid1", 64, 40, env=_env(STREAM, _grid(1)), passes=3)
_add("st-k64-res-grid1", _stream(64, tail="/res") + "/grid1", 64, 40, "res", env=_env(STREAM, _grid(1)))
_add("st-k192-res-grid3", _stream(192, tail="/res") + "/grid3", 192, 40, "res", env=_env(STREAM, _grid(3)))
_add("st-k64-yc-grid1", _stream(64, stg="dir", tail="/yc") + "/grid1", 64, 48, "entry", env=_env(STREAM, _grid(1)))
_add("st-k160-yc-grid3", _stream(160, stg="dir", tail="/yc") + "/grid3", 160, 48, "entry", env=_env(STREAM, _grid(3)))

# =============================================================================== k_pw_tiled, float32 interface
# ---- each tiling just above the previous tiling's width (waves of the block are empty) and at its full width; K = 64, 128, 192:
# one, two and three 64-deep stages (the double buffer wraps); K = 100 and 136: the guarded K tail
for _t, _n, _k in ((411, 40, 64), (411, 64, 128), (411, 40, 100), (222, 72, 128), (222, 128, 192), (222, 72, 136),
                   (144, 136, 192), (144, 256, 64), (144, 136, 100), (184, 264, 64), (184, 512, 128), (184, 264, 136)):
    _add(f"ti-{_t}-k{_k}-n{_n}", _tiled(_t, _k), _k, _n, env=TILED)
_add("ti-222-116-116-default", _tiled(222, 116), 116, 116)
# ---- three passes (the stream kernel keeps every W up to 100 KiB whatever the switch says; no 512-channel tiling: 264 channels
# run on {1,4,4}) and SFP<3,3>
for _t, _n, _k in ((411, 40, 448), (222, 72, 232), (144, 136, 192), (144, 264, 128)):
    _add(f"ti-{_t}-k{_k}-n{_n}-f16x3", _tiled(_t, _k, p=3), _k, _n, env=TILED, passes=3)
for _t, _n, _k in ((411, 40, 100), (222, 72, 64), (144, 136, 192), (184, 264, 128)):
    _add(f"ti-{_t}-k{_k}-n{_n}-sfp7", _tiled(_t, _k, fmt="sfp7"), _k, _n, env=TILED, qbits=7)
# ---- the workloads' remaining combinations of tiling, K form and mode (the census)
_add("ti-144-k136-n136-f16x3", _tiled(144, 136, p=3), 136, 136, env=TILED, passes=3)
_add("ti-222-k256-n72-f16x3", _tiled(222, 256, p=3), 256, 72, env=TILED, passes=3)
_add("ti-144-k100-n136-sfp7", _tiled(144, 100, fmt="sfp7"), 100, 136, env=TILED, qbits=7)
_add("ti-184-k136-n264-sfp7", _tiled(184, 136, fmt="sfp7"), 136, 264, env=TILED, qbits=7)
_add("ti-222-k136-n72-sfp7", _tiled(222, 136, fmt="sfp7"), 136, 72, env=TILED, qbits=7)
_add("ti-411-k64-n40-sfp7", _tiled(411, 64, fmt="sfp7"), 64, 40, env=TILED, qbits=7)
# ---- direct stores, long-form quantizer
_add("ti-411-nostg", _tiled(411, 64, stg="dir"), 64, 40, env=_env(TILED, NOSTG))
_add("ti-184-nostg", _tiled(184, 136, stg="dir"), 136, 264, env=_env(TILED, NOSTG))
_add("ti-144-nostg-f16x3", _tiled(144, 192, stg="dir", p=3), 192, 136, env=_env(TILED, NOSTG), passes=3)
_add("ti-222-notab", _tiled(222, 136, tab="long", stg="dir"), 136, 72, env=_env(TILED, NOTAB))
_add("ti-411-notab-sfp7", _tiled(411, 100, tab="long", stg="dir", fmt="sfp7"), 100, 40, env=_env(TILED, NOTAB), qbits=7)
_add("ti-144-long-f16x3", _tiled(144, 192, tab="long", stg="dir", p=3), 192, 136, env=_env(TILED, LONG), passes=3)
_add("ti-184-long", _tiled(184, 64, tab="long", stg="dir"), 64, 264, env=_env(TILED, LONG))
# ---- stride 2
_add("ti-411-s2", _tiled(411, 100), 100, 40, env=TILED, stride=2)
_add("ti-222-s2", _tiled(222, 128), 128, 72, env=TILED, stride=2)
# ---- residual operand (staged epilogue only)
for _t, _n, _k in ((411, 40, 64), (222, 72, 136), (144, 136, 192), (184, 264, 64)):
    _add(f"ti-{_t}-k{_k}-n{_n}-res", _tiled(_t, _k, tail="/res"), _k, _n, "res", env=TILED)
_add("ti-144-res-f16x3", _tiled(144, 192, p=3, tail="/res"), 192, 136, "res", env=TILED, passes=3)
_add("ti-222-res-sfp7", _tiled(222, 64, fmt="sfp7", tail="/res"), 64, 72, "res", env=TILED, qbits=7)
# ---- code output (no staging area)
for _t, _n, _k in ((411, 48, 64), (222, 80, 100), (144, 144, 128), (184, 272, 64)):
    _add(f"ti-{_t}-k{_k}-n{_n}-yc", _tiled(_t, _k, stg="dir", tail="/yc"), _k, _n, "entry", env=TILED)
_add("ti-222-k128-n80-yc", _tiled(222, 128, stg="dir", tail="/yc"), 128, 80, "entry", env=TILED)
_add("ti-184-k136-n272-yc", _tiled(184, 136, stg="dir", tail="/yc"), 136, 272, "entry", env=TILED)
_add("ti-184-k136-n272-yc-sfp7", _tiled(184, 136, stg="dir", fmt="sfp7", tail="/yc"), 136, 272, "entry", env=TILED, qbits=7)
_add("ti-144-k128-n144-yc-sfp7", _tiled(144, 128, stg="dir", fmt="sfp7", tail="/yc"), 128, 144, "entry", env=TILED, qbits=7)
_add("ti-411-k64-n48-yc-sfp7", _tiled(411, 64, stg="dir", fmt="sfp7", tail="/yc"), 64, 48, "entry", env=TILED, qbits=7)
_add("ti-222-yc-sfp7", _tiled(222, 64, stg="dir", fmt="sfp7", tail="/yc"), 64, 80, "entry", env=TILED, qbits=7)

# =============================================================================== the kernels on codes
_CODE_IFACES = ("cin", "cout", "cres", "cdual")
# ---- k_pwc_stream: K = 16, 48 (HALF), 32, 96 (dword loads), 64, 128, 256 (16-byte loads), each in its four forms; C_out = 48 keeps
# K = 256 off the slice kernel (it wants whole 64-channel slices)
for _k, _w in ((16, "ks1/half"), (48, "ks2/half"), (32, "ks1/dw"), (64, "ks2/xw"), (96, "ks3/dw"), (128, "ks4/xw"), (256, "ks8/xw")):
    for _i in _CODE_IFACES:
        _add(f"cs-k{_k}-{_i}", f"pwc-stream/{_w}/act8/{_FORM[_i]}", _k, 48, _i)
# ---- k_pwc_slice: K = 256 with one slice of four tiles, one and two slices of eight
for _n, _nts in ((64, 4), (128, 8), (256, 8)):
    for _i in _CODE_IFACES:
        _add(f"sl-n{_n}-{_i}", f"slice/nts{_nts}/act8/{_FORM[_i]}", 256, _n, _i)
# ---- k_pwc_tiled: five and eight 64-deep stages on the four tilings, each tiling in its four forms
for _t, _n, _k in ((411, 48, 320), (222, 80, 512), (144, 144, 320), (184, 272, 512)):
    for _i in _CODE_IFACES:
        _add(f"ct-{_t}-k{_k}-{_i}", f"pwc-tiled/{_t}/act8/{_FORM[_i]}", _k, _n, _i)
_add("ct-411-k512-cin", "pwc-tiled/411/act8/f32", 512, 48, "cin")
_add("ct-184-k320-cout", "pwc-tiled/184/act8/yc", 320, 272, "cout")
# SLFP_PWC_NOSLICE: K = 256 on the tiled kernel (320 channels are beyond the stream kernel's capacity) and on the stream kernel
_add("ct-184-k256-noslice-cin", "pwc-tiled/184/act8/f32", 256, 320, "cin", env={"SLFP_PWC_NOSLICE": "1"})
_add("ct-184-k256-noslice-cdual", "pwc-tiled/184/act8/res/dual", 256, 320, "cdual", env={"SLFP_PWC_NOSLICE": "1"})
_add("cs-k256-n256-noslice-cout", "pwc-stream/ks8/xw/act8/yc", 256, 256, "cout", env={"SLFP_PWC_NOSLICE": "1"})
_add("sl-n320-cin", "slice/nts4/act8/f32", 256, 320, "cin")   # ... which the slice kernel takes as five slices of four tiles
# ---- SFP<3,3>
for _k, _w in ((16, "ks1/half"), (48, "ks2/half"), (32, "ks1/dw"), (64, "ks2/xw"), (96, "ks3/dw"), (128, "ks4/xw"), (256, "ks8/xw")):
    for _i in ("cin", "cout"):   # SqueezeNet's Fire modules in SFP<3,3>
        _add(f"cs-k{_k}-{_i}-sfp7", f"pwc-stream/{_w}/sfp7/{_FORM[_i]}", _k, 48, _i, qbits=7)
_add("ct-411-k320-cin-sfp7", "pwc-tiled/411/sfp7/f32", 320, 48, "cin", qbits=7)
_add("ct-411-k320-cout-sfp7", "pwc-tiled/411/sfp7/yc", 320, 48, "cout", qbits=7)
_add("ct-184-k512-cin-sfp7", "pwc-tiled/184/sfp7/f32", 512, 272, "cin", qbits=7)
_add("cs-k96-cres-sfp7", "pwc-stream/ks3/dw/sfp7/res", 96, 48, "cres", qbits=7)
_add("sl-n128-cdual-sfp7", "slice/nts8/sfp7/res/dual", 256, 128, "cdual", qbits=7)
_add("sl-n64-cout-sfp7", "slice/nts4/sfp7/yc", 256, 64, "cout", qbits=7)
_add("ct-222-k512-cout-sfp7", "pwc-tiled/222/sfp7/yc", 512, 80, "cout", qbits=7)
_add("ct-411-k320-cres-sfp7", "pwc-tiled/411/sfp7/res", 320, 48, "cres", qbits=7)
# ---- stride 2 on codes
_add("cs-k64-cin-s2", "pwc-stream/ks2/xw/act8/f32", 64, 48, "cin", stride=2)
_add("cs-k48-cout-s2", "pwc-stream/ks2/half/act8/yc", 48, 48, "cout", stride=2)
_add("ct-144-k320-cin-s2", "pwc-tiled/144/act8/f32", 320, 144, "cin", stride=2)
_add("sl-n64-cin-s2", "slice/nts4/act8/f32", 256, 64, "cin", stride=2)
# ---- code output into a channel slice of a tensor twice as wide: one row per kernel
_add("cs-k64-slice", "pwc-stream/ks2/xw/act8/yc", 64, 48, "slice")
_add("cs-k16-slice", "pwc-stream/ks1/half/act8/yc", 16, 48, "slice")
_add("sl-n128-slice", "slice/nts8/act8/yc", 256, 128, "slice")
_add("ct-411-k320-slice", "pwc-tiled/411/act8/yc", 320, 48, "slice")
# ---- capped grids: one workgroup runs all 13 units (two trips, the second ragged), three share them unevenly
for _i in _CODE_IFACES:
    _add(f"cs-k64-{_i}-grid1", f"pwc-stream/ks2/xw/act8/{_FORM[_i]}/grid1", 64, 48, _i, env=_grid(1))
_add("cs-k48-cin-grid1", "pwc-stream/ks2/half/act8/f32/grid1", 48, 48, "cin", env=_grid(1))
_add("cs-k96-cout-grid3", "pwc-stream/ks3/dw/act8/yc/grid3", 96, 48, "cout", env=_grid(3))
_add("cs-k256-cdual-grid3", "pwc-stream/ks8/xw/act8/res/dual/grid3", 256, 48, "cdual", env=_grid(3))
# k_pwc_slice, one rank group (64 waves per slice): 84 units = a full trip and a ragged one; the first chunk of the next unit's
# codes is carried across (xrn, v[])
for _i in _CODE_IFACES:
    _add(f"sl-n128-{_i}-grid1", f"slice/nts8/act8/{_FORM[_i]}/grid1", 256, 128, _i, env=_grid(1), h=23, w=29)
_add("sl-n64-cout-grid1", "slice/nts4/act8/yc/grid1", 256, 64, "cout", env=_grid(1), h=23, w=29)
_add("sl-n256-cin-grid1", "slice/nts8/act8/f32/grid1", 256, 256, "cin", env=_grid(1), h=23, w=29)

del _k, _n, _t, _i, _w, _g, _nts


def desc_key(r):
    """Rows with the same key describe the same layer: every kernel, form and switch must give it the same bits."""
    return (r.c_in, r.c_out, r.stride, r.n, r.h, r.w, r.qbits, r.passes)


def strip_grid(v):
    return v.rsplit("/grid", 1)[0]


def make_desc(lib, r, ka=0.21, kw_scale=0.027):
    import numpy as np
    return lib.ConvDesc(n=r.n, c_in=r.c_in, h=r.h, w=r.w, c_out=r.c_out, kh=1, kw=1, stride_h=r.stride, stride_w=r.stride,
                        pad_h=0, pad_w=0, dil_h=1, dil_w=1, groups=1, x_layout=lib.LAYOUT_NHWC, y_layout=lib.LAYOUT_NHWC,
                        qbits=r.qbits, ka=float(np.float32(ka)), kw_scale=float(np.float32(kw_scale)),
                        mfma_passes=lib.MFMA_F16X3 if r.passes == 3 else lib.MFMA_F16X1, reserved=0)


def variant(lib, d, iface, qbits, y_ka=0.2345):
    """slfp_debug_pw_variant for descriptor `d` called through interface `iface` (the reader of output codes: y_ka, the layer's qbits)"""
    import ctypes
    import numpy as np
    x_codes = iface in ("cin", "cout", "cres", "cdual", "slice")
    y_codes = iface in ("entry", "cout", "cdual", "slice")
    io = lib.ConvIo(x_codes=int(x_codes), y_codes=int(y_codes), y_ka=float(np.float32(y_ka if y_codes else 1.0)), y_qbits=qbits)
    has_res = iface in ("res", "cres", "cdual")
    y_ld = 2 * d.c_out if iface == "slice" else 0
    return lib.load().slfp_debug_pw_variant(ctypes.byref(d), ctypes.byref(io), int(has_res), int(iface == "cdual"), y_ld).decode()


SWITCHES = ("SLFP_PW_STREAM_MAX_KB", "SLFP_PW_NOTAB", "SLFP_PW_NOSTG", "SLFP_PW_STG_MAXKS", "SLFP_LONG_ENCODE", "SLFP_PWC_NOSLICE", "SLFP_PW_GRID")


def set_switches(L, env):
    """Leave exactly `env` (a dict or a tuple of pairs; None: nothing) of the pointwise switches set and have the library re-read them."""
    import os
    for k in SWITCHES:
        os.environ.pop(k, None)
    for k, v in dict(env or ()).items():
        assert k in SWITCHES, k
        os.environ[k] = v
    L.slfp_debug_reload_switches()
