"""Small ragged cases for every instance of the pointwise (1x1) kernels on codes in the float32-equivalent (three-pass) mode
(csrc/conv_pw_codes.hip: k_pwc_stream / k_pwc_tiled with PASSES = 3; slfp_conv2d_fwd_codes_x3), shared by
tests/test_pw_codes_x3_host.py (the table reaches what it claims; the nets' three-pass census is covered by it) and
tests/test_gpu_pw_codes_x3.py (each row bit for bit against the float32-interface three-pass launch, and against the oracle).

A row = the descriptor fields, the output form ("cin": codes in, float32 out; "cout": codes in, codes out), the switches to set and
the string slfp_debug_pwc_x3_variant must then report:

    pwc-stream/ks<N>/<xw|dw>/act8/<f32|yc>/p3[/grid<n>]      k_pwc_stream<kFmtAct8, N, XW, YC, ..., 3>
    pwc-tiled/<wm><wn><mt>/act8/<f32|yc>/p3                  k_pwc_tiled<kFmtAct8, WM, WN, MT, YC, ..., 3>

Shapes, as tests/_pw_variants.py: n = 2, 9 x 11, so M = 198 = 12 units of 16 pixels + 6 rows = three 64-pixel blocks + a 6-row one,
99 pixels per image: units and blocks cross the image boundary.  Stride-2 rows sample the same image (5 x 6 outputs, M = 60).
Stream rows: every k-step count the launcher has (K = 32, 64, 96, 128, 256), C_out = 40 for float32 out (the third channel tile half
empty, the fourth -- the blob's padding -- wholly) and 48 for code out.  Tiled rows: K = 320 (beyond the stream kernel's 256), C_out
just above each tiling's previous width (40 / 72 / 136) with code-out twins at multiples of 16 (48 / 80 / 144); 264 / 272 channels
make a second block of channels on {1,4,4} (three passes have no 512-channel tiling); K = 192 is six k-steps, a count the stream
kernel has no instance for, and K = 256 -> 256 is the layer the single-pass path gives to k_pwc_slice: both planes of its W are
256 KiB, so it runs tiled.  The capped rows run all 13 units on one workgroup's 8 waves: a second, ragged trip."""
from collections import namedtuple

Row = namedtuple("Row", "name c_in c_out stride n h w iface env variant")

ROWS = []
_FORM = {"cin": "f32", "cout": "yc"}


def _add(name, variant, c_in, c_out, iface, env=None, stride=1, n=2, h=9, w=11):
    assert iface in _FORM
    ROWS.append(Row(name, c_in, c_out, stride, n, h, w, iface, tuple(sorted((env or {}).items())), variant))


# ---- k_pwc_stream: every KS instance, both output forms
for _k, _w in ((32, "ks1/dw"), (64, "ks2/xw"), (96, "ks3/dw"), (128, "ks4/xw"), (256, "ks8/xw")):
    _add(f"x3-cs-k{_k}-cin", f"pwc-stream/{_w}/act8/f32/p3", _k, 40, "cin")
    _add(f"x3-cs-k{_k}-cout", f"pwc-stream/{_w}/act8/yc/p3", _k, 48, "cout")
_add("x3-cs-k64-cin-s2", "pwc-stream/ks2/xw/act8/f32/p3", 64, 40, "cin", stride=2)
_add("x3-cs-k96-cout-s2", "pwc-stream/ks3/dw/act8/yc/p3", 96, 48, "cout", stride=2)
# the capacity limit: both planes of 256 -> 128 are 128 KiB of W, 8 channel tiles
_add("x3-cs-k256-n128-cout", "pwc-stream/ks8/xw/act8/yc/p3", 256, 128, "cout")
# the persistent loop's second trip
_add("x3-cs-k64-cin-grid1", "pwc-stream/ks2/xw/act8/f32/p3/grid1", 64, 40, "cin", env={"SLFP_PW_GRID": "1"})
_add("x3-cs-k128-cout-grid1", "pwc-stream/ks4/xw/act8/yc/p3/grid1", 128, 48, "cout", env={"SLFP_PW_GRID": "1"})
# ---- k_pwc_tiled: five 64-deep stages on the three tilings, both output forms
for _t, _n in ((411, 40), (222, 72), (144, 136), (144, 264)):
    _add(f"x3-ct-{_t}-n{_n}-cin", f"pwc-tiled/{_t}/act8/f32/p3", 320, _n, "cin")
for _t, _n in ((411, 48), (222, 80), (144, 144), (144, 272)):
    _add(f"x3-ct-{_t}-n{_n}-cout", f"pwc-tiled/{_t}/act8/yc/p3", 320, _n, "cout")
_add("x3-ct-144-n144-cin-s2", "pwc-tiled/144/act8/f32/p3", 320, 144, "cin", stride=2)
_add("x3-ct-411-k192-cin", "pwc-tiled/411/act8/f32/p3", 192, 40, "cin")            # six k-steps: no stream instance
_add("x3-ct-144-k256-n256-cout", "pwc-tiled/144/act8/yc/p3", 256, 256, "cout")     # single pass: k_pwc_slice

del _k, _w, _t, _n

SWITCHES = ("SLFP_PW_GRID",)   # the one switch the three-pass selection reads


def strip_grid(v):
    return v.rsplit("/grid", 1)[0]


def make_desc(lib, r, ka=0.21, kw_scale=0.027, qbits=8, passes=None):
    import numpy as np
    return lib.ConvDesc(n=r.n, c_in=r.c_in, h=r.h, w=r.w, c_out=r.c_out, kh=1, kw=1, stride_h=r.stride, stride_w=r.stride,
                        pad_h=0, pad_w=0, dil_h=1, dil_w=1, groups=1, x_layout=lib.LAYOUT_NHWC, y_layout=lib.LAYOUT_NHWC,
                        qbits=qbits, ka=float(np.float32(ka)), kw_scale=float(np.float32(kw_scale)),
                        mfma_passes=lib.MFMA_F16X3 if passes is None else passes, reserved=0)


def make_io(lib, iface, y_ka=0.2345, y_qbits=8):
    import numpy as np
    y_codes = iface == "cout"
    return lib.ConvIo(x_codes=1, y_codes=int(y_codes), y_ka=float(np.float32(y_ka if y_codes else 1.0)), y_qbits=y_qbits)


def variant(lib, d, io):
    import ctypes
    return lib.load().slfp_debug_pwc_x3_variant(ctypes.byref(d), ctypes.byref(io)).decode()


def set_switches(L, env):
    """Leave exactly `env` (a dict or a tuple of pairs; None: nothing) of SWITCHES set and have the library re-read them."""
    import os
    for k in SWITCHES:
        os.environ.pop(k, None)
    for k, v in dict(env or ()).items():
        assert k in SWITCHES, k
        os.environ[k] = v
    L.slfp_debug_reload_switches()
