"""CPU: the argument checks of the five conv2d forward entry points (slfp_conv2d_fwd_post, slfp_conv2d_fwd_codes[_ws],
slfp_conv2d_fwd_codes_slice, slfp_conv2d_fwd_entry, slfp_conv2d_fwd_res), as one table: every single defect and the status it
returns, then pairs of defects that pin which status wins when two things are wrong at once.  No device work is done here:
every pointer is a made-up integer and every row is refused before anything would be dereferenced or launched -- the test
asserts that no row returns SLFP_OK.  A failing call must leave a message that names the function: an slfp_conv2d_* entry point,
or `conv2d:` where the descriptor itself is refused (make_plan speaks for every entry point)."""
import ctypes
import types

import pytest

from cnns_slfp_quantization_amd import _lib

BAD, SHAPE, UNSUP, ALIGN = _lib.ERR_BAD_ARG, _lib.ERR_SHAPE, _lib.ERR_UNSUPPORTED, _lib.ERR_ALIGNMENT
X, W, Y, B, PS, PSH, WS = 1 << 20, 1 << 30, 1 << 32, 1 << 34, 1 << 35, 1 << 36, 1 << 37   # 16-byte aligned, never touched
RELU, LAYEROUT = 1, 2


def _desc(c_in=64, c_out=64, h=28, k=1, pad=0, n=2, qbits=8, groups=1):
    return _lib.ConvDesc(n=n, c_in=c_in, h=h, w=h, c_out=c_out, kh=k, kw=k, stride_h=1, stride_w=1, pad_h=pad, pad_w=pad,
                         dil_h=1, dil_w=1, groups=groups, x_layout=_lib.LAYOUT_NHWC, y_layout=_lib.LAYOUT_NHWC, qbits=qbits,
                         ka=0.25, kw_scale=0.02, mfma_passes=0, reserved=0)


def _dense():
    return _desc(k=3, pad=1)   # the dense k x k family: the one with a workspace on NHWC tensors


NBYTES = 2 * 64 * 28 * 28 * 4   # the float32 output of _desc()


def _args(x_codes, y_codes):
    """A complete, acceptable argument set (1x1, 64 -> 64 channels); each row of the table breaks it in one or two places."""
    return types.SimpleNamespace(d=_desc(), io=_lib.ConvIo(x_codes=x_codes, y_codes=y_codes, y_ka=0.3, y_qbits=8), x=X, w=W, b=B,
                                 ps=None, psh=None, relu=RELU, y=Y, res=Y + 2 * NBYTES, y_ld=128, ws=WS)


def _ref(s):
    return ctypes.byref(s) if s is not None else None


# entry point -> (io of the acceptable call, the call itself)
ENTRY_POINTS = {
    "post": (None, lambda L, a: L.slfp_conv2d_fwd_post(_ref(a.d), a.x, a.w, a.b, a.ps, a.psh, a.relu, a.y, None, a.ws, None)),
    "codes": ((1, 1), lambda L, a: L.slfp_conv2d_fwd_codes(_ref(a.d), _ref(a.io), a.x, a.w, a.b, a.ps, a.psh, a.relu, a.y, None)),
    "codes_ws": ((1, 1), lambda L, a: L.slfp_conv2d_fwd_codes_ws(_ref(a.d), _ref(a.io), a.x, a.w, a.b, a.ps, a.psh, a.relu, a.y,
                                                                  a.ws, None)),
    "slice": ((1, 1), lambda L, a: L.slfp_conv2d_fwd_codes_slice(_ref(a.d), _ref(a.io), a.x, a.w, a.b, a.ps, a.psh, a.relu, a.y,
                                                                  a.y_ld, a.ws, None)),
    "entry": ((0, 1), lambda L, a: L.slfp_conv2d_fwd_entry(_ref(a.d), _ref(a.io), a.x, a.w, a.b, a.ps, a.psh, a.relu, a.y, None)),
    "res": ((0, 0), lambda L, a: L.slfp_conv2d_fwd_res(_ref(a.d), _ref(a.io), a.x, a.w, a.b, a.ps, a.psh, a.relu, a.res, a.y, None,
                                                        None)),
}


def _set(**kw):
    def apply(a):
        for k, v in kw.items():
            setattr(a, k, v() if callable(v) else v)   # a descriptor is made anew for every row
    return apply


def _set_d(**kw):
    def apply(a):
        for k, v in kw.items():
            setattr(a.d, k, v)
    return apply


def _set_io(**kw):
    def apply(a):
        for k, v in kw.items():
            setattr(a.io, k, v)
    return apply


# ---- the defects: name -> what it does to the argument set
D = {
    "null_d": _set(d=None),
    "null_io": _set(io=None),
    "shape": _set_d(n=0),                                   # make_plan: SLFP_ERR_SHAPE
    "null_x": _set(x=None), "null_w": _set(w=None), "null_y": _set(y=None), "null_res": _set(res=None),
    "lone_ps": _set(ps=PS),                                 # post_scale without post_shift
    "lone_psh": _set(psh=PSH),
    "lone_mis_ps": _set(ps=PS + 4),                         # alone AND misaligned: being alone is found first
    "mis_x": _set(x=X + 4), "mis_y": _set(y=Y + 8), "mis_w": _set(w=W + 4), "mis_b": _set(b=B + 8),
    "mis_ps": _set(ps=PS + 4, psh=PSH), "mis_psh": _set(ps=PS, psh=PSH + 8), "mis_res": _set(res=Y + 2 * NBYTES + 4),
    "flag4": _set(relu=RELU | 4),                           # an unknown flag bit
    "layerout": _set(relu=LAYEROUT),                        # SLFP_POST_LAYEROUT without post vectors
    "layerout_post": _set(relu=RELU | LAYEROUT, ps=PS, psh=PSH),
    "x_codes1": _set_io(x_codes=1), "x_codes0": _set_io(x_codes=0), "y_codes0": _set_io(y_codes=0), "y_codes1": _set_io(y_codes=1),
    "y_qbits6": _set_io(y_qbits=6), "y_ka0": _set_io(y_ka=0.0), "y_ka1e31": _set_io(y_ka=1e31),
    "c_out24": _set_d(c_out=24),                            # code output needs C_out % 16 == 0
    "dense": _set(d=_dense),                                # a layer family the entry point does not take
    "depthwise": _set(d=lambda: _desc(k=3, pad=1, groups=64)),
    "no_ws": _set(d=_dense, ws=None),                       # 3x3 dense: a workspace is required
    "mis_ws": _set(d=_dense, ws=WS + 8),
    "y_ld_small": _set(y_ld=48), "y_ld_odd": _set(y_ld=136), "y_ld0": _set(y_ld=0),
    "overlap": _set(res=Y), "overlap_part": _set(res=Y + NBYTES - 16),
}

# ---- single defects: entry point -> [(defect, status, substring the message must keep or None)]
NULLS_IO = [("null_d", BAD, None), ("null_io", BAD, None), ("shape", SHAPE, None), ("null_x", BAD, None), ("null_w", BAD, None),
            ("null_y", BAD, None)]
CODES_ROWS = NULLS_IO + [
    ("lone_ps", BAD, "post_scale"), ("lone_psh", BAD, "post_scale"), ("lone_mis_ps", BAD, "post_scale"),
    ("mis_x", ALIGN, None), ("mis_y", ALIGN, None), ("mis_w", ALIGN, None), ("mis_b", ALIGN, None), ("mis_ps", ALIGN, None),
    ("mis_psh", ALIGN, None),
    ("flag4", UNSUP, "code-path"), ("layerout", UNSUP, "code-path"), ("layerout_post", UNSUP, "code-path"),
    ("y_qbits6", UNSUP, "code-path"), ("y_ka0", UNSUP, "code-path"), ("y_ka1e31", UNSUP, "code-path"),
    ("x_codes0", UNSUP, "code-path"),                       # pointwise, float32 in -> codes out: slfp_conv2d_fwd_entry's ground
    ("c_out24", UNSUP, "code-path"),
]
SINGLE = {
    "post": [("null_d", BAD, None), ("shape", SHAPE, None), ("null_x", BAD, None), ("null_w", BAD, None), ("null_y", BAD, None),
             ("lone_ps", BAD, "post_scale"), ("lone_psh", BAD, "post_scale"), ("lone_mis_ps", BAD, "post_scale"),
             ("mis_ps", ALIGN, None), ("mis_psh", ALIGN, None), ("flag4", BAD, None), ("layerout", BAD, None),
             ("mis_x", ALIGN, None), ("mis_y", ALIGN, None), ("mis_w", ALIGN, None), ("mis_b", ALIGN, None),
             ("no_ws", BAD, "workspace"), ("mis_ws", BAD, "workspace")],
    "codes": CODES_ROWS + [("dense", BAD, "workspace")],    # slfp_conv2d_fwd_codes hands no workspace on
    "codes_ws": CODES_ROWS + [("no_ws", BAD, "workspace"), ("mis_ws", BAD, "workspace")],
    "slice": NULLS_IO + [
        ("y_codes0", BAD, None), ("mis_y", ALIGN, None),
        ("y_ld_small", BAD, "y_ld"), ("y_ld_odd", BAD, "y_ld"), ("y_ld0", BAD, "y_ld"),
        ("flag4", UNSUP, "slfp_conv2d_codes_slice_supported"), ("layerout", UNSUP, "slfp_conv2d_codes_slice_supported"),
        ("layerout_post", UNSUP, "slfp_conv2d_codes_slice_supported"),
        ("y_qbits6", UNSUP, "slfp_conv2d_codes_slice_supported"), ("y_ka0", UNSUP, "slfp_conv2d_codes_slice_supported"),
        ("y_ka1e31", UNSUP, "slfp_conv2d_codes_slice_supported"), ("x_codes0", UNSUP, "slfp_conv2d_codes_slice_supported"),
        ("depthwise", UNSUP, "slfp_conv2d_codes_slice_supported"),   # runs on codes, but has no channel-slice store
        ("lone_ps", BAD, "post_scale"), ("lone_psh", BAD, "post_scale"), ("lone_mis_ps", BAD, "post_scale"),
        ("mis_x", ALIGN, None), ("mis_w", ALIGN, None), ("mis_b", ALIGN, None), ("mis_ps", ALIGN, None), ("mis_psh", ALIGN, None),
        ("no_ws", BAD, "workspace"), ("mis_ws", BAD, "workspace")],
    "entry": NULLS_IO + [
        ("lone_ps", BAD, "post_scale"), ("lone_psh", BAD, "post_scale"), ("lone_mis_ps", BAD, "post_scale"),
        ("mis_x", ALIGN, None), ("mis_y", ALIGN, None), ("mis_w", ALIGN, None), ("mis_b", ALIGN, None), ("mis_ps", ALIGN, None),
        ("mis_psh", ALIGN, None),
        ("x_codes1", BAD, "slfp_conv2d_entry_supported"), ("y_codes0", BAD, "slfp_conv2d_entry_supported"),
        ("y_qbits6", BAD, "slfp_conv2d_entry_supported"), ("y_ka0", BAD, "slfp_conv2d_entry_supported"),
        ("y_ka1e31", BAD, "slfp_conv2d_entry_supported"),
        ("flag4", UNSUP, "slfp_conv2d_entry_supported"), ("layerout", UNSUP, "slfp_conv2d_entry_supported"),
        ("layerout_post", UNSUP, "slfp_conv2d_entry_supported"), ("c_out24", UNSUP, "slfp_conv2d_entry_supported"),
        ("dense", UNSUP, "slfp_conv2d_entry_supported")],
    "res": NULLS_IO + [
        ("null_res", BAD, None), ("lone_ps", BAD, "post_scale"), ("lone_psh", BAD, "post_scale"), ("lone_mis_ps", BAD, "post_scale"),
        ("mis_x", ALIGN, None), ("mis_y", ALIGN, None), ("mis_w", ALIGN, None), ("mis_b", ALIGN, None), ("mis_ps", ALIGN, None),
        ("mis_psh", ALIGN, None), ("mis_res", ALIGN, None),
        ("overlap", BAD, "overlap"), ("overlap_part", BAD, "overlap"),
        ("flag4", UNSUP, "slfp_conv2d_res_supported"), ("layerout", UNSUP, "slfp_conv2d_res_supported"),
        ("layerout_post", UNSUP, "slfp_conv2d_res_supported"), ("y_codes1", UNSUP, "slfp_conv2d_res_supported"),
        ("dense", UNSUP, "slfp_conv2d_res_supported")],
}

# ---- pairs: for every two neighbours in the entry point's order of checks, both defects at once: the earlier check's status wins.
# One representative defect per check, chosen so that the two of a pair touch different arguments.
ORDER = {
    "post": [("shape", SHAPE), ("null_x", BAD), ("lone_ps", BAD), ("mis_ps", ALIGN), ("flag4", BAD), ("mis_x", ALIGN), ("no_ws", BAD)],
    "codes_ws": [("null_io", BAD), ("shape", SHAPE), ("null_x", BAD), ("lone_ps", BAD), ("mis_x", ALIGN), ("flag4", UNSUP),
                 ("no_ws", BAD)],
    "slice": [("null_io", BAD), ("shape", SHAPE), ("null_x", BAD), ("y_codes0", BAD), ("mis_y", ALIGN), ("y_ld_odd", BAD),
              ("flag4", UNSUP), ("lone_ps", BAD), ("mis_x", ALIGN), ("no_ws", BAD)],
    "entry": [("null_io", BAD), ("shape", SHAPE), ("null_x", BAD), ("lone_ps", BAD), ("mis_x", ALIGN), ("x_codes1", BAD),
              ("y_qbits6", BAD), ("y_ka0", BAD), ("flag4", UNSUP)],
    "res": [("null_io", BAD), ("shape", SHAPE), ("null_x", BAD), ("lone_ps", BAD), ("mis_x", ALIGN), ("overlap_part", BAD),
            ("flag4", UNSUP)],
}
ORDER["codes"] = ORDER["codes_ws"][:-1] + [("dense", BAD)]
SAME_ARGUMENT = {("post", "lone_ps", "mis_ps")}   # a pair that cannot be given at once: the row `lone_mis_ps` stands for it
# neighbours whose representative above shares an argument with the next one, and further pairs worth pinning
EXTRA_PAIRS = {
    "post": [("lone_ps", "flag4", BAD), ("mis_psh", "layerout", ALIGN), ("layerout", "mis_x", BAD), ("mis_b", "no_ws", ALIGN)],
    "codes": [("mis_b", "y_qbits6", ALIGN), ("y_ka0", "dense", UNSUP)],
    "codes_ws": [("mis_b", "y_qbits6", ALIGN), ("y_ka0", "no_ws", UNSUP), ("layerout", "no_ws", UNSUP)],
    "slice": [("y_ld_small", "y_qbits6", BAD), ("mis_y", "x_codes0", ALIGN), ("y_qbits6", "mis_w", UNSUP), ("x_codes0", "lone_psh", UNSUP),
              ("mis_b", "no_ws", ALIGN), ("y_codes0", "y_ld0", BAD)],
    "entry": [("mis_y", "y_codes0", ALIGN), ("y_codes0", "c_out24", BAD), ("y_ka1e31", "dense", BAD), ("y_qbits6", "layerout", BAD)],
    "res": [("mis_y", "overlap", ALIGN), ("overlap", "y_codes1", BAD), ("overlap", "dense", BAD), ("null_res", "lone_ps", BAD)],
}


def _rows():
    rows = []
    for ep, table in SINGLE.items():
        for name, status, text in table:
            rows.append((ep, (name,), status, text))
    for ep, order in ORDER.items():
        for (a, sa), (b, _) in zip(order, order[1:]):
            if (ep, a, b) in SAME_ARGUMENT:
                continue
            rows.append((ep, (a, b), sa, None))
        for a, b, status in EXTRA_PAIRS[ep]:
            rows.append((ep, (a, b), status, None))
    return rows


ROWS = _rows()


def test_the_acceptable_call_is_one_the_library_has_a_kernel_for():
    """What every row starts from is supported, so each row's status is the defect's own: the queries say yes to the plain
    argument set, and the 3x3 layer of the workspace rows is a code-path layer that needs one."""
    L = _lib.load()
    d, dn = _desc(), _dense()
    io = {k: _lib.ConvIo(x_codes=v[0][0], y_codes=v[0][1], y_ka=0.3, y_qbits=8) for k, v in ENTRY_POINTS.items() if v[0]}
    assert L.slfp_conv2d_codes_supported(_ref(d), _ref(io["codes"]), 1, RELU) == 1
    assert L.slfp_conv2d_codes_slice_supported(_ref(d), _ref(io["slice"]), 1, RELU, 128) == 1
    assert L.slfp_conv2d_entry_supported(_ref(d), _ref(io["entry"]), 1, RELU) == 1
    assert L.slfp_conv2d_res_supported(_ref(d), _ref(io["res"]), 1, RELU) == 1
    assert L.slfp_conv2d_workspace_bytes(_ref(d)) == 0 and L.slfp_conv2d_workspace_bytes(_ref(dn)) > 0
    assert L.slfp_conv2d_codes_supported(_ref(dn), _ref(io["codes"]), 1, RELU) == 1
    assert L.slfp_conv2d_codes_slice_supported(_ref(dn), _ref(io["slice"]), 1, RELU, 128) == 1
    assert L.slfp_conv2d_kernel_name(_ref(dn)).decode().startswith("dense_mfma")
    for ep in ENTRY_POINTS:   # every entry point has its table, its order of checks and its pairs
        assert ep in SINGLE and len(ORDER[ep]) >= 6 and EXTRA_PAIRS[ep]


@pytest.mark.parametrize("ep,defects,status,text", ROWS, ids=[f"{r[0]}-{'+'.join(r[1])}" for r in ROWS])
def test_defect_returns_its_status(ep, defects, status, text):
    L = _lib.load()
    io, call = ENTRY_POINTS[ep]
    a = _args(*(io or (0, 0)))
    for name in defects:
        D[name](a)
    rc = call(L, a)
    msg = _lib.last_error()
    assert rc != _lib.OK, "a row of this table must never reach a launch"
    assert rc == status, (rc, msg)
    assert msg, "a failing call records why"
    assert "slfp_conv2d_" in msg or msg.startswith("conv2d:"), msg
    if text is not None:
        assert text in msg, msg
