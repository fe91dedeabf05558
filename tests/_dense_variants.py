"""Small ragged cases for every dense k x k kernel variant (csrc/conv_dense.hip), shared by tests/test_dense_variants_host.py
(the table reaches what it claims; the workloads' census is covered by it) and tests/test_gpu_dense_variants.py (each row
against the oracle, across tilings, on codes, twice).

A row = the descriptor fields, the SLFP_DENSE_* switches to set, and the string slfp_debug_dense_variant must then report:
    <wm><wn><mt>/<k3x3|gen>/nwb<2|3>/ns<3|6|9>/p<1|2>      the per-tile kernels k_dense3x3 / k_dense_mfma
    res/mt<1|2>/ns<3|6>[/encx]                             the weights-resident persistent k_dense3x3_res
SLFP_DENSE_CFG forces a tiling only where it fits (otherwise the cost model decides), hence the expected string on every row.

Shapes: n = 2 (tile indices cross an image); 19 x 21 outputs with padding 1, 17 x 19 without: two tiles or more each way with a
ragged last row tile for TH = 4, 8 and 16 and a ragged last 16-column tile; C_in = 96 = one and a half 64-channel chunks;
C_out = 80 (code rows: a multiple of 16) or 72 (float32 rows): part of one 64-channel wave slice, whole waves of the 128- and
256-channel blocks empty."""
from collections import namedtuple

Row = namedtuple("Row", "name c_in c_out kh kw stride pad_h pad_w n h w qbits passes env variant")

TILINGS = (244, 424, 422, 421, 812, 811)


def _row(name, variant, env=None, c_in=96, c_out=80, k=(3, 3), stride=1, pad=(1, 1), n=2, h=19, w=21, qbits=8, passes=1):
    return Row(name, c_in, c_out, k[0], k[1], stride, pad[0], pad[1], n, h, w, qbits, passes, tuple(sorted((env or {}).items())), variant)


def _cfg(t, **kw):
    env = {"SLFP_DENSE_CFG": str(t)}
    env.update(kw)
    return env


# what each tiling runs for a 3x3 stride-1 single-plane layer (body, weight buffers, halo slots follow from the tiling alone)
_K3 = {244: "244/k3x3/nwb3/ns3/p1", 424: "424/k3x3/nwb3/ns6/p1", 422: "422/gen/nwb2/ns3/p1",
       421: "421/k3x3/nwb2/ns3/p1", 812: "812/gen/nwb3/ns6/p1", 811: "811/k3x3/nwb2/ns3/p1"}

ROWS = []
# ---- the basic 3x3 stride-1 case on all six tilings: code rows (C_out 80, padding 1), float32 rows (C_out 72, no padding)
for _t in TILINGS:
    ROWS.append(_row(f"k3-pad1-{_t}", _K3[_t], _cfg(_t)))
    ROWS.append(_row(f"k3-pad0-{_t}", _K3[_t], _cfg(_t), c_out=72, pad=(0, 0)))
    # SFP<3,3> (exact): the same kernels behind another pre-pass table and epilogue format
    ROWS.append(_row(f"k3-sfp7-{_t}", _K3[_t], _cfg(_t), qbits=7))
# ---- float32-equivalent mode (two operand planes) on every tiling whose two-plane geometry fits 160 KiB of LDS
for _t in (422, 421, 811):
    ROWS.append(_row(f"k3-f16x3-{_t}", f"{_t}/gen/nwb2/ns3/p2", _cfg(_t), c_out=72, passes=3))
# ---- forced switches: the general body where the unrolled one would run; two weight buffers where three would be taken
ROWS.append(_row("k3-generic-424", "424/gen/nwb3/ns6/p1", _cfg(424, SLFP_DENSE_GENERIC="1")))
ROWS.append(_row("k3-generic-244", "244/gen/nwb3/ns3/p1", _cfg(244, SLFP_DENSE_GENERIC="1")))
ROWS.append(_row("k3-generic-811", "811/gen/nwb2/ns3/p1", _cfg(811, SLFP_DENSE_GENERIC="1")))
ROWS.append(_row("k3-nwb2-424", "424/k3x3/nwb2/ns6/p1", _cfg(424, SLFP_DENSE_NWB="2")))
# ---- a grid of more than 8 workgroups whose count is no multiple of 8 (xcd_remap's tail): 3 images x 3 x 2 tiles x 2 slices = 36
ROWS.append(_row("k3-xcd-811", _K3[811], _cfg(811), c_out=72, n=3))
# ---- C_in = 64: exactly one chunk; a forced tiling switches the resident form off, so the per-tile kernels run a one-chunk K loop
ROWS.append(_row("k3-cin64-424", _K3[424], _cfg(424), c_in=64))
ROWS.append(_row("k3-cin64-811", _K3[811], _cfg(811), c_in=64))
ROWS.append(_row("k3-cin64-812", _K3[812], _cfg(812), c_in=64))
# ... and what that layer runs unforced: the resident kernel, 8-row tiles (19 rows pad to 32 with 16-row tiles) and, at 30 rows,
# 16-row tiles; float32 input of one channel slice is encoded on load
ROWS.append(_row("res-mt1", "res/mt1/ns3", None, c_in=64))
ROWS.append(_row("res-mt1-encx", "res/mt1/ns3/encx", None, c_in=64, c_out=48))
ROWS.append(_row("res-mt2", "res/mt2/ns6", None, c_in=64, h=30))
ROWS.append(_row("res-mt2-encx", "res/mt2/ns6/encx", None, c_in=64, c_out=64, h=30))
# ---- C_in = 256: four chunks (the halo double buffer goes round twice)
ROWS.append(_row("k3-cin256-424", _K3[424], _cfg(424), c_in=256))
ROWS.append(_row("k3-cin256-244", _K3[244], _cfg(244), c_in=256))
ROWS.append(_row("k3-cin256-422", _K3[422], _cfg(422), c_in=256))
# ---- other kernel sizes: the general body
ROWS.append(_row("k1x3-424", "424/gen/nwb3/ns9/p1", _cfg(424), k=(1, 3), pad=(0, 1)))        # 3 taps: the fewest that take three weight buffers
ROWS.append(_row("k2x2-244", "244/gen/nwb3/ns3/p1", _cfg(244), k=(2, 2), pad=(0, 0)))        # 4 taps
ROWS.append(_row("k2x2-811", "811/gen/nwb2/ns3/p1", _cfg(811), k=(2, 2), pad=(0, 0), c_out=72))
ROWS.append(_row("k5x5-244", "244/gen/nwb3/ns9/p1", _cfg(244), k=(5, 5), pad=(2, 2)))
ROWS.append(_row("k5x5-421", "421/gen/nwb2/ns3/p1", _cfg(421), k=(5, 5), pad=(2, 2), c_out=72))
ROWS.append(_row("k5x5-f16x3-811", "811/gen/nwb2/ns9/p2", _cfg(811), k=(5, 5), pad=(2, 2), c_out=72, passes=3))
# ---- stride 2 at 23 x 19 (12 x 10 outputs): the halo of a 16-column tile is 33 wide, so only the 4- and 8-row tilings with a narrow
# channel block fit; {8,1,1} takes all nine halo slots a wave can stage and has no room for a third weight buffer
ROWS.append(_row("k3s2-421", "421/gen/nwb3/ns9/p1", _cfg(421), stride=2, h=23, w=19))
ROWS.append(_row("k3s2-811", "811/gen/nwb2/ns9/p1", _cfg(811), stride=2, h=23, w=19, c_out=72))

del _t


def desc_key(r):
    """Rows with the same key describe the same layer: every tiling and body must give it the same bits."""
    return r[1:13]


def make_desc(lib, r, ka=0.21, kw_scale=0.027):
    import numpy as np
    return lib.ConvDesc(n=r.n, c_in=r.c_in, h=r.h, w=r.w, c_out=r.c_out, kh=r.kh, kw=r.kw, stride_h=r.stride, stride_w=r.stride,
                        pad_h=r.pad_h, pad_w=r.pad_w, dil_h=1, dil_w=1, groups=1, x_layout=lib.LAYOUT_NHWC, y_layout=lib.LAYOUT_NHWC,
                        qbits=r.qbits, ka=float(np.float32(ka)), kw_scale=float(np.float32(kw_scale)),
                        mfma_passes=lib.MFMA_F16X3 if r.passes == 3 else lib.MFMA_F16X1, reserved=0)


SWITCHES = ("SLFP_DENSE_CFG", "SLFP_DENSE_GENERIC", "SLFP_DENSE_NWB", "SLFP_DENSE_NORES", "SLFP_DENSE_NOENCX")


def set_switches(L, env):
    """Leave exactly `env` (a dict or a tuple of pairs; None: nothing) of the dense switches set and have the library re-read them."""
    import os
    for k in SWITCHES:
        os.environ.pop(k, None)
    for k, v in dict(env or ()).items():
        assert k in SWITCHES, k
        os.environ[k] = v
    L.slfp_debug_reload_switches()
