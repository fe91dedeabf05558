"""Cases of the byte-input image stems (slfp_conv2d_fwd_u8), shared by tests/test_image_u8_host.py (the query
accepts every row and slfp_debug_stem_u8_instance reports the tabled string) and tests/test_gpu_image_u8.py (each row against the
float32 entry point of the same interface on the expanded tensor, byte for byte).

A row is a tests/_stem_variants.Row: geometry, interface ("f32" / "post": float32 out; "cout": codes out), bias / post vectors /
flags, the switches to set, and in `variant` the string slfp_debug_stem_u8_instance must report:

    stem/fixed/tab/u8/<f32|yc|yc-signed>              k_stem_fixed<Act8, 3, 3, 3, 2, 32, TAB, 16, YC, false, U8>
    small/nt<1..4>/<act8|sfp7>/u8/<f32|yc|yc-signed>  k_stem_small<FMT, NT, false, U8>
    rows/nt<4|6>/<act8|sfp7>/u8/<f32|yc|yc-signed>    k_stem_rows<FMT, NT, YC, U8>
    im2row/nt<4|6>/<act8|sfp7>/u8/<f32|yc|yc-signed>  k_stem_im2row<FMT, U8> + k_stem_mfma<NT, 8, YC>

The shapes are the smallest at which each fill can still go wrong; n >= 2 throughout, so tiles cross image boundaries and, where
H * W * C is odd, images 1.. start at odd addresses (on top of the batch itself starting at an odd address in the GPU test).

fixed/tab (16 x 16 output tiles, 3x3 s2 3 -> 32):
    33 x 36 pad 1, n 3     k_stem_mx's geometry on the float32 interface: the byte entry must report stem/fixed/tab/u8
    35 x 36 pad 0          no padding: every tap inside the image
    33 x 35 pad 1, n 3     W * 3 = 105, 3 465 bytes per image: odd
    7 x 8 pad 1            an image smaller than a tile
    each as plain (raw accumulator), f32 (bias + affine + ReLU), the layer-output quantizer, yc (ReLU folded) and yc-signed;
    one row at qbits 7 and one whose reader takes SFP<3,3> codes (y_qbits 7)
small (8 x 32 tiles): 3 -> 64 3x3 s1 at 9 x 35 pad 1, n 3 (f32, yc, yc-signed; both formats); 3 -> 24 s2 at 17 x 67 pad 1;
    1 -> 64 5x5 s2 at 17 x 67 pad 2; 4 -> 4 (2 x 4) s2 at 17 x 67 pad (0, 1)
rows (8 x 32 tiles): 7x7 s2 3 -> 64 at 20 x 70 pad 3; 3 -> 96 at 21 x 69 pad 0 (4 347 bytes per image: odd; nt6); 5x5 s1 4 -> 64 at
    10 x 35 pad 2; yc and yc-signed on the first two
im2row: 11x11 s4 3 -> 64 at 35 x 51 pad 2 (5 355 bytes: odd; the rows form overflows LDS); 7x7 s1 3 -> 64 at 10 x 35 pad 3 (odd
    stride * c_in); the SLFP_STEM_IM2ROW twin of the first rows case; one yc"""
from _stem_variants import IM2ROW, LAYEROUT, RELU, Row, _pair

ROWS = []


def _add(name, variant, c_in, c_out, k, h, w, pad=0, stride=1, n=2, iface="f32", bias=False, post=False, flags=0, env=None, qbits=8,
         y_qbits=None):
    assert iface in ("f32", "post", "cout") and (iface != "f32" or (not post and not flags))
    ROWS.append(Row(name, c_in, c_out, _pair(k), _pair(stride), _pair(pad), (1, 1), 1, n, h, w, qbits, iface, bool(bias), bool(post), flags,
                    0, tuple(sorted((env or {}).items())), y_qbits or qbits, variant))


# output form -> (interface, bias, post vectors, flags)
FORMS = {"plain": ("f32", False, False, 0), "f32": ("post", True, True, RELU), "lo": ("post", False, True, LAYEROUT),
         "yc": ("cout", False, True, RELU), "yc-signed": ("cout", True, True, 0)}
_OUT = {"plain": "f32", "f32": "f32", "lo": "f32", "yc": "yc", "yc-signed": "yc-signed"}


def _forms(tag, head, forms, *geom, **kw):
    for f in forms:
        i, b, p, fl = FORMS[f]
        _add(f"{tag}-{f}", f"{head}/u8/{_OUT[f]}", *geom, iface=i, bias=b, post=p, flags=fl, **kw)


# ---- k_stem_fixed<TAB> (3x3 s2 3 -> 32)
for _t, _h, _w, _p, _n in (("33x36p1", 33, 36, 1, 3), ("35x36p0", 35, 36, 0, 2), ("33x35p1", 33, 35, 1, 3), ("7x8p1", 7, 8, 1, 2)):
    _forms(f"fixed-{_t}", "stem/fixed/tab", ("plain", "f32", "lo", "yc", "yc-signed"), 3, 32, 3, _h, _w, _p, 2, n=_n)
_add("fixed-33x35p1-sfp7", "stem/fixed/tab/u8/f32", 3, 32, 3, 33, 35, 1, 2, n=3, qbits=7, iface="post", bias=True, post=True, flags=RELU)
_add("fixed-35x36p0-yc-to-sfp7", "stem/fixed/tab/u8/yc", 3, 32, 3, 35, 36, 0, 2, iface="cout", post=True, flags=RELU, y_qbits=7)

# ---- k_stem_small
for _q, _f in ((8, "act8"), (7, "sfp7")):
    _forms(f"small-3x3s1-o64-{_f}", f"small/nt4/{_f}", ("f32", "yc", "yc-signed"), 3, 64, 3, 9, 35, 1, 1, n=3, qbits=_q)
_forms("small-3x3s2-o24", "small/nt2/act8", ("plain", "f32"), 3, 24, 3, 17, 67, 1, 2)
_forms("small-5x5s2c1-o64", "small/nt4/act8", ("f32", "yc"), 1, 64, 5, 17, 67, 2, 2)
_forms("small-2x4s2c4-o4", "small/nt1/act8", ("plain",), 4, 4, (2, 4), 17, 67, (0, 1), 2, n=3)

# ---- k_stem_rows
_forms("rows-7x7s2-o64", "rows/nt4/act8", ("f32", "yc", "yc-signed"), 3, 64, 7, 20, 70, 3, 2)
_forms("rows-7x7s2-o96", "rows/nt6/act8", ("plain", "yc", "yc-signed"), 3, 96, 7, 21, 69, 0, 2)
_forms("rows-5x5s1c4-o64", "rows/nt4/act8", ("f32",), 4, 64, 5, 10, 35, 2, 1)
_forms("rows-7x7s2-o64-sfp7", "rows/nt4/sfp7", ("f32",), 3, 64, 7, 20, 70, 3, 2, qbits=7)

# ---- k_stem_im2row + k_stem_mfma
_forms("im2row-11x11s4-o64", "im2row/nt4/act8", ("f32", "yc"), 3, 64, 11, 35, 51, 2, 4)
_forms("im2row-7x7s1-o64", "im2row/nt4/act8", ("plain",), 3, 64, 7, 10, 35, 3, 1)
_forms("im2row-7x7s2-o64-twin", "im2row/nt4/act8", ("f32",), 3, 64, 7, 20, 70, 3, 2, env=IM2ROW)

del _t, _h, _w, _p, _n, _q, _f

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CIFAR_MEAN, CIFAR_STD = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)
KA_NORM = 0.1   # pass (a): P / Ka passes the 15.5 clamp on both sides (P spans about -2.1 .. 2.6)

# pass (b): where the NaN and the infinities go in the synthetic table, as (channel, byte); channels taken modulo C_in.  Small byte
# values, so that the 7 x 8 image (a prefix of the byte ramp per channel) holds them too
NAN_ENTRIES = ((0, 3, float("nan")), (1, 11, float("inf")), (2, 7, float("-inf")))


def io_of(lib, r, y_ka):
    """the io struct of row `r` (None: float32 out)"""
    import numpy as np
    if r.iface != "cout":
        return None
    return lib.ConvIo(x_codes=0, y_codes=1, y_ka=float(np.float32(y_ka)), y_qbits=r.y_qbits)


def u8_instance(lib, d, r, y_ka):
    import ctypes
    io = io_of(lib, r, y_ka)
    return lib.load().slfp_debug_stem_u8_instance(ctypes.byref(d), ctypes.byref(io) if io is not None else None, int(r.bias), int(r.flags),
                                                  int(r.post)).decode()


def u8_supported(lib, d, r, y_ka):
    import ctypes
    io = io_of(lib, r, y_ka)
    return lib.load().slfp_conv2d_u8_supported(ctypes.byref(d), ctypes.byref(io) if io is not None else None, int(r.bias), int(r.flags))


def pixels(r):
    """Seeded uint8 NHWC batch of row `r`: 0 and 255 alternating along every image's border, corners included -- a padded tap read as
    table[c][0] instead of the operand +0 shows there -- and, per channel, the values 0..255 dealt in a random order over the batch's
    interior pixels, so that every value occurs in every channel where the batch has the pixels for it (every row but the 7 x 8 one
    has 512 interior pixels or more: each value at least twice).  Three interior pixels of the first image then take the bytes of
    NAN_ENTRIES."""
    import numpy as np
    rng = np.random.default_rng(9100 + 7 * r.c_in + 131 * r.n + 17 * r.h + r.w)
    alt = ((np.add.outer(np.arange(r.h), np.arange(r.w)) % 2) * 255).astype(np.uint8)
    x = np.repeat(np.repeat(alt[None, :, :, None], r.n, axis=0), r.c_in, axis=3)
    n_in = r.n * (r.h - 2) * (r.w - 2)
    for c in range(r.c_in):
        x[:, 1:-1, 1:-1, c] = (rng.permutation(n_in) % 256).astype(np.uint8).reshape(r.n, r.h - 2, r.w - 2)
    x[:, 0, 0, :] = 0
    x[:, -1, -1, :] = 255
    for i, (c, v, _) in enumerate(NAN_ENTRIES):   # interior pixels of the first image that draw pass (b)'s NaN and infinities
        x[0, r.h // 2, r.w // 2 - i, c % r.c_in] = v
    return x


def norm_table(c_in):
    """pass (a): pixel_table of the ImageNet constants, repeated or cut to c_in channels"""
    from cnns_slfp_quantization_amd import image_u8
    idx = [c % 3 for c in range(c_in)]
    return image_u8.pixel_table([IMAGENET_MEAN[i] for i in idx], [IMAGENET_STD[i] for i in idx]).numpy()


def synth_table(r, ka):
    """pass (b): seeded values of both signs at the quantizer's scale, the specials of tests/_stem_variants.py written over seeded
    entries, then NaN / +inf / -inf at NAN_ENTRIES"""
    import numpy as np
    from _stem_variants import specials
    rng = np.random.default_rng(9200 + r.c_in)
    t = (rng.standard_normal((r.c_in, 256)) * (4.0 * ka)).astype(np.float32)
    vals = np.array(specials(ka), dtype=np.float32)
    pos = rng.permutation(t.size)[:4 * len(vals)]
    pos = pos[~np.isin(pos, [(c % r.c_in) * 256 + v for c, v, _ in NAN_ENTRIES])]
    t.reshape(-1)[pos] = vals[np.arange(len(pos)) % len(vals)]
    for c, v, s in NAN_ENTRIES:
        t[c % r.c_in, v] = s
    return t


def expand_np(x, table):
    """x32[n, h, w, c] = table[c][x[n, h, w, c]] on the host"""
    import numpy as np
    return table[np.arange(x.shape[-1]), x.astype(np.int64)]
