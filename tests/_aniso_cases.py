"""Non-square convolution geometries shared by tests/test_aniso_host.py (where they dispatch) and tests/test_gpu_aniso.py
(what the kernels compute on them).  On a square input `row * W + col` and `row * H + col` are the same number, so a swapped
extent, padding, stride or kernel side in an index expression is invisible to every square test; each row here has H != W
and, where its family permits, kh != kw / pad_h != pad_w / stride_h != stride_w / dil_h != dil_w.

A row names the kernel family slfp_conv2d_kernel_name reports in the three operand modes MODES, and for depthwise rows what
slfp_debug_dw3x3_variant reports.  twin() is the same layer with the two axes exchanged: it must reach the same family."""
from collections import namedtuple

MODES = ((8, 0), (8, 3), (7, 0))   # (qbits, mfma_passes): single-pass fp16, float32-equivalent, SFP<3,3>

Case = namedtuple("Case", "fam C H W O kh kw sh sw ph pw dh dw g names variant")

PW = ("pw_mfma_f16x1", "pw_mfma_f16x3", "pw_mfma_f16_exact")
RPW = tuple("repad+" + n for n in PW)
DENSE = ("dense_mfma_f16x1", "dense_mfma_f16x3", "dense_mfma_f16_exact")
DENSE_S2 = ("dense_mfma_f16x1", "direct_nhwc", "dense_mfma_f16_exact")   # no float32-equivalent dense kernel off stride 1
SMALL = ("stem_small_mfma_f16x1", "stem_nhwc", "stem_small_mfma_f16_exact")
SMALL_D = ("stem_small_mfma_f16x1", "direct_nhwc", "stem_small_mfma_f16_exact")
STEM = ("stem_nhwc",) * 3
BIG = ("stem_mfma_f16x1", "stem_nhwc", "stem_mfma_f16_exact")
BIG_D = ("stem_mfma_f16x1", "direct_nhwc", "stem_mfma_f16_exact")
DW = ("dw3x3_nhwc",) * 3
RDW = ("repad+dw3x3_nhwc",) * 3
DIRECT = ("direct_nhwc",) * 3


def _two(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _c(fam, C, hw, O, k, s, p, d, g, names, variant=None):
    return Case(fam, C, hw[0], hw[1], O, *_two(k), *_two(s), *_two(p), *_two(d), g, names, variant)


ROWS = [
    # depthwise 3x3: the LDS-tile kernel, the register-window kernel (stride 2), the general kernel (8-byte lanes), padded copies
    _c("dw", 32, (5, 14), 32, 3, 1, 1, 1, 32, DW, "tile"),
    _c("dw", 64, (7, 19), 64, 3, 1, 1, 1, 64, DW, "tile"),
    _c("dw", 32, (9, 20), 32, 3, 1, 0, 1, 32, DW, "tile"),
    _c("dw", 32, (9, 20), 32, 3, 1, 2, 1, 32, DW, "tile"),
    _c("dw", 32, (29, 14), 32, 3, 2, 1, 1, 32, DW, "rows"),
    _c("dw", 58, (9, 20), 58, 3, 1, 1, 1, 58, DW, "general"),
    _c("dw", 58, (21, 10), 58, 3, 2, 1, 1, 58, DW, "general"),
    _c("dw", 29, (8, 13), 29, 3, 1, 1, 1, 29, RDW, "general"),     # of the 32-channel padded copy
    _c("dw", 32, (10, 16), 32, 3, 1, (1, 0), 1, 32, DIRECT, "none"),
    _c("dw", 32, (10, 16), 32, 3, (1, 2), 1, 1, 32, DIRECT, "none"),
    _c("dw", 32, (10, 16), 32, 3, 1, 2, 2, 32, DIRECT, "none"),
    # 1x1
    _c("pw", 64, (5, 23), 128, 1, 1, 0, 1, 1, PW),
    _c("pw", 64, (23, 5), 128, 1, 2, 0, 1, 1, PW),
    _c("pw", 512, (3, 11), 512, 1, 1, 0, 1, 1, PW),
    _c("pw", 58, (7, 12), 58, 1, 1, 0, 1, 1, PW),
    _c("pw", 27, (6, 11), 58, 1, 1, 0, 1, 1, RPW),
    _c("pw", 64, (9, 12), 64, 1, (1, 2), 0, 1, 1, DIRECT),
    _c("pw", 64, (9, 12), 64, 1, 1, (1, 0), 1, 1, DIRECT),
    # dense k x k on the matrix cores
    _c("dense", 16, (11, 18), 32, (3, 5), 1, (1, 2), 1, 1, DENSE),
    _c("dense", 16, (18, 11), 32, (5, 3), 2, (0, 1), 1, 1, DENSE_S2),
    _c("dense", 64, (9, 21), 64, 3, 1, (1, 0), 1, 1, DENSE),       # the persistent resident-weight form in 8/0 and 7/0
    _c("dense", 64, (21, 9), 64, 3, 1, (0, 1), 1, 1, DENSE),
    _c("dense", 64, (10, 37), 64, 3, 1, 1, 1, 1, DENSE),
    _c("dense", 128, (13, 30), 128, 3, 2, 1, 1, 1, DENSE_S2),
    _c("dense", 32, (12, 19), 48, (1, 3), 1, (0, 1), 1, 1, DENSE),
    _c("dense", 32, (19, 12), 48, (3, 1), 1, (1, 0), 1, 1, DENSE),
    _c("dense", 32, (12, 19), 48, (2, 4), 2, (0, 1), 1, 1, DENSE_S2),
    # image stems: one MFMA k-step, the vector kernels, im2row + MFMA
    _c("stem_small", 3, (33, 20), 64, 3, 1, 1, 1, 1, SMALL),
    _c("stem_small", 1, (30, 17), 16, (5, 3), 2, (2, 0), 1, 1, SMALL),
    _c("stem_small", 4, (17, 30), 24, (2, 4), 1, (0, 1), 1, 1, SMALL_D),
    _c("stem", 3, (20, 33), 64, (3, 5), 1, (0, 2), 1, 1, STEM),
    _c("stem", 3, (40, 22), 32, 3, 2, 1, 1, 1, STEM),               # the k_stem_fixed form
    _c("stem_mfma", 3, (41, 26), 32, (7, 5), 2, (3, 1), 1, 1, BIG),
    _c("stem_mfma", 3, (26, 41), 64, (5, 7), 2, (2, 3), 1, 1, BIG),
    _c("stem_mfma", 3, (45, 30), 64, 11, 4, 2, 1, 1, BIG_D),
    _c("stem_mfma", 3, (30, 45), 96, 7, 2, (0, 3), 1, 1, BIG_D),
    _c("stem_mfma", 3, (30, 45), 64, (11, 7), 4, (5, 0), 1, 1, BIG_D),
    # the direct kernel: the only home of stride_h != stride_w, dilation and 1 < groups < C
    _c("direct", 12, (13, 17), 18, (3, 2), (2, 1), (1, 0), (2, 3), 3, DIRECT),
    _c("direct", 16, (12, 20), 32, 3, (1, 2), 1, (2, 1), 1, DIRECT),
    _c("direct", 16, (12, 20), 32, 3, (2, 1), (0, 2), 1, 1, DIRECT),
    _c("direct", 16, (12, 20), 32, 3, 1, 2, 2, 1, DIRECT),
    _c("direct", 3, (20, 33), 32, 3, (2, 1), 1, 1, 1, DIRECT),
    _c("direct", 8, (9, 15), 8, 3, 1, 1, 1, 2, DIRECT),
    _c("direct", 5, (9, 15), 7, (4, 2), (3, 2), (2, 1), (1, 2), 1, DIRECT),
]


def twin(c):
    """The same layer with the two spatial axes exchanged."""
    return c._replace(H=c.W, W=c.H, kh=c.kw, kw=c.kh, sh=c.sw, sw=c.sh, ph=c.pw, pw=c.ph, dh=c.dw, dw=c.dh)


def all_cases():
    """Every row, then every twin that is not itself a row: (case, is_twin, index of the row it comes from)."""
    seen, out = set(), []
    for i, c in enumerate(ROWS):
        seen.add(c[1:14])
        out.append((c, False, i))
    for i, c in enumerate(ROWS):
        t = twin(c)
        if t[1:14] not in seen:
            seen.add(t[1:14])
            out.append((t, True, i))
    return out


FAMILIES = ("dw", "pw", "dense", "stem_small", "stem", "stem_mfma", "direct")


def out_hw(c):
    """The reference's output size (torch.nn.functional.conv2d)."""
    return ((c.H + 2 * c.ph - c.dh * (c.kh - 1) - 1) // c.sh + 1, (c.W + 2 * c.pw - c.dw * (c.kw - 1) - 1) // c.sw + 1)


def desc(lib, c, n, qbits, passes, x_layout=None, y_layout=None):
    """The slfp_conv2d_desc of a case (`lib` is cnns_slfp_quantization_amd._lib); scales are the tests' usual pair."""
    import numpy as np
    return lib.ConvDesc(n=n, c_in=c.C, h=c.H, w=c.W, c_out=c.O, kh=c.kh, kw=c.kw, stride_h=c.sh, stride_w=c.sw, pad_h=c.ph,
                        pad_w=c.pw, dil_h=c.dh, dil_w=c.dw, groups=c.g, x_layout=lib.LAYOUT_NHWC if x_layout is None else x_layout,
                        y_layout=lib.LAYOUT_NHWC if y_layout is None else y_layout, qbits=qbits, ka=float(np.float32(KA)),
                        kw_scale=float(np.float32(KW)), mfma_passes=passes, reserved=0)


KA, KW = 2.6023073196411133 / 15.5, 1.9635683298110962 / 15.5


SWEEP_DRAWS = 200
SWEEP_FAMILIES = ("dw3x3_nhwc", "repad+dw3x3_nhwc", "dense_mfma_f16x1", "dense_mfma_f16x3", "dense_mfma_f16_exact",
                  "stem_small_mfma_f16x1", "stem_mfma_f16x1", "direct_nhwc", "pw_mfma_f16x1", "pw_mfma_f16x3", "pw_mfma_f16_exact",
                  "repad+pw_mfma_f16x1")   # what tests/test_gpu_parity.py's square sweep asserts it reaches


def sweep_draws(seed=20261017, n=SWEEP_DRAWS):
    """The rectangular random sweep of tests/test_gpu_aniso.py: n seeded draws of (case, N, qbits, passes, bias).  H and W are
    drawn independently; kh / kw and pad_h / pad_w independently where the family takes a pair (dense, stems, the direct
    kernel); stride_h == stride_w and dilation 1 except for one draw in five each, which draws the two sides independently
    and lands on the direct kernel.  The ranges leave no degenerate shape (an input smaller than the kernel's extent)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        kind = str(rng.choice(["dw", "pw", "dense", "stem", "any"]))
        if kind == "dw":
            C = int(rng.choice([4, 6, 8, 20, 24, 29, 30, 32, 58, 64, 100, 116])); O = C; g = C
            kh = kw = 3
            sh = sw = int(rng.choice([1, 2]))
            ph = pw = int(rng.integers(0, 3))
        elif kind == "pw":
            C = int(rng.choice([8, 12, 16, 24, 27, 32, 58, 64, 96, 130, 256, 320]))
            O = int(rng.choice([4, 10, 16, 30, 58, 64, 100, 128, 258, 520])); g = 1
            kh = kw = 1
            ph = pw = 0
            sh = sw = int(rng.choice([1, 1, 2]))
        elif kind == "dense":
            C = int(rng.choice([16, 20, 32, 48, 64, 80, 128])); O = int(rng.choice([4, 16, 20, 64, 72, 128, 192, 260])); g = 1
            kh, kw = (int(v) for v in rng.choice([1, 2, 3, 3, 3, 5], 2))
            if kh == kw == 1:
                kw = 3
            sh = sw = int(rng.choice([1, 1, 2]))
            ph, pw = int(rng.integers(0, kh // 2 + 1)), int(rng.integers(0, kw // 2 + 1))
        elif kind == "stem":
            C = int(rng.choice([1, 2, 3, 3, 4])); O = int(rng.choice([4, 8, 16, 24, 32, 64, 96])); g = 1
            kh, kw = (int(v) for v in rng.choice([2, 3, 3, 5, 7, 11], 2))
            sh = sw = int(rng.choice([1, 1, 2, 2, 3, 4]))
            ph, pw = int(rng.integers(0, kh // 2 + 1)), int(rng.integers(0, kw // 2 + 1))
        else:
            C = int(rng.choice([5, 6, 9, 12, 15, 18])); O = int(rng.choice([3, 6, 9, 12, 18]))
            g = int(rng.choice([1, 3])) if (C % 3 == 0 and O % 3 == 0) else 1
            kh, kw = int(rng.integers(1, 8)), int(rng.integers(1, 8))
            sh = sw = int(rng.choice([1, 1, 2, 2, 3, 4]))
            ph, pw = int(rng.integers(0, kh // 2 + 2)), int(rng.integers(0, kw // 2 + 2))
        dh = dw = 1
        if rng.integers(0, 5) == 0:
            sh, sw = int(rng.choice([1, 2, 3])), int(rng.choice([1, 2, 3]))
        if rng.integers(0, 5) == 0:
            dh, dw = int(rng.choice([1, 2, 3])), int(rng.choice([1, 2, 3]))
        H = int(rng.integers(max(dh * (kh - 1) + 1, 2 * sh) + 1, 41))
        W = int(rng.integers(max(dw * (kw - 1) + 1, 2 * sw) + 1, 41))
        qbits = int(rng.choice([8, 8, 7]))
        passes = int(rng.choice([0, 0, 3])) if qbits == 8 else 0
        bias = bool(rng.integers(0, 2))
        N = int(rng.integers(1, 4))
        out.append((Case(kind, C, H, W, O, kh, kw, sh, sw, ph, pw, dh, dw, g, None, None), N, qbits, passes, bias))
    return out


def degenerate(c):
    """An input (with its padding) smaller than the kernel's extent: no output."""
    return c.H + 2 * c.ph < c.dh * (c.kh - 1) + 1 or c.W + 2 * c.pw < c.dw * (c.kw - 1) + 1
