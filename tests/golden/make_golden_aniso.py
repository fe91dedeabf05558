#!/usr/bin/env python3
"""Pin the oracle to the IMPORTED reference on non-square convolutions and write the fixture the suite replays:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_aniso.py --reference <directory of the reference checkout>

make_golden.py's CONV_CASES are all square with one scalar each for kernel size, stride and padding and dilation 1, so the
oracle's handling of (h, w) pairs was never compared with the reference.  The cases here have H != W both ways round,
kh != kw, pad_h != pad_w, stride_h != stride_w, dil_h != dil_w, 1 < groups < C, both bias classes (conv2d_Q without a bias,
conv2d_Q_bias) and Qbits 8 and 7.  For every case the reference's Conv2d_Q module runs on this repository's own seeded
inputs, and the generator asserts what make_golden.py asserts: input_q and weight_q bit-equal to the oracle's, the oracle's
output within 2e-6 (tensor-relative), oracle/torch_port.py bit-equal.

Writes conv_aniso_golden.npz (inputs + the reference's outputs; data only).  The archive is written with fixed member
timestamps, so a rerun reproduces it byte for byte."""
import argparse
import io
import os
import sys
import warnings
import zipfile

import numpy as np

warnings.filterwarnings("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "conv_aniso_golden.npz")

# (name, N, C, H, W, O, (kh, kw), (sh, sw), (ph, pw), (dh, dw), groups, bias, relu_input)
ANISO_CASES = [
    ("dw3_5x14", 2, 32, 5, 14, 32, (3, 3), (1, 1), (1, 1), (1, 1), 32, False, True),
    ("dw3_s2_29x14", 1, 32, 29, 14, 32, (3, 3), (2, 2), (1, 1), (1, 1), 32, False, True),
    ("dw3_d2_10x16_bias", 1, 32, 10, 16, 32, (3, 3), (1, 1), (2, 2), (2, 2), 32, True, True),
    ("pw_s2_23x5", 2, 64, 23, 5, 128, (1, 1), (2, 2), (0, 0), (1, 1), 1, False, True),
    ("dense_3x5_p12_bias", 2, 16, 11, 18, 32, (3, 5), (1, 1), (1, 2), (1, 1), 1, True, True),
    ("dense_5x3_s2_p01", 1, 16, 18, 11, 32, (5, 3), (2, 2), (0, 1), (1, 1), 1, False, True),
    ("stem_7x5_s2_p31_bias", 1, 3, 41, 26, 32, (7, 5), (2, 2), (3, 1), (1, 1), 1, True, False),
    ("stem_11x7_s4_p50", 1, 3, 30, 45, 16, (11, 7), (4, 4), (5, 0), (1, 1), 1, False, False),
    ("g3_3x2_s21_p10_d23_bias", 2, 12, 13, 17, 18, (3, 2), (2, 1), (1, 0), (2, 3), 3, True, True),
    ("s12_p1_d21", 1, 16, 12, 20, 32, (3, 3), (1, 2), (1, 1), (2, 1), 1, False, True),
    ("g2_9x15", 2, 8, 9, 15, 8, (3, 3), (1, 1), (1, 1), (1, 1), 2, False, True),
    ("c5_4x2_s32_p21_d12_bias", 2, 5, 9, 15, 7, (4, 2), (3, 2), (2, 1), (1, 2), 1, True, True),
]
CONV_SCALES = [(2.6023073196411133 / 15.5, 1.9635683298110962 / 15.5),
               (6.629735469818115 / 15.5, 0.5438900589942932 / 15.5),
               (1.7093303203582764 / 15.5, 0.21044661104679108 / 15.5)]


def gen_case(idx, case):
    """Deterministic inputs for one case: the repo's own generator (numpy PCG64), as make_golden.gen_case."""
    name, N, C, H, W, O, k, s, p, d, g, has_bias, relu = case
    rng = np.random.default_rng(7000 + idx)
    Ka, Kw = CONV_SCALES[idx % len(CONV_SCALES)]
    x = rng.standard_normal((N, C, H, W)).astype(np.float32) * np.float32(6.0 * Ka)
    if relu:
        x = np.maximum(x, 0)  # post-ReLU-like: ~50 % exact zeros
    w = rng.standard_normal((O, C // g, k[0], k[1])).astype(np.float32) * np.float32(5.0 * Kw)
    w[rng.random(w.shape) < 0.02] = 0.0  # a few exactly-zero (pruned) weights
    b = (rng.standard_normal(O).astype(np.float32) * np.float32(0.5)) if has_bias else None
    return x, w, b, Ka, Kw


def same_bits(a, b):
    """bit-equal, treating every NaN as equal to every NaN."""
    a, b = a.view(np.uint32), b.view(np.uint32)
    na = (a & 0x7FFFFFFF) > 0x7F800000
    nb = (b & 0x7FFFFFFF) > 0x7F800000
    return np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb])


def save_npz_reproducibly(path, arrays):
    """np.savez_compressed stamps every member with the current time; fixed stamps make the file a function of its data."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for key, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="directory of the reference checkout (holds its utils/ package)")
    args = ap.parse_args()
    ref = os.path.abspath(args.reference)
    sys.path.insert(0, ref)   # `utils` must be the REFERENCE package here, not this repository's drop-in of the same name
    sys.path.insert(1, ROOT)
    sys.path.append(HERE)
    import torch
    import golden_parts as gp
    from oracle import slfp_oracle as so
    from oracle import torch_port as tp
    from utils.conv2d_func import conv2d_Q, conv2d_Q_bias
    assert os.path.abspath(sys.modules["utils.conv2d_func"].__file__).startswith(ref + os.sep), "must import the REFERENCE utils"

    torch.manual_seed(0)
    out, keys, worst = {}, [], 0.0
    for idx, case in enumerate(ANISO_CASES):
        name, N, C, H, W, O, k, s, p, d, g, has_bias, relu = case
        x, w, b, Ka, Kw = gen_case(idx, case)
        out[name + "_x"], out[name + "_w"] = x, w
        if has_bias:
            out[name + "_b"] = b
        out[name + "_meta"] = np.array([N, C, H, W, O, *k, *s, *p, *d, g, int(has_bias)], dtype=np.int64)
        out[name + "_scales"] = np.array([Ka, Kw], dtype=np.float64)
        for q in (8, 7):
            factory = conv2d_Q_bias if has_bias else conv2d_Q
            Conv = factory(q_bit=q, Kw=np.float64(Kw), Ka=np.float64(Ka))
            m = Conv(C, O, k, np.float64(Kw), np.float64(Ka), s, p, d, groups=g, bias=has_bias).eval()
            with torch.no_grad():
                m.weight.copy_(torch.from_numpy(w))
                if has_bias:
                    m.bias.copy_(torch.from_numpy(b))
                y = m(torch.from_numpy(x.copy())).numpy()
                xq, wq = m.input_q.numpy(), m.weight_q.numpy()
            yo, xqo, wqo = so.conv2d(x, w, b, s, p, d, g, Ka, Kw, q, want_q=True)
            assert same_bits(xq, xqo), (name, q, "input_q")
            assert same_bits(wq, wqo), (name, q, "weight_q")
            err = float(np.abs(yo - y).max() / np.abs(y).max())
            worst = max(worst, err)
            assert err < 2e-6, (name, q, err)
            yt, _, _ = tp.conv2d_q(torch.from_numpy(x.copy()), torch.from_numpy(w), None if b is None else torch.from_numpy(b),
                                   s, p, d, g, np.float64(Ka), np.float64(Kw), q)
            assert np.array_equal(yt.numpy(), y), (name, q, "torch_port differs from the reference")
            key = f"{name}_q{q}"
            keys.append(key)
            out[key + "_y"], out[key + "_xq"], out[key + "_wq"] = y, xq, wq
    out["case_keys"] = np.array(keys)
    save_npz_reproducibly(OUT, out)
    size = os.path.getsize(OUT)
    assert size < gp.MAX_PART_BYTES, size
    print(f"aniso conv cases: {len(keys)}; worst oracle-vs-reference max-rel error {worst:.2e}; {os.path.basename(OUT)} {size} bytes")


if __name__ == "__main__":
    main()
