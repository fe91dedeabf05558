"""Parity bars of a conv kernel family against the CPU oracle (BASELINE.json north_star), shared by the GPU tests.

    max|d| <= tol * max|ref|   and   ||d||_2 <= tol * ||ref||_2        (conftest.rel_errors)

and, on outputs of ELEM_MIN elements or more, at most elem_frac_bar(kern) of the elements beyond 1e-3 * |ref|
(conftest.elem_exceed_frac)."""
TOL_EXACT = 1e-5   # float32-equivalent paths
TOL_F16X1 = 1e-3   # north-star tolerance; measured ~2.5e-4
ELEM_MIN = 2048    # the elementwise fraction is a statistical bound: meaningless on a few dozen outputs


def tol(kern):
    """Single-pass fp16 MFMA kernels (pointwise and dense k x k) are held to the north-star 1e-3;
    everything else (fp32 VALU kernels, fp16x3, SFP<3,3>-exact MFMA) to float32 round-off."""
    return TOL_F16X1 if kern.endswith("_f16x1") else TOL_EXACT


def elem_frac_bar(kern):
    """Float32-equivalent kernels: only cancellation noise near zero crossings; single-pass fp16 MFMA: SURVEY section 7
    measured 14 % (mean 13-14 %)."""
    return 0.30 if kern.endswith("_f16x1") else 0.02
