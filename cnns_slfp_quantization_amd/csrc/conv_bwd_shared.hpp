// conv_bwd_shared.hpp -- what conv_bwd.hip lends the other backward translation units (conv_bwd_bf16.hip, conv_bwd_dense_bf16.hip):
// the family tests, the dense geometry, the split rule of a weight-gradient contraction and the fixed-order reduction of its
// partials.  Defined in conv_bwd.hip.
#pragma once
#include "slfp_host.hpp"

namespace slfp {

// stride-1 pad-0 groups-1 1x1 layers (a Linear_Q is one with h = w = 1): the `pw` family of bwd_kind
bool bwd_is_pw(const slfp_conv2d_desc& d);
// what SLFP_BWD_DENSE adds under `flags`: groups 1, dilation 1, any kernel size / stride / padding that is neither pw nor the
// depthwise 3x3, within dense_ok's 32-bit limits
bool bwd_is_dense(const slfp_conv2d_desc& d, const ConvPlan& p, unsigned flags);

// The geometry of a dense layer as its kernels take it.
struct DenseGeom {
    int N, H, W, Cin, Ho, Wo, Cout, KH, KW, sh, sw, padh, padw;
};
DenseGeom dense_geom(const slfp_conv2d_desc& d, const ConvPlan& p);

// rows (input pixels) of phase (a, b): n x ceil((H - a) / sh) x ceil((W - b) / sw)
__host__ __device__ __forceinline__ int dense_phase_extent(int extent, int phase, int stride) {
    return (extent - phase + stride - 1) / stride;
}
// workgroups of a dense gx kernel along x: the 128-row tiles of every (h mod stride_h, w mod stride_w) phase, phases in (a, b) order
int64_t dense_gx_tiles(const DenseGeom& g);

// The split of a GW contraction over its M rows: ~8 workgroups per CU, at least 256 rows per split, partials (cout x ncol
// and the cout bias sums per split) within 32 MiB, at most 1024 splits, each a whole number of 16-row k-steps.
struct GwSplit {
    int splits, kps;
};
GwSplit gw_split(int64_t M, int64_t cout, int64_t ncol, int64_t tiles);

// k_reduce_parts: gw[col] = scale * sum_p part[p][col] in a fixed order (dwC, Cin, T: the depthwise / dense output layouts; 0 here)
int reduce_parts(hipStream_t st, const float* part, int P, int64_t ncols, float scale, int dwC, int Cin, int T, float* gw, float* gb);
// gb[co] = sum over the splits of the GW kernels' bias partials
int reduce_gb(hipStream_t st, const float* gbpart, int splits, int64_t cout, float* gb);

}  // namespace slfp
