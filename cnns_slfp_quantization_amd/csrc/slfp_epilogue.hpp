// slfp_epilogue.hpp -- the per-tile epilogue of the forward matrix-core kernels (gfx950), written once.
//
// A thread of a forward kernel ends with the four accumulator lanes of a 16x16 MFMA tile (four consecutive output channels of
// one pixel) and does the same work on them whatever the kernel:
//   bias_q256   the quantized-domain bias 256 * ((bias / s1) / s2),
//   epilogue    the reference's two roundings ((acc + bq) * s1x) * s2 (utils/conv2d_func.py:23-24),
//   affine4     the fused BatchNorm affine, one fma per lane,
//   layerout4 (slfp_device.hpp), relu4, res_add      the optional layer-output quantizer, ReLU, residual add + ReLU,
//   code4       the four values' code bytes: the ONE place that chooses between the layer-output byte table, the reader's
//               threshold table with signed codes and the threshold table with the ReLU folded in,
//   store_codes16   four tiles' code dwords through rows_transpose4 and out as one 16-byte store.
// post_apply / post_apply_v / post_apply1 are the PostOp forms of affine -> layerout -> ReLU for the kernels that keep no
// per-channel vectors of their own.  Everything here is __device__ __forceinline__: a kernel's instructions are what they were
// with the arithmetic spelled out at the site (profiles/compare_kernels.py compares two builds by kernel name).
#pragma once
#include "slfp_device.hpp"
#include "slfp_enc.hpp"
#include "slfp_codes.hpp"
#include "slfp_layerout_lut.hpp"

namespace slfp {

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// 256 * bias / s1 / s2 with the reference's two divisions, one channel
__device__ __forceinline__ float bias_q256_1(const float b, const float s1, const float s2) { return 256.f * ((b / s1) / s2); }

// ... of channels n .. n + 3; zeros for a layer without bias
__device__ __forceinline__ float4 bias_q256(const float* bias, int n, const float s1, const float s2) {
    if (!bias) return make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 bb = *reinterpret_cast<const float4*>(bias + n);
    return make_float4(bias_q256_1(bb.x, s1, s2), bias_q256_1(bb.y, s1, s2), bias_q256_1(bb.z, s1, s2), bias_q256_1(bb.w, s1, s2));
}

// out = ((acc * 2^-8 + bq) * s1) * s2 with the 2^-8 folded: ((acc + 256*bq) * (s1/256)) * s2
__device__ __forceinline__ float4 epilogue(const floatx4 acc, const float4 bq256, const float s1x, const float s2) {
    float4 r;
    r.x = ((acc[0] + bq256.x) * s1x) * s2;
    r.y = ((acc[1] + bq256.y) * s1x) * s2;
    r.z = ((acc[2] + bq256.z) * s1x) * s2;
    r.w = ((acc[3] + bq256.w) * s1x) * s2;
    return r;
}

__device__ __forceinline__ float4 affine4(float4 r, const float4 sc, const float4 sh) {
    r.x = __builtin_fmaf(r.x, sc.x, sh.x); r.y = __builtin_fmaf(r.y, sc.y, sh.y);
    r.z = __builtin_fmaf(r.z, sc.z, sh.z); r.w = __builtin_fmaf(r.w, sc.w, sh.w);
    return r;
}

__device__ __forceinline__ float4 relu4(float4 r) {
    r.x = fmaxf(r.x, 0.f); r.y = fmaxf(r.y, 0.f); r.z = fmaxf(r.z, 0.f); r.w = fmaxf(r.w, 0.f);
    return r;
}

// The residual epilogue (slfp_conv2d_fwd_res): t = r + q, one float32 add AFTER the affine's rounding (the library is built
// with -ffp-contract=off, so the add never merges into the fma in front of it), then the ReLU's max: what torch.add and
// torch.relu compute on the unfused result.
__device__ __forceinline__ float4 res_add(float4 r, const float4 q, const int relu) {
    r.x = r.x + q.x; r.y = r.y + q.y; r.z = r.z + q.z; r.w = r.w + q.w;
    return relu ? relu4(r) : r;
}

// ---- PostOp forms: y = relu?(layerout?(r * scale[c] + shift[c])) ----------------------------------------------------
__device__ __forceinline__ float4 post_apply(float4 r, const PostOp po, int c) {
    if (po.scale) r = affine4(r, *reinterpret_cast<const float4*>(po.scale + c), *reinterpret_cast<const float4*>(po.shift + c));
    return po.relu ? relu4(r) : r;
}

// The same split in two, so that kernels whose lanes keep their channels for many outputs load the
// per-channel vectors ONCE: fetched inside the store loop, the two loads sit on the critical path of
// every store (measured: +12-38 % on the pointwise kernels, +5-8 % on depthwise, bench.py --post).
struct PostVec {
    float4 sc, sh;
};

__device__ __forceinline__ PostVec post_load(const PostOp po, int c) {
    PostVec v;
    v.sc = make_float4(1.f, 1.f, 1.f, 1.f);
    v.sh = make_float4(0.f, 0.f, 0.f, 0.f);
    if (po.scale) {
        v.sc = *reinterpret_cast<const float4*>(po.scale + c);
        v.sh = *reinterpret_cast<const float4*>(po.shift + c);
    }
    return v;
}

__device__ __forceinline__ float4 post_apply_v(float4 r, const PostOp po, const PostVec& v) {
    if (po.scale) {
        r = affine4(r, v.sc, v.sh);
        if (po.layerout) r = layerout4(r);
    }
    return po.relu ? relu4(r) : r;
}

__device__ __forceinline__ float post_apply1(float r, const PostOp po, int c) {
    if (po.scale) {
        r = __builtin_fmaf(r, po.scale[c], po.shift[c]);
        if (po.layerout) r = layerout1(r);
    }
    if (po.relu) r = fmaxf(r, 0.f);
    return r;
}

// ---- code output ----------------------------------------------------------------------------------------------------
// The reader's quantizer as a code-writing epilogue needs it: the threshold table's scale and clamp (EncArgs::r1 / lo / hi),
// whether the codes carry a sign (no ReLU in front of the quantizer) and their format (kFmtAct8 | kFmtSfp7).
struct CodeQuant {
    float r1, lo, hi;
    int sgn, fmt;
};

// The 4 code bytes of r (byte k = lane k).
//   LUTQ:      the byte table of the layer-output classes (lut_tab: an LDS array or a lut_gptr); r is the affine's result.
//   q.sgn:     the threshold table (enc_tab, kEncCode, in LDS), codes with a sign.
//   otherwise: the threshold table with the ReLU folded into the quantizer (enc4_code_relu).
// NANFIX (the folded-ReLU choice only): a NaN takes the code of exact zero, what the float32 interface's fmaxf(NaN, 0) followed by
// slfp_encode_f32 gives; without it a NaN takes the code slfp_encode_f32 gives a NaN (0x00).  Which kernel family passes which is
// listed in DESIGN.md ("NaN in front of a folded ReLU").
template <bool LUTQ, bool NANFIX, typename TAB = const unsigned char*>
__device__ __forceinline__ uint32_t code4(const float4 r, const CodeQuant& q, const unsigned char* __restrict__ enc_tab, TAB lut_tab = nullptr) {
    if constexpr (LUTQ) return lut4_code(r, lut_tab);
    else if (q.sgn) return code_sign4(enc4_code<false>(r, q.r1, q.lo, q.hi, enc_tab), r, q.fmt);
    else if constexpr (NANFIX) return enc4_code_relu(relu_of_nan4(r), q.r1, q.lo, q.hi, enc_tab);
    else return enc4_code_relu(r, q.r1, q.lo, q.hi, enc_tab);
}

// c[j] = the code dword of channel tile j (4 channels) of this lane's pixel, j = 0..3.  After the transpose lane-quarter kq holds
// the 16 consecutive channel codes of tile kq: `dst` is that run's address, `ok` guards the store only (every lane of the wave
// takes part in the transpose).
__device__ __forceinline__ void store_codes16(uint32_t (&c)[4], uint8_t* dst, const bool ok) {
    rows_transpose4(c[0], c[1], c[2], c[3]);
    if (ok) *reinterpret_cast<u32x4*>(dst) = u32x4{c[0], c[1], c[2], c[3]};
}

}  // namespace slfp
