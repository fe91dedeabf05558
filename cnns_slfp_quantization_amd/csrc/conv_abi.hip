// conv_abi.hip -- C ABI for the quantized conv2d / linear forward (include/slfp.h):
// descriptor validation, kernel selection, weight preparation, dispatch.
#include <algorithm>
#include <cstring>
#include "slfp_device.hpp"
#include "slfp_codes.hpp"
#include "slfp_layerout_lut.hpp"
#include "slfp_host.hpp"

namespace slfp {

static size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }

static int make_plan_core(const slfp_conv2d_desc* d, ConvPlan* plan) {
    if (!d || !plan) return fail(SLFP_ERR_BAD_ARG, "conv2d: null descriptor");
    if (d->n <= 0 || d->c_in <= 0 || d->h <= 0 || d->w <= 0 || d->c_out <= 0 || d->kh <= 0 || d->kw <= 0)
        return fail(SLFP_ERR_SHAPE, "conv2d: non-positive size");
    if (d->stride_h <= 0 || d->stride_w <= 0 || d->dil_h <= 0 || d->dil_w <= 0 || d->pad_h < 0 || d->pad_w < 0)
        return fail(SLFP_ERR_SHAPE, "conv2d: bad stride/dilation/padding");
    if (d->groups <= 0 || d->c_in % d->groups || d->c_out % d->groups)
        return fail(SLFP_ERR_SHAPE, "conv2d: groups=%d does not divide C_in=%lld / C_out=%lld", d->groups,
                    (long long)d->c_in, (long long)d->c_out);
    if (d->qbits != 8 && d->qbits != 7)
        return fail(SLFP_ERR_BAD_ARG, "conv2d: qbits must be 8 (SLFP<3,4>) or 7 (SFP<3,3>), got %d", d->qbits);
    if ((d->x_layout != SLFP_LAYOUT_NCHW && d->x_layout != SLFP_LAYOUT_NHWC) ||
        (d->y_layout != SLFP_LAYOUT_NCHW && d->y_layout != SLFP_LAYOUT_NHWC))
        return fail(SLFP_ERR_BAD_ARG, "conv2d: unknown layout");
    if (!(d->ka > 0.f) || !(d->kw_scale > 0.f)) return fail(SLFP_ERR_BAD_ARG, "conv2d: Ka and Kw must be > 0");
    if (!scale_div_ok(d->ka) || !scale_div_ok(d->kw_scale))
        return fail(SLFP_ERR_UNSUPPORTED, "conv2d: Ka and Kw must be within [1e-30, 1e30]");
    if (d->mfma_passes != SLFP_MFMA_DEFAULT && d->mfma_passes != SLFP_MFMA_F16X1 && d->mfma_passes != SLFP_MFMA_F16X3)
        return fail(SLFP_ERR_BAD_ARG, "conv2d: mfma_passes must be 0, 1 or 3");
    const int64_t eh = d->h + 2 * (int64_t)d->pad_h - (int64_t)d->dil_h * (d->kh - 1) - 1;
    const int64_t ew = d->w + 2 * (int64_t)d->pad_w - (int64_t)d->dil_w * (d->kw - 1) - 1;
    if (eh < 0 || ew < 0) return fail(SLFP_ERR_SHAPE, "conv2d: kernel larger than the padded input");
    plan->h_out = eh / d->stride_h + 1;
    plan->w_out = ew / d->stride_w + 1;
    if (d->n > 0x7FFFFFFF || d->h > 0x7FFFFFFF || d->w > 0x7FFFFFFF || d->c_in > 0x7FFFFFFF || d->c_out > 0x7FFFFFFF)
        return fail(SLFP_ERR_UNSUPPORTED, "conv2d: dimension exceeds 2^31");
    plan->fmt_act = d->qbits == 8 ? kFmtAct8 : kFmtSfp7;
    plan->fmt_w = d->qbits == 8 ? kFmtW8 : kFmtSfp7;
    plan->passes = d->qbits == 7 ? 1 : (d->mfma_passes == SLFP_MFMA_F16X3 ? 3 : 1);
    plan->k_pad = plan->n_pad = 0;
    plan->repad = false;
    plan->cpi = d->c_in; plan->cpo = d->c_out;
    plan->s1 = d->ka;
    plan->s2 = d->kw_scale;
    const int64_t cg = d->c_in / d->groups;
    const bool sq_stride = d->stride_h == d->stride_w;
    if (d->groups == d->c_in && d->c_out == d->c_in && d->kh == 3 && d->kw == 3 && d->dil_h == 1 && d->dil_w == 1 &&
        sq_stride && (d->stride_h == 1 || d->stride_h == 2) && d->pad_h == d->pad_w && d->pad_h <= 2 &&
        (d->c_in % 2) == 0) {   // multiples of 4: 16-byte lanes; other even counts (58): 8-byte lanes
        plan->family = kDw3x3;
        plan->wprep_bytes = round256((size_t)9 * d->c_in * sizeof(float));
    } else if (d->kh == 1 && d->kw == 1 && d->groups == 1 && d->pad_h == 0 && d->pad_w == 0 && sq_stride &&
               (((d->c_in % 4) == 0 && (d->c_out % 4) == 0) ||
                // even channel counts (ShuffleNetV2: 58): the LDS-resident stream kernel with 8-byte accesses
                ((d->c_in % 2) == 0 && (d->c_out % 2) == 0 && d->c_in >= 8 &&
                 pointwise_stream_fits(ceil_div(d->c_in, 64) * 64, ceil_div(d->c_out, 64) * 64, plan->passes)))) {
        plan->family = kPointwise;
        plan->k_pad = ceil_div(d->c_in, 64) * 64;
        plan->n_pad = ceil_div(d->c_out, 64) * 64;
        plan->wprep_bytes = round256((size_t)2 * plan->k_pad * plan->n_pad * sizeof(_Float16));
    } else if (stem_small_applicable(*d, plan->passes)) {
        plan->family = kStemSmall;
        plan->n_pad = stem_small_tiles(*d);  // 16-channel tiles
        plan->wprep_bytes = round256((size_t)plan->n_pad * 1024);
    } else if (stem_mfma_applicable(*d, plan->passes)) {
        plan->family = kStemMfma;
        int ksub, nt;
        stem_mfma_blob_shape(*d, &ksub, &nt);
        plan->k_pad = ksub;  // k-steps per tap row
        plan->n_pad = nt;    // 16-channel tiles
        plan->wprep_bytes = round256((size_t)d->kh * ksub * nt * 1024);
    } else if (dense_mfma_applicable(*d, plan->passes)) {
        plan->family = kDenseMfma;
        plan->k_pad = ceil_div(d->c_in, 64) * 64;
        plan->n_pad = ceil_div(d->c_out, 16) * 16;
        // one fp16 plane, plus the residual plane in float32-equivalent mode
        plan->wprep_bytes = round256((size_t)(plan->passes == 3 ? 2 : 1) * d->kh * d->kw * plan->k_pad * plan->n_pad * sizeof(_Float16));
    } else {
        plan->family = kDirect;
        plan->wprep_bytes = round256((size_t)d->kh * d->kw * cg * d->c_out * sizeof(float));
    }
    return SLFP_OK;
}

static int64_t round4(int64_t c) { return (c + 3) & ~(int64_t)3; }

// The descriptor of the channel-padded launch, if this layer qualifies (see ConvPlan::repad).
static bool padded_desc(const slfp_conv2d_desc& d, slfp_conv2d_desc* d2) {
    if ((d.c_in % 4) == 0 && (d.c_out % 4) == 0) return false;
    *d2 = d;
    d2->x_layout = d2->y_layout = SLFP_LAYOUT_NHWC;
    if (d.groups == d.c_in && d.c_out == d.c_in) {          // depthwise
        d2->c_in = d2->c_out = round4(d.c_in);
        d2->groups = (int32_t)d2->c_in;
    } else if (d.groups == 1 && d.kh == 1 && d.kw == 1 && d.c_in >= 8) {  // pointwise
        d2->c_in = round4(d.c_in);
        d2->c_out = round4(d.c_out);
    } else {
        return false;
    }
    return true;
}

int make_plan(const slfp_conv2d_desc* d, ConvPlan* plan) {
    int rc = make_plan_core(d, plan);
    if (rc != SLFP_OK || plan->family != kDirect) return rc;
    slfp_conv2d_desc d2;
    if (!padded_desc(*d, &d2)) return rc;
    ConvPlan inner;
    if (make_plan_core(&d2, &inner) != SLFP_OK || (inner.family != kDw3x3 && inner.family != kPointwise)) return rc;
    const int64_t ho = plan->h_out, wo = plan->w_out;
    *plan = inner;
    plan->h_out = ho; plan->w_out = wo;
    plan->repad = true;
    plan->cpi = d2.c_in; plan->cpo = d2.c_out;
    return SLFP_OK;
}

// dst[row][c] = c < cs ? src[row][c] : 0 for c < cd  (channel re-padding of an NHWC tensor, either way).
// V = floats per thread: 2 when both widths are even (58 <-> 60: 8-byte accesses), else 1.
template <int V>
__global__ __launch_bounds__(256) void k_repad(const float* __restrict__ src, float* __restrict__ dst, int64_t total_v,
                                               int cs, int cd) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total_v) return;
    const int cdv = cd / V;
    const int64_t row = idx / cdv;
    const int c = (int)(idx - row * cdv) * V;
    if (V == 2) {
        float2 v = make_float2(0.f, 0.f);
        if (c < cs) v = *reinterpret_cast<const float2*>(src + row * cs + c);
        *reinterpret_cast<float2*>(dst + row * cd + c) = v;
    } else {
        dst[idx] = c < cs ? src[row * cs + c] : 0.f;
    }
}

static int launch_repad(const float* src, float* dst, int64_t rows, int64_t cs, int64_t cd, hipStream_t stream) {
    if ((cs % 2) == 0 && (cd % 2) == 0) {
        const int64_t total = rows * (cd / 2);
        hipLaunchKernelGGL(k_repad<2>, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, stream, src, dst, total, (int)cs, (int)cd);
    } else {
        const int64_t total = rows * cd;
        hipLaunchKernelGGL(k_repad<1>, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, stream, src, dst, total, (int)cs, (int)cd);
    }
    return check_launch("slfp channel re-pad kernel");
}

// One thread per OIHW weight element: weight_q = QW(w / Kw) (utils/conv2d_func.py:22), written
// in the layout the selected kernel family reads.
// CODES: `w` is not float32 weights but their 1-byte extended codes (slfp_encode_f32 with SLFP_FMT_EXT): the value is
// decoded instead of quantized (decode(encode(x)) == quantize(x) bit for bit), so a blob built from broadcast codes
// is identical to one built from the weights themselves (multi-GPU: sharding.py).
template <int FMT, bool CODES = false>
__global__ __launch_bounds__(256) void k_prepare(const float* __restrict__ w, void* __restrict__ prep,
                                                 float* __restrict__ wq_oihw, int64_t total, int O, int Cg, int KH,
                                                 int KW, const ScaleDiv sd, int family, int KS, int64_t plane, int ldo) {
    __shared__ uint32_t sT[16];
    lut_fill<FMT>(sT);   // W8 / SFP7: the identity table the decoder indexes as well
    __syncthreads();
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    float q;
    if constexpr (CODES) q = __uint_as_float(decode_bits<FMT>(reinterpret_cast<const uint8_t*>(w)[idx], true, sT));
    else q = quantize_scaled<FMT>(w[idx], sd, sT);
    if (wq_oihw) wq_oihw[idx] = q;
    int64_t r = idx;
    const int kw = (int)(r % KW); r /= KW;
    const int kh = (int)(r % KH); r /= KH;
    const int ci = (int)(r % Cg); r /= Cg;
    const int o = (int)r;
    if (family == kDw3x3) {
        reinterpret_cast<float*>(prep)[(size_t)(kh * 3 + kw) * ldo + o] = q;  // [9][C (padded)]
    } else if (family == kDirect) {
        reinterpret_cast<float*>(prep)[((size_t)(kh * KW + kw) * Cg + ci) * O + o] = q;  // [KH][KW][Cg][O]
    } else if (family == kStemSmall) {
        // one 32-deep k-step: k = (kh*KW + kw)*C_in + ci; A-fragment lane (k/8, o%16), element k%8: conv_stem_small.hip
        const int k = (kh * KW + kw) * Cg + ci;
        const size_t at = (((size_t)(o >> 4) * 64) + (size_t)((k >> 3) * 16 + (o & 15))) * 8 + (k & 7);
        reinterpret_cast<_Float16*>(prep)[at] = (_Float16)(16.0f * q);
    } else if (family == kStemMfma) {
        // K = (kh, run element r = kw*C_in + ci padded to 32*KS): k-step kh*KS + r/32, lane-quarter (r%32)/8;
        // `plane` carries the number of channel tiles: conv_stem_mfma.hip
        const int r = kw * Cg + ci, ks = kh * KS + (r >> 5);
        const size_t at = ((((size_t)ks * plane + (o >> 4)) * 64) + (size_t)(((r & 31) >> 3) * 16 + (o & 15))) * 8 + (r & 7);
        reinterpret_cast<_Float16*>(prep)[at] = (_Float16)(16.0f * q);
    } else if (family == kDenseMfma) {
        // tap-major copy of the pointwise fragment order (single fp16 plane): conv_dense.hip
        const int nt = o >> 4, row = o & 15, ks = ci >> 5, kk = ci & 31;
        const int kq = (kk & 15) >> 2, j = (kk >> 4) * 4 + (kk & 3);
        const size_t ntiles = (size_t)(plane / ((int64_t)KS * 32 * 16));
        const size_t at = ((((size_t)(kh * KW + kw) * ntiles + nt) * KS + ks) * 64 + (size_t)(kq * 16 + row)) * 8 + j;
        const float v = 16.0f * q;
        const _Float16 hi = (_Float16)v;
        reinterpret_cast<_Float16*>(prep)[at] = hi;
        if (ldo) reinterpret_cast<_Float16*>(prep)[(size_t)KH * KW * plane + at] = (_Float16)(v - (float)hi);  // ldo != 0: residual plane
    } else {
        // MFMA 16x16x32 A-fragment order: tile (o/16, k/32), lane = kq*16 + o%16 where lane-quarter kq
        // holds k%32 in {kq*4..kq*4+3} (elements 0-3) and {16+kq*4..16+kq*4+3} (elements 4-7): conv_pw.hip
        const int nt = o >> 4, row = o & 15, ks = ci >> 5, kk = ci & 31;
        const int kq = (kk & 15) >> 2, j = (kk >> 4) * 4 + (kk & 3);
        const size_t at = (((size_t)nt * KS + ks) * 64 + (size_t)(kq * 16 + row)) * 8 + j;
        const float v = 16.0f * q;  // 2^4 pre-scale (exact), see conv_pw.hip
        const _Float16 hi = (_Float16)v;
        _Float16* blob = reinterpret_cast<_Float16*>(prep);
        blob[at] = hi;
        blob[plane + at] = (_Float16)(v - (float)hi);
    }
}

int launch_prepare_weights(const slfp_conv2d_desc& d, const ConvPlan& p, const float* w_oihw, void* wprep,
                           float* weight_q_oihw, hipStream_t stream, bool codes) {
    const int Cg = (int)(d.c_in / d.groups);
    const int64_t total = d.c_out * Cg * d.kh * d.kw;
    if (p.family == kPointwise || p.family == kDenseMfma || p.family == kStemMfma || p.family == kStemSmall || p.repad) {
        if (hipMemsetAsync(wprep, 0, p.wprep_bytes, stream) != hipSuccess) return check_launch("hipMemsetAsync(wprep)");
    }
    const int64_t plane = p.family == kStemMfma ? p.n_pad : p.k_pad * p.n_pad;
    const int KS = p.family == kStemMfma ? (int)p.k_pad : (int)(p.k_pad / 32);
    const unsigned grid = (unsigned)ceil_div(total, 256);
    const ScaleDiv sd = make_scale_div(d.kw_scale);
    // depthwise: row pitch of the [9][C] table (padded channel count); dense MFMA: 1 = also write the residual plane
    const int ldo = p.family == kDenseMfma ? (p.passes == 3 ? 1 : 0) : (int)p.cpo;
#define SLFP_PREP(FF, CC) hipLaunchKernelGGL((k_prepare<FF, CC>), dim3(grid), dim3(256), 0, stream, w_oihw, wprep, weight_q_oihw, total, \
                                             (int)d.c_out, Cg, (int)d.kh, (int)d.kw, sd, (int)p.family, KS, plane, ldo)
    if (p.fmt_w == kFmtW8) { if (codes) SLFP_PREP(kFmtW8, true); else SLFP_PREP(kFmtW8, false); }
    else { if (codes) SLFP_PREP(kFmtSfp7, true); else SLFP_PREP(kFmtSfp7, false); }
#undef SLFP_PREP
    return check_launch("slfp weight prepare kernel");
}

static const char* family_name(const ConvPlan& p, const slfp_conv2d_desc& d) {
    if (p.family == kDirect && stem_applicable(d)) return "stem_nhwc";
    if (p.repad) {  // the same kernels on channel-padded copies (ConvPlan::repad)
        if (p.family == kDw3x3) return "repad+dw3x3_nhwc";
        return p.fmt_act == kFmtSfp7 ? "repad+pw_mfma_f16_exact" : (p.passes == 3 ? "repad+pw_mfma_f16x3" : "repad+pw_mfma_f16x1");
    }
    switch (p.family) {
        case kDw3x3: return "dw3x3_nhwc";
        case kPointwise: return p.fmt_act == kFmtSfp7 ? "pw_mfma_f16_exact" : (p.passes == 3 ? "pw_mfma_f16x3" : "pw_mfma_f16x1");
        case kDenseMfma: return p.fmt_act == kFmtSfp7 ? "dense_mfma_f16_exact" : (p.passes == 3 ? "dense_mfma_f16x3" : "dense_mfma_f16x1");
        case kStemMfma: return p.fmt_act == kFmtSfp7 ? "stem_mfma_f16_exact" : "stem_mfma_f16x1";
        case kStemSmall: return p.fmt_act == kFmtSfp7 ? "stem_small_mfma_f16_exact" : "stem_small_mfma_f16x1";
        default: return "direct_nhwc";
    }
}

}  // namespace slfp

using namespace slfp;

static const char* pw_variant(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, bool has_res, bool has_res_codes, int64_t y_ld);
static const char* dw3x3_instance(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, bool has_bias, int post_flags, bool has_post);
static const char* stem_instance(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, bool has_bias, int post_flags, bool has_post);

extern "C" {

int slfp_conv2d_out_shape(const slfp_conv2d_desc* d, int64_t* h_out, int64_t* w_out) {
    ConvPlan p;
    const int rc = make_plan(d, &p);
    if (rc != SLFP_OK) return rc;
    if (h_out) *h_out = p.h_out;
    if (w_out) *w_out = p.w_out;
    return SLFP_OK;
}

const char* slfp_conv2d_kernel_name(const slfp_conv2d_desc* d) {
    ConvPlan p;
    if (make_plan(d, &p) != SLFP_OK) return "invalid";
    return family_name(p, *d);
}

const char* slfp_debug_dw3x3_variant(const slfp_conv2d_desc* d, int has_post) {
    ConvPlan p;
    if (make_plan(d, &p) != SLFP_OK || p.family != kDw3x3) return "none";
    static const float one = 1.f;   // the predicates only ask whether a scale / shift pair is present
    const PostOp post = {has_post ? &one : nullptr, has_post ? &one : nullptr, 0, 0};
    if (dw3x3_rows_applicable(*d, p, nullptr, post)) return "rows";
    return dw3x3_tile_applicable(*d, p, nullptr, post) ? "tile" : "general";
}

const char* slfp_debug_dw3x3_instance(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, int has_bias, int post_flags, int has_post) {
    return dw3x3_instance(d, io, has_bias != 0, post_flags, has_post != 0);
}

const char* slfp_debug_stem_instance(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, int has_bias, int post_flags, int has_post) {
    return stem_instance(d, io, has_bias != 0, post_flags, has_post != 0);
}

const char* slfp_debug_dense_variant(const slfp_conv2d_desc* d, int x_codes) {
    ConvPlan p;
    if (make_plan(d, &p) != SLFP_OK) return "none";
    return dense_variant_name(*d, p, x_codes != 0);
}

const char* slfp_debug_pw_variant(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, int has_res, int has_res_codes, int64_t y_ld) {
    return pw_variant(d, io, has_res != 0, has_res_codes != 0, y_ld);
}

size_t slfp_conv2d_wprep_bytes(const slfp_conv2d_desc* d) {
    ConvPlan p;
    if (make_plan(d, &p) != SLFP_OK) return 0;
    return p.wprep_bytes;
}

static int prepare_weights(const char* fn, const slfp_conv2d_desc* d, const void* w, void* wprep, float* weight_q_oihw, void* stream,
                           bool codes) {
    ConvPlan p;
    const int rc = make_plan(d, &p);
    if (rc != SLFP_OK) return rc;
    if (!w || !wprep) return fail(SLFP_ERR_BAD_ARG, "%s: null pointer", fn);
    if (!aligned16(wprep)) return fail(SLFP_ERR_ALIGNMENT, "%s: wprep must be 16-byte aligned", fn);
    return launch_prepare_weights(*d, p, reinterpret_cast<const float*>(w), wprep, weight_q_oihw, as_stream(stream), codes);
}

int slfp_conv2d_prepare_weights(const slfp_conv2d_desc* d, const float* w_oihw, void* wprep, float* weight_q_oihw,
                                void* stream) {
    return prepare_weights("slfp_conv2d_prepare_weights", d, w_oihw, wprep, weight_q_oihw, stream, false);
}

int slfp_conv2d_prepare_weights_codes(const slfp_conv2d_desc* d, const uint8_t* codes_oihw, void* wprep, float* weight_q_oihw,
                                      void* stream) {
    return prepare_weights("slfp_conv2d_prepare_weights_codes", d, codes_oihw, wprep, weight_q_oihw, stream, true);
}

}  // extern "C"

// Where each part of the workspace lies: byte offsets in this order, the copies rounded up to 256 bytes; a part the call does
// not need takes no room.  slfp_conv2d_workspace_bytes reports `total`, the forward carves the buffer by the same offsets.
struct WsLayout {
    size_t x_nhwc, y_nhwc;   // NCHW <-> NHWC copies of x and y
    size_t operand;          // dense k x k: the input encoded once to fp16; large-kernel stem: the im2row'ed input
    size_t x_pad, y_pad;     // channel-padded copies (ConvPlan::repad)
    size_t vec[3];           // bias / post_scale / post_shift, padded (read 16 bytes at a time)
    size_t total;
};

static WsLayout ws_layout(const slfp_conv2d_desc* d, const ConvPlan& p) {
    WsLayout l;
    size_t at = 0;
    auto take = [&at](bool needed, size_t bytes) { const size_t off = at; if (needed) at += bytes; return off; };
    l.x_nhwc = take(d->x_layout == SLFP_LAYOUT_NCHW, round256((size_t)d->n * d->c_in * d->h * d->w * sizeof(float)));
    l.y_nhwc = take(d->y_layout == SLFP_LAYOUT_NCHW, round256((size_t)d->n * d->c_out * p.h_out * p.w_out * sizeof(float)));
    l.operand = at;
    if (p.family == kDenseMfma) at += dense_mfma_workspace_bytes(*d, p.passes);
    if (p.family == kStemMfma) at += stem_mfma_workspace_bytes(*d, p.w_out);
    l.x_pad = take(p.repad && p.cpi != d->c_in, round256((size_t)d->n * d->h * d->w * p.cpi * sizeof(float)));
    l.y_pad = take(p.repad && p.cpo != d->c_out, round256((size_t)d->n * p.h_out * p.w_out * p.cpo * sizeof(float)));
    for (size_t& v : l.vec) v = take(p.repad, round256((size_t)p.cpo * sizeof(float)));
    l.total = at;
    return l;
}

extern "C" size_t slfp_conv2d_workspace_bytes(const slfp_conv2d_desc* d) {
    ConvPlan p;
    if (make_plan(d, &p) != SLFP_OK) return 0;
    return ws_layout(d, p).total;
}

// ---- 1-byte activation codes between layers (include/slfp.h; csrc/slfp_codes.hpp) ----
// The kernel a call with codes on either side goes to.
enum CodeRoute {
    kRouteNone = 0,    // no code-path kernel for the layer / io combination
    kRouteDwc,         // depthwise 3x3 on codes
    kRoutePwc,         // pointwise on codes
    kRouteStemCodes,   // the image stem with code output
    kRouteDense,       // dense k x k (needs the workspace)
    kRouteStemSmall,   // the small-K MFMA stem with code output
    kRouteStemMfma,    // the large-kernel MFMA stem with code output (its two-kernel form needs the workspace)
};

static int y_fmt_of(int y_qbits) { return y_qbits == 7 ? kFmtSfp7 : kFmtAct8; }

// Is the consumer's quantizer in `io` (format and scale of the codes to write) one the kernels can apply?
static bool consumer_quant_ok(const slfp_conv2d_io* io) {
    return (io->y_qbits == 8 || io->y_qbits == 7) && io->y_ka > 0.f && scale_div_ok(io->y_ka);
}

// What all code-path kernels share: NHWC on both sides, known flag bits, no layer-output quantizer, the threshold tables in use.
static bool code_path_ok(const slfp_conv2d_desc* d, int relu) {
    if (d->x_layout != SLFP_LAYOUT_NHWC || d->y_layout != SLFP_LAYOUT_NHWC) return false;
    if ((relu & ~(SLFP_POST_RELU | SLFP_POST_LAYEROUT)) != 0 || (relu & SLFP_POST_LAYEROUT)) return false;
    return !long_encode_forced();
}

// The three route functions take the plan make_plan built for `d`.
// need_table: the producer applies the reader's quantizer through its threshold table (not the table epilogue: lut_route).
static CodeRoute codes_route(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, bool has_bias, int relu, const ConvPlan& p, bool need_table = true) {
    if (!code_path_ok(d, relu)) return kRouteNone;
    if (io->y_codes && (!consumer_quant_ok(io) || (need_table && !enc_table(io->y_ka, y_fmt_of(io->y_qbits), kEncCode)->valid))) return kRouteNone;
    if (io->x_codes) {
        if (dwc_applicable(*d, p, has_bias ? reinterpret_cast<const float*>(1) : nullptr, relu)) return kRouteDwc;
        if (pwc_applicable(*d, p, relu, io->y_codes != 0)) return kRoutePwc;
        if (dense_codes_applicable(*d, p, relu, io->y_codes != 0)) return kRouteDense;
        return kRouteNone;
    }
    if (!io->y_codes) return kRouteNone;
    if (stem_codes_applicable(*d, p, relu)) return kRouteStemCodes;
    if (dense_codes_applicable(*d, p, relu, true)) return kRouteDense;
    if (stem_small_codes_applicable(*d, p, relu)) return kRouteStemSmall;
    if (stem_mfma_codes_applicable(*d, p, relu)) return kRouteStemMfma;
    return kRouteNone;
}

// The kernels whose code store takes a pixel stride (a channel slice of a wider tensor): pw_mfma_* on codes, the dense code epilogue.
static bool slice_route(CodeRoute route) { return route == kRoutePwc || route == kRouteDense; }
static bool y_ld_ok(const slfp_conv2d_desc* d, int64_t y_ld) { return y_ld >= d->c_out && y_ld % 16 == 0 && y_ld <= 0x7FFFFFFF; }

// Pointwise, float32 in -> codes out: the layer at which a chain of codes begins (slfp_conv2d_fwd_entry).  A query and an entry
// point of their own: slfp_conv2d_codes_supported keeps answering 0 for this combination, so every link count that rests on it stays.
static bool entry_route(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, int relu, const ConvPlan& p) {
    if (io->x_codes != 0 || io->y_codes != 1 || !code_path_ok(d, relu) || !consumer_quant_ok(io)) return false;
    return pointwise_entry_applicable(*d, p, relu, io->y_ka, y_fmt_of(io->y_qbits));
}

// A residual operand in the pointwise epilogue (slfp_conv2d_fwd_res): float32 out, no layer-output quantizer.
static bool res_route(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, bool has_bias, int relu, const ConvPlan& p) {
    if ((relu & ~SLFP_POST_RELU) != 0 || io->y_codes || !code_path_ok(d, relu)) return false;
    if (!io->x_codes) return pointwise_res_applicable(*d, p);
    const slfp_conv2d_io cio{1, 0, 1.f, 8};
    return p.family == kPointwise && d->stride_h == 1 && d->stride_w == 1 && codes_route(d, &cio, has_bias, relu, p) == kRoutePwc;
}

// The residual epilogue on codes that also writes the next block's codes (slfp_conv2d_fwd_res_codes): exactly where the residual route
// takes the layer with code input and float32 output, C_out is whole 16-channel tiles and the reader's quantizer has a code table.  A
// query and an entry point of their own: slfp_conv2d_res_supported keeps refusing y_codes.
static bool res_codes_route(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, bool has_bias, int relu, const ConvPlan& p) {
    if (io->x_codes != 1 || io->y_codes != 1 || d->c_out % 16 != 0 || !consumer_quant_ok(io)) return false;
    const slfp_conv2d_io rio{1, 0, 1.f, 8};
    return res_route(d, &rio, has_bias, relu, p) && enc_table(io->y_ka, y_fmt_of(io->y_qbits), kEncCode)->valid;
}

// The table epilogue (slfp_conv2d_fwd_codes_lut): the code route of the same layer without the layer-output bit, where the
// selected kernel has a table instance: depthwise 3x3 and 1x1 on codes, dense 3x3 (codes or float32 in), the two 3x3 RGB stems.
// Large-kernel stems, the entry kernel and the residual forms have none.  A query and an entry point of their own: the four
// older queries keep refusing SLFP_POST_LAYEROUT.
static CodeRoute lut_route(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, bool has_bias, const ConvPlan& p) {
    if (io->y_codes != 1 || (io->x_codes != 0 && io->x_codes != 1) || !consumer_quant_ok(io)) return kRouteNone;
    // the reader's scale and format are validated as for slfp_conv2d_fwd_codes; its threshold table is not needed
    const CodeRoute route = codes_route(d, io, has_bias, 0, p, false);
    switch (route) {
        case kRouteDwc: case kRouteStemCodes: case kRouteStemSmall: return route;
        case kRoutePwc: return strcmp(pwc_variant_name(*d, p, true, false, false, true), "none") != 0 ? route : kRouteNone;
        case kRouteDense: return dense_lut_applicable(*d, p, io->x_codes != 0) ? route : kRouteNone;
        default: return kRouteNone;
    }
}

// Pointwise on codes in the float32-equivalent (three-pass) mode (slfp_conv2d_fwd_codes_x3): SLFP<3,4> codes in, float32 or codes out.
// A query and an entry point of their own: the older queries keep answering 0 for three-pass descriptors with codes on either side
// of a 1x1 layer, so every link count that rests on them stays.
static bool x3_route(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, int relu, const ConvPlan& p) {
    if (io->x_codes != 1 || (io->y_codes != 0 && io->y_codes != 1) || !code_path_ok(d, relu)) return false;
    if (d->qbits != 8 || d->mfma_passes != SLFP_MFMA_F16X3 || d->groups != 1) return false;
    if (io->y_codes && (!consumer_quant_ok(io) || !enc_table(io->y_ka, y_fmt_of(io->y_qbits), kEncCode)->valid)) return false;
    return pwc_x3_applicable(*d, p, relu, io->y_codes != 0);
}

// slfp_debug_pw_variant: the route the matching forward entry point takes (refused: "none"), then the launcher's own selection.
static const char* pw_variant(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, bool has_res, bool has_res_codes, int64_t y_ld) {
    ConvPlan p;
    if (!d || make_plan(d, &p) != SLFP_OK || p.family != kPointwise) return "none";
    const slfp_conv2d_io f32{0, 0, 1.f, 8};
    if (!io) io = &f32;
    const int y_fmt = y_fmt_of(io->y_qbits);
    if (has_res_codes) {   // slfp_conv2d_fwd_res_codes
        if (!has_res || y_ld || !res_codes_route(d, io, false, 0, p)) return "none";
        return pwc_variant_name(*d, p, false, true, true);
    }
    if (has_res) {         // slfp_conv2d_fwd_res
        if (y_ld || !res_route(d, io, false, 0, p)) return "none";
        return io->x_codes ? pwc_variant_name(*d, p, false, true, false) : pw_variant_name(*d, p, true, false, 1.f, kFmtAct8);
    }
    if (y_ld) {            // slfp_conv2d_fwd_codes_slice
        if (!io->y_codes || !y_ld_ok(d, y_ld) || codes_route(d, io, false, 0, p) != kRoutePwc) return "none";
        return pwc_variant_name(*d, p, true, false, false);
    }
    if (io->x_codes) {     // slfp_conv2d_fwd_codes
        if (codes_route(d, io, false, 0, p) != kRoutePwc) return "none";
        return pwc_variant_name(*d, p, io->y_codes != 0, false, false);
    }
    if (io->y_codes) {     // slfp_conv2d_fwd_entry
        if (!entry_route(d, io, 0, p)) return "none";
        return pw_variant_name(*d, p, false, true, io->y_ka, y_fmt);
    }
    if (p.repad) {         // slfp_conv2d_fwd_post on channel-padded copies: the padded descriptor is what launches
        slfp_conv2d_desc d2;
        padded_desc(*d, &d2);
        return pw_variant_name(d2, p, false, false, 1.f, kFmtAct8);
    }
    return pw_variant_name(*d, p, false, false, 1.f, kFmtAct8);
}

// slfp_debug_dw3x3_instance: the route the matching forward entry point takes (refused: "none"), then the launcher's own selection.
static const char* dw3x3_instance(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, bool has_bias, int post_flags, bool has_post) {
    ConvPlan p;
    if (!d || make_plan(d, &p) != SLFP_OK || p.family != kDw3x3) return "none";
    if ((post_flags & ~(SLFP_POST_RELU | SLFP_POST_LAYEROUT)) != 0) return "none";
    static const float one = 1.f;   // the selections only ask whether a scale / shift pair is present
    const float* vec = has_post ? &one : nullptr;
    if (!io || (!io->x_codes && !io->y_codes)) {   // slfp_conv2d_fwd / slfp_conv2d_fwd_post
        if ((post_flags & SLFP_POST_LAYEROUT) && !has_post) return "none";
        const PostOp post{vec, vec, (post_flags & SLFP_POST_RELU) ? 1 : 0, (post_flags & SLFP_POST_LAYEROUT) ? 1 : 0};
        if (p.repad) {   // on channel-padded copies: the padded descriptor is what launches
            slfp_conv2d_desc d2;
            padded_desc(*d, &d2);
            return dw3x3_instance_name(d2, p, has_bias, post);
        }
        return dw3x3_instance_name(*d, p, has_bias, post);
    }
    const PostOp post{vec, vec, (post_flags & SLFP_POST_RELU) ? 1 : 0, 0};
    CodeIo cio{io->x_codes != 0, io->y_codes != 0, io->y_ka, y_fmt_of(io->y_qbits), 0};
    if (post_flags & SLFP_POST_LAYEROUT) {   // slfp_conv2d_fwd_codes_lut: the layer-output quantizer on codes is the table epilogue
        if (!has_post || (post_flags & SLFP_POST_RELU) || lut_route(d, io, has_bias, p) != kRouteDwc) return "none";
        cio.lut = reinterpret_cast<const uint8_t*>(&one);   // dwc_select only asks whether there is a table
        return dwc_instance_name(*d, p, post, cio);
    }
    if (codes_route(d, io, has_bias, post_flags, p) != kRouteDwc) return "none";   // slfp_conv2d_fwd_codes
    return dwc_instance_name(*d, p, post, cio);
}

// slfp_debug_stem_instance: the route the matching forward entry point takes (refused: "none"), then the launcher's own selection.
static const char* stem_instance(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, bool has_bias, int post_flags, bool has_post) {
    ConvPlan p;
    if (!d || make_plan(d, &p) != SLFP_OK || p.repad) return "none";
    if (p.family != kDirect && p.family != kStemSmall && p.family != kStemMfma) return "none";
    if ((post_flags & ~(SLFP_POST_RELU | SLFP_POST_LAYEROUT)) != 0) return "none";
    static const float one = 1.f;   // the selections only ask whether a scale / shift pair is present
    const float* vec = has_post ? &one : nullptr;
    if (!io || (!io->x_codes && !io->y_codes)) {   // slfp_conv2d_fwd / slfp_conv2d_fwd_post
        if ((post_flags & SLFP_POST_LAYEROUT) && !has_post) return "none";
        const PostOp post{vec, vec, (post_flags & SLFP_POST_RELU) ? 1 : 0, (post_flags & SLFP_POST_LAYEROUT) ? 1 : 0};
        const CodeIo f32{false, false, 1.f, kFmtAct8};
        if (p.family == kStemSmall) return stem_small_instance_name(*d, p, post, f32);
        if (p.family == kStemMfma) return stem_mfma_instance_name(*d, p, post, f32);
        return direct_instance_name(*d, p, post, nullptr);
    }
    if (io->x_codes) return "none";   // the image stems and the direct kernel read float32
    const PostOp post{vec, vec, (post_flags & SLFP_POST_RELU) ? 1 : 0, 0};
    CodeIo cio{false, true, io->y_ka, y_fmt_of(io->y_qbits), 0};
    CodeRoute route;
    if (post_flags & SLFP_POST_LAYEROUT) {   // slfp_conv2d_fwd_codes_lut: the layer-output quantizer in front of codes is the table epilogue
        if (!has_post || (post_flags & SLFP_POST_RELU)) return "none";
        route = lut_route(d, io, has_bias, p);
        cio.lut = reinterpret_cast<const uint8_t*>(&one);   // the selections only ask whether there is a table
    } else {
        route = codes_route(d, io, has_bias, post_flags, p);   // slfp_conv2d_fwd_codes / slfp_conv2d_fwd_codes_ws
    }
    switch (route) {
        case kRouteStemCodes: return direct_instance_name(*d, p, post, &cio);
        case kRouteStemSmall: return stem_small_instance_name(*d, p, post, cio);
        case kRouteStemMfma: return stem_mfma_instance_name(*d, p, post, cio);
        default: return "none";
    }
}

// slfp_debug_layerout_lut_mismatches: every float32 pattern through layerout_bits, its class and back
__global__ __launch_bounds__(256) void k_layerout_lut_check(unsigned long long* __restrict__ out) {
    unsigned long long bad = 0;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < (1ull << 32); i += stride) {
        const uint32_t v = layerout_bits((uint32_t)i);
        const uint32_t c = layerout_class(v);
        const uint32_t w = layerout_value(c);
        const bool vnan = (v & 0x7FFFFFFFu) > 0x7F800000u, wnan = (w & 0x7FFFFFFFu) > 0x7F800000u;   // all NaNs are one class
        if (c >= (uint32_t)kLayeroutClasses || (vnan ? !wnan : w != v)) ++bad;
    }
    if (bad) atomicAdd(out, bad);
}

// ---- the one argument check of the forward entry points ----
struct FwdArgs {   // what a forward entry point was handed; io / res / y_ld / workspace: null or 0 where it has none
    const slfp_conv2d_desc* d; const slfp_conv2d_io* io;
    const void* x; const void* wprep; const float* bias; const float* post_scale; const float* post_shift; int relu;
    void* y; const float* res; int64_t y_ld; void* workspace;
    void* y_codes = nullptr;   // slfp_conv2d_fwd_res_codes: the second, uint8 output
    const uint8_t* lut = nullptr;   // slfp_conv2d_fwd_codes_lut: the byte table of the layer-output classes
};
enum FwdKind { kFwdPost, kFwdCodes, kFwdSlice, kFwdEntry, kFwdRes, kFwdResCodes, kFwdLut, kFwdCodesX3 };
struct Resolved { ConvPlan p; PostOp post; CodeIo cio; CodeRoute route; };

static int need_workspace(const char* fn, const FwdArgs& a, const ConvPlan& p) {
    const size_t ws_need = ws_layout(a.d, p).total;
    if (ws_need && (!a.workspace || !aligned16(a.workspace)))
        return fail(SLFP_ERR_BAD_ARG, "%s: %zu bytes of 16-byte aligned workspace required (slfp_conv2d_workspace_bytes)", fn, ws_need);
    return SLFP_OK;
}

// Checks everything that precedes device work, in the order that decides which status a call with several defects gets, and
// resolves the call ONCE: plan, route, PostOp and CodeIo.  Nothing is launched before this returns SLFP_OK.
static int resolve(FwdKind kind, const char* fn, const FwdArgs& a, Resolved* r) {
    const slfp_conv2d_desc* d = a.d;
    const slfp_conv2d_io* io = a.io;
    if (kind != kFwdPost && (!d || !io)) return fail(SLFP_ERR_BAD_ARG, "%s: null descriptor", fn);
    const int rc = make_plan(d, &r->p);
    if (rc != SLFP_OK) return rc;
    const bool with_res = kind == kFwdRes || kind == kFwdResCodes;
    if (!a.x || !a.wprep || !a.y || (with_res && !a.res) || (kind == kFwdResCodes && !a.y_codes)) return fail(SLFP_ERR_BAD_ARG, "%s: null pointer", fn);
    const bool has_bias = a.bias != nullptr;
    r->route = kRouteNone;
    if (kind == kFwdLut) {   // the table epilogue's own arguments come first
        if (!a.lut || !a.post_scale || !a.post_shift)
            return fail(SLFP_ERR_BAD_ARG, "%s: lut, post_scale and post_shift are required (the table is indexed by the layer-output class of the affine's result)", fn);
        if (!aligned16(a.lut)) return fail(SLFP_ERR_ALIGNMENT, "%s: lut must be 16-byte aligned", fn);
        if (io->y_codes != 1) return fail(SLFP_ERR_BAD_ARG, "%s: the table epilogue writes codes (io->y_codes == 1)", fn);
        if (!consumer_quant_ok(io))
            return fail(SLFP_ERR_BAD_ARG, "%s: io->y_qbits must be 8 or 7 (got %d) and io->y_ka a positive scale within [1e-30, 1e30]", fn, io->y_qbits);
        if (a.y_ld != d->c_out && !y_ld_ok(d, a.y_ld))
            return fail(SLFP_ERR_BAD_ARG, "%s: y_ld = %lld must be C_out = %lld or a multiple of 16 above it", fn, (long long)a.y_ld, (long long)d->c_out);
        r->route = lut_route(d, io, has_bias, r->p);
        if (r->route == kRouteNone || (a.y_ld != d->c_out && !slice_route(r->route)))
            return fail(SLFP_ERR_UNSUPPORTED, "%s: this layer / io combination has no table-epilogue kernel (slfp_conv2d_codes_lut_supported)", fn);
    }
    if (kind == kFwdSlice) {   // the slice's own arguments come first
        if (!io->y_codes) return fail(SLFP_ERR_BAD_ARG, "%s: a channel slice is written as codes (io->y_codes == 1)", fn);
        if (!aligned16(a.y)) return fail(SLFP_ERR_ALIGNMENT, "%s: y (the slice's first channel) must be 16-byte aligned", fn);
        if (!y_ld_ok(d, a.y_ld))
            return fail(SLFP_ERR_BAD_ARG, "%s: y_ld = %lld must be a multiple of 16, >= C_out = %lld", fn, (long long)a.y_ld, (long long)d->c_out);
        r->route = codes_route(d, io, has_bias, a.relu, r->p);
        if (!slice_route(r->route))
            return fail(SLFP_ERR_UNSUPPORTED, "%s: this layer / io combination has no code kernel with a channel-slice store "
                                              "(slfp_conv2d_codes_slice_supported)", fn);
    }
    if ((a.post_scale == nullptr) != (a.post_shift == nullptr))
        return fail(SLFP_ERR_BAD_ARG, "%s: post_scale and post_shift must be given together", fn);
    if (a.post_scale && (!aligned16(a.post_scale) || !aligned16(a.post_shift)))
        return fail(SLFP_ERR_ALIGNMENT, "%s: post_scale / post_shift must be 16-byte aligned", fn);
    if (kind == kFwdPost) {   // on the code paths these two are a refusal of the route
        if ((a.relu & ~(SLFP_POST_RELU | SLFP_POST_LAYEROUT)) != 0) return fail(SLFP_ERR_BAD_ARG, "%s: unknown flag bits in `relu`", fn);
        if ((a.relu & SLFP_POST_LAYEROUT) && !a.post_scale)
            return fail(SLFP_ERR_BAD_ARG, "%s: SLFP_POST_LAYEROUT needs post_scale / post_shift", fn);
    }
    if (!aligned16(a.x) || !aligned16(a.y) || !aligned16(a.wprep) || !aligned16(a.bias) || !aligned16(a.res))
        return fail(SLFP_ERR_ALIGNMENT, "%s: x, y, wprep, bias and res must be 16-byte aligned", fn);
    if (!aligned16(a.y_codes)) return fail(SLFP_ERR_ALIGNMENT, "%s: y_codes must be 16-byte aligned", fn);
    r->post = PostOp{a.post_scale, a.post_shift, (a.relu & SLFP_POST_RELU) ? 1 : 0, (kind == kFwdPost && (a.relu & SLFP_POST_LAYEROUT)) ? 1 : 0};
    if (kind == kFwdPost) return need_workspace(fn, a, r->p);
    r->cio = CodeIo{io->x_codes != 0, io->y_codes != 0, io->y_ka, y_fmt_of(io->y_qbits), a.y_ld};
    if (kind == kFwdLut) {
        r->cio.lut = a.lut;
        if (a.y_ld == d->c_out) r->cio.y_ld = 0;   // a dense tensor
        return r->route == kRouteDense ? need_workspace(fn, a, r->p) : SLFP_OK;
    }
    if (kind == kFwdEntry) {
        if (io->x_codes != 0 || io->y_codes != 1)
            return fail(SLFP_ERR_BAD_ARG, "%s: reads float32 and writes codes (io->x_codes == 0, io->y_codes == 1; "
                                          "slfp_conv2d_entry_supported)", fn);
        if (!consumer_quant_ok(io))
            return fail(SLFP_ERR_BAD_ARG, "%s: io->y_qbits must be 8 or 7 (got %d) and io->y_ka a positive scale within [1e-30, 1e30] "
                                          "(slfp_conv2d_entry_supported)", fn, io->y_qbits);
        if (!entry_route(d, io, a.relu, r->p))
            return fail(SLFP_ERR_UNSUPPORTED, "%s: this layer / io combination has no float32 -> codes kernel "
                                              "(slfp_conv2d_entry_supported); use slfp_conv2d_fwd_post and slfp_encode_f32", fn);
        return SLFP_OK;
    }
    if (kind == kFwdCodesX3) {
        if (!x3_route(d, io, a.relu, r->p))
            return fail(SLFP_ERR_UNSUPPORTED, "%s: this layer / io combination has no three-pass pointwise kernel on codes "
                                              "(slfp_conv2d_codes_x3_supported); use slfp_conv2d_fwd_post", fn);
        return SLFP_OK;
    }
    if (with_res) {   // res is read while y is written, in a different order by different workgroups: the two must not overlap
        const uintptr_t nbytes = (uintptr_t)d->n * (uintptr_t)d->c_out * (uintptr_t)r->p.h_out * (uintptr_t)r->p.w_out * sizeof(float);
        const uintptr_t ra = reinterpret_cast<uintptr_t>(a.res), ya = reinterpret_cast<uintptr_t>(a.y);
        if (ra < ya + nbytes && ya < ra + nbytes) return fail(SLFP_ERR_BAD_ARG, "%s: res and y overlap", fn);
        if (kind == kFwdResCodes) {   // nor may the code tensor (1 B per element) lie in either of them
            const uintptr_t ca = reinterpret_cast<uintptr_t>(a.y_codes), cbytes = nbytes / sizeof(float);
            if ((ca < ya + nbytes && ya < ca + cbytes) || (ca < ra + nbytes && ra < ca + cbytes))
                return fail(SLFP_ERR_BAD_ARG, "%s: y_codes overlaps y or res", fn);
            if (!res_codes_route(d, io, has_bias, a.relu, r->p))
                return fail(SLFP_ERR_UNSUPPORTED, "%s: this layer / io combination has no residual kernel that also writes codes "
                                                  "(slfp_conv2d_res_codes_supported); use slfp_conv2d_fwd_res and slfp_encode_f32", fn);
            return SLFP_OK;
        }
        if (!res_route(d, io, has_bias, a.relu, r->p))
            return fail(SLFP_ERR_UNSUPPORTED, "%s: this layer / io combination has no residual kernel "
                                              "(slfp_conv2d_res_supported); use slfp_conv2d_fwd_post and add the residual afterwards", fn);
        return SLFP_OK;
    }
    if (kind == kFwdCodes) r->route = codes_route(d, io, has_bias, a.relu, r->p);
    if (r->route == kRouteNone)
        return fail(SLFP_ERR_UNSUPPORTED, "%s: this layer / io combination has no code-path kernel "
                                          "(slfp_conv2d_codes_supported); use slfp_conv2d_fwd_post", fn);
    if (r->route == kRouteStemMfma && !stem_mfma_uses_workspace(*d, true)) return SLFP_OK;   // k_stem_rows: everything in LDS
    return r->route == kRouteDense || r->route == kRouteStemMfma ? need_workspace(fn, a, r->p) : SLFP_OK;
}

// slfp_conv2d_fwd_codes[_ws] and slfp_conv2d_fwd_codes_slice once resolved.
static int launch_codes(const FwdArgs& a, const Resolved& r, hipStream_t st) {
    const slfp_conv2d_desc& d = *a.d;
    const float* xf = reinterpret_cast<const float*>(a.x);
    const uint8_t* xc = reinterpret_cast<const uint8_t*>(a.x);
    switch (r.route) {
        case kRouteDwc: return launch_dwc(d, r.p, xc, reinterpret_cast<const float*>(a.wprep), r.post, a.y, r.cio, st);
        case kRoutePwc: return launch_pwc(d, r.p, xc, a.wprep, a.bias, r.post, a.y, r.cio, st);
        case kRouteDense: return launch_dense_mfma_io(d, r.p, a.x, a.wprep, a.bias, r.post, a.y, a.workspace, r.cio, st);
        case kRouteStemSmall: return launch_stem_small_io(d, r.p, xf, a.wprep, a.bias, r.post, a.y, r.cio, st);
        case kRouteStemMfma: return launch_stem_mfma_io(d, r.p, xf, a.wprep, a.bias, r.post, a.y, a.workspace, r.cio, st);
        default: return launch_stem_codes(d, r.p, xf, reinterpret_cast<const float*>(a.wprep), a.bias, r.post, a.y, r.cio, st);
    }
}

extern "C" {

int slfp_conv2d_fwd(const slfp_conv2d_desc* d, const float* x, const void* wprep, const float* bias, float* y,
                    float* input_q, void* workspace, void* stream) {
    return slfp_conv2d_fwd_post(d, x, wprep, bias, nullptr, nullptr, 0, y, input_q, workspace, stream);
}

int slfp_conv2d_fwd_post(const slfp_conv2d_desc* d, const float* x, const void* wprep, const float* bias,
                         const float* post_scale, const float* post_shift, int relu, float* y, float* input_q,
                         void* workspace, void* stream) {
    const FwdArgs a{d, nullptr, x, wprep, bias, post_scale, post_shift, relu, y, nullptr, 0, workspace};
    Resolved r;
    int rc = resolve(kFwdPost, "slfp_conv2d_fwd_post", a, &r);
    if (rc != SLFP_OK) return rc;
    const ConvPlan& p = r.p;
    const PostOp& post = r.post;
    hipStream_t st = as_stream(stream);
    if (input_q) {  // the reference's self.input_q (utils/conv2d_func.py:21), in x's layout
        rc = launch_quantize(x, input_q, (size_t)d->n * d->c_in * d->h * d->w, d->ka, p.fmt_act, st);
        if (rc != SLFP_OK) return rc;
    }
    const WsLayout l = ws_layout(d, p);
    unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
    const float* x_nhwc = x;
    float* y_nhwc = y;
    if (d->x_layout == SLFP_LAYOUT_NCHW) {
        float* t = reinterpret_cast<float*>(ws + l.x_nhwc);
        rc = slfp_nchw_to_nhwc_f32(x, t, d->n, d->c_in, d->h, d->w, stream);
        if (rc != SLFP_OK) return rc;
        x_nhwc = t;
    }
    if (d->y_layout == SLFP_LAYOUT_NCHW) y_nhwc = reinterpret_cast<float*>(ws + l.y_nhwc);
    if (p.repad) {
        slfp_conv2d_desc d2;
        padded_desc(*d, &d2);
        const float* xin = x_nhwc;
        float* yout = y_nhwc;
        if (p.cpi != d->c_in) {
            float* xp = reinterpret_cast<float*>(ws + l.x_pad);
            rc = launch_repad(x_nhwc, xp, d->n * d->h * d->w, d->c_in, p.cpi, st);
            if (rc != SLFP_OK) return rc;
            xin = xp;
        }
        if (p.cpo != d->c_out) yout = reinterpret_cast<float*>(ws + l.y_pad);
        const float* vec[3] = {bias, post_scale, post_shift};  // per-channel vectors are read 16 bytes at a time
        for (int i = 0; i < 3; ++i) {
            if (!vec[i] || p.cpo == d->c_out) continue;
            float* vp = reinterpret_cast<float*>(ws + l.vec[i]);
            rc = launch_repad(vec[i], vp, 1, d->c_out, p.cpo, st);
            if (rc != SLFP_OK) return rc;
            vec[i] = vp;
        }
        const PostOp post2{vec[1], vec[2], post.relu, post.layerout};
        if (p.family == kDw3x3) rc = launch_dw3x3(d2, p, xin, reinterpret_cast<const float*>(wprep), vec[0], post2, yout, st);
        else rc = launch_pointwise(d2, p, xin, wprep, vec[0], post2, yout, st);
        if (rc != SLFP_OK) return rc;
        if (p.cpo != d->c_out) rc = launch_repad(yout, y_nhwc, d->n * p.h_out * p.w_out, p.cpo, d->c_out, st);
    } else {
        switch (p.family) {
            case kDw3x3: rc = launch_dw3x3(*d, p, x_nhwc, reinterpret_cast<const float*>(wprep), bias, post, y_nhwc, st); break;
            case kPointwise: rc = launch_pointwise(*d, p, x_nhwc, wprep, bias, post, y_nhwc, st); break;
            case kDenseMfma: rc = launch_dense_mfma(*d, p, x_nhwc, wprep, bias, post, y_nhwc, ws + l.operand, st); break;
            case kStemMfma: rc = launch_stem_mfma(*d, p, x_nhwc, wprep, bias, post, y_nhwc, ws + l.operand, st); break;
            case kStemSmall: rc = launch_stem_small(*d, p, x_nhwc, wprep, bias, post, y_nhwc, st); break;
            default: rc = launch_direct(*d, p, x_nhwc, reinterpret_cast<const float*>(wprep), bias, post, y_nhwc, st); break;
        }
    }
    if (rc != SLFP_OK) return rc;
    if (d->y_layout == SLFP_LAYOUT_NCHW) rc = slfp_nhwc_to_nchw_f32(y_nhwc, y, d->n, d->c_out, p.h_out, p.w_out, stream);
    return rc;
}

// ---- the table epilogue: codes behind the layer-output quantizer (csrc/slfp_layerout_lut.hpp) ----
int slfp_layerout_lut_classes(void) { return kLayeroutClasses; }

int slfp_layerout_lut_values(float* out, int n) {
    if (!out || n < 0) return fail(SLFP_ERR_BAD_ARG, "slfp_layerout_lut_values: bad argument");
    for (int i = 0; i < n; ++i) {
        const uint32_t v = layerout_value((uint32_t)i);
        memcpy(out + i, &v, 4);
    }
    return SLFP_OK;
}

int slfp_layerout_lut_index(float v) {
    uint32_t b;
    memcpy(&b, &v, 4);
    const uint32_t i = layerout_class(b);
    if (i == 0u) return (b & 0x7FFFFFFFu) > 0x7F800000u ? 0 : -1;
    return (i < (uint32_t)kLayeroutClasses && layerout_value(i) == b) ? (int)i : -1;   // -1: not a value of the quantizer
}

int slfp_debug_layerout_lut_mismatches(unsigned long long* out1, void* stream) {
    if (!out1) return fail(SLFP_ERR_BAD_ARG, "slfp_debug_layerout_lut_mismatches: null pointer");
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(out1, 0, sizeof(unsigned long long), st) != hipSuccess) return check_launch("hipMemsetAsync");
    hipLaunchKernelGGL(k_layerout_lut_check, dim3(256 * 16), dim3(256), 0, st, out1);
    return check_launch("slfp layer-output class self-check kernel");
}

int slfp_conv2d_codes_lut_supported(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, int has_bias, int64_t y_ld) {
    ConvPlan p;
    if (!d || !io || make_plan(d, &p) != SLFP_OK) return 0;
    const CodeRoute route = lut_route(d, io, has_bias != 0, p);
    if (route == kRouteNone) return 0;
    return y_ld == d->c_out || (slice_route(route) && y_ld_ok(d, y_ld));
}

int slfp_conv2d_fwd_codes_lut(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, const void* x, const void* wprep,
                              const float* bias, const float* post_scale, const float* post_shift, const uint8_t* lut, void* y,
                              int64_t y_ld, void* workspace, void* stream) {
    FwdArgs a{d, io, x, wprep, bias, post_scale, post_shift, 0, y, nullptr, y_ld, workspace};
    a.lut = lut;
    Resolved r;
    const int rc = resolve(kFwdLut, "slfp_conv2d_fwd_codes_lut", a, &r);
    return rc != SLFP_OK ? rc : launch_codes(a, r, as_stream(stream));
}

// The four queries: the route functions behind a null check and make_plan.
int slfp_conv2d_codes_supported(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, int has_bias, int relu) {
    ConvPlan p;
    return d && io && make_plan(d, &p) == SLFP_OK && codes_route(d, io, has_bias != 0, relu, p) != kRouteNone;
}

int slfp_conv2d_codes_slice_supported(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, int has_bias, int relu, int64_t y_ld) {
    ConvPlan p;
    return d && io && io->y_codes && make_plan(d, &p) == SLFP_OK && slice_route(codes_route(d, io, has_bias != 0, relu, p)) && y_ld_ok(d, y_ld);
}

int slfp_conv2d_entry_supported(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, int has_bias, int relu) {
    (void)has_bias;   // both kernels take a bias
    ConvPlan p;
    return d && io && make_plan(d, &p) == SLFP_OK && entry_route(d, io, relu, p);
}

int slfp_conv2d_res_supported(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, int has_bias, int relu) {
    ConvPlan p;
    return d && io && make_plan(d, &p) == SLFP_OK && res_route(d, io, has_bias != 0, relu, p);
}

int slfp_conv2d_res_codes_supported(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, int has_bias, int relu) {
    ConvPlan p;
    return d && io && make_plan(d, &p) == SLFP_OK && res_codes_route(d, io, has_bias != 0, relu, p);
}

int slfp_conv2d_codes_x3_supported(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, int has_bias, int relu) {
    (void)has_bias;   // both kernels take a bias
    ConvPlan p;
    return d && io && make_plan(d, &p) == SLFP_OK && x3_route(d, io, relu, p);
}

int slfp_conv2d_fwd_codes_x3(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, const void* x, const void* wprep,
                             const float* bias, const float* post_scale, const float* post_shift, int relu, void* y, void* stream) {
    const FwdArgs a{d, io, x, wprep, bias, post_scale, post_shift, relu, y, nullptr, 0, nullptr};
    Resolved r;
    const int rc = resolve(kFwdCodesX3, "slfp_conv2d_fwd_codes_x3", a, &r);
    return rc != SLFP_OK ? rc : launch_pwc_x3(*d, r.p, reinterpret_cast<const uint8_t*>(x), wprep, bias, r.post, y, r.cio, as_stream(stream));
}

const char* slfp_debug_pwc_x3_variant(const slfp_conv2d_desc* d, const slfp_conv2d_io* io) {
    ConvPlan p;
    if (!d || !io || make_plan(d, &p) != SLFP_OK || !x3_route(d, io, 0, p)) return "none";
    return pwc_x3_variant_name(*d, p, io->y_codes != 0);
}

int slfp_conv2d_fwd_codes(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, const void* x, const void* wprep,
                          const float* bias, const float* post_scale, const float* post_shift, int relu, void* y, void* stream) {
    return slfp_conv2d_fwd_codes_ws(d, io, x, wprep, bias, post_scale, post_shift, relu, y, nullptr, stream);
}

int slfp_conv2d_fwd_codes_ws(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, const void* x, const void* wprep,
                             const float* bias, const float* post_scale, const float* post_shift, int relu, void* y,
                             void* workspace, void* stream) {
    const FwdArgs a{d, io, x, wprep, bias, post_scale, post_shift, relu, y, nullptr, 0, workspace};
    Resolved r;
    const int rc = resolve(kFwdCodes, "slfp_conv2d_fwd_codes_ws", a, &r);
    return rc != SLFP_OK ? rc : launch_codes(a, r, as_stream(stream));
}

// y_ld: the channel count of the wider NHWC code tensor that y is a channel slice of
int slfp_conv2d_fwd_codes_slice(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, const void* x, const void* wprep,
                                const float* bias, const float* post_scale, const float* post_shift, int relu, void* y,
                                int64_t y_ld, void* workspace, void* stream) {
    const FwdArgs a{d, io, x, wprep, bias, post_scale, post_shift, relu, y, nullptr, y_ld, workspace};
    Resolved r;
    const int rc = resolve(kFwdSlice, "slfp_conv2d_fwd_codes_slice", a, &r);
    return rc != SLFP_OK ? rc : launch_codes(a, r, as_stream(stream));
}

int slfp_conv2d_fwd_entry(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, const float* x, const void* wprep,
                          const float* bias, const float* post_scale, const float* post_shift, int relu, void* y_codes, void* stream) {
    const FwdArgs a{d, io, x, wprep, bias, post_scale, post_shift, relu, y_codes, nullptr, 0, nullptr};
    Resolved r;
    const int rc = resolve(kFwdEntry, "slfp_conv2d_fwd_entry", a, &r);
    return rc != SLFP_OK ? rc : launch_pointwise_entry(*d, r.p, x, wprep, bias, r.post, y_codes, r.cio, as_stream(stream));
}

int slfp_conv2d_fwd_res(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, const void* x, const void* wprep,
                        const float* bias, const float* post_scale, const float* post_shift, int relu,
                        const float* res, float* y, void* workspace, void* stream) {
    (void)workspace;
    const FwdArgs a{d, io, x, wprep, bias, post_scale, post_shift, relu, y, res, 0, nullptr};
    Resolved r;
    const int rc = resolve(kFwdRes, "slfp_conv2d_fwd_res", a, &r);
    if (rc != SLFP_OK) return rc;
    hipStream_t st = as_stream(stream);
    if (!io->x_codes) return launch_pointwise(*d, r.p, reinterpret_cast<const float*>(x), wprep, bias, r.post, y, st, res);
    const CodeIo codes_in{true, false, 1.f, kFmtAct8};
    return launch_pwc(*d, r.p, reinterpret_cast<const uint8_t*>(x), wprep, bias, r.post, y, codes_in, st, res);
}

int slfp_conv2d_fwd_res_codes(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, const void* x, const void* wprep,
                              const float* bias, const float* post_scale, const float* post_shift, int relu,
                              const float* res, float* y, void* y_codes, void* workspace, void* stream) {
    (void)workspace;
    const FwdArgs a{d, io, x, wprep, bias, post_scale, post_shift, relu, y, res, 0, nullptr, y_codes};
    Resolved r;
    const int rc = resolve(kFwdResCodes, "slfp_conv2d_fwd_res_codes", a, &r);
    if (rc != SLFP_OK) return rc;
    // float32 out as slfp_conv2d_fwd_res launches it; y_ka / y_fmt describe the reader of y_codes
    const CodeIo codes_in{true, false, io->y_ka, y_fmt_of(io->y_qbits)};
    return launch_pwc(*d, r.p, reinterpret_cast<const uint8_t*>(x), wprep, bias, r.post, y, codes_in, as_stream(stream), res, y_codes);
}

}  // extern "C"

// ---- image stems on uint8 pixels + a float32 pixel table (include/slfp.h: slfp_conv2d_fwd_u8) ----
enum U8Route { kU8None = 0, kU8Fixed, kU8Small, kU8Mfma };

// One selection behind the query, the entry point and the reporter.  cio: the code interface's arguments of the launch.
static U8Route u8_route(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, int post_flags, const ConvPlan& p, CodeIo* cio) {
    if (io && (io->x_codes != 0 || (io->y_codes != 0 && io->y_codes != 1))) return kU8None;
    const bool yc = io && io->y_codes == 1;
    if (d->x_layout != SLFP_LAYOUT_NHWC || d->y_layout != SLFP_LAYOUT_NHWC || d->groups != 1 || d->c_in > 4 || p.repad) return kU8None;
    if ((post_flags & ~(SLFP_POST_RELU | SLFP_POST_LAYEROUT)) != 0) return kU8None;
    if (d->qbits == 8 && d->mfma_passes == SLFP_MFMA_F16X3) return kU8None;
    *cio = CodeIo{false, yc, yc ? io->y_ka : 1.f, yc ? y_fmt_of(io->y_qbits) : (int)kFmtAct8};
    if (yc) {   // the reader's quantizer as slfp_conv2d_fwd_codes validates it; the layer-output quantizer has no code form here
        if (!code_path_ok(d, post_flags) || !consumer_quant_ok(io) || !enc_table(io->y_ka, cio->y_fmt, kEncCode)->valid) return kU8None;
    }
    const PostOp post{nullptr, nullptr, (post_flags & SLFP_POST_RELU) ? 1 : 0, 0};   // the selections read the ReLU bit only
    switch (p.family) {
        case kDirect: return stem_u8_applicable(*d, p, post, yc ? cio : nullptr) ? kU8Fixed : kU8None;
        case kStemSmall: return !yc || stem_small_codes_applicable(*d, p, post_flags) ? kU8Small : kU8None;
        case kStemMfma: return !yc || stem_mfma_codes_applicable(*d, p, post_flags) ? kU8Mfma : kU8None;
        default: return kU8None;
    }
}

// y[e] = pix[(e % C)][x[e]] over n_el = n_pixels * C elements, four per lane (one 16-byte store); the table in LDS.
__global__ __launch_bounds__(256) void k_image_u8_expand(const uint8_t* __restrict__ x, const float* __restrict__ pix, float* __restrict__ y,
                                                         int64_t n_el, int C) {
    __shared__ float sP[256 * 4];
    for (int i = threadIdx.x; i < 256 * C; i += 256) sP[i] = pix[i];
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * 256 * 4;
    for (int64_t e = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; e < n_el; e += stride) {
        int c = (int)(e % C);
        if (e + 4 <= n_el) {
            float r[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                r[k] = sP[c * 256 + x[e + k]];
                c = c + 1 == C ? 0 : c + 1;
            }
            *reinterpret_cast<float4*>(y + e) = make_float4(r[0], r[1], r[2], r[3]);
        } else {
            for (int64_t k = e; k < n_el; ++k) {
                y[k] = sP[c * 256 + x[k]];
                c = c + 1 == C ? 0 : c + 1;
            }
        }
    }
}

extern "C" {

int slfp_conv2d_u8_supported(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, int has_bias, int post_flags) {
    (void)has_bias;   // every stem kernel takes a bias
    ConvPlan p;
    CodeIo cio;
    return d && make_plan(d, &p) == SLFP_OK && u8_route(d, io, post_flags, p, &cio) != kU8None;
}

const char* slfp_debug_stem_u8_instance(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, int has_bias, int post_flags, int has_post) {
    (void)has_bias;
    ConvPlan p;
    CodeIo cio{false, false, 1.f, kFmtAct8};
    if (!d || make_plan(d, &p) != SLFP_OK) return "none";
    if ((post_flags & SLFP_POST_LAYEROUT) && !has_post) return "none";
    const U8Route route = u8_route(d, io, post_flags, p, &cio);
    static const float one = 1.f;   // the selections only ask whether a scale / shift pair is present
    const float* vec = has_post ? &one : nullptr;
    const PostOp post{vec, vec, (post_flags & SLFP_POST_RELU) ? 1 : 0, (!cio.y_codes && (post_flags & SLFP_POST_LAYEROUT)) ? 1 : 0};
    switch (route) {
        case kU8Fixed: return direct_instance_name(*d, p, post, cio.y_codes ? &cio : nullptr, true);
        case kU8Small: return stem_small_instance_name(*d, p, post, cio, true);
        case kU8Mfma: return stem_mfma_instance_name(*d, p, post, cio, true);
        default: return "none";
    }
}

int slfp_conv2d_fwd_u8(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, const uint8_t* x, const float* pix_table,
                       const void* wprep, const float* bias, const float* post_scale, const float* post_shift,
                       int post_flags, void* y, void* workspace, void* stream) {
    const char* fn = "slfp_conv2d_fwd_u8";
    if (!d) return fail(SLFP_ERR_BAD_ARG, "%s: null descriptor", fn);
    ConvPlan p;
    const int rc = make_plan(d, &p);
    if (rc != SLFP_OK) return rc;
    if (!x || !pix_table || !wprep || !y) return fail(SLFP_ERR_BAD_ARG, "%s: null pointer", fn);
    if ((post_scale == nullptr) != (post_shift == nullptr))
        return fail(SLFP_ERR_BAD_ARG, "%s: post_scale and post_shift must be given together", fn);
    CodeIo cio;
    const U8Route route = u8_route(d, io, post_flags, p, &cio);
    if (route == kU8None)
        return fail(SLFP_ERR_UNSUPPORTED, "%s: this layer / io combination has no byte-input stem kernel (slfp_conv2d_u8_supported); "
                                          "use slfp_image_u8_expand_f32 and the float32 entry point", fn);
    if ((post_flags & SLFP_POST_LAYEROUT) && !post_scale) return fail(SLFP_ERR_BAD_ARG, "%s: SLFP_POST_LAYEROUT needs post_scale / post_shift", fn);
    if (!aligned16(pix_table) || !aligned16(y) || !aligned16(wprep) || !aligned16(bias) || !aligned16(post_scale) || !aligned16(post_shift))
        return fail(SLFP_ERR_ALIGNMENT, "%s: pix_table, y, wprep, bias, post_scale and post_shift must be 16-byte aligned (x: any alignment)", fn);
    const bool needs_ws = route == kU8Mfma && stem_mfma_uses_workspace(*d, cio.y_codes, true);
    if (needs_ws && (!workspace || !aligned16(workspace)))
        return fail(SLFP_ERR_BAD_ARG, "%s: %zu bytes of 16-byte aligned workspace required (slfp_conv2d_workspace_bytes)", fn, ws_layout(d, p).total);
    const PostOp post{post_scale, post_shift, (post_flags & SLFP_POST_RELU) ? 1 : 0, (post_flags & SLFP_POST_LAYEROUT) ? 1 : 0};
    hipStream_t st = as_stream(stream);
    const float* xf = reinterpret_cast<const float*>(x);   // the U8 forms read it as bytes
    unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
    switch (route) {
        case kU8Fixed: return launch_stem_u8(*d, p, x, pix_table, reinterpret_cast<const float*>(wprep), bias, post, y, cio.y_codes ? &cio : nullptr, st);
        case kU8Small: return launch_stem_small_io(*d, p, xf, wprep, bias, post, y, cio, st, pix_table);
        default: return launch_stem_mfma_io(*d, p, xf, wprep, bias, post, y, needs_ws ? ws + ws_layout(d, p).operand : nullptr, cio, st, pix_table);
    }
}

int slfp_image_u8_expand_f32(const uint8_t* x, const float* pix_table, float* y, int64_t n_pixels, int c, void* stream) {
    if (!x || !pix_table || !y) return fail(SLFP_ERR_BAD_ARG, "slfp_image_u8_expand_f32: null pointer");
    if (c < 1 || c > 4 || n_pixels < 0) return fail(SLFP_ERR_SHAPE, "slfp_image_u8_expand_f32: 1 <= c <= 4 and n_pixels >= 0 required");
    if (!aligned16(pix_table) || !aligned16(y)) return fail(SLFP_ERR_ALIGNMENT, "slfp_image_u8_expand_f32: pix_table and y must be 16-byte aligned");
    if (n_pixels == 0) return SLFP_OK;
    const int64_t n_el = n_pixels * c;
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(n_el, 256 * 4), 4096);
    hipLaunchKernelGGL(k_image_u8_expand, dim3(grid), dim3(256), 0, as_stream(stream), x, pix_table, y, n_el, c);
    return check_launch("slfp image byte expansion kernel");
}

}  // extern "C"

extern "C" {

static void linear_desc(slfp_conv2d_desc* d, int64_t batch, int64_t in_f, int64_t out_f, float ka, float kw_scale,
                        int qbits, int mfma_passes) {
    // Linear_Q.forward (utils/conv2d_func.py:60-65) = a 1x1 convolution over `batch` pixels,
    // except that the reference divides the bias by Kw first and rescales by Kw first.
    memset(d, 0, sizeof(*d));
    d->n = batch; d->c_in = in_f; d->h = 1; d->w = 1; d->c_out = out_f; d->kh = 1; d->kw = 1;
    d->stride_h = d->stride_w = d->dil_h = d->dil_w = d->groups = 1;
    d->x_layout = d->y_layout = SLFP_LAYOUT_NHWC; d->qbits = qbits; d->ka = ka; d->kw_scale = kw_scale;
    d->mfma_passes = mfma_passes;
}

size_t slfp_linear_workspace_bytes(int64_t batch, int64_t in_f, int64_t out_f) {
    slfp_conv2d_desc d;
    linear_desc(&d, batch, in_f, out_f, 1.f, 1.f, 8, SLFP_MFMA_DEFAULT);
    ConvPlan p;
    if (make_plan_core(&d, &p) != SLFP_OK) return 0;  // the plan slfp_linear_fwd uses (no channel re-padding)
    return p.wprep_bytes;
}

int slfp_linear_prepare_weights(const float* w, void* wprep, int64_t in_f, int64_t out_f, float kw_scale, int qbits,
                                int mfma_passes, void* stream) {
    slfp_conv2d_desc d;
    linear_desc(&d, 1, in_f, out_f, 1.0f, kw_scale, qbits, mfma_passes);
    ConvPlan p;
    const int rc = make_plan_core(&d, &p);  // no channel re-padding here: odd feature counts take the direct kernel
    if (rc != SLFP_OK) return rc;
    if (!w || !wprep) return fail(SLFP_ERR_BAD_ARG, "slfp_linear_prepare_weights: null pointer");
    if (!aligned16(wprep)) return fail(SLFP_ERR_ALIGNMENT, "slfp_linear_prepare_weights: wprep must be 16-byte aligned");
    return launch_prepare_weights(d, p, w, wprep, nullptr, as_stream(stream));
}

int slfp_linear_fwd_prepared(const float* x, const void* wprep, const float* bias, float* y, int64_t batch, int64_t in_f,
                             int64_t out_f, float ka, float kw_scale, int qbits, int mfma_passes, void* stream) {
    slfp_conv2d_desc d;
    linear_desc(&d, batch, in_f, out_f, ka, kw_scale, qbits, mfma_passes);
    ConvPlan p;
    const int rc = make_plan_core(&d, &p);
    if (rc != SLFP_OK) return rc;
    if (!x || !wprep || !y) return fail(SLFP_ERR_BAD_ARG, "slfp_linear_fwd: null pointer");
    if (!aligned16(x) || !aligned16(y) || !aligned16(wprep) || (bias && !aligned16(bias)))
        return fail(SLFP_ERR_ALIGNMENT, "slfp_linear_fwd: pointers must be 16-byte aligned");
    p.s1 = kw_scale;
    p.s2 = ka;
    const PostOp none{nullptr, nullptr, 0, 0};
    hipStream_t st = as_stream(stream);
    if (p.family == kPointwise) return launch_pointwise(d, p, x, wprep, bias, none, y, st);
    return launch_direct(d, p, x, reinterpret_cast<const float*>(wprep), bias, none, y, st);
}

int slfp_linear_fwd(const float* x, const float* w, const float* bias, float* y, int64_t batch, int64_t in_f,
                    int64_t out_f, float ka, float kw_scale, int qbits, int mfma_passes, void* workspace,
                    void* stream) {
    if (!workspace) return fail(SLFP_ERR_BAD_ARG, "slfp_linear_fwd: null pointer");
    // the reference re-quantizes the weights on every call; so does this entry point
    const int rc = slfp_linear_prepare_weights(w, workspace, in_f, out_f, kw_scale, qbits, mfma_passes, stream);
    if (rc != SLFP_OK) return rc;
    return slfp_linear_fwd_prepared(x, workspace, bias, y, batch, in_f, out_f, ka, kw_scale, qbits, mfma_passes, stream);
}

}  // extern "C"
