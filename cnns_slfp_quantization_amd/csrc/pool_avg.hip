// pool_avg.hip -- the global average pool between the last convolution and the classifier (gfx950, wave64).
//
//   y[n, c] = mean over the H*W pixels of x[n, :, :, c]        float32 x, NHWC or NCHW
//
// nn.AdaptiveAvgPool2d((1, 1)) (nets_imgnet/resnet50.py:146, nets_imgnet/squeezenet1_0.py:85), nn.AdaptiveAvgPool2d(1)
// (nets_cifar/mobilenetv1.py:62) and nn.AvgPool2d(7) on a 7 x 7 map (nets_imgnet/mobilenetv1.py:58).  The summation order is part
// of the contract (include/slfp.h), so that a row of y is a pure function of one image's values -- whatever the batch, the grid
// or the layout:
//   p = h W + w,  v_p = relu ? max(x_p, 0) : x_p
//   s_j = sum of v_p over p == j (mod 4), p ascending, from +0.0f      (j = 0..3)
//   y   = ((s_0 + s_1) + (s_2 + s_3)) / (float)(H W)                   IEEE division
// Four independent add chains per channel; the library is built with -ffp-contract=off and without fast-math, so the compiler
// neither reassociates them nor turns the division into a multiply.
//   NHWC  k_gap_nhwc: a workgroup is 4 waves; wave j owns partial j of 64 (image, 4-channel group) pairs, one pair per lane: one
//         16-byte load per pixel, coalesced across the lanes, four loads issued ahead of their adds.  The four partials meet in
//         LDS and wave 0 pairs, divides and stores.  N = 256, C = 1024: 16 waves per CU with 64 KiB of loads in flight.
//   NCHW  k_gap_nchw: four neighbouring lanes own one (image, channel) plane, lane j its partial j: the quad reads 16 consecutive
//         bytes of the plane per step; the partials meet through two lane exchanges ((s_0 + s_1) and (s_2 + s_3) first: float
//         addition commutes, so every lane of the quad ends with the same bits).  Any C, 4-byte loads.
// Output: float32 [N, C], or the reader Linear_Q's codes (signed classes: no ReLU stands behind the pool) through code4 of
// slfp_epilogue.hpp, 4 channels = one dword.  No atomics, nothing of N or the grid in the arithmetic.
#include "slfp_device.hpp"
#include "slfp_enc.hpp"
#include "slfp_codes.hpp"
#include "slfp_epilogue.hpp"
#include "slfp_host.hpp"
#include "conv_pw_params.hpp"

namespace slfp {

struct GapParams {
    const float* x;
    void* y;            // [N][C] float32, or uint8 codes (YC)
    int64_t total;      // NHWC: N * C / 4 (image, channel group) pairs; NCHW: N * C planes
    int64_t hw;         // pixels per plane
    int64_t c;          // channels
    float div;          // (float)(H W)
    int relu;
    int fmt_out;        // YC: format of the codes
    EncArgs enc;        // YC: code table of the reader's Ka (kEncCode)
};
static_assert(sizeof(GapParams) <= 4096, "GapParams must fit the 4 KiB kernel-argument segment");

__device__ __forceinline__ float4 gap_add(const float4 s, float4 v, const int relu) {
    if (relu) v = relu4(v);
    return make_float4(s.x + v.x, s.y + v.y, s.z + v.z, s.w + v.w);
}

template <bool YC>
__global__ __launch_bounds__(256) void k_gap_nhwc(const GapParams p) {
    __shared__ __attribute__((aligned(16))) float4 spart[4][64];
    __shared__ __attribute__((aligned(16))) unsigned char senc[YC ? kPwTab : 16];
    if constexpr (YC) enc_fill<256>(reinterpret_cast<uint2*>(senc), p.enc);

    const int lane = threadIdx.x & 63, j = threadIdx.x >> 6;
    const int64_t idx = (int64_t)blockIdx.x * 64 + lane;
    const bool ok = idx < p.total;
    const int64_t id = ok ? idx : p.total - 1;   // lanes past the end re-read the last pair and store nothing
    const int64_t c4 = p.c >> 2;
    const int64_t n = id / c4, cg = id - n * c4;
    const float* px = p.x + (size_t)n * (size_t)p.hw * (size_t)p.c + (size_t)cg * 4;
    const size_t ld = (size_t)p.c;
    const int relu = p.relu;

    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    int64_t q = j;
    for (; q + 12 < p.hw; q += 16) {   // four loads ahead of the four adds of this lane's ONE chain per channel
        const float4 v0 = *reinterpret_cast<const float4*>(px + (size_t)q * ld);
        const float4 v1 = *reinterpret_cast<const float4*>(px + (size_t)(q + 4) * ld);
        const float4 v2 = *reinterpret_cast<const float4*>(px + (size_t)(q + 8) * ld);
        const float4 v3 = *reinterpret_cast<const float4*>(px + (size_t)(q + 12) * ld);
        s = gap_add(s, v0, relu); s = gap_add(s, v1, relu); s = gap_add(s, v2, relu); s = gap_add(s, v3, relu);
    }
    for (; q < p.hw; q += 4) s = gap_add(s, *reinterpret_cast<const float4*>(px + (size_t)q * ld), relu);
    spart[j][lane] = s;
    __syncthreads();
    if (j != 0) return;

    const float4 s0 = spart[0][lane], s1 = spart[1][lane], s2 = spart[2][lane], s3 = spart[3][lane];
    float4 r;
    r.x = ((s0.x + s1.x) + (s2.x + s3.x)) / p.div;
    r.y = ((s0.y + s1.y) + (s2.y + s3.y)) / p.div;
    r.z = ((s0.z + s1.z) + (s2.z + s3.z)) / p.div;
    r.w = ((s0.w + s1.w) + (s2.w + s3.w)) / p.div;
    if constexpr (YC) {
        const CodeQuant cq{p.enc.r1, p.enc.lo, p.enc.hi, 1, p.fmt_out};
        const uint32_t code = code4<false, true>(r, cq, senc);
        if (ok) *reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(p.y) + (size_t)idx * 4) = code;
    } else {
        if (ok) *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.y) + (size_t)idx * 4) = r;
    }
}

template <bool YC>
__global__ __launch_bounds__(256) void k_gap_nchw(const GapParams p) {
    __shared__ __attribute__((aligned(16))) unsigned char senc[YC ? kPwTab : 16];
    if constexpr (YC) {
        enc_fill<256>(reinterpret_cast<uint2*>(senc), p.enc);
        __syncthreads();
    }
    const int j = threadIdx.x & 3;
    const int64_t idx = (int64_t)blockIdx.x * 64 + (threadIdx.x >> 2);   // plane n * C + c
    const bool ok = idx < p.total;
    const int64_t id = ok ? idx : p.total - 1;   // every lane takes part in the exchanges
    const float* px = p.x + (size_t)id * (size_t)p.hw;
    const int relu = p.relu;

    float s = 0.f;
    int64_t q = j;
    for (; q + 12 < p.hw; q += 16) {
        float v0 = px[q], v1 = px[q + 4], v2 = px[q + 8], v3 = px[q + 12];
        if (relu) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); v2 = fmaxf(v2, 0.f); v3 = fmaxf(v3, 0.f); }
        s = s + v0; s = s + v1; s = s + v2; s = s + v3;
    }
    for (; q < p.hw; q += 4) {
        float v = px[q];
        if (relu) v = fmaxf(v, 0.f);
        s = s + v;
    }
    const float a = s + __shfl_xor(s, 1);   // lanes 0, 1: s_0 + s_1; lanes 2, 3: s_2 + s_3
    const float t = a + __shfl_xor(a, 2);   // (s_0 + s_1) + (s_2 + s_3) in all four
    const float r = t / p.div;
    if constexpr (YC) {
        // C is a multiple of 4: planes 4 g .. 4 g + 3 are four channels of one image and sit in lanes 16 k, + 4, + 8, + 12
        const int l = threadIdx.x & 63;
        const float4 r4 = make_float4(r, __shfl(r, (l + 4) & 63), __shfl(r, (l + 8) & 63), __shfl(r, (l + 12) & 63));
        const CodeQuant cq{p.enc.r1, p.enc.lo, p.enc.hi, 1, p.fmt_out};
        const uint32_t code = code4<false, true>(r4, cq, senc);
        if (ok && (l & 15) == 0) *reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(p.y) + (size_t)idx) = code;
    } else {
        if (ok && j == 0) reinterpret_cast<float*>(p.y)[idx] = r;
    }
}

static int gap_fmt(int qbits) { return qbits == 7 ? kFmtSfp7 : kFmtAct8; }

// The host-only answer of slfp_global_avgpool_supported.
static bool gap_supported(int64_t n, int64_t h, int64_t w, int64_t c, int x_layout, const slfp_conv2d_io* io) {
    if (!io || n < 0 || h < 1 || w < 1 || c < 1) return false;
    if (x_layout != SLFP_LAYOUT_NHWC && x_layout != SLFP_LAYOUT_NCHW) return false;
    if (io->x_codes != 0 || (io->y_codes != 0 && io->y_codes != 1)) return false;
    if (x_layout == SLFP_LAYOUT_NHWC && c % 4) return false;
    if (h > 0x7FFFFFFF || w > 0x7FFFFFFF || h * w > 0x7FFFFFFF || c > 0x7FFFFFFF) return false;
    if (n > (int64_t)0x7FFFFFFF * 64 / c) return false;   // the grid: at most ceil(N C / 64) workgroups
    if (io->y_codes) {
        if (c % 4) return false;
        if ((io->y_qbits != 8 && io->y_qbits != 7) || !(io->y_ka > 0.f) || !scale_div_ok(io->y_ka)) return false;
        if (long_encode_forced()) return false;   // SLFP_LONG_ENCODE keeps every kernel off the tables
        if (!enc_table(io->y_ka, gap_fmt(io->y_qbits), kEncCode)->valid) return false;
    }
    return true;
}

}  // namespace slfp

using namespace slfp;

extern "C" {

int slfp_global_avgpool_supported(int64_t n, int64_t h, int64_t w, int64_t c, int x_layout, const slfp_conv2d_io* io) {
    return gap_supported(n, h, w, c, x_layout, io) ? 1 : 0;
}

int slfp_global_avgpool_f32(const float* x, void* y, int64_t n, int64_t h, int64_t w, int64_t c, int x_layout, int relu,
                            const slfp_conv2d_io* io, void* stream) {
    if (!io) return fail(SLFP_ERR_BAD_ARG, "slfp_global_avgpool_f32: null io");
    if (!x || !y) return fail(SLFP_ERR_BAD_ARG, "slfp_global_avgpool_f32: null pointer");
    if (x_layout != SLFP_LAYOUT_NHWC && x_layout != SLFP_LAYOUT_NCHW) return fail(SLFP_ERR_BAD_ARG, "slfp_global_avgpool_f32: bad layout");
    if (relu != 0 && relu != 1) return fail(SLFP_ERR_BAD_ARG, "slfp_global_avgpool_f32: relu must be 0 or 1");
    if ((io->y_codes != 0 && io->y_codes != 1) || io->x_codes != 0) return fail(SLFP_ERR_BAD_ARG, "slfp_global_avgpool_f32: x is float32 (x_codes 0), y_codes 0 or 1");
    if (io->y_codes && io->y_qbits != 8 && io->y_qbits != 7) return fail(SLFP_ERR_BAD_ARG, "slfp_global_avgpool_f32: y_qbits must be 8 or 7");
    if (n < 0 || h < 1 || w < 1 || c < 1) return fail(SLFP_ERR_SHAPE, "slfp_global_avgpool_f32: bad geometry");
    if (!gap_supported(n, h, w, c, x_layout, io))
        return fail(SLFP_ERR_UNSUPPORTED, "slfp_global_avgpool_f32: no kernel for this shape / layout / io combination "
                                          "(slfp_global_avgpool_supported): NHWC and code output need C % 4 == 0, codes a y_ka with a table");
    const bool nhwc = x_layout == SLFP_LAYOUT_NHWC;
    const uintptr_t bits = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y);
    if (nhwc && (bits & 15)) return fail(SLFP_ERR_ALIGNMENT, "slfp_global_avgpool_f32: NHWC needs 16-byte aligned pointers");
    if (!nhwc && (bits & 3)) return fail(SLFP_ERR_ALIGNMENT, "slfp_global_avgpool_f32: pointers must be 4-byte aligned");
    if (n == 0) return SLFP_OK;
    GapParams p = {};
    p.x = x; p.y = y;
    p.hw = h * w; p.c = c;
    p.total = nhwc ? n * (c / 4) : n * c;
    p.div = (float)p.hw;
    p.relu = relu;
    p.fmt_out = gap_fmt(io->y_qbits);
    p.enc.valid = 0;
    if (io->y_codes) p.enc = *enc_table(io->y_ka, p.fmt_out, kEncCode);
    const int64_t grid = ceil_div(p.total, 64);
    if (grid > 0x7FFFFFFF) return fail(SLFP_ERR_UNSUPPORTED, "slfp_global_avgpool_f32: grid too large");
    void (*k)(const GapParams) = nhwc ? (io->y_codes ? k_gap_nhwc<true> : k_gap_nhwc<false>)
                                      : (io->y_codes ? k_gap_nchw<true> : k_gap_nchw<false>);
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), p);
    return check_launch("slfp global average pool kernel");
}

}  // extern "C"
