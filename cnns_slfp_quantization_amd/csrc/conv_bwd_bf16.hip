// conv_bwd_bf16.hip -- the pointwise / Linear_Q backward (conv_bwd.hip's `pw` family) on the bf16 matrix cores, float32-equivalent
// through an exact three-way split (include/slfp.h: slfp_conv2d_bwd_bf16; opt-in, options.backward_gemm = "bf16x3").
//
//     gx[M x Cin]    = (GY[M x Cout] * WQ[Cout x Cin]) * Kw          M = N*H*W rows of NHWC
//     gw[Cout x Cin] = (GY^T * XQ[M x Cin]) * Ka, split over M       xq = QA(x / Ka), never materialised
//     gb[Cout]       = sum_m GY                                      float32 VALU adds
//
// A float32 a is p1 + p2 + p3 exactly, each p a bf16: p1 = the top 16 bits of a (truncation), p2 = the top 16 bits of a - p1, p3 = the
// rest (a carries 24 significant bits, each piece at most 8; the subtractions are exact, nothing rounds, nothing overflows).  A product
// of two pieces has at most 16 significant bits and is exact in float32, so v_mfma_f32_32x32x16_bf16 on the pieces accumulates what
// the float32 MFMA of conv_bwd.hip accumulates.  Both operands carry three planes and the six cross terms g_i * x_j with i + j <= 2
// are kept ("t6"; the three dropped ones are below 2 * 2^-24 |g||x| per product): eight k per instruction and six instructions against
// one float32 MFMA per two k.  SLFP<3,4> values 2^(m/16) need all 24 bits.  SFP<3,3> values have 4 significant bits and would fit one
// plane (a three-term form), but both quantizers also emit the class +-1e-10 (sfp_quant.py:43,92), a full 24-bit float32: in one
// plane it would be off by 2^-8, and a gradient element whose terms all come from that class would miss the 1e-5 bar.  So q_bit 7
// takes the six terms too and no three-term instance is built.  Within one MFMA k-step (16) the lowest-order terms are issued first.
//
// The kernel, k_bf16_gemm, its LDS and bank layout and the split helpers are in conv_bwd_bf16_core.hpp, which conv_bwd_dense_bf16.hip
// (the dense family on the same arithmetic) includes too; this file keeps k_wq_planes, the pw family's shapes and its entry points.
//
// Differences to the float32 kernels: an inf in gy splits into (inf, NaN, NaN), so outputs the float32 kernels make +-inf can be NaN
// here (the set of non-finite elements is the same); pieces below 2^-126 may be flushed by the matrix unit.
#include "conv_bwd_bf16_core.hpp"
#include <algorithm>
#include <cstdio>

namespace slfp {

// planes[p][ci][k] = piece p of wq[k][ci] as bf16, k < kpad (zeros from c_out on).  A workgroup transposes a tile of 32 k x 32 ci
// through LDS: the reads are 128-byte rows of wq (ci contiguous), the writes 16-byte chunks of 64-byte rows of the planes (k contiguous).
__global__ __launch_bounds__(256) void k_wq_planes(const float* __restrict__ wq, uint16_t* __restrict__ planes, int Cout, int Cin, int kpad) {
    __shared__ __attribute__((aligned(16))) uint16_t tile[kPlanes][32][kPitch];   // [plane][ci][k]
    const int ci0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
    const int c = threadIdx.x & 31;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = (threadIdx.x >> 5) + 8 * i;
        const bool ok = k0 + r < Cout && ci0 + c < Cin;
        const float v = wq[ok ? (int64_t)(k0 + r) * Cin + ci0 + c : 0];
        uint32_t b[3];
        split3(ok ? v : 0.f, b[0], b[1], b[2]);
#pragma unroll
        for (int p = 0; p < kPlanes; ++p) tile[p][c][r] = (uint16_t)(b[p] >> 16);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < kPlanes * 32 * 4; e += 256) {   // 16-byte chunks: (plane, ci, quarter of the 32 k)
        const int p = e >> 7, cc = (e >> 2) & 31, q = e & 3;
        if (ci0 + cc < Cin)   // k0 + 31 < kpad: the planes are padded to whole k-steps
            *reinterpret_cast<uint4*>(planes + ((int64_t)p * Cin + ci0 + cc) * kpad + k0 + q * 8) = *reinterpret_cast<const uint4*>(&tile[p][cc][q * 8]);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------
// What the launch is sized by: the tiles, the planes of the quantized operand, the gw split.  A function of the descriptor only.
struct Bf16Shape {
    int64_t M;        // rows = N*H*W
    int tm_x, tn_x;   // gx tiling
    int tm_w, tn_w;   // gw tiling
    int kpad;         // k pitch of the WQ planes
    int splits, kps;  // gw split of M (gw_split)
};

static Bf16Shape bf16_shape(const slfp_conv2d_desc& d) {
    Bf16Shape s;
    s.M = d.n * d.h * d.w;
    const int64_t cin = d.c_in, cout = d.c_out;
    s.tm_x = s.M >= 128 ? 2 : 1;  s.tn_x = cin >= 128 ? 2 : 1;
    s.tm_w = cout >= 128 ? 2 : 1; s.tn_w = cin >= 128 ? 2 : 1;
    s.kpad = (int)(ceil_div(cout, kBK) * kBK);
    const GwSplit sp = gw_split(s.M, cout, cin, ceil_div(cout, 64 * s.tm_w) * ceil_div(cin, 64 * s.tn_w));
    s.splits = sp.splits; s.kps = sp.kps;
    return s;
}

// The layers the kernels take, whichever way x arrives (what the workspace is sized for): 0 and the reason in slfp_last_error, or 1.
static int bf16_layer_ok(const slfp_conv2d_desc* d) {
    auto no = [](const char* why) { fail(SLFP_ERR_UNSUPPORTED, "slfp_conv2d_bwd_bf16: %s", why); return 0; };
    if (!bwd_is_pw(*d)) return no("only stride-1 1x1 layers (the pw family); depthwise and dense layers stay on slfp_conv2d_bwd_ex");
    if (d->x_layout != SLFP_LAYOUT_NHWC || d->y_layout != SLFP_LAYOUT_NHWC) return no("NHWC only");
    if (d->c_in % 8 != 0 || d->c_out % 8 != 0) return no("C_in and C_out must be multiples of 8");
    if (d->n * d->h * d->w >= 0x7FFFFF00) return no("N*H*W must stay below 2^31");
    // measured not faster than the float32 kernels by more than the spread (profiles/backward_bf16_bench.json), so not taken:
    // (a) the weight planes cost the same at every batch, what the GEMMs save grows with the rows: 25088 -> 4096 loses at 128 rows
    // (0.88x) and wins at 512 (1.24x); 4096 -> 4096 (2^24 elements) wins at 128 already
    if (d->n * d->h * d->w < 512 && d->c_in * d->c_out > ((int64_t)1 << 24))
        return no("fewer than 512 rows under a weight of more than 2^24 elements: the weight planes cost more than the GEMMs save");
    // (b) the HBM-bound layers with a narrow and a wide side at image sizes (64 -> 128, 64 -> 256, 256 -> 64 at 56 x 56, batch 128):
    // 1.01-1.09x, inside the spread in one of two runs; 32 -> 64 and 64 -> 64 stay in (1.18x, 1.02-1.07x beyond the spread in both)
    if (std::min(d->c_in, d->c_out) <= 64 && std::max(d->c_in, d->c_out) >= 128 && d->n * d->h * d->w >= 65536)
        return no("a side of at most 64 channels against one of at least 128 over 65536 rows or more measured level with the float32 kernels");
    return 1;
}

// ... and this operand form: float32 x needs the threshold table (codes are decoded, not encoded; NHWC with C_in % 8 == 0 is codes_ok)
static int bf16_supported(const slfp_conv2d_desc* d, const ConvPlan& p, bool x_codes) {
    if (!bf16_layer_ok(d)) return 0;
    if (!x_codes && !act_table(d->ka, p.fmt_act, kEncF32)) {
        fail(SLFP_ERR_UNSUPPORTED, "slfp_conv2d_bwd_bf16: no threshold table for this Ka (float32 x)");
        return 0;
    }
    return 1;
}

struct Bf16Layout {  // byte offsets into the workspace
    size_t wq, planes, part, gbpart, total;
};

static Bf16Layout bf16_layout(const slfp_conv2d_desc& d, const Bf16Shape& s, bool need_gx, bool need_gw) {
    Bf16Layout L;
    size_t off = 0;
    L.wq = off; if (need_gx) off += r256((size_t)d.c_out * d.c_in * sizeof(float));
    L.planes = off; if (need_gx) off += r256((size_t)kPlanes * d.c_in * s.kpad * sizeof(uint16_t));
    L.part = off; if (need_gw && s.splits > 1) off += r256((size_t)s.splits * d.c_out * d.c_in * sizeof(float));
    L.gbpart = off; if (need_gw) off += r256((size_t)s.splits * d.c_out * sizeof(float));
    L.total = off;
    return L;
}

}  // namespace slfp

using namespace slfp;

extern "C" {

int slfp_conv2d_bwd_bf16_supported(const slfp_conv2d_desc* d, unsigned flags, int x_codes) {
    ConvPlan p;
    if (!d || (flags & ~SLFP_BWD_DENSE) || make_plan(d, &p) != SLFP_OK) return 0;
    return bf16_supported(d, p, x_codes != 0);
}

size_t slfp_conv2d_bwd_bf16_workspace_bytes(const slfp_conv2d_desc* d, unsigned flags, int need_gx, int need_gw) {
    ConvPlan p;
    if (!d || (flags & ~SLFP_BWD_DENSE) || make_plan(d, &p) != SLFP_OK || !bf16_layer_ok(d)) return 0;   // the same for x and x_codes
    return bf16_layout(*d, bf16_shape(*d), need_gx != 0, need_gw != 0).total;
}

const char* slfp_debug_bwd_bf16_instance(const slfp_conv2d_desc* d, unsigned flags, int x_codes, int need_gx, int need_gw) {
    static thread_local char buf[160];
    ConvPlan p;
    if (!d || (flags & ~SLFP_BWD_DENSE) || make_plan(d, &p) != SLFP_OK || !bf16_supported(d, p, x_codes != 0)) return "none";
    if (!need_gx && !need_gw) return "none";
    const Bf16Shape s = bf16_shape(*d);
    int n = 0;
    if (need_gx) n += std::snprintf(buf + n, sizeof buf - n, "pwb/gx/tm%dtn%d/t6", s.tm_x, s.tn_x);
    if (need_gw)
        std::snprintf(buf + n, sizeof buf - n, "%spwb/gw/tm%dtn%d/t6/%s/p%dk%d", n ? "+" : "", s.tm_w, s.tn_w,
                      x_codes ? "codes" : "tab", s.splits, s.kps);
    return buf;
}

int slfp_conv2d_bwd_bf16(const slfp_conv2d_desc* d, unsigned flags, const float* x, const uint8_t* x_codes, const float* w_oihw,
                         const float* gy, float* gx, float* gw_oihw, float* gb, void* workspace, void* stream) {
    if (!d) return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd_bf16: null descriptor");
    if (flags & ~SLFP_BWD_DENSE) return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd_bf16: unknown flag bits 0x%x", flags & ~SLFP_BWD_DENSE);
    if ((x != nullptr) == (x_codes != nullptr)) return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd_bf16: exactly one of x and x_codes");
    if ((x && !aligned16(x)) || (w_oihw && !aligned16(w_oihw)) || (gy && !aligned16(gy)) || (gx && !aligned16(gx)) ||
        (gw_oihw && !aligned16(gw_oihw)) || (gb && !aligned16(gb)))
        return fail(SLFP_ERR_ALIGNMENT, "slfp_conv2d_bwd_bf16: tensors must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(x_codes) & 3) return fail(SLFP_ERR_ALIGNMENT, "slfp_conv2d_bwd_bf16: x_codes must be 4-byte aligned");
    ConvPlan p;
    int rc = make_plan(d, &p);
    if (rc != SLFP_OK) return rc;
    const bool codes = x_codes != nullptr;
    if (!bf16_supported(d, p, codes)) return SLFP_ERR_UNSUPPORTED;   // the reason is recorded
    if (!gy) return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd_bf16: null gy");
    if (gx && !w_oihw) return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd_bf16: gx needs the weights");
    if (gb && !gw_oihw) return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd_bf16: gb is computed together with gw");
    const bool need_gx = gx != nullptr, need_gw = gw_oihw != nullptr;
    if (!need_gx && !need_gw) return SLFP_OK;
    const Bf16Shape s = bf16_shape(*d);
    const Bf16Layout L = bf16_layout(*d, s, need_gx, need_gw);
    if (L.total && (!workspace || !aligned16(workspace)))
        return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd_bf16: %zu bytes of 16-byte aligned workspace required (slfp_conv2d_bwd_bf16_workspace_bytes)", L.total);
    unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
    hipStream_t st = as_stream(stream);
    const int Cin = (int)d->c_in, Cout = (int)d->c_out, M = (int)s.M;

    if (need_gx) {
        float* wq = reinterpret_cast<float*>(ws + L.wq);
        uint16_t* planes = reinterpret_cast<uint16_t*>(ws + L.planes);
        if ((rc = launch_quantize(w_oihw, wq, (size_t)Cout * Cin, d->kw_scale, p.fmt_w, st)) != SLFP_OK) return rc;
        hipLaunchKernelGGL(k_wq_planes, dim3((unsigned)ceil_div(Cin, 32), (unsigned)(s.kpad / 32)), dim3(256), 0, st, wq, planes, Cout, Cin, s.kpad);
        if ((rc = check_launch("slfp bf16 backward weight planes kernel")) != SLFP_OK) return rc;
        const Bf16Args a{gy, planes, gx, nullptr, M, Cin, Cout, s.kpad, s.kpad, d->kw_scale};
        launch_bf16<false, kXBlob>(a, s.tm_x, s.tn_x, st, EncArgs{});
        if ((rc = check_launch("slfp bf16 pointwise backward (gx) kernel")) != SLFP_OK) return rc;
    }
    if (need_gw) {
        float* part = s.splits > 1 ? reinterpret_cast<float*>(ws + L.part) : gw_oihw;
        float* gbp = reinterpret_cast<float*>(ws + L.gbpart);
        const Bf16Args a{gy, codes ? (const void*)x_codes : (const void*)x, part, gb ? gbp : nullptr, Cout, Cin, M, 0, s.kps,
                         s.splits > 1 ? 1.0f : d->ka};
        launch_bf16_gw(a, s.tm_w, s.tn_w, st, codes, p.fmt_act, act_table(d->ka, p.fmt_act, kEncF32));
        if ((rc = check_launch("slfp bf16 pointwise backward (gw) kernel")) != SLFP_OK) return rc;
        if (s.splits > 1 && (rc = reduce_parts(st, part, s.splits, (int64_t)Cout * Cin, d->ka, 0, 0, 0, gw_oihw, nullptr)) != SLFP_OK) return rc;
        if (gb && (rc = reduce_gb(st, gbp, s.splits, Cout, gb)) != SLFP_OK) return rc;
    }
    return SLFP_OK;
}

}  // extern "C"
