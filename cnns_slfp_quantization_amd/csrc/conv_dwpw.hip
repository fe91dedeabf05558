// conv_dwpw.hip -- one MobileNet block in one kernel: depthwise 3x3 Conv2d_Q -> eval BatchNorm -> ReLU ->
// pointwise 1x1 Conv2d_Q (-> BatchNorm -> ReLU), the intermediate tensor never leaving the CU (gfx950).
//
// The reference runs nets_imgnet/mobilenetv1.py:24-41's conv_dw block as six modules: Conv2d_Q(3x3, groups = C),
// BatchNorm2d, ReLU, Conv2d_Q(1x1), BatchNorm2d, ReLU.  fusion.fuse_bn_relu folds each BatchNorm/ReLU into the
// preceding conv's epilogue; fusion.fuse_dw_pw then pairs the two convs here (second half): the
// depthwise result is quantized for the pointwise layer (QA(. / Ka_pw), utils/conv2d_func.py:21) right where it is
// produced and goes to the MFMA through LDS as fp16, instead of a float32 round trip through HBM
// (4 B written + 4 B read per element = 40 % of the block's traffic for 32->64 at 112x112).
//
// Arithmetic is EXACTLY the two separate kernels' (conv_dw2.hip, conv_pw.hip: k_pw_stream), step for step, so the
// output is bit-identical to running them back to back.  The workgroup's plan, the geometry, the parameters and the
// steps shared with k_dwpw_codes (conv_dwpw_codes.hip) are in conv_dwpw_core.hpp.  This kernel's own:
//   input       float32 halo by 16-byte buffer loads, quantized through the threshold table (enc4_f32_raw), a NaN stays a NaN;
//   hand-over   the threshold-table quantizer in its packed-fp16 form with conv_pw.hip's NaN policy (enc4_f16);
//   epilogue    ((acc + 256 bq) * s1/256) * s2 with a branch around the bias add for a pair without epilogue vectors (it
//               decides the kernel's SGPR count, so it is not slfp_epilogue.hpp's epilogue(): DESIGN.md section 29), fma, max.
//
// Measured (profiles/dwpw_bench.py, batch 256, cold): the kernel removes 40 % (32->64) to 33 % of the pair's HBM
// traffic but runs 1-2 workgroups per CU with its phases in series, so it only breaks even on 32@112->64
// (399 vs 407 us) and is slower on the K = 64 / 128 pairs (412 vs 352, 420 vs 337, 316 vs 204 us).  fusion.fuse_dw_pw is
// therefore opt-in; DESIGN.md lists what the next version needs (fp16 halo tile, k-outer accumulation, >= 3 workgroups/CU).
#include "conv_dwpw_core.hpp"

namespace slfp {

struct DwPwParams : DwPwBase {
    EncArgsCompact enc1;   // QA(x / Ka_dw) as float32
    EncArgsCompact enc2;   // fp16(16 * QA(. / Ka_pw)), packed pairs (two tables: compact form, 4 KiB of kernel arguments in all)
};

// S, KS, NT: DwPwGeom's
template <int S, int KS, int NT>
__global__ __launch_bounds__(kDwPwT, 2) void k_dwpw(const DwPwParams p) {
    using G = DwPwGeom<S, KS, NT>;
    constexpr int TH = G::TH, TW = G::TW, IH = G::IH, RPL = G::RPL, NI = G::NI, ROWB = G::ROWB, NPX = G::NPX, NU = G::NU, NWV = G::NWV, UW = G::UW;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* tab2 = smem + kDwTabBytes;
    unsigned char* lds = tab2 + kDwTabBytes;
    unsigned char *tile = lds + G::tile, *x16 = lds + G::x16, *wl = lds + G::wl;
    float* ep = reinterpret_cast<float*>(lds + G::ep);

    enc_fill_compact<kDwPwT>(reinterpret_cast<uint2*>(smem), p.enc1);
    enc_fill_compact<kDwPwT>(reinterpret_cast<uint2*>(tab2), p.enc2);
    for (int i = threadIdx.x; i < NT * KS * 64; i += kDwPwT) {     // W -> LDS, 16 bytes per thread
        const int l = i & 63, t = i >> 6, ks = t % KS, j = t / KS;
        *reinterpret_cast<u32x4*>(wl + (size_t)i * 16) = *reinterpret_cast<const u32x4*>(p.wpw + ((size_t)j * p.KSb + ks) * 512 + l * 8);
    }
    dwpw_fill_ep_zero<G>(ep, x16, p);
    const DwPwIdx d = dwpw_index<G>(p);
    // in locals: read through `d` at the sites, the values reach the scheduler in another order and the register counts move
    const uint32_t n = d.n, lds_w = d.lds_w, lds_r0 = d.lds_r0;
    const int th = d.th, tw = d.tw, c4 = d.c4, iw = d.iw, ihh = d.ihh;
    const bool col_live = d.col_live;
    const float r1 = p.enc1.r1, lo1 = p.enc1.lo, hi1 = p.enc1.hi;
    const float r2 = p.enc2.r1, lo2 = p.enc2.lo, hi2 = p.enc2.hi;

    const __amdgpu_buffer_rsrc_t rs = dw_rsrc(reinterpret_cast<const float*>(p.x) + (size_t)n * p.H * p.W * p.C, (uint32_t)p.H * p.W * p.C * 4u);
    const int gw = tw * TW * S - p.pad + iw;
    const int gh0 = th * TH * S - p.pad + ihh;
    const bool w_ok = col_live && (unsigned)gw < (unsigned)p.W;
    const uint32_t off0 = (uint32_t)((gh0 * p.W + gw) * p.C + c4 * 4) * 4u;
    const uint32_t step = (uint32_t)(RPL * p.W * p.C) * 4u;
    uint32_t voff[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const bool ok = w_ok && (unsigned)(gh0 + RPL * i) < (unsigned)p.H && (RPL * i + ihh) < IH;
        voff[i] = ok ? off0 + (uint32_t)i * step : kDwOob;
        asm volatile("" : "+v"(voff[i]));
    }
    floatx4 v[NI];
    auto issue = [&](int cg) {   // halo tile of channel group cg: soffset moves along the channel axis
#pragma unroll
        for (int i = 0; i < NI; ++i)
            v[i] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff[i], (uint32_t)cg * 128u, 0));
    };

    // ================= phase 1: depthwise, one 32-channel group at a time =================
    issue(0);
    __syncthreads();   // tables, W, zero rows visible
#pragma unroll 1
    for (int cg = 0; cg < KS; ++cg) {
        const int c = cg * 32 + c4 * 4;
        floatx4 wt[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) wt[k] = *reinterpret_cast<const floatx4*>(p.wdw + (size_t)k * p.C + c);
        floatx4 psc, psh;
        dw_load_bn<true>(psc, psh, p.sc1, p.sh1, c);
        dw_put_halo<NI, RPL * ROWB>(tile + lds_w, v, r1, lo1, hi1, smem);
        __syncthreads();
        if (cg + 1 < KS) issue(cg + 1);   // in flight under the convolution below
#pragma unroll
        for (int j = 0; j < G::NO; ++j) {   // conv_dw2.hip's epilogue, then conv_pw.hip's quantizer
            const floatx4 acc = dw_mac9_lds<S, ROWB>(wt, tile + lds_r0 + j * G::RPI * S * ROWB);
            const float4 rr = dwpw_bn1(acc, psc, psh, p);
            dwpw_put_quad<G>(x16, d, j, cg, enc4_f16(rr, r2, lo2, hi2, tab2));
        }
        __syncthreads();   // the tile is free for the next group; after the last group: the fp16 image is complete
    }

    // ================= phase 2: pointwise on the matrix cores =================
    const int lane = threadIdx.x & 63, col = lane & 15, kq = lane >> 4;
    const int wv = threadIdx.x >> 6;
    half8 xh[UW][KS];
#pragma unroll
    for (int ui = 0; ui < UW; ++ui) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) xh[ui][ks] = dwpw_frag<G>(x16, wv + NWV * ui, col, kq, ks);
    }
    const __amdgpu_buffer_rsrc_t ry = dw_rsrc(reinterpret_cast<float*>(p.y) + (size_t)n * p.Ho * p.Wo * p.O, (uint32_t)p.Ho * p.Wo * p.O * 4u);
    unsigned char* stg = tile + wv * 2048;   // [8 waves][2 KiB]: phase 2 reuses the (then idle) halo tile
    const int spx = lane >> 3, sch = lane & 7;
    const bool has_vec = p.bias2 != nullptr || p.sc2 != nullptr;
    const int oh0 = th * TH, ow0 = tw * TW;
#pragma unroll 1
    for (int j0 = 0; j0 < NT; j0 += 2) {
#pragma unroll
        for (int ui = 0; ui < UW; ++ui) {
            const int u = wv + NWV * ui;
            if (u < NU) {   // wave-uniform
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const int j = j0 + jj;
                    const floatx4 acc = dwpw_mma<G>(wl, xh[ui], j, lane);
                    const int nl = j * 16 + kq * 4;
                    float4 r = make_float4(acc[0], acc[1], acc[2], acc[3]);
                    if (has_vec) {
                        const float4 bq = *reinterpret_cast<const float4*>(ep + nl);
                        r.x += bq.x; r.y += bq.y; r.z += bq.z; r.w += bq.w;
                    }
                    r.x = (r.x * p.s1x) * p.s2; r.y = (r.y * p.s1x) * p.s2; r.z = (r.z * p.s1x) * p.s2; r.w = (r.w * p.s1x) * p.s2;
                    if (p.sc2) {
                        const float4 sc = *reinterpret_cast<const float4*>(ep + NT * 16 + nl);
                        const float4 sh = *reinterpret_cast<const float4*>(ep + 2 * NT * 16 + nl);
                        r = affine4(r, sc, sh);
                    }
                    if (p.relu2) r = relu4(r);
                    *reinterpret_cast<float4*>(stg + col * 128 + jj * 64 + kq * 16) = r;
                }
                // LDS operations of one wave execute in order: reads see the writes, the next writes follow the reads
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const u32x4 vv = *reinterpret_cast<const u32x4*>(stg + lane * 16 + h * 1024);
                    const int pix = u * 16 + spx + 8 * h;                      // pixel of the tile
                    const int oh = pix / TW, owp = pix - oh * TW;
                    const bool live = pix < NPX && (oh0 + oh) < p.Ho && (ow0 + owp) < p.Wo;
                    uint32_t so = live ? (uint32_t)(((oh0 + oh) * p.Wo + ow0 + owp) * p.O + j0 * 16 + sch * 4) * 4u : kDwOob;
                    asm volatile("" : "+v"(so));
                    __builtin_amdgcn_raw_buffer_store_b128(vv, ry, so, 0, 0);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------- host
static bool dwpw_shape(const slfp_conv2d_desc& dw, const slfp_conv2d_desc& pw, int* ks, int* nt) {
    if (dw.groups != dw.c_in || dw.c_out != dw.c_in || dw.kh != 3 || dw.kw != 3 || dw.dil_h != 1 || dw.dil_w != 1) return false;
    if (dw.stride_h != dw.stride_w || (dw.stride_h != 1 && dw.stride_h != 2) || dw.pad_h != dw.pad_w || dw.pad_h > 2) return false;
    if (pw.kh != 1 || pw.kw != 1 || pw.groups != 1 || pw.stride_h != 1 || pw.stride_w != 1 || pw.pad_h || pw.pad_w) return false;
    if (pw.c_in != dw.c_out || dw.qbits != pw.qbits) return false;
    if (dw.x_layout != SLFP_LAYOUT_NHWC || pw.y_layout != SLFP_LAYOUT_NHWC) return false;
    const int K = (int)dw.c_in, N = (int)pw.c_out;
    if (K != 32 && K != 64 && K != 128) return false;
    if (N != 64 && N != 128 && N != 256) return false;
    if ((size_t)K * N * 2 > 64 * 1024) return false;
    if (dw.stride_h == 1 && (dw.h < 14 || dw.w < 14)) return false;
    *ks = K / 32; *nt = N / 16;
    return true;
}

static size_t dwpw_lds(int S, int KS, int NT) { return (size_t)2 * kDwTabBytes + dwpw_geom_bytes(S, KS, NT); }

// What slfp_dwpw_fwd chooses among k_dwpw's instances; slfp_dwpw_supported is this function's answer.
bool dwpw_select(const slfp_conv2d_desc* dw, const slfp_conv2d_desc* pw, DwPwSel* s) {
    if (!dw || !pw || long_encode_forced()) return false;
    ConvPlan p1, p2;
    if (make_plan(dw, &p1) != SLFP_OK || make_plan(pw, &p2) != SLFP_OK) return false;
    if (p1.family != kDw3x3 || p2.family != kPointwise || p1.repad || p2.repad || p2.passes != 1) return false;
    if (pw->n != dw->n || pw->h != p1.h_out || pw->w != p1.w_out) return false;
    int ks, nt;
    if (!dwpw_shape(*dw, *pw, &ks, &nt)) return false;
    if (!dwpw_instance_built(dw->stride_h, ks, nt)) return false;
    if (dwpw_lds(dw->stride_h, ks, nt) > 160 * 1024) return false;
    if (!act_table(dw->ka, p1.fmt_act, kEncF32) || !act_table(pw->ka, p2.fmt_act, kEncF16P)) return false;
    s->s = dw->stride_h; s->ks = ks; s->nt = nt;
    s->fmt_in = p1.fmt_act; s->yc = false;   // not k_dwpw's: float32 in and out
    return true;
}

}  // namespace slfp

using namespace slfp;

extern "C" int slfp_dwpw_supported(const slfp_conv2d_desc* dw, const slfp_conv2d_desc* pw) {
    DwPwSel sel;
    return dwpw_select(dw, pw, &sel) ? 1 : 0;
}

extern "C" int slfp_dwpw_fwd(const slfp_conv2d_desc* dw, const slfp_conv2d_desc* pw, const float* x, const void* wprep_dw,
                             const float* post1_scale, const float* post1_shift, int relu1, const void* wprep_pw,
                             const float* bias_pw, const float* post2_scale, const float* post2_shift, int relu2, float* y,
                             void* stream) {
    if ((relu1 & ~1) != 0 || (relu2 & ~1) != 0) return fail(SLFP_ERR_BAD_ARG, "slfp_dwpw_fwd: relu1 / relu2 are 0 or 1");
    DwPwSel sel;
    if (!dwpw_select(dw, pw, &sel)) return fail(SLFP_ERR_UNSUPPORTED, "slfp_dwpw_fwd: this pair of layers is not fusable (slfp_dwpw_supported)");
    if (!x || !wprep_dw || !wprep_pw || !y || !post1_scale || !post1_shift)
        return fail(SLFP_ERR_BAD_ARG, "slfp_dwpw_fwd: null pointer (the depthwise layer's folded BatchNorm is required)");
    if ((post2_scale == nullptr) != (post2_shift == nullptr)) return fail(SLFP_ERR_BAD_ARG, "slfp_dwpw_fwd: post2_scale and post2_shift go together");
    if (!aligned16(x) || !aligned16(y) || !aligned16(wprep_dw) || !aligned16(wprep_pw) || !aligned16(post1_scale) || !aligned16(post1_shift))
        return fail(SLFP_ERR_ALIGNMENT, "slfp_dwpw_fwd: pointers must be 16-byte aligned");
    ConvPlan p1, p2;
    make_plan(dw, &p1);
    make_plan(pw, &p2);
    const int S = sel.s, ks = sel.ks, nt = sel.nt;
    DwPwParams p;
    const int64_t nblocks = dwpw_fill_base(p, dw, pw, p1, p2, x, wprep_dw, post1_scale, post1_shift, relu1, wprep_pw, bias_pw, post2_scale,
                                           post2_shift, relu2, y);
    if (nblocks > 0x7FFFFFFF || (int64_t)p.H * p.W * p.C >= (1ll << 29) || (int64_t)p.Ho * p.Wo * p.O >= (1ll << 29))
        return fail(SLFP_ERR_UNSUPPORTED, "slfp_dwpw_fwd: tensor too large");
    p.enc1 = enc_compact(*act_table(dw->ka, p1.fmt_act, kEncF32));
    p.enc2 = enc_compact(*act_table(pw->ka, p2.fmt_act, kEncF16P));
    static_assert(sizeof(DwPwParams) <= 4096, "kernel arguments must fit the 4 KiB kernarg segment");
    const size_t lds = dwpw_lds(S, ks, nt);
    hipStream_t st = as_stream(stream);
#define SLFP_F(SS, KK, NN)                                                                                         \
    if (S == SS && ks == KK && nt == NN) {                                                                          \
        auto fn = k_dwpw<SS, KK, NN>;                                                                               \
        const int rc = raise_lds_limit(reinterpret_cast<const void*>(fn), lds);                                     \
        if (rc != SLFP_OK) return rc;                                                                               \
        hipLaunchKernelGGL(fn, dim3(p.nblocks), dim3(kDwPwT), lds, st, p);                                          \
        return check_launch("slfp fused depthwise + pointwise kernel");                                             \
    }
    SLFP_DWPW_INSTANCES(SLFP_F)
#undef SLFP_F
    return fail(SLFP_ERR_UNSUPPORTED, "slfp_dwpw_fwd: no instantiation for this shape");   // not reached: dwpw_select admits SLFP_DWPW_INSTANCES only
}
