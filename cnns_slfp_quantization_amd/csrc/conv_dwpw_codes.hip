// conv_dwpw_codes.hip -- one MobileNet block in one kernel ON 1-BYTE CODES: depthwise 3x3 Conv2d_Q -> eval BatchNorm -> ReLU ->
// pointwise 1x1 Conv2d_Q (-> BatchNorm -> ReLU), codes in, codes or float32 out, the intermediate tensor never leaving the CU (gfx950).
//
// conv_dwpw.hip (k_dwpw) is this pair on the float32 interface; inside a chain linked by fusion.link_codes the pair runs as
// conv_dwc.hip (k_dwc) -> conv_pw_codes.hip (k_pwc_stream), and the hand-over between the two costs one encode (threshold-table
// lookup + pack), one 1-byte store, one load and one decode through a 256-entry LDS table per element, in kernels that are bound by
// instruction issue.  Here the depthwise result goes through the pointwise layer's quantizer straight into the fp16 MFMA operand
// (enc4_f16, kEncF16P table) in LDS: no code is formed for it.
//
// Arithmetic is EXACTLY the two code kernels', step for step, so the output is bit-identical to running them back to back:
//   k_dwc:        codes -> float32 through the kDecF32 table (an out-of-image tap is the exact-zero code 0x01 = +0.0), float32 FMAs in
//                 (kh, kw) order from +0, (acc * Ka) * Kw, fma(scale, shift), the ReLU;
//   hand-over:    k_dwc writes the code of the class QA(. / Ka_pw), k_pwc_stream reads fp16(16 * value of that class) from its decode
//                 table; enc4_f16's table holds fp16(16 * QA(. / Ka_pw)) of the same classes (a NaN has no code: k_dwc writes 0x00, the
//                 "tiny" class, whose operand is the fp16 zero -- patched to the same zero here);
//   k_pwc_stream: v_mfma_f32_16x16x32_f16 over k in blob order from +0, the tile epilogue of slfp_epilogue.hpp, then the ReLU
//                 (float32 out) or the reader's code quantizer (code4: the ReLU folded in, or signed codes).
//
// The workgroup's plan, the geometry, the parameters and the steps shared with k_dwpw are in conv_dwpw_core.hpp.  This kernel's own:
//   input       the halo's codes by dword loads through a buffer descriptor, decoded to the float32 halo tile (dec4_f32);
//   hand-over   enc4_f16_raw and the NaN patch above;
//   output      float32 staged to 128-byte pieces as in k_dwpw, or (YC) codes, four channel tiles at a time through
//               rows_transpose4, 16 bytes per lane = 64 contiguous bytes per pixel and wave.
// The K >= 256 blocks (W does not fit LDS) are not covered.  Measurements: profiles/dwpw_codes_bench.py, DESIGN.md section 23.
#include "slfp_codes.hpp"
#include "conv_dwpw_core.hpp"

namespace slfp {

struct DwPwCodesParams : DwPwBase {   // fmt_out (DwPwBase) is set for YC
    EncArgsCompact enc2;   // fp16(16 * QA(. / Ka_pw)), packed pairs (kEncF16P)
    EncArgsCompact encY;   // YC: code table of the reader's Ka (kEncCode); two compact tables: 4 KiB of kernel arguments in all
};

// S, KS, NT: DwPwGeom's; FMT: what the input codes are (kFmtAct8 | kFmtSfp7); YC: output as codes (else float32)
template <int S, int KS, int NT, int FMT, bool YC>
__global__ __launch_bounds__(kDwPwT, 2) void k_dwpw_codes(const DwPwCodesParams p) {
    using G = DwPwGeom<S, KS, NT>;
    constexpr int TH = G::TH, TW = G::TW, IH = G::IH, RPL = G::RPL, NI = G::NI, ROWB = G::ROWB, NPX = G::NPX, NU = G::NU, NWV = G::NWV, UW = G::UW;
    static_assert(NT % 4 == 0, "code output leaves in groups of 4 channel tiles");

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* dtab = smem;                                // 256-entry decode table (kDecF32)
    unsigned char* tab2 = dtab + kDecBytes;                    // pointwise quantizer (kEncF16P)
    unsigned char* tabY = tab2 + kDwTabBytes;                     // reader's code table (YC)
    unsigned char* lds = tabY + kDwTabBytes;
    unsigned char *tile = lds + G::tile, *x16 = lds + G::x16, *wl = lds + G::wl;
    float* ep = reinterpret_cast<float*>(lds + G::ep);

    dec_fill<FMT, kDecF32, kDwPwT>(reinterpret_cast<uint32_t*>(dtab));
    enc_fill_compact<kDwPwT>(reinterpret_cast<uint2*>(tab2), p.enc2);
    if constexpr (YC) enc_fill_compact<kDwPwT>(reinterpret_cast<uint2*>(tabY), p.encY);
    for (int i = threadIdx.x; i < NT * KS * 64; i += kDwPwT) {     // W -> LDS, 16 bytes per thread
        const int l = i & 63, t = i >> 6, ks = t % KS, j = t / KS;
        *reinterpret_cast<u32x4*>(wl + (size_t)i * 16) = *reinterpret_cast<const u32x4*>(p.wpw + ((size_t)j * p.KSb + ks) * 512 + l * 8);
    }
    dwpw_fill_ep_zero<G>(ep, x16, p);
    const DwPwIdx d = dwpw_index<G>(p);
    // in locals, as in k_dwpw
    const uint32_t n = d.n, lds_w = d.lds_w, lds_r0 = d.lds_r0;
    const int th = d.th, tw = d.tw, c4 = d.c4, iw = d.iw, ihh = d.ihh;
    const bool col_live = d.col_live;
    const float r2 = p.enc2.r1, lo2 = p.enc2.lo, hi2 = p.enc2.hi;

    // the image's codes, 1 B per element: a lane's dword = 4 channels of one halo pixel
    const __amdgpu_buffer_rsrc_t rs = dw_rsrc(reinterpret_cast<const uint8_t*>(p.x) + (size_t)n * p.H * p.W * p.C, (uint32_t)p.H * p.W * p.C);
    const int gw = tw * TW * S - p.pad + iw;
    const int gh0 = th * TH * S - p.pad + ihh;
    const bool w_ok = col_live && (unsigned)gw < (unsigned)p.W;
    const uint32_t off0 = (uint32_t)((gh0 * p.W + gw) * p.C + c4 * 4);
    const uint32_t step = (uint32_t)(RPL * p.W * p.C);
    uint32_t voff[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const bool ok = w_ok && (unsigned)(gh0 + RPL * i) < (unsigned)p.H && (RPL * i + ihh) < IH;
        voff[i] = ok ? off0 + (uint32_t)i * step : kDwBadRow;   // past every tensor (< 2^29 bytes) with the channel group's offset added
        asm volatile("" : "+v"(voff[i]));
    }
    uint32_t v[NI];
    auto issue = [&](int cg) {   // halo codes of channel group cg: soffset moves along the channel axis
#pragma unroll
        for (int i = 0; i < NI; ++i) v[i] = __builtin_amdgcn_raw_buffer_load_b32(rs, voff[i], (uint32_t)cg * 32u, 0);
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
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            // zero padding (and the halo slots outside the tile's window) = the exact-zero code, as in k_dwc: the returned 0 would be
            // the code of the "tiny" class
            const uint32_t codes = voff[i] == kDwBadRow ? 0x01010101u : v[i];
            *reinterpret_cast<float4*>(tile + lds_w + (uint32_t)i * (uint32_t)(RPL * ROWB)) = dec4_f32(codes, dtab);
        }
        __syncthreads();
        if (cg + 1 < KS) issue(cg + 1);   // in flight under the convolution below
#pragma unroll
        for (int j = 0; j < G::NO; ++j) {   // k_dwc's epilogue, then the pointwise layer's quantizer
            floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const int tap = j * G::RPI * S * ROWB + ((S == 1) ? (kh * ROWB + kw * 128) : (kh * ROWB + ((kw & 1) * 8 + (kw >> 1)) * 128));
                    const floatx4 a = *reinterpret_cast<const floatx4*>(tile + lds_r0 + tap);
                    const floatx4 w = wt[kh * 3 + kw];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] = fmaf(a[e], w[e], acc[e]);
                }
            }
            const float4 rr = dwpw_bn1(acc, psc, psh, p);
            uint2 q = enc4_f16_raw(rr, r2, lo2, hi2, tab2);
            if (__builtin_expect(enc_has_nan4(rr), 0)) {   // no ReLU in front: k_dwc gives a NaN the code 0x00, whose operand is the fp16 zero
                if (rr.x != rr.x) q.x &= 0xFFFF0000u;
                if (rr.y != rr.y) q.x &= 0x0000FFFFu;
                if (rr.z != rr.z) q.y &= 0xFFFF0000u;
                if (rr.w != rr.w) q.y &= 0x0000FFFFu;
            }
            dwpw_put_quad<G>(x16, d, j, cg, q);
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
    const int oh0 = th * TH, ow0 = tw * TW;
    // the tile epilogue of k_pwc_stream: channels j * 16 + kq * 4 .. + 3 of pixel `col` of unit ui
    auto tile_out = [&](int ui, int j) {
        const floatx4 acc = dwpw_mma<G>(wl, xh[ui], j, lane);
        const int nl = j * 16 + kq * 4;
        float4 r = epilogue(acc, *reinterpret_cast<const float4*>(ep + nl), p.s1x, p.s2);
        if (p.sc2) r = affine4(r, *reinterpret_cast<const float4*>(ep + NT * 16 + nl), *reinterpret_cast<const float4*>(ep + 2 * NT * 16 + nl));
        if constexpr (!YC) {   // with code output the ReLU is the quantizer's (code4)
            if (p.relu2) r = relu4(r);
        }
        return r;
    };
    if constexpr (YC) {
        const CodeQuant cq{p.encY.r1, p.encY.lo, p.encY.hi, p.relu2 ? 0 : 1, p.fmt_out};
        const __amdgpu_buffer_rsrc_t ry = dw_rsrc(reinterpret_cast<uint8_t*>(p.y) + (size_t)n * p.Ho * p.Wo * p.O, (uint32_t)p.Ho * p.Wo * p.O);
#pragma unroll
        for (int ui = 0; ui < UW; ++ui) {
            const int u = wv + NWV * ui;
            if (u < NU) {   // wave-uniform: every lane of the wave takes part in the transposes
                const int pix = u * 16 + col;
                const int oh = pix / TW, owp = pix - oh * TW;
                const bool live = pix < NPX && (oh0 + oh) < p.Ho && (ow0 + owp) < p.Wo;
                const uint32_t pixoff = (uint32_t)(((oh0 + oh) * p.Wo + ow0 + owp) * p.O);
#pragma unroll 1
                for (int j0 = 0; j0 < NT; j0 += 4) {
                    uint32_t c[4];
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) c[jj] = code4<false, false>(tile_out(ui, j0 + jj), cq, tabY);
                    rows_transpose4(c[0], c[1], c[2], c[3]);   // lane-quarter kq now holds channels 16 (j0 + kq) + 0..15 of its pixel
                    uint32_t so = live ? pixoff + (uint32_t)((j0 + kq) * 16) : kDwOob;
                    asm volatile("" : "+v"(so));
                    __builtin_amdgcn_raw_buffer_store_b128(u32x4{c[0], c[1], c[2], c[3]}, ry, so, 0, 0);
                }
            }
        }
    } else {
        const __amdgpu_buffer_rsrc_t ry = dw_rsrc(reinterpret_cast<float*>(p.y) + (size_t)n * p.Ho * p.Wo * p.O, (uint32_t)p.Ho * p.Wo * p.O * 4u);
        unsigned char* stg = tile + wv * 2048;   // [8 waves][2 KiB]: phase 2 reuses the (then idle) halo tile
        const int spx = lane >> 3, sch = lane & 7;
#pragma unroll 1
        for (int j0 = 0; j0 < NT; j0 += 2) {
#pragma unroll
            for (int ui = 0; ui < UW; ++ui) {
                const int u = wv + NWV * ui;
                if (u < NU) {   // wave-uniform
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj)
                        *reinterpret_cast<float4*>(stg + col * 128 + jj * 64 + kq * 16) = tile_out(ui, j0 + jj);
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
}

// ---------------------------------------------------------------------------- host
static size_t dwpw_codes_lds(int S, int KS, int NT) { return (size_t)kDecBytes + (size_t)2 * kDwTabBytes + dwpw_geom_bytes(S, KS, NT); }

// the reader's quantizer of a code-writing call (conv_abi.hip: consumer_quant_ok), and its table in the form the kernel carries
static const EncArgs* dwpw_codes_reader(const slfp_conv2d_io& io) {
    if ((io.y_qbits != 8 && io.y_qbits != 7) || !(io.y_ka > 0.f) || !scale_div_ok(io.y_ka)) return nullptr;
    const EncArgs* t = enc_table(io.y_ka, io.y_qbits == 7 ? kFmtSfp7 : kFmtAct8, kEncCode);
    return t->valid && enc_compact_covers(*t) ? t : nullptr;
}

// What slfp_dwpw_fwd_codes chooses among k_dwpw_codes' instances; slfp_dwpw_codes_supported is this function's answer.
bool dwpw_codes_select(const slfp_conv2d_desc* dw, const slfp_conv2d_desc* pw, const slfp_conv2d_io* io, int relu1, int relu2, DwPwSel* s) {
    if (!dw || !pw || !io) return false;
    if (io->x_codes != 1 || (io->y_codes != 0 && io->y_codes != 1)) return false;
    if ((relu1 & ~1) != 0 || (relu2 & ~1) != 0) return false;   // 0 / 1 only: no SLFP_POST_LAYEROUT
    if (!dwpw_select(dw, pw, s)) return false;   // geometry, a built (S, KS, NT), single-pass mode, tables in use (not the long form)
    ConvPlan p1, p2;
    if (make_plan(dw, &p1) != SLFP_OK || make_plan(pw, &p2) != SLFP_OK) return false;
    if (dw->y_layout != SLFP_LAYOUT_NHWC || pw->x_layout != SLFP_LAYOUT_NHWC) return false;
    if (!dwc_applicable(*dw, p1, nullptr, 0)) return false;
    const EncArgs* t2 = act_table(pw->ka, p2.fmt_act, kEncF16P);
    if (!t2 || !enc_compact_covers(*t2)) return false;
    if (io->y_codes && !dwpw_codes_reader(*io)) return false;
    if (dwpw_codes_lds(s->s, s->ks, s->nt) > 160 * 1024) return false;
    const int TH = dwpw_th(s->s);
    const int64_t nblocks = dw->n * ceil_div(p1.h_out, TH) * ceil_div(p1.w_out, TH);
    if (nblocks > 0x7FFFFFFF || dw->h * dw->w * dw->c_in >= (1ll << 29) || p1.h_out * p1.w_out * pw->c_out >= (1ll << 29)) return false;
    s->fmt_in = p1.fmt_act;
    s->yc = io->y_codes != 0;
    return true;
}

}  // namespace slfp

using namespace slfp;

extern "C" int slfp_dwpw_codes_supported(const slfp_conv2d_desc* dw, const slfp_conv2d_desc* pw, const slfp_conv2d_io* io,
                                         int has_bias_pw, int relu1, int relu2) {
    (void)has_bias_pw;   // a bias of the pointwise layer is the kernel's epilogue vector: every pair takes one
    DwPwSel sel;
    return dwpw_codes_select(dw, pw, io, relu1, relu2, &sel) ? 1 : 0;
}

// Host only: the instance slfp_dwpw_fwd (io == NULL) / slfp_dwpw_fwd_codes would run, printed from the selection they consume.
extern "C" const char* slfp_debug_dwpw_instance(const slfp_conv2d_desc* dw, const slfp_conv2d_desc* pw, const slfp_conv2d_io* io,
                                                int has_bias_pw, int relu1, int relu2) {
    (void)has_bias_pw;
    static thread_local char buf[64];
    DwPwSel s;
    if (!io) {
        if ((relu1 & ~1) != 0 || (relu2 & ~1) != 0 || !dwpw_select(dw, pw, &s)) return "none";
        snprintf(buf, sizeof buf, "f32/s%d/k%d/n%d", s.s, s.ks, s.nt);
        return buf;
    }
    if (!dwpw_codes_select(dw, pw, io, relu1, relu2, &s)) return "none";
    snprintf(buf, sizeof buf, "codes/s%d/k%d/n%d/%s/%s", s.s, s.ks, s.nt, s.fmt_in == kFmtSfp7 ? "sfp7" : "act8", s.yc ? "yc" : "f32");
    return buf;
}

template <int S, int KS, int NT>
static int launch_dwpw_codes(const DwPwCodesParams& p, bool sfp7, bool yc, size_t lds, hipStream_t st) {
    auto fn = sfp7 ? (yc ? k_dwpw_codes<S, KS, NT, kFmtSfp7, true> : k_dwpw_codes<S, KS, NT, kFmtSfp7, false>)
                   : (yc ? k_dwpw_codes<S, KS, NT, kFmtAct8, true> : k_dwpw_codes<S, KS, NT, kFmtAct8, false>);
    const int rc = raise_lds_limit(reinterpret_cast<const void*>(fn), lds);
    if (rc != SLFP_OK) return rc;
    hipLaunchKernelGGL(fn, dim3(p.nblocks), dim3(kDwPwT), lds, st, p);
    return check_launch("slfp fused depthwise + pointwise kernel (codes)");
}

extern "C" int slfp_dwpw_fwd_codes(const slfp_conv2d_desc* dw, const slfp_conv2d_desc* pw, const slfp_conv2d_io* io, const void* x,
                                   const void* wprep_dw, const float* post1_scale, const float* post1_shift, int relu1,
                                   const void* wprep_pw, const float* bias_pw, const float* post2_scale, const float* post2_shift,
                                   int relu2, void* y, void* stream) {
    if (!dw || !pw || !io) return fail(SLFP_ERR_BAD_ARG, "slfp_dwpw_fwd_codes: null descriptor");
    DwPwSel sel;
    if (!dwpw_codes_select(dw, pw, io, relu1, relu2, &sel))
        return fail(SLFP_ERR_UNSUPPORTED, "slfp_dwpw_fwd_codes: this pair of layers does not run as one kernel on codes (slfp_dwpw_codes_supported)");
    if (!x || !wprep_dw || !wprep_pw || !y || !post1_scale || !post1_shift)
        return fail(SLFP_ERR_BAD_ARG, "slfp_dwpw_fwd_codes: null pointer (the depthwise layer's folded BatchNorm is required)");
    if ((post2_scale == nullptr) != (post2_shift == nullptr)) return fail(SLFP_ERR_BAD_ARG, "slfp_dwpw_fwd_codes: post2_scale and post2_shift go together");
    if (!aligned16(x) || !aligned16(y) || !aligned16(wprep_dw) || !aligned16(wprep_pw) || !aligned16(post1_scale) || !aligned16(post1_shift) ||
        !aligned16(bias_pw) || !aligned16(post2_scale) || !aligned16(post2_shift))
        return fail(SLFP_ERR_ALIGNMENT, "slfp_dwpw_fwd_codes: pointers must be 16-byte aligned");
    ConvPlan p1, p2;
    make_plan(dw, &p1);
    make_plan(pw, &p2);
    const int S = sel.s, ks = sel.ks, nt = sel.nt;
    DwPwCodesParams p;
    dwpw_fill_base(p, dw, pw, p1, p2, x, wprep_dw, post1_scale, post1_shift, relu1, wprep_pw, bias_pw, post2_scale, post2_shift, relu2, y);
    p.fmt_out = io->y_qbits == 7 ? kFmtSfp7 : kFmtAct8;
    p.enc2 = enc_compact(*act_table(pw->ka, p2.fmt_act, kEncF16P));
    p.encY = io->y_codes ? enc_compact(*dwpw_codes_reader(*io)) : p.enc2;   // float32 out: not read
    static_assert(sizeof(DwPwCodesParams) <= 4096, "kernel arguments must fit the 4 KiB kernarg segment");
    const size_t lds = dwpw_codes_lds(S, ks, nt);
    const bool sfp7 = sel.fmt_in == kFmtSfp7, yc = sel.yc;
    hipStream_t st = as_stream(stream);
#define SLFP_FC(SS, KK, NN) \
    if (S == SS && ks == KK && nt == NN) return launch_dwpw_codes<SS, KK, NN>(p, sfp7, yc, lds, st);
    SLFP_DWPW_INSTANCES(SLFP_FC)
#undef SLFP_FC
    return fail(SLFP_ERR_UNSUPPORTED, "slfp_dwpw_fwd_codes: no instantiation for this shape");   // not reached: dwpw_select admits SLFP_DWPW_INSTANCES only
}
