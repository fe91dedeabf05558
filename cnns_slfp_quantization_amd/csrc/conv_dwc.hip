// conv_dwc.hip -- SLFP-quantized depthwise 3x3 convolution on 1-byte activation codes, NHWC, gfx950.
//
// The depthwise 3x3 layers, stride 1 / 2 (the 13 "dw" layers of MobileNetV1, nets_imgnet/mobilenetv1.py:27), INSIDE a chain of
// quantized convolutions (csrc/slfp_codes.hpp): the input arrives as the codes the previous layer's epilogue wrote (QA(x / Ka) is
// already applied), the output leaves as the codes of the NEXT layer's QA(. / Ka_next), or as float32 at the end of the chain.
// The arithmetic is the family's (include/slfp.h, next to slfp_debug_dw3x3_instance; shared steps: conv_dw_core.hpp) over the decoded
// values: outputs are bit-identical to the float32-interface kernel fed with the decoded tensor.
//
// Structure: no LDS tile, no barrier after the prologue.  At 1 B per element a pixel's channels are too few bytes for the
// (pixel slot, 32-channel group) lanes of conv_dw2.hip (32-byte pieces), so here a lane owns 4 channels of ONE output
// column and walks down TH output rows with a 3-row x 3-column window of decoded values in registers:
//   * lanes of a wave = (consecutive output columns) x (up to 128 consecutive channels): every load / store instruction
//     of a wave covers whole 128-byte lines (C >= 128) or one contiguous 256-byte run (C = 32, 64);
//   * all (TH-1)*S+3 rows x 3 columns of a lane's input codes (27 dwords) are requested back to back through a buffer
//     descriptor (out-of-image taps: out-of-range offset, the returned 0 is replaced by the exact-zero code 0x01), and
//     consumed row by row under counted vmcnt waits while the later rows are still in flight;
//   * decode = 1 VALU + 1 LDS lookup per element (256-entry table), encode = 5 VALU + 1 LDS (slfp_codes.hpp).
// The 3 columns of a lane overlap its neighbours' (they hit the same lines in L1); the redundancy is in decode
// instructions, not in HBM bytes.
#include "slfp_codes.hpp"
#include "slfp_layerout_lut.hpp"
#include "conv_dw_core.hpp"

namespace slfp {

constexpr int kDwcThreads = 256;

struct DwcParams {
    int N, H, W, C, Ho, Wo, pad;
    int cgs;              // channel groups of LC * 4 channels
    int row_tiles;        // ceil(Ho / TH)
    int col_tiles;        // ceil(Wo / TW)
    uint32_t ntasks;      // N * row_tiles * col_tiles * cgs
    uint32_t nblocks;
    int fmt_in;           // kFmtAct8 | kFmtSfp7: what the input codes are
    int fmt_out;          // the same for the output codes (YC)
    float ka, kw;
    int relu;
    const float* post_scale;
    const float* post_shift;
    EncArgs enc;          // YC: code table of the consumer's Ka (kEncCode)
};

// S: stride; LCS: log2(lanes across channels) = 3 / 4 / 5 for C = 32 / 64 / >= 128; TH x TW: output rows x columns per lane;
// YC: output as codes (else float32); POST: fused per-channel scale / shift; SIGNED: no ReLU before the output quantizer.
// LUTQ (YC, POST; slfp_conv2d_fwd_codes_lut): the code is the byte table's entry for the layer-output class of the affine's
// result (slfp_layerout_lut.hpp); the table (4.8 KiB) takes the place of the reader's threshold table in LDS -- the kernel
// keeps 1 KiB besides it, and a lookup is one ds_read_u8 next to the decode lookups it already issues.
// VALU-issue-bound (profiles/r03c*): what is counted is instructions per output element.  A lane's TW adjacent columns
// share TW + 2 decoded input columns; row / column validity is one select each on the row and the column part of the offset.
template <int S, int LCS, int TH, int TW, bool YC, bool POST, bool SIGNED, bool LUTQ = false>
__global__ __launch_bounds__(kDwcThreads) void k_dwc(const uint8_t* __restrict__ x, const float* __restrict__ wq,
                                                     void* __restrict__ y, const DwcParams p) {
    constexpr int LC = 1 << LCS;
    constexpr int NR = (TH - 1) * S + 3, NC = (TW - 1) * S + 3;
    static_assert(!LUTQ || (YC && POST && SIGNED), "the table epilogue writes codes behind an affine; the ReLU lies in the table");
    __shared__ __attribute__((aligned(16))) unsigned char senc[LUTQ ? kLayeroutLutBytes : (YC ? kDwTabBytes : 16)];
    __shared__ __attribute__((aligned(16))) uint32_t sdec[256];
    if constexpr (LUTQ) layerout_lut_fill<kDwcThreads>(senc, enc_carried_ptr(p.enc));
    else if constexpr (YC) enc_fill<kDwcThreads>(reinterpret_cast<uint2*>(senc), p.enc);
    if (p.fmt_in == kFmtSfp7) dec_fill<kFmtSfp7, kDecF32, kDwcThreads>(sdec);
    else dec_fill<kFmtAct8, kDecF32, kDwcThreads>(sdec);
    const unsigned char* dtab = reinterpret_cast<const unsigned char*>(sdec);

    const uint32_t b = xcd_remap(blockIdx.x, p.nblocks);
    uint32_t t = b * (kDwcThreads / LC) + (threadIdx.x >> LCS);
    const bool valid = t < p.ntasks;
    t = valid ? t : p.ntasks - 1;
    const int cg = (int)(t % (uint32_t)p.cgs); t /= (uint32_t)p.cgs;
    const int ow0 = (int)(t % (uint32_t)p.col_tiles) * TW; t /= (uint32_t)p.col_tiles;
    const int rt = (int)(t % (uint32_t)p.row_tiles);
    const int n = (int)(t / (uint32_t)p.row_tiles);
    const int c = (cg * LC + (threadIdx.x & (LC - 1))) * 4;

    // ---- every input dword of this lane, back to back
    uint32_t raw[NR][NC];
    {
        const uint32_t in_bytes = (uint32_t)p.N * p.H * p.W * p.C;
        const __amdgpu_buffer_rsrc_t rs = dw_rsrc(x, in_bytes);
        const int ih0 = rt * TH * S - p.pad, iw0 = ow0 * S - p.pad;
        const uint32_t rowb = (uint32_t)(n * p.H + ih0) * (uint32_t)(p.W * p.C) + (uint32_t)c;   // wraps for negative rows: only used in range
        const uint32_t rstep = (uint32_t)(p.W * p.C);
        uint32_t roff[NR], coff[NC];
        bool rok[NR], cok[NC];
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            rok[j] = valid && (unsigned)(ih0 + j) < (unsigned)p.H;
            roff[j] = rok[j] ? rowb + (uint32_t)j * rstep : kDwBadRow;
        }
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            cok[k] = (unsigned)(iw0 + k) < (unsigned)p.W;
            coff[k] = cok[k] ? (uint32_t)((iw0 + k) * p.C) : kDwBadCol;
        }
#pragma unroll
        for (int j = 0; j < NR; ++j)
#pragma unroll
            for (int k = 0; k < NC; ++k) raw[j][k] = __builtin_amdgcn_raw_buffer_load_b32(rs, roff[j] + coff[k], 0, 0);
#pragma unroll
        for (int j = 0; j < NR; ++j)
#pragma unroll
            for (int k = 0; k < NC; ++k) raw[j][k] = (rok[j] && cok[k]) ? raw[j][k] : 0x01010101u;   // zero padding = the exact-zero code
    }

    // this lane's 4 channels x 9 taps, fused BN vectors
    f32x4 wt[9], psc, psh;
    dw_load_taps(wt, wq, (uint32_t)p.C, c);
    dw_load_bn<POST>(psc, psh, p.post_scale, p.post_shift, c);
    __syncthreads();   // tables visible

    const uint32_t out_bytes = (uint32_t)p.N * p.Ho * p.Wo * p.C * (YC ? 1u : 4u);
    const __amdgpu_buffer_rsrc_t ry = dw_rsrc(y, out_bytes);
    const int oh0 = rt * TH;
    const uint32_t ostep = (uint32_t)(p.Wo * p.C) * (YC ? 1u : 4u);
    uint32_t ocol[TW];
#pragma unroll
    for (int q = 0; q < TW; ++q)
        ocol[q] = (valid && ow0 + q < p.Wo) ? (((uint32_t)(n * p.Ho + oh0) * (uint32_t)p.Wo + (uint32_t)(ow0 + q)) * (uint32_t)p.C + (uint32_t)c) * (YC ? 1u : 4u)
                                            : kDwBadRow;
    const float r1 = p.enc.r1, lo = p.enc.lo, hi = p.enc.hi;

    float4 win[3][NC];   // ring of decoded input rows: row j lives in slot j % 3
#pragma unroll
    for (int j = 0; j < 3 - S; ++j)
#pragma unroll
        for (int k = 0; k < NC; ++k) win[j][k] = dec4_f32(raw[j][k], dtab);
#pragma unroll
    for (int r = 0; r < TH; ++r) {
#pragma unroll
        for (int j = r * S + 3 - S; j < r * S + 3; ++j)   // the S rows this step adds
#pragma unroll
            for (int k = 0; k < NC; ++k) win[j % 3][k] = dec4_f32(raw[j][k], dtab);
        const uint32_t orow = (oh0 + r) < p.Ho ? (uint32_t)r * ostep : kDwBadCol;
#pragma unroll
        for (int q = 0; q < TW; ++q) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const float4 a = win[(r * S + kh) % 3][q * S + kw];
                    const f32x4 w = wt[kh * 3 + kw];
                    acc[0] = fmaf(a.x, w[0], acc[0]); acc[1] = fmaf(a.y, w[1], acc[1]);
                    acc[2] = fmaf(a.z, w[2], acc[2]); acc[3] = fmaf(a.w, w[3], acc[3]);
                }
            }
            // no ReLU here: with code output it is the quantizer's (or the table's); the float32 form keeps its branch around four max below
            f32x4 rr = dw_finish<POST>(acc, p.ka, p.kw, psc, psh, 0);
            const uint32_t so = ocol[q] + orow;
            if constexpr (YC) {
                uint32_t code;
                if constexpr (LUTQ) {
                    code = lut4_code(make_float4(rr[0], rr[1], rr[2], rr[3]), senc);
                } else if constexpr (SIGNED) {
                    code = enc4_code<true>(make_float4(rr[0], rr[1], rr[2], rr[3]), r1, lo, hi, senc);
                    if (p.fmt_out == kFmtSfp7) code = (code & 0x3F3F3F3Fu) | ((code & 0x80808080u) >> 1);
                } else {
                    // the ReLU is the quantizer's: a negative value selects the lowest bin and fails its compare = the zero code;
                    // a NaN takes that code too (the float32 form's fmaxf(NaN, 0) == 0), on the encoder's cold branch (NANZERO)
                    code = enc4_code_relu<true>(make_float4(rr[0], rr[1], rr[2], rr[3]), r1, lo, hi, senc);
                }
                __builtin_amdgcn_raw_buffer_store_b32(code, ry, so, 0, 0);
            } else {
                if (p.relu) { rr[0] = fmaxf(rr[0], 0.f); rr[1] = fmaxf(rr[1], 0.f); rr[2] = fmaxf(rr[2], 0.f); rr[3] = fmaxf(rr[3], 0.f); }
                dw_store16(rr, ry, so, 0);
            }
        }
    }
}

bool dwc_applicable(const slfp_conv2d_desc& d, const ConvPlan& plan, const float* bias, int post_flags) {
    if (bias || plan.family != kDw3x3 || plan.repad) return false;
    if (d.c_in % 32 != 0 || (post_flags & SLFP_POST_LAYEROUT)) return false;
    if (d.c_in > 64 && d.c_in % 128 != 0) return false;
    if (d.pad_h > 2 || d.pad_h != d.pad_w) return false;
    const uint64_t in_b = (uint64_t)d.n * d.h * d.w * d.c_in, out_b = (uint64_t)d.n * plan.h_out * plan.w_out * d.c_in * 4;
    return in_b < (1ull << 30) && out_b < (1ull << 30);   // offsets: bit 30 / 31 mark an invalid column / row
}

// What launch_dwc chooses among k_dwc's instances (and the one runtime format word).  dwc_instance maps it to the kernel: the
// launcher launches that pointer and dwc_instance_name (slfp_debug_dw3x3_instance) asks for it before it prints.
struct DwcSel {
    int s;          // S; TH x TW = 7 x 2 (stride 1) / 4 x 1 (stride 2) follow from it
    int lcs;        // LCS
    bool yc, post, sgn, lut;   // YC, POST, SIGNED, LUTQ
    int fmt_in;     // DwcParams::fmt_in (not a template argument: the decode table is filled by it)
};

static int dwc_select(const slfp_conv2d_desc& d, const ConvPlan& plan, const PostOp& post, const CodeIo& io, DwcSel* s) {
    s->s = d.stride_h == 2 ? 2 : 1;
    s->lcs = d.c_in >= 128 ? 5 : (d.c_in == 64 ? 4 : 3);
    s->lut = io.lut != nullptr;
    if (s->lut && (!io.y_codes || !post.scale))
        return fail(SLFP_ERR_BAD_ARG, "dw3x3 (codes): the table epilogue needs code output and post_scale / post_shift");
    s->yc = io.y_codes;
    s->post = post.scale != nullptr;
    s->sgn = s->lut || (s->yc && !post.relu);   // float32 output: the ReLU is a runtime flag of the SIGNED = false instance
    s->fmt_in = plan.fmt_act;
    return SLFP_OK;
}

typedef void (*DwcFn)(const uint8_t*, const float*, void*, const DwcParams);
// the 7 output forms of one (S, LCS) geometry: the table epilogue; codes with / without BatchNorm, signed / ReLU-folded; float32
template <int S, int LCS, int TH, int TW>
static DwcFn dwc_instance_form(const DwcSel& s) {
    if (s.lut) return (s.yc && s.post && s.sgn) ? k_dwc<S, LCS, TH, TW, true, true, true, true> : nullptr;
    if (!s.yc) return s.sgn ? nullptr : (s.post ? k_dwc<S, LCS, TH, TW, false, true, false> : k_dwc<S, LCS, TH, TW, false, false, false>);
    if (s.post) return s.sgn ? k_dwc<S, LCS, TH, TW, true, true, true> : k_dwc<S, LCS, TH, TW, true, true, false>;
    return s.sgn ? k_dwc<S, LCS, TH, TW, true, false, true> : k_dwc<S, LCS, TH, TW, true, false, false>;
}
static DwcFn dwc_instance(const DwcSel& s) {
    switch (s.s * 10 + s.lcs) {   // TH x TW = 7 x 2 (stride 1) / 4 x 1 (stride 2), as launch_dwc's tile counts
        case 13: return dwc_instance_form<1, 3, 7, 2>(s);
        case 14: return dwc_instance_form<1, 4, 7, 2>(s);
        case 15: return dwc_instance_form<1, 5, 7, 2>(s);
        case 23: return dwc_instance_form<2, 3, 4, 1>(s);
        case 24: return dwc_instance_form<2, 4, 4, 1>(s);
        case 25: return dwc_instance_form<2, 5, 4, 1>(s);
        default: return nullptr;
    }
}

static const char* dwc_sel_name(const DwcSel& s) {
    static thread_local char buf[64];
    snprintf(buf, sizeof buf, "dwc/s%d/lc%d/%s/%s/%s", s.s, s.lcs, s.lut ? "lut" : (!s.yc ? "f32" : (s.sgn ? "yc-signed" : "yc")),
             s.post ? "post" : "plain", s.fmt_in == kFmtSfp7 ? "sfp7" : "act8");
    return buf;
}

const char* dwc_instance_name(const slfp_conv2d_desc& d, const ConvPlan& plan, const PostOp& post, const CodeIo& io) {
    DwcSel s;
    if (plan.family != kDw3x3 || dwc_select(d, plan, post, io, &s) != SLFP_OK || !dwc_instance(s)) return "none";
    return dwc_sel_name(s);
}

// io.y_codes: output codes for a consumer with scale io.y_ka and format io.y_fmt (kFmtAct8 | kFmtSfp7); else float32
int launch_dwc(const slfp_conv2d_desc& d, const ConvPlan& plan, const uint8_t* x, const float* wq9c, const PostOp& post,
               void* y, const CodeIo& io, hipStream_t stream) {
    DwcSel sel;
    const int src = dwc_select(d, plan, post, io, &sel);
    if (src != SLFP_OK) return src;
    DwcParams p;
    dw_fill_geom(p, d, plan);
    p.cgs = p.C / (4 << sel.lcs);
    p.row_tiles = (int)ceil_div(p.Ho, sel.s == 2 ? 4 : 7);
    p.col_tiles = (int)ceil_div(p.Wo, sel.s == 2 ? 1 : 2);
    const int64_t ntasks = (int64_t)p.N * p.row_tiles * p.col_tiles * p.cgs;
    if (const int rc = dw_grid_check(ntasks, "dw3x3 (codes)")) return rc;
    p.ntasks = (uint32_t)ntasks;
    p.nblocks = (uint32_t)ceil_div(ntasks, kDwcThreads >> sel.lcs);
    p.fmt_in = sel.fmt_in;
    p.fmt_out = io.y_fmt;
    p.relu = post.relu;
    p.post_scale = post.scale; p.post_shift = post.shift;
    p.enc.valid = 0;
    if (sel.lut) {
        enc_carry_ptr(p.enc, io.lut);
    } else if (sel.yc) {
        const EncArgs* t = enc_table(io.y_ka, io.y_fmt, kEncCode);
        if (!t->valid) return fail(SLFP_ERR_UNSUPPORTED, "dw3x3 (codes): no code table for the consumer's scale %g", (double)io.y_ka);
        p.enc = *t;
    }
    return dw_launch(dwc_instance(sel), "dw3x3 (codes)", dwc_sel_name(sel), p.nblocks, kDwcThreads, 0, stream, "slfp dw3x3 (codes) kernel",
                     x, wq9c, y, p);
}

}  // namespace slfp
