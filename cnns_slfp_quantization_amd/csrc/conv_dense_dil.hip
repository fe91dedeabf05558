// conv_dense_dil.hip -- SLFP-quantized DILATED dense k x k convolution (groups 1, stride 1) on the gfx950 matrix cores:
// the 3x3 dilation-2 / dilation-4 layers of an output-stride-8 ResNet-50 (replace_stride_with_dilation), DeepLab / DRN heads.
//
// Phase decomposition, not a wider halo.  At stride 1 the output pixel (oh, ow) with oh = rh + dil_h * i, ow = rw + dil_w * j
// reads the input pixels (rh - pad_h + dil_h * (i + kh), rw - pad_w + dil_w * (j + kw)): one residue class per axis.  The layer
// is dil_h * dil_w independent UNDILATED convolutions on sub-sampled images ("phases"), and a phase is exactly the problem
// k_dense_mfma (conv_dense.hip) solves at stride 1:
//   * a workgroup owns one image, one phase (rh, rw), one TH x TW tile of phase-grid pixels (i, j) and BN output channels;
//   * in phase-grid coordinates its halo is (TH + KH - 1) x (TW + KW - 1) pixels whatever the dilation: the same 128-byte
//     pixel rows, the same dn_x_off swizzle, the same tap loop over shifted 16-pixel fragments.  Only the SOURCE addresses of
//     the 1 KiB LDS-DMA pieces know about the dilation: they step dil_w pixels along a halo row and dil_h rows between halo
//     rows; conv padding and out-of-image pixels come from the zero page;
//   * operands are the dense family's: k_dense_encode's fp16 NHWC copy (launch_dense_encode) and the dense weight blob
//     [tap][n_tile][k_step][64][8]; the next chunk's halo arrives behind the current taps' MFMAs, weight tiles are
//     double-buffered by LDS-DMA, one barrier per tap (k_dense_mfma's pipeline with two weight buffers);
//   * the epilogue (slfp_epilogue.hpp) stores 4 consecutive channels of pixel (rh + dil_h * i, rw + dil_w * j).
// Phase grids are narrow (28 / 4 = 7 columns): the 16 pixels of an MFMA fragment are FR rows x 16 / FR columns, FR = 1
// (16 x 1) or 2 (8 x 2: lanes 0-7 read one halo row, lanes 8-15 the next), and TW = 16 / FR.  dil_select picks per layer the
// fragment shape and the (WM, WN, MT) tiling that pad the phase grid least; dense_dil_variant_name prints that selection.
// Single-pass fp16 (SLFP<3,4>) or exact (SFP<3,3>); float32 in, float32 out.  Opt-in: SLFP_DESC_DILATED_MFMA (include/slfp.h).
#include <algorithm>
#include "slfp_device.hpp"
#include "slfp_host.hpp"
#include "slfp_epilogue.hpp"
#include "conv_dense_core.hpp"

namespace slfp {

constexpr int kDilThreads = 512;
constexpr int kDilMaxSlots = 9;   // halo pieces a wave stages per chunk = ceil(x_pieces / 8); dil_geometry enforces it

struct DilParams {
    const _Float16* xe;              // pre-encoded input, NHWC with C padded to Cp (k_dense_encode)
    const unsigned char* zero_page;  // 256 zero bytes: DMA source of padding pixels
    const _Float16* w;               // [tap][n_tile][k_step][64 lanes][8]
    const float* bias;
    float* y;
    int N, H, W, Cp, O, KH, KW, dh, dw, ph, pw, Ho, Wo;
    int phases_h, phases_w;          // min(dil, output size): phases that own at least one output pixel
    int tiles_h, tiles_w, n_blocks;  // tiles of the LARGEST phase grid (ceil(Ho / dh) x ceil(Wo / dw)); channel slices
    int IW, n_pix;                   // halo tile: pitch TW + KW - 1, pixels
    int KS, n_tiles;                 // 32-deep k-steps per tap (even); 16-channel tiles in the blob
    int x_pieces, x_per_tap;         // 1 KiB pieces per chunk; pieces slots a wave issues per tap
    float s1x, s1, s2;
    PostOp post;
    uint32_t nblocks;
};

// WM x WN = 8 waves; a wave owns MT fragments (rows of FR phase-grid rows each) x 64 output channels.
// FR: phase-grid rows per 16-pixel fragment.  NSLOT: halo pieces a wave stages per chunk (3 covers the 3x3 tilings).
// Two workgroups per CU (128 registers) except MT = 2 with nine slots, which spills there and whose halo fills LDS past 80 KiB anyway.
template <int WM, int WN, int MT, int FR, int NSLOT>
__global__ __launch_bounds__(kDilThreads, (MT == 2 && NSLOT > 3 ? 2 : 4)) void k_dense_dil(const DilParams p) {
    static_assert(WM * WN == 8, "8 waves");
    static_assert(FR == 1 || FR == 2, "16 x 1 or 8 x 2 fragments");
    constexpr int TW = 16 / FR, TH = WM * MT * FR, BN = WN * 64, WT = BN * 128;   // WT: bytes of one tap's weight tile
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* wbuf = smem;            // [2 buffers][WT]
    unsigned char* xsb = wbuf + 2 * WT;    // [2 buffers][x_pieces * 1 KiB]   (8 halo pixels x 128 B per piece)
    const uint32_t xbytes = (uint32_t)p.x_pieces * 1024u;

    uint32_t b = xcd_remap(blockIdx.x, p.nblocks);   // channel slice slowest: an XCD's L2 holds one W slice
    const int tw = b % p.tiles_w; b /= p.tiles_w;
    const int th = b % p.tiles_h; b /= p.tiles_h;
    const int rw = b % p.phases_w; b /= p.phases_w;
    const int rh = b % p.phases_h; b /= p.phases_h;
    const int n = b % p.N;
    const int nb = b / p.N;
    const int i0 = th * TH, j0 = tw * TW;            // first phase-grid pixel of the tile
    // phases shorter than the largest one: a tile past this phase's grid has nothing to store (whole workgroup)
    if (rh + p.dh * i0 >= p.Ho || rw + p.dw * j0 >= p.Wo) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int col = lane & 15, kq = lane >> 4;
    const int h_in0 = rh - p.ph + p.dh * i0, w_in0 = rw - p.pw + p.dw * j0;   // input pixel of halo pixel (0, 0)

    // ---- halo tile: piece q of a chunk = 8 consecutive halo pixels x 64 channels (fp16), one DMA; lane -> (pixel
    // pc*8 + lane/8, LDS slot lane%8), the slot holding 16-byte chunk slot ^ swz(pixel) (dn_x_off).  Halo pixel (a, c) is
    // input pixel (h_in0 + dh * a, w_in0 + dw * c): the one place the dilation enters.  Worked out once, before the loops.
    const unsigned char* xen = reinterpret_cast<const unsigned char*>(p.xe) + (size_t)n * p.H * p.W * p.Cp * 2;
    const unsigned char* zp = p.zero_page + (lane & 7) * 16;
    constexpr uint32_t kPad = 0xFFFFFFFFu;
    uint32_t xoff[NSLOT];   // chunk-0 byte offset (from xen) of this lane's 16 bytes of piece slot j; kPad = zero page
#pragma unroll
    for (int j = 0; j < NSLOT; ++j) {
        const int pc = wave + 8 * j;
        const int pix = pc * 8 + (lane >> 3);
        const int a = pix / p.IW, c = pix - a * p.IW;
        const int gh = h_in0 + p.dh * a, gw = w_in0 + p.dw * c;
        const int c16 = (lane & 7) ^ (((pix >> 1) & 3) << 1);
        const bool inb = pc < p.x_pieces && pix < p.n_pix && (unsigned)gh < (unsigned)p.H && (unsigned)gw < (unsigned)p.W;
        xoff[j] = inb ? (uint32_t)((gh * p.W + gw) * p.Cp) * 2u + (uint32_t)c16 * 16u : kPad;   // < 2^31 (dense_dil_applicable)
    }
    auto stage_x = [&](int j, int chunk, int buf) {   // piece slot j (compile-time after unrolling) of this wave
        const int pc = wave + 8 * j;
        const unsigned char* src = xoff[j] != kPad ? xen + (xoff[j] + (uint32_t)chunk * 128u) : zp;   // Cp: whole chunks
        glds16(src, xsb + (size_t)buf * xbytes + (size_t)pc * 1024);
    };

    // ---- weight tap tile: BN/8 pieces of 1 KiB (channel tile, k-step), WN per wave
    const int nt0 = nb * (BN / 16);
    const unsigned char* wsrc[WN];
#pragma unroll
    for (int j = 0; j < WN; ++j) {
        const int pc = wave * WN + j;                     // piece = (channel tile pc >> 1, k-step pc & 1)
        int nt = nt0 + (pc >> 1);
        nt = nt < p.n_tiles ? nt : p.n_tiles - 1;         // tiles past C_out: clamp (results never stored)
        wsrc[j] = reinterpret_cast<const unsigned char*>(p.w) + ((size_t)nt * p.KS + (pc & 1)) * 1024 + (size_t)lane * 16;
    }
    const size_t w_tap_stride = (size_t)p.n_tiles * p.KS * 1024;
    auto stage_w = [&](int tap, int chunk, int buf) {
        const size_t o = (size_t)tap * w_tap_stride + (size_t)chunk * 2048;   // wave-uniform
#pragma unroll
        for (int j = 0; j < WN; ++j) glds16(wsrc[j] + o, wbuf + (size_t)buf * WT + (size_t)(wave * WN + j) * 1024);
    };

    // this lane's pixel of fragment i: phase-grid row fr[i] (inside the tile), column fc; its halo pixel at tap (0, 0)
    const int fc = FR == 2 ? (col & 7) : col;
    int fr[MT], fpix[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        fr[i] = (wm * MT + i) * FR + (FR == 2 ? (col >> 3) : 0);
        fpix[i] = fr[i] * p.IW + fc;
    }

    floatx4 acc[MT][4];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

    const int n_chunks = p.KS >> 1, n_taps = p.KH * p.KW;   // n_taps >= 2 (dense_dil_applicable)
    stage_w(0, 0, 0);
    stage_w(1, 0, 1);
#pragma unroll
    for (int j = 0; j < NSLOT; ++j)
        if (wave + 8 * j < p.x_pieces) stage_x(j, 0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // Per tap (k_dense_mfma's order): (1) this tap's fragments LDS -> registers; (2) barrier: every wave has read wbuf[wb], and
    // the DMAs issued one tap ago have landed (explicit vmcnt(0): hipcc does not count a global_load_lds of the previous
    // iteration when it lowers __syncthreads()); (3) the DMA for tap + 2 goes into the buffer just freed, plus a slice of the
    // next chunk's halo; (4) the MFMAs run from registers while those DMAs fly.
    int wb = 0, xb = 0;
    for (int chunk = 0; chunk < n_chunks; ++chunk) {
        const bool more_chunks = chunk + 1 < n_chunks;
        const unsigned char* xs = xsb + (size_t)xb * xbytes;
        for (int tap = 0; tap < n_taps; ++tap) {
            const int kh = tap / p.KW, kw = tap - kh * p.KW;
            const int tpix = kh * p.IW + kw;
            const unsigned char* wt = wbuf + (size_t)wb * WT + (size_t)(wn * 4) * 2048 + lane * 16;
            half8 wf[2][4], xf[2][MT];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
                for (int j = 0; j < 4; ++j) wf[ks][j] = *reinterpret_cast<const half8*>(wt + j * 2048 + ks * 1024);
#pragma unroll
                for (int i = 0; i < MT; ++i) xf[ks][i] = *reinterpret_cast<const half8*>(xs + dn_x_off(fpix[i] + tpix, ks * 4 + kq));
            }
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            // a slice of the next chunk's halo; nothing on the last tap: its DMA would still be in flight when the next
            // chunk's first fragments are read
            if (more_chunks && tap + 1 < n_taps) {
#pragma unroll
                for (int j = 0; j < NSLOT; ++j) {   // slot j goes out with tap j / x_per_tap (wave-uniform)
                    if (j / p.x_per_tap == tap && wave + 8 * j < p.x_pieces) stage_x(j, chunk + 1, xb ^ 1);
                }
            }
            // the weight tile two taps ahead -> the buffer every wave has just finished reading
            int tap2 = tap + 2, chunk2 = chunk;
            while (tap2 >= n_taps) { tap2 -= n_taps; ++chunk2; }
            if (chunk2 < n_chunks) stage_w(tap2, chunk2, wb);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[ks][j], xf[ks][i], acc[i][j], 0, 0, 0);
            wb ^= 1;
        }
        xb ^= 1;
    }

    // ---- epilogue: (acc * Ka) * Kw with the reference's roundings, bias, post-op; a lane holds 4 consecutive channels of its
    // pixel (rh + dh * (i0 + fr), rw + dw * (j0 + fc)): the channel run of a pixel stays contiguous, pixels scatter by the phase
    const int ow = rw + p.dw * (j0 + fc);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ch = (nt0 + wn * 4 + j) * 16 + kq * 4;
        if (ch >= p.O) continue;
        const float4 bq = bias_q256(p.bias, ch, p.s1, p.s2);
        const PostVec pv = post_load(p.post, ch);
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int oh = rh + p.dh * (i0 + fr[i]);
            if (oh >= p.Ho || ow >= p.Wo) continue;
            const float4 r = epilogue(acc[i][j], bq, p.s1x, p.s2);
            st_stream4<SLFP_NT_DENSE>(p.y + (((size_t)n * p.Ho + oh) * p.Wo + ow) * p.O + ch, post_apply_v(r, p.post, pv));
        }
    }
}

// ---- host side: one selection (dil_select) behind the plan, the launch and the debug name -------------------------------
struct DilCfg { int wm, wn, mt; };
// instantiated (rows-per-wave, channel-slice) tilings, widest first; each with FR = 1 and FR = 2
static const DilCfg kDilCfgs[] = {{4, 2, 2}, {4, 2, 1}, {8, 1, 1}};

struct DilSel {
    DilCfg cfg;
    int fr;                 // phase-grid rows per fragment: 1 (16 x 1) or 2 (8 x 2)
    int th, tw;             // tile of phase-grid pixels
    int iw, n_pix, pieces, per_tap, nslot;
    size_t lds;
};

static bool dil_geometry(const slfp_conv2d_desc& d, const DilCfg& c, int fr, DilSel* s) {
    const int taps = (int)(d.kh * d.kw);
    s->cfg = c; s->fr = fr;
    s->th = c.wm * c.mt * fr; s->tw = 16 / fr;
    s->iw = s->tw + (int)d.kw - 1;
    s->n_pix = (s->th + (int)d.kh - 1) * s->iw;
    s->pieces = (s->n_pix + 7) / 8;
    const int slots = (int)ceil_div(s->pieces, 8);
    s->per_tap = (int)ceil_div(slots, taps - 1);   // all slices issued before the last tap
    s->nslot = slots <= 3 ? 3 : kDilMaxSlots;
    s->lds = 2 * (size_t)c.wn * 64 * 128 + 2 * (size_t)s->pieces * 1024;
    return s->lds <= 160 * 1024 && slots <= kDilMaxSlots;
}

// The (fragment shape, tiling) that pads the phase grid least: padded MACs of the launch = phases x padded phase-grid pixels
// x padded channels; among equals the one that stages the fewest halo pixels, then the earlier in the list (wider tiles).
static bool dil_select(const slfp_conv2d_desc& d, int64_t h_out, int64_t w_out, DilSel* best) {
    const int64_t gh = ceil_div(h_out, d.dil_h), gw = ceil_div(w_out, d.dil_w);   // the largest phase grid
    int64_t best_macs = 0, best_halo = 0;
    bool found = false;
    for (int fr = 1; fr <= 2; ++fr)
        for (const DilCfg& c : kDilCfgs) {
            DilSel s;
            if (!dil_geometry(d, c, fr, &s)) continue;
            const int64_t tiles = ceil_div(gh, s.th) * ceil_div(gw, s.tw), slices = ceil_div(d.c_out, c.wn * 64);
            const int64_t macs = tiles * s.th * s.tw * slices * c.wn * 64, halo = tiles * slices * s.n_pix;
            if (!found || macs < best_macs || (macs == best_macs && halo < best_halo)) { best_macs = macs; best_halo = halo; *best = s; found = true; }
        }
    return found;
}

bool dense_dil_applicable(const slfp_conv2d_desc& d, int passes) {
    if (d.groups != 1 || d.kh * d.kw <= 1 || (d.dil_h == 1 && d.dil_w == 1)) return false;
    if (d.stride_h != 1 || d.stride_w != 1 || passes != 1) return false;
    if (d.c_in % 4 || d.c_in < 16 || d.c_out % 4) return false;
    if ((int64_t)d.h * d.w * (d.c_in + 63) >= (1ll << 30)) return false;   // 32-bit byte offsets inside one image of the fp16 copy
    const int64_t eh = d.h + 2 * (int64_t)d.pad_h - (int64_t)d.dil_h * (d.kh - 1), ew = d.w + 2 * (int64_t)d.pad_w - (int64_t)d.dil_w * (d.kw - 1);
    if (eh <= 0 || ew <= 0) return false;
    DilSel s;
    return dil_select(d, eh, ew, &s);
}

const char* dense_dil_variant_name(const slfp_conv2d_desc& d, const ConvPlan& plan) {
    static thread_local char buf[48];
    DilSel s;
    if (plan.family != kDenseDil || !dil_select(d, plan.h_out, plan.w_out, &s)) return "none";
    snprintf(buf, sizeof buf, "%s/%d%d%d/ns%d", s.fr == 2 ? "8x2" : "16x1", s.cfg.wm, s.cfg.wn, s.cfg.mt, s.nslot);
    return buf;
}

template <int WM, int WN, int MT, int FR>
static int launch_dil_t(const DilParams& p, const DilSel& s, hipStream_t stream) {
    auto fn = s.nslot == 3 ? k_dense_dil<WM, WN, MT, FR, 3> : k_dense_dil<WM, WN, MT, FR, kDilMaxSlots>;
    const int rc = raise_lds_limit(reinterpret_cast<const void*>(fn), 160 * 1024);   // once per (device, kernel)
    if (rc != SLFP_OK) return rc;
    hipLaunchKernelGGL(fn, dim3(p.nblocks), dim3(kDilThreads), s.lds, stream, p);
    return check_launch("slfp dilated dense MFMA conv kernel");
}

template <int FR>
static int launch_dil_f(const DilParams& p, const DilSel& s, hipStream_t stream) {
    switch (s.cfg.wm * 100 + s.cfg.wn * 10 + s.cfg.mt) {
        case 422: return launch_dil_t<4, 2, 2, FR>(p, s, stream);
        case 421: return launch_dil_t<4, 2, 1, FR>(p, s, stream);
        default: return launch_dil_t<8, 1, 1, FR>(p, s, stream);
    }
}

int launch_dense_dil(const slfp_conv2d_desc& d, const ConvPlan& plan, const float* x, const void* wblob, const float* bias,
                     const PostOp& post, float* y, void* workspace, hipStream_t stream) {
    DilSel s;
    if (!dil_select(d, plan.h_out, plan.w_out, &s)) return fail(SLFP_ERR_UNSUPPORTED, "dilated dense MFMA conv: no tiling fits");
    if (!workspace) return fail(SLFP_ERR_BAD_ARG, "dilated dense MFMA conv: workspace required (slfp_conv2d_workspace_bytes)");
    // ---- pass 1: the dense family's pre-pass (zero page + fp16 copy in B-fragment chunk order)
    launch_dense_encode(d, plan.fmt_act, x, workspace, false, stream);
    int rc = check_launch("slfp dense encode kernel");
    if (rc != SLFP_OK) return rc;
    // ---- pass 2: the phases
    DilParams p;
    p.zero_page = reinterpret_cast<const unsigned char*>(workspace);
    p.xe = reinterpret_cast<const _Float16*>(p.zero_page + 256);
    p.w = reinterpret_cast<const _Float16*>(wblob); p.bias = bias; p.y = y; p.post = post;
    p.N = (int)d.n; p.H = (int)d.h; p.W = (int)d.w; p.Cp = (int)plan.k_pad; p.O = (int)d.c_out;
    p.KH = (int)d.kh; p.KW = (int)d.kw; p.dh = d.dil_h; p.dw = d.dil_w; p.ph = d.pad_h; p.pw = d.pad_w;
    p.Ho = (int)plan.h_out; p.Wo = (int)plan.w_out;
    p.phases_h = std::min(p.dh, p.Ho); p.phases_w = std::min(p.dw, p.Wo);
    p.tiles_h = (int)ceil_div(ceil_div(p.Ho, p.dh), s.th); p.tiles_w = (int)ceil_div(ceil_div(p.Wo, p.dw), s.tw);
    p.n_blocks = (int)ceil_div((int64_t)p.O, s.cfg.wn * 64);
    p.IW = s.iw; p.n_pix = s.n_pix; p.x_pieces = s.pieces; p.x_per_tap = s.per_tap;
    p.KS = (int)(plan.k_pad / 32); p.n_tiles = (int)(plan.n_pad / 16);
    p.s1 = plan.s1; p.s2 = plan.s2; p.s1x = plan.s1 * (1.0f / 256.0f);
    const int64_t nblocks = (int64_t)p.N * p.phases_h * p.phases_w * p.tiles_h * p.tiles_w * p.n_blocks;
    if (nblocks > 0x7FFFFFFF) return fail(SLFP_ERR_UNSUPPORTED, "dilated dense MFMA conv: grid too large");
    p.nblocks = (uint32_t)nblocks;
    return s.fr == 2 ? launch_dil_f<2>(p, s, stream) : launch_dil_f<1>(p, s, stream);
}

}  // namespace slfp
