// conv_dwk.hip -- SLFP-quantized depthwise 5x5 / 7x7 convolution, NHWC, float32 in, float32 out, gfx950 (opt-in: SLFP_DESC_DW_KXK).
//
// The depthwise layers whose kernel is not 3x3 (MobileNetV3 / EfficientNet / MnasNet 5x5, ConvNeXt 7x7) fell to k_direct, where a
// workgroup serves one channel and 16 of its 256 threads have a live output.  Here, as in the depthwise 3x3 family (conv_dw_core.hpp):
//   * one workgroup = one (image, TH x TW output tile, 32-channel group); lane = (pixel slot, channel quad), so every global access is
//     16 bytes per lane and a whole 128-byte line per 8 lanes;
//   * all halo loads go out back to back through a per-image buffer descriptor: padding, ragged edges, dead slots and the dead
//     quads of a ragged last channel group are out-of-range offsets (the load returns 0, the store is dropped), no branches;
//   * every input element is quantized ONCE per workgroup (threshold table, dw_put_halo) into a float32 LDS tile of 128 B per
//     pixel; at stride 2 a row keeps its even columns first, then its odd ones, so a lane's operands stay 128 B apart;
//   * the K * K * 32 weights of the channel group sit in LDS as well (3.1 / 6.1 KiB): 49 weight quads do not fit in registers.
// The convolution is a run-and-row window: a lane owns R consecutive output columns x RH consecutive output rows of its channel quad
// (a "unit") and walks the (RH - 1) S + K input rows of that block once.  Per input row it reads the (R - 1) S + K operand quads
// into registers and applies them to every output row they feed (kh = input row - S * output row), reading that weight row (K
// quads, the same address in every pixel slot: a broadcast) for each.  kh ascends with the input row and kw runs inside, so each
// output's chain is k_direct's: one fma per tap from +0 in (kh, kw) order, then ((acc + bq) * s1) * s2 and the post-op -- the
// outputs are bit-equal to the direct kernel's (tests/test_gpu_dwk.py).  The fmas are issued as two v_pk_fma_f32 per quad.
// At stride 2 with RH = 2 a weight row serves output row 0 at input row kh and output row 1 at input row kh + 2: it is read once and
// kept in a rolling window of three rows (registers) in between, so the unit reads each weight row once, not once per output row.
// Units that would hang over the tile's edge are moved back inside it (min(b * R, TW - R)): a few outputs are computed and stored
// twice with equal bits, and nothing is read outside the tile.  Pixel slots without a unit (stride 2) leave after the tile is
// quantized: they take no part in the convolution.  Outputs of a tile that overhangs the image are computed and dropped by the store.
// LDS reads (ds_read_b128) per output quad, computed: DESIGN.md section 48.  dwk_select is the one place that decides what the
// family takes, the tile, the grid and the debug name.
#include "conv_dw_core.hpp"

namespace slfp {

struct DwkParams {
    int N, H, W, C, Ho, Wo;
    int tiles_h, tiles_w, cgroups;
    int pad_h, pad_w;
    uint32_t nblocks;
    float s1, s2;
    int nt_out;           // store the output with the nt hint (dw_nt_out)
    PostOp post;
    EncArgs enc;
};

__device__ __forceinline__ f32x4 dwk_fma4(const f32x4 a, const f32x4 w, const f32x4 acc) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const f32x2 lo = __builtin_elementwise_fma(f32x2{a[0], a[1]}, f32x2{w[0], w[1]}, f32x2{acc[0], acc[1]});   // v_pk_fma_f32: the same
    const f32x2 hi = __builtin_elementwise_fma(f32x2{a[2], a[3]}, f32x2{w[2], w[3]}, f32x2{acc[2], acc[3]});   // IEEE fma per element
    return f32x4{lo[0], lo[1], hi[0], hi[1]};
}

// K: kernel (5, 7); S: stride (1, 2); TH x TW: output tile; R x RH: a lane's unit (columns x rows); NT: threads; POST: fused
// per-channel scale / shift present.
template <int K, int S, int TH, int TW, int R, int RH, int NT, bool POST>
__global__ __launch_bounds__(NT) void k_dwk(const float* __restrict__ x, const float* __restrict__ wq, const float* __restrict__ bias,
                                            float* __restrict__ y, const DwkParams p) {
    constexpr int IH = (TH - 1) * S + K, IW = (TW - 1) * S + K;     // halo tile
    constexpr int NSLOT = NT / 8, NPIX = IH * IW;
    constexpr int NI = (NPIX + NSLOT - 1) / NSLOT;                  // load items per thread: pixels slot + i * NSLOT of the LDS tile
    constexpr int EH = (IW + 1) / 2;                                // stride 2: a row's even columns in 0 .. EH - 1, then the odd ones
    constexpr int BW = (TW + R - 1) / R, BH = (TH + RH - 1) / RH, UNITS = BW * BH;
    constexpr int NOP = (R - 1) * S + K, NIR = (RH - 1) * S + K;    // operand quads per input row, input rows per unit
    constexpr int NWQ = K * K * 8, NWI = (NWQ + NT - 1) / NT;       // weight quads of the channel group, per thread
    static_assert(UNITS <= NSLOT && TW >= R && TH >= RH && NT % 64 == 0, "a unit per pixel slot, inside the tile");
    static_assert(S == 1 || S == 2, "stride 1 or 2");

    // static LDS: the table at address 0 (conv_dw2.hip), the weights [K * K][32], the tile [NI * NSLOT pixels][32] float32
    __shared__ __attribute__((aligned(16))) unsigned char smem[kDwTabBytes + NWQ * 16 + NI * NSLOT * 128];
    unsigned char* sw = smem + kDwTabBytes;
    unsigned char* tile = sw + NWQ * 16;
    enc_fill<NT>(reinterpret_cast<uint2*>(smem), p.enc);
    const float r1 = p.enc.r1, lo = p.enc.lo, hi = p.enc.hi;

    const uint32_t lb = xcd_remap(blockIdx.x, p.nblocks);
    const int cg = (int)(lb % (uint32_t)p.cgroups);
    const uint32_t t = lb / (uint32_t)p.cgroups;   // tile: (image, tile row, tile column)
    const uint32_t tiles_per_img = (uint32_t)(p.tiles_h * p.tiles_w);
    const uint32_t n = t / tiles_per_img, tr = t - n * tiles_per_img;
    const int th = (int)(tr / (uint32_t)p.tiles_w), tw = (int)(tr - (uint32_t)th * p.tiles_w);

    const int c4 = threadIdx.x & 7, slot = threadIdx.x >> 3;   // 8 lanes per pixel slot
    const int c = cg * 32 + c4 * 4;
    const bool c_live = c < p.C;                               // the last group is ragged: its dead quads load 0 and store nothing

    // ---- the group's weights [kh][kw][C] -> LDS, and all halo loads of the tile, back to back
    {
        const __amdgpu_buffer_rsrc_t rw = dw_rsrc(wq, (uint32_t)(K * K) * (uint32_t)p.C * 4u);
        u32x4 wv[NWI];
#pragma unroll
        for (int i = 0; i < NWI; ++i) {
            const int item = (int)threadIdx.x + i * NT, cw = cg * 32 + (item & 7) * 4;
            uint32_t wo = (item < NWQ && cw < p.C) ? (uint32_t)((item >> 3) * p.C + cw) * 4u : kDwOob;
            asm volatile("" : "+v"(wo));
            wv[i] = __builtin_amdgcn_raw_buffer_load_b128(rw, wo, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < NWI; ++i) {
            const int item = (int)threadIdx.x + i * NT;
            if (item < NWQ) *reinterpret_cast<u32x4*>(sw + item * 16) = wv[i];
        }
    }
    f32x4 v[NI];
    {
        const uint32_t img_in_bytes = (uint32_t)p.H * p.W * p.C * 4u;
        const __amdgpu_buffer_rsrc_t rs = dw_rsrc(x + (size_t)n * p.H * p.W * p.C, img_in_bytes);
        const int gh0 = th * TH * S - p.pad_h, gw0 = tw * TW * S - p.pad_w;
        uint32_t voff[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int pix = slot + i * NSLOT;
            const int row = pix / IW, dc = pix - row * IW;                                      // compile-time divisor
            const int col = (S == 2) ? (dc < EH ? 2 * dc : 2 * (dc - EH) + 1) : dc;            // the column LDS slot dc holds
            const int gh = gh0 + row, gw = gw0 + col;
            const bool ok = c_live && pix < NPIX && (unsigned)gh < (unsigned)p.H && (unsigned)gw < (unsigned)p.W;
            voff[i] = ok ? (uint32_t)((gh * p.W + gw) * p.C + c) * 4u : kDwOob;
            asm volatile("" : "+v"(voff[i]));   // a value, not control flow (conv_dw2.hip)
        }
#pragma unroll
        for (int i = 0; i < NI; ++i)
            v[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff[i], 0, (SLFP_NT_DW & 1) ? 2 : 0));
    }
    __syncthreads();   // threshold table and weights visible

    // ---- quantize the tile into LDS: Q(0) == 0, so padding and dead slots go through the same path
    dw_put_halo<NI, NSLOT * 128>(tile + slot * 128 + c4 * 16, v, r1, lo, hi, smem);
    __syncthreads();

    // ---- convolve: this lane's unit, R columns x RH rows from (oy, ox) of the tile
    if (UNITS < NSLOT && slot >= UNITS) return;   // no unit for this slot; no barrier follows (at 128 threads: all of the second wave)
    const int by = slot / BW, bx = slot - by * BW;
    const int oy = by * RH < TH - RH ? by * RH : TH - RH, ox = bx * R < TW - R ? bx * R : TW - R;
    // the unit's first input pixel: row oy * S; column ox * S, which at stride 2 is even and sits in slot ox of its row
    const unsigned char* win = tile + (uint32_t)((oy * S * IW + ox) * 128 + c4 * 16);
    const unsigned char* wl = sw + c4 * 16;
    f32x4 acc[RH][R];
#pragma unroll
    for (int r = 0; r < RH; ++r)
#pragma unroll
        for (int q = 0; q < R; ++q) acc[r][q] = f32x4{0.f, 0.f, 0.f, 0.f};
    // ROLL: each weight row is read once, at input row kh, and kept until output row RH - 1 has used it, S (RH - 1) input rows later
    constexpr bool ROLL = S == 2 && RH == 2;
    constexpr int WD = ROLL ? S * (RH - 1) + 1 : 1;
    f32x4 ww[WD][K];   // ww[j]: weight row (input row - j)
    if constexpr (ROLL) {
#pragma unroll
        for (int j = 0; j < WD; ++j)
#pragma unroll
            for (int kw = 0; kw < K; ++kw) ww[j][kw] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll 1   // one input row at a time: unrolled, hipcc hoists every LDS read of the unit and spills (as in k_stem_fixed)
    for (int ir = 0; ir < NIR; ++ir) {
        f32x4 op[NOP];
#pragma unroll
        for (int j = 0; j < NOP; ++j)
            op[j] = *reinterpret_cast<const f32x4*>(win + (ir * IW + ((S == 2) ? (j & 1) * EH + (j >> 1) : j)) * 128);
        if constexpr (ROLL) {
#pragma unroll
            for (int j = WD - 1; j > 0; --j)
#pragma unroll
                for (int kw = 0; kw < K; ++kw) ww[j][kw] = ww[j - 1][kw];
            if (ir < K) {
#pragma unroll
                for (int kw = 0; kw < K; ++kw) ww[0][kw] = *reinterpret_cast<const f32x4*>(wl + (ir * K + kw) * 128);
            }
        }
#pragma unroll
        for (int r = 0; r < RH; ++r) {
            const int kh = ir - r * S;   // the weight row this input row meets in output row r: the same in every lane (a scalar branch)
            if (kh < 0 || kh >= K) continue;
#pragma unroll
            for (int kw = 0; kw < K; ++kw) {
                f32x4 w;
                if constexpr (ROLL) w = ww[r * S][kw];
                else w = *reinterpret_cast<const f32x4*>(wl + (kh * K + kw) * 128);
#pragma unroll
                for (int q = 0; q < R; ++q) acc[r][q] = dwk_fma4(op[q * S + kw], w, acc[r][q]);
            }
        }
    }

    // ---- finish + store
    const int cs = c_live ? c : 0;   // dead quads read channel 0's vectors and store nothing
    f32x4 psc, psh, bq = {0.f, 0.f, 0.f, 0.f};
    dw_load_bn<POST>(psc, psh, p.post.scale, p.post.shift, cs);
    if (bias) {
        const f32x4 bb = *reinterpret_cast<const f32x4*>(bias + cs);
#pragma unroll
        for (int e = 0; e < 4; ++e) bq[e] = (bb[e] / p.s1) / p.s2;   // bias_q (k_direct)
    }
    const __amdgpu_buffer_rsrc_t ry = dw_rsrc(y + (size_t)n * p.Ho * p.Wo * p.C, (uint32_t)p.Ho * p.Wo * p.C * 4u);
    const int oh0 = th * TH + oy, ow0 = tw * TW + ox;
#pragma unroll
    for (int r = 0; r < RH; ++r) {
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const f32x4 rr = dw_finish_bias<POST>(acc[r][q], bq, p.s1, p.s2, psc, psh, p.post.relu);
            const bool live = c_live && (oh0 + r) < p.Ho && (ow0 + q) < p.Wo;
            uint32_t so = live ? (uint32_t)(((oh0 + r) * p.Wo + ow0 + q) * p.C + c) * 4u : kDwOob;
            asm volatile("" : "+v"(so));
            dw_store16(rr, ry, so, p.nt_out);
        }
    }
}

// ---- host side: one selection (dwk_select) behind the plan, the launch and the debug name -------------------------------
// The (K, S, TH, TW, R, RH, NT) shapes dwk_select chooses among; POST doubles them.
//   stride 1, maps above 7 x 7:  14 x 14 tile, 4 x 4 units, 128 threads (16 units = 16 pixel slots)
//   stride 1, maps up to 7 x 7:   7 x 7 tile, 4 x 2 units, 64 threads (8 units = 8 slots)
//   stride 2, 7 x 7:              7 x 8 tile, 8 x 1 units, 128 threads (7 units; the halo is as large as the 14 x 14 tile's)
//   stride 2, 5 x 5:              7 x 8 tile, 8 x 2 units with the rolling weight window, 128 threads (4 units: what keeps the LDS
//                                 reads per stored output quad within K * K / 2)
// At stride 2 the slots without a unit load and quantize their share of the halo, then leave.
#define SLFP_DWK_SHAPES(X) X(5, 1, 14, 14, 4, 4, 128) X(5, 1, 7, 7, 4, 2, 64) X(5, 2, 7, 8, 8, 2, 128) \
                           X(7, 1, 14, 14, 4, 4, 128) X(7, 1, 7, 7, 4, 2, 64) X(7, 2, 7, 8, 8, 1, 128)

bool dwk_select(const slfp_conv2d_desc& d, int fmt_act, DwkSel* s) {
    if (d.groups != d.c_in || d.c_out != d.c_in || d.kh != d.kw || (d.kh != 5 && d.kh != 7)) return false;
    if (d.dil_h != 1 || d.dil_w != 1 || d.stride_h != d.stride_w || (d.stride_h != 1 && d.stride_h != 2)) return false;
    const int k = (int)d.kh;
    if (d.pad_h < 0 || d.pad_h > (k - 1) / 2 || d.pad_w < 0 || d.pad_w > (k - 1) / 2 || d.c_in % 4) return false;
    const int64_t ho = (d.h + 2 * (int64_t)d.pad_h - k) / d.stride_h + 1, wo = (d.w + 2 * (int64_t)d.pad_w - k) / d.stride_w + 1;
    if (d.h + 2 * (int64_t)d.pad_h < k || d.w + 2 * (int64_t)d.pad_w < k) return false;
    // 32-bit byte offsets inside one image of x, of y and inside the weights (conv_dw_core.hpp: a descriptor spans < 2^31 bytes)
    if ((int64_t)d.h * d.w * d.c_in >= (1ll << 29) || ho * wo * d.c_in >= (1ll << 29) || (int64_t)k * k * d.c_in >= (1ll << 29)) return false;
    if (!act_table(d.ka, fmt_act, kEncF32)) return false;   // the quantizer on load is the threshold table
    s->k = k; s->s = d.stride_h;
    if (s->s == 2) { s->th = 7; s->tw = 8; s->r = 8; s->rh = k == 5 ? 2 : 1; s->nt = 128; }
    else if (ho <= 7 && wo <= 7) { s->th = 7; s->tw = 7; s->r = 4; s->rh = 2; s->nt = 64; }
    else { s->th = 14; s->tw = 14; s->r = 4; s->rh = 4; s->nt = 128; }
    s->tiles_h = (int)ceil_div(ho, s->th); s->tiles_w = (int)ceil_div(wo, s->tw);
    s->cgroups = (int)ceil_div(d.c_in, 32);
    const int64_t nblocks = d.n * s->tiles_h * s->tiles_w * s->cgroups;
    if (nblocks > 0x7FFFFFFF) return false;
    s->nblocks = (uint32_t)nblocks;
    return true;
}

typedef void (*DwkFn)(const float*, const float*, const float*, float*, const DwkParams);
static DwkFn dwk_instance(const DwkSel& s, bool post) {
#define SLFP_DWK_PICK(KK, SS, TH, TW, RR, RH, NT)                                                              \
    if (s.k == KK && s.s == SS && s.th == TH && s.tw == TW && s.r == RR && s.rh == RH && s.nt == NT)          \
        return post ? k_dwk<KK, SS, TH, TW, RR, RH, NT, true> : k_dwk<KK, SS, TH, TW, RR, RH, NT, false>;
    SLFP_DWK_SHAPES(SLFP_DWK_PICK)
#undef SLFP_DWK_PICK
    return nullptr;
}

static const char* dwk_sel_name(const DwkSel& s) {
    static thread_local char buf[64];
    snprintf(buf, sizeof buf, "k%d/s%d/%dx%d/r%dx%d", s.k, s.s, s.th, s.tw, s.r, s.rh);
    return buf;
}

const char* dwk_variant_name(const slfp_conv2d_desc& d, const ConvPlan& plan) {
    DwkSel s;
    if (plan.family != kDwKxK || !dwk_select(d, plan.fmt_act, &s) || !dwk_instance(s, false)) return "none";
    return dwk_sel_name(s);
}

int launch_dwk(const slfp_conv2d_desc& d, const ConvPlan& plan, const float* x, const float* wq, const float* bias, const PostOp& post,
               float* y, hipStream_t stream) {
    DwkSel s;
    if (!dwk_select(d, plan.fmt_act, &s) || post.layerout) return fail(SLFP_ERR_UNSUPPORTED, "dwk: layer outside the family");
    DwkParams p;
    p.N = (int)d.n; p.H = (int)d.h; p.W = (int)d.w; p.C = (int)d.c_in; p.Ho = (int)plan.h_out; p.Wo = (int)plan.w_out;
    p.tiles_h = s.tiles_h; p.tiles_w = s.tiles_w; p.cgroups = s.cgroups;
    p.pad_h = d.pad_h; p.pad_w = d.pad_w;
    p.nblocks = s.nblocks;
    p.s1 = plan.s1; p.s2 = plan.s2;
    p.nt_out = dw_nt_out((int64_t)p.N * p.Ho * p.Wo * p.C * 4);
    p.post = post;
    p.enc = *act_table(d.ka, plan.fmt_act, kEncF32);
    return dw_launch(dwk_instance(s, post.scale != nullptr), "dwk", dwk_sel_name(s), p.nblocks, s.nt, 0, stream, "slfp depthwise k x k kernel",
                     x, wq, bias, y, p);
}

}  // namespace slfp
