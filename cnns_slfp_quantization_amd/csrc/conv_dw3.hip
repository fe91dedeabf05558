// conv_dw3.hip -- SLFP-quantized depthwise 3x3 convolution, stride 2, NHWC, gfx950: the register-window ("rows") kernel.
//
// The stride-2 layers of conv_dw2.hip, float32 in and out, outputs bit-identical to k_dw3x3_tile (arithmetic: include/slfp.h, next
// to slfp_debug_dw3x3_instance; shared steps: conv_dw_core.hpp).  What differs is where the quantized values live.  Stride-2 windows
// overlap by one row and one column only, so the LDS halo tile of conv_dw2.hip buys little reuse there and costs a 32 KiB tile (4 workgroups per CU),
// two barriers, an LDS write per input and 9 LDS reads per output on top of the table lookups -- and the LDS is what that
// kernel keeps busiest (profiles/r04a_summary.md).  Here, as in conv_dwc.hip, the window lives in registers:
//   * one WAVE = one (image, 7 x 7 output tile, 32-channel group), the tile kernel's workgroup: lane = (column group g = 0..7,
//     4 channels).  Group g < 7 owns output column g of the tile and walks down its TH = 7 output rows; every load and store
//     instruction of the wave covers whole 128-byte lines;
//   * a group loads and quantizes only the TWO input columns no other group has (2g, 2g + 1 of the tile's 15); the third
//     column of its window is its right neighbour's first, fetched already quantized from lane + 8 by ds_bpermute (4 dwords
//     per row instead of 4 table lookups with their bank conflicts).  Group 7 exists for its first column only: it is the
//     halo of group 6.  So 15 columns are quantized for 14 new ones, where a lane that keeps its own 3 columns quantizes 21;
//   * a float4 is four registers, so a lane cannot hold all 15 rows: it keeps a ring of 3 + 2 rows -- the three quantized
//     rows of the current window and the 2 rows of the next step in flight -- and quantizes each row in place when its
//     (counted) vmcnt wait is reached;
//   * loads and stores go through per-image buffer descriptors with out-of-range offsets for padding, ragged edges, the halo
//     group and idle waves (Q(0) == 0: a padded tap takes the same path), so the body is one straight line, fully unrolled;
//   * LDS holds the 2 KiB threshold table only; one barrier after its fill, none after.
#include "conv_dw_core.hpp"

namespace slfp {

constexpr int kDwrThreads = 256;
constexpr int kDwrWaves = kDwrThreads / 64;
constexpr int kDwrTile = 7;                              // output tile: 7 x 7, as conv_dw2.hip at stride 2

struct DwrParams {
    int N, H, W, C, Ho, Wo, pad;
    int cgs;              // channel groups of 32
    int tiles_h, tiles_w;
    uint32_t ntasks;      // N * tiles_h * tiles_w * cgs: one per wave
    uint32_t nblocks;
    float ka, kw;
    int nt_out;           // store the output with the nt hint (outputs too large for the Infinity Cache, as conv_dw2.hip)
    PostOp post;
    EncArgs enc;
};

// TH: output rows a wave walks down; POST: fused per-channel scale / shift.
// Row / column validity is one select each on the row and the column part of the byte offset (kDwBadRow / kDwBadCol).
template <int TH, bool POST>
__global__ __launch_bounds__(kDwrThreads, 4) void k_dw3x3_rows(const float* __restrict__ x, const float* __restrict__ wq,
                                                               float* __restrict__ y, const DwrParams p) {
    constexpr int S = 2, TW = kDwrTile;
    constexpr int NR = (TH - 1) * S + 3;
    constexpr int RING = 3 + S;

    // static LDS at address 0: every table lookup is `ds_read_b64 v, bin` (conv_dw2.hip)
    __shared__ __attribute__((aligned(16))) unsigned char smem[kDwTabBytes];
    enc_fill<kDwrThreads>(reinterpret_cast<uint2*>(smem), p.enc);
    const float r1 = p.enc.r1, lo = p.enc.lo, hi = p.enc.hi;

    // the wave's task: channel group fastest, then (image, tile row, tile column) -- the order of conv_dw2.hip's workgroups
    uint32_t t = xcd_remap(blockIdx.x, p.nblocks) * kDwrWaves + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const bool valid = t < p.ntasks;   // the last workgroup may have idle waves: every offset of theirs is out of range
    t = valid ? t : p.ntasks - 1;
    const int cg = (int)(t % (uint32_t)p.cgs); t /= (uint32_t)p.cgs;
    const int tw = (int)(t % (uint32_t)p.tiles_w); t /= (uint32_t)p.tiles_w;
    const int th = (int)(t % (uint32_t)p.tiles_h);
    const int n = (int)(t / (uint32_t)p.tiles_h);
    const int lane = (int)(threadIdx.x & 63), g = lane >> 3;
    const int c = cg * 32 + (lane & 7) * 4;

    // this lane's 4 channels x 9 taps, fused BN vectors (requested before the input rows: they return first)
    f32x4 wt[9], psc, psh;
    dw_load_taps(wt, wq, (uint32_t)p.C, c);
    dw_load_bn<POST>(psc, psh, p.post.scale, p.post.shift, c);

    const uint32_t img_in = (uint32_t)(p.H * p.W * p.C) * 4u, img_out = (uint32_t)(p.Ho * p.Wo * p.C) * 4u;
    const __amdgpu_buffer_rsrc_t rs = dw_rsrc(x + (size_t)n * (img_in / 4u), img_in);
    const __amdgpu_buffer_rsrc_t ry = dw_rsrc(y + (size_t)n * (img_out / 4u), img_out);

    // an idle wave starts so far above the image that none of its rows is in range
    const int ih0 = valid ? th * TH * S - p.pad : -0x40000000;
    const int ow = tw * TW + g, iw0 = ow * S - p.pad;
    const uint32_t rstep = (uint32_t)(p.W * p.C) * 4u;
    const uint32_t rowb = (uint32_t)ih0 * rstep + (uint32_t)c * 4u;   // wraps for negative rows: only used in range
    uint32_t coff[2];   // the halo group needs its first column only
    coff[0] = (unsigned)iw0 < (unsigned)p.W ? (uint32_t)(iw0 * p.C) * 4u : kDwBadCol;
    coff[1] = (g < TW && (unsigned)(iw0 + 1) < (unsigned)p.W) ? (uint32_t)((iw0 + 1) * p.C) * 4u : kDwBadCol;
    const int nb_addr = ((lane + 8) & 63) * 4;   // ds_bpermute address of the right neighbour's lane

    f32x4 win[RING][3];   // input row j lives in slot j % RING: columns 0 / 1 requested raw and quantized in place, column 2 fetched
    auto request = [&](const int j) {
        const uint32_t roff = (unsigned)(ih0 + j) < (unsigned)p.H ? rowb + (uint32_t)j * rstep : kDwBadRow;
#pragma unroll
        for (int k = 0; k < 2; ++k)
            win[j % RING][k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, roff + coff[k], 0, (SLFP_NT_DW & 1) ? 2 : 0));
    };
    // rows j0 .. j0 + nj - 1: quantize in place (NaN in -> NaN out by a cold patch, never taken on real activations), then
    // complete the window with the neighbour's first column
    auto quantize = [&](const int j0, const int nj) {
        bool any_nan = false;
#pragma unroll
        for (int j = j0; j < j0 + nj; ++j)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const f32x4 v = win[j % RING][k];
                any_nan |= enc_has_nan4(make_float4(v[0], v[1], v[2], v[3]));
            }
        uint32_t nan_mask = 0;   // one bit per element of these rows
        if (__builtin_expect(any_nan, 0)) {
#pragma unroll
            for (int j = j0; j < j0 + nj; ++j)
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const f32x4 v = win[j % RING][k];
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (v[e] != v[e]) nan_mask |= 1u << (((j - j0) * 2 + k) * 4 + e);
                }
        }
#pragma unroll
        for (int j = j0; j < j0 + nj; ++j)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const f32x4 v = win[j % RING][k];
                const float4 q = enc4_f32_raw(make_float4(v[0], v[1], v[2], v[3]), r1, lo, hi, smem);
                win[j % RING][k] = f32x4{q.x, q.y, q.z, q.w};
            }
        if (__builtin_expect(nan_mask != 0, 0)) {
#pragma unroll
            for (int j = j0; j < j0 + nj; ++j)
#pragma unroll
                for (int k = 0; k < 2; ++k)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (nan_mask >> (((j - j0) * 2 + k) * 4 + e) & 1u) win[j % RING][k][e] = __uint_as_float(kBitsQNaN);
        }
#pragma unroll
        for (int j = j0; j < j0 + nj; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                win[j % RING][2][e] = __int_as_float(__builtin_amdgcn_ds_bpermute(nb_addr, __float_as_int(win[j % RING][0][e])));
    };

#pragma unroll
    for (int j = 0; j < RING && j < NR; ++j) request(j);

    const int oh0 = th * TH;
    const uint32_t ostep = (uint32_t)(p.Wo * p.C) * 4u;
    const uint32_t ocol = (valid && g < TW && ow < p.Wo) ? (uint32_t)((oh0 * p.Wo + ow) * p.C + c) * 4u : kDwBadRow;

    __syncthreads();   // threshold table visible

    quantize(0, 3 - S);
#pragma unroll
    for (int r = 0; r < TH; ++r) {
        quantize(r * S + 3 - S, S);   // the S rows this step adds
        const f32x4 acc = dw_mac9(wt, [&](const int kh, const int kw) { return win[(r * S + kh) % RING][kw]; });
        const f32x4 rr = dw_finish<POST>(acc, p.ka, p.kw, psc, psh, p.post.relu);
        dw_store16(rr, ry, ocol + ((oh0 + r) < p.Ho ? (uint32_t)r * ostep : kDwBadCol), p.nt_out);
        // rows r*S .. r*S + S - 1 are dead now: their slots take the rows of the step after the next
#pragma unroll
        for (int j = r * S + RING; j < r * S + RING + S && j < NR; ++j) request(j);
    }
}

// size classes (dw_rows_class) that take this kernel when SLFP_DW_ROWS is unset: the whole-step A/B of profiles/notes/README.md
constexpr int kDwrRule = 0xF;

bool dw3x3_rows_applicable(const slfp_conv2d_desc& d, const ConvPlan& plan, const float* bias, const PostOp& post) {
    const int sw = switches().dw_rows;
    if (sw == 0) return false;
    if (!dw3x3_tile_applicable(d, plan, bias, post)) return false;
    if (d.stride_h != 2 || d.stride_w != 2 || d.pad_h != d.pad_w) return false;
    // offsets: bit 30 / 31 mark an invalid column / row, so one image is at most 2^30 bytes
    if ((int64_t)d.h * d.w * d.c_in * 4 > (1ll << 30) || plan.h_out * plan.w_out * d.c_in * 4 > (1ll << 30)) return false;
    return (((sw < 0) ? kDwrRule : sw) >> dw_rows_class(plan.h_out, plan.w_out)) & 1;
}

// What launch_dw3x3_rows chooses among k_dw3x3_rows' instances.  dwr_instance maps it to the kernel: the launcher launches that
// pointer and dw3x3_rows_name asks for it before it prints (conv_dw2.hip).
struct DwrSel { bool post; };   // template argument POST (TH is kDwrTile)
static DwrSel dwr_select(const PostOp& post) { return DwrSel{post.scale != nullptr}; }

typedef void (*DwrFn)(const float*, const float*, float*, const DwrParams);
static DwrFn dwr_instance(const DwrSel& s) { return s.post ? k_dw3x3_rows<kDwrTile, true> : k_dw3x3_rows<kDwrTile, false>; }
static const char* dwr_sel_name(const DwrSel& s) { return s.post ? "rows/post" : "rows/plain"; }

const char* dw3x3_rows_name(const slfp_conv2d_desc& d, const ConvPlan& plan, const PostOp& post) {
    const DwrSel s = dwr_select(post);
    return dwr_instance(s) ? dwr_sel_name(s) : "none";
}

int launch_dw3x3_rows(const slfp_conv2d_desc& d, const ConvPlan& plan, const float* x, const float* wq9c,
                      const PostOp& post, float* y, hipStream_t stream) {
    DwrParams p;
    const DwrSel sel = dwr_select(post);
    p.post = post;
    dw_fill_geom(p, d, plan);
    p.cgs = p.C / 32;
    p.tiles_h = (int)ceil_div(p.Ho, kDwrTile);
    p.tiles_w = (int)ceil_div(p.Wo, kDwrTile);
    const int64_t ntasks = (int64_t)p.N * p.tiles_h * p.tiles_w * p.cgs;
    if (const int rc = dw_grid_check(ntasks, "dw3x3 (rows)")) return rc;
    p.ntasks = (uint32_t)ntasks;
    p.nblocks = (uint32_t)ceil_div(ntasks, kDwrWaves);
    p.nt_out = dw_nt_out((int64_t)p.N * p.Ho * p.Wo * p.C * 4);
    p.enc = *act_table(d.ka, plan.fmt_act, kEncF32);
    return dw_launch(dwr_instance(sel), "dw3x3 (rows)", dwr_sel_name(sel), p.nblocks, kDwrThreads, 0, stream, "slfp dw3x3 (rows) kernel",
                     x, wq9c, y, p);
}

}  // namespace slfp
