// conv_dw3.hip -- SLFP-quantized depthwise 3x3 convolution, stride 2, NHWC, gfx950: the register-window ("rows") kernel.
//
// Same layers and the same arithmetic as conv_dw2.hip (float32 in, float32 out, input quantized once per loaded element by
// the threshold table, float32 FMAs from +0 in (kh, kw) order, (acc * Ka) * Kw, fused scale / shift, ReLU): outputs are
// bit-identical to k_dw3x3_tile.  What differs is where the quantized values live.  Stride-2 windows overlap by one row and
// one column only, so the LDS halo tile of conv_dw2.hip buys little reuse there and costs a 32 KiB tile (4 workgroups per CU),
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
#include "slfp_device.hpp"
#include "slfp_enc.hpp"
#include "slfp_host.hpp"

namespace slfp {

constexpr int kDwrThreads = 256;
constexpr int kDwrWaves = kDwrThreads / 64;
constexpr int kDwrTab = (kEncEntries * 8 + 15) & ~15;   // LDS bytes of the threshold table
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

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4r __attribute__((ext_vector_type(4)));

// TH: output rows a wave walks down; POST: fused per-channel scale / shift.
// Row / column validity is one select each on the row and the column part of the byte offset: the parts are >= 2^30 when
// invalid, so their sum is beyond the descriptor (one image: at most 2^30 bytes, dw3x3_rows_applicable).
template <int TH, bool POST>
__global__ __launch_bounds__(kDwrThreads, 4) void k_dw3x3_rows(const float* __restrict__ x, const float* __restrict__ wq,
                                                               float* __restrict__ y, const DwrParams p) {
    constexpr int S = 2, TW = kDwrTile;
    constexpr int NR = (TH - 1) * S + 3;
    constexpr int RING = 3 + S;

    // static LDS at address 0: every table lookup is `ds_read_b64 v, bin` (conv_dw2.hip)
    __shared__ __attribute__((aligned(16))) unsigned char smem[kDwrTab];
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
    f32x4 wt[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) wt[k] = *reinterpret_cast<const f32x4*>(wq + (uint32_t)(k * p.C + c));
    f32x4 psc = {1.f, 1.f, 1.f, 1.f}, psh = {0.f, 0.f, 0.f, 0.f};
    if constexpr (POST) {
        psc = *reinterpret_cast<const f32x4*>(p.post.scale + c);
        psh = *reinterpret_cast<const f32x4*>(p.post.shift + c);
    }

    const uint32_t img_in = (uint32_t)(p.H * p.W * p.C) * 4u, img_out = (uint32_t)(p.Ho * p.Wo * p.C) * 4u;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x + (size_t)n * (img_in / 4u)), 0, img_in, 0x00020000);
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(y + (size_t)n * (img_out / 4u), 0, img_out, 0x00020000);

    // an idle wave starts so far above the image that none of its rows is in range
    const int ih0 = valid ? th * TH * S - p.pad : -0x40000000;
    const int ow = tw * TW + g, iw0 = ow * S - p.pad;
    const uint32_t rstep = (uint32_t)(p.W * p.C) * 4u;
    const uint32_t rowb = (uint32_t)ih0 * rstep + (uint32_t)c * 4u;   // wraps for negative rows: only used in range
    uint32_t coff[2];   // the halo group needs its first column only
    coff[0] = (unsigned)iw0 < (unsigned)p.W ? (uint32_t)(iw0 * p.C) * 4u : 0x40000000u;
    coff[1] = (g < TW && (unsigned)(iw0 + 1) < (unsigned)p.W) ? (uint32_t)((iw0 + 1) * p.C) * 4u : 0x40000000u;
    const int nb_addr = ((lane + 8) & 63) * 4;   // ds_bpermute address of the right neighbour's lane

    f32x4 win[RING][3];   // input row j lives in slot j % RING: columns 0 / 1 requested raw and quantized in place, column 2 fetched
    auto request = [&](const int j) {
        const uint32_t roff = (unsigned)(ih0 + j) < (unsigned)p.H ? rowb + (uint32_t)j * rstep : 0x80000000u;
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
    const uint32_t ocol = (valid && g < TW && ow < p.Wo) ? (uint32_t)((oh0 * p.Wo + ow) * p.C + c) * 4u : 0x80000000u;

    __syncthreads();   // threshold table visible

    quantize(0, 3 - S);
#pragma unroll
    for (int r = 0; r < TH; ++r) {
        quantize(r * S + 3 - S, S);   // the S rows this step adds
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const f32x4 a = win[(r * S + kh) % RING][kw];
                const f32x4 w = wt[kh * 3 + kw];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = fmaf(a[e], w[e], acc[e]);
            }
        }
        f32x4 rr;   // (out * Ka) * Kw: two float32 roundings, as utils/conv2d_func.py:24; then the fused BN / ReLU
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float u = (acc[e] * p.ka) * p.kw;
            if constexpr (POST) u = __builtin_fmaf(u, psc[e], psh[e]);
            if (p.post.relu) u = fmaxf(u, 0.f);
            rr[e] = u;
        }
        const uint32_t so = ocol + ((oh0 + r) < p.Ho ? (uint32_t)r * ostep : 0x40000000u);
        if (p.nt_out) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4r, rr), ry, so, 0, 2);
        else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4r, rr), ry, so, 0, 0);
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

// What launch_dw3x3_rows chooses among k_dw3x3_rows' instances: the launcher dispatches on it, dw3x3_rows_name prints it.
struct DwrSel { bool post; };   // template argument POST (TH is kDwrTile)
static DwrSel dwr_select(const PostOp& post) { return DwrSel{post.scale != nullptr}; }

const char* dw3x3_rows_name(const slfp_conv2d_desc& d, const ConvPlan& plan, const PostOp& post) {
    return dwr_select(post).post ? "rows/post" : "rows/plain";
}

int launch_dw3x3_rows(const slfp_conv2d_desc& d, const ConvPlan& plan, const float* x, const float* wq9c,
                      const PostOp& post, float* y, hipStream_t stream) {
    DwrParams p;
    const DwrSel sel = dwr_select(post);
    p.post = post;
    p.N = (int)d.n; p.H = (int)d.h; p.W = (int)d.w; p.C = (int)d.c_in;
    p.Ho = (int)plan.h_out; p.Wo = (int)plan.w_out; p.pad = d.pad_h;
    p.cgs = p.C / 32;
    p.tiles_h = (int)ceil_div(p.Ho, kDwrTile);
    p.tiles_w = (int)ceil_div(p.Wo, kDwrTile);
    const int64_t ntasks = (int64_t)p.N * p.tiles_h * p.tiles_w * p.cgs;
    if (ntasks > 0x7FFFFFFF) return fail(SLFP_ERR_UNSUPPORTED, "dw3x3 (rows): grid too large");
    p.ntasks = (uint32_t)ntasks;
    p.nblocks = (uint32_t)ceil_div(ntasks, kDwrWaves);
    p.ka = d.ka; p.kw = d.kw_scale;
    p.nt_out = ((SLFP_NT_DW & 2) && (int64_t)p.N * p.Ho * p.Wo * p.C * 4 >= (switches().dw_nt_min_mb << 20)) ? 1 : 0;
    p.enc = *act_table(d.ka, plan.fmt_act, kEncF32);
    if (sel.post) hipLaunchKernelGGL((k_dw3x3_rows<kDwrTile, true>), dim3(p.nblocks), dim3(kDwrThreads), 0, stream, x, wq9c, y, p);
    else hipLaunchKernelGGL((k_dw3x3_rows<kDwrTile, false>), dim3(p.nblocks), dim3(kDwrThreads), 0, stream, x, wq9c, y, p);
    return check_launch("slfp dw3x3 (rows) kernel");
}

}  // namespace slfp
