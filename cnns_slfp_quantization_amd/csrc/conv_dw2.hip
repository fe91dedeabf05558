// conv_dw2.hip -- SLFP-quantized depthwise 3x3 convolution, NHWC, gfx950: the straight-line tile kernel.
//
// The depthwise 3x3 layers with C a multiple of 32, stride 1 / 2 (the 13 "dw" layers of MobileNetV1, nets_imgnet/mobilenetv1.py:27);
// conv_dw.hip, the general kernel, keeps the odd shapes.  Arithmetic: include/slfp.h, next to slfp_debug_dw3x3_instance; the steps
// shared with the other depthwise kernels: conv_dw_core.hpp.
//
// What changed, and why (profiles/r02a, r02b; profiles/variants.py):
//   * every global access is a buffer_load / buffer_store through a per-image descriptor: out-of-image halo
//     pixels and ragged tile edges get an out-of-range offset (the range check returns 0 / drops the store),
//     so the body is ONE straight line: all 8 x 16-byte loads of the halo tile are issued back to back and
//     hipcc counts them exactly (conv_dw.hip's per-item bounds branches made it wait vmcnt(0) before every
//     encode and split the encode stream into 4-element pieces);
//   * the quantizer is the threshold table of slfp_enc.hpp (7 VALU instructions per element, was 22);
//   * halo and output geometry are fixed at 16 (8) pixel slots per row (lane = (pixel slot, 4 channels)):
//     every LDS and global offset is `per-thread constant + immediate`, no index arithmetic is left in the loops.
// One workgroup = one (image, 14x14 | 7x7 output tile, 32-channel group), many small workgroups in flight: a
// persistent, software-pipelined variant (loads of tile t+1 in flight under the convolution of tile t, 4 / 8 /
// 16 tiles per workgroup) was built and measured 2-12 % SLOWER on every layer -- the hardware's workgroup
// dispatcher balances 16 k small workgroups better than a static partition, and four co-resident workgroups in
// different phases already overlap loads with compute.  Same-box, interleaved (us per layer, batch 256):
// conv_dw.hip + table 1058 total, this kernel 984 (5.2 TB/s algorithmic), persistent x16 1126.
// Neighbouring tiles share 2-pixel halos; logical workgroup ids are dealt to XCDs contiguously (xcd_remap) so
// the re-reads hit the same L2 (HBM reads = algorithmic bytes, profiles/r02c).
// Round 4: the stride-2 layers take conv_dw3.hip (k_dw3x3_rows, no LDS tile) unless SLFP_DW_ROWS=0; the stride-2 instance here is
// their reference (tests/test_gpu_dw_rows.py: byte-equal) and the A/B arm.
#include "conv_dw_core.hpp"

namespace slfp {

constexpr int kDw2Threads = 256;

struct Dw2Params {
    int N, H, W, C, Ho, Wo;
    int tiles_h, tiles_w, cgroups;
    int pad;
    uint32_t ntiles;      // N * tiles_h * tiles_w: tiles per channel group
    uint32_t nblocks;
    float ka, kw;
    int nt_out;           // store the output with the nt hint (set by the launcher: outputs too large for the Infinity Cache)
    PostOp post;
    EncArgs enc;
};

// S: stride (1, 2); TH x TW: output tile (14x14 or 7x7 for stride 1, 7x7 for stride 2); POST: fused
// per-channel scale/shift (eval-mode BatchNorm) present.
template <int S, int TH, int TW, bool POST>
__global__ __launch_bounds__(kDw2Threads, 4) void k_dw3x3_tile(const float* __restrict__ x, const float* __restrict__ wq,
                                                               float* __restrict__ y, const Dw2Params p) {
    constexpr int IH = (TH - 1) * S + 3, IW = (TW - 1) * S + 3;
    static_assert(IW <= 16 && IH <= 16, "halo tile is at most 16 x 16 pixel slots");
    constexpr int NI = (IH + 1) / 2;            // load items per thread: rows 2i + (slot >> 4)
    constexpr int ROWB = 16 * 32 * 4;           // LDS bytes per halo row: 16 pixel slots x 32 channels

    // static LDS: the table sits at LDS address 0, a compile-time constant, so every table lookup is `ds_read_b64 v, bin`
    // without the add of a (link-time) dynamic-LDS base that hipcc otherwise emits per lookup
    __shared__ __attribute__((aligned(16))) unsigned char smem[kDwTabBytes + 2 * NI * ROWB];
    unsigned char* tile = smem + kDwTabBytes;       // [2 * NI rows][16 slots][32 ch] float32
    enc_fill<kDw2Threads>(reinterpret_cast<uint2*>(smem), p.enc);
    const float r1 = p.enc.r1, lo = p.enc.lo, hi = p.enc.hi;

    const uint32_t lb = xcd_remap(blockIdx.x, p.nblocks);
    const int cg = (int)(lb % (uint32_t)p.cgroups);
    const uint32_t t = lb / (uint32_t)p.cgroups;   // tile: (image, tile row, tile column)

    const int c4 = threadIdx.x & 7, slot = threadIdx.x >> 3;   // 8 lanes per pixel, 32 pixel slots
    const int c = cg * 32 + c4 * 4;
    const int iw = slot & 15, ihh = slot >> 4;

    // this thread's 4 channels x 9 taps, fused BN vectors (layers with a bias take conv_dw.hip)
    f32x4 wt[9], psc, psh;
    dw_load_taps(wt, wq, (size_t)p.C, c);
    dw_load_bn<POST>(psc, psh, p.post.scale, p.post.shift, c);

    // per-thread constants of the halo load / LDS write
    const int colslot = (S == 2) ? ((iw & 1) * 8 + (iw >> 1)) : iw;          // stride 2: even columns, then odd
    const uint32_t lds_w = (uint32_t)((ihh * 16 + colslot) * 128 + c4 * 16);  // + i * 2 * ROWB
    const bool col_live = iw < IW;
    // outputs: the 32 pixel slots are CW columns x 32/CW rows per step (16 x 2 for 14-wide tiles, 8 x 4 for 7-wide
    // ones), so every per-step offset is `constant + step * immediate` and no per-output index math is left
    constexpr int CW = TW > 8 ? 16 : 8, RPI = 32 / CW, NO = (TH + RPI - 1) / RPI;
    const int ow = slot & (CW - 1), ohb = slot / CW;
    const bool ocol_live = ow < TW;
    const uint32_t lds_r0 = (uint32_t)(((ohb * S) * 16 + ow) * 128 + c4 * 16);           // + j * RPI * S * ROWB
    const uint32_t out_rel0 = (uint32_t)((ohb * p.Wo + ow) * p.C + c) * 4u;              // + j * RPI * Wo * C * 4
    const uint32_t out_step = (uint32_t)(RPI * p.Wo * p.C) * 4u;
    const uint32_t img_in_bytes = (uint32_t)p.H * p.W * p.C * 4u, img_out_bytes = (uint32_t)p.Ho * p.Wo * p.C * 4u;
    const uint32_t tiles_per_img = (uint32_t)(p.tiles_h * p.tiles_w);

    const uint32_t n = t / tiles_per_img, tr = t - n * tiles_per_img;
    const int th = (int)(tr / (uint32_t)p.tiles_w), tw = (int)(tr - (uint32_t)th * p.tiles_w);

    // ---- all halo loads of the tile, back to back
    f32x4 v[NI];
    {
        const __amdgpu_buffer_rsrc_t rs = dw_rsrc(x + (size_t)n * p.H * p.W * p.C, img_in_bytes);
        const int gw = tw * TW * S - p.pad + iw;
        const int gh0 = th * TH * S - p.pad + ihh;
        const bool w_ok = col_live && (unsigned)gw < (unsigned)p.W;
        const uint32_t off0 = (uint32_t)((gh0 * p.W + gw) * p.C + c) * 4u;   // wraps for negative rows: only used when in range
        const uint32_t step = (uint32_t)(2 * p.W * p.C) * 4u;
        uint32_t voff[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            bool ok = w_ok && (unsigned)(gh0 + 2 * i) < (unsigned)p.H;
            if (2 * i + 1 >= IH) ok = ok && ihh == 0;          // the odd last halo row does not exist
            voff[i] = ok ? off0 + (uint32_t)i * step : kDwOob;
            asm volatile("" : "+v"(voff[i]));                   // a value, not control flow: hipcc otherwise branches around the load
        }
#pragma unroll
        for (int i = 0; i < NI; ++i)
            v[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff[i], 0, (SLFP_NT_DW & 1) ? 2 : 0));
    }
    __syncthreads();   // threshold table visible

    // ---- quantize the tile into LDS: Q(0) == 0, so padding and dead slots go through the same path
    dw_put_halo<NI, 2 * ROWB>(tile + lds_w, v, r1, lo, hi, smem);
    __syncthreads();

    // ---- convolve + store
    const __amdgpu_buffer_rsrc_t ry = dw_rsrc(y + (size_t)n * p.Ho * p.Wo * p.C, img_out_bytes);
    const int oh0 = th * TH, ow0 = tw * TW;
    const uint32_t org = (uint32_t)((oh0 * p.Wo + ow0) * p.C) * 4u;
#pragma unroll
    for (int j = 0; j < NO; ++j) {
        const f32x4 acc = dw_mac9_lds<S, ROWB>(wt, tile + lds_r0 + j * RPI * S * ROWB);
        const f32x4 rr = dw_finish<POST>(acc, p.ka, p.kw, psc, psh, p.post.relu);
        const bool live = ocol_live && (oh0 + ohb + j * RPI) < p.Ho && (j * RPI + ohb) < TH && (ow0 + ow) < p.Wo;
        uint32_t so = live ? org + out_rel0 + (uint32_t)j * out_step : kDwOob;
        asm volatile("" : "+v"(so));
        dw_store16(rr, ry, so, p.nt_out);
    }
}

bool dw3x3_tile_applicable(const slfp_conv2d_desc& d, const ConvPlan& plan, const float* bias, const PostOp& post) {
    if (bias) return false;
    if (long_encode_forced() || dw_old_forced()) return false;
    if (plan.family != kDw3x3 || plan.repad) return false;
    if (d.c_in % 32 != 0 || post.layerout) return false;
    if (d.pad_h > 2) return false;
    if (d.stride_h == 1 && plan.h_out <= 7 && plan.w_out <= 7) return false;   // 7x7 images: conv_dw.hip's 64-channel tiles are faster
    if ((int64_t)d.h * d.w * d.c_in >= (1ll << 29) || plan.h_out * plan.w_out * d.c_in >= (1ll << 29)) return false;
    return act_table(d.ka, plan.fmt_act, kEncF32) != nullptr;
}

// What launch_dw3x3_tile chooses among k_dw3x3_tile's instances.  dw2_instance maps it to the kernel: the launcher launches that
// pointer and dw3x3_tile_name asks for it before it prints, so a name is only ever given for an instance that exists.
struct Dw2Sel { int s; bool post; };   // template arguments S (TH = TW = 14 / 7 follow from it) and POST
static Dw2Sel dw2_select(const slfp_conv2d_desc& d, const PostOp& post) { return Dw2Sel{d.stride_h == 2 ? 2 : 1, post.scale != nullptr}; }

typedef void (*Dw2Fn)(const float*, const float*, float*, const Dw2Params);
static Dw2Fn dw2_instance(const Dw2Sel& s) {
    if (s.s == 2) return s.post ? k_dw3x3_tile<2, 7, 7, true> : k_dw3x3_tile<2, 7, 7, false>;
    if (s.s == 1) return s.post ? k_dw3x3_tile<1, 14, 14, true> : k_dw3x3_tile<1, 14, 14, false>;
    return nullptr;
}

static const char* dw2_sel_name(const Dw2Sel& s) { return s.s == 2 ? (s.post ? "tile/s2/post" : "tile/s2/plain") : (s.post ? "tile/s1/post" : "tile/s1/plain"); }

const char* dw3x3_tile_name(const slfp_conv2d_desc& d, const ConvPlan& plan, const PostOp& post) {
    const Dw2Sel s = dw2_select(d, post);
    return dw2_instance(s) ? dw2_sel_name(s) : "none";
}

int launch_dw3x3_tile(const slfp_conv2d_desc& d, const ConvPlan& plan, const float* x, const float* wq9c,
                      const PostOp& post, float* y, hipStream_t stream) {
    Dw2Params p;
    const Dw2Sel sel = dw2_select(d, post);
    p.post = post;
    dw_fill_geom(p, d, plan);
    const int S = sel.s;
    const int TH = S == 2 ? 7 : 14, TW = TH;
    p.tiles_h = (int)ceil_div(p.Ho, TH);
    p.tiles_w = (int)ceil_div(p.Wo, TW);
    p.cgroups = p.C / 32;
    const int64_t ntiles = (int64_t)p.N * p.tiles_h * p.tiles_w;
    if (const int rc = dw_grid_check(ntiles * p.cgroups, "dw3x3")) return rc;
    p.ntiles = (uint32_t)ntiles;
    p.nblocks = (uint32_t)(ntiles * p.cgroups);
    p.nt_out = dw_nt_out((int64_t)p.N * p.Ho * p.Wo * p.C * 4);
    p.enc = *act_table(d.ka, plan.fmt_act, kEncF32);
    return dw_launch(dw2_instance(sel), "dw3x3 (tile)", dw2_sel_name(sel), p.nblocks, kDw2Threads, 0, stream, "slfp dw3x3 (tile) kernel",
                     x, wq9c, y, p);
}

}  // namespace slfp
