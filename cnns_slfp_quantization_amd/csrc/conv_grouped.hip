// conv_grouped.hip -- SLFP-quantized GROUPED k x k convolution (1 < groups < C_in) on the gfx950 matrix cores: the 3x3 conv2
// layers of ResNeXt-50/101 (32x4d, 32x8d, 64x4d), RegNet group widths up to 32, any "cardinality" block of
// conv2d_Q(..)(c, c, k, groups=g).
//
// Block-diagonal implicit GEMM over GROUP SETS.  With Cg = C_in / groups and Og = C_out / groups, a set is
// gs = 16 / gcd(Og, 16) consecutive groups: its output width gs * Og is a whole number of 16-channel MFMA tiles, its input span
// gs * Cg channels (a multiple of 8, at most 64).  Inside a set every 16-channel output tile contracts over the whole span, the
// weights of foreign groups being zeros in the prepared blob (efficiency 1 / gs of the dense MFMA rate; the layer is bound by
// its 4 B in + 4 B out per element, not by the matrix cores).  No set is split across workgroups, and no workgroup reads a
// channel it does not own, so the quantizer runs on load: one pass over x, one over y, no pre-pass, no workspace.
//   * workgroup = 4 waves, one image, SW adjacent sets (SW * span >= 32 channels: each halo pixel is one contiguous run of at
//     least 128 B of float32), and a strided share of the image's 8 x 16 output-pixel tiles;
//   * once per workgroup: the threshold table of the layer's (Ka, format) (slfp_enc.hpp), the sets' weight blob
//     [set][n_tile][k_step][64 lanes][8] fp16 and a table of k-offsets go to LDS and stay there for every tile it walks.  LDS,
//     not registers: k_steps * n_tiles * 4 VGPRs is 20 for ResNeXt-50's 16-wide sets but 288 for a 64-wide 3x3 set, and a
//     register form needs (k_steps, n_tiles) at compile time; one LDS form serves the whole envelope with four instances;
//   * per tile: the halo ((8-1)S + KH) x ((16-1)S + KW) pixels x SW * span channels is read as float32 with 16-byte loads (four
//     in flight per thread), encoded with enc4_f16 (NaN -> fp16 NaN) and stored as fp16 at a pixel pitch of an odd number of
//     16-byte chunks; pixels outside the image and channels >= C_in of a ragged last set are zeros written by the loader;
//   * contraction index k = tap * span + c, padded ONCE at the end to a multiple of 32: the 8 consecutive k of a lane of
//     v_mfma_f32_16x16x32_f16 lie inside one tap (span % 8 == 0), so its B operand is ONE 16-byte LDS read at the tap's pixel
//     shift (S halo pixels per output pixel); span 16 packs two taps per MFMA (3x3: 5 k-steps).  k >= taps * span reads a zero
//     slot (the halo may hold NaNs; the blob's zeros alone would not do);
//   * a wave owns two tile rows (two 16-pixel fragments) and reuses every weight fragment for both; the shared tile epilogue
//     (slfp_epilogue.hpp) stores 4 consecutive channels per lane, guarded at C_out for a ragged last set.  No atomics.
// NaN: the off-diagonal zeros turn a NaN activation into NaN for every output channel of its group SET (the direct kernel: of
// its group) at the pixels whose window holds it -- the reason the family is opt-in (SLFP_DESC_GROUPED_MFMA, include/slfp.h).
// Single-pass fp16 (SLFP<3,4>) or exact (SFP<3,3>); float32 in, float32 out.
#include <algorithm>
#include "slfp_device.hpp"
#include "slfp_host.hpp"
#include "slfp_epilogue.hpp"

namespace slfp {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));

constexpr int kGrThreads = 256;
constexpr int kGrTH = 8, kGrTW = 16;              // output tile: wave w owns rows 2w and 2w + 1
constexpr int kGrTabBytes = (kEncEntries * 8 + 15) & ~15;
constexpr size_t kGrLdsMax = 160 * 1024;

struct GroupedParams {
    const float* x;
    const _Float16* w;       // [set][n_tile][k_step][64 lanes][8]
    const float* bias;
    float* y;
    int N, H, W, C, O, KH, KW, S, ph, pw, Ho, Wo;
    int span, ow;            // channels a set reads / writes
    int n_sets, sw, n_chunks;   // sets; sets per workgroup; workgroup channel chunks = ceil(n_sets / sw)
    int ksteps, taps;
    int tiles_h, tiles_w, walkers;   // walkers: workgroups that share the tiles of one (image, chunk)
    int IH, IW, pitch, cq, n_items;  // halo: rows, pixels per row, bytes per pixel, float4 per pixel, float4 per halo
    uint32_t m_cq, m_iw;     // ceil(2^20 / cq), ceil(2^20 / IW): exact quotients of the loader's (small) indices
    uint32_t off_koff, off_w, off_x;   // LDS: table | zero slot | k-offsets | weights | halo
    float s1, s2, s1x;
    PostOp post;
    uint32_t nblocks;
    EncArgs enc;             // kEncF16P table of (Ka, format)
};

template <int NT>
__global__ __launch_bounds__(kGrThreads) void k_grouped(const GroupedParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* stab = smem;
    unsigned char* szero = smem + kGrTabBytes;             // 16 zero bytes: the operand of k >= taps * span
    int* skoff = reinterpret_cast<int*>(smem + p.off_koff);   // [k_step][lane-quarter]: byte offset of (tap shift, channel) or -1
    unsigned char* swt = smem + p.off_w;
    unsigned char* tile = smem + p.off_x;

    uint32_t b = xcd_remap(blockIdx.x, p.nblocks);   // walkers of one (image, chunk) are neighbours: shared halo rows in one L2
    const int wk = b % p.walkers; b /= p.walkers;
    const int chunk = b % p.n_chunks;
    const int n = b / p.n_chunks;
    const int set0 = chunk * p.sw;
    const int sets_here = min(p.sw, p.n_sets - set0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, kq = lane >> 4;

    // ---- once per workgroup: table, zero slot, k-offsets, the sets' weights (published by the first tile's barrier)
    enc_fill<kGrThreads>(reinterpret_cast<uint2*>(stab), p.enc);
    if (threadIdx.x < 4) reinterpret_cast<uint32_t*>(szero)[threadIdx.x] = 0u;
    for (int i = threadIdx.x; i < p.ksteps * 4; i += kGrThreads) {
        const int k0 = i * 8;   // (k_step * 4 + lane-quarter) * 8
        const int tap = k0 / p.span, c = k0 - tap * p.span;
        const int kh = tap / p.KW, kw = tap - kh * p.KW;
        skoff[i] = tap < p.taps ? (kh * p.IW + kw) * p.pitch + c * 2 : -1;
    }
    {
        const size_t per_set = (size_t)NT * p.ksteps * 64;   // 16-byte pieces
        const u32x4* src = reinterpret_cast<const u32x4*>(p.w) + (size_t)set0 * per_set;
        const int n16 = sets_here * (int)per_set;
        for (int i = threadIdx.x; i < n16; i += kGrThreads) reinterpret_cast<u32x4*>(swt)[i] = src[i];
    }

    const int c0 = set0 * p.span;
    const float* xn = p.x + (size_t)n * p.H * p.W * p.C;
    const float r1 = p.enc.r1, lo = p.enc.lo, hi = p.enc.hi;
    int pixbase[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) pixbase[i] = (((wave * 2 + i) * p.S) * p.IW + col * p.S) * p.pitch;

    const int n_tiles = p.tiles_h * p.tiles_w;
    for (int t = wk; t < n_tiles; t += p.walkers) {
        const int th = t / p.tiles_w, tw = t - th * p.tiles_w;
        const int h0 = th * kGrTH * p.S - p.ph, w0 = tw * kGrTW * p.S - p.pw;
        __syncthreads();   // first tile: the tables; later tiles: every wave has read the previous halo

        // ---- halo: float32, 16-byte loads (always issued, clamped: a load under a divergent branch is waited for at once),
        // quantizer on load, fp16 to LDS
        constexpr int U = 4;
        for (int base = threadIdx.x; base < p.n_items; base += kGrThreads * U) {
            float4 v[U];
            int dst[U];
            bool inb[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t item = (uint32_t)(base + u * kGrThreads);
                const uint32_t pix = (item * p.m_cq) >> 20, q = item - pix * (uint32_t)p.cq;
                const uint32_t a = (pix * p.m_iw) >> 20, cc = pix - a * (uint32_t)p.IW;
                const int gh = h0 + (int)a, gw = w0 + (int)cc, ch = c0 + (int)q * 4;
                const bool live = item < (uint32_t)p.n_items;
                inb[u] = live && (unsigned)gh < (unsigned)p.H && (unsigned)gw < (unsigned)p.W && ch < p.C;
                dst[u] = live ? (int)(pix * (uint32_t)p.pitch + q * 8u) : -1;
                v[u] = ld_stream4<SLFP_NT_DENSE>(xn + (inb[u] ? (gh * p.W + gw) * p.C + ch : 0));   // < 2^30 (grouped_applicable)
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                uint2 e = enc4_f16(v[u], r1, lo, hi, stab);
                if (!inb[u]) e = make_uint2(0u, 0u);
                if (dst[u] >= 0) *reinterpret_cast<uint2*>(tile + dst[u]) = e;
            }
        }
        __syncthreads();

        // ---- the sets of this workgroup, one after the other: K = taps * span, NT channel tiles, two pixel fragments
        const int ow_ = tw * kGrTW + col;
        for (int sl = 0; sl < sets_here; ++sl) {
            const unsigned char* ws = swt + (size_t)sl * NT * p.ksteps * 1024 + lane * 16;
            const unsigned char* xs = tile + sl * p.span * 2;
            floatx4 acc[2][NT];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
            for (int ks = 0; ks < p.ksteps; ++ks) {
                const int ko = skoff[ks * 4 + kq];
                half8 wf[NT], xf[2];
#pragma unroll
                for (int j = 0; j < NT; ++j) wf[j] = *reinterpret_cast<const half8*>(ws + (size_t)(j * p.ksteps + ks) * 1024);
#pragma unroll
                for (int i = 0; i < 2; ++i) xf[i] = *reinterpret_cast<const half8*>(ko >= 0 ? xs + pixbase[i] + ko : szero);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[j], xf[i], acc[i][j], 0, 0, 0);
            }
            // epilogue: a lane holds 4 consecutive channels of its pixel in each fragment
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int ch = (set0 + sl) * p.ow + j * 16 + kq * 4;
                if (ch >= p.O) continue;   // ragged last set
                const float4 bq = bias_q256(p.bias, ch, p.s1, p.s2);
                const PostVec pv = post_load(p.post, ch);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int oh = th * kGrTH + wave * 2 + i;
                    if (oh >= p.Ho || ow_ >= p.Wo) continue;
                    const float4 r = epilogue(acc[i][j], bq, p.s1x, p.s2);
                    st_stream4<SLFP_NT_DENSE>(p.y + (((size_t)n * p.Ho + oh) * p.Wo + ow_) * p.O + ch, post_apply_v(r, p.post, pv));
                }
            }
        }
    }
}

// ---- host side: one selection (grouped_select) behind the plan, the blob, the launch and the debug name -----------------
static int gcd_i(int a, int b) { return b ? gcd_i(b, a % b) : a; }

bool grouped_select(const slfp_conv2d_desc& d, int passes, int fmt_act, GroupedSel* s) {
    if (d.groups <= 1 || d.c_in % d.groups || d.c_out % d.groups) return false;
    if (d.dil_h != 1 || d.dil_w != 1 || d.stride_h != d.stride_w || d.stride_h < 1 || d.stride_h > 2) return false;
    if (d.kh < 1 || d.kh > 5 || d.kw < 1 || d.kw > 5 || d.pad_h >= d.kh || d.pad_w >= d.kw) return false;
    if (passes != 1) return false;   // SLFP_MFMA_F16X3 stays on the direct kernel
    const int64_t cg = d.c_in / d.groups, og = d.c_out / d.groups;
    if (cg % 4 || og % 4 || cg > 64 || og > 64) return false;
    const int gs = 16 / gcd_i((int)og, 16);
    const int span = gs * (int)cg, ow = gs * (int)og;
    if (span % 8 || span > 64 || ow > 64) return false;
    if ((int64_t)d.h * d.w * d.c_in >= (1ll << 30)) return false;   // 32-bit element offsets inside one image
    if (!act_table(d.ka, fmt_act, kEncF16P)) return false;           // the quantizer on load is the threshold table
    s->gs = gs; s->span = span; s->ow = ow; s->nt = ow / 16;
    s->n_sets = (int)ceil_div(d.groups, gs);
    s->taps = (int)(d.kh * d.kw);
    s->ksteps = (int)ceil_div((int64_t)s->taps * span, 32);
    s->sw = std::min((int)ceil_div(32, span), s->n_sets);   // adjacent sets until a halo pixel is a run of >= 128 B
    s->ih = (kGrTH - 1) * d.stride_h + (int)d.kh;
    s->iw = (kGrTW - 1) * d.stride_w + (int)d.kw;
    const int chunks16 = s->sw * span / 8;
    s->pitch = (chunks16 | 1) * 16;                         // odd number of 16-byte chunks: consecutive pixels on distinct bank groups
    s->off_koff = kGrTabBytes + 16;
    s->off_w = s->off_koff + (uint32_t)((s->ksteps * 16 + 15) & ~15);
    s->off_x = s->off_w + (uint32_t)s->sw * s->nt * s->ksteps * 1024u;
    s->lds = (size_t)s->off_x + (size_t)s->ih * s->iw * s->pitch;
    return s->lds <= kGrLdsMax;   // the sets' weights plus one halo tile
}

bool grouped_applicable(const slfp_conv2d_desc& d, int passes, int fmt_act) {
    GroupedSel s;
    return grouped_select(d, passes, fmt_act, &s);
}

// walkers per (image, chunk): as many as give the launch ~8 workgroups per CU, so that a workgroup's weight load serves several tiles
static int grouped_walkers(const slfp_conv2d_desc& d, const ConvPlan& plan, const GroupedSel& s) {
    const int64_t tiles = ceil_div(plan.h_out, kGrTH) * ceil_div(plan.w_out, kGrTW);
    const int64_t chunks = ceil_div(s.n_sets, s.sw);
    return (int)std::min<int64_t>(tiles, std::max<int64_t>(1, ceil_div(2048, d.n * chunks)));
}

const char* grouped_variant_name(const slfp_conv2d_desc& d, const ConvPlan& plan) {
    static thread_local char buf[64];
    GroupedSel s;
    if (plan.family != kGroupedMfma || !grouped_select(d, plan.passes, plan.fmt_act, &s)) return "none";
    snprintf(buf, sizeof buf, "gs%d/sp%d/nt%d/ks%d/sw%d/wk%d", s.gs, s.span, s.nt, s.ksteps, s.sw, grouped_walkers(d, plan, s));
    return buf;
}

int launch_grouped(const slfp_conv2d_desc& d, const ConvPlan& plan, const float* x, const void* wblob, const float* bias,
                   const PostOp& post, float* y, hipStream_t stream) {
    GroupedSel s;
    if (!grouped_select(d, plan.passes, plan.fmt_act, &s)) return fail(SLFP_ERR_UNSUPPORTED, "grouped MFMA conv: layer outside the family");
    GroupedParams p;
    p.x = x; p.w = reinterpret_cast<const _Float16*>(wblob); p.bias = bias; p.y = y; p.post = post;
    p.N = (int)d.n; p.H = (int)d.h; p.W = (int)d.w; p.C = (int)d.c_in; p.O = (int)d.c_out;
    p.KH = (int)d.kh; p.KW = (int)d.kw; p.S = d.stride_h; p.ph = d.pad_h; p.pw = d.pad_w;
    p.Ho = (int)plan.h_out; p.Wo = (int)plan.w_out;
    p.span = s.span; p.ow = s.ow; p.n_sets = s.n_sets; p.sw = s.sw; p.n_chunks = (int)ceil_div(s.n_sets, s.sw);
    p.ksteps = s.ksteps; p.taps = s.taps;
    p.tiles_h = (int)ceil_div(p.Ho, kGrTH); p.tiles_w = (int)ceil_div(p.Wo, kGrTW);
    p.walkers = grouped_walkers(d, plan, s);
    p.IH = s.ih; p.IW = s.iw; p.pitch = s.pitch; p.cq = s.sw * s.span / 4; p.n_items = s.ih * s.iw * p.cq;
    p.m_cq = ((1u << 20) + (uint32_t)p.cq - 1u) / (uint32_t)p.cq;
    p.m_iw = ((1u << 20) + (uint32_t)p.IW - 1u) / (uint32_t)p.IW;
    p.off_koff = s.off_koff; p.off_w = s.off_w; p.off_x = s.off_x;
    p.s1 = plan.s1; p.s2 = plan.s2; p.s1x = plan.s1 * (1.0f / 256.0f);
    p.enc = *act_table(d.ka, plan.fmt_act, kEncF16P);
    const int64_t nblocks = (int64_t)p.N * p.n_chunks * p.walkers;
    if (nblocks > 0x7FFFFFFF) return fail(SLFP_ERR_UNSUPPORTED, "grouped MFMA conv: grid too large");
    p.nblocks = (uint32_t)nblocks;
    auto fn = s.nt == 1 ? k_grouped<1> : s.nt == 2 ? k_grouped<2> : s.nt == 3 ? k_grouped<3> : k_grouped<4>;
    const int rc = raise_lds_limit(reinterpret_cast<const void*>(fn), kGrLdsMax);   // once per (device, kernel)
    if (rc != SLFP_OK) return rc;
    hipLaunchKernelGGL(fn, dim3(p.nblocks), dim3(kGrThreads), s.lds, stream, p);
    return check_launch("slfp grouped MFMA conv kernel");
}

}  // namespace slfp
