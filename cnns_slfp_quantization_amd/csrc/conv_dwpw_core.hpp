// conv_dwpw_core.hpp -- what the two depthwise -> pointwise block kernels share (conv_dwpw.hip: k_dwpw, float32 in and out;
// conv_dwpw_codes.hip: k_dwpw_codes, 1-byte codes in, float32 or codes out), written once (gfx950).
//
//   workgroup (512 threads) = one image x one 14x14 (stride 1) or 7x7 (stride 2) tile of depthwise outputs x ALL channels:
//   phase 1, per 32-channel group: halo tile -> LDS as float32 (the loads of the next group are issued before this group is
//            convolved), 3x3 conv, BN / ReLU, quantize -> fp16 row [pixel][K] in LDS;
//   phase 2: the tile's 13 (4) sixteen-pixel units x all output channels on the matrix cores, W resident in LDS
//            (K * N * 2 B <= 64 KiB), float32 outputs staged to 128-byte pieces (the staging area reuses the halo tile).
//
// Here: the tile geometry and the LDS carve-up (DwPwGeom; the host's LDS size is the same struct's), the parameters both kernels
// take (DwPwBase) with the one host function that fills them, and those device steps that leave every instance's register
// counts where they were when they are called instead of spelled out (profiles/compare_kernels.py compares two builds by kernel
// name).  What each kernel keeps is its input path, the NaN policy of the hand-over quantizer and the output branch, and three
// spans that are the same text in both files because every shared form of them moved a register count of some instance: the W
// copy, voff[] and the staged float32 store.  The depthwise stage's steps are conv_dw_core.hpp's where calling
// them passes the same check (section 36: k_dwpw_codes keeps the tap loop, both keep the tap loads and the ReLU branch spelled out).
// Everything here is __device__ __forceinline__ or constexpr.
#pragma once
#include "slfp_device.hpp"
#include "slfp_enc.hpp"
#include "slfp_host.hpp"
#include "slfp_epilogue.hpp"
#include "conv_dw_core.hpp"

namespace slfp {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int kDwPwT = 512;                      // threads: 64 pixel slots x 8 channel quads in phase 1, 8 waves in phase 2
constexpr int dwpw_th(int s) { return s == 2 ? 7 : 14; }   // tile edge in depthwise outputs

// S: depthwise stride; KS: K / 32 (1, 2, 4); NT: N / 16 channel tiles (4, 8, 16)
template <int S_, int KS_, int NT_>
struct DwPwGeom {
    static constexpr int S = S_, KS = KS_, NT = NT_;
    static constexpr int TH = dwpw_th(S), TW = TH;
    static constexpr int IH = (TH - 1) * S + 3, IW = IH;
    static constexpr int RPL = kDwPwT / 8 / 16;          // halo rows loaded per step (4)
    static constexpr int NI = (IH + RPL - 1) / RPL;
    static constexpr int ROWB = 16 * 32 * 4;
    static constexpr int NPX = TH * TW;                  // depthwise outputs of the tile = pointwise pixels
    static constexpr int NU = (NPX + 15) / 16;           // 16-pixel MFMA units (13 / 4)
    static constexpr int NWV = kDwPwT / 64;
    static constexpr int UW = (NU + NWV - 1) / NWV;      // units per wave
    static constexpr int K = KS * 32;
    static constexpr int XROW = K * 2 + 16;              // bytes per pixel row of the fp16 image (+16: conflict-free fragment reads)
    static constexpr int CW = TW > 8 ? 16 : 8, RPI = (kDwPwT / 8) / CW, NO = (TH + RPI - 1) / RPI;
    // LDS behind the kernel's tables, byte offsets from the end of that prefix
    static constexpr int tile = 0;                       // [RPL * NI rows][16 slots][32 ch] float32; phase 2: [8 waves][2 KiB] staging
    static constexpr int x16 = tile + RPL * NI * ROWB;   // [NU * 16 rows][XROW]
    static constexpr int wl = x16 + NU * 16 * XROW;      // [tile j][k-step][lane] 16 B
    static constexpr int ep = wl + NT * KS * 1024;       // [3][NT * 16] float32
    static constexpr int bytes = ep + 3 * NT * 16 * 4;
};

// DwPwGeom<s, ks, nt>::bytes of a built instance (0: none)
inline size_t dwpw_geom_bytes(int s, int ks, int nt) {
#define SLFP_DWPW_BYTES(SS, KK, NN) if (s == SS && ks == KK && nt == NN) return DwPwGeom<SS, KK, NN>::bytes;
    SLFP_DWPW_INSTANCES(SLFP_DWPW_BYTES)
#undef SLFP_DWPW_BYTES
    return 0;
}

struct DwPwBase {
    const void* x;         // depthwise input, NHWC: float32 (k_dwpw) or codes of QA(. / Ka_dw) (k_dwpw_codes)
    const float* wdw;      // [9][C] quantized depthwise weights (slfp_conv2d_prepare_weights of the dw layer)
    const float* sc1;      // BatchNorm 1 folded: scale / shift [C]
    const float* sh1;
    const _Float16* wpw;   // pointwise blob (hi plane), tile (nt, ks) at (nt * KSb + ks) * 512 halves
    const float* bias2;    // pointwise bias or nullptr
    const float* sc2;      // BatchNorm 2 folded or nullptr
    const float* sh2;
    void* y;               // pointwise output, NHWC: float32, or (k_dwpw_codes, YC) codes of the reader's quantizer
    int N, H, W, C, Ho, Wo, O;   // images, dw input size, channels, dw output size, pointwise channels
    int tiles_h, tiles_w, pad;
    int KSb;               // k-steps per tile in the pointwise blob
    int relu1, relu2;
    float ka1, kw1;        // depthwise scales
    float s1, s2, s1x;     // pointwise epilogue (Ka2, Kw2, Ka2 / 256)
    uint32_t nblocks;
    int fmt_out;           // k_dwpw_codes, YC: format of the output codes (kFmtAct8 | kFmtSfp7), else 0.  Last, where k_dwpw's block had
                           // padding in front of its 8-byte aligned tables: k_dwpw's arguments stay where they were, both blocks keep their size
};

// Fills `p` for the (selected) pair; returns the workgroup count before it is narrowed to p.nblocks.
inline int64_t dwpw_fill_base(DwPwBase& p, const slfp_conv2d_desc* dw, const slfp_conv2d_desc* pw, const ConvPlan& p1, const ConvPlan& p2,
                              const void* x, const void* wprep_dw, const float* post1_scale, const float* post1_shift, int relu1,
                              const void* wprep_pw, const float* bias_pw, const float* post2_scale, const float* post2_shift, int relu2, void* y) {
    p.x = x; p.wdw = reinterpret_cast<const float*>(wprep_dw); p.sc1 = post1_scale; p.sh1 = post1_shift;
    p.wpw = reinterpret_cast<const _Float16*>(wprep_pw); p.bias2 = bias_pw; p.sc2 = post2_scale; p.sh2 = post2_shift; p.y = y;
    p.N = (int)dw->n; p.H = (int)dw->h; p.W = (int)dw->w; p.C = (int)dw->c_in; p.Ho = (int)p1.h_out; p.Wo = (int)p1.w_out; p.O = (int)pw->c_out;
    const int TH = dwpw_th(dw->stride_h);
    p.tiles_h = (int)ceil_div(p.Ho, TH); p.tiles_w = (int)ceil_div(p.Wo, TH); p.pad = dw->pad_h;
    p.KSb = (int)(p2.k_pad / 32);
    p.relu1 = relu1; p.relu2 = relu2;
    p.ka1 = dw->ka; p.kw1 = dw->kw_scale;
    p.s1 = p2.s1; p.s2 = p2.s2; p.s1x = p2.s1 * (1.0f / 256.0f);
    const int64_t nblocks = (int64_t)p.N * p.tiles_h * p.tiles_w;
    p.nblocks = (uint32_t)nblocks;
    p.fmt_out = 0;
    return nblocks;
}

// ---------------------------------------------------------------------------- device steps
// The resident data next to W: the three epilogue vectors (256 * bias / s1 / s2, BatchNorm 2 scale, shift) and the zero rows of
// the fp16 image (rows beyond the tile's pixels)
template <typename G>
__device__ __forceinline__ void dwpw_fill_ep_zero(float* ep, unsigned char* x16, const DwPwBase& p) {
    for (int i = threadIdx.x; i < G::NT * 16; i += kDwPwT) {
        ep[i] = p.bias2 ? bias_q256_1(p.bias2[i], p.s1, p.s2) : 0.f;
        ep[G::NT * 16 + i] = p.sc2 ? p.sc2[i] : 1.f;
        ep[2 * G::NT * 16 + i] = p.sc2 ? p.sh2[i] : 0.f;
    }
    for (int i = threadIdx.x; i < (G::NU * 16 - G::NPX) * (G::XROW / 8); i += kDwPwT)
        reinterpret_cast<uint2*>(x16 + G::NPX * G::XROW)[i] = make_uint2(0u, 0u);
}

// The workgroup's image and tile, and the thread's two phase-1 roles: the halo slot (iw, ihh) it loads and the output slot
// (ow, ohb) it convolves, both for channel quad c4 of the 32-channel group.
struct DwPwIdx {
    uint32_t n;
    int th, tw;
    int c4, iw, ihh, ow, ohb;
    uint32_t lds_w, lds_r0;     // tile offsets: where the halo element is written, where the output's taps start
    bool col_live, ocol_live;   // the halo column is inside the window; the output column is inside the tile
};

template <typename G>
__device__ __forceinline__ DwPwIdx dwpw_index(const DwPwBase& p) {
    constexpr int S = G::S;
    DwPwIdx d;
    const uint32_t lb = xcd_remap(blockIdx.x, p.nblocks);
    const uint32_t tiles_per_img = (uint32_t)(p.tiles_h * p.tiles_w);
    d.n = lb / tiles_per_img;
    const uint32_t tr = lb - d.n * tiles_per_img;
    d.th = (int)(tr / (uint32_t)p.tiles_w);
    d.tw = (int)(tr - (uint32_t)d.th * p.tiles_w);

    d.c4 = threadIdx.x & 7;
    const int slot = threadIdx.x >> 3;
    d.iw = slot & 15;
    d.ihh = slot >> 4;
    const int colslot = (S == 2) ? ((d.iw & 1) * 8 + (d.iw >> 1)) : d.iw;
    d.lds_w = (uint32_t)((d.ihh * 16 + colslot) * 128 + d.c4 * 16);
    d.col_live = d.iw < G::IW;
    d.ow = slot & (G::CW - 1);
    d.ohb = slot / G::CW;
    d.ocol_live = d.ow < G::TW;
    d.lds_r0 = (uint32_t)(((d.ohb * S) * 16 + d.ow) * 128 + d.c4 * 16);
    return d;
}

// The depthwise kernels' finish (conv_dw_core.hpp) of one accumulator quad, psc / psh being the folded BatchNorm 1 of its channels
__device__ __forceinline__ float4 dwpw_bn1(const floatx4 acc, const floatx4 psc, const floatx4 psh, const DwPwBase& p) {
    const floatx4 u = dw_finish<true>(acc, p.ka1, p.kw1, psc, psh, 0);
    float4 r = make_float4(u[0], u[1], u[2], u[3]);
    if (p.relu1) r = relu4(r);   // one branch around four max, as in k_dwc's float32 form: inside the finish it moves VGPR counts here
    return r;
}

// Output quad j of the thread, quantized (q), into the fp16 image (channel group cg)
template <typename G>
__device__ __forceinline__ void dwpw_put_quad(unsigned char* x16, const DwPwIdx& d, const int j, const int cg, const uint2 q) {
    const int oh = d.ohb + j * G::RPI;
    if (d.ocol_live && oh < G::TH)
        *reinterpret_cast<uint2*>(x16 + (uint32_t)(oh * G::TW + d.ow) * G::XROW + (uint32_t)(cg * 64 + d.c4 * 8)) = q;
}

// MFMA B fragment of k-step ks: pixel `col` of unit u (a unit past the tile reads the last one), k-quarter kq
template <typename G>
__device__ __forceinline__ half8 dwpw_frag(const unsigned char* x16, const int u, const int col, const int kq, const int ks) {
    const unsigned char* row = x16 + (uint32_t)((u < G::NU ? u : G::NU - 1) * 16 + col) * G::XROW + kq * 8;
    const u32x2 a = *reinterpret_cast<const u32x2*>(row + ks * 64);
    const u32x2 b = *reinterpret_cast<const u32x2*>(row + ks * 64 + 32);
    return __builtin_bit_cast(half8, u32x4{a[0], a[1], b[0], b[1]});
}

// Channel tile j of one unit: v_mfma_f32_16x16x32_f16 over k in blob order from +0
template <typename G>
__device__ __forceinline__ floatx4 dwpw_mma(const unsigned char* wl, const half8 (&xh)[G::KS], const int j, const int lane) {
    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < G::KS; ++ks) {
        const half8 wf = *reinterpret_cast<const half8*>(wl + (uint32_t)((j * G::KS + ks) * 1024) + lane * 16);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf, xh[ks], acc, 0, 0, 0);
    }
    return acc;
}

}  // namespace slfp

