// conv_pw_core.hpp -- what the pointwise (1x1) kernels of conv_pw.hip (float32 in) and conv_pw_codes.hip (1-byte codes in) share,
// written once (gfx950): the steps that do not depend on how the B operand is made.  Each file keeps its kernels, its input path
// (encode / decode), its W loader and its selection; conv_pw_params.hpp (also read by pool_avg.hip and linear_fc.hip) stays as it is.
//
// Device steps are __device__ __forceinline__ and take the parameter struct as `const P&`: PwParams and PwcParams keep their layouts
// (a compact second table against a full one; the 4 KiB argument segment is why).  A kernel calls a step only where that leaves every
// .amdhsa_* directive and every MFMA, vector-memory and LDS instruction count of every instance where it was
// (profiles/compare_kernels.py); DESIGN.md section 37 lists the spans that stay spelled out in both files for that reason.
// The diagnostic macros of k_pw_tiled (SLFP_ABL_*, SLFP_PW_STAMPS*) stay in conv_pw.hip: no step here carries one.
#pragma once
#include "slfp_codes.hpp"
#include "conv_pw_params.hpp"

namespace slfp {

constexpr int kStreamThreads = 512;   // k_pw_stream / k_pwc_stream: 8 waves, a wave's unit of work is 16 pixels

// ---------------------------------------------------------------------------- device steps
// element offset of input pixel row m (strided 1x1 reads pixel (oh*S, ow*S))
template <typename P>
__device__ __forceinline__ size_t x_row_offset(const P& p, int64_t m) {
    if (p.S == 1) return (size_t)m * p.K;
    const int64_t hw = (int64_t)p.Ho * p.Wo;
    const int64_t img = m / hw, r = m - img * hw;
    const int oh = (int)(r / p.Wo), ow = (int)(r - (int64_t)oh * p.Wo);
    return (size_t)(((img * p.H) + (int64_t)oh * p.S) * p.W + (int64_t)ow * p.S) * p.K;
}

// per-channel epilogue vectors -> LDS once per workgroup: [256 * bias/s1/s2 | post scale | post shift] of channels n_lo .. n_lo +
// n_ch - 1 (n_ch: the blob's padded channel count, or a slice of it).  Read from global inside the sweep, the loads (and the 12 bias
// divisions) sit on the critical path of every 16-byte store: +12-38 % on these layers (bench.py --post).
template <int THREADS, typename P>
__device__ __forceinline__ void pw_fill_ep(float* ep, const P& p, const int n_lo, const int n_ch) {
    for (int i = threadIdx.x; i < n_ch; i += THREADS) {
        const bool in = n_lo + i < p.N;
        ep[i] = (p.bias && in) ? bias_q256_1(p.bias[n_lo + i], p.s1, p.s2) : 0.f;
        ep[n_ch + i] = (p.post.scale && in) ? p.post.scale[n_lo + i] : 1.f;
        ep[2 * n_ch + i] = (p.post.scale && in) ? p.post.shift[n_lo + i] : 0.f;
    }
}

// Finish of one accumulator tile of the LDS-resident kernels: channels n .. n + 3 of the ep vectors (has_vec: bias and/or fused BN,
// wave-uniform; all three vectors from LDS).  LAYEROUT: the float32-input kernels' layer-output quantizer (no such quantizer in front
// of a code output: refused on the host).  RELU: off with a residual (the ReLU follows the add, res_add) and with code output (it is
// the code quantizer's, enc4_code_relu).
template <bool RELU, bool LAYEROUT, typename P>
__device__ __forceinline__ float4 pw_finish(const floatx4 acc, const P& p, const float* ep, const int n_ch, const int n, const bool has_vec) {
    float4 r;
    if (has_vec) {
        const float4 bq = *reinterpret_cast<const float4*>(ep + n);
        const float4 sc = *reinterpret_cast<const float4*>(ep + n_ch + n);
        const float4 sh = *reinterpret_cast<const float4*>(ep + 2 * n_ch + n);
        r = epilogue(acc, bq, p.s1x, p.s2);
        if (p.post.scale) {
            r = affine4(r, sc, sh);
            if constexpr (LAYEROUT) {
                if (p.post.layerout) r = layerout4(r);
            }
        }
    } else {
        r = epilogue(acc, make_float4(0.f, 0.f, 0.f, 0.f), p.s1x, p.s2);
    }
    if constexpr (RELU) {
        if (p.post.relu) r = relu4(r);
    }
    return r;
}

// The LDS-resident sweep of one channel tile: wj = the tile's first W fragment (this lane's 16 bytes), lo_plane = halves from the hi
// plane to the lo plane.  Three passes issue (w_lo, x_hi), (w_hi, x_lo), (w_hi, x_hi) per k-step: both files' kernels, bit for bit.
template <int PASSES, int KS, int KL>
__device__ __forceinline__ floatx4 pw_sweep_lds(const _Float16* wj, const size_t lo_plane, const half8 (&xh)[KS], const half8 (&xl)[KL]) {
    floatx4 acc = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const half8 wh = *reinterpret_cast<const half8*>(wj + ks * 512);
        if constexpr (PASSES == 3) {
            const half8 wl = *reinterpret_cast<const half8*>(wj + lo_plane + ks * 512);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, xh[ks], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xl[ks], acc, 0, 0, 0);
        }
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xh[ks], acc, 0, 0, 0);
    }
    return acc;
}

// Code output of the LDS-resident kernels, one group of four channel tiles j0 .. j0 + 3 (tile(j): the finished float4 of tile j; the
// DUAL forms add the residual and store the float32 value inside it): the four code dwords go through rows_transpose4 and every lane
// stores 16 consecutive channel codes of its pixel.  yr: the pixel's codes of channel n_lo; after the transpose lane-quarter kq holds
// channels 16 (j0 + kq) + 0..15.
template <bool LUTQ, bool NANFIX, typename Tile, typename TAB = const unsigned char*>
__device__ __forceinline__ void pw_codes16_out(const int j0, uint8_t* yr, const bool live, const int n_lo, const int N, const int kq,
                                               const CodeQuant& cq, const unsigned char* enc_tab, Tile&& tile, TAB lut_tab = nullptr) {
    uint32_t c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float4 r = tile(j0 + j);
        c[j] = code4<LUTQ, NANFIX>(r, cq, enc_tab, lut_tab);
    }
    const int n = (j0 + kq) * 16;
    store_codes16(c, yr + n, live && n_lo + n < N);
}

// ---- the tiled kernels (k_pw_tiled, k_pwc_tiled): a workgroup owns BM pixels x BN channels, WM x WN waves of MT x NT 16 x 16 tiles.
// Only steps that take and return plain values are here: forms that take the kernels' register arrays (acc, wh / wl, src, wsoff) by
// reference, or a tile functor, moved register counts of k_pw_tiled / k_pwc_tiled instances.
template <int WM, int WN, int MT, int NT = 4>
struct PwTile {
    static constexpr int kWM = WM, kWN = WN, kMT = MT;
    static constexpr int T = 64 * WM * WN;     // threads
    static constexpr int BM = WM * MT * 16;    // pixel rows
    static constexpr int BN = WN * NT * 16;    // channels
    static constexpr int NLD = BM * 16 / T;    // 4-element pieces (float4 / code dword) per thread per 64-deep stage
    static constexpr int XBYTES = BM * 128;    // one plane of one X buffer: BM rows of 64 fp16
    static_assert(BM * 16 % T == 0, "staging must divide evenly");
};

// Staging: piece #i of a thread covers row (tid>>4) + i*(T/16) of the workgroup's tile; the element offset of that row's pixel in x.
// Every global load in the main loop is UNCONDITIONAL, so rows are clamped here and never stored.
template <int T, typename P>
__device__ __forceinline__ size_t pw_stage_row_offset(const P& p, const int64_t m0, const int i) {
    const int row = (threadIdx.x >> 4) + i * (T / 16);
    int64_t m = m0 + (row < p.rb ? row : p.rb - 1);  // padding rows of the tile re-read its last row (L1 hits) ...
    m = m < p.M ? m : p.M - 1;                       // ... and rows past the end the last pixel: computed and dropped
    return x_row_offset(p, m);
}

// W fragments (fragment (n-tile, k-step): 1 KiB, lane-linear) by buffer loads: a descriptor over one plane of the blob + per-tile byte
// offsets in scalar registers (the caller makes the wave's first tile uniform for the compiler with readfirstlane; padded tiles clamp
// to the last real one), ONE vector register of address (lane * 16) for all of them (8 address registers less than per-tile pointers).
template <typename P>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t pw_w_rsrc(const _Float16* plane, const P& p) {
    const uint64_t wbytes = (uint64_t)p.n_tiles * p.KS * 1024;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(plane), 0, (uint32_t)(wbytes > 0xFFFFFFFFull ? 0xFFFFFFFFull : wbytes), 0x00020000);
}
template <typename P>
__device__ __forceinline__ uint32_t pw_w_offset(const P& p, const int ntile) {
    const int nt = ntile < p.n_tiles ? ntile : p.n_tiles - 1;
    return (uint32_t)nt * (uint32_t)p.KS * 1024u;
}

// fused BN/ReLU: this workgroup's BN-channel slices of scale / shift go through the (now free) X tile
// in LDS, so the store loop reads them with two ds_read_b128 instead of two global loads per store
// (those sat on the critical path of every store: +13 % on these layers).  Between two barriers of the caller's.
template <int BN, int T>
__device__ __forceinline__ void pw_bn_slice_fill(float* lsc, float* lsh, const float* scale, const float* shift, const int N, const int n_lo) {
    for (int i = threadIdx.x; i < BN; i += T) {
        const bool in = n_lo + i < N;
        lsc[i] = in ? scale[n_lo + i] : 1.f;
        lsh[i] = in ? shift[n_lo + i] : 0.f;
    }
}

// Finish of one accumulator tile of the tiled kernels: channels n .. n + 3, scale / shift from the LDS slices that start at channel
// n_lo.  Channel tiles past C_out are computed from clamped weights and never stored.  RELU, LAYEROUT: as pw_finish.
template <bool RELU, bool LAYEROUT, typename P>
__device__ __forceinline__ float4 pw_tile_finish(const floatx4 acc, const P& p, const int n, const int n_lo, const float* lsc, const float* lsh) {
    const bool in = n < p.N;
    float4 r = epilogue(acc, bias_q256(in ? p.bias : nullptr, n, p.s1, p.s2), p.s1x, p.s2);
    if (p.post.scale) {
        const float4 sc = *reinterpret_cast<const float4*>(lsc + (in ? n - n_lo : 0));
        const float4 sh = *reinterpret_cast<const float4*>(lsh + (in ? n - n_lo : 0));
        r = affine4(r, sc, sh);
        if constexpr (LAYEROUT) {
            if (p.post.layerout) r = layerout4(r);
        }
    }
    if constexpr (RELU) {
        if (p.post.relu) r = relu4(r);
    }
    return r;
}

// ---------------------------------------------------------------------------- host steps
inline const char* pw_fmt_word(int fmt) { return fmt == kFmtSfp7 ? "sfp7" : "act8"; }

// The tiled kernels' tiling by C_out (NT = 4 throughout): the widest channel tile, fewest re-reads / re-encodes of X.  (Narrower
// tiles for the small-M, deep-K layers of ResNet-50's last stages -- 49-196 pixel tiles at batch 64 -- were measured: more
// workgroups, but the redundant encode costs more than the idle CUs did.)  wide_ok: whether the caller has the 8-wave form; the
// three-pass forms of both files do not (they hold the lo fragments in registers, which the 128-VGPR form has no room for).
struct PwTiling {
    int wm, wn, mt;
};
inline PwTiling pw_tiling(int N, bool wide_ok) {
    if (N > 256 && wide_ok) return {1, 8, 4};   // 64 px x 512 ch, 8 waves, 2 workgroups/CU
    if (N > 128) return {1, 4, 4};              // 64 px x 256 ch
    if (N > 64) return {2, 2, 2};               // 64 px x 128 ch
    return {4, 1, 1};                           // 64 px x  64 ch
}
// ... and from a selection's (wm, wn, mt) to the instance: f(PwTile<WM, WN, MT>{}) returns the kernel pointer (nullptr: no instance).
template <bool WIDE_OK, typename F>
inline auto pw_tiling_instance(int wm, int wn, int mt, F&& f) -> decltype(f(PwTile<1, 4, 4>{})) {
    const int t = wm * 100 + wn * 10 + mt;
    if constexpr (WIDE_OK) {
        if (t == 184) return f(PwTile<1, 8, 4>{});
    }
    if (t == 144) return f(PwTile<1, 4, 4>{});
    if (t == 222) return f(PwTile<2, 2, 2>{});
    if (t == 411) return f(PwTile<4, 1, 1>{});
    return nullptr;
}

// What every pointwise launch takes from the descriptor and the plan, whatever the element type of x.
template <typename P>
inline void pw_fill_geom(P& p, const slfp_conv2d_desc& d, const ConvPlan& plan) {
    p.K = (int)d.c_in; p.N = (int)d.c_out;
    p.KS = (int)(plan.k_pad / 32);
    p.n_tiles = (int)(plan.n_pad / 16);
    p.H = (int)d.h; p.W = (int)d.w; p.Ho = (int)plan.h_out; p.Wo = (int)plan.w_out; p.S = d.stride_h;
    p.M = d.n * plan.h_out * plan.w_out;
    p.s1 = plan.s1; p.s2 = plan.s2; p.s1x = plan.s1 * (1.0f / 256.0f);
}

// Launch of a stream kernel (persistent grid): as many workgroups per CU as LDS and registers allow (<= 4), on every CU of the
// device, no more than there are 16-pixel units, and no more than grid_cap (SLFP_PW_GRID: several trips of the persistent loop at
// small shapes; 0: no cap).  lds: the dynamic part; the tables are static LDS.
template <typename P>
inline int pw_launch_stream(void (*fn)(const P), const P& p, size_t lds, int grid_cap, hipStream_t stream, const char* what) {
    int rc = raise_lds_limit(reinterpret_cast<const void*>(fn), lds);
    if (rc != SLFP_OK) return rc;
    int per_cu = resident_blocks_per_cu(reinterpret_cast<const void*>(fn), kStreamThreads, lds);
    per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);
    const int64_t groups = (p.M + 15) / 16;
    int64_t grid = (int64_t)device_cu_count() * per_cu;
    const int64_t need = ceil_div(groups, kStreamThreads / 64);
    if (grid > need) grid = need;
    if (grid_cap > 0 && grid > grid_cap) grid = grid_cap;
    hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(kStreamThreads), lds, stream, p);
    return check_launch(what);
}

// Launch of a tiled kernel: the grid fields of p, the LDS size (dynamic part: the X double buffer of `passes` planes, and the
// per-wave staging area of the staged float32 epilogue) and the launch.  who: "pointwise", "pointwise (codes)" as in the error texts.
// (Workgroups that own fewer rows than their tile -- 49 = a quarter image instead of 64, for an integral number of
// rounds on the 512 resident slots -- were measured: no gain, 61-64 vs 60 us on 512->512.  A workgroup's time is set
// by streaming all of W from L2, not by its rows.)
template <typename P>
inline int pw_launch_tiled(void (*fn)(const P), P& p, const PwTiling& t, int passes, bool staged, hipStream_t stream, const char* who,
                           const char* what) {
    const int BM = t.wm * t.mt * 16, BN = t.wn * 4 * 16, T = 64 * t.wm * t.wn;
    p.n_blocks = (uint32_t)ceil_div((int64_t)p.N, BN);
    p.rb = BM;
    p.m_blocks = (uint32_t)ceil_div(p.M, p.rb);
    const int64_t nblocks = (int64_t)p.m_blocks * p.n_blocks;
    if (nblocks > 0x7FFFFFFF) return fail(SLFP_ERR_UNSUPPORTED, "%s: grid too large", who);
    p.nblocks = (uint32_t)nblocks;
    const size_t lds = (size_t)2 * (passes == 3 ? 2 : 1) * BM * 128 + (staged ? (size_t)(T / 64) * 16 * kStgRow : 0);
    int rc = raise_lds_limit(reinterpret_cast<const void*>(fn), lds);
    if (rc != SLFP_OK) return rc;
    hipLaunchKernelGGL(fn, dim3(p.nblocks), dim3(T), lds, stream, p);
    return check_launch(what);
}

}  // namespace slfp
