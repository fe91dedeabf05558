// conv_dw_core.hpp -- what the depthwise 3x3 kernels share, written once (gfx950): conv_dw.hip (k_dw3x3), conv_dw2.hip (k_dw3x3_tile),
// conv_dw3.hip (k_dw3x3_rows), conv_dwc.hip (k_dwc) and, through conv_dwpw_core.hpp, the depthwise stage of the two block kernels.
// The arithmetic these steps carry out is stated once, in include/slfp.h next to slfp_debug_dw3x3_instance.
//
// Everything is __device__ __forceinline__, constexpr or inline.  A kernel calls a step only where that leaves every .amdhsa_*
// directive of every instance where it was (profiles/compare_kernels.py); DESIGN.md section 36 lists the spans that stay spelled out
// in their files for that reason.  k_dw3x3 (DwVec<V> lanes of 2 or 4 floats, a bias) shares the constants and the host steps only.
#pragma once
#include "slfp_device.hpp"
#include "slfp_enc.hpp"
#include "slfp_host.hpp"

namespace slfp {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));   // slfp_epilogue.hpp declares the same type under the same name

// Byte offsets outside every buffer descriptor of the family (the load returns 0, the store is dropped).  All three rely on the limit
// the *_applicable / *_select functions enforce: a descriptor spans at most 2^30 bytes (float32 kernels: one image; code kernels: the tensor).
constexpr uint32_t kDwOob = 0xFFFFFFF0u;      // past everything, on its own
constexpr uint32_t kDwBadRow = 0x80000000u;   // offsets built as row part + column part (each < 2^30 when valid): either marker
constexpr uint32_t kDwBadCol = 0x40000000u;   // puts the sum at or beyond 2^30 whatever the other part is
constexpr int kDwTabBytes = (kEncEntries * 8 + 15) & ~15;   // LDS bytes of one threshold table (slfp_enc.hpp)

__device__ __forceinline__ __amdgpu_buffer_rsrc_t dw_rsrc(const void* base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}

// ---------------------------------------------------------------------------- device steps: a lane owns channels c .. c + 3
// The 9 taps, wq = [9][C].  I (uint32_t | size_t) is the width of the index arithmetic, given with C: each kernel keeps the one it
// had (the other is 9 to 13 instructions longer or shorter, and the 64-bit form moves an SGPR count of k_dw3x3_rows).
template <typename I>
__device__ __forceinline__ void dw_load_taps(f32x4 (&wt)[9], const float* wq, const I C, const int c) {
#pragma unroll
    for (int k = 0; k < 9; ++k) wt[k] = *reinterpret_cast<const f32x4*>(wq + ((I)k * C + (I)c));
}

// The folded BatchNorm pair; (1, 0) without POST.
template <bool POST>
__device__ __forceinline__ void dw_load_bn(f32x4& psc, f32x4& psh, const float* scale, const float* shift, const int c) {
    psc = f32x4{1.f, 1.f, 1.f, 1.f}; psh = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (POST) { psc = *reinterpret_cast<const f32x4*>(scale + c); psh = *reinterpret_cast<const f32x4*>(shift + c); }
}

// The lane's NI raw halo quads through the threshold table at `tab` into the float32 LDS tile, STEP bytes apart from dst.  Q(0) == 0, so
// padding and dead slots take the same path; NaN in -> NaN out by a cold patch, never taken on real activations.
template <int NI, int STEP>
__device__ __forceinline__ void dw_put_halo(unsigned char* dst, const f32x4 (&v)[NI], float r1, float lo, float hi, const unsigned char* tab) {
    bool any_nan = false;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const float4 xi = make_float4(v[i][0], v[i][1], v[i][2], v[i][3]);
        any_nan |= enc_has_nan4(xi);
        *reinterpret_cast<float4*>(dst + i * STEP) = enc4_f32_raw(xi, r1, lo, hi, tab);
    }
    if (__builtin_expect(any_nan, 0)) {
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (v[i][e] != v[i][e]) reinterpret_cast<uint32_t*>(dst + i * STEP)[e] = kBitsQNaN;
    }
}

// The window product: nine fmaf per channel from +0 in (kh, kw) order; tap(kh, kw) gives the operand quad, from registers or LDS.
template <typename Tap>
__device__ __forceinline__ f32x4 dw_mac9(const f32x4 (&wt)[9], Tap&& tap) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const f32x4 a = tap(kh, kw);
            const f32x4 w = wt[kh * 3 + kw];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(a[e], w[e], acc[e]);
        }
    }
    return acc;
}

// ... with the operands in an LDS halo tile of 16 pixel slots x 32 channels x float32 per row (ROWB bytes), win: the window's first tap.
// Stride 2 keeps a row's even columns in slots 0..7 and its odd ones in 8..15.
template <int S, int ROWB>
__device__ __forceinline__ f32x4 dw_mac9_lds(const f32x4 (&wt)[9], const unsigned char* win) {
    return dw_mac9(wt, [&](const int kh, const int kw) {
        return *reinterpret_cast<const f32x4*>(win + kh * ROWB + ((S == 1) ? kw : ((kw & 1) * 8 + (kw >> 1))) * 128);
    });
}

// The finish: (acc * Ka) * Kw with the reference's two float32 roundings (utils/conv2d_func.py:24), the folded BatchNorm as one fma
// under POST, the ReLU as one max per element.  k_dwc and the block kernels pass relu = 0 and keep their one branch around four max.
template <bool POST>
__device__ __forceinline__ f32x4 dw_finish(const f32x4 acc, const float ka, const float kw, const f32x4 psc, const f32x4 psh, const int relu) {
    f32x4 rr;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float u = (acc[e] * ka) * kw;
        if constexpr (POST) u = __builtin_fmaf(u, psc[e], psh[e]);
        if (relu) u = fmaxf(u, 0.f);
        rr[e] = u;
    }
    return rr;
}

// 16 bytes out.  nt (dw_nt_out) for outputs the 256 MiB Infinity Cache cannot hold anyway: the store then does not displace what the
// next kernel reads; smaller outputs are stored normally so that the layer that consumes them finds them in the cache.
__device__ __forceinline__ void dw_store16(const f32x4 r, const __amdgpu_buffer_rsrc_t ry, const uint32_t so, const int nt) {
    if (nt) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, r), ry, so, 0, 2);
    else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, r), ry, so, 0, 0);
}

// ---------------------------------------------------------------------------- host steps
// The geometry and scale fields DwParams, Dw2Params, DwrParams and DwcParams name alike; no base struct: the argument blocks stay as they are.
template <typename P>
inline void dw_fill_geom(P& p, const slfp_conv2d_desc& d, const ConvPlan& plan) {
    p.N = (int)d.n; p.H = (int)d.h; p.W = (int)d.w; p.C = (int)d.c_in;
    p.Ho = (int)plan.h_out; p.Wo = (int)plan.w_out; p.pad = d.pad_h;
    p.ka = d.ka; p.kw = d.kw_scale;
}

// Whether a float32 output of `bytes` takes nt stores: SLFP_NT_DW bit 1 enables it, SLFP_DW_NT_MIN_MB (experiment; 0 = always) moves the threshold.
inline int dw_nt_out(int64_t bytes) { return ((SLFP_NT_DW & 2) && bytes >= ((int64_t)switches().dw_nt_min_mb << 20)) ? 1 : 0; }

inline int dw_grid_check(int64_t workgroups, const char* who) {   // who: "dw3x3", "dw3x3 (rows)", ... as in the family's error texts
    return workgroups > 0x7FFFFFFF ? fail(SLFP_ERR_UNSUPPORTED, "%s: grid too large", who) : SLFP_OK;
}
// Launches what a launcher's instance lookup returned for its selection; nullptr: no such instance (sel_name: the selection's string).
template <typename... KArgs, typename... Args>
inline int dw_launch(void (*fn)(KArgs...), const char* who, const char* sel_name, uint32_t nblocks, int threads, size_t lds,
                     hipStream_t stream, const char* what, const Args&... args) {
    if (!fn) return fail(SLFP_ERR_UNSUPPORTED, "%s: no kernel instance for %s", who, sel_name);
    hipLaunchKernelGGL(fn, dim3(nblocks), dim3(threads), lds, stream, args...);
    return check_launch(what);
}

}  // namespace slfp
