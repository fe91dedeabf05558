// conv_pw.hip -- SLFP-quantized pointwise (1x1) convolution on the gfx950 matrix cores.
//
// Replaces Conv2d_Q.forward (utils/conv2d_func.py:20-25 / :41-47) for 1x1 kernels,
// groups == 1 (the 13 "pw" layers of MobileNetV1, nets_imgnet/mobilenetv1.py:31; the
// 36 1x1 layers of ResNet-50; Fire squeeze/expand1x1 of SqueezeNet) and Linear_Q (:60-65).
//
// NHWC makes this a plain GEMM  Y^T[N x M] = Wq[N x K] . Xq^T[K x M]  (M = pixels) with
// K contiguous on both operands.  58 flop/B at float32 would be compute-bound on gfx950
// (ridge 19.6 flop/B), so the contraction runs on v_mfma_f32_16x16x32_f16 with float32
// accumulation and the kernels stay HBM-bound (4 B in + 4 B out per element).
//   A operand = W (rows = output channels), B operand = X (columns = pixels): each lane
//   ends up holding 4 CONSECUTIVE output channels of one pixel = one 16-byte NHWC store.
//   W is quantized ONCE per weight update into an MFMA-fragment-ordered fp16 blob
//   (slfp_conv2d_prepare_weights): fragment (n-tile, k-step) is 1 KiB, lane-linear.
//   Inside a 32-deep k-step lane (col, kq) holds k = {kq*4..kq*4+3, 16+kq*4..16+kq*4+3}
//   (any k order is legal as long as A and B agree): a lane's two 16-byte X loads then sit
//   in two 64-byte runs that the wave reads whole.
// Two kernels, chosen by the size of W:
//   k_pw_stream  K*N small enough for W to live in LDS (MobileNetV1 pw1-pw5: 71 % of the
//                pointwise bytes).  Persistent workgroups; a wave's unit of work is 16
//                pixels: it loads their K channels straight into MFMA B fragments
//                (x/Ka + SLFP encode inline, no LDS round trip for X, no barriers), sweeps
//                the W fragments out of LDS, and stores each 16-channel tile as it is done.
//   k_pw_tiled   larger W: a workgroup owns BM pixels x BN channels; X rows are encoded
//                once into a swizzled LDS tile shared by its waves (double-buffered over
//                64-deep K stages), each wave streams the W fragments of its own channels
//                straight from L2.  Ablation (512->512, 0.081 ms): X loads 0.026, stores
//                0.021, W 0.014, encode 0.011, MFMA 0: the pieces add up (serial chain per
//                workgroup), so the tile that maximises co-resident waves won (64 px x 512
//                ch, 8 waves, 126 VGPRs).  Tried and dropped: deeper X register rings, W
//                double-buffering (vmcnt retires in order: a W wait drains younger-issued X
//                loads anyway), a warp-specialised producer/consumer variant (no faster;
//                MT = 7 tiles spill at the 168-VGPR cap of a 12-wave workgroup), and an
//                "X-stationary" variant that separates the phases in time (whole 64 px x K tile
//                burst-loaded and parked in LDS as fp16, then an MFMA sweep with only L2 W loads,
//                two workgroups per CU, optionally persistent with the second resident started
//                half a period late): 0.082 ms non-persistent, 0.097 ms persistent+staggered vs
//                0.076 ms for this kernel on 512->512 @14x14 -- all CUs burst, encode, multiply
//                and store in lockstep and the start offset does not survive the first tile.
// Operand precision: SFP<3,3> values are exact in fp16 (1 pass, exact products).
// SLFP<3,4> values are 2^(m/16) multiples; fp16x1 rounds them to 11 bits (~2.5e-4
// tensor-relative error), fp16x3 splits both operands hi+lo (3 MFMA passes,
// float32-equivalent).  Both operands are pre-scaled by 2^4 (range [2, 245]: the scale
// is folded into the divisor, x/(Ka/16)) so hi is always a normal fp16 and lo keeps 2^-26
// relative precision; the 2^-8 is folded into the first epilogue scale (power-of-two
// scaling commutes with rounding), which keeps the reference's (out * Ka) * Kw roundings.
// Residual operand (slfp_conv2d_fwd_res; the tail of a ResNet block, out = relu(bn3(conv3(h)) + identity)): a compile-time RES
// switch on both kernels' store path adds p.res to the finished value -- one float32 add after the affine's fma, the ReLU
// after it -- with every 16 bytes of the residual loaded in the layout of the store they pair with and requested one tile ahead
// of the values they are added to.  The instantiations without it are unchanged.
// Code output (slfp_conv2d_fwd_entry; the layer at which a chain of 1-byte codes begins): a compile-time YC switch on both kernels
// (single-pass table forms only) turns the finished float4 into 4 code bytes of the CONSUMER's quantizer -- the store path of
// conv_pw_codes.hip under this file's load path: the dwords of four channel tiles go through rows_transpose4 and every lane stores
// 16 consecutive channel codes of its pixel.  The consumer's code table rides in PwParams::enc_lo in compact form (the single-pass
// forms do not use that slot).  The instantiations without it are unchanged.
#include <cstdlib>
#include "slfp_device.hpp"
#include "slfp_enc.hpp"
#include "slfp_codes.hpp"
#include "slfp_host.hpp"
#include "conv_pw_core.hpp"

namespace slfp {

// two float4 (k = kq*4.., 16 + kq*4..) -> one MFMA B fragment through the threshold table; NaNs not patched
__device__ __forceinline__ half8 enc_frag(const float4 a, const float4 b, const EncArgs& e, const unsigned char* tb) {
    const uint2 pa = enc4_f16_raw(a, e.r1, e.lo, e.hi, tb), pb = enc4_f16_raw(b, e.r1, e.lo, e.hi, tb);
    return __builtin_bit_cast(half8, u32x4{pa.x, pa.y, pb.x, pb.y});
}
__device__ __forceinline__ half8 enc_frag_nan(const float4 a, const float4 b, const EncArgs& e, const unsigned char* tb) {
    const uint2 pa = enc4_f16(a, e.r1, e.lo, e.hi, tb), pb = enc4_f16(b, e.r1, e.lo, e.hi, tb);
    return __builtin_bit_cast(half8, u32x4{pa.x, pa.y, pb.x, pb.y});
}

// the same for the three-pass mode: hi and lo fragments from the two tables (NaN: patched by the caller's cold branch)
__device__ __forceinline__ void enc_frag_hl(const float4 a, const float4 b, const EncArgs& e, const unsigned char* tb,
                                            const unsigned char* tl, half8& h, half8& l) {
    uint32_t h0, h1, h2, h3, l0, l1, l2, l3;
    enc2_f16_hl(a.x, a.y, e.r1, e.lo, e.hi, tb, tl, h0, l0);
    enc2_f16_hl(a.z, a.w, e.r1, e.lo, e.hi, tb, tl, h1, l1);
    enc2_f16_hl(b.x, b.y, e.r1, e.lo, e.hi, tb, tl, h2, l2);
    enc2_f16_hl(b.z, b.w, e.r1, e.lo, e.hi, tb, tl, h3, l3);
    h = __builtin_bit_cast(half8, u32x4{h0, h1, h2, h3});
    l = __builtin_bit_cast(half8, u32x4{l0, l1, l2, l3});
}
// NaN inputs of a fragment -> NaN in the hi plane, 0 in the lo plane (what (_Float16)NaN and NaN - NaN... give is NaN either way)
__device__ __forceinline__ void frag_patch_nan(const float4 a, const float4 b, half8& h) {
    const float xs[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (xs[i] != xs[i]) h[i] = (_Float16)__uint_as_float(0x7FC00000u);
}

template <int FMT, int PASSES>
__device__ __forceinline__ void encode4(const float4 v, const ScaleDiv sd, const uint32_t* sT, half4& h, half4& l) {
    const float v0 = quantize_scaled<FMT, 4>(v.x, sd, sT);
    const float v1 = quantize_scaled<FMT, 4>(v.y, sd, sT);
    const float v2 = quantize_scaled<FMT, 4>(v.z, sd, sT);
    const float v3 = quantize_scaled<FMT, 4>(v.w, sd, sT);
    h[0] = (_Float16)v0; h[1] = (_Float16)v1; h[2] = (_Float16)v2; h[3] = (_Float16)v3;
    if constexpr (PASSES == 3) {
        l[0] = (_Float16)(v0 - (float)h[0]); l[1] = (_Float16)(v1 - (float)h[1]);
        l[2] = (_Float16)(v2 - (float)h[2]); l[3] = (_Float16)(v3 - (float)h[3]);
    }
}

__device__ __forceinline__ half8 join(const half4 a, const half4 b) {
    return half8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// ======================================================================================
// k_pw_stream: W resident in LDS, X straight into MFMA fragments, 16-pixel work units.
// ======================================================================================
// KS = number of 32-deep k-steps actually swept (ceil(K/32)); the blob's stride is p.KS.
// KFULL: K == 32 * KS, every k-step swept holds real channels (its loads carry no bound).  A8: K and N are even but not both multiples of 4 (ShuffleNetV2's
// 58-channel branches): pixel rows are only 8-byte aligned, so every 16-byte access becomes two
// 8-byte ones and the per-channel vectors are read with bounds.
// TAB (single-pass modes only): the quantizer is the threshold table of slfp_enc.hpp, which yields the packed fp16
// operand directly (6 VALU instructions per element instead of 22 + convert + pack).
// STG (with TAB): the outputs of two channel tiles at a time go through a 2 KiB per-wave LDS buffer and leave as 128-byte
// pieces (8 pixels x 32 channels per store instruction) instead of the accumulator layout's 64-byte pieces (16 pixels x
// 16 channels): HBM writes of 64-byte pieces run at about half the rate (profiles/micro/bw_patterns.hip).
// RES (with TAB): y = relu?(affine(conv) + res) (slfp_conv2d_fwd_res).  Each piece of p.res is loaded with the address pattern
// of the store it pairs with, one tile (STG: one pair of tiles) ahead of the MFMA sweep that produces the values it is added to.
// YC (with TAB, single pass): the output leaves as the consumer's 1-byte codes (p.yc; N a multiple of 16), four channel tiles per
// 16-byte store as in k_pwc_stream; the ReLU, if any, is the code quantizer's (enc4_code_relu).
template <int FMT, int PASSES, int KS, bool KFULL, bool A8 = false, bool TAB = false, bool STG = false, bool RES = false, bool YC = false>
__global__ __launch_bounds__(kStreamThreads) void k_pw_stream(const PwParams p) {
    static_assert(!STG || (TAB && !A8), "staged stores: table kernels with 16-byte channel alignment");
    static_assert(!RES || (TAB && !A8), "residual operand: table kernels with 16-byte channel alignment");
    static_assert(!YC || (TAB && !A8 && !STG && !RES && PASSES == 1), "code output: single-pass table kernels, 16-byte channel alignment");
    constexpr int TABB = TAB ? kPwTab : 64;
    constexpr int TABL = (TAB && (PASSES == 3 || YC)) ? kPwTab : 16;   // three-pass table kernels: the residual plane's table; YC: the code table
    // The quantizer's table is STATIC LDS: its address is a compile-time constant, so a lookup is `ds_read_b64 v, bin`
    // with no add of the (link-time) dynamic-LDS base -- hipcc emitted one VALU add per lookup (33 in the depthwise kernel).
    __shared__ __attribute__((aligned(16))) unsigned char stab[TABB];
    __shared__ __attribute__((aligned(16))) unsigned char stab_lo[TABL];
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // everything else (sizes depend on the layer)
    uint32_t* sT = reinterpret_cast<uint32_t*>(stab);
    _Float16* wl_hi = reinterpret_cast<_Float16*>(smem);
    const int wfrags = p.n_tiles * p.KS;  // 1 KiB each
    _Float16* wl_lo = wl_hi + (size_t)wfrags * 512;
    if constexpr (TAB) enc_fill<kStreamThreads>(reinterpret_cast<uint2*>(stab), p.enc);
    else lut_fill<FMT>(sT);
    if constexpr (TAB && (PASSES == 3 || YC)) enc_fill_compact<kStreamThreads>(reinterpret_cast<uint2*>(stab_lo), p.enc_lo);
    // W blob -> LDS (same fragment order), 16 bytes per thread per step
    for (int i = threadIdx.x; i < wfrags * 64; i += kStreamThreads) {
        reinterpret_cast<half8*>(wl_hi)[i] = reinterpret_cast<const half8*>(p.whi)[i];
        if constexpr (PASSES == 3) reinterpret_cast<half8*>(wl_lo)[i] = reinterpret_cast<const half8*>(p.wlo)[i];
    }
    // per-channel epilogue vectors (pw_fill_ep), padded to the blob's channel count
    float* ep = reinterpret_cast<float*>(smem + (size_t)(PASSES == 3 ? 2 : 1) * wfrags * 1024);
    const int n_pad = p.n_tiles * 16;
    unsigned char* stg = reinterpret_cast<unsigned char*>(ep + 3 * n_pad) + (threadIdx.x >> 6) * 2048;   // STG: this wave's 2 KiB
    const bool has_vec = p.bias != nullptr || p.post.scale != nullptr;   // wave-uniform
    if (has_vec) pw_fill_ep<kStreamThreads>(ep, p, 0, n_pad);
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int col = lane & 15, kq = lane >> 4;
    const int64_t n_groups = (p.M + 15) >> 4;
    const int64_t waves_total = (int64_t)gridDim.x * (kStreamThreads / 64);
    const int64_t wave_id = (int64_t)blockIdx.x * (kStreamThreads / 64) + (threadIdx.x >> 6);

    for (int64_t g = wave_id; g < n_groups; g += waves_total) {
        const int64_t m = g * 16 + col;
        const bool live = m < p.M;
        // unconditional loads (rows past the end are clamped and dropped): hipcc cannot count
        // conditional loads and falls back to vmcnt(0) waits
        const float* xr = p.x + x_row_offset(p, live ? m : p.M - 1) + kq * 4;
        // ---- X: 2 x 16-byte loads per k-step, CH k-steps (up to 8 loads per lane) in flight
        // before their encodes
        constexpr int CH = KS;  // (chunking the loads made hipcc allocate MORE registers, not fewer)
        half8 xh[KS], xl[KS];
#pragma unroll
        for (int c0 = 0; c0 < KS; c0 += CH) {
            float4 raw[CH][2];
#pragma unroll
            for (int c = 0; c < CH; ++c) {
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
                    if constexpr (A8) {
                        const int k = (c0 + c) * 32 + hf * 16 + kq * 4;   // K is even: each 8-byte half is all real or all padding
                        const float* row = xr - kq * 4;
                        float2 a = *reinterpret_cast<const float2*>(row + (k < p.K ? k : p.K - 2));
                        float2 b = *reinterpret_cast<const float2*>(row + (k + 2 < p.K ? k + 2 : p.K - 2));
                        if (k >= p.K) a = make_float2(0.f, 0.f);
                        if (k + 2 >= p.K) b = make_float2(0.f, 0.f);
                        raw[c][hf] = make_float4(a.x, a.y, b.x, b.y);
                    } else if constexpr (KFULL) {
                        raw[c][hf] = ld_stream4<SLFP_NT_PW>(xr + (c0 + c) * 32 + hf * 16);
                    } else {
                        const int k = (c0 + c) * 32 + hf * 16 + kq * 4;
                        raw[c][hf] = *reinterpret_cast<const float4*>(xr + (k < p.K ? (c0 + c) * 32 + hf * 16 : p.K - 4 - kq * 4));
                        if (k >= p.K) raw[c][hf] = make_float4(0.f, 0.f, 0.f, 0.f);
                    }
                }
            }
            if constexpr (TAB && PASSES == 3) {
                bool any_nan = false;
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    any_nan |= enc_has_nan4(raw[c][0]) | enc_has_nan4(raw[c][1]);
                    enc_frag_hl(raw[c][0], raw[c][1], p.enc, stab, stab_lo, xh[c0 + c], xl[c0 + c]);
                }
                if (__builtin_expect(any_nan, 0)) {   // NaN in -> NaN out; never taken on real activations
#pragma unroll
                    for (int c = 0; c < CH; ++c) frag_patch_nan(raw[c][0], raw[c][1], xh[c0 + c]);
                }
            } else if constexpr (TAB) {
                bool any_nan = false;
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    any_nan |= enc_has_nan4(raw[c][0]) | enc_has_nan4(raw[c][1]);
                    xh[c0 + c] = enc_frag(raw[c][0], raw[c][1], p.enc, stab);
                }
                if (__builtin_expect(any_nan, 0)) {   // NaN in -> NaN out; never taken on real activations
#pragma unroll
                    for (int c = 0; c < CH; ++c) xh[c0 + c] = enc_frag_nan(raw[c][0], raw[c][1], p.enc, stab);
                }
            } else {
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    half4 h0, h1, l0, l1;
                    encode4<FMT, PASSES>(raw[c][0], p.sd, sT, h0, l0);
                    encode4<FMT, PASSES>(raw[c][1], p.sd, sT, h1, l1);
                    xh[c0 + c] = join(h0, h1);
                    if constexpr (PASSES == 3) xl[c0 + c] = join(l0, l1);
                }
            }
            // keep the chunks sequential: without this hipcc hoists every load of every chunk
            // to the top and runs out of registers at K = 256
            if constexpr (KS > CH) asm volatile("" ::: "memory");
        }
        // ---- sweep the output-channel tiles
        auto tile_out = [&](int j) {
            const floatx4 acc = pw_sweep_lds<PASSES, KS>(wl_hi + ((size_t)j * p.KS) * 512 + lane * 8, (size_t)wfrags * 512, xh, xl);
            return pw_finish<!RES && !YC, !YC>(acc, p, ep, n_pad, j * 16 + kq * 4, has_vec);
        };
        if constexpr (YC) {
            uint8_t* yr = p.yc + (size_t)m * p.N;
            const CodeQuant cq{p.enc_lo.r1, p.enc_lo.lo, p.enc_lo.hi, p.sgn, p.fmt_out};
            for (int j0 = 0; j0 < p.n_tiles; j0 += 4)   // n_tiles is a multiple of 4 (the blob is padded to 64 channels)
                pw_codes16_out<false, true>(j0, yr, live, 0, p.N, kq, cq, stab_lo, tile_out);
        } else if constexpr (STG) {
            // per-unit descriptor: rows beyond M and channels beyond N get an out-of-range offset (store dropped)
            const uint32_t ybytes = (uint32_t)(((uint64_t)(p.M - g * 16) * p.N * 4) > 0xFFFFFFFFull ? 0xFFFFFFFFull : ((uint64_t)(p.M - g * 16) * p.N * 4));
            const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(p.y + (size_t)g * 16 * p.N, 0, ybytes, 0x00020000);
            const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(RES ? p.res : p.y) + (size_t)g * 16 * p.N, 0, ybytes, 0x00020000);
            const int spx = lane >> 3, sch = lane & 7;
            // byte offset of piece h of tile pair j0 inside the unit (stores and residual loads alike)
            auto piece = [&](int j0, int h) {
                return (j0 * 16 + sch * 4) < p.N ? (uint32_t)((spx + 8 * h) * p.N + j0 * 16 + sch * 4) * 4u : 0xFFFFFFF0u;
            };
            u32x4 rq[2];   // RES: the residual pieces of the NEXT pair, in flight under this pair's MFMAs
            if constexpr (RES) { rq[0] = res_load_stg(rr, piece(0, 0)); rq[1] = res_load_stg(rr, piece(0, 1)); }
            for (int j0 = 0; j0 < p.n_tiles; j0 += 2) {
                u32x4 rc[2];
                if constexpr (RES) {
                    rc[0] = rq[0]; rc[1] = rq[1];
                    rq[0] = res_load_stg(rr, piece(j0 + 2, 0)); rq[1] = res_load_stg(rr, piece(j0 + 2, 1));   // past the last pair: out of range
                }
                const float4 ra = tile_out(j0), rb = tile_out(j0 + 1);
                *reinterpret_cast<float4*>(stg + col * 128 + kq * 16) = ra;
                *reinterpret_cast<float4*>(stg + col * 128 + 64 + kq * 16) = rb;
                // LDS operations of one wave execute in order: the reads see the writes, the next pair's writes follow the reads
                const bool ch_ok = (j0 * 16 + sch * 4) < p.N;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    u32x4 v = *reinterpret_cast<const u32x4*>(stg + lane * 16 + h * 1024);
                    if constexpr (RES) v = res_add_stg(v, rc[h], p.post.relu);
                    uint32_t so = ch_ok ? (uint32_t)((spx + 8 * h) * p.N + j0 * 16 + sch * 4) * 4u : 0xFFFFFFF0u;
                    asm volatile("" : "+v"(so));
                    if (p.nt_out) __builtin_amdgcn_raw_buffer_store_b128(v, ry, so, 0, 2);
                    else __builtin_amdgcn_raw_buffer_store_b128(v, ry, so, 0, 0);
                }
            }
        } else {   // this loop stands in conv_pw_codes.hip's k_pwc_stream too (without the A8 two-half store)
            float* yr = p.y + (size_t)m * p.N + kq * 4;
            // RES: the 16 bytes a store will overwrite, one tile ahead (unconditional: dead rows / channels re-read a live element)
            const float* rrow = (RES ? p.res : p.y) + (size_t)(live ? m : p.M - 1) * p.N;
            float4 rn;
            if constexpr (RES) rn = ld_stream4<SLFP_NT_PW_RES>(rrow + (kq * 4 < p.N ? kq * 4 : 0));
            for (int j = 0; j < p.n_tiles; ++j) {
                float4 rc;
                if constexpr (RES) {
                    rc = rn;
                    const int n1 = (j + 1) * 16 + kq * 4;
                    rn = ld_stream4<SLFP_NT_PW_RES>(rrow + (n1 < p.N ? n1 : 0));
                }
                float4 r = tile_out(j);
                if constexpr (RES) r = res_add(r, rc, p.post.relu);
                const int n = j * 16 + kq * 4;
                if constexpr (A8) {
                    if (live && n < p.N) *reinterpret_cast<float2*>(yr + j * 16) = make_float2(r.x, r.y);
                    if (live && n + 2 < p.N) *reinterpret_cast<float2*>(yr + j * 16 + 2) = make_float2(r.z, r.w);
                } else {
                    if (live && n < p.N) st_stream4<SLFP_NT_PW>(yr + j * 16, r);
                }
            }
        }
    }
}

// ======================================================================================
// k_pw_tiled: X via a swizzled LDS tile (encoded once), W fragments straight from L2.
// ======================================================================================

// KFULL: K is a multiple of 64 (no masking of the K tail).  Every global load in the main
// loop is UNCONDITIONAL (rows beyond M are clamped to the last row and never stored, padded
// output tiles are clamped and never stored) and the loop body has no branches: with a
// per-load `if` hipcc cannot count the loads in flight and falls back to s_waitcnt vmcnt(0)
// in the middle of the MFMA block, draining the HBM loads it has just issued (r01c ISA).
// STG: the epilogue goes through a per-wave LDS staging area so that every store instruction writes whole 256-byte runs
// (4 pixel rows x the wave's 64 adjacent channels) instead of 64-byte pieces, with the nt hint (SLFP_NT_PW_STG).
// RES (with STG): y = relu?(affine(conv) + res) (slfp_conv2d_fwd_res).  The residual is loaded in the staged layout (the 16 bytes
// each staged store writes), one 16-row tile ahead: the first tile row's pieces are requested before the last MFMA sweep.
// YC (with TAB, single pass, NT == 4): the output leaves as the consumer's 1-byte codes (p.yc; N a multiple of 16): per tile row
// the wave's four channel tiles are the four dwords of k_pwc_tiled's code epilogue; no staging area.
template <int FMT, int PASSES, int WM, int WN, int MT, int NT, bool KFULL, bool TAB = false, bool STG = false, bool RES = false, bool YC = false>
__global__ __launch_bounds__(64 * WM * WN, (WM * WN) <= 4 ? 2 : 4) void k_pw_tiled(const PwParams p) {
    static_assert(!STG || NT == 4, "the staged epilogue stores a wave's 64 channels per row");
    static_assert(!RES || STG, "residual operand: staged epilogue only");
    static_assert(!YC || (TAB && !STG && !RES && PASSES == 1 && NT == 4), "code output: single-pass table kernels, four channel tiles per wave");
    constexpr int TABB = TAB ? kPwTab : 64;
    constexpr int TABL = (TAB && (PASSES == 3 || YC)) ? kPwTab : 16;
    using G = PwTile<WM, WN, MT, NT>;
    constexpr int T = G::T, BM = G::BM, BN = G::BN, XBYTES = G::XBYTES;
    constexpr int NLD = G::NLD;  // float4 loads per thread per 64-deep stage

    __shared__ __attribute__((aligned(16))) unsigned char stab[TABB];      // static: constant address (see k_pw_stream)
    __shared__ __attribute__((aligned(16))) unsigned char stab_lo[TABL];
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* sT = reinterpret_cast<uint32_t*>(stab);
    unsigned char* xs = smem;  // [2 buffers][hi, lo][BM rows][128 B]
    if constexpr (TAB) enc_fill<T>(reinterpret_cast<uint2*>(stab), p.enc);
    else lut_fill<FMT>(sT);
    if constexpr (TAB && (PASSES == 3 || YC)) enc_fill_compact<T>(reinterpret_cast<uint2*>(stab_lo), p.enc_lo);

    const uint32_t b = xcd_remap(blockIdx.x, p.nblocks);
    const uint32_t nb = b % p.n_blocks, mb = b / p.n_blocks;
    const int64_t m0 = (int64_t)mb * p.rb;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int col = lane & 15, kq = lane >> 4;

    // ---- staging geometry (conv_pw_core.hpp): float4 #i of a thread covers row (tid>>4) + i*(T/16), k = (tid&15)*4
    const int kc = threadIdx.x & 15;
    const int st_chunk = (kc >> 3) * 4 + (kc & 3);
    const uint32_t st_sub = (uint32_t)((kc & 7) >> 2) * 8u;
    const float* src[NLD];
#pragma unroll
    for (int i = 0; i < NLD; ++i) src[i] = p.x + pw_stage_row_offset<T>(p, m0, i) + kc * 4;

    float4 st[NLD];
    auto load_stage = [&](int t) {
#ifdef SLFP_ABL_NOX   // diagnostic builds only (profiles/ablate_pw.sh): wrong results, what does the kernel cost without ...
        if (t >= 2) {
#pragma unroll
            for (int i = 0; i < NLD; ++i) asm volatile("" : "+v"(st[i].x), "+v"(st[i].y), "+v"(st[i].z), "+v"(st[i].w));
            return;
        }
#endif
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            if constexpr (KFULL) {
                st[i] = ld_stream4<SLFP_NT_PWT>(src[i] + t * 64);
            } else {
                const int k = t * 64 + kc * 4;
                const int kk = k < p.K ? t * 64 : p.K - 4 - kc * 4;  // clamp inside the row
                st[i] = *reinterpret_cast<const float4*>(src[i] + kk);
                if (k >= p.K) st[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    };
    auto encode_store = [&](int buf) {
        unsigned char* hi = xs + (size_t)buf * (PASSES == 3 ? 2 : 1) * XBYTES;
        unsigned char* lo = hi + XBYTES;
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int row = (threadIdx.x >> 4) + i * (T / 16);
            const uint32_t off = lds_x_off(row, st_chunk) + st_sub;
            if constexpr (TAB && PASSES == 3) {
                uint2 ph, pl;
                enc2_f16_hl(st[i].x, st[i].y, p.enc.r1, p.enc.lo, p.enc.hi, stab, stab_lo, ph.x, pl.x);
                enc2_f16_hl(st[i].z, st[i].w, p.enc.r1, p.enc.lo, p.enc.hi, stab, stab_lo, ph.y, pl.y);
                if (__builtin_expect(enc_has_nan4(st[i]), 0)) enc_patch_nan4_f16(st[i], ph);
                *reinterpret_cast<uint2*>(hi + off) = ph;
                *reinterpret_cast<uint2*>(lo + off) = pl;
            } else if constexpr (TAB) {
#ifdef SLFP_ABL_NOENC
                uint2 pk;
                pk.x = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(st[i].x, st[i].y));
                pk.y = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(st[i].z, st[i].w));
                *reinterpret_cast<uint2*>(hi + off) = pk;
#else
                *reinterpret_cast<uint2*>(hi + off) = enc4_f16(st[i], p.enc.r1, p.enc.lo, p.enc.hi, stab);
#endif
            } else {
                half4 h, l;
                encode4<FMT, PASSES>(st[i], p.sd, sT, h, l);
                *reinterpret_cast<half4*>(hi + off) = h;
                if constexpr (PASSES == 3) *reinterpret_cast<half4*>(lo + off) = l;
            }
        }
    };

    floatx4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

    const int KT = p.KS >> 1;  // 64-deep stages
    const int ntile0 = (int)nb * (BN / 16) + wn * NT;
    // W fragments by buffer loads (pw_w_rsrc, pw_w_offset): the addresses are scalar but for one vector register, so a second W set
    // (W double-buffered by k-step, as k_pwc_tiled does) fits without spills, and was measured: 118.19 vs 118.53 k images/s
    // without it (200-step A/B, 9 / 6 runs) -- on the float32 interface the X loads and the encoder set the stage time.
    // This single-buffered load_w and k_pwc_tiled's double-buffered one differ on purpose.
    const int wn_u = __builtin_amdgcn_readfirstlane(wn);
    const int ntile0u = (int)nb * (BN / 16) + wn_u * NT;
    const __amdgpu_buffer_rsrc_t rwh = pw_w_rsrc(p.whi, p);
    const __amdgpu_buffer_rsrc_t rwl = pw_w_rsrc(PASSES == 3 ? p.wlo : p.whi, p);
    uint32_t wsoff[NT];   // scalar
#pragma unroll
    for (int j = 0; j < NT; ++j) wsoff[j] = pw_w_offset(p, ntile0u + j);
    const uint32_t wvoff = (uint32_t)lane * 16u;
    half8 wh[NT], wl[NT];
    auto load_w = [&](int kstep) {
#ifdef SLFP_ABL_NOW
        if (kstep >= 1) {
#pragma unroll
            for (int j = 0; j < NT; ++j) asm volatile("" : "+v"(wh[j]));
            return;
        }
#endif
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const uint32_t so = wsoff[j] + (uint32_t)kstep * 1024u;
            wh[j] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rwh, wvoff, so, 0));
            if constexpr (PASSES == 3) wl[j] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rwl, wvoff, so, 0));
        }
    };
    // (this step stands in k_pwc_tiled too, there with the double-buffered W registers: the shared form, which takes acc / wh / wl by
    // reference, moved register counts of both kernels)
    auto mfma_step = [&](int buf, int ks) {
        const unsigned char* hi = xs + (size_t)buf * (PASSES == 3 ? 2 : 1) * XBYTES;
        const unsigned char* lo = hi + XBYTES;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int row = (wm * MT + i) * 16 + col;
            const uint32_t off = lds_x_off(row, ks * 4 + kq);
            const half8 xh = *reinterpret_cast<const half8*>(hi + off);
            half8 xl;
            if constexpr (PASSES == 3) xl = *reinterpret_cast<const half8*>(lo + off);
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                if constexpr (PASSES == 3) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[j], xh, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[j], xl, acc[i][j], 0, 0, 0);
                }
#ifdef SLFP_ABL_NOMFMA
                asm volatile("" :: "v"(wh[j]), "v"(xh));
#else
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[j], xh, acc[i][j], 0, 0, 0);
#endif
            }
        }
    };

    SLFP_STAMP(0);
    __syncthreads();  // LUT visible
    SLFP_STAMP(1);
    load_stage(0);
    encode_store(0);
    load_stage(KT > 1 ? 1 : 0);
    __syncthreads();
    SLFP_STAMP(2);

    for (int t = 0; t + 1 < KT; ++t) {  // branch-free body
        const int buf = t & 1;
#ifdef SLFP_PW_STAMPS2   // diagnostic builds only: fine-grained stamps of stage 3 in slots 3..7 (profiles/stamps_fine.py)
        if (t == 3) SLFP_STAMP(3);
#endif
        load_w(t * 2);
        encode_store(buf ^ 1);                       // stage t+1 (fetched one stage ago) -> the other LDS buffer
        load_stage(t + 2 < KT ? t + 2 : KT - 1);     // stage t+2's HBM loads fly during the MFMAs (last: harmless re-read)
#ifdef SLFP_PW_STAMPS2
        if (t == 3) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); SLFP_STAMP(4); }
#endif
        mfma_step(buf, 0);
#ifdef SLFP_PW_STAMPS2
        if (t == 3) { asm volatile("s_nop 0" : "+v"(acc[0][0]), "+v"(acc[3][3])); SLFP_STAMP(5); }
#endif
        load_w(t * 2 + 1);
        mfma_step(buf, 1);
#ifdef SLFP_PW_STAMPS2
        if (t == 3) { asm volatile("s_nop 0" : "+v"(acc[0][0]), "+v"(acc[3][3])); SLFP_STAMP(6); }
#endif
        __syncthreads();
#ifdef SLFP_PW_STAMPS2
        if (t == 3) SLFP_STAMP(7);
#else
        SLFP_STAMP(3 + (t < 8 ? t : 8));
#endif
    }
    SLFP_STAMP(12);
    // staged epilogue geometry: piece h of tile row i = 4 pixel rows x the wave's 64 channels, 16 bytes per lane
    const int srow = lane >> 4, sch = lane & 15;
    const int n_st = ntile0 * 16 + sch * 4;
    const uint64_t yleft = (uint64_t)(p.M - m0) * p.N * 4;
    const uint32_t ybytes = (uint32_t)(yleft > 0xFFFFFFFFull ? 0xFFFFFFFFull : yleft);
    auto piece = [&](int i, int h) {   // byte offset from row m0 (stores and residual loads alike); out of range: dropped / 0
        const int row = (wm * MT + i) * 16 + h * 4 + srow;
        const bool ok = row < p.rb && m0 + row < p.M && n_st < p.N;
        return ok ? (uint32_t)(row * p.N + n_st) * 4u : 0xFFFFFFF0u;
    };
    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(RES ? p.res : p.y) + (size_t)m0 * p.N, 0, ybytes, 0x00020000);
    u32x4 rq[4];   // RES: four residual pieces in flight (16 registers): piece h of the tile row that is stored next
    {   // last stage: nothing left to prefetch
        const int t = KT - 1, buf = t & 1;
        load_w(t * 2);
        mfma_step(buf, 0);
        load_w(t * 2 + 1);
        if constexpr (RES) {   // behind the last W loads (loads retire in order: the W wait must not include these), under the last sweep
#pragma unroll
            for (int h = 0; h < 4; ++h) rq[h] = res_load_stg(rr, piece(0, h));
        }
        mfma_step(buf, 1);
    }

    const int n_lo = (int)nb * BN;
    float* lsc = reinterpret_cast<float*>(xs);   // LDS: the (now free) X tile
    float* lsh = lsc + BN;
    if (p.post.scale) {
        __syncthreads();   // every wave is done with the X tile
        pw_bn_slice_fill<BN, T>(lsc, lsh, p.post.scale, p.post.shift, p.N, n_lo);
        __syncthreads();
    }
    SLFP_STAMP(13);
    if constexpr (YC) {
        const CodeQuant cq{p.enc_lo.r1, p.enc_lo.lo, p.enc_lo.hi, p.sgn, p.fmt_out};
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            uint32_t c[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const float4 r = pw_tile_finish<false, false>(acc[i][j], p, (ntile0 + j) * 16 + kq * 4, n_lo, lsc, lsh);
                c[j] = code4<false, true>(r, cq, stab_lo);   // the ReLU, if any, is the quantizer's
            }
            const int row = (wm * MT + i) * 16 + col;
            const int n = (ntile0 + kq) * 16;   // after the transpose lane-quarter kq: channels 16 (ntile0 + kq) + 0..15 of pixel row `col`
            store_codes16(c, p.yc + (size_t)(m0 + row) * p.N + n, row < p.rb && m0 + row < p.M && n < p.N);
        }
        return;
    }
    if constexpr (STG) {
        // The staged store loop and the geometry above stand in k_pwc_tiled too (there with the DUAL code store, here with the nt hint
        // and the diagnostics).
        unsigned char* stg = xs + 2 * (PASSES == 3 ? 2 : 1) * XBYTES + wave * (16 * kStgRow);   // private to this wave
        const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(p.y + (size_t)m0 * p.N, 0, ybytes, 0x00020000);
#pragma unroll
        for (int i = 0; i < MT; ++i) {
#pragma unroll
            for (int j = 0; j < NT; ++j)   // with a residual the ReLU follows the add (res_add_stg)
                *reinterpret_cast<float4*>(stg + col * kStgRow + j * 64 + kq * 16) =
                    pw_tile_finish<!RES, true>(acc[i][j], p, (ntile0 + j) * 16 + kq * 4, n_lo, lsc, lsh);
            // LDS operations of one wave execute in order: the reads see the writes, the next tile's writes follow the reads
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const int row = (wm * MT + i) * 16 + h * 4 + srow;
                u32x4 v = *reinterpret_cast<const u32x4*>(stg + (h * 4 + srow) * kStgRow + sch * 16);
                if constexpr (RES) {
                    v = res_add_stg(v, rq[h], p.post.relu);
                    if (i + 1 < MT) rq[h] = res_load_stg(rr, piece(i + 1, h));   // the next tile row's piece takes the register over
                }
                const bool ok = row < p.rb && m0 + row < p.M && n_st < p.N;
                uint32_t so = ok ? (uint32_t)(row * p.N + n_st) * 4u : 0xFFFFFFF0u;
#ifdef SLFP_ABL_NOST
                so = 0xFFFFFFF0u;
#endif
                asm volatile("" : "+v"(so));
                if (p.nt_out) __builtin_amdgcn_raw_buffer_store_b128(v, ry, so, 0, 2);
                    else __builtin_amdgcn_raw_buffer_store_b128(v, ry, so, 0, 0);
            }
        }
        SLFP_STAMP(14);
#ifdef SLFP_PW_STAMPS
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        SLFP_STAMP(15);
#endif
        return;
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = (ntile0 + j) * 16 + kq * 4;
        if (n >= p.N) continue;
        const float4 bq = bias_q256(p, n);
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int row = (wm * MT + i) * 16 + col;
            const int64_t m = m0 + row;
            if (m >= p.M || row >= p.rb) continue;
            float4 r = epilogue(acc[i][j], bq, p.s1x, p.s2);
            if (p.post.scale) {
                const float4 sc = *reinterpret_cast<const float4*>(lsc + (n - n_lo));
                const float4 sh = *reinterpret_cast<const float4*>(lsh + (n - n_lo));
                r = affine4(r, sc, sh);
                if (p.post.layerout) r = layerout4(r);
            }
            if (p.post.relu) r = relu4(r);
            st_stream4<SLFP_NT_PW>(p.y + (size_t)m * p.N + n, r);
        }
    }
}


// ---------------------------------------------------------------------------- launch
// CAN the LDS-resident stream kernel take this layer (W next to the tables and the staging area)?  Also what the planner asks
// for channel counts that are even but not multiples of 4 (only that kernel has the 8-byte access path).
bool pointwise_stream_fits(int64_t k_pad, int64_t n_pad, int passes) {
    const size_t w = (size_t)k_pad * n_pad * 2 * (passes == 3 ? 2 : 1);
    return k_pad <= 256 && w <= (size_t)128 * 1024;
}
// SHOULD it?  Above SLFP_PW_STREAM_MAX_KB (default 30 KiB of W) the tiled kernel is faster on whole steps (codec.hip: Switches).
static bool stream_fits(const ConvPlan& plan, int passes, const PwParams& p) {
    if (!pointwise_stream_fits(plan.k_pad, plan.n_pad, passes)) return false;
    if (p.K % 4 || p.N % 4) return true;   // 8-byte access path: the stream kernel only
    const size_t w = (size_t)plan.k_pad * plan.n_pad * 2 * (passes == 3 ? 2 : 1);
    // three-pass mode (two planes, 3 MFMAs per tile): the stream kernel stays ahead up to 100 KiB (99.4 vs 95.6 k images/s)
    return w <= (size_t)(passes == 3 ? 100 : switches().pw_stream_max_kb) * 1024;
}

// Everything a float32-input pointwise launch decides, worked out in ONE place (pw_select): the launchers below only dispatch on
// it and pw_variant_name (slfp_debug_pw_variant) prints it, so the reported string cannot drift from what runs.
enum PwKernel { kPwStream = 0, kPwTiled };
struct PwSel {
    int kernel;
    int fmt, passes;         // template arguments FMT / PASSES
    bool kfull;              // stream: K == 32 * KS; tiled: K % 64 == 0
    bool tab, stg, res, yc;  // template arguments TAB / STG / RES / YC
    int ks; bool a8;         // k_pw_stream: KS instance (1, 2, 3, 4, 6, 8), A8
    int wm, wn, mt;          // k_pw_tiled: tiling (NT = 4 throughout)
    int grid_cap;            // k_pw_stream: SLFP_PW_GRID, the most workgroups the persistent grid may have (0: no cap)
};
// staged 128-byte stores (with the nt hint) pay where stores dominate and follow each other closely (K <= 64: pw1
// -14 %, pw2 -13 %) and at K = 256 (256->256 @28: 113 -> 97-105 us).  At K = 128 the layer itself loses 5-8 % (profiles/
// variants.py --var SLFP_PW_STG_MAXKS=4 / 8) but the depthwise layer that reads its output gains more (whole step, 200-step
// same-box A/B profiles/ab_env_long.sh, 3 rounds: depthwise family 1.035 -> 0.997 ms, pointwise 1.098 -> 1.112, step -1 %):
// staged everywhere since round 3.  K = 160 / 192 (KS 5..6: no MobileNetV1 layer) keep the direct stores they were measured with
constexpr bool stream_stg_default(int ks) { return ks <= 4 || ks == 8; }

// p: K, N, res, yc and the tables (enc / enc_lo) as launch_pointwise_any fills them.  SLFP_OK, or the refusal (error text recorded).
static int pw_select(const PwParams& p, const ConvPlan& plan, PwSel* s) {
    *s = PwSel{};
    s->fmt = plan.fmt_act;
    const int passes = s->passes = (plan.fmt_act != kFmtSfp7 && plan.passes == 3) ? 3 : 1;   // SFP<3,3>: exact in fp16
    const bool tab = p.enc.valid != 0 && (passes == 1 || p.enc_lo.valid != 0);
    const int steps = (p.K + 31) / 32;   // k-steps that hold real channels (the blob is zero-padded to p.KS)
    if (stream_fits(plan, passes, p) && steps >= 1 && steps <= 8) {
        s->kernel = kPwStream;
        s->ks = steps <= 4 ? steps : (steps <= 6 ? 6 : 8);   // the instances: 1, 2, 3, 4, 6 (five or six steps), 8 (seven or eight)
        s->a8 = p.K % 4 || p.N % 4;
        // KFULL loads every one of the KS k-steps without a bound: only when all of them hold real channels.  (K = 160 and 224 are
        // multiples of 32 that fill five of six / seven of eight: the guarded form)
        s->kfull = !s->a8 && p.K == 32 * s->ks;
        s->grid_cap = switches().pw_grid;
        if (p.yc) {   // code output: the single-pass table form, 16-byte channel alignment (pointwise_entry_applicable)
            if (passes != 1 || !p.enc.valid || !p.enc_lo.valid || p.res || p.K % 4 || p.N % 16)
                return fail(SLFP_ERR_UNSUPPORTED, "pointwise: no code-output form of this kernel variant");
            s->tab = s->yc = true;
            return SLFP_OK;
        }
        const int mk = switches().pw_stg_maxks;   // experiment switch (slfp_host.hpp), read once at load
        const bool stg_ks = (mk >= 0 && !p.res) ? s->ks <= mk : stream_stg_default(s->ks);   // the residual forms exist for the default rule only
        s->tab = tab;
        s->stg = tab && stg_ks && !s->a8 && !switches().pw_nostg;
        s->res = p.res != nullptr;
        if (p.res && (!tab || s->a8 || s->stg != stream_stg_default(s->ks)))
            return fail(SLFP_ERR_UNSUPPORTED, "pointwise: no residual form of this kernel variant");
        return SLFP_OK;
    }
    if (p.K % 4 || p.N % 4) return fail(SLFP_ERR_UNSUPPORTED, "pointwise: channel counts not a multiple of 4 need the stream kernel");
    s->kernel = kPwTiled;
    const PwTiling t = pw_tiling(p.N, passes == 1);   // the three-pass path never takes {1, 8, 4}
    s->wm = t.wm; s->wn = t.wn; s->mt = t.mt;
    s->kfull = p.K % 64 == 0;
    if (p.yc) {   // code output: the single-pass table form only (pointwise_entry_applicable)
        if (passes != 1 || !p.enc.valid || !p.enc_lo.valid || p.res)
            return fail(SLFP_ERR_UNSUPPORTED, "pointwise: no code-output form of this kernel variant");
        s->tab = s->yc = true;
        return SLFP_OK;
    }
    s->tab = tab;
    s->stg = tab && !switches().pw_nostg;   // experiment switch (slfp_host.hpp), read once at load
    s->res = p.res != nullptr;
    if (p.res && !s->stg)   // residual operand: the table quantizer + staged epilogue form only (pointwise_res_applicable asks for both)
        return fail(SLFP_ERR_UNSUPPORTED, "pointwise: no residual form of this kernel variant");
    return SLFP_OK;
}

static const char* pw_sel_name(const PwSel& s) {
    static thread_local char buf[80];
    const char* tail = s.res ? "/res" : (s.yc ? "/yc" : "");
    int n;
    if (s.kernel == kPwStream)
        n = snprintf(buf, sizeof buf, "stream/ks%d/%s/%s/%s/p%d/%s%s", s.ks, s.a8 ? "a8" : (s.kfull ? "kfull" : "kpart"), s.tab ? "tab" : "long",
                     s.stg ? "stg" : "dir", s.passes, pw_fmt_word(s.fmt), tail);
    else
        n = snprintf(buf, sizeof buf, "tiled/%d%d%d/%s/%s/%s/p%d/%s%s", s.wm, s.wn, s.mt, s.kfull ? "kfull" : "kpart", s.tab ? "tab" : "long",
                     s.stg ? "stg" : "dir", s.passes, pw_fmt_word(s.fmt), tail);
    if (s.kernel == kPwStream && s.grid_cap > 0) snprintf(buf + n, sizeof buf - n, "/grid%d", s.grid_cap);
    return buf;
}

// From the selection to the kernel: one typed lookup per kernel template.  nullptr: the launchers have no such instance.  The
// launchers launch what the lookup returns and pw_variant_name asks it before it prints a name.
typedef void (*PwFn)(const PwParams);

template <int FMT, int PASSES, int KS>
static PwFn pw_stream_instance_ks(const PwSel& s) {
    constexpr bool kStgDefault = stream_stg_default(KS);
    if (s.yc) {
        if constexpr (PASSES == 1)
            return s.kfull ? k_pw_stream<FMT, 1, KS, true, false, true, false, false, true> : k_pw_stream<FMT, 1, KS, false, false, true, false, false, true>;
        return nullptr;
    }
    if (s.res) {   // the residual forms exist for the default staging rule only
        if (s.stg != kStgDefault) return nullptr;
        return s.kfull ? k_pw_stream<FMT, PASSES, KS, true, false, true, kStgDefault, true> : k_pw_stream<FMT, PASSES, KS, false, false, true, kStgDefault, true>;
    }
    if (s.a8) return s.tab ? k_pw_stream<FMT, PASSES, KS, false, true, true> : k_pw_stream<FMT, PASSES, KS, false, true>;
    if (s.stg) return s.kfull ? k_pw_stream<FMT, PASSES, KS, true, false, true, true> : k_pw_stream<FMT, PASSES, KS, false, false, true, true>;
    if (s.tab) return s.kfull ? k_pw_stream<FMT, PASSES, KS, true, false, true> : k_pw_stream<FMT, PASSES, KS, false, false, true>;
    return s.kfull ? k_pw_stream<FMT, PASSES, KS, true> : k_pw_stream<FMT, PASSES, KS, false>;
}
template <int FMT, int PASSES>
static PwFn pw_stream_instance_fp(const PwSel& s) {
    switch (s.ks) {
        case 1: return pw_stream_instance_ks<FMT, PASSES, 1>(s);
        case 2: return pw_stream_instance_ks<FMT, PASSES, 2>(s);
        case 3: return pw_stream_instance_ks<FMT, PASSES, 3>(s);
        case 4: return pw_stream_instance_ks<FMT, PASSES, 4>(s);
        case 6: return pw_stream_instance_ks<FMT, PASSES, 6>(s);
        case 8: return pw_stream_instance_ks<FMT, PASSES, 8>(s);
        default: return nullptr;
    }
}

template <int FMT, int PASSES, int WM, int WN, int MT, bool KFULL>
static PwFn pw_tiled_instance_k(const PwSel& s) {
    constexpr int NT = 4;
    if (s.yc) {
        if constexpr (PASSES == 1) return k_pw_tiled<FMT, 1, WM, WN, MT, NT, KFULL, true, false, false, true>;
        return nullptr;
    }
    if (s.res) return k_pw_tiled<FMT, PASSES, WM, WN, MT, NT, KFULL, true, true, true>;
    if (s.stg) return k_pw_tiled<FMT, PASSES, WM, WN, MT, NT, KFULL, true, true>;
    if (s.tab) return k_pw_tiled<FMT, PASSES, WM, WN, MT, NT, KFULL, true>;
    return k_pw_tiled<FMT, PASSES, WM, WN, MT, NT, KFULL>;
}
template <int FMT, int PASSES>
static PwFn pw_tiled_instance_fp(const PwSel& s) {
    return pw_tiling_instance<PASSES == 1>(s.wm, s.wn, s.mt, [&](auto t) -> PwFn {
        using G = decltype(t);
        return s.kfull ? pw_tiled_instance_k<FMT, PASSES, G::kWM, G::kWN, G::kMT, true>(s) : pw_tiled_instance_k<FMT, PASSES, G::kWM, G::kWN, G::kMT, false>(s);
    });
}

// FMT / PASSES: SFP<3,3> is exact in fp16 (one pass), SLFP<3,4> takes one pass or three
static PwFn pw_stream_instance(const PwSel& s) {
    if (s.fmt == kFmtSfp7) return pw_stream_instance_fp<kFmtSfp7, 1>(s);
    return s.passes == 3 ? pw_stream_instance_fp<kFmtAct8, 3>(s) : pw_stream_instance_fp<kFmtAct8, 1>(s);
}
static PwFn pw_tiled_instance(const PwSel& s) {
    if (s.fmt == kFmtSfp7) return pw_tiled_instance_fp<kFmtSfp7, 1>(s);
    return s.passes == 3 ? pw_tiled_instance_fp<kFmtAct8, 3>(s) : pw_tiled_instance_fp<kFmtAct8, 1>(s);
}
static PwFn pw_instance(const PwSel& s) { return s.kernel == kPwStream ? pw_stream_instance(s) : pw_tiled_instance(s); }

static int launch_stream_ks(PwParams& p, const PwSel& s, hipStream_t stream) {
    const PwFn fn = pw_stream_instance(s);
    if (!fn) return fail(SLFP_ERR_UNSUPPORTED, "pointwise: no stream kernel instance for %s", pw_sel_name(s));
    const size_t lds = (size_t)(s.passes == 3 ? 2 : 1) * p.n_tiles * p.KS * 1024 + (size_t)3 * p.n_tiles * 16 * sizeof(float) +
                       (s.stg ? (size_t)(kStreamThreads / 64) * 2048 : 0);   // dynamic part; the tables are static LDS
    return pw_launch_stream(fn, p, lds, s.grid_cap, stream, "slfp pointwise (stream) kernel");
}

static int launch_tiled(PwParams& p, const PwSel& s, hipStream_t stream) {
    const PwFn fn = pw_tiled_instance(s);
    if (!fn) return fail(SLFP_ERR_UNSUPPORTED, "pointwise: no tiled kernel instance for %s", pw_sel_name(s));
    return pw_launch_tiled(fn, p, PwTiling{s.wm, s.wn, s.mt}, s.passes, s.stg, stream, "pointwise", "slfp pointwise (tiled) kernel");
}

// Does a residual form of the kernel launch_pointwise would pick exist?  Host-only: the planner's answer, the quantizer table
// of the layer's scale and the two experiment switches that take the table / the staged stores away.
bool pointwise_res_applicable(const slfp_conv2d_desc& d, const ConvPlan& plan) {
    if (plan.family != kPointwise || plan.repad || d.stride_h != 1 || d.stride_w != 1) return false;
    if (d.c_in % 4 || d.c_out % 4) return false;   // the 8-byte (A8) forms have no residual variant
    if (switches().pw_notab || switches().pw_nostg) return false;
    if (!act_table(d.ka, plan.fmt_act, kEncF16P)) return false;
    if (plan.passes == 3 && !act_table(d.ka, plan.fmt_act, kEncF16LO)) return false;
    return true;
}

// Does the code-output form (YC) of the kernel launch_pointwise would pick exist for this layer and this consumer?  Host-only.
bool pointwise_entry_applicable(const slfp_conv2d_desc& d, const ConvPlan& plan, int post_flags, float y_ka, int y_fmt) {
    if (plan.family != kPointwise || plan.repad || plan.passes != 1) return false;
    if (post_flags & SLFP_POST_LAYEROUT) return false;
    if (d.c_out % 16 || d.c_in % 4) return false;
    if (switches().pw_notab || !act_table(d.ka, plan.fmt_act, kEncF16P)) return false;
    const EncArgs* t = enc_table(y_ka, y_fmt, kEncCode);
    return t->valid && enc_compact_covers(*t);   // the code table travels in PwParams::enc_lo's compact form
}

static int launch_pointwise_any(const slfp_conv2d_desc& d, const ConvPlan& plan, const float* x, const void* wfrag, const float* bias,
                                const PostOp& post, float* y, hipStream_t stream, const float* res, uint8_t* yc, float y_ka, int y_fmt);

int launch_pointwise(const slfp_conv2d_desc& d, const ConvPlan& plan, const float* x, const void* wfrag,
                     const float* bias, const PostOp& post, float* y, hipStream_t stream, const float* res) {
    return launch_pointwise_any(d, plan, x, wfrag, bias, post, y, stream, res, nullptr, 1.f, kFmtAct8);
}

int launch_pointwise_entry(const slfp_conv2d_desc& d, const ConvPlan& plan, const float* x, const void* wfrag, const float* bias,
                           const PostOp& post, void* y_codes, const CodeIo& io, hipStream_t stream) {
    // applicability is the caller's check (pointwise_entry_applicable at the ABI boundary); the table is looked up once, below
    if (!y_codes || io.x_codes || !io.y_codes || io.y_ld || post.layerout || plan.family != kPointwise || plan.repad || d.c_out % 16)
        return fail(SLFP_ERR_UNSUPPORTED, "pointwise: no float32 -> codes kernel for this layer (slfp_conv2d_entry_supported)");
    return launch_pointwise_any(d, plan, x, wfrag, bias, post, nullptr, stream, nullptr, reinterpret_cast<uint8_t*>(y_codes), io.y_ka, io.y_fmt);
}

// The host-side part of PwParams: what the descriptor and the plan give (the selection reads the channel counts), which operands are
// present, the quantizer tables.
static int pw_host_params(PwParams& p, const slfp_conv2d_desc& d, const ConvPlan& plan, const float* res, uint8_t* yc, float y_ka, int y_fmt) {
    p.res = res;
    p.yc = yc; p.fmt_out = y_fmt;
    pw_fill_geom(p, d, plan);
    p.enc.valid = 0;
    p.enc_lo.valid = 0;
    if (!switches().pw_notab) {   // experiment switch (slfp_host.hpp), read once at load
        if (const EncArgs* t = act_table(d.ka, plan.fmt_act, kEncF16P)) p.enc = *t;
        if (plan.passes == 3 && p.enc.valid) {   // three-pass mode: the residual plane's table of the same scale (round 3)
            if (const EncArgs* t = act_table(d.ka, plan.fmt_act, kEncF16LO)) p.enc_lo = enc_compact(*t);
            else p.enc.valid = 0;
        }
    }
    if (yc) {   // the consumer's code table in the slot the single-pass forms leave unused
        const EncArgs* t = enc_table(y_ka, y_fmt, kEncCode);
        if (plan.passes != 1 || !p.enc.valid || !t->valid || !enc_compact_covers(*t))
            return fail(SLFP_ERR_UNSUPPORTED, "pointwise: no code table for the consumer's scale %g in the single-pass table form", (double)y_ka);
        p.enc_lo = enc_compact(*t);
    }
    return SLFP_OK;
}

const char* pw_variant_name(const slfp_conv2d_desc& d, const ConvPlan& plan, bool has_res, bool y_codes, float y_ka, int y_fmt) {
    if (plan.family != kPointwise) return "none";
    PwParams p = {};   // only the presence of res / yc matters: nothing is dereferenced
    static float some_res;
    static uint8_t some_codes;
    PwSel s;
    if (pw_host_params(p, d, plan, has_res ? &some_res : nullptr, y_codes ? &some_codes : nullptr, y_ka, y_fmt) != SLFP_OK) return "none";
    if (pw_select(p, plan, &s) != SLFP_OK || !pw_instance(s)) return "none";
    return pw_sel_name(s);
}

static int launch_pointwise_any(const slfp_conv2d_desc& d, const ConvPlan& plan, const float* x, const void* wfrag, const float* bias,
                                const PostOp& post, float* y, hipStream_t stream, const float* res, uint8_t* yc, float y_ka, int y_fmt) {
    PwParams p;
    p.post = post;
    p.x = x; p.bias = bias; p.y = y;
    p.sgn = post.relu ? 0 : 1;
    int rc = pw_host_params(p, d, plan, res, yc, y_ka, y_fmt);
    if (rc != SLFP_OK) return rc;
    p.whi = reinterpret_cast<const _Float16*>(wfrag);
    p.wlo = p.whi + (size_t)plan.n_pad * plan.k_pad;
    p.sd = make_scale_div(d.ka, 4);  // x / (Ka/16) == 16 * (x / Ka)
#ifdef SLFP_PW_STAMPS
    { const char* e = getenv("SLFP_PW_DBG"); p.dbg = e ? reinterpret_cast<unsigned long long*>(strtoull(e, nullptr, 16)) : nullptr; }
#endif
    {   // staged stores always carry the nt hint: a size threshold as in conv_dw2.hip (plain stores for outputs that fit the
        // Infinity Cache) measured 1.5 % SLOWER on the whole net here (profiles/ab_env_wn.sh); SLFP_PW_NT_MIN_MB: experiment switch
        const int64_t min_mb = switches().pw_nt_min_mb;
        p.nt_out = ((SLFP_NT_PW_STG & 2) && p.M * p.N * 4 >= (min_mb << 20)) ? 1 : 0;
    }
    PwSel s;
    rc = pw_select(p, plan, &s);
    if (rc != SLFP_OK) return rc;
    return s.kernel == kPwStream ? launch_stream_ks(p, s, stream) : launch_tiled(p, s, stream);
}

}  // namespace slfp
