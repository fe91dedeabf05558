// conv_pw_codes.hip -- SLFP-quantized pointwise (1x1) convolution on 1-byte activation codes, gfx950 matrix cores.
//
// Replaces Conv2d_Q.forward (utils/conv2d_func.py:20-25 / :41-47) for 1x1 kernels, groups == 1 (the 13 "pw" layers of
// MobileNetV1, nets_imgnet/mobilenetv1.py:31) when the layer sits inside a chain of quantized convolutions
// (csrc/slfp_codes.hpp): the input arrives as the codes the previous layer's epilogue wrote (input_q = QA(x / Ka),
// utils/conv2d_func.py:21, is already applied), the output leaves as the NEXT layer's codes (YC) or as float32.
//
// Same contraction as conv_pw.hip -- v_mfma_f32_16x16x32_f16, A = W fragments of the SAME prepared blob, B = fp16(16 * Q),
// one MFMA per 32-deep k-step in k order from +0, the same epilogue arithmetic -- so the outputs are bit-identical to
// the float32-interface kernels fed with the decoded tensor (single-pass mode; SFP<3,3> exact).  What differs is how the
// B fragments are made and how the result leaves:
//   * a lane loads 16 CONSECUTIVE channel codes of its pixel with one 16-byte load (a wave: 16 pixels x 64 contiguous
//     bytes); a 4 x 4 dword transpose across the wave's four 16-lane rows (2 x v_permlane32_swap + 2 x
//     v_permlane16_swap) turns that into the fragment order of the blob (lane-quarter kq owns channels 4kq.. and
//     16 + 4kq.. of every 32), so the weights need no second layout;
//   * byte -> fp16 operand is one SDWA shift + one 256-entry LDS lookup (+ half a v_bfi to pair two): 1.5 VALU per
//     element where the float32 interface spends 6-7 on the encode;
//   * YC: the 4 output channels a lane holds per 16-channel tile become 4 code bytes (5 VALU + 1 LDS each, written in
//     place by the byte select); the dwords of 4 tiles go back through the same transpose and leave as ONE 16-byte store
//     per lane: per pixel the wave writes 64 contiguous bytes.
// Two kernels, as in conv_pw.hip: k_pwc_stream (W resident in LDS, persistent, a wave's unit = 16 pixels) and
// k_pwc_tiled (W fragments streamed from L2, X tile decoded once into the swizzled LDS image).
// The float32-output forms of all three take a residual operand (RES; slfp_conv2d_fwd_res with io->x_codes = 1): conv3 of a
// ResNet block that reads conv2's codes and adds the float32 trunk, as in conv_pw.hip.
// The residual forms have a DUAL form each (slfp_conv2d_fwd_res_codes): the float32 trunk is stored as before and the value is also
// coded for the NEXT block's quantizer into a second, uint8 tensor, so the next conv1 / downsample.0 never read the float32 trunk.
// k_pwc_stream and k_pwc_tiled also have a float32-equivalent form (PASSES = 3; slfp_conv2d_fwd_codes_x3, launch_pwc_x3): hi + lo
// planes on both operands, three MFMAs per k-step in the order of conv_pw.hip's three-pass kernels, bit-identical to those.
#include "slfp_device.hpp"
#include "slfp_enc.hpp"
#include "slfp_codes.hpp"
#include "slfp_layerout_lut.hpp"
#include "slfp_host.hpp"
#include "conv_pw_core.hpp"

namespace slfp {

struct PwcParams {
    const uint8_t* x;
    const _Float16* whi;
    const _Float16* wlo;  // PASSES == 3: the residual plane of the same blob (n_tiles * KS * 512 halves after whi); nullptr otherwise
    const float* bias;
    void* y;
    const float* res;     // RES kernels (float32 out): the residual operand, NHWC like y; nullptr otherwise
    int64_t M;            // output pixels
    int K, N, KS, n_tiles;
    int H, W, Ho, Wo, S;
    float s1, s2, s1x;
    uint32_t m_blocks, n_blocks, nblocks;
    int rb;
    int sgn;              // YC: no ReLU in front of the output quantizer: codes carry a sign
    int fmt_out;          // YC: format of the output codes (kFmtAct8 | kFmtSfp7)
    PostOp post;
    EncArgs enc;          // YC: code table of the consumer's Ka (kEncCode)
    int y_ld;             // YC: bytes from one pixel's codes to the next (N: a dense tensor; more: a channel slice of a wider one)
    uint8_t* yc;          // DUAL (RES kernels, slfp_conv2d_fwd_res_codes): the second, uint8 output, NHWC, N bytes per pixel; sgn / fmt_out / enc
                          // describe its reader as they do for YC; nullptr otherwise
};

__device__ __forceinline__ half8 dec_frag(uint32_t ca, uint32_t cb, const unsigned char* dtab) {
    const uint2 pa = dec4_f16(ca, dtab), pb = dec4_f16(cb, dtab);
    return __builtin_bit_cast(half8, u32x4{pa.x, pa.y, pb.x, pb.y});
}

// float32-equivalent mode (kDecF16HL table): both planes of the same fragment
__device__ __forceinline__ void dec_frag_hl(uint32_t ca, uint32_t cb, const unsigned char* dtab, half8& xh, half8& xl) {
    uint2 ha, la, hb, lb;
    dec4_f16hl(ca, dtab, ha, la);
    dec4_f16hl(cb, dtab, hb, lb);
    xh = __builtin_bit_cast(half8, u32x4{ha.x, ha.y, hb.x, hb.y});
    xl = __builtin_bit_cast(half8, u32x4{la.x, la.y, lb.x, lb.y});
}

// ======================================================================================
// k_pwc_stream: W resident in LDS, codes straight into MFMA fragments, 16-pixel work units.
// ======================================================================================
// KS: 32-deep k-steps (K = 32 * KS exactly); XW: K is a multiple of 64 (16-byte code loads + transpose), else two
// dword loads per k-step; YC: output codes (N a multiple of 16), else float32.  RES (float32 out): y = relu?(affine(conv) + res),
// each 16 bytes of p.res loaded with the address of the store they pair with, one channel tile ahead of its MFMA sweep.
// HALF (K = 32 * KS - 16, SqueezeNet's 16- and 48-channel squeeze outputs): only channels 0..15 of the last
// k-step exist.  Its second dword -- channels 16..31, which would be the NEXT pixel's codes, or past the tensor for the last
// pixel -- is not loaded: that half of the fragment is the fp16 zero (the blob holds zero weights there; the float32
// interface's k_pw_stream feeds the same zeros), so the accumulators are the same bit for bit.
// DUAL (RES only, N a multiple of 16; slfp_conv2d_fwd_res_codes): the finished float32 value -- after the add and the ReLU -- is stored as
// in the RES form AND coded for the next block's quantizer (p.enc / p.sgn / p.fmt_out, as YC) into p.yc: the 4 tiles of a group are
// swept as before, their code dwords go through rows_transpose4 and leave as one 16-byte store per lane.
// LUTQ (YC only; slfp_conv2d_fwd_codes_lut): the 4 code bytes of a tile come from the byte table of the layer-output classes
// (slfp_layerout_lut.hpp) instead of the reader's threshold table.  The table is read from global memory through the vector cache
// (4.8 KiB, resident in every CU's L1 after the first units): this kernel's LDS holds W up to its capacity and serves a 1 KiB
// fragment read per MFMA, so the lookups go to the pipe that idles during the epilogue.  (Unmeasured against an LDS copy.)
// PASSES == 3 (SLFP<3,4> codes, plain float32 / code output only; slfp_conv2d_fwd_codes_x3): the float32-equivalent mode.  Both planes
// of W are resident (the blob's lo plane follows its hi plane, so one copy loop takes both), the table is kDecF16HL and every k-step
// issues (w_lo, x_hi), (w_hi, x_lo), (w_hi, x_hi) as conv_pw.hip's three-pass k_pw_stream does: the same accumulators bit for bit.
template <int FMT, int KS, bool XW, bool YC, bool RES = false, bool HALF = false, bool DUAL = false, bool LUTQ = false, int PASSES = 1>
__global__ __launch_bounds__(kStreamThreads) void k_pwc_stream(const PwcParams p) {
    static_assert(PASSES == 1 || (PASSES == 3 && FMT == kFmtAct8 && !RES && !HALF && !DUAL && !LUTQ), "three passes: SLFP<3,4>, plain float32 or code output");
    constexpr int PL = PASSES == 3 ? 2 : 1;   // planes of W
    static_assert(!XW || KS % 2 == 0, "16-byte code loads cover two k-steps");
    static_assert(!RES || !YC, "residual operand: float32 output only");
    static_assert(!HALF || !XW, "a half-live last k-step is loaded dword by dword");
    static_assert(!DUAL || RES, "the second, code output belongs to the residual forms");
    static_assert(!LUTQ || (YC && !HALF), "the table epilogue belongs to the code-writing forms");
    __shared__ __attribute__((aligned(16))) uint32_t sdec[256];
    __shared__ __attribute__((aligned(16))) unsigned char senc[((YC && !LUTQ) || DUAL) ? kPwTab : 16];
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    _Float16* wl = reinterpret_cast<_Float16*>(smem);
    const int wfrags = p.n_tiles * p.KS;  // 1 KiB each
    dec_fill<FMT, PASSES == 3 ? kDecF16HL : kDecF16D, kStreamThreads>(sdec);
    if constexpr ((YC && !LUTQ) || DUAL) enc_fill<kStreamThreads>(reinterpret_cast<uint2*>(senc), p.enc);
    const lut_gptr lutg = LUTQ ? enc_carried_ptr(p.enc) : nullptr;
    for (int i = threadIdx.x; i < PL * wfrags * 64; i += kStreamThreads)
        reinterpret_cast<half8*>(wl)[i] = reinterpret_cast<const half8*>(p.whi)[i];
    float* ep = reinterpret_cast<float*>(smem + (size_t)PL * wfrags * 1024);   // [256 * bias/s1/s2 | post scale | post shift]
    const int n_pad = p.n_tiles * 16;
    const bool has_vec = p.bias != nullptr || p.post.scale != nullptr;   // wave-uniform
    if (has_vec) pw_fill_ep<kStreamThreads>(ep, p, 0, n_pad);
    __syncthreads();
    const unsigned char* dtab = reinterpret_cast<const unsigned char*>(sdec);
    const CodeQuant cq{p.enc.r1, p.enc.lo, p.enc.hi, p.sgn, p.fmt_out};

    const int lane = threadIdx.x & 63;
    const int col = lane & 15, kq = lane >> 4;
    const int64_t n_groups = (p.M + 15) >> 4;
    const int64_t waves_total = (int64_t)gridDim.x * (kStreamThreads / 64);
    const int64_t wave_id = (int64_t)blockIdx.x * (kStreamThreads / 64) + (threadIdx.x >> 6);

    for (int64_t g = wave_id; g < n_groups; g += waves_total) {
        const int64_t m = g * 16 + col;
        const bool live = m < p.M;
        const uint8_t* xr = p.x + x_row_offset(p, live ? m : p.M - 1);   // rows past the end: clamped, computed, dropped
        uint32_t cw[KS][2];
        if constexpr (XW) {
            u32x4 v[KS / 2];
#pragma unroll
            for (int c2 = 0; c2 < KS / 2; ++c2) v[c2] = *reinterpret_cast<const u32x4*>(xr + c2 * 64 + kq * 16);
#pragma unroll
            for (int c2 = 0; c2 < KS / 2; ++c2) {
                uint32_t a0 = v[c2][0], a1 = v[c2][1], a2 = v[c2][2], a3 = v[c2][3];
                rows_transpose4(a0, a1, a2, a3);   // lane-quarter kq now holds channels 64 c2 + 16 i + 4 kq
                cw[2 * c2][0] = a0; cw[2 * c2][1] = a1; cw[2 * c2 + 1][0] = a2; cw[2 * c2 + 1][1] = a3;
            }
        } else {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                cw[ks][0] = *reinterpret_cast<const uint32_t*>(xr + ks * 32 + kq * 4);
                if (!HALF || ks + 1 < KS) cw[ks][1] = *reinterpret_cast<const uint32_t*>(xr + ks * 32 + 16 + kq * 4);
            }
        }
        half8 xh[KS], xl[PASSES == 3 ? KS : 1];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if constexpr (PASSES == 3) {
                dec_frag_hl(cw[ks][0], cw[ks][1], dtab, xh[ks], xl[ks]);
            } else if (HALF && ks + 1 == KS) {
                const uint2 pa = dec4_f16(cw[ks][0], dtab);
                xh[ks] = __builtin_bit_cast(half8, u32x4{pa.x, pa.y, 0u, 0u});
            } else {
                xh[ks] = dec_frag(cw[ks][0], cw[ks][1], dtab);
            }
        }

        auto tile_out = [&](int j) {
            const floatx4 acc = pw_sweep_lds<PASSES, KS>(wl + ((size_t)j * p.KS) * 512 + lane * 8, (size_t)wfrags * 512, xh, xl);
            return pw_finish<!YC && !RES, false>(acc, p, ep, n_pad, j * 16 + kq * 4, has_vec);
        };
        if constexpr (YC) {
            uint8_t* yr = reinterpret_cast<uint8_t*>(p.y) + (size_t)m * p.y_ld;
            for (int j0 = 0; j0 < p.n_tiles; j0 += 4)   // n_tiles is a multiple of 4 (the blob is padded to 64 channels)
                pw_codes16_out<LUTQ, false>(j0, yr, live, 0, p.N, kq, cq, senc, tile_out, lutg);
        } else {
            float* yr = reinterpret_cast<float*>(p.y) + (size_t)m * p.N + kq * 4;
            // RES: unconditional loads (dead rows / channels re-read a live element and are dropped)
            const float* rrow = (RES ? p.res : reinterpret_cast<const float*>(p.y)) + (size_t)(live ? m : p.M - 1) * p.N;
            if constexpr (DUAL) {
                uint8_t* ycr = p.yc + (size_t)m * p.N;
                float4 rn = ld_stream4<SLFP_NT_PW_RES>(rrow + (kq * 4 < p.N ? kq * 4 : 0));
                for (int j0 = 0; j0 < p.n_tiles; j0 += 4) {   // n_tiles is a multiple of 4 (the blob is padded to 64 channels)
                    // the codes of the value just stored (the ReLU, where there is one, has run: enc4_code_relu sees r >= 0)
                    pw_codes16_out<false, false>(j0, ycr, live, 0, p.N, kq, cq, senc, [&](int j) {
                        const float4 rc = rn;
                        const int n1 = (j + 1) * 16 + kq * 4;
                        rn = ld_stream4<SLFP_NT_PW_RES>(rrow + (n1 < p.N ? n1 : 0));
                        const float4 r = res_add(tile_out(j), rc, p.post.relu);
                        if (live && j * 16 + kq * 4 < p.N) *reinterpret_cast<float4*>(yr + j * 16) = r;
                        return r;
                    });
                }
            } else {   // this loop stands in conv_pw.hip's k_pw_stream too (there with the A8 two-half store)
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
                    if (live && j * 16 + kq * 4 < p.N) *reinterpret_cast<float4*>(yr + j * 16) = r;
                }
            }
        }
    }
}


// ======================================================================================
// k_pwc_slice: deep layers (K = 256 ... 1024).  W does not fit LDS, but a SLICE of output channels does: a workgroup keeps
// the fragments of NTS channel tiles x all K resident (<= 128 KiB) and streams pixel units past them, as k_pwc_stream does.
// Every slice reads all of X -- at 1 B per element that costs little (the float32 interface could not afford it: X four
// to sixteen times through the encoder): the n_slices workgroups that work on the same pixels share an XCD (blocks b and
// b + 8), so the re-reads are L2 hits, and a byte decodes in 1.5 VALU instructions.  What it removes is k_pwc_tiled's
// per-workgroup W stream from L2 (512 KiB per 64 pixels: 4x the X + Y bytes of these layers) and its barrier per stage.
// K is swept in chunks of KC k-steps with the accumulators of the slice's NTS tiles in registers; k order and MFMA shape
// are those of the other pointwise kernels (bit-identical results).
// ======================================================================================
// The codes of the NEXT chunk -- or of the next unit's first chunk -- are always in flight under the current chunk's MFMAs.
// Measured (round 3, batch 256, us per layer, k_pwc_stream / k_pwc_tiled -> this kernel): 256->256 @28 73 -> 56, 256->512 @14
// 42 -> 34; but 512->512 @14 54 -> 54-64 and 1024->1024 @7 45 -> 66-76 (512 or 1024 threads): with W in LDS every MFMA needs a
// 1 KiB fragment read, exactly the LDS rate of a CU, and the decode lookups come on top -- at K >= 512 the register-blocked
// k_pwc_tiled (4 x 4 tiles per wave, W straight from L2) stays.  Used for K = 256 only (two workgroups per CU).
// RES (float32 out): y = relu?(affine(conv) + res); the first RP tiles' 16-byte pieces of p.res are requested before the unit's K
// sweep, RP more right after it (in the registers the decoded X fragments leave), then one per tile stored: the kernel has to
// stay within 128 VGPRs (two workgroups per CU).
// DUAL (RES only): as in k_pwc_stream, the codes of the stored value leave per group of 4 tiles.
constexpr int kSliceThreads = 512;
constexpr int kSliceDualWaves = 4;   // DUAL: fits the 128 VGPRs too
// LUTQ (YC only): the table epilogue, read from global memory as in k_pwc_stream and for the same reason (the slice's W fills LDS).
template <int FMT, int NTS, bool YC, bool RES = false, bool DUAL = false, bool LUTQ = false>
__global__ __launch_bounds__(kSliceThreads, RES ? (DUAL ? kSliceDualWaves : 4) : 1) void k_pwc_slice(const PwcParams p) {   // RES: 4 waves per SIMD = the 128 VGPRs of two workgroups per CU
    static_assert(!RES || !YC, "residual operand: float32 output only");
    static_assert(!DUAL || RES, "the second, code output belongs to the residual forms");
    static_assert(!LUTQ || YC, "the table epilogue belongs to the code-writing forms");
    constexpr int KC = 8;   // k-steps per chunk = 256 channels = 4 x 16-byte code loads per lane
    constexpr int RP = 2;   // RES: residual pieces in flight under the K sweep
    static_assert(NTS % 4 == 0, "code output leaves in groups of 4 channel tiles");
    __shared__ __attribute__((aligned(16))) uint32_t sdec[256];
    __shared__ __attribute__((aligned(16))) unsigned char senc[((YC && !LUTQ) || DUAL) ? kPwTab : 16];
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    _Float16* wl = reinterpret_cast<_Float16*>(smem);
    const lut_gptr lutg = LUTQ ? enc_carried_ptr(p.enc) : nullptr;
    const int n_slices = p.n_tiles / NTS;
    // blocks b and b + 8 share an XCD: the slices of one pixel range sit on consecutive (b / 8)
    const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;
    const int slice = q % n_slices;
    const int rank = xcd + 8 * (q / n_slices);
    const int n_ranks = 8 * ((int)(gridDim.x >> 3) / n_slices);
    const int wfrags = NTS * p.KS;  // 1 KiB each
    dec_fill<FMT, kDecF16D, kSliceThreads>(sdec);
    if constexpr ((YC && !LUTQ) || DUAL) enc_fill<kSliceThreads>(reinterpret_cast<uint2*>(senc), p.enc);
    {
        const half8* src = reinterpret_cast<const half8*>(p.whi) + (size_t)slice * wfrags * 64;
        for (int i = threadIdx.x; i < wfrags * 64; i += kSliceThreads) reinterpret_cast<half8*>(wl)[i] = src[i];
    }
    float* ep = reinterpret_cast<float*>(smem + (size_t)wfrags * 1024);   // [256 * bias/s1/s2 | post scale | post shift] of the slice
    constexpr int NCH = NTS * 16;
    const int n_lo = slice * NCH;
    const bool has_vec = p.bias != nullptr || p.post.scale != nullptr;
    if (has_vec) pw_fill_ep<kSliceThreads>(ep, p, n_lo, NCH);
    __syncthreads();
    const unsigned char* dtab = reinterpret_cast<const unsigned char*>(sdec);
    const CodeQuant cq{p.enc.r1, p.enc.lo, p.enc.hi, p.sgn, p.fmt_out};

    const int lane = threadIdx.x & 63;
    const int col = lane & 15, kq = lane >> 4;
    const int64_t n_groups = (p.M + 15) >> 4;
    const int64_t stride = (int64_t)n_ranks * (kSliceThreads / 64);
    const int n_chunks = p.KS / KC;

    u32x4 v[KC / 2];
    {
        const int64_t g0 = (int64_t)rank * (kSliceThreads / 64) + (threadIdx.x >> 6);
        const int64_t m0 = (g0 < n_groups ? g0 : n_groups - 1) * 16 + col;
        const uint8_t* x0 = p.x + x_row_offset(p, m0 < p.M ? m0 : p.M - 1) + kq * 16;
#pragma unroll
        for (int c2 = 0; c2 < KC / 2; ++c2) v[c2] = *reinterpret_cast<const u32x4*>(x0 + c2 * 64);
    }
    for (int64_t g = (int64_t)rank * (kSliceThreads / 64) + (threadIdx.x >> 6); g < n_groups; g += stride) {
        const int64_t m = g * 16 + col;
        const bool live = m < p.M;
        const uint8_t* xr = p.x + x_row_offset(p, live ? m : p.M - 1) + kq * 16;
        // first chunk of the next unit of this wave (its own unit again on the last round: L1 hits, unused)
        const int64_t gn = g + stride < n_groups ? g + stride : g;
        const int64_t mn = gn * 16 + col;
        const uint8_t* xrn = p.x + x_row_offset(p, mn < p.M ? mn : p.M - 1) + kq * 16;
        floatx4 acc[NTS];
#pragma unroll
        for (int j = 0; j < NTS; ++j) acc[j] = floatx4{0.f, 0.f, 0.f, 0.f};
        // RES: unconditional loads (dead rows / channels re-read a live element and are dropped)
        const float* rrow = (RES ? p.res : reinterpret_cast<const float*>(p.y)) + (size_t)(live ? m : p.M - 1) * p.N;
        auto res_at = [&](int j) { const int n = n_lo + j * 16 + kq * 4; return ld_stream4<SLFP_NT_PW_RES>(rrow + (n < p.N ? n : 0)); };
        float4 rq[NTS];
        if constexpr (RES) {
#pragma unroll
            for (int j = 0; j < RP && j < NTS; ++j) rq[j] = res_at(j);
        }
        for (int kc = 0; kc < n_chunks; ++kc) {
            half8 xh[KC];
#pragma unroll
            for (int c2 = 0; c2 < KC / 2; ++c2) {
                uint32_t a0 = v[c2][0], a1 = v[c2][1], a2 = v[c2][2], a3 = v[c2][3];
                rows_transpose4(a0, a1, a2, a3);
                xh[2 * c2] = dec_frag(a0, a1, dtab);
                xh[2 * c2 + 1] = dec_frag(a2, a3, dtab);
            }
            {   // the next chunk's codes -- after the last chunk: the next unit's first -- fly during this chunk's MFMAs
                const uint8_t* nx = kc + 1 < n_chunks ? xr + (kc + 1) * (KC * 32) : xrn;
#pragma unroll
                for (int c2 = 0; c2 < KC / 2; ++c2) v[c2] = *reinterpret_cast<const u32x4*>(nx + c2 * 64);
            }
            const _Float16* wk = wl + (size_t)(kc * KC) * 512 + lane * 8;
#pragma unroll
            for (int j = 0; j < NTS; ++j) {
#pragma unroll
                for (int ks = 0; ks < KC; ++ks) {
                    const half8 wh = *reinterpret_cast<const half8*>(wk + ((size_t)j * p.KS + ks) * 512);
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xh[ks], acc[j], 0, 0, 0);
                }
            }
        }
        auto finish = [&](int j) {   // j * 16 + kq * 4: channel inside the slice
            return pw_finish<!YC && !RES, false>(acc[j], p, ep, NCH, j * 16 + kq * 4, has_vec);
        };
        if constexpr (YC) {
            uint8_t* yr = reinterpret_cast<uint8_t*>(p.y) + (size_t)m * p.y_ld + n_lo;
#pragma unroll
            for (int j0 = 0; j0 < NTS; j0 += 4) pw_codes16_out<LUTQ, false>(j0, yr, live, n_lo, p.N, kq, cq, senc, finish, lutg);
        } else {
            float* yr = reinterpret_cast<float*>(p.y) + (size_t)m * p.N + n_lo + kq * 4;
            if constexpr (RES) {
#pragma unroll
                for (int j = RP; j < 2 * RP && j < NTS; ++j) rq[j] = res_at(j);
            }
            if constexpr (DUAL) {
                uint8_t* ycr = p.yc + (size_t)m * p.N + n_lo;
#pragma unroll
                for (int j0 = 0; j0 < NTS; j0 += 4) {   // pw_codes16_out spelled out: through it the NTS = 8 instances grew by 9 vector instructions
                    uint32_t c[4];
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        const int j = j0 + jj;
                        const float4 r = res_add(finish(j), rq[j], p.post.relu);
                        if (j + 2 * RP < NTS) rq[j + 2 * RP] = res_at(j + 2 * RP);
                        if (live && n_lo + j * 16 + kq * 4 < p.N) *reinterpret_cast<float4*>(yr + j * 16) = r;
                        c[jj] = code4<false, false>(r, cq, senc);
                    }
                    const int n = (j0 + kq) * 16;
                    store_codes16(c, ycr + n, live && n_lo + n < p.N);
                }
            } else {
#pragma unroll
                for (int j = 0; j < NTS; ++j) {
                    float4 r = finish(j);
                    if constexpr (RES) {
                        r = res_add(r, rq[j], p.post.relu);
                        if (j + 2 * RP < NTS) rq[j + 2 * RP] = res_at(j + 2 * RP);   // 2 RP pieces in flight: the consumed one's registers
                    }
                    if (live && n_lo + j * 16 + kq * 4 < p.N) *reinterpret_cast<float4*>(yr + j * 16) = r;
                }
            }
        }
    }
}


// ======================================================================================
// k_pwc_tiled: codes -> swizzled fp16 LDS tile (decoded once), W fragments straight from L2.
// ======================================================================================
// K a multiple of 64; NT = 4 channel tiles per wave.  STG-style float32 epilogue as in conv_pw.hip's k_pw_tiled.
// RES (float32 out): y = relu?(affine(conv) + res), the residual loaded in the staged layout one 16-row tile ahead, the first
// tile row's pieces in front of the staging barrier, while the last sweep's MFMAs drain.
// DUAL (RES only): the residual is added in the staged layout, where a lane holds 4 consecutive channels of one pixel: their 4 codes
// are one dword, stored by the lane itself -- the 16 lanes of a pixel row write the wave's 64 channels as 64 contiguous bytes.
// LUTQ (YC only): the table epilogue with the table in LDS, where the reader's threshold table lay (4.8 KiB instead of 2 KiB next to
// the 16 KiB X tile): W streams through the vector memory pipe here, LDS is idle in the epilogue.  (Unmeasured against global reads.)
// PASSES == 3 (SLFP<3,4> codes, plain float32 / code output only; slfp_conv2d_fwd_codes_x3): the float32-equivalent mode.  A buffer of
// the X tile holds the hi plane, then the lo plane (one kDecF16HL lookup per element fills both); the lo fragments of W (p.wlo) are
// double-buffered next to the hi ones; per k-step and accumulator (w_lo, x_hi), (w_hi, x_lo), (w_hi, x_hi) as conv_pw.hip's three-pass
// k_pw_tiled: the same accumulators bit for bit.
template <int FMT, int WM, int WN, int MT, bool YC, bool RES = false, bool DUAL = false, bool LUTQ = false, int PASSES = 1>
__global__ __launch_bounds__(64 * WM * WN, (WM * WN) <= 4 ? 2 : 4) void k_pwc_tiled(const PwcParams p) {
    static_assert(PASSES == 1 || (PASSES == 3 && FMT == kFmtAct8 && !RES && !DUAL && !LUTQ && WM * WN <= 4), "three passes: SLFP<3,4>, plain float32 or code output, 4 waves");
    constexpr int PL = PASSES == 3 ? 2 : 1;   // planes of X per LDS buffer
    static_assert(!RES || !YC, "residual operand: float32 output only");
    static_assert(!DUAL || RES, "the second, code output belongs to the residual forms");
    static_assert(!LUTQ || YC, "the table epilogue belongs to the code-writing forms");
    constexpr int NT = 4;
    using G = PwTile<WM, WN, MT, NT>;
    constexpr int T = G::T, BM = G::BM, BN = G::BN, XBYTES = G::XBYTES;
    constexpr int NLD = G::NLD;  // code dwords per thread per 64-deep stage

    __shared__ __attribute__((aligned(16))) uint32_t sdec[256];
    __shared__ __attribute__((aligned(16))) unsigned char senc[LUTQ ? kLayeroutLutBytes : ((YC || DUAL) ? kPwTab : 16)];
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* xs = smem;  // [2 buffers][PL planes][BM rows][128 B]
    dec_fill<FMT, PASSES == 3 ? kDecF16HL : kDecF16D, T>(sdec);
    if constexpr (LUTQ) layerout_lut_fill<T>(senc, enc_carried_ptr(p.enc));
    else if constexpr (YC || DUAL) enc_fill<T>(reinterpret_cast<uint2*>(senc), p.enc);
    const unsigned char* dtab = reinterpret_cast<const unsigned char*>(sdec);

    const uint32_t b = xcd_remap(blockIdx.x, p.nblocks);
    const uint32_t nb = b % p.n_blocks, mb = b / p.n_blocks;
    const int64_t m0 = (int64_t)mb * p.rb;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int col = lane & 15, kq = lane >> 4;

    // staging geometry (conv_pw_core.hpp): dword #i of a thread = the 4 codes of row (tid>>4) + i*(T/16), k = (tid&15)*4
    const int kc = threadIdx.x & 15;
    const int st_chunk = (kc >> 3) * 4 + (kc & 3);
    const uint32_t st_sub = (uint32_t)((kc & 7) >> 2) * 8u;
    const uint8_t* src[NLD];
#pragma unroll
    for (int i = 0; i < NLD; ++i) src[i] = p.x + pw_stage_row_offset<T>(p, m0, i) + kc * 4;
    uint32_t st[NLD];
    auto load_stage = [&](int t) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) st[i] = *reinterpret_cast<const uint32_t*>(src[i] + t * 64);
    };
    auto decode_store = [&](int buf) {
        unsigned char* hi = xs + (size_t)buf * PL * XBYTES;
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int row = (threadIdx.x >> 4) + i * (T / 16);
            if constexpr (PASSES == 3) {
                uint2 ph, pl;
                dec4_f16hl(st[i], dtab, ph, pl);
                *reinterpret_cast<uint2*>(hi + lds_x_off(row, st_chunk) + st_sub) = ph;
                *reinterpret_cast<uint2*>(hi + XBYTES + lds_x_off(row, st_chunk) + st_sub) = pl;
            } else {
                *reinterpret_cast<uint2*>(hi + lds_x_off(row, st_chunk) + st_sub) = dec4_f16(st[i], dtab);
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
    // W fragments by buffer loads (pw_w_rsrc, pw_w_offset): scalar addresses but for one vector register -- the double buffer
    // below needs the registers
    const int wn_u = __builtin_amdgcn_readfirstlane(wn);
    const int ntile0u = (int)nb * (BN / 16) + wn_u * NT;
    const __amdgpu_buffer_rsrc_t rw = pw_w_rsrc(p.whi, p);
    uint32_t wsoff[NT];   // scalar
#pragma unroll
    for (int j = 0; j < NT; ++j) wsoff[j] = pw_w_offset(p, ntile0u + j);
    const uint32_t wvoff = (uint32_t)lane * 16u;
    // W fragments double-buffered by k-step (a stage of codes is 2 registers per lane, so there is room -- the float32-interface
    // kernel has none): W(2t+1) is requested at the top of stage t, BEFORE the X loads of stage t+2, W(2t+2) once the first
    // k-step's MFMAs have read its buffer.  Every vmcnt wait is then for loads issued at least half a stage earlier, and no W
    // wait sits behind X loads that have not been waited for already (loads retire in order through one counter).
    half8 whb[2][NT];
    half8 wlb[2][PASSES == 3 ? NT : 1];   // PASSES == 3: the lo plane's fragments, same offsets behind p.wlo
    const __amdgpu_buffer_rsrc_t rwl = pw_w_rsrc(PASSES == 3 ? p.wlo : p.whi, p);
    auto load_w = [&](int kstep, int b) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rw, wvoff, wsoff[j] + (uint32_t)kstep * 1024u, 0);
            whb[b][j] = __builtin_bit_cast(half8, v);
            if constexpr (PASSES == 3)
                wlb[b][j] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rwl, wvoff, wsoff[j] + (uint32_t)kstep * 1024u, 0));
        }
    };
    // (this step stands in conv_pw.hip's k_pw_tiled too, there with single-buffered W and a diagnostic macro)
    auto mfma_step = [&](int buf, int ks, int b) {
        const unsigned char* hi = xs + (size_t)buf * PL * XBYTES;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int row = (wm * MT + i) * 16 + col;
            const half8 xh = *reinterpret_cast<const half8*>(hi + lds_x_off(row, ks * 4 + kq));
            if constexpr (PASSES == 3) {
                const half8 xl = *reinterpret_cast<const half8*>(hi + XBYTES + lds_x_off(row, ks * 4 + kq));
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wlb[b][j], xh, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(whb[b][j], xl, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(whb[b][j], xh, acc[i][j], 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(whb[b][j], xh, acc[i][j], 0, 0, 0);
            }
        }
    };

    load_stage(0);
    __syncthreads();  // tables visible
    decode_store(0);
    load_w(0, 0);
    load_stage(KT > 1 ? 1 : 0);
    __syncthreads();
    for (int t = 0; t + 1 < KT; ++t) {  // branch-free body
        const int buf = t & 1;
        load_w(t * 2 + 1, 1);
        decode_store(buf ^ 1);
        load_stage(t + 2 < KT ? t + 2 : KT - 1);
        __builtin_amdgcn_sched_barrier(0);
        mfma_step(buf, 0, 0);
        load_w(t * 2 + 2, 0);
        mfma_step(buf, 1, 1);
        __syncthreads();
    }
    // staged epilogue geometry (float32 out; this and the staged store loop below stand in k_pw_tiled too): piece h of tile row i = 4 pixel rows x the wave's 64 channels, 16 bytes per lane
    const int srow = lane >> 4, sch = lane & 15;
    const int n_st = ntile0 * 16 + sch * 4;
    const uint64_t yleft = (uint64_t)(p.M - m0) * p.N * 4;
    const uint32_t ybytes = (uint32_t)(yleft > 0xFFFFFFFFull ? 0xFFFFFFFFull : yleft);
    auto piece = [&](int i, int h) {   // byte offset from row m0 (stores and residual loads alike); out of range: dropped / 0
        const int row = (wm * MT + i) * 16 + h * 4 + srow;
        const bool ok = row < p.rb && m0 + row < p.M && n_st < p.N;
        return ok ? (uint32_t)(row * p.N + n_st) * 4u : 0xFFFFFFF0u;
    };
    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(RES ? p.res : reinterpret_cast<const float*>(p.y)) + (size_t)m0 * p.N, 0, ybytes, 0x00020000);
    u32x4 rq[4];   // RES: four residual pieces in flight (16 registers): piece h of the tile row that is stored next
    {
        const int t = KT - 1, buf = t & 1;
        load_w(t * 2 + 1, 1);
        mfma_step(buf, 0, 0);
        mfma_step(buf, 1, 1);
        // RES: requested behind the last sweep's MFMA issue, in the registers of the W buffers it frees (the 8-wave form sits
        // at its 128-VGPR cap): in flight while the matrix pipeline drains and through the epilogue vectors' barriers below
        if constexpr (RES) {
#pragma unroll
            for (int h = 0; h < 4; ++h) rq[h] = res_load_stg(rr, piece(0, h));
        }
    }

    const int n_lo = (int)nb * BN;
    float* lsc = reinterpret_cast<float*>(xs);   // the (now free) X tile
    float* lsh = lsc + BN;
    if (p.post.scale) {
        __syncthreads();
        pw_bn_slice_fill<BN, T>(lsc, lsh, p.post.scale, p.post.shift, p.N, n_lo);
        __syncthreads();
    }
    auto out_tile = [&](int i, int j) {   // with a residual the ReLU follows the add; with code output it is the quantizer's
        return pw_tile_finish<!YC && !RES, false>(acc[i][j], p, (ntile0 + j) * 16 + kq * 4, n_lo, lsc, lsh);
    };
    if constexpr (YC) {
        const CodeQuant cq{p.enc.r1, p.enc.lo, p.enc.hi, p.sgn, p.fmt_out};
        uint8_t* yb = reinterpret_cast<uint8_t*>(p.y);
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            uint32_t c[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const float4 r = out_tile(i, j);
                c[j] = code4<LUTQ, false>(r, cq, senc, senc);
            }
            const int row = (wm * MT + i) * 16 + col;
            const int n = (ntile0 + kq) * 16;   // after the transpose lane-quarter kq: channels 16 (ntile0 + kq) + 0..15 of pixel row `col`
            store_codes16(c, yb + (size_t)(m0 + row) * p.y_ld + n, row < p.rb && m0 + row < p.M && n < p.N);
        }
    } else {
        // float32 out: staged through a per-wave LDS area into 256-byte runs (4 rows x the wave's 64 channels per store)
        unsigned char* stg = xs + 2 * PL * XBYTES + wave * (16 * kStgRow);
        const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<float*>(p.y) + (size_t)m0 * p.N, 0, ybytes, 0x00020000);
        // DUAL: the workgroup's own rows of the code tensor and nothing more (offsets are relative to row m0)
        const uint64_t cleft = (uint64_t)(p.M - m0 < BM ? p.M - m0 : BM) * p.N;
        const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc((DUAL ? p.yc : reinterpret_cast<uint8_t*>(p.y)) + (size_t)m0 * p.N, 0,
                                                                            (uint32_t)cleft, 0x00020000);
        const CodeQuant cq{p.enc.r1, p.enc.lo, p.enc.hi, p.sgn, p.fmt_out};
#pragma unroll
        for (int i = 0; i < MT; ++i) {
#pragma unroll
            for (int j = 0; j < NT; ++j) *reinterpret_cast<float4*>(stg + col * kStgRow + j * 64 + kq * 16) = out_tile(i, j);
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
                asm volatile("" : "+v"(so));
                __builtin_amdgcn_raw_buffer_store_b128(v, ry, so, 0, 0);
                if constexpr (DUAL) {
                    const float4 f = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
                    const uint32_t c = code4<false, false>(f, cq, senc);
                    uint32_t co = ok ? (uint32_t)(row * p.N + n_st) : 0xFFFFFFF0u;   // out of range: dropped
                    asm volatile("" : "+v"(co));
                    __builtin_amdgcn_raw_buffer_store_b32(c, rc, co, 0, 0);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------- launch
static bool pwc_stream_fits(const ConvPlan& plan) { return pointwise_stream_fits(plan.k_pad, plan.n_pad, 1); }

bool pwc_applicable(const slfp_conv2d_desc& d, const ConvPlan& plan, int post_flags, bool y_codes) {
    if (plan.family != kPointwise || plan.repad || plan.passes != 1) return false;
    if (post_flags & SLFP_POST_LAYEROUT) return false;
    if (y_codes ? (d.c_out % 16 != 0) : (d.c_out % 4 != 0)) return false;
    // 16 and 48 channels (a half-live last k-step: k_pwc_stream's HALF form), inside the LDS-resident kernel's range only
    if (d.c_in == 16 || d.c_in == 48) return pwc_stream_fits(plan);
    if (d.c_in % 32 != 0) return false;
    if (pwc_stream_fits(plan)) {
        const int ks = (int)(d.c_in / 32);
        return ks == 1 || ks == 2 || ks == 3 || ks == 4 || ks == 8;   // 3: the 96 -> 16 squeeze behind SqueezeNet's stem
    }
    return d.c_in % 64 == 0;
}

// Everything a code-input pointwise launch decides, worked out in ONE place (pwc_select): the launchers below only dispatch on it
// and pwc_variant_name (slfp_debug_pw_variant) prints it, so the reported string cannot drift from what runs.
enum PwcKernel { kPwcStream = 0, kPwcSlice, kPwcTiled };
struct PwcSel {
    int kernel;
    int fmt;                 // template argument FMT
    bool yc, res, dual;      // template arguments YC / RES / DUAL
    int ks; bool xw, half;   // k_pwc_stream: KS, XW, HALF
    int nts;                 // k_pwc_slice: NTS (4 or 8)
    int wm, wn, mt;          // k_pwc_tiled: tiling
    int grid_cap;            // SLFP_PW_GRID: k_pwc_stream: the most workgroups; k_pwc_slice: the most rank groups (0: no cap)
    bool lut;                // template argument LUTQ (yc only): set by the caller after pwc_select; the tiling does not depend on it
    int passes;              // template argument PASSES: 3 from pwc_x3_select (slfp_conv2d_fwd_codes_x3), else 1 (0 reads as 1)
};

// slice kernel: K a multiple of 256, the slice's W (NTS tiles x K) <= 128 KiB, N a multiple of 16 * NTS
static int pwc_slice_nts(int K, int N, int n_tiles) {
    if (K != 256 || !switches().pwc_slice) return 0;   // see k_pwc_slice: deeper layers stay on k_pwc_tiled
    for (int nts : {8, 4}) {
        if ((size_t)nts * 16 * K * 2 <= 128 * 1024 && N % (nts * 16) == 0 && n_tiles % nts == 0) return nts;
    }
    return 0;
}

static int pwc_select(int K, int N, const ConvPlan& plan, bool y_codes, bool has_res, bool has_dual, PwcSel* s) {
    *s = PwcSel{};
    s->fmt = plan.fmt_act == kFmtSfp7 ? kFmtSfp7 : kFmtAct8;
    s->yc = y_codes; s->dual = !y_codes && has_dual; s->res = !y_codes && (has_res || has_dual);
    if (const int nts = pwc_slice_nts(K, N, (int)(plan.n_pad / 16))) {
        s->kernel = kPwcSlice;
        s->nts = nts;
        s->grid_cap = switches().pw_grid;
        return SLFP_OK;
    }
    if (pwc_stream_fits(plan)) {
        s->kernel = kPwcStream;
        s->grid_cap = switches().pw_grid;
        if (K == 16 || K == 48) { s->ks = (K + 16) / 32; s->half = true; return SLFP_OK; }
        s->ks = K / 32;
        s->xw = s->ks % 2 == 0;   // K a multiple of 64: 16-byte code loads + transpose
        if (K % 32 == 0 && (s->ks == 1 || s->ks == 2 || s->ks == 3 || s->ks == 4 || s->ks == 8)) return SLFP_OK;
        return fail(SLFP_ERR_UNSUPPORTED, "pointwise (codes): unsupported channel count %d", K);
    }
    s->kernel = kPwcTiled;
    const PwTiling t = pw_tiling(N, true);
    s->wm = t.wm; s->wn = t.wn; s->mt = t.mt;
    return SLFP_OK;
}

static const char* pwc_sel_name(const PwcSel& s) {
    static thread_local char buf[64];
    const char* fmt = pw_fmt_word(s.fmt);
    const char* form = s.yc ? (s.lut ? "yc-lut" : "yc") : (s.dual ? "res/dual" : (s.res ? "res" : "f32"));
    int n;
    if (s.kernel == kPwcStream) n = snprintf(buf, sizeof buf, "pwc-stream/ks%d/%s/%s/%s", s.ks, s.half ? "half" : (s.xw ? "xw" : "dw"), fmt, form);
    else if (s.kernel == kPwcSlice) n = snprintf(buf, sizeof buf, "slice/nts%d/%s/%s", s.nts, fmt, form);
    else n = snprintf(buf, sizeof buf, "pwc-tiled/%d%d%d/%s/%s", s.wm, s.wn, s.mt, fmt, form);
    if (s.passes == 3) n += snprintf(buf + n, sizeof buf - n, "/p3");
    if (s.kernel != kPwcTiled && s.grid_cap > 0) snprintf(buf + n, sizeof buf - n, "/grid%d", s.grid_cap);
    return buf;
}

// From the selection to the kernel: one typed lookup per kernel template.  nullptr: the launchers have no such instance.  launch_pwc_sel
// launches what the lookup returns and the name functions ask it before they print a name.  The restrictions of the table epilogue
// (LUT_OK) and of the three-pass mode live here, not in the kernels.
typedef void (*PwcFn)(const PwcParams);

template <int FMT, int KS, bool XW, bool HALF = false, int PASSES = 1>
static PwcFn pwc_stream_form(const PwcSel& s) {
    // the table epilogue: the whole-tile k-step counts the layerout nets' 1x1 layers have (32 / 64 / 128 input channels)
    constexpr bool LUT_OK = PASSES == 1 && !HALF && (KS == 1 || KS == 2 || KS == 4);
    if (s.lut && !LUT_OK) return nullptr;
    if constexpr (PASSES == 3) {   // plain float32 or code output only
        if (s.res || s.dual) return nullptr;
        return s.yc ? k_pwc_stream<FMT, KS, XW, true, false, false, false, false, 3> : k_pwc_stream<FMT, KS, XW, false, false, false, false, false, 3>;
    } else {
        if (s.yc) return s.lut ? k_pwc_stream<FMT, KS, XW, true, false, HALF, false, LUT_OK> : k_pwc_stream<FMT, KS, XW, true, false, HALF>;
        if (s.dual) return k_pwc_stream<FMT, KS, XW, false, true, HALF, true>;
        return s.res ? k_pwc_stream<FMT, KS, XW, false, true, HALF> : k_pwc_stream<FMT, KS, XW, false, false, HALF>;
    }
}
template <int FMT, int PASSES>
static PwcFn pwc_stream_instance_fp(const PwcSel& s) {
    if (s.half) {
        if constexpr (PASSES == 1) {
            if (s.ks == 1) return pwc_stream_form<FMT, 1, false, true>(s);
            if (s.ks == 2) return pwc_stream_form<FMT, 2, false, true>(s);
        }
        return nullptr;
    }
    switch (s.ks * 2 + (s.xw ? 1 : 0)) {
        case 2: return pwc_stream_form<FMT, 1, false, false, PASSES>(s);
        case 5: return pwc_stream_form<FMT, 2, true, false, PASSES>(s);
        case 6: return pwc_stream_form<FMT, 3, false, false, PASSES>(s);
        case 9: return pwc_stream_form<FMT, 4, true, false, PASSES>(s);
        case 17: return pwc_stream_form<FMT, 8, true, false, PASSES>(s);
        default: return nullptr;
    }
}
static PwcFn pwc_stream_instance(const PwcSel& s) {
    if (s.passes == 3) return s.fmt == kFmtAct8 ? pwc_stream_instance_fp<kFmtAct8, 3>(s) : nullptr;
    return s.fmt == kFmtSfp7 ? pwc_stream_instance_fp<kFmtSfp7, 1>(s) : pwc_stream_instance_fp<kFmtAct8, 1>(s);
}

template <int FMT, int WM, int WN, int MT, int PASSES>
static PwcFn pwc_tiled_form(const PwcSel& s) {
    constexpr bool LUT_OK = PASSES == 1 && WM == 1 && WN == 8 && MT == 4;   // the table epilogue: the deep layers (C_out > 256)
    if (s.lut && !LUT_OK) return nullptr;
    if constexpr (PASSES == 3) {   // plain float32 or code output only
        if (s.res || s.dual) return nullptr;
        return s.yc ? k_pwc_tiled<FMT, WM, WN, MT, true, false, false, false, 3> : k_pwc_tiled<FMT, WM, WN, MT, false, false, false, false, 3>;
    } else {
        if (s.yc) return s.lut ? k_pwc_tiled<FMT, WM, WN, MT, true, false, false, LUT_OK> : k_pwc_tiled<FMT, WM, WN, MT, true>;
        if (s.dual) return k_pwc_tiled<FMT, WM, WN, MT, false, true, true>;
        return s.res ? k_pwc_tiled<FMT, WM, WN, MT, false, true> : k_pwc_tiled<FMT, WM, WN, MT, false>;
    }
}
template <int FMT, int PASSES>
static PwcFn pwc_tiled_instance_fp(const PwcSel& s) {
    return pw_tiling_instance<PASSES == 1>(s.wm, s.wn, s.mt, [&](auto t) -> PwcFn {
        using G = decltype(t);
        return pwc_tiled_form<FMT, G::kWM, G::kWN, G::kMT, PASSES>(s);
    });
}
static PwcFn pwc_tiled_instance(const PwcSel& s) {
    if (s.passes == 3) return s.fmt == kFmtAct8 ? pwc_tiled_instance_fp<kFmtAct8, 3>(s) : nullptr;
    return s.fmt == kFmtSfp7 ? pwc_tiled_instance_fp<kFmtSfp7, 1>(s) : pwc_tiled_instance_fp<kFmtAct8, 1>(s);
}

template <int FMT, int NTS>
static PwcFn pwc_slice_form(const PwcSel& s) {
    constexpr bool LUT_OK = NTS == 8;   // the table epilogue: 256 -> 256 / 512
    if (s.lut && !LUT_OK) return nullptr;
    if (s.yc) return s.lut ? k_pwc_slice<FMT, NTS, true, false, false, LUT_OK> : k_pwc_slice<FMT, NTS, true>;
    if (s.dual) return k_pwc_slice<FMT, NTS, false, true, true>;
    return s.res ? k_pwc_slice<FMT, NTS, false, true> : k_pwc_slice<FMT, NTS, false>;
}
static PwcFn pwc_slice_instance(const PwcSel& s) {
    if (s.passes == 3) return nullptr;
    if (s.nts == 8) return s.fmt == kFmtSfp7 ? pwc_slice_form<kFmtSfp7, 8>(s) : pwc_slice_form<kFmtAct8, 8>(s);
    if (s.nts == 4) return s.fmt == kFmtSfp7 ? pwc_slice_form<kFmtSfp7, 4>(s) : pwc_slice_form<kFmtAct8, 4>(s);
    return nullptr;
}

static PwcFn pwc_instance(const PwcSel& s) {
    return s.kernel == kPwcSlice ? pwc_slice_instance(s) : (s.kernel == kPwcStream ? pwc_stream_instance(s) : pwc_tiled_instance(s));
}

static int launch_pwc_slice(PwcFn fn, PwcParams& p, const PwcSel& s, hipStream_t stream) {
    const size_t lds = (size_t)s.nts * p.KS * 1024 + (size_t)3 * s.nts * 16 * sizeof(float);
    int rc = raise_lds_limit(reinterpret_cast<const void*>(fn), lds);
    if (rc != SLFP_OK) return rc;
    int per_cu = resident_blocks_per_cu(reinterpret_cast<const void*>(fn), kSliceThreads, lds);
    per_cu = per_cu < 1 ? 1 : (per_cu > 2 ? 2 : per_cu);
    const int n_slices = p.n_tiles / s.nts;
    // grid = 8 (XCDs) x n_slices x ranks-per-XCD: as many whole (slice set) groups as fit the device
    const int64_t slots = (int64_t)device_cu_count() * per_cu;
    int64_t groups = slots / (8 * n_slices);
    if (groups < 1) groups = 1;
    const int64_t units = (p.M + 15) / 16;
    const int64_t need = ceil_div(units, (int64_t)8 * (kSliceThreads / 64));   // ranks needed, in multiples of 8 (one per XCD)
    if (groups > need) groups = need < 1 ? 1 : need;
    if (s.grid_cap > 0 && groups > s.grid_cap) groups = s.grid_cap;   // SLFP_PW_GRID: the grid stays a multiple of 8 * n_slices
    const int64_t grid = groups * 8 * n_slices;
    hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(kSliceThreads), lds, stream, p);
    return check_launch("slfp pointwise (codes, slice) kernel");
}

// Launches the instance of a selection (pwc_select or pwc_x3_select).
static int launch_pwc_sel(PwcParams& p, const PwcSel& s, hipStream_t stream) {
    const PwcFn fn = pwc_instance(s);
    if (!fn) return fail(SLFP_ERR_UNSUPPORTED, "pointwise (codes): no kernel instance for %s", pwc_sel_name(s));
    if (s.kernel == kPwcSlice) return launch_pwc_slice(fn, p, s, stream);
    if (s.kernel == kPwcTiled)   // float32 out: the staged epilogue
        return pw_launch_tiled(fn, p, PwTiling{s.wm, s.wn, s.mt}, s.passes, !s.yc, stream, "pointwise (codes)", "slfp pointwise (codes, tiled) kernel");
    const size_t lds = (size_t)(s.passes == 3 ? 2 : 1) * p.n_tiles * p.KS * 1024 + (size_t)3 * p.n_tiles * 16 * sizeof(float);
    return pw_launch_stream(fn, p, lds, s.grid_cap, stream, "slfp pointwise (codes, stream) kernel");
}

// ---- float32-equivalent (three-pass) mode: slfp_conv2d_fwd_codes_x3 ----
// The selection, as pwc_select with two planes of W: the LDS-resident kernel where both planes fit and it has the k-step count, else
// the tiled kernel (K a multiple of 64; also what the single-pass path gives to k_pwc_slice or to the 8-wave tiling: three passes
// hold the lo fragments in registers next to the hi ones, which the 128-VGPR forms have no room for).
static int pwc_x3_select(int K, int N, const ConvPlan& plan, bool y_codes, PwcSel* s) {
    *s = PwcSel{};
    s->fmt = kFmtAct8; s->yc = y_codes; s->passes = 3;
    if (K % 32 != 0) return fail(SLFP_ERR_UNSUPPORTED, "pointwise (codes, three passes): unsupported channel count %d", K);
    const int ks = K / 32;
    if (pointwise_stream_fits(plan.k_pad, plan.n_pad, 3) && (ks == 1 || ks == 2 || ks == 3 || ks == 4 || ks == 8)) {
        s->kernel = kPwcStream;
        s->grid_cap = switches().pw_grid;
        s->ks = ks;
        s->xw = ks % 2 == 0;
        return SLFP_OK;
    }
    if (K % 64 != 0) return fail(SLFP_ERR_UNSUPPORTED, "pointwise (codes, three passes): unsupported channel count %d", K);
    s->kernel = kPwcTiled;
    const PwTiling t = pw_tiling(N, false);   // the x3 path never takes {1, 8, 4}
    s->wm = t.wm; s->wn = t.wn; s->mt = t.mt;
    return SLFP_OK;
}

const char* pwc_x3_variant_name(const slfp_conv2d_desc& d, const ConvPlan& plan, bool y_codes) {
    PwcSel s;
    if (plan.family != kPointwise || plan.passes != 3 || pwc_x3_select((int)d.c_in, (int)d.c_out, plan, y_codes, &s) != SLFP_OK) return "none";
    return pwc_instance(s) ? pwc_sel_name(s) : "none";
}

bool pwc_x3_applicable(const slfp_conv2d_desc& d, const ConvPlan& plan, int post_flags, bool y_codes) {
    if (plan.family != kPointwise || plan.repad || plan.passes != 3 || plan.fmt_act != kFmtAct8) return false;
    if (post_flags & SLFP_POST_LAYEROUT) return false;
    if (y_codes ? (d.c_out % 16 != 0) : (d.c_out % 4 != 0)) return false;
    return strcmp(pwc_x3_variant_name(d, plan, y_codes), "none") != 0;
}

// What every code-input pointwise launch takes from the descriptor and the plan.
static void pwc_fill(PwcParams& p, const slfp_conv2d_desc& d, const ConvPlan& plan, const uint8_t* x, const void* wfrag, const float* bias,
                     const PostOp& post, void* y, const CodeIo& io) {
    p.post = post;
    p.x = x; p.bias = bias; p.y = y; p.res = nullptr; p.yc = nullptr;
    pw_fill_geom(p, d, plan);
    p.y_ld = io.y_ld ? (int)io.y_ld : p.N;
    p.whi = reinterpret_cast<const _Float16*>(wfrag);
    p.wlo = plan.passes == 3 ? p.whi + (size_t)plan.n_pad * plan.k_pad : nullptr;
    p.sgn = post.relu ? 0 : 1;
    p.fmt_out = io.y_fmt;
    p.enc.valid = 0;
}

int launch_pwc_x3(const slfp_conv2d_desc& d, const ConvPlan& plan, const uint8_t* x, const void* wfrag, const float* bias,
                  const PostOp& post, void* y, const CodeIo& io, hipStream_t stream) {
    if (plan.passes != 3) return fail(SLFP_ERR_UNSUPPORTED, "pointwise (codes, three passes): a float32-equivalent SLFP<3,4> descriptor is required");
    if (io.y_ld || io.lut) return fail(SLFP_ERR_UNSUPPORTED, "pointwise (codes, three passes): no channel-slice or table-epilogue form");
    PwcParams p;
    pwc_fill(p, d, plan, x, wfrag, bias, post, y, io);
    if (io.y_codes) {
        const EncArgs* t = enc_table(io.y_ka, io.y_fmt, kEncCode);
        if (!t->valid) return fail(SLFP_ERR_UNSUPPORTED, "pointwise (codes): no code table for the consumer's scale %g", (double)io.y_ka);
        p.enc = *t;
    }
    PwcSel s;
    const int rc = pwc_x3_select(p.K, p.N, plan, io.y_codes, &s);
    if (rc != SLFP_OK) return rc;
    return launch_pwc_sel(p, s, stream);
}

int launch_pwc(const slfp_conv2d_desc& d, const ConvPlan& plan, const uint8_t* x, const void* wfrag, const float* bias,
               const PostOp& post, void* y, const CodeIo& io, hipStream_t stream, const float* res, void* res_codes) {
    const bool y_codes = io.y_codes;
    const int64_t y_ld = io.y_ld;
    if (res && y_codes) return fail(SLFP_ERR_UNSUPPORTED, "pointwise (codes): a residual operand needs float32 output");
    if (res_codes && (!res || d.c_out % 16 != 0))
        return fail(SLFP_ERR_UNSUPPORTED, "pointwise (codes): the second, code output needs a residual operand and C_out a multiple of 16");
    if (y_ld && (!y_codes || y_ld < d.c_out || y_ld % 16 || y_ld > 0x7FFFFFFF))
        return fail(SLFP_ERR_BAD_ARG, "pointwise (codes): a channel-slice output needs code output and a pixel stride that is a multiple of 16, >= C_out");
    PwcParams p;
    pwc_fill(p, d, plan, x, wfrag, bias, post, y, io);
    p.res = res; p.yc = reinterpret_cast<uint8_t*>(res_codes);
    if (io.lut) {
        if (!y_codes || res || !post.scale) return fail(SLFP_ERR_BAD_ARG, "pointwise (codes): the table epilogue needs code output and post_scale / post_shift");
        enc_carry_ptr(p.enc, io.lut);
    } else if (y_codes || res_codes) {   // io.y_ka / io.y_fmt: the reader of the codes, in y or (DUAL) next to the float32 y
        const EncArgs* t = enc_table(io.y_ka, io.y_fmt, kEncCode);
        if (!t->valid) return fail(SLFP_ERR_UNSUPPORTED, "pointwise (codes): no code table for the consumer's scale %g", (double)io.y_ka);
        p.enc = *t;
    }
    PwcSel s;
    const int rc = pwc_select(p.K, p.N, plan, y_codes, res != nullptr, res_codes != nullptr, &s);
    if (rc != SLFP_OK) return rc;
    s.lut = io.lut != nullptr;
    return launch_pwc_sel(p, s, stream);
}

const char* pwc_variant_name(const slfp_conv2d_desc& d, const ConvPlan& plan, bool y_codes, bool has_res, bool has_dual, bool lut) {
    PwcSel s;
    if (plan.family != kPointwise || pwc_select((int)d.c_in, (int)d.c_out, plan, y_codes, has_res, has_dual, &s) != SLFP_OK) return "none";
    s.lut = lut;
    return pwc_instance(s) ? pwc_sel_name(s) : "none";
}

}  // namespace slfp
