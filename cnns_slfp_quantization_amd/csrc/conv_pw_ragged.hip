// conv_pw_ragged.hip -- the two 1x1 layers at the ends of a ShuffleNetV2 residual branch, gfx950 matrix cores.
//
// A branch is [1x1, BN, layerout, ReLU, dw3x3, BN, 1x1, BN, layerout, ReLU] on c = 58 / 116 / 232 channels (24 .. 488 at the other
// width ratios): no multiple of 16, so neither conv_pw.hip's code output nor conv_pw_codes.hip's code input takes it.  Inside the
// branch the hand-over tensors are private, so their pixel pitch is free: codes are stored with P = round_up(c, 32) bytes per pixel,
// the padding bytes 0x00.  The prepared blob holds zero weights up to k_pad / n_pad, so padding contributes exact zeros, and the
// depthwise 3x3 in the middle is an ordinary C = P layer of k_dwc.  What is left is one kernel per end, each with a ragged float32
// side:
//   k_pwr_entry  float32 channel slice (any even c_in, pitch x_ld floats: the split of the trunk is never copied) -> the layer's
//                quantizer (threshold table) -> MFMA -> affine -> layer-output class -> byte table T (folded ReLU + the reader's
//                quantizer, slfp_layerout_lut.hpp) -> codes at pitch y_ld, channels c_out .. y_ld - 1 stored as 0x00.
//   k_pwr_exit   codes at pitch x_ld -> decode table -> MFMA -> affine -> layer-output quantizer -> ReLU -> float32 channel i at
//                y[pix * y_ld + y_c0 + i * y_cs].  With y_cs = 2 and a `pass` operand the kernel also copies pass[pix][i] in front
//                of result i: concat + channel_shuffle(., 2) of a unit are the store pattern of its last layer.  A wave stages a
//                tile's results in LDS and leaves with (pass, result) pairs in 128-byte runs of the 2c-channel row.
// Both: wave64, v_mfma_f32_16x16x32_f16, the layer's own slfp_conv2d_prepare_weights blob resident in LDS, persistent over 16-pixel
// wave units with a ragged last unit, one MFMA per 32-deep k-step in ascending k from +0 (the accumulators of k_pw_stream /
// k_pwc_stream bit for bit), single-pass mode.  Only the ceil(c_in / 32) k-steps that hold real channels are swept.
#include "slfp_device.hpp"
#include "slfp_enc.hpp"
#include "slfp_codes.hpp"
#include "slfp_layerout_lut.hpp"
#include "slfp_epilogue.hpp"
#include "slfp_host.hpp"
#include "conv_pw_core.hpp"

namespace slfp {

struct PwrParams {
    const void* x;         // entry: float32, exit: codes
    const _Float16* whi;
    const float* bias;
    void* y;               // entry: codes, exit: float32
    const float* pass;     // exit, y_cs == 2: the float32 slice interleaved in front of the results; nullptr otherwise
    const uint8_t* lut;    // entry: the byte table of the layer-output classes (device memory)
    int64_t M;             // pixels
    int K, N;              // real input / output channels
    int KS, n_tiles;       // the blob: 32-deep k-steps per channel tile (k_pad / 32), 16-channel tiles (n_pad / 16)
    int x_ld, y_ld, pass_ld;   // pixel pitches in elements of the tensor's type
    int y_c0, y_cs;        // exit: first output channel and channel stride
    float s1, s2, s1x;
    PostOp post;
    EncArgs enc;           // entry: threshold table of fp16(16 * QA(x / Ka))
};
static_assert(sizeof(PwrParams) <= 4096, "PwrParams must fit the 4 KiB kernel-argument segment");

constexpr int kPwrStgRow = 20;                  // floats per staged pixel row: 16 channels + 4 (16-byte aligned, rows spread over the banks)
constexpr int kPwrStgWave = 16 * kPwrStgRow;    // floats per wave

// The W blob and the epilogue vectors -> LDS; returns the vectors' address.  The caller's __syncthreads() publishes both.
__device__ __forceinline__ float* pwr_fill_w(unsigned char* smem, const PwrParams& p, const bool has_vec) {
    const int wfrags = p.n_tiles * p.KS;   // 1 KiB each
    for (int i = threadIdx.x; i < wfrags * 64; i += kStreamThreads)
        reinterpret_cast<half8*>(smem)[i] = reinterpret_cast<const half8*>(p.whi)[i];
    float* ep = reinterpret_cast<float*>(smem + (size_t)wfrags * 1024);   // [256 * bias/s1/s2 | post scale | post shift]
    if (has_vec) pw_fill_ep<kStreamThreads>(ep, p, 0, p.n_tiles * 16);
    return ep;
}

// ======================================================================================
// k_pwr_entry: float32 slice -> codes behind the layer-output table.  KS: k-steps swept = ceil(K / 32).
// ======================================================================================
template <int KS>
__global__ __launch_bounds__(kStreamThreads) void k_pwr_entry(const PwrParams p) {
    __shared__ __attribute__((aligned(16))) unsigned char stab[kPwTab];
    __shared__ __attribute__((aligned(16))) unsigned char slut[kLayeroutLutBytes];
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const _Float16* wl = reinterpret_cast<const _Float16*>(smem);
    enc_fill<kStreamThreads>(reinterpret_cast<uint2*>(stab), p.enc);
    layerout_lut_fill<kStreamThreads>(slut, (lut_gptr)p.lut);
    const float* ep = pwr_fill_w(smem, p, true);
    __syncthreads();
    const int n_pad = p.n_tiles * 16;

    const int lane = threadIdx.x & 63;
    const int col = lane & 15, kq = lane >> 4;
    const int64_t n_groups = (p.M + 15) >> 4;
    const int64_t waves_total = (int64_t)gridDim.x * (kStreamThreads / 64);
    const int64_t wave_id = (int64_t)blockIdx.x * (kStreamThreads / 64) + (threadIdx.x >> 6);
    const float* xb = reinterpret_cast<const float*>(p.x);

    for (int64_t g = wave_id; g < n_groups; g += waves_total) {
        const int64_t m = g * 16 + col;
        const bool live = m < p.M;
        const float* row = xb + (size_t)(live ? m : p.M - 1) * p.x_ld;   // rows past the end: clamped, computed, dropped
        // 8-byte lanes bounded by K (K is even: each half is all real or all padding); unconditional loads at clamped offsets
        float4 raw[KS][2];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int k = ks * 32 + hf * 16 + kq * 4;
                float2 a = *reinterpret_cast<const float2*>(row + (k < p.K ? k : p.K - 2));
                float2 b = *reinterpret_cast<const float2*>(row + (k + 2 < p.K ? k + 2 : p.K - 2));
                if (k >= p.K) a = make_float2(0.f, 0.f);
                if (k + 2 >= p.K) b = make_float2(0.f, 0.f);
                raw[ks][hf] = make_float4(a.x, a.y, b.x, b.y);
            }
        }
        half8 xh[KS], xl[1];
        bool any_nan = false;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const bool na = enc_has_nan4(raw[ks][0]), nb = enc_has_nan4(raw[ks][1]);
            any_nan |= na;
            any_nan |= nb;
            const uint2 pa = enc4_f16_raw(raw[ks][0], p.enc.r1, p.enc.lo, p.enc.hi, stab), pb = enc4_f16_raw(raw[ks][1], p.enc.r1, p.enc.lo, p.enc.hi, stab);
            xh[ks] = __builtin_bit_cast(half8, u32x4{pa.x, pa.y, pb.x, pb.y});
        }
        if (__builtin_expect(any_nan, 0)) {   // NaN in -> NaN out; never taken on real activations
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const uint2 pa = enc4_f16(raw[ks][0], p.enc.r1, p.enc.lo, p.enc.hi, stab), pb = enc4_f16(raw[ks][1], p.enc.r1, p.enc.lo, p.enc.hi, stab);
                xh[ks] = __builtin_bit_cast(half8, u32x4{pa.x, pa.y, pb.x, pb.y});
            }
        }

        uint8_t* yr = reinterpret_cast<uint8_t*>(p.y) + (size_t)m * p.y_ld;
        for (int j0 = 0; j0 * 16 < p.y_ld; j0 += 4) {   // groups of four channel tiles = 64 code bytes of the pixel
            uint32_t c[4];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int j = j0 + jj, n = j * 16 + kq * 4;
                c[jj] = 0u;   // tiles past the blob and channels past C_out: 0x00
                if (j < p.n_tiles && j * 16 < p.N) {   // wave-uniform
                    const floatx4 acc = pw_sweep_lds<1, KS>(wl + ((size_t)j * p.KS) * 512 + lane * 8, 0, xh, xl);
                    const float4 r = pw_finish<false, false>(acc, p, ep, n_pad, n, true);   // the table holds layerout's image, ReLU and quantizer
                    const int left = p.N - n;   // real channels among this lane's four (C_out is even: 0, 2 or 4 at the ragged end)
                    const uint32_t keep = left >= 4 ? 0xFFFFFFFFu : (left <= 0 ? 0u : (1u << (8 * left)) - 1u);
                    c[jj] = lut4_code(r, slut) & keep;
                }
            }
            const int n16 = (j0 + kq) * 16;
            store_codes16(c, yr + n16, live && n16 < p.y_ld);
        }
    }
}

// ======================================================================================
// k_pwr_exit: padded codes -> float32 behind the layer-output epilogue, written with a channel offset and stride.
// ======================================================================================
// KS: k-steps swept = ceil(K / 32) (x_ld >= 32 * KS); KS even: 16-byte code loads + transpose (x_ld is a multiple of 32 and x is
// 16-byte aligned), else two dwords per k-step -- k_pwc_stream's two load paths.  PASS: the interleaving form (y_cs == 2).
template <int FMT, int KS, bool PASS>
__global__ __launch_bounds__(kStreamThreads) void k_pwr_exit(const PwrParams p) {
    constexpr bool XW = KS % 2 == 0;
    __shared__ __attribute__((aligned(16))) uint32_t sdec[256];
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const _Float16* wl = reinterpret_cast<const _Float16*>(smem);
    dec_fill<FMT, kDecF16D, kStreamThreads>(sdec);
    const bool has_vec = p.bias != nullptr || p.post.scale != nullptr;   // wave-uniform
    float* ep = pwr_fill_w(smem, p, has_vec);
    __syncthreads();
    const int n_pad = p.n_tiles * 16;
    const unsigned char* dtab = reinterpret_cast<const unsigned char*>(sdec);
    float* stg = ep + 3 * n_pad + (threadIdx.x >> 6) * kPwrStgWave;   // PASS: this wave's 16 pixels x 16 channels

    const int lane = threadIdx.x & 63;
    const int col = lane & 15, kq = lane >> 4;
    const int64_t n_groups = (p.M + 15) >> 4;
    const int64_t waves_total = (int64_t)gridDim.x * (kStreamThreads / 64);
    const int64_t wave_id = (int64_t)blockIdx.x * (kStreamThreads / 64) + (threadIdx.x >> 6);
    const uint8_t* xb = reinterpret_cast<const uint8_t*>(p.x);
    float* yb = reinterpret_cast<float*>(p.y);

    for (int64_t g = wave_id; g < n_groups; g += waves_total) {
        const int64_t m = g * 16 + col;
        const bool live = m < p.M;
        const uint8_t* xr = xb + (size_t)(live ? m : p.M - 1) * p.x_ld;   // rows past the end: clamped, computed, dropped
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
                cw[ks][1] = *reinterpret_cast<const uint32_t*>(xr + ks * 32 + 16 + kq * 4);
            }
        }
        half8 xh[KS], xl[1];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const uint2 pa = dec4_f16(cw[ks][0], dtab), pb = dec4_f16(cw[ks][1], dtab);
            xh[ks] = __builtin_bit_cast(half8, u32x4{pa.x, pa.y, pb.x, pb.y});
        }

        for (int j = 0; j * 16 < p.N; ++j) {
            const int n = j * 16 + kq * 4;
            float pv[4];
            if constexpr (PASS) {   // the shortcut values of this tile, in the layout of the stores below, in flight under the sweep
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int64_t mm = g * 16 + 4 * i + kq;
                    const int ch = j * 16 + col;
                    const bool ok = mm < p.M && ch < p.N;
                    pv[i] = p.pass[ok ? (size_t)mm * p.pass_ld + ch : 0];   // unconditional: dead lanes re-read a live element
                }
            }
            const floatx4 acc = pw_sweep_lds<1, KS>(wl + ((size_t)j * p.KS) * 512 + lane * 8, 0, xh, xl);
            const float4 r = pw_finish<true, true>(acc, p, ep, n_pad, n, has_vec);
            if constexpr (PASS) {
                // LDS operations of one wave execute in order: the reads see the writes, the next tile's writes follow the reads
                *reinterpret_cast<float4*>(stg + col * kPwrStgRow + kq * 4) = r;
#pragma unroll
                for (int i = 0; i < 4; ++i) {   // store i: pixels 4i .. 4i + 3, 16 (pass, result) pairs = 128 contiguous bytes each
                    const int px = 4 * i + kq;
                    const int64_t mm = g * 16 + px;
                    const int ch = j * 16 + col;
                    const float v = stg[px * kPwrStgRow + col];
                    if (mm < p.M && ch < p.N)
                        *reinterpret_cast<float2*>(yb + (size_t)mm * p.y_ld + (p.y_c0 - 1) + 2 * ch) = make_float2(pv[i], v);
                }
            } else {   // 8-byte lanes: rows and the channel offset are only 8-byte aligned
                float* yr = yb + (size_t)m * p.y_ld + p.y_c0 + n;
                if (live && n < p.N) *reinterpret_cast<float2*>(yr) = make_float2(r.x, r.y);
                if (live && n + 2 < p.N) *reinterpret_cast<float2*>(yr + 2) = make_float2(r.z, r.w);
            }
        }
    }
}

// ---------------------------------------------------------------------------- selection and launch
// Everything a launch decides, worked out in ONE place (pwr_select): the launchers dispatch on it and pwr_instance_name
// (slfp_debug_pwr_instance) prints it, so the reported string cannot drift from what runs.
struct PwrSel {
    bool entry;      // k_pwr_entry, else k_pwr_exit
    int fmt;         // exit: template argument FMT (what the input codes are)
    int ks;          // template argument KS
    bool pass;       // exit: template argument PASS
    int grid_cap;    // SLFP_PW_GRID
    size_t lds;      // dynamic LDS of the launch
};
constexpr size_t kPwrLdsBudget = 160 * 1024;

static int pwr_select(const slfp_conv2d_desc& d, const ConvPlan& plan, bool entry, bool pass, PwrSel* s) {
    *s = PwrSel{};
    const char* who = entry ? "pointwise entry (table)" : "pointwise exit (layerout)";
    if (plan.family != kPointwise || plan.repad || d.c_in % 2 || d.c_out % 2)
        return fail(SLFP_ERR_UNSUPPORTED, "%s: a 1x1, groups 1 layer with even C_in >= 8 and even C_out is required (got %lld -> %lld)", who,
                    (long long)d.c_in, (long long)d.c_out);
    if (d.x_layout != SLFP_LAYOUT_NHWC || d.y_layout != SLFP_LAYOUT_NHWC) return fail(SLFP_ERR_UNSUPPORTED, "%s: NHWC on both sides only", who);
    if (d.stride_h != 1 || d.stride_w != 1) return fail(SLFP_ERR_UNSUPPORTED, "%s: stride 1 only", who);
    if (plan.passes != 1) return fail(SLFP_ERR_UNSUPPORTED, "%s: single-pass mode only (no three-pass form)", who);
    s->entry = entry; s->pass = pass;
    s->fmt = plan.fmt_act == kFmtSfp7 ? kFmtSfp7 : kFmtAct8;
    s->ks = (int)ceil_div(d.c_in, 32);
    s->grid_cap = switches().pw_grid;
    const size_t w = (size_t)plan.k_pad * plan.n_pad * 2;
    s->lds = w + (size_t)3 * plan.n_pad * sizeof(float) + (pass ? (size_t)(kStreamThreads / 64) * kPwrStgWave * sizeof(float) : 0);
    const size_t tables = entry ? (size_t)kPwTab + kLayeroutLutBytes : (size_t)kDecBytes;   // static LDS
    if (s->ks > 8 || s->lds + tables > kPwrLdsBudget)
        return fail(SLFP_ERR_UNSUPPORTED, "%s: W (%zu KiB padded) with its tables and epilogue vectors does not fit the %zu KiB of LDS", who, w / 1024,
                    kPwrLdsBudget / 1024);
    return SLFP_OK;
}

typedef void (*PwrFn)(const PwrParams);

static PwrFn pwr_entry_instance(const PwrSel& s) {
    switch (s.ks) {
        case 1: return k_pwr_entry<1>;
        case 2: return k_pwr_entry<2>;
        case 3: return k_pwr_entry<3>;
        case 4: return k_pwr_entry<4>;
        case 5: return k_pwr_entry<5>;
        case 6: return k_pwr_entry<6>;
        case 7: return k_pwr_entry<7>;
        case 8: return k_pwr_entry<8>;
        default: return nullptr;
    }
}
template <int FMT, bool PASS>
static PwrFn pwr_exit_form(const PwrSel& s) {
    switch (s.ks) {
        case 1: return k_pwr_exit<FMT, 1, PASS>;
        case 2: return k_pwr_exit<FMT, 2, PASS>;
        case 3: return k_pwr_exit<FMT, 3, PASS>;
        case 4: return k_pwr_exit<FMT, 4, PASS>;
        case 5: return k_pwr_exit<FMT, 5, PASS>;
        case 6: return k_pwr_exit<FMT, 6, PASS>;
        case 7: return k_pwr_exit<FMT, 7, PASS>;
        case 8: return k_pwr_exit<FMT, 8, PASS>;
        default: return nullptr;
    }
}
static PwrFn pwr_exit_instance(const PwrSel& s) {
    if (s.fmt == kFmtSfp7) return s.pass ? pwr_exit_form<kFmtSfp7, true>(s) : pwr_exit_form<kFmtSfp7, false>(s);
    return s.pass ? pwr_exit_form<kFmtAct8, true>(s) : pwr_exit_form<kFmtAct8, false>(s);
}
static PwrFn pwr_instance(const PwrSel& s) { return s.entry ? pwr_entry_instance(s) : pwr_exit_instance(s); }

static const char* pwr_sel_name(const PwrSel& s) {
    static thread_local char buf[64];
    int n;
    if (s.entry) n = snprintf(buf, sizeof buf, "pwr-entry/ks%d/%s/lut", s.ks, pw_fmt_word(s.fmt));
    else n = snprintf(buf, sizeof buf, "pwr-exit/ks%d/%s/%s/%s", s.ks, s.ks % 2 == 0 ? "xw" : "dw", pw_fmt_word(s.fmt), s.pass ? "pass" : "f32");
    if (s.grid_cap > 0) snprintf(buf + n, sizeof buf - n, "/grid%d", s.grid_cap);
    return buf;
}

const char* pwr_instance_name(const slfp_conv2d_desc& d, const ConvPlan& plan, bool entry, bool pass) {
    PwrSel s;
    if (pwr_select(d, plan, entry, pass, &s) != SLFP_OK || !pwr_instance(s)) return "none";
    return pwr_sel_name(s);
}

// The pitches, offsets and the selection of a call, without pointers: what the support queries and the launchers share.  SLFP_OK, or
// the refusal with its text recorded.
int pwr_entry_check(const slfp_conv2d_desc& d, const ConvPlan& plan, int64_t x_ld, int64_t y_ld) {
    PwrSel s;
    const int rc = pwr_select(d, plan, true, false, &s);
    if (rc != SLFP_OK) return rc;
    if (x_ld < d.c_in || x_ld % 2 || x_ld > 0x7FFFFFFF)
        return fail(SLFP_ERR_UNSUPPORTED, "pointwise entry (table): x_ld = %lld floats must be even (8-byte aligned pixel rows), >= C_in = %lld and below 2^31",
                    (long long)x_ld, (long long)d.c_in);
    if (y_ld < d.c_out || y_ld % 32 || y_ld > 0x7FFFFFFF)
        return fail(SLFP_ERR_UNSUPPORTED, "pointwise entry (table): y_ld = %lld must be a multiple of 32, >= C_out = %lld and below 2^31", (long long)y_ld,
                    (long long)d.c_out);
    if (switches().pw_notab || !act_table(d.ka, plan.fmt_act, kEncF16P))
        return fail(SLFP_ERR_UNSUPPORTED, "pointwise entry (table): no threshold table for the layer's scale %g", (double)d.ka);
    return SLFP_OK;
}

int pwr_exit_check(const slfp_conv2d_desc& d, const ConvPlan& plan, bool has_pass, int64_t x_ld, int64_t pass_ld, int64_t y_ld, int64_t y_c0,
                   int64_t y_cs) {
    PwrSel s;
    const int rc = pwr_select(d, plan, false, has_pass, &s);
    if (rc != SLFP_OK) return rc;
    const char* who = "pointwise exit (layerout)";
    if (x_ld < d.c_in || x_ld % 32 || x_ld > 0x7FFFFFFF)
        return fail(SLFP_ERR_UNSUPPORTED, "%s: x_ld = %lld must be a multiple of 32, >= C_in = %lld and below 2^31", who, (long long)x_ld, (long long)d.c_in);
    if (y_cs != 1 && y_cs != 2) return fail(SLFP_ERR_UNSUPPORTED, "%s: y_cs must be 1 or 2 (got %lld)", who, (long long)y_cs);
    if (y_cs == 2 && !has_pass) return fail(SLFP_ERR_UNSUPPORTED, "%s: y_cs = 2 needs the `pass` operand that fills the channels in between", who);
    if (y_cs == 1 && has_pass) return fail(SLFP_ERR_UNSUPPORTED, "%s: a `pass` operand needs y_cs = 2", who);
    // y_cs 1: channels y_c0 .. y_c0 + C_out - 1; y_cs 2: pass i at y_c0 - 1 + 2i, result i at y_c0 + 2i.  8-byte stores either way.
    const int64_t first = y_cs == 2 ? y_c0 - 1 : y_c0, width = d.c_out * y_cs;
    if (y_ld % 2 || y_ld > 0x7FFFFFFF || first < 0 || first % 2 || first + width > y_ld)
        return fail(SLFP_ERR_UNSUPPORTED, "%s: channels %lld .. %lld of a y_ld = %lld row: y_ld and the first channel must be even (8-byte aligned "
                                          "float32 slices), the slice inside the row, y_ld below 2^31", who, (long long)first, (long long)(first + width - 1), (long long)y_ld);
    if (has_pass && (pass_ld < d.c_out || pass_ld > 0x7FFFFFFF))
        return fail(SLFP_ERR_UNSUPPORTED, "%s: pass_ld = %lld must be >= C_out = %lld and below 2^31", who, (long long)pass_ld, (long long)d.c_out);
    return SLFP_OK;
}

static void pwr_fill(PwrParams& p, const slfp_conv2d_desc& d, const ConvPlan& plan, const void* x, const void* wfrag, const float* bias,
                     const PostOp& post, void* y) {
    p.x = x; p.whi = reinterpret_cast<const _Float16*>(wfrag); p.bias = bias; p.y = y; p.pass = nullptr; p.lut = nullptr;
    p.M = d.n * d.h * d.w;
    p.K = (int)d.c_in; p.N = (int)d.c_out;
    p.KS = (int)(plan.k_pad / 32); p.n_tiles = (int)(plan.n_pad / 16);
    p.x_ld = p.y_ld = p.pass_ld = 0; p.y_c0 = 0; p.y_cs = 1;
    p.s1 = plan.s1; p.s2 = plan.s2; p.s1x = plan.s1 * (1.0f / 256.0f);
    p.post = post;
    p.enc.valid = 0;
}

static int pwr_launch(PwrParams& p, const PwrSel& s, hipStream_t stream) {
    const PwrFn fn = pwr_instance(s);
    if (!fn) return fail(SLFP_ERR_UNSUPPORTED, "pointwise (ragged): no kernel instance for %s", pwr_sel_name(s));
    if (p.M <= 0) return SLFP_OK;
    return pw_launch_stream(fn, p, s.lds, s.grid_cap, stream, s.entry ? "slfp pointwise entry (table) kernel" : "slfp pointwise exit (layerout) kernel");
}

int launch_pwr_entry(const slfp_conv2d_desc& d, const ConvPlan& plan, const float* x, int64_t x_ld, const void* wfrag, const float* bias,
                     const PostOp& post, const uint8_t* lut, uint8_t* y_codes, int64_t y_ld, hipStream_t stream) {
    int rc = pwr_entry_check(d, plan, x_ld, y_ld);
    if (rc != SLFP_OK) return rc;
    if (!post.scale || !post.shift || !lut) return fail(SLFP_ERR_BAD_ARG, "pointwise entry (table): post_scale, post_shift and lut are required");
    PwrSel s;
    rc = pwr_select(d, plan, true, false, &s);
    if (rc != SLFP_OK) return rc;
    PwrParams p;
    pwr_fill(p, d, plan, x, wfrag, bias, PostOp{post.scale, post.shift, 0, 0}, y_codes);
    p.lut = lut;
    p.x_ld = (int)x_ld; p.y_ld = (int)y_ld;
    p.enc = *act_table(d.ka, plan.fmt_act, kEncF16P);
    return pwr_launch(p, s, stream);
}

int launch_pwr_exit(const slfp_conv2d_desc& d, const ConvPlan& plan, const uint8_t* x_codes, int64_t x_ld, const void* wfrag, const float* bias,
                    const PostOp& post, const float* pass, int64_t pass_ld, float* y, int64_t y_ld, int64_t y_c0, int64_t y_cs, hipStream_t stream) {
    int rc = pwr_exit_check(d, plan, pass != nullptr, x_ld, pass_ld, y_ld, y_c0, y_cs);
    if (rc != SLFP_OK) return rc;
    PwrSel s;
    rc = pwr_select(d, plan, false, pass != nullptr, &s);
    if (rc != SLFP_OK) return rc;
    PwrParams p;
    pwr_fill(p, d, plan, x_codes, wfrag, bias, post, y);
    p.pass = pass;
    p.x_ld = (int)x_ld; p.y_ld = (int)y_ld; p.pass_ld = (int)pass_ld;
    p.y_c0 = (int)y_c0; p.y_cs = (int)y_cs;
    return pwr_launch(p, s, stream);
}

}  // namespace slfp
