// conv_pw_fp8.hip -- SFP<3,3> pointwise (1x1) convolution on 1-byte codes with OCP E4M3 operands, gfx950 matrix cores
// (SLFP_MFMA_FP8; slfp_conv2d_fwd_codes / slfp_conv2d_fwd_codes_slice).
//
// Every SFP<3,3> value +-(1 + m/8) * 2^E, E in [-3, 3], is exact in E4M3 once scaled by 16 (the pre-scale of the fp16 kernels:
// 15 * 16 = 240 <= 448), and its extended code sign<<6 | (E+4)<<3 | m is the E4M3 byte sign<<7 | (E+11)<<3 | m up to a constant.
// So the code bytes of a pixel ARE the B operand of v_mfma_f32_16x16x32_fp8_fp8 after a few whole-register integer instructions
// (sfp7x4_to_e4m3): no decode table, no LDS lookup, and -- a lane supplies 8 consecutive k values as 8 bytes -- no transpose.
//
//   * W: a blob of its own (k_pw8_prepare): E4M3 of 16 * QW(w / Kw), fragment (n-tile o/16, k-step k/32) = 512 B, lane-linear:
//     lane (o % 16) + 16 kq holds k = 32 s + 8 kq .. + 7.  C_out padded to 64, C_in to 64, with zero bytes.
//   * k_pw8<KS, PG, YC>: persistent workgroups of kStreamThreads threads, grid = slices x workgroups per slice.  A slice is a run
//     of whole 64-channel groups of C_out whose W (live k-steps only, 1 KiB per tile and k-step in two parts) and epilogue vectors fit kPw8LdsBudget, resident in LDS for
//     the workgroup's life; with several slices every slice reads all of X (1 B per element, L2 hits between the slices of one
//     pixel range: blocks b and b + 8 share an XCD, as k_pwc_slice places them).
//   * a wave's unit = PG groups of 16 pixels.  Per k-step a lane loads its 8 code bytes with ONE 8-byte load (all loads of the
//     unit first) and converts the two dwords in registers; four channel tiles are swept together (4 x PG independent
//     accumulator chains), each in k order from +0.
//   * the matrix unit does not add 8 products of widely different exponents exactly, so both operands are split by exponent
//     (e4m3x4_hi below: W once, on its way into LDS; X per k-step in registers) and a k-step is FOUR MFMAs per tile and pixel group,
//     each exact; two ds_read_b64 of W feed 4 x PG MFMAs.
//   * the epilogue is the project's: pw_fill_ep, pw_finish, pw_codes16_out / store_codes16 (conv_pw_core.hpp), the 2^-8 of the two
//     pre-scales folded into s1x as on the fp16 path.
// C_in = 16 / 48: the lane-quarters whose channels lie at or past C_in load nothing and supply zero bytes (the blob holds zero
// weights there): a row's last load never runs into the next pixel's codes or past the tensor.
#include "slfp_device.hpp"
#include "slfp_enc.hpp"
#include "slfp_codes.hpp"
#include "slfp_host.hpp"
#include "conv_pw_core.hpp"

namespace slfp {

constexpr size_t kPw8LdsBudget = 72 * 1024;   // dynamic LDS of a workgroup: two workgroups (16 waves) per CU next to the code table
constexpr int kPw8NominalSlots = 512;         // the PG rule counts waves on 256 CUs x 2 workgroups, so the choice needs no device

struct Pw8Params {
    const uint8_t* x;
    const uint8_t* w;     // the fp8 blob: n_tiles x KS fragments of 512 B
    const float* bias;
    void* y;
    int64_t M;            // output pixels
    int K, N, KS, n_tiles;   // KS: k-steps per tile IN THE BLOB (k_pad / 32); the kernel's template KS counts the live ones
    int H, W, Ho, Wo, S;     // pw_fill_geom; stride 1 only: not read
    float s1, s2, s1x;
    int nts, n_slices;    // channel tiles per slice (a multiple of 4; the last slice may hold fewer), slices
    int sgn, fmt_out;     // YC: as PwcParams
    PostOp post;
    EncArgs enc;          // YC: code table of the consumer's Ka (kEncCode)
    int y_ld;             // YC: bytes from one pixel's codes to the next
};

// Four SFP<3,3> extended codes -> four E4M3 bytes of 16 * value.  a = magnitude fields; (a + 0x38) re-biases the exponent
// (E + 4 -> E + 11), no carry leaves a byte (0x3F + 0x38 = 0x77); the sign moves from bit 6 to bit 7.  The tiny class (0x00 /
// 0x40) and exact zero (0x01) become 0: with the sign bit added to the magnitude these three, and only these, stay below 2, and
// bit 7 of (that + 0x7E) marks the others (0x3F + 1 + 0x7E = 0xBE); h - (h >> 7) widens the mark to 0x7F without a borrow between
// bytes.  Magnitudes 1..7 (0x41, 0x02..0x07, 0x42..0x47) are no codes of the encoder; they convert to the values the decode table
// gives them (2^-4 (1 + m/8), exact in E4M3 too), so every byte means what decode_ext_bits says, the tiny class as 0.
__device__ __forceinline__ uint32_t sfp7x4_to_e4m3(const uint32_t d) {
    const uint32_t a = d & 0x3F3F3F3Fu;
    const uint32_t h = (a + ((d >> 6) & 0x01010101u) + 0x7E7E7E7Eu) & 0x80808080u;
    const uint32_t keep = h - (h >> 7);
    return ((a + 0x38383838u) & keep) | ((d << 1) & h);
}

// The matrix unit adds the 8 products of a lane (one lane-quarter's k values) after aligning them to the largest exponent sum
// among them, and keeps 13 bits below it: measured on an MI355X, a product is exact there iff its exponent sum lies within 7 of
// the largest of its group of 8; across the four quarters and into the accumulator the sum is wide enough.
// The exponent fields of 16 * value span 7 .. 14, so one MFMA per k-step is NOT exact (2e-5 of the tensor's max).  Both operands
// are therefore split by exponent field into a low and a high part, the other bytes zero: W at 12 (fields 7..11 | 12..14), X at
// 11 (7..10 | 11..14).  In each of the four (W part, X part) MFMAs the exponent sums span at most 4 + 3 = 7: every product exact.
// hi = the bytes of d whose exponent field is at least (0x80 - ADD) >> 3; the sum cannot carry (0x78 + 0x28 = 0xA0).
template <uint32_t ADD>
__device__ __forceinline__ uint32_t e4m3x4_hi(const uint32_t d) {
    const uint32_t h = ((d & 0x78787878u) + ADD * 0x01010101u) & 0x80808080u;
    return d & ((h - (h >> 7)) | h);
}
constexpr uint32_t kPw8SplitW = 0x20, kPw8SplitX = 0x28;   // fields >= 12 / >= 11

template <int KS, int PG, bool YC>
__global__ __launch_bounds__(kStreamThreads) void k_pw8(const Pw8Params p) {
    __shared__ __attribute__((aligned(16))) unsigned char senc[YC ? kPwTab : 16];
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // blocks b and b + 8 share an XCD: the slices of one pixel range sit on consecutive (b / 8)
    const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;
    const int slice = q % p.n_slices;
    const int rank = xcd + 8 * (q / p.n_slices);
    const int n_ranks = 8 * ((int)(gridDim.x >> 3) / p.n_slices);
    const int t_lo = slice * p.nts;
    const int nts = p.n_tiles - t_lo < p.nts ? p.n_tiles - t_lo : p.nts;   // a multiple of 4: the blob is padded to 64 channels
    if (nts <= 0) return;
    if constexpr (YC) enc_fill<kStreamThreads>(reinterpret_cast<uint2*>(senc), p.enc);
    // W of the slice, the live k-steps of every tile, split by exponent on the way in: [tile][KS][low part | high part] of 512 B each,
    // 16 bytes of the blob per thread and trip
    for (int i = threadIdx.x; i < nts * KS * 32; i += kStreamThreads) {
        const int f = i >> 5, j = f / KS, s = f - j * KS;
        const u32x4 v = reinterpret_cast<const u32x4*>(p.w)[((size_t)(t_lo + j) * p.KS + s) * 32 + (i & 31)];
        const u32x4 hi = u32x4{e4m3x4_hi<kPw8SplitW>(v[0]), e4m3x4_hi<kPw8SplitW>(v[1]), e4m3x4_hi<kPw8SplitW>(v[2]), e4m3x4_hi<kPw8SplitW>(v[3])};
        reinterpret_cast<u32x4*>(smem)[f * 64 + (i & 31)] = v ^ hi;
        reinterpret_cast<u32x4*>(smem)[f * 64 + 32 + (i & 31)] = hi;
    }
    float* ep = reinterpret_cast<float*>(smem + (size_t)p.nts * KS * 1024);   // [256 * bias/s1/s2 | post scale | post shift] of the slice
    const int n_ch = p.nts * 16, n_lo = t_lo * 16;
    const bool has_vec = p.bias != nullptr || p.post.scale != nullptr;   // wave-uniform
    if (has_vec) pw_fill_ep<kStreamThreads>(ep, p, n_lo, n_ch);
    __syncthreads();
    const CodeQuant cq{p.enc.r1, p.enc.lo, p.enc.hi, p.sgn, p.fmt_out};

    const int lane = threadIdx.x & 63;
    const int col = lane & 15, kq = lane >> 4;
    const int64_t n_groups = (p.M + 15) >> 4;
    const int64_t n_units = (n_groups + PG - 1) / PG;
    const int64_t stride = (int64_t)n_ranks * (kStreamThreads / 64);
    const bool q_live = (KS - 1) * 32 + kq * 8 < p.K;   // the last k-step's quarter (C_in = 16 / 48: quarters 2 and 3 are dead)

    for (int64_t u = (int64_t)rank * (kStreamThreads / 64) + (threadIdx.x >> 6); u < n_units; u += stride) {
        int64_t m[PG];
        bool live[PG];
        uint2 xb[PG][KS];
#pragma unroll
        for (int g = 0; g < PG; ++g) {
            m[g] = (u * PG + g) * 16 + col;
            live[g] = m[g] < p.M;
            const uint8_t* xr = p.x + (size_t)(live[g] ? m[g] : p.M - 1) * p.K + kq * 8;   // rows past the end: clamped, computed, dropped
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                xb[g][s] = make_uint2(0u, 0u);
                if (s + 1 < KS || q_live) xb[g][s] = *reinterpret_cast<const uint2*>(xr + s * 32);
            }
        }
#pragma unroll
        for (int g = 0; g < PG; ++g) {
#pragma unroll
            for (int s = 0; s < KS; ++s) xb[g][s] = make_uint2(sfp7x4_to_e4m3(xb[g][s].x), sfp7x4_to_e4m3(xb[g][s].y));
        }

        for (int j0 = 0; j0 < nts; j0 += 4) {
            floatx4 acc[4][PG];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                for (int g = 0; g < PG; ++g) acc[jj][g] = floatx4{0.f, 0.f, 0.f, 0.f};
            const unsigned char* wj = smem + (size_t)j0 * KS * 1024 + lane * 8;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                long xl[PG], xh[PG];   // split here, not kept: two more registers per k-step and pixel group would not fit at KS = 32
#pragma unroll
                for (int g = 0; g < PG; ++g) {
                    const uint2 h = make_uint2(e4m3x4_hi<kPw8SplitX>(xb[g][s].x), e4m3x4_hi<kPw8SplitX>(xb[g][s].y));
                    xh[g] = __builtin_bit_cast(long, h);
                    xl[g] = __builtin_bit_cast(long, make_uint2(xb[g][s].x ^ h.x, xb[g][s].y ^ h.y));
                }
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const long wl = *reinterpret_cast<const long*>(wj + (jj * KS + s) * 1024);
                    const long wh = *reinterpret_cast<const long*>(wj + (jj * KS + s) * 1024 + 512);
#pragma unroll
                    for (int g = 0; g < PG; ++g) {   // small exponent sums first
                        acc[jj][g] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(wl, xl[g], acc[jj][g], 0, 0, 0);
                        acc[jj][g] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(wl, xh[g], acc[jj][g], 0, 0, 0);
                        acc[jj][g] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(wh, xl[g], acc[jj][g], 0, 0, 0);
                        acc[jj][g] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(wh, xh[g], acc[jj][g], 0, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int g = 0; g < PG; ++g) {
                if constexpr (YC) {   // the ReLU, where there is one, is the code quantizer's
                    uint8_t* yr = reinterpret_cast<uint8_t*>(p.y) + (size_t)m[g] * p.y_ld + n_lo;
                    pw_codes16_out<false, false>(j0, yr, live[g], n_lo, p.N, kq, cq, senc, [&](int j) {
                        return pw_finish<false, false>(acc[j - j0][g], p, ep, n_ch, j * 16 + kq * 4, has_vec);
                    });
                } else {
                    float* yr = reinterpret_cast<float*>(p.y) + (size_t)m[g] * p.N + n_lo + kq * 4;
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        const int n = (j0 + jj) * 16 + kq * 4;
                        const float4 r = pw_finish<true, false>(acc[jj][g], p, ep, n_ch, n, has_vec);
                        if (live[g] && n_lo + n < p.N) *reinterpret_cast<float4*>(yr + (j0 + jj) * 16) = r;
                    }
                }
            }
        }
    }
}

// One thread per blob byte: the whole blob is written (zero bytes in the padding), no memset in front.
// CODES: `w` holds 1-byte extended weight codes instead of float32 weights, as k_prepare's CODES form (conv_abi.hip).
template <bool CODES>
__global__ __launch_bounds__(256) void k_pw8_prepare(const float* __restrict__ w, uint8_t* __restrict__ blob, float* __restrict__ wq_oihw,
                                                     int64_t total, int O, int K, int KSB, const ScaleDiv sd) {
    __shared__ uint32_t sT[16];
    lut_fill<kFmtSfp7>(sT);
    __syncthreads();
    const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= total) return;
    const int b = (int)(at & 7), lane = (int)((at >> 3) & 63);
    const int64_t frag = at >> 9;
    const int s = (int)(frag % KSB), nt = (int)(frag / KSB);
    const int o = nt * 16 + (lane & 15), k = 32 * s + 8 * (lane >> 4) + b;
    uint8_t e = 0;
    if (o < O && k < K) {
        const size_t idx = (size_t)o * K + k;
        float qv;
        if constexpr (CODES) qv = __uint_as_float(decode_bits<kFmtSfp7>(reinterpret_cast<const uint8_t*>(w)[idx], true, sT));
        else qv = quantize_scaled<kFmtSfp7>(w[idx], sd, sT);
        if (wq_oihw) wq_oihw[idx] = qv;
        const uint32_t bits = __float_as_uint(qv);
        const uint32_t ex = (bits >> 23) & 0xFFu;   // 124 .. 130 for the values of the format (123: the decode of a magnitude below 8); the tiny class (1e-10) and 0 lie below
        if (ex >= 123u) e = (uint8_t)(((bits >> 24) & 0x80u) | ((ex - 116u) << 3) | ((bits >> 20) & 7u));   // E4M3 of 16 * value, exact
    }
    blob[at] = e;
}

// ---------------------------------------------------------------------------- host
static int pw8_ks(int64_t c_in) {   // live k-steps, 0: no instance
    if (c_in == 16 || c_in == 48) return (int)(c_in + 16) / 32;
    if (c_in % 32) return 0;
    const int ks = (int)(c_in / 32);
    return (ks == 1 || ks == 2 || ks == 3 || ks == 4 || ks == 8 || ks == 12 || ks == 16 || ks == 32) ? ks : 0;
}

bool pw8_applicable(const slfp_conv2d_desc& d) {
    return d.qbits == 7 && d.kh == 1 && d.kw == 1 && d.groups == 1 && d.stride_h == 1 && d.stride_w == 1 && d.pad_h == 0 && d.pad_w == 0 &&
           d.x_layout == SLFP_LAYOUT_NHWC && d.y_layout == SLFP_LAYOUT_NHWC && pw8_ks(d.c_in) != 0 && d.c_out % 4 == 0;
}

// Everything a launch decides, in ONE place: launch_pw8 dispatches on it and pw8_variant_name prints it.
struct Pw8Sel {
    int ks, pg, n_slices, nts;
    bool yc;
    int grid_cap;   // SLFP_PW_GRID: the most rank groups of 8 x n_slices workgroups (0: no cap)
};

static size_t pw8_lds(int ks, int nts) { return (size_t)nts * ks * 1024 + (size_t)3 * nts * 16 * sizeof(float); }   // W in two parts

static void pw8_select(const slfp_conv2d_desc& d, const ConvPlan& plan, bool y_codes, Pw8Sel* s) {
    s->ks = pw8_ks(d.c_in);
    s->yc = y_codes;
    s->grid_cap = switches().pw_grid;
    const int groups64 = (int)(plan.n_pad / 64);
    int fit = (int)(kPw8LdsBudget / pw8_lds(s->ks, 4));   // 64-channel groups whose W and vectors fit; 32 k-steps: one group, 128 KiB, one workgroup per CU
    fit = fit < 1 ? 1 : fit;
    const int slices = (int)ceil_div(groups64, fit);
    const int per = (int)ceil_div(groups64, slices);       // even slices ...
    s->n_slices = (int)ceil_div(groups64, per);            // ... none of them empty
    s->nts = per * 4;
    // PG = 2 where the layer has at most two k-steps and a slice has at least two 16-pixel groups per wave (on the nominal device),
    // else 1: measured (profiles/pw_fp8_bench.json), PG = 2 gains up to 7 % there and loses 2-38 % from four k-steps on.
    // SLFP_PW8_PG forces it
    const int64_t waves = (int64_t)8 * std::max(1, kPw8NominalSlots / (8 * s->n_slices)) * (kStreamThreads / 64);
    const int64_t n_groups = ((int64_t)d.n * plan.h_out * plan.w_out + 15) / 16;
    s->pg = (s->ks <= 2 && n_groups >= 2 * waves) ? 2 : 1;
    if (switches().pw8_pg == 1 || switches().pw8_pg == 2) s->pg = switches().pw8_pg;
    if (s->ks == 32) s->pg = 1;   // two pixel groups of 32 k-steps do not fit the registers (the instance spilled): not built
}

typedef void (*Pw8Fn)(const Pw8Params);
template <int KS>
static Pw8Fn pw8_form(const Pw8Sel& s) {
    if (s.pg == 2) return s.yc ? k_pw8<KS, 2, true> : k_pw8<KS, 2, false>;
    return s.yc ? k_pw8<KS, 1, true> : k_pw8<KS, 1, false>;
}
static Pw8Fn pw8_instance(const Pw8Sel& s) {
    switch (s.ks) {
        case 1: return pw8_form<1>(s);
        case 2: return pw8_form<2>(s);
        case 3: return pw8_form<3>(s);
        case 4: return pw8_form<4>(s);
        case 8: return pw8_form<8>(s);
        case 12: return pw8_form<12>(s);
        case 16: return pw8_form<16>(s);
        case 32: return s.yc ? k_pw8<32, 1, true> : k_pw8<32, 1, false>;
        default: return nullptr;
    }
}

const char* pw8_variant_name(const slfp_conv2d_desc& d, const ConvPlan& plan, bool y_codes) {
    static thread_local char buf[64];
    if (!plan.fp8 || (y_codes && d.c_out % 16 != 0)) return "none";
    Pw8Sel s;
    pw8_select(d, plan, y_codes, &s);
    if (!pw8_instance(s)) return "none";
    const int n = snprintf(buf, sizeof buf, "fp8/ks%d/pg%d/ns%d/%s", s.ks, s.pg, s.n_slices, s.yc ? "yc" : "f32");
    if (s.grid_cap > 0) snprintf(buf + n, sizeof buf - n, "/grid%d", s.grid_cap);
    return buf;
}

size_t pw8_wprep_bytes(const ConvPlan& plan) { return (size_t)plan.k_pad * plan.n_pad; }

int launch_pw8_prepare(const slfp_conv2d_desc& d, const ConvPlan& plan, const void* w, void* wprep, float* weight_q_oihw,
                       hipStream_t stream, bool codes) {
    const int64_t total = (int64_t)pw8_wprep_bytes(plan);
    const unsigned grid = (unsigned)ceil_div(total, 256);
    const ScaleDiv sd = make_scale_div(d.kw_scale);
    const float* wf = reinterpret_cast<const float*>(w);
    uint8_t* blob = reinterpret_cast<uint8_t*>(wprep);
    if (codes) hipLaunchKernelGGL(k_pw8_prepare<true>, dim3(grid), dim3(256), 0, stream, wf, blob, weight_q_oihw, total, (int)d.c_out, (int)d.c_in, (int)(plan.k_pad / 32), sd);
    else hipLaunchKernelGGL(k_pw8_prepare<false>, dim3(grid), dim3(256), 0, stream, wf, blob, weight_q_oihw, total, (int)d.c_out, (int)d.c_in, (int)(plan.k_pad / 32), sd);
    return check_launch("slfp weight prepare kernel (fp8)");
}

int launch_pw8(const slfp_conv2d_desc& d, const ConvPlan& plan, const uint8_t* x, const void* wprep, const float* bias,
               const PostOp& post, void* y, const CodeIo& io, hipStream_t stream) {
    if (!plan.fp8 || !io.x_codes || io.lut || (io.y_codes && d.c_out % 16 != 0))
        return fail(SLFP_ERR_UNSUPPORTED, "pointwise (fp8): SLFP_MFMA_FP8 needs code input and, for code output, C_out a multiple of 16");
    if (io.y_ld && (!io.y_codes || io.y_ld < d.c_out || io.y_ld % 16 || io.y_ld > 0x7FFFFFFF))
        return fail(SLFP_ERR_BAD_ARG, "pointwise (fp8): a channel-slice output needs code output and a pixel stride that is a multiple of 16, >= C_out");
    Pw8Params p;
    p.post = post;
    p.x = x; p.w = reinterpret_cast<const uint8_t*>(wprep); p.bias = bias; p.y = y;
    pw_fill_geom(p, d, plan);
    p.y_ld = io.y_ld ? (int)io.y_ld : p.N;
    p.sgn = post.relu ? 0 : 1;
    p.fmt_out = io.y_fmt;
    p.enc.valid = 0;
    if (io.y_codes) {
        const EncArgs* t = enc_table(io.y_ka, io.y_fmt, kEncCode);
        if (!t->valid) return fail(SLFP_ERR_UNSUPPORTED, "pointwise (fp8): no code table for the consumer's scale %g", (double)io.y_ka);
        p.enc = *t;
    }
    Pw8Sel s;
    pw8_select(d, plan, io.y_codes, &s);
    const Pw8Fn fn = pw8_instance(s);
    if (!fn) return fail(SLFP_ERR_UNSUPPORTED, "pointwise (fp8): no kernel instance for C_in = %d", p.K);
    p.nts = s.nts; p.n_slices = s.n_slices;
    const size_t lds = pw8_lds(s.ks, s.nts);
    int rc = raise_lds_limit(reinterpret_cast<const void*>(fn), lds);
    if (rc != SLFP_OK) return rc;
    int per_cu = resident_blocks_per_cu(reinterpret_cast<const void*>(fn), kStreamThreads, lds);
    per_cu = per_cu < 1 ? 1 : (per_cu > 2 ? 2 : per_cu);
    // grid = 8 (XCDs) x n_slices x rank groups: as many whole groups as fit the device, no more than there are units
    int64_t groups = (int64_t)device_cu_count() * per_cu / (8 * s.n_slices);
    const int64_t units = ceil_div(ceil_div(p.M, 16), s.pg);
    const int64_t need = ceil_div(units, (int64_t)8 * (kStreamThreads / 64));
    if (groups > need) groups = need;
    if (s.grid_cap > 0 && groups > s.grid_cap) groups = s.grid_cap;
    if (groups < 1) groups = 1;
    hipLaunchKernelGGL(fn, dim3((unsigned)(groups * 8 * s.n_slices)), dim3(kStreamThreads), lds, stream, p);
    return check_launch("slfp pointwise (codes, fp8) kernel");
}

}  // namespace slfp
