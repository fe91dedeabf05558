// conv_bwd.hip -- quantization-aware backward of Conv2d_Q / Linear_Q for the depthwise 3x3 and pointwise 1x1 families
// (include/slfp.h: slfp_conv2d_bwd) and, under SLFP_BWD_DENSE (slfp_conv2d_bwd_ex), every other groups-1 dilation-1 layer.
//
// The reference's forward is y = conv(QA(x/Ka), QW(w/Kw)) * Ka * Kw with straight-through estimators in both quantizers
// (utils/sfp_quant.py:50-53, 99-102), so its backward is
//     gx = conv_input(wq, gy) * Kw        wq = QW(w / Kw)
//     gw = conv_weight(xq, gy) * Ka       xq = QA(x / Ka)
//     gb = sum_{n,h,w} gy                 (conv2d_Q_bias; conv2d_Q's raw bias is added outside the Function)
// Everything accumulates in float32.  xq is never materialised: it is encoded on load with the forward's threshold table
// (slfp_enc.hpp; the long form of slfp_device.hpp where the table is unavailable), bit-identical to slfp_quantize_f32.
// wq is small: the caller quantizes it into the workspace first.
// slfp_conv2d_bwd_codes: x arrives as the 1-byte extended codes of xq (slfp_codes.hpp; NHWC, C_in % 4 == 0) and every x load
// becomes a byte load -- a dword of four channels where the float path loads a float4 -- decoded through the 256-entry kDecF32
// table in LDS: decode(code) is xq bit for bit, so gw equals the float path's.  The gx half never reads x.
//
// Determinism: no atomics.  Each workgroup writes its gw / gb partial sums to the workspace and k_reduce_parts sums them
// in a fixed order, so equal inputs give bitwise-equal gradients.
//
// Depthwise (k_dw3x3_bwd): one pass over x and gy produces gx and the gw / gb partials.  A thread owns one channel and a
// unit of kDwTH x kDwTW output positions of one image, and slides a three-column window of xq and gy along the unit's
// columns, so each x element is encoded ~1.9 times (stride 1) and every HBM byte is read once; the overlap of
// neighbouring units hits the caches.  Channels sit on the lanes, so any channel count works.
//
// Pointwise (k_gemm_f32): two float32 GEMMs on NHWC rows (M = N*H*W) on v_mfma_f32_32x32x2_f32 (exact f32 products, one
// rounding each): GX[M x Cin] = GY[M x Cout] * WQ[Cout x Cin], and GW[Cout x Cin] = GY^T * XQ split over M, with XQ encoded
// on load and the bias sum taken from the staged GY tiles of the first column of workgroups.
#include "slfp_device.hpp"
#include "slfp_enc.hpp"
#include "slfp_codes.hpp"
#include "slfp_host.hpp"
#include <cstdio>
#include <type_traits>

namespace slfp {

constexpr int kEncTabQ = -1;   // AF template argument: the threshold table (otherwise kFmtAct8 / kFmtSfp7: the long form)
constexpr int kNoEnc = -2;     // AF: the operand is used as is
constexpr int kCodes8 = -3;    // AF: the operand is the 1-byte extended codes of QA(x / Ka), SLFP<3,4> (decoded, not encoded)
constexpr int kCodes7 = -4;    // AF: the same, SFP<3,3>
constexpr bool af_codes(int af) { return af == kCodes8 || af == kCodes7; }
constexpr uint32_t kCodeZero4 = 0x01010101u;   // four codes of exact zero: what padding decodes from
// LDS of a kernel's activation table, in uint2: the threshold table, the 1 KiB decode table of the code forms, or nothing
constexpr int act_lds(int af) { return af == kEncTabQ ? kEncEntries + 1 : (af_codes(af) ? kDecBytes / 8 : 1); }

// A kernel's activation encoder: q(x) = QA(x / Ka), bit-identical to slfp_quantize_f32 (codec.hip: k_quantize_tab / k_codec).
// act_enc fills the workgroup's threshold table sE (AF == kEncTabQ) or the long form's LUT sT with NT threads; the
// caller's next __syncthreads() publishes them.  The code forms (af_codes) keep the decode table in sE instead: q of a byte and
// q4 of a dword of four are lookups (dec4_f32), and cx() is the operand's address as bytes -- element offsets stay what they are.
template <int AF>
struct ActEnc {
    static constexpr bool kCodes = af_codes(AF);
    using X4 = std::conditional_t<kCodes, uint32_t, float4>;   // four consecutive channels as loaded
    static __device__ __forceinline__ const uint8_t* cx(const float* x) { return reinterpret_cast<const uint8_t*>(x); }
    __device__ __forceinline__ float q(uint8_t code) const { return __uint_as_float(*reinterpret_cast<const uint32_t*>(tb + 4u * code)); }
    __device__ __forceinline__ float4 q4(uint32_t codes) const { return dec4_f32(codes, tb); }
    const unsigned char* tb;
    const uint32_t* sT;
    float r1, lo, hi;
    ScaleDiv sd;
    __device__ __forceinline__ float q(float x) const {
        if constexpr (AF == kNoEnc || kCodes) {   // (the code forms never call this)
            return x;
        } else if constexpr (AF == kEncTabQ) {
            const float r = enc_f32(x, r1, lo, hi, tb) + 0.0f;
            return x != x ? __uint_as_float(kBitsQNaN) : r;
        } else {
            return quantize_scaled<AF>(x, sd, sT);
        }
    }
    __device__ __forceinline__ float4 q4(float4 v) const { return make_float4(q(v.x), q(v.y), q(v.z), q(v.w)); }
};

template <int AF, int NT>
__device__ __forceinline__ ActEnc<AF> act_enc(uint2* sE, uint32_t* sT, const EncArgs& t, const ScaleDiv& sd) {
    if constexpr (AF == kEncTabQ) enc_fill<NT>(sE, t);
    else if constexpr (AF == kCodes8) dec_fill<kFmtAct8, kDecF32, NT>(reinterpret_cast<uint32_t*>(sE));
    else if constexpr (AF == kCodes7) dec_fill<kFmtSfp7, kDecF32, NT>(reinterpret_cast<uint32_t*>(sE));
    else if constexpr (AF != kNoEnc) lut_fill<AF>(sT);
    return ActEnc<AF>{reinterpret_cast<const unsigned char*>(sE), sT, t.r1, t.lo, t.hi, sd};
}

// ---- depthwise 3x3, pad 1 ----------------------------------------------------------------------------------------------
constexpr int kDwTH = 4;        // output rows per unit
constexpr int kDwTW = 8;        // output columns per unit
constexpr int kDwThreads = 256;
constexpr int kDwParts = 10;    // per channel: 9 taps + the bias sum

struct DwGeom {
    int N, H, W, C, Ho, Wo;
    int nbh, nbw;     // units per image: row bands x column segments
    int cw, rows;     // channels per workgroup (lanes) and unit slots per workgroup: cw * rows <= 256
    int64_t units;
};

template <int S, int AF>
__global__ __launch_bounds__(kDwThreads) void k_dw3x3_bwd(const float* __restrict__ x, const float* __restrict__ gy,
                                                           const float* __restrict__ wq, float* __restrict__ gx,
                                                           float* __restrict__ part, const DwGeom g, float kw_scale,
                                                           int need_gx, int need_gw, const EncArgs t, const ScaleDiv sd) {
    __shared__ __attribute__((aligned(16))) uint2 sE[kEncEntries + 1];
    __shared__ uint32_t sT[16];
    __shared__ float sRed[kDwThreads * kDwParts];
    const ActEnc<AF> enc = act_enc<AF, kDwThreads>(sE, sT, t, sd);
    __syncthreads();

    const int cl = threadIdx.x % g.cw, r = threadIdx.x / g.cw;
    const int c = blockIdx.y * g.cw + cl;
    const bool active = r < g.rows && c < g.C;
    const int C = g.C, H = g.H, W = g.W, Ho = g.Ho, Wo = g.Wo;
    float acc[kDwParts];
#pragma unroll
    for (int k = 0; k < kDwParts; ++k) acc[k] = 0.f;
    float w9[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) w9[k] = active ? wq[(int64_t)c * 9 + k] : 0.f;

    constexpr int XR = S * (kDwTH - 1) + 3;           // x rows of a unit (gw)
    constexpr int GR = S == 1 ? kDwTH + 2 : kDwTH + 1;  // gy rows of a unit (gx, and gw's interior rows)
    constexpr int GC = S == 1 ? 3 : 2;                 // gy columns in the window
    const int64_t nslots = (int64_t)gridDim.x * g.rows;
    for (int64_t u = (int64_t)blockIdx.x * g.rows + r; active && u < g.units; u += nslots) {
        const int n = (int)(u / ((int64_t)g.nbh * g.nbw));
        const int rem = (int)(u - (int64_t)n * g.nbh * g.nbw);
        const int oh0 = (rem / g.nbw) * kDwTH, ow0 = (rem % g.nbw) * kDwTW;
        const int64_t xo = (int64_t)n * H * W * C + c;   // in elements: float32, or bytes in the code forms
        const float* xn = x + xo;
        const float* gn = gy + (int64_t)n * Ho * Wo * C + c;
        const int xr0 = S * oh0 - 1;                    // first x row
        const int gr0 = S == 1 ? oh0 - 1 : oh0;         // first gy row
        auto ldx = [&](int row, int col) -> float {
            if (row < 0 || row >= H || col < 0 || col >= W) return 0.f;   // zero padding of xq
            if constexpr (af_codes(AF)) return enc.q(enc.cx(x)[xo + ((int64_t)row * W + col) * C]);   // one byte per channel
            else return enc.q(xn[((int64_t)row * W + col) * C]);
        };
        auto ldg = [&](int row, int col) -> float {
            if (row < 0 || row >= Ho || col < 0 || col >= Wo) return 0.f;
            return gn[((int64_t)row * Wo + col) * C];
        };
        float xw[3][XR], gw_[GC][GR];
        // prime the window so that the first slide yields x columns S*ow0-1 .. S*ow0+1 and gy columns ow0-1 .. ow0+1 (S == 1)
        // or ow0, ow0+1 (S == 2)
#pragma unroll
        for (int i = 0; i < XR; ++i) {
            if (S == 1) { xw[1][i] = need_gw ? ldx(xr0 + i, ow0 - 1) : 0.f; xw[2][i] = need_gw ? ldx(xr0 + i, ow0) : 0.f; }
            else xw[2][i] = need_gw ? ldx(xr0 + i, 2 * ow0 - 1) : 0.f;
        }
#pragma unroll
        for (int i = 0; i < GR; ++i) {
            if (S == 1) { gw_[1][i] = ldg(gr0 + i, ow0 - 1); gw_[2][i] = ldg(gr0 + i, ow0); }
            else gw_[1][i] = ldg(gr0 + i, ow0);
        }
        for (int k = 0; k < kDwTW; ++k) {
            const int ow = ow0 + k;
            if (ow >= Wo) break;
            // slide: S == 1 shifts one column, S == 2 two x columns / one gy column
#pragma unroll
            for (int i = 0; i < XR; ++i) {
                if (S == 1) {
                    xw[0][i] = xw[1][i]; xw[1][i] = xw[2][i];
                    xw[2][i] = need_gw ? ldx(xr0 + i, ow + 1) : 0.f;
                } else {
                    xw[0][i] = xw[2][i];
                    xw[1][i] = need_gw ? ldx(xr0 + i, 2 * ow) : 0.f;
                    xw[2][i] = need_gw ? ldx(xr0 + i, 2 * ow + 1) : 0.f;
                }
            }
#pragma unroll
            for (int i = 0; i < GR; ++i) {
                if (S == 1) { gw_[0][i] = gw_[1][i]; gw_[1][i] = gw_[2][i]; gw_[2][i] = ldg(gr0 + i, ow + 1); }
                else { gw_[0][i] = gw_[1][i]; gw_[1][i] = ldg(gr0 + i, ow + 1); }
            }
            // gw / gb: output positions (oh0 + tr, ow); only valid ones contribute (a NaN in xq must not meet a padded gy)
            if (need_gw) {
#pragma unroll
                for (int tr = 0; tr < kDwTH; ++tr) {
                    if (oh0 + tr >= Ho) break;
                    const float gv = S == 1 ? gw_[1][tr + 1] : gw_[0][tr];
#pragma unroll
                    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                        for (int kw = 0; kw < 3; ++kw) acc[kh * 3 + kw] = __builtin_fmaf(gv, xw[kw][S * tr + kh], acc[kh * 3 + kw]);
                    acc[9] += gv;
                }
            }
            // gx: input positions; gy positions outside the output are zero, the 9 taps are summed in a fixed order
            if (need_gx) {
                float* gxn = gx + (int64_t)n * H * W * C + c;
                if (S == 1) {
                    // gx[ih][ow] = sum_{kh,kw} gy[ih + 1 - kh][ow + 1 - kw] * w[kh][kw]
#pragma unroll
                    for (int tr = 0; tr < kDwTH; ++tr) {
                        const int ih = oh0 + tr;
                        if (ih >= H) break;
                        float s = 0.f;
#pragma unroll
                        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                            for (int kw = 0; kw < 3; ++kw) s = __builtin_fmaf(gw_[2 - kw][tr + 2 - kh], w9[kh * 3 + kw], s);
                        gxn[((int64_t)ih * W + ow) * C] = s * kw_scale;
                    }
                } else {
                    // ih = 2m: kh = 1 -> gy row m;  ih = 2m + 1: kh = 0 -> row m + 1, kh = 2 -> row m (columns alike)
#pragma unroll
                    for (int tr = 0; tr < kDwTH; ++tr) {
#pragma unroll
                        for (int py = 0; py < 2; ++py) {
                            const int ih = 2 * (oh0 + tr) + py;
                            if (ih >= H) continue;
#pragma unroll
                            for (int px = 0; px < 2; ++px) {
                                const int iw = 2 * ow + px;
                                if (iw >= W) continue;
                                float s = 0.f;
#pragma unroll
                                for (int kh = 0; kh < 3; ++kh) {
                                    if ((kh & 1) == py) continue;          // py = 0 takes kh = 1; py = 1 takes kh = 0, 2
                                    const int gr = tr + (kh == 0 ? 1 : 0);
#pragma unroll
                                    for (int kw = 0; kw < 3; ++kw) {
                                        if ((kw & 1) == px) continue;
                                        const int gc = kw == 0 ? 1 : 0;
                                        s = __builtin_fmaf(gw_[gc][gr], w9[kh * 3 + kw], s);
                                    }
                                }
                                gxn[((int64_t)ih * W + iw) * C] = s * kw_scale;
                            }
                        }
                    }
                }
            }
        }
        // S == 1: the units of the last column segment also cover ow0 + kDwTW > Wo; S == 2: the odd last input column
        // (W even) is written by the step of ow = W/2 - 1 (px = 1), and rows alike, so no input position is left out.
    }
    if (!need_gw) return;
    // fixed-order reduction of the workgroup's unit slots, then one partial per (block, part, channel)
#pragma unroll
    for (int k = 0; k < kDwParts; ++k) sRed[k * kDwThreads + threadIdx.x] = acc[k];
    __syncthreads();
    if (r == 0 && c < C) {
        for (int k = 0; k < kDwParts; ++k) {
            float s = 0.f;
            for (int q = 0; q < g.rows; ++q) s += sRed[k * kDwThreads + q * g.cw + cl];
            part[((int64_t)blockIdx.x * kDwParts + k) * C + c] = s;
        }
    }
}

// sum[col] = sum_p part[p][col] over p = 0 .. P-1, in a fixed order: thread row tr adds p = tr, tr + 16, ... in increasing p,
// row 0 then adds the 16 row sums in order.  Where it goes:
//   dwC > 0: the depthwise layout col = k*C + c, k < 9 -> gw[c*9 + k] = sum * scale, k == 9 -> gb[c] = sum;
//   T > 0:   the dense layout col = (co*T + tap)*Cin + ci -> gw[(co*Cin + ci)*T + tap] = sum * scale (OIHW);
//   else:    gw[col] = sum * scale.
constexpr int kRedCols = 16, kRedRows = 16;
__global__ __launch_bounds__(kRedCols * kRedRows) void k_reduce_parts(const float* __restrict__ part, int P, int64_t ncols,
                                                                       float scale, int dwC, int Cin, int T,
                                                                       float* __restrict__ gw, float* __restrict__ gb) {
    __shared__ float s[kRedRows][kRedCols];
    const int tc = threadIdx.x % kRedCols, tr = threadIdx.x / kRedCols;
    const int64_t col = (int64_t)blockIdx.x * kRedCols + tc;
    float a = 0.f;
    if (col < ncols) {
        int p = tr;
        for (; p + 3 * kRedRows < P; p += 4 * kRedRows) {
            const float v0 = part[(int64_t)p * ncols + col], v1 = part[(int64_t)(p + kRedRows) * ncols + col];
            const float v2 = part[(int64_t)(p + 2 * kRedRows) * ncols + col], v3 = part[(int64_t)(p + 3 * kRedRows) * ncols + col];
            a += v0; a += v1; a += v2; a += v3;
        }
        for (; p < P; p += kRedRows) a += part[(int64_t)p * ncols + col];
    }
    s[tr][tc] = a;
    __syncthreads();
    if (tr != 0 || col >= ncols) return;
    float sum = 0.f;
    for (int q = 0; q < kRedRows; ++q) sum += s[q][tc];
    if (dwC > 0) {
        const int k = (int)(col / dwC), c = (int)(col - (int64_t)k * dwC);
        if (k < 9) { if (gw) gw[(int64_t)c * 9 + k] = sum * scale; }
        else if (gb) gb[c] = sum;
    } else if (T > 0) {
        const int ci = (int)(col % Cin);
        const int64_t r = col / Cin;
        gw[(r / T * Cin + ci) * T + r % T] = sum * scale;
    } else {
        gw[col] = sum * scale;
    }
}

// ---- the float32 MFMA tile core of k_gemm_f32, k_dense_gx and k_dense_gw ------------------------------------------------
// 4 waves in a 2 x 2 grid (wm, wn), each owning TM x TN accumulators of 32 x 32 (v_mfma_f32_32x32x2_f32); the workgroup's
// 64 TM x 64 TN tile advances BK = 16 per k-step through two k-major LDS tiles sA[BK][BM or more], sB[BK][BN].  The LDS
// arrays are passed by reference to array, so their row pitch (k_dense_gx pads sA) is a compile-time constant.
constexpr int kGemmBK = 16;
typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int TM, int TN>
__device__ __forceinline__ void acc_zero(f32x16 (&acc)[TM][TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
}

// acc += sA^T * sB over the BK staged k rows
template <int TM, int TN, int PA, int PB>
__device__ __forceinline__ void mfma_chunk(f32x16 (&acc)[TM][TN], const float (&sA)[kGemmBK][PA], const float (&sB)[kGemmBK][PB],
                                           int wm, int wn, int lane) {
#pragma unroll
    for (int kk = 0; kk < kGemmBK; kk += 2) {
        float a[TM], b[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) a[i] = sA[kk + (lane >> 5)][(wm * TM + i) * 32 + (lane & 31)];
#pragma unroll
        for (int j = 0; j < TN; ++j) b[j] = sB[kk + (lane >> 5)][(wn * TN + j) * 32 + (lane & 31)];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
}

// The epilogue.  C/D map of the 32x32 f32 MFMA: col = lane & 31, row = (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5).
// row(r) gives the address of tile row r at the tile's first column, or null for a row outside the matrix; ncols: the
// matrix columns from the tile's first one on.
template <int TM, int TN, class Row>
__device__ __forceinline__ void store_acc(const f32x16 (&acc)[TM][TN], int wm, int wn, int lane, int ncols, float scale, Row row) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            float* dst = row((wm * TM + i) * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5));
            if (!dst) continue;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int col = (wn * TN + j) * 32 + (lane & 31);
                if (col < ncols) dst[col] = acc[i][j][q] * scale;
            }
        }
}

// The software-pipelined K loop: load(s) fetches k-step s into registers, store() stages them in LDS, and the loads of
// step next(s) are in flight while staged() (the bias sums) and the MFMAs run on step s.  live(s): s is a step.
template <int TM, int TN, int PA, int PB, class Step, class Live, class Next, class Load, class Store, class Staged>
__device__ __forceinline__ void tile_loop(f32x16 (&acc)[TM][TN], const float (&sA)[kGemmBK][PA], const float (&sB)[kGemmBK][PB],
                                          int wm, int wn, int lane, Step s, Live live, Next next, Load load, Store store,
                                          Staged staged) {
    acc_zero(acc);
    if (live(s)) load(s);
    while (live(s)) {
        store();
        __syncthreads();
        const Step s1 = next(s);
        if (live(s1)) load(s1);
        staged();
        mfma_chunk(acc, sA, sB, wm, wn, lane);
        __syncthreads();
        s = s1;
    }
}

// Float4 group e of a tile into LDS: k-major as it is (row e / (P/4)), or transposed from m-major (row e / (BK/4) of the
// matrix holds four consecutive k)
template <int P>
__device__ __forceinline__ void st4_kmaj(float (&s)[kGemmBK][P], int e, float4 v) {
    *reinterpret_cast<float4*>(&s[e / (P / 4)][(e % (P / 4)) * 4]) = v;
}
template <int P>
__device__ __forceinline__ void st4_mmaj(float (&s)[kGemmBK][P], int e, float4 v) {
    const int mm = e / (kGemmBK / 4), kk = (e % (kGemmBK / 4)) * 4;
    s[kk][mm] = v.x; s[kk + 1][mm] = v.y; s[kk + 2][mm] = v.z; s[kk + 3][mm] = v.w;
}

// Guarded loads of the gathered tiles: the address is clamped to p where the element is out of range, the load is
// unconditional and the value selected, so no branch surrounds a global load.  ld4_guard: p[off .. off+3], of which
// the first n exist (n <= 0: none; VEC: n is 0 or at least 4 and off is a multiple of 4).
__device__ __forceinline__ float ld_guard(const float* __restrict__ p, int64_t off, bool ok) {
    const float v = p[ok ? off : 0];
    return ok ? v : 0.f;
}
template <bool VEC>
__device__ __forceinline__ float4 ld4_guard(const float* __restrict__ p, int64_t off, bool ok, int n) {
    if constexpr (VEC) {
        const bool ok4 = ok && n > 0;
        const float4 v = *reinterpret_cast<const float4*>(p + (ok4 ? off : 0));
        return ok4 ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        return make_float4(ld_guard(p, off, ok && n > 0), ld_guard(p, off + 1, ok && n > 1), ld_guard(p, off + 2, ok && n > 2),
                           ld_guard(p, off + 3, ok && n > 3));
    }
}

// The bias gradient from the staged GY^T tiles: thread tid < BM sums column tid of sA (on: it does)
template <int P>
__device__ __forceinline__ void gb_add(float& gbs, const float (&sA)[kGemmBK][P], bool on) {
    if (!on) return;
#pragma unroll
    for (int kk = 0; kk < kGemmBK; ++kk) gbs += sA[kk][threadIdx.x];
}
__device__ __forceinline__ void gb_store(float* __restrict__ gbpart, int M, int m0, float gbs, bool on) {
    if (on && m0 + (int)threadIdx.x < M) gbpart[(int64_t)blockIdx.z * M + m0 + threadIdx.x] = gbs;
}

// ---- C[M x N] = scale * A[M x K] * B[K x N] ------------------------------------------------------------------------------
// A_KMAJ: A is stored [K][M] (m contiguous, lda = row pitch), else [M][K] (k contiguous).  B is stored [K][N] and goes
// through the encoder AF on the way into LDS.  blockIdx.z: a split of K (kps rows each); C then points at the split's
// partial [z][M][N].  gbpart != null (A_KMAJ only): the first column of workgroups also writes the sums of A over its K range
// per m, gbpart[z][m] (the bias gradient: A = GY^T).
struct GemmArgs {
    const float* A;
    const float* B;
    float* C;
    float* gbpart;
    int M, N, K;
    int64_t lda, ldb, ldc;
    int kps;      // K rows per split
    float scale;
};

template <int TM, int TN, bool A_KMAJ, int AF, bool VEC>
__global__ __launch_bounds__(256) void k_gemm_f32(const GemmArgs ga, const EncArgs t, const ScaleDiv sd) {
    constexpr int BM = 64 * TM, BN = 64 * TN, BK = kGemmBK;
    __shared__ __attribute__((aligned(16))) float sA[BK][BM];
    __shared__ __attribute__((aligned(16))) float sB[BK][BN];
    __shared__ __attribute__((aligned(16))) uint2 sE[act_lds(AF)];
    __shared__ uint32_t sT[16];
    const ActEnc<AF> enc = act_enc<AF, 256>(sE, sT, t, sd);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int kb = blockIdx.z * ga.kps;
    const int ke = min(ga.K, kb + ga.kps);
    const int M = ga.M, N = ga.N;
    const bool gb_on = ga.gbpart != nullptr && blockIdx.y == 0 && tid < BM;

    // global -> register staging: BK x BM of A and BK x BN of B as float4 groups (4 consecutive elements along the
    // contiguous dimension), zero outside the matrix
    constexpr int AV = BM * BK / 4 / 256, BV = BN * BK / 4 / 256;   // float4 groups per thread
    static_assert(AV >= 1 && BV >= 1, "tile too small for 256 threads");
    float4 ra[AV];
    typename ActEnc<AF>::X4 rb[BV];
    auto ld4 = [&](const float* base, int64_t ld, int row, int col, int rows_end, int cols_end) -> float4 {
        // element (row, col .. col+3) of a row-major [rows][cols] matrix
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row >= rows_end) return v;
        const float* p = base + (int64_t)row * ld + col;
        if (VEC && col + 3 < cols_end) return *reinterpret_cast<const float4*>(p);
        if (col < cols_end) v.x = p[0];
        if (col + 1 < cols_end) v.y = p[1];
        if (col + 2 < cols_end) v.z = p[2];
        if (col + 3 < cols_end) v.w = p[3];
        return v;
    };
    auto load_tiles = [&](int k0) {
#pragma unroll
        for (int i = 0; i < AV; ++i) {
            const int e = tid + i * 256;
            if constexpr (A_KMAJ) {   // [k][m]: BK rows of BM/4 groups
                const int kk = e / (BM / 4), mm = (e % (BM / 4)) * 4;
                ra[i] = ld4(ga.A, ga.lda, k0 + kk, m0 + mm, ke, M);
            } else {                  // [m][k]: BM rows of BK/4 groups
                const int mm = e / (BK / 4), kk = (e % (BK / 4)) * 4;
                ra[i] = ld4(ga.A, ga.lda, m0 + mm, k0 + kk, M, ke);
            }
        }
#pragma unroll
        for (int i = 0; i < BV; ++i) {
            const int e = tid + i * 256;
            const int kk = e / (BN / 4), nn = (e % (BN / 4)) * 4;
            if constexpr (af_codes(AF)) {   // N % 4 == 0: the four channels are all there or none is
                const bool ok = k0 + kk < ke && n0 + nn < N;
                const uint32_t v = *reinterpret_cast<const uint32_t*>(enc.cx(ga.B) + (ok ? (int64_t)(k0 + kk) * ga.ldb + n0 + nn : 0));
                rb[i] = ok ? v : kCodeZero4;
            } else {
                rb[i] = ld4(ga.B, ga.ldb, k0 + kk, n0 + nn, ke, N);
            }
        }
    };
    auto store_tiles = [&]() {
#pragma unroll
        for (int i = 0; i < AV; ++i) {
            if constexpr (A_KMAJ) st4_kmaj(sA, tid + i * 256, ra[i]);
            else st4_mmaj(sA, tid + i * 256, ra[i]);
        }
#pragma unroll
        for (int i = 0; i < BV; ++i) st4_kmaj(sB, tid + i * 256, enc.q4(rb[i]));   // padding zeros stay zero (Q(0) == 0)
    };

    f32x16 acc[TM][TN];
    float gbs = 0.f;
    __syncthreads();   // the encode table is in LDS
    tile_loop(acc, sA, sB, wm, wn, lane, kb, [&](int k0) { return k0 < ke; }, [](int k0) { return k0 + BK; }, load_tiles,
              store_tiles, [&]() { gb_add(gbs, sA, gb_on); });
    float* cz = ga.C + (int64_t)blockIdx.z * M * N + n0;
    store_acc(acc, wm, wn, lane, N - n0, ga.scale,
              [&](int r) -> float* { return m0 + r < M ? cz + (int64_t)(m0 + r) * ga.ldc : nullptr; });
    gb_store(ga.gbpart, M, m0, gbs, gb_on);
}

// ---- dense k x k / strided / stem layers (groups 1, dilation 1): implicit GEMM on the same tile core --------------------
// k_dense_gx: GX[(n,h,w)][ci] = Kw * sum_{tap,co} GY[n, (h+pad_h-kh)/stride_h, (w+pad_w-kw)/stride_w, co] * WT[tap][co][ci].
// The rows of a workgroup lie in one (h mod stride_h, w mod stride_w) phase, so a tap either reaches every row of the tile
// or none; the taps that reach none are skipped.  GEMM K runs over (tap, co) with each tap's co run padded to whole BK
// (zeros), so a k-chunk never straddles two taps.  The A tile is gathered from NHWC gy.  A phase no tap reaches (1x1
// stride 2: three of four) gets exact zeros.
// k_dense_gw: GWp[z][co][(tap,ci)] = sum_{m=(n,ho,wo) in split z} GY[m][co] * QA(X[n, ho*stride_h-pad_h+kh, wo*stride_w-pad_w+kw, ci]/Ka),
// xq encoded on load as in k_gemm_f32 (never materialised), which it differs from in the B-tile gather only;
// k_reduce_parts adds the splits in a fixed order, applies Ka and writes OIHW.
struct DenseGeom {
    int N, H, W, Cin, Ho, Wo, Cout, KH, KW, sh, sw, padh, padw;
};

// rows (input pixels) of phase (a, b): n x ceil((H - a) / sh) x ceil((W - b) / sw)
__host__ __device__ __forceinline__ int dense_phase_extent(int extent, int phase, int stride) {
    return (extent - phase + stride - 1) / stride;
}

struct TapStep { int t, c0; };   // a k-step of k_dense_gx: BK output channels from c0 of tap t

template <int TN, bool VEC>
__global__ __launch_bounds__(256) void k_dense_gx(const float* __restrict__ gy, const float* __restrict__ wt,
                                                   float* __restrict__ gx, const DenseGeom g, const float scale) {
    constexpr int TM = 2, BM = 64 * TM, BN = 64 * TN, BK = kGemmBK;
    constexpr int BMP = BM + 2;   // the scalar stores of a lane group land on distinct banks
    __shared__ float sA[BK][BMP];
    __shared__ __attribute__((aligned(16))) float sB[BK][BN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int Cin = g.Cin, Cout = g.Cout, Ho = g.Ho, Wo = g.Wo, T = g.KH * g.KW;

    // the workgroup's phase and its row tile inside the phase (workgroup-uniform)
    int bx = blockIdx.x, ph = 0, pw = 0, Hp = 0, Wp = 0, rows = 0;   // N*H*W < 2^31 (dense_ok)
    for (int a = 0, found = 0; a < g.sh && !found; ++a)
        for (int b = 0; b < g.sw; ++b) {
            const int hp = dense_phase_extent(g.H, a, g.sh), wp = dense_phase_extent(g.W, b, g.sw);
            const int r = g.N * hp * wp;
            const int cnt = r / BM + (r % BM != 0);
            if (bx < cnt) { ph = a; pw = b; Hp = hp; Wp = wp; rows = r; found = 1; break; }
            bx -= cnt;
        }
    const int r0 = bx * BM;
    const int n0 = blockIdx.y * BN;
    const int HWp = Hp * Wp;

    constexpr int AV = BM * BK / 4 / 256, BV = BN * BK / 4 / 256;
    float4 ra[AV], rb[BV];
    // the A rows of this thread: fixed for the whole K loop
    int a_nb[AV], a_h[AV], a_w[AV];
    bool a_ok[AV];
#pragma unroll
    for (int i = 0; i < AV; ++i) {
        const int r = r0 + (tid + i * 256) / (BK / 4);
        a_ok[i] = r < rows;
        const int rc = a_ok[i] ? r : 0;
        const int n = rc / HWp, rem = rc - n * HWp;
        a_nb[i] = n * Ho; a_h[i] = rem / Wp; a_w[i] = rem - a_h[i] * Wp;
    }
    // first tap at or after t that reaches this phase; T if none
    auto next_tap = [&](int t) -> int {
        for (; t < T; ++t) {
            const int th = ph + g.padh - t / g.KW, tw = pw + g.padw - t % g.KW;
            if (th % g.sh == 0 && tw % g.sw == 0) break;
        }
        return t;
    };
    auto next_step = [&](TapStep s) -> TapStep {
        if (s.c0 + BK < Cout) return TapStep{s.t, s.c0 + BK};
        return TapStep{next_tap(s.t + 1), 0};
    };
    auto load_tiles = [&](TapStep s) {
        const int t = s.t, c0 = s.c0;
        const int dh = (ph + g.padh - t / g.KW) / g.sh, dw = (pw + g.padw - t % g.KW) / g.sw;   // exact
#pragma unroll
        for (int i = 0; i < AV; ++i) {
            const int co = c0 + ((tid + i * 256) % (BK / 4)) * 4;
            const int ho = a_h[i] + dh, wo = a_w[i] + dw;
            const bool ok = a_ok[i] && (unsigned)ho < (unsigned)Ho && (unsigned)wo < (unsigned)Wo;
            const int64_t base = ok ? ((int64_t)(a_nb[i] + ho) * Wo + wo) * Cout : 0;
            ra[i] = ld4_guard<VEC>(gy, base + co, ok, Cout - co);
        }
#pragma unroll
        for (int i = 0; i < BV; ++i) {
            const int e = tid + i * 256;
            const int co = c0 + e / (BN / 4), ci = n0 + (e % (BN / 4)) * 4;
            rb[i] = ld4_guard<VEC>(wt, ((int64_t)t * Cout + co) * Cin + ci, co < Cout, Cin - ci);
        }
    };
    auto store_tiles = [&]() {
#pragma unroll
        for (int i = 0; i < AV; ++i) st4_mmaj(sA, tid + i * 256, ra[i]);
#pragma unroll
        for (int i = 0; i < BV; ++i) st4_kmaj(sB, tid + i * 256, rb[i]);
    };

    f32x16 acc[TM][TN];
    tile_loop(acc, sA, sB, wm, wn, lane, TapStep{next_tap(0), 0}, [&](TapStep s) { return s.t < T; }, next_step, load_tiles,
              store_tiles, []() {});
    store_acc(acc, wm, wn, lane, Cin - n0, scale, [&](int tr) -> float* {
        const int r = r0 + tr;
        if (r >= rows) return nullptr;
        const int n = r / HWp, rem = r - n * HWp;
        const int hh = rem / Wp, ww = rem - hh * Wp;
        return gx + (((int64_t)n * g.H + ph + hh * g.sh) * g.W + pw + ww * g.sw) * Cin + n0;
    });
}

template <int TM, int TN, int AF, bool VEC>
__global__ __launch_bounds__(256) void k_dense_gw(const float* __restrict__ gy, const float* __restrict__ x,
                                                   float* __restrict__ part, float* __restrict__ gbpart, const DenseGeom g,
                                                   const int64_t K, const int kps, const EncArgs t, const ScaleDiv sd) {
    constexpr int BM = 64 * TM, BN = 64 * TN, BK = kGemmBK;
    __shared__ __attribute__((aligned(16))) float sA[BK][BM];
    __shared__ __attribute__((aligned(16))) float sB[BK][BN];
    __shared__ __attribute__((aligned(16))) uint2 sE[act_lds(AF)];
    __shared__ uint32_t sT[16];
    const ActEnc<AF> enc = act_enc<AF, 256>(sE, sT, t, sd);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int Cin = g.Cin, Cout = g.Cout, Ho = g.Ho, Wo = g.Wo, H = g.H, W = g.W;
    const int M = Cout, N = g.KH * g.KW * Cin;   // GEMM rows and columns
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int64_t kb = (int64_t)blockIdx.z * kps;
    const int64_t ke = kb + kps < K ? kb + kps : K;
    const int HWo = Ho * Wo;
    const bool gb_on = gbpart != nullptr && blockIdx.y == 0 && tid < BM;

    constexpr int AV = BM * BK / 4 / 256, BV = BN * BK / 4 / 256;
    static_assert(256 % (BN / 4) == 0, "a thread keeps its B columns over the K loop");
    float4 ra[AV];
    typename ActEnc<AF>::X4 rb[BV];
    // the B columns (tap, ci) of this thread: fixed for the whole K loop.  VEC: C_in % 4 == 0, so the four lie in one tap.
    constexpr int NC = VEC ? 1 : 4;
    int b_kh[NC], b_kw[NC], b_ci[NC];
    bool b_ok[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int c = n0 + (tid % (BN / 4)) * 4 + j;
        b_ok[j] = c < N;
        const int cc = b_ok[j] ? c : 0;
        const int tap = cc / Cin;
        b_ci[j] = cc - tap * Cin; b_kh[j] = tap / g.KW - g.padh; b_kw[j] = tap % g.KW - g.padw;
    }
    auto load_tiles = [&](int64_t k0) {
#pragma unroll
        for (int i = 0; i < AV; ++i) {   // GY^T: [k = m][co], co contiguous
            const int e = tid + i * 256;
            const int64_t k = k0 + e / (BM / 4);
            const int co = m0 + (e % (BM / 4)) * 4;
            const bool okk = k < ke;
            ra[i] = ld4_guard<VEC>(gy, (okk ? k * Cout : 0) + co, okk, M - co);
        }
#pragma unroll
        for (int i = 0; i < BV; ++i) {   // X gathered at the shifted pixel; padding and rows past the split are zero
            const int64_t k = k0 + (tid + i * 256) / (BN / 4);
            const bool okk = k < ke;
            const int64_t kc = okk ? k : 0;
            const int n = (int)(kc / HWo), rem = (int)(kc - (int64_t)n * HWo);
            const int ho = rem / Wo, wo = rem - ho * Wo;
            int64_t off[NC];
            bool ok[NC];
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const int hi_ = ho * g.sh + b_kh[j], wi = wo * g.sw + b_kw[j];
                ok[j] = okk && b_ok[j] && (unsigned)hi_ < (unsigned)H && (unsigned)wi < (unsigned)W;
                off[j] = (((int64_t)n * H + hi_) * W + wi) * Cin + b_ci[j];
            }
            if constexpr (af_codes(AF)) {   // C_in % 4 == 0: the four columns lie in one tap, whatever VEC says of gy
                const uint32_t v = *reinterpret_cast<const uint32_t*>(enc.cx(x) + (ok[0] ? off[0] : 0));
                rb[i] = ok[0] ? v : kCodeZero4;
            } else if constexpr (VEC) rb[i] = ld4_guard<true>(x, off[0], ok[0], 4);
            else rb[i] = make_float4(ld_guard(x, off[0], ok[0]), ld_guard(x, off[1], ok[1]), ld_guard(x, off[2], ok[2]),
                                     ld_guard(x, off[3], ok[3]));
        }
    };
    auto store_tiles = [&]() {
#pragma unroll
        for (int i = 0; i < AV; ++i) st4_kmaj(sA, tid + i * 256, ra[i]);
#pragma unroll
        for (int i = 0; i < BV; ++i) st4_kmaj(sB, tid + i * 256, enc.q4(rb[i]));   // padding zeros stay zero (Q(0) == 0)
    };

    f32x16 acc[TM][TN];
    float gbs = 0.f;
    __syncthreads();   // the encode table is in LDS
    tile_loop(acc, sA, sB, wm, wn, lane, kb, [&](int64_t k0) { return k0 < ke; }, [](int64_t k0) { return k0 + BK; }, load_tiles,
              store_tiles, [&]() { gb_add(gbs, sA, gb_on); });
    float* dstz = part + (int64_t)blockIdx.z * M * N + n0;
    store_acc(acc, wm, wn, lane, N - n0, 1.0f, [&](int r) -> float* { return m0 + r < M ? dstz + (int64_t)(m0 + r) * N : nullptr; });
    gb_store(gbpart, M, m0, gbs, gb_on);
}

// wt[tap][co][ci] = wq[co][ci][tap]
__global__ __launch_bounds__(256) void k_oihw_to_tap(const float* __restrict__ wq, float* __restrict__ wt, int Cout, int Cin, int T) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;   // over wt
    if (i >= (int64_t)Cout * Cin * T) return;
    const int ci = (int)(i % Cin);
    const int64_t r = i / Cin;
    const int co = (int)(r % Cout), tap = (int)(r / Cout);
    wt[i] = wq[((int64_t)co * Cin + ci) * T + tap];
}

// ---- host side -------------------------------------------------------------------------------------------------------
enum BwdKind { kBwdNone = 0, kBwdDw = 1, kBwdPw = 2, kBwdDense = 3 };

static BwdKind bwd_kind(const slfp_conv2d_desc& d) {
    if (d.groups == d.c_in && d.c_out == d.c_in && d.kh == 3 && d.kw == 3 && d.stride_h == d.stride_w &&
        (d.stride_h == 1 || d.stride_h == 2) && d.pad_h == 1 && d.pad_w == 1 && d.dil_h == 1 && d.dil_w == 1)
        return kBwdDw;
    if (d.groups == 1 && d.kh == 1 && d.kw == 1 && d.stride_h == 1 && d.stride_w == 1 && d.pad_h == 0 && d.pad_w == 0 &&
        d.dil_h == 1 && d.dil_w == 1)
        return kBwdPw;
    return kBwdNone;
}

// The dense family (SLFP_BWD_DENSE) takes what bwd_kind leaves: groups 1, dilation 1, any kernel size / stride / padding.
static bool dense_ok(const slfp_conv2d_desc& d, const ConvPlan& p) {
    if (d.groups != 1 || d.dil_h != 1 || d.dil_w != 1) return false;
    const int64_t lim = 0x7FFFFFFF;   // the kernels index rows and GEMM columns in 32 bits
    return d.n * d.h * d.w < lim && d.n * p.h_out * p.w_out < lim && (int64_t)d.kh * d.kw * d.c_in < lim;
}

static BwdKind bwd_kind_ex(const slfp_conv2d_desc& d, const ConvPlan& p, unsigned flags) {
    const BwdKind k = bwd_kind(d);
    if (k == kBwdNone && (flags & SLFP_BWD_DENSE) && dense_ok(d, p)) return kBwdDense;
    return k;
}

static size_t r256(size_t b) { return (b + 255) & ~(size_t)255; }

// The split choices depend on the shape only (not on the device), so that the workspace size is a pure function of the
// descriptor.  kBwdCUs: the MI355X's compute units.
constexpr int64_t kBwdCUs = 256;
constexpr int64_t kPartCapFloats = (int64_t)8 << 20;   // partials: at most 32 MiB
constexpr int kMaxParts = 1024;                        // rows summed per column by k_reduce_parts

static DwGeom dw_geom(const slfp_conv2d_desc& d, const ConvPlan& p) {
    DwGeom g;
    g.N = (int)d.n; g.H = (int)d.h; g.W = (int)d.w; g.C = (int)d.c_in; g.Ho = (int)p.h_out; g.Wo = (int)p.w_out;
    g.nbh = (int)ceil_div(g.Ho, kDwTH);
    g.nbw = (int)ceil_div(g.Wo, kDwTW);
    g.cw = g.C < 64 ? g.C : 64;
    g.rows = kDwThreads / g.cw;
    g.units = (int64_t)g.N * g.nbh * g.nbw;
    return g;
}

static int dw_blocks(const DwGeom& g) {
    int64_t pb = ceil_div(g.units, g.rows);
    const int64_t cap = kPartCapFloats / ((int64_t)kDwParts * g.C);
    if (pb > kMaxParts) pb = kMaxParts;
    if (pb > cap) pb = cap;
    return (int)(pb < 1 ? 1 : pb);
}

// The split of a GW contraction over its M rows: ~8 workgroups per CU, at least 256 rows per split, partials (cout x ncol
// and the cout bias sums per split) within kPartCapFloats, at most kMaxParts splits of whole k-steps.
struct GwSplit {
    int splits, kps;
};

// Whole float4 groups of channels on both sides: what the VEC instances need of the shape (the pointers' 16-byte alignment is
// checked at the entry points).
static bool chan_vec(const slfp_conv2d_desc& d) { return d.c_in % 4 == 0 && d.c_out % 4 == 0; }

static GwSplit gw_split(int64_t M, int64_t cout, int64_t ncol, int64_t tiles) {
    int64_t sp = ceil_div(8 * kBwdCUs, tiles);
    sp = std::min<int64_t>(sp, std::max<int64_t>(1, M / 256));
    sp = std::min<int64_t>(sp, std::max<int64_t>(1, kPartCapFloats / (cout * ncol + cout)));
    sp = std::min<int64_t>(sp, kMaxParts);
    if (sp < 1) sp = 1;
    const int64_t kps = ceil_div(ceil_div(M, sp), kGemmBK) * kGemmBK;
    return GwSplit{(int)ceil_div(M, kps), (int)kps};
}

struct PwShape {
    int64_t M;       // rows = N*H*W
    int tm_x, tn_x;  // GX tiling
    int tm_w, tn_w;  // GW tiling
    bool vec;        // float4 loads (chan_vec)
    int splits, kps; // GW split of M (gw_split)
};

static PwShape pw_shape(const slfp_conv2d_desc& d) {
    PwShape s;
    s.M = d.n * d.h * d.w;
    const int64_t cin = d.c_in, cout = d.c_out;
    s.tm_x = s.M >= 128 ? 2 : 1;  s.tn_x = cin >= 128 ? 2 : 1;
    s.tm_w = cout >= 128 ? 2 : 1; s.tn_w = cin >= 128 ? 2 : 1;
    s.vec = chan_vec(d);
    const GwSplit sp = gw_split(s.M, cout, cin, ceil_div(cout, 64 * s.tm_w) * ceil_div(cin, 64 * s.tn_w));
    s.splits = sp.splits; s.kps = sp.kps;
    return s;
}

struct DenseShape {
    int64_t M;       // rows of the gw contraction = N*Ho*Wo
    int64_t ncol;    // gw GEMM columns = taps * C_in
    int tn_x;        // GX tiling (TM = 2)
    int tm_w, tn_w;  // GW tiling
    bool vec;        // float4 loads (chan_vec); the scalar instances are tn_x = 1 and tm_w = tn_w = 1
    int splits, kps; // GW split of M (gw_split)
};

static DenseShape dense_shape(const slfp_conv2d_desc& d, const ConvPlan& p) {
    DenseShape s;
    s.M = d.n * p.h_out * p.w_out;
    s.ncol = (int64_t)d.kh * d.kw * d.c_in;
    const int64_t cout = d.c_out;
    s.vec = chan_vec(d);   // the scalar-gather instantiations exist at 64 x 64 only
    s.tn_x = s.vec && d.c_in >= 128 ? 2 : 1;
    s.tm_w = s.vec && cout >= 128 ? 2 : 1; s.tn_w = s.vec && s.ncol >= 128 ? 2 : 1;
    const GwSplit sp = gw_split(s.M, cout, s.ncol, ceil_div(cout, 64 * s.tm_w) * ceil_div(s.ncol, 64 * s.tn_w));
    s.splits = sp.splits; s.kps = sp.kps;
    return s;
}

static DenseGeom dense_geom(const slfp_conv2d_desc& d, const ConvPlan& p) {
    return DenseGeom{(int)d.n, (int)d.h, (int)d.w, (int)d.c_in, (int)p.h_out, (int)p.w_out, (int)d.c_out, (int)d.kh, (int)d.kw,
                     (int)d.stride_h, (int)d.stride_w, (int)d.pad_h, (int)d.pad_w};
}

// workgroups of k_dense_gx along x: the 128-row tiles of every (h mod stride_h, w mod stride_w) phase
static int64_t dense_gx_tiles(const DenseGeom& g) {
    int64_t tiles = 0;
    for (int a = 0; a < g.sh; ++a)
        for (int b = 0; b < g.sw; ++b)
            tiles += ceil_div((int64_t)g.N * dense_phase_extent(g.H, a, g.sh) * dense_phase_extent(g.W, b, g.sw), 128);
    return tiles;
}

struct BwdLayout {  // byte offsets into the workspace
    size_t x_nhwc, gy_nhwc, gx_nhwc, wq, wt, part, gbpart, total;
};

static BwdLayout bwd_layout(const slfp_conv2d_desc& d, const ConvPlan& p, BwdKind kind, bool need_gx, bool need_gw) {
    BwdLayout L;
    size_t off = 0;
    const size_t xb = (size_t)d.n * d.c_in * d.h * d.w * sizeof(float);
    const size_t yb = (size_t)d.n * d.c_out * p.h_out * p.w_out * sizeof(float);
    L.x_nhwc = off; if (need_gw && d.x_layout == SLFP_LAYOUT_NCHW) off += r256(xb);
    L.gy_nhwc = off; if (d.y_layout == SLFP_LAYOUT_NCHW) off += r256(yb);
    L.gx_nhwc = off; if (need_gx && d.x_layout == SLFP_LAYOUT_NCHW) off += r256(xb);
    L.wq = off; if (need_gx) off += r256((size_t)d.c_out * (d.c_in / d.groups) * d.kh * d.kw * sizeof(float));
    L.wt = off; if (need_gx && kind == kBwdDense) off += r256((size_t)d.c_out * d.c_in * d.kh * d.kw * sizeof(float));   // [tap][co][ci]
    L.part = off;
    L.gbpart = off;
    if (kind == kBwdDw && need_gw) {
        const DwGeom g = dw_geom(d, p);
        off += r256((size_t)dw_blocks(g) * kDwParts * g.C * sizeof(float));
    } else if (kind == kBwdPw && need_gw) {
        const PwShape s = pw_shape(d);
        if (s.splits > 1) off += r256((size_t)s.splits * d.c_out * d.c_in * sizeof(float));
        L.gbpart = off;
        off += r256((size_t)s.splits * d.c_out * sizeof(float));
    } else if (kind == kBwdDense && need_gw) {
        const DenseShape s = dense_shape(d, p);
        off += r256((size_t)s.splits * d.c_out * s.ncol * sizeof(float));   // [split][co][tap][ci], reduced into OIHW
        L.gbpart = off;
        off += r256((size_t)s.splits * d.c_out * sizeof(float));
    }
    L.total = off;
    return L;
}

// A runtime choice as a template argument: fn gets a std::integral_constant to read ::value from.
template <int V>
using Int = std::integral_constant<int, V>;

static const EncArgs kNone{};   // the table argument of a kernel that uses none

// The activation encode: the threshold table where act_table has one, else the long form of the format; the decode of the
// format's codes where x arrives as codes.
enum ActForm { kActTab = 0, kActLong = 1, kActCodes = 2 };
static ActForm act_form(const EncArgs* tab, bool x_codes) { return x_codes ? kActCodes : (tab ? kActTab : kActLong); }

template <class F>
static void with_act_enc(const EncArgs* tab, int fmt_act, bool x_codes, F fn) {
    const bool a8 = fmt_act == kFmtAct8;
    switch (act_form(tab, x_codes)) {
        case kActCodes:
            if (a8) fn(Int<kCodes8>{}, kNone);
            else fn(Int<kCodes7>{}, kNone);
            break;
        case kActTab: fn(Int<kEncTabQ>{}, *tab); break;
        default:
            if (a8) fn(Int<kFmtAct8>{}, kNone);
            else fn(Int<kFmtSfp7>{}, kNone);
    }
}

template <class F>
static void with_1_or_2(int v, F fn) {   // TM, TN, the depthwise stride
    if (v == 2) fn(Int<2>{});
    else fn(Int<1>{});
}

template <class F>
static void with_bool(bool b, F fn) {
    if (b) fn(std::true_type{});
    else fn(std::false_type{});
}

template <bool A_KMAJ, int AF>
static void launch_gemm(const GemmArgs& a, int tm, int tn, bool vec, hipStream_t st, const EncArgs& t, const ScaleDiv& sd) {
    const dim3 grid((unsigned)ceil_div(a.M, 64 * tm), (unsigned)ceil_div(a.N, 64 * tn), (unsigned)ceil_div(a.K, a.kps));
    with_1_or_2(tm, [&](auto TM) { with_1_or_2(tn, [&](auto TN) { with_bool(vec, [&](auto VEC) {
        hipLaunchKernelGGL((k_gemm_f32<decltype(TM)::value, decltype(TN)::value, A_KMAJ, AF, decltype(VEC)::value>), grid, dim3(256),
                           0, st, a, t, sd);
    }); }); });
}

static void launch_dense_gx(const DenseGeom& g, int tn, bool vec, hipStream_t st, const float* gy, const float* wt, float* gx,
                            float scale) {
    const dim3 grid((unsigned)dense_gx_tiles(g), (unsigned)ceil_div(g.Cin, 64 * tn));
    with_1_or_2(tn, [&](auto TN) { with_bool(vec, [&](auto VEC) {
        hipLaunchKernelGGL((k_dense_gx<decltype(TN)::value, decltype(VEC)::value>), grid, dim3(256), 0, st, gy, wt, gx, g, scale);
    }); });
}

template <int AF>
static void launch_dense_gw(const DenseGeom& g, const DenseShape& s, hipStream_t st, const float* gy, const float* x,
                            float* part, float* gbp, const EncArgs& t, const ScaleDiv& sd) {
    const dim3 grid((unsigned)ceil_div(g.Cout, 64 * s.tm_w), (unsigned)ceil_div(s.ncol, 64 * s.tn_w), (unsigned)s.splits);
    auto go = [&](auto TM, auto TN, auto VEC) {
        hipLaunchKernelGGL((k_dense_gw<decltype(TM)::value, decltype(TN)::value, AF, decltype(VEC)::value>), grid, dim3(256), 0, st,
                           gy, x, part, gbp, g, s.M, s.kps, t, sd);
    };
    if (!s.vec) go(Int<1>{}, Int<1>{}, std::false_type{});   // the scalar gather exists at 64 x 64 only (dense_shape)
    else with_1_or_2(s.tm_w, [&](auto TM) { with_1_or_2(s.tn_w, [&](auto TN) { go(TM, TN, std::true_type{}); }); });
}

static int reduce_parts(hipStream_t st, const float* part, int P, int64_t ncols, float scale, int dwC, int Cin, int T, float* gw,
                        float* gb) {
    hipLaunchKernelGGL(k_reduce_parts, dim3((unsigned)ceil_div(ncols, kRedCols)), dim3(kRedCols * kRedRows), 0, st, part, P, ncols,
                       scale, dwC, Cin, T, gw, gb);
    return check_launch("slfp backward reduction kernel");
}

// gb[co] = sum over the splits of the GW kernels' bias partials
static int reduce_gb(hipStream_t st, const float* gbpart, int splits, int64_t cout, float* gb) {
    return reduce_parts(st, gbpart, splits, cout, 1.0f, 0, 0, 0, gb, nullptr);
}

// What the code entry point adds to the supported set: the codes are NHWC with whole dwords of channels.
static bool codes_ok(const slfp_conv2d_desc& d) { return d.x_layout == SLFP_LAYOUT_NHWC && d.c_in % 4 == 0; }

// x_codes: x points at the 1-byte extended codes of QA(x / Ka) (slfp_conv2d_bwd_codes) instead of float32 values.
static int run_bwd(const slfp_conv2d_desc* d, unsigned flags, const float* x, const float* w, const float* gy, float* gx, float* gw,
                   float* gb, void* workspace, void* stream, bool x_codes = false) {
    ConvPlan p;
    int rc = make_plan(d, &p);
    if (rc != SLFP_OK) return rc;
    const BwdKind kind = bwd_kind_ex(*d, p, flags);
    if (kind == kBwdNone)
        return fail(SLFP_ERR_UNSUPPORTED, flags & SLFP_BWD_DENSE
                        ? "slfp_conv2d_bwd: only 3x3 depthwise (stride 1/2, pad 1) and groups-1 dilation-1 layers"
                        : "slfp_conv2d_bwd: only 3x3 depthwise (stride 1/2, pad 1) and stride-1 1x1 layers");
    if (x_codes && !codes_ok(*d))
        return fail(SLFP_ERR_UNSUPPORTED, "slfp_conv2d_bwd_codes: x_codes are NHWC with C_in a multiple of 4");
    if (!gy) return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd: null gy");
    if (gx && !w) return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd: gx needs the weights");
    if (gw && !x) return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd: gw needs the input");
    if (gb && !gw) return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd: gb is computed together with gw");
    const bool need_gx = gx != nullptr, need_gw = gw != nullptr, need_gb = gb != nullptr;
    if (!need_gx && !need_gw && !need_gb) return SLFP_OK;
    const BwdLayout L = bwd_layout(*d, p, kind, need_gx, need_gw);
    if (L.total && (!workspace || !aligned16(workspace)))
        return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd: %zu bytes of 16-byte aligned workspace required (slfp_conv2d_bwd_workspace_bytes)", L.total);
    unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
    hipStream_t st = as_stream(stream);
    const int64_t N = d->n, H = d->h, W = d->w, Cin = d->c_in, Cout = d->c_out, Ho = p.h_out, Wo = p.w_out;

    const float* x_n = x;
    if (need_gw && d->x_layout == SLFP_LAYOUT_NCHW) {
        float* t = reinterpret_cast<float*>(ws + L.x_nhwc);
        if ((rc = slfp_nchw_to_nhwc_f32(x, t, N, Cin, H, W, stream)) != SLFP_OK) return rc;
        x_n = t;
    }
    const float* gy_n = gy;
    if (d->y_layout == SLFP_LAYOUT_NCHW) {
        float* t = reinterpret_cast<float*>(ws + L.gy_nhwc);
        if ((rc = slfp_nchw_to_nhwc_f32(gy, t, N, Cout, Ho, Wo, stream)) != SLFP_OK) return rc;
        gy_n = t;
    }
    float* gx_n = gx;
    if (need_gx && d->x_layout == SLFP_LAYOUT_NCHW) gx_n = reinterpret_cast<float*>(ws + L.gx_nhwc);
    float* wq = reinterpret_cast<float*>(ws + L.wq);
    if (need_gx) {
        if ((rc = launch_quantize(w, wq, (size_t)Cout * (Cin / d->groups) * d->kh * d->kw, d->kw_scale, p.fmt_w, st)) != SLFP_OK)
            return rc;
    }
    const EncArgs* tab = act_table(d->ka, p.fmt_act, kEncF32);
    const ScaleDiv sd = make_scale_div(d->ka);

    if (kind == kBwdDw) {
        const DwGeom g = dw_geom(*d, p);
        const int pb = dw_blocks(g);
        float* part = reinterpret_cast<float*>(ws + L.part);
        const dim3 grid((unsigned)pb, (unsigned)ceil_div(g.C, g.cw));
        with_act_enc(tab, p.fmt_act, x_codes, [&](auto AF, const EncArgs& t) { with_1_or_2((int)d->stride_h, [&](auto S) {
            hipLaunchKernelGGL((k_dw3x3_bwd<decltype(S)::value, decltype(AF)::value>), grid, dim3(kDwThreads), 0, st, x_n, gy_n, wq,
                               gx_n, part, g, d->kw_scale, (int)need_gx, (int)need_gw, t, sd);
        }); });
        if ((rc = check_launch("slfp depthwise backward kernel")) != SLFP_OK) return rc;
        if (need_gw && (rc = reduce_parts(st, part, pb, (int64_t)kDwParts * g.C, d->ka, g.C, 0, 0, gw, gb)) != SLFP_OK) return rc;
    } else if (kind == kBwdDense) {
        const DenseShape s = dense_shape(*d, p);
        const DenseGeom g = dense_geom(*d, p);
        const int T = g.KH * g.KW;
        // every operand is 16-byte aligned (checked at the entry point; workspace offsets are multiples of 256)
        if (need_gx) {
            float* wt = reinterpret_cast<float*>(ws + L.wt);
            const int64_t nw = Cout * Cin * T;
            hipLaunchKernelGGL(k_oihw_to_tap, dim3((unsigned)ceil_div(nw, 256)), dim3(256), 0, st, wq, wt, (int)Cout, (int)Cin, T);
            if ((rc = check_launch("slfp dense backward weight re-layout kernel")) != SLFP_OK) return rc;
            launch_dense_gx(g, s.tn_x, s.vec, st, gy_n, wt, gx_n, d->kw_scale);
            if ((rc = check_launch("slfp dense backward (gx) kernel")) != SLFP_OK) return rc;
        }
        if (need_gw) {
            float* part = reinterpret_cast<float*>(ws + L.part);
            float* gbp = need_gb ? reinterpret_cast<float*>(ws + L.gbpart) : nullptr;
            with_act_enc(tab, p.fmt_act, x_codes, [&](auto AF, const EncArgs& t) {
                launch_dense_gw<decltype(AF)::value>(g, s, st, gy_n, x_n, part, gbp, t, sd);
            });
            if ((rc = check_launch("slfp dense backward (gw) kernel")) != SLFP_OK) return rc;
            if ((rc = reduce_parts(st, part, s.splits, Cout * s.ncol, d->ka, 0, (int)Cin, T, gw, nullptr)) != SLFP_OK) return rc;
            if (need_gb && (rc = reduce_gb(st, gbp, s.splits, Cout, gb)) != SLFP_OK) return rc;
        }
    } else {
        const PwShape s = pw_shape(*d);
        const bool vec = s.vec && aligned16(gy_n) && (!need_gw || x_codes || aligned16(x_n)) &&
                         (!need_gx || aligned16(wq));   // (codes are read a dword at a time whatever vec says)
        if (need_gx) {
            GemmArgs a{gy_n, wq, gx_n, nullptr, (int)s.M, (int)Cin, (int)Cout, Cout, Cin, Cin, (int)Cout, d->kw_scale};
            a.kps = (int)ceil_div(Cout, kGemmBK) * kGemmBK;
            launch_gemm<false, kNoEnc>(a, s.tm_x, s.tn_x, vec, st, kNone, sd);
            if ((rc = check_launch("slfp pointwise backward (gx) kernel")) != SLFP_OK) return rc;
        }
        if (need_gw) {
            float* part = s.splits > 1 ? reinterpret_cast<float*>(ws + L.part) : gw;
            float* gbp = reinterpret_cast<float*>(ws + L.gbpart);
            GemmArgs a{gy_n, x_n, part, need_gb ? gbp : nullptr, (int)Cout, (int)Cin, (int)s.M, Cout, Cin, Cin, s.kps,
                       s.splits > 1 ? 1.0f : d->ka};
            with_act_enc(tab, p.fmt_act, x_codes, [&](auto AF, const EncArgs& t) {
                launch_gemm<true, decltype(AF)::value>(a, s.tm_w, s.tn_w, vec, st, t, sd);
            });
            if ((rc = check_launch("slfp pointwise backward (gw) kernel")) != SLFP_OK) return rc;
            if (s.splits > 1 && (rc = reduce_parts(st, part, s.splits, Cout * Cin, d->ka, 0, 0, 0, gw, nullptr)) != SLFP_OK) return rc;
            if (need_gb && (rc = reduce_gb(st, gbp, s.splits, Cout, gb)) != SLFP_OK) return rc;
        }
    }
    if (need_gx && d->x_layout == SLFP_LAYOUT_NCHW) rc = slfp_nhwc_to_nchw_f32(gx_n, gx, N, Cin, H, W, stream);
    return rc;
}

}  // namespace slfp

using namespace slfp;

extern "C" {

int slfp_conv2d_bwd_supported_ex(const slfp_conv2d_desc* d, unsigned flags) {
    ConvPlan p;
    if (!d || (flags & ~SLFP_BWD_DENSE) || make_plan(d, &p) != SLFP_OK) return 0;
    return bwd_kind_ex(*d, p, flags) != kBwdNone ? 1 : 0;
}

const char* slfp_conv2d_bwd_kernel_name_ex(const slfp_conv2d_desc* d, unsigned flags) {
    ConvPlan p;
    if (!d || (flags & ~SLFP_BWD_DENSE) || make_plan(d, &p) != SLFP_OK) return "composite";
    switch (bwd_kind_ex(*d, p, flags)) {
        case kBwdDw: return "dw3x3_bwd";
        case kBwdPw: return "pw_bwd_mfma_f32";
        case kBwdDense: return "dense_bwd_mfma_f32";
        default: return "composite";
    }
}

size_t slfp_conv2d_bwd_workspace_bytes_ex(const slfp_conv2d_desc* d, unsigned flags, int need_gx, int need_gw) {
    ConvPlan p;
    if (!d || (flags & ~SLFP_BWD_DENSE) || make_plan(d, &p) != SLFP_OK) return 0;
    const BwdKind kind = bwd_kind_ex(*d, p, flags);
    if (kind == kBwdNone) return 0;
    return bwd_layout(*d, p, kind, need_gx != 0, need_gw != 0).total;
}

const char* slfp_debug_bwd_instance(const slfp_conv2d_desc* d, unsigned flags, int x_codes, int need_gx, int need_gw) {
    static thread_local char buf[192];
    ConvPlan p;
    if (!d || (flags & ~SLFP_BWD_DENSE) || make_plan(d, &p) != SLFP_OK) return "composite";
    const BwdKind kind = bwd_kind_ex(*d, p, flags);
    if (kind == kBwdNone || (x_codes && !codes_ok(*d))) return "composite";
    if (!need_gx && !need_gw) return "none";
    static const char* const kForm[] = {"tab", "long", "codes"};
    char enc[16];
    std::snprintf(enc, sizeof enc, "%s/%s", kForm[act_form(act_table(d->ka, p.fmt_act, kEncF32), x_codes != 0)],
                  p.fmt_act == kFmtAct8 ? "act8" : "sfp7");
    auto v = [](bool vec) { return vec ? "v4" : "v1"; };
    int n = 0;
    if (kind == kBwdDw) {
        std::snprintf(buf, sizeof buf, "dw/s%d/%s/b%d", (int)d->stride_h == 2 ? 2 : 1, enc, dw_blocks(dw_geom(*d, p)));
        return buf;
    }
    if (kind == kBwdDense) {
        const DenseShape s = dense_shape(*d, p);
        if (need_gx) n += std::snprintf(buf + n, sizeof buf - n, "dense/gx/tn%d/%s", s.tn_x, v(s.vec));
        if (need_gw)
            std::snprintf(buf + n, sizeof buf - n, "%sdense/gw/tm%dtn%d/%s/%s/p%dk%d", n ? "+" : "", s.tm_w, s.tn_w, v(s.vec), enc, s.splits,
                          s.kps);   // (!vec: dense_shape keeps tm_w = tn_w = 1, the one scalar instance launch_dense_gw has)
        return buf;
    }
    const PwShape s = pw_shape(*d);
    if (need_gx) n += std::snprintf(buf + n, sizeof buf - n, "pw/gx/tm%dtn%d/%s", s.tm_x, s.tn_x, v(s.vec));
    if (need_gw)
        std::snprintf(buf + n, sizeof buf - n, "%spw/gw/tm%dtn%d/%s/%s/p%dk%d", n ? "+" : "", s.tm_w, s.tn_w, v(s.vec), enc, s.splits, s.kps);
    return buf;
}

int slfp_conv2d_bwd_ex(const slfp_conv2d_desc* d, unsigned flags, const float* x, const float* w_oihw, const float* gy,
                       float* gx, float* gw_oihw, float* gb, void* workspace, void* stream) {
    if (!d) return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd: null descriptor");
    if (flags & ~SLFP_BWD_DENSE) return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd: unknown flag bits 0x%x", flags & ~SLFP_BWD_DENSE);
    if ((x && !aligned16(x)) || (w_oihw && !aligned16(w_oihw)) || (gy && !aligned16(gy)) || (gx && !aligned16(gx)) ||
        (gw_oihw && !aligned16(gw_oihw)) || (gb && !aligned16(gb)))
        return fail(SLFP_ERR_ALIGNMENT, "slfp_conv2d_bwd: tensors must be 16-byte aligned");
    return run_bwd(d, flags, x, w_oihw, gy, gx, gw_oihw, gb, workspace, stream);
}

int slfp_conv2d_bwd_codes_supported(const slfp_conv2d_desc* d, unsigned flags) {
    return slfp_conv2d_bwd_supported_ex(d, flags) && codes_ok(*d) ? 1 : 0;
}

int slfp_conv2d_bwd_codes(const slfp_conv2d_desc* d, unsigned flags, const uint8_t* x_codes, const float* w_oihw, const float* gy,
                          float* gx, float* gw_oihw, float* gb, void* workspace, void* stream) {
    if (!d) return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd_codes: null descriptor");
    if (flags & ~SLFP_BWD_DENSE) return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd_codes: unknown flag bits 0x%x", flags & ~SLFP_BWD_DENSE);
    if ((w_oihw && !aligned16(w_oihw)) || (gy && !aligned16(gy)) || (gx && !aligned16(gx)) || (gw_oihw && !aligned16(gw_oihw)) ||
        (gb && !aligned16(gb)))
        return fail(SLFP_ERR_ALIGNMENT, "slfp_conv2d_bwd_codes: tensors must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(x_codes) & 3) return fail(SLFP_ERR_ALIGNMENT, "slfp_conv2d_bwd_codes: x_codes must be 4-byte aligned");
    // the kernels take x as one pointer type; the code forms read it as bytes at the same element offsets (ActEnc::cx)
    return run_bwd(d, flags, reinterpret_cast<const float*>(x_codes), w_oihw, gy, gx, gw_oihw, gb, workspace, stream, true);
}

int slfp_conv2d_bwd_supported(const slfp_conv2d_desc* d) { return slfp_conv2d_bwd_supported_ex(d, 0u); }

const char* slfp_conv2d_bwd_kernel_name(const slfp_conv2d_desc* d) { return slfp_conv2d_bwd_kernel_name_ex(d, 0u); }

size_t slfp_conv2d_bwd_workspace_bytes(const slfp_conv2d_desc* d, int need_gx, int need_gw) {
    return slfp_conv2d_bwd_workspace_bytes_ex(d, 0u, need_gx, need_gw);
}

int slfp_conv2d_bwd(const slfp_conv2d_desc* d, const float* x, const float* w_oihw, const float* gy, float* gx,
                    float* gw_oihw, float* gb, void* workspace, void* stream) {
    return slfp_conv2d_bwd_ex(d, 0u, x, w_oihw, gy, gx, gw_oihw, gb, workspace, stream);
}

}  // extern "C"

