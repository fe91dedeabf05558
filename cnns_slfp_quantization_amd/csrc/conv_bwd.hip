// conv_bwd.hip -- quantization-aware backward of Conv2d_Q / Linear_Q for the depthwise 3x3 and pointwise 1x1 families
// (include/slfp.h: slfp_conv2d_bwd).
//
// The reference's forward is y = conv(QA(x/Ka), QW(w/Kw)) * Ka * Kw with straight-through estimators in both quantizers
// (utils/sfp_quant.py:50-53, 99-102), so its backward is
//     gx = conv_input(wq, gy) * Kw        wq = QW(w / Kw)
//     gw = conv_weight(xq, gy) * Ka       xq = QA(x / Ka)
//     gb = sum_{n,h,w} gy                 (conv2d_Q_bias; conv2d_Q's raw bias is added outside the Function)
// Everything accumulates in float32.  xq is never materialised: it is encoded on load with the forward's threshold table
// (slfp_enc.hpp; the long form of slfp_device.hpp where the table is unavailable), bit-identical to slfp_quantize_f32.
// wq is small: the caller quantizes it into the workspace first.
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
#include "slfp_host.hpp"

namespace slfp {

constexpr int kEncTabQ = -1;   // AF template argument: the threshold table (otherwise kFmtAct8 / kFmtSfp7: the long form)
constexpr int kNoEnc = -2;     // AF: the operand is used as is

// QA(x / Ka), bit-identical to slfp_quantize_f32 (codec.hip: k_quantize_tab / k_codec)
template <int AF>
__device__ __forceinline__ float qa1(float x, const float r1, const float lo, const float hi, const unsigned char* __restrict__ tb,
                                     const ScaleDiv sd, const uint32_t* __restrict__ sT) {
    if constexpr (AF == kEncTabQ) {
        const float r = enc_f32(x, r1, lo, hi, tb) + 0.0f;
        return x != x ? __uint_as_float(kBitsQNaN) : r;
    } else {
        return quantize_scaled<AF>(x, sd, sT);
    }
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
    if constexpr (AF == kEncTabQ) enc_fill<kDwThreads>(sE, t);
    else lut_fill<AF>(sT);
    __syncthreads();
    const unsigned char* tb = reinterpret_cast<const unsigned char*>(sE);
    const float r1 = t.r1, lo = t.lo, hi = t.hi;

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
        const float* xn = x + (int64_t)n * H * W * C + c;
        const float* gn = gy + (int64_t)n * Ho * Wo * C + c;
        const int xr0 = S * oh0 - 1;                    // first x row
        const int gr0 = S == 1 ? oh0 - 1 : oh0;         // first gy row
        auto ldx = [&](int row, int col) -> float {
            if (row < 0 || row >= H || col < 0 || col >= W) return 0.f;   // zero padding of xq
            return qa1<AF>(xn[((int64_t)row * W + col) * C], r1, lo, hi, tb, sd, sT);
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

// dst[col] = scale * sum_p part[p][col] over p = 0 .. P-1, in a fixed order.  dwC > 0: the depthwise layout col = k*C + c,
// k < 9 -> gw[c*9 + k] * scale, k == 9 -> gb[c] (unscaled); dwC == 0: gw[col] * scale.
constexpr int kRedCols = 16, kRedRows = 16;
__global__ __launch_bounds__(kRedCols * kRedRows) void k_reduce_parts(const float* __restrict__ part, int P, int64_t ncols,
                                                                       float scale, int dwC, float* __restrict__ gw,
                                                                       float* __restrict__ gb) {
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
    } else {
        gw[col] = sum * scale;
    }
}

// ---- float32 MFMA GEMM: C[M x N] = scale * A[M x K] * B[K x N] ---------------------------------------------------------
// A_KMAJ: A is stored [K][M] (m contiguous, lda = row pitch), else [M][K] (k contiguous).  B is stored [K][N].
// 4 waves in a 2 x 2 grid, each owning TM x TN tiles of 32 x 32; BK = 16.  blockIdx.z: a split of K (kps rows each);
// C then points at the split's partial [z][M][N].  gbpart != null (A_KMAJ only): the first column of workgroups also writes
// the sums of A over its K range per m, gbpart[z][m] (the bias gradient: A = GY^T).
constexpr int kGemmBK = 16;
typedef float f32x16 __attribute__((ext_vector_type(16)));

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
    __shared__ __attribute__((aligned(16))) uint2 sE[AF == kEncTabQ ? kEncEntries + 1 : 1];
    __shared__ uint32_t sT[16];
    if constexpr (AF == kEncTabQ) enc_fill<256>(sE, t);
    else if constexpr (AF != kNoEnc) lut_fill<AF>(sT);
    const unsigned char* tb = reinterpret_cast<const unsigned char*>(sE);
    const float r1 = t.r1, lo = t.lo, hi = t.hi;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int kb = blockIdx.z * ga.kps;
    const int ke = min(ga.K, kb + ga.kps);
    const int M = ga.M, N = ga.N;
    const bool do_gb = ga.gbpart != nullptr && blockIdx.y == 0;

    // global -> register staging: BK x BM of A and BK x BN of B as float4 groups (4 consecutive elements along the
    // contiguous dimension), zero outside the matrix
    constexpr int AV = BM * BK / 4 / 256, BV = BN * BK / 4 / 256;   // float4 groups per thread
    static_assert(AV >= 1 && BV >= 1, "tile too small for 256 threads");
    float4 ra[AV], rb[BV];
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
            rb[i] = ld4(ga.B, ga.ldb, k0 + kk, n0 + nn, ke, N);
        }
    };
    auto store_tiles = [&]() {
#pragma unroll
        for (int i = 0; i < AV; ++i) {
            const int e = tid + i * 256;
            if constexpr (A_KMAJ) {
                const int kk = e / (BM / 4), mm = (e % (BM / 4)) * 4;
                *reinterpret_cast<float4*>(&sA[kk][mm]) = ra[i];
            } else {
                const int mm = e / (BK / 4), kk = (e % (BK / 4)) * 4;
                sA[kk][mm] = ra[i].x; sA[kk + 1][mm] = ra[i].y; sA[kk + 2][mm] = ra[i].z; sA[kk + 3][mm] = ra[i].w;
            }
        }
#pragma unroll
        for (int i = 0; i < BV; ++i) {
            const int e = tid + i * 256;
            const int kk = e / (BN / 4), nn = (e % (BN / 4)) * 4;
            float4 v = rb[i];
            if constexpr (AF != kNoEnc) {   // QA(x / Ka) on load; padding zeros stay zero (Q(0) == 0)
                v.x = qa1<AF>(v.x, r1, lo, hi, tb, sd, sT); v.y = qa1<AF>(v.y, r1, lo, hi, tb, sd, sT);
                v.z = qa1<AF>(v.z, r1, lo, hi, tb, sd, sT); v.w = qa1<AF>(v.w, r1, lo, hi, tb, sd, sT);
            }
            *reinterpret_cast<float4*>(&sB[kk][nn]) = v;
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
    float gbs = 0.f;

    __syncthreads();   // the encode table is in LDS
    if (kb < ke) load_tiles(kb);
    for (int k0 = kb; k0 < ke; k0 += BK) {
        store_tiles();
        __syncthreads();
        if (k0 + BK < ke) load_tiles(k0 + BK);   // in flight while the MFMAs run
        if (do_gb && tid < BM) {
#pragma unroll
            for (int kk = 0; kk < BK; ++kk) gbs += sA[kk][tid];
        }
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
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
        __syncthreads();
    }
    // C/D map of the 32x32 f32 MFMA: col = lane & 31, row = (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int col = n0 + (wn * TN + j) * 32 + (lane & 31);
            if (col >= N) continue;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int row = m0 + (wm * TM + i) * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
                if (row < M) ga.C[(int64_t)blockIdx.z * M * N + (int64_t)row * ga.ldc + col] = acc[i][j][q] * ga.scale;
            }
        }
    if (do_gb && tid < BM && m0 + tid < M) ga.gbpart[(int64_t)blockIdx.z * M + m0 + tid] = gbs;
}

// ---- host side -------------------------------------------------------------------------------------------------------
enum BwdKind { kBwdNone = 0, kBwdDw = 1, kBwdPw = 2 };

static BwdKind bwd_kind(const slfp_conv2d_desc& d) {
    if (d.groups == d.c_in && d.c_out == d.c_in && d.kh == 3 && d.kw == 3 && d.stride_h == d.stride_w &&
        (d.stride_h == 1 || d.stride_h == 2) && d.pad_h == 1 && d.pad_w == 1 && d.dil_h == 1 && d.dil_w == 1)
        return kBwdDw;
    if (d.groups == 1 && d.kh == 1 && d.kw == 1 && d.stride_h == 1 && d.stride_w == 1 && d.pad_h == 0 && d.pad_w == 0 &&
        d.dil_h == 1 && d.dil_w == 1)
        return kBwdPw;
    return kBwdNone;
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

struct PwShape {
    int64_t M;       // rows = N*H*W
    int tm_x, tn_x;  // GX tiling
    int tm_w, tn_w;  // GW tiling
    int splits, kps; // GW split of M
};

static PwShape pw_shape(const slfp_conv2d_desc& d) {
    PwShape s;
    s.M = d.n * d.h * d.w;
    const int64_t cin = d.c_in, cout = d.c_out;
    s.tm_x = s.M >= 128 ? 2 : 1;  s.tn_x = cin >= 128 ? 2 : 1;
    s.tm_w = cout >= 128 ? 2 : 1; s.tn_w = cin >= 128 ? 2 : 1;
    const int64_t tiles = ceil_div(cout, 64 * s.tm_w) * ceil_div(cin, 64 * s.tn_w);
    int64_t sp = ceil_div(8 * kBwdCUs, tiles);                 // ~8 workgroups per CU
    sp = std::min<int64_t>(sp, std::max<int64_t>(1, s.M / 256)); // at least 256 rows per split
    sp = std::min<int64_t>(sp, std::max<int64_t>(1, kPartCapFloats / (cout * cin + cout)));
    sp = std::min<int64_t>(sp, kMaxParts);
    if (sp < 1) sp = 1;
    int64_t kps = ceil_div(ceil_div(s.M, sp), kGemmBK) * kGemmBK;
    s.kps = (int)kps;
    s.splits = (int)ceil_div(s.M, kps);
    return s;
}

struct BwdLayout {  // byte offsets into the workspace
    size_t x_nhwc, gy_nhwc, gx_nhwc, wq, part, gbpart, total;
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
    }
    L.total = off;
    return L;
}

template <int S>
static void launch_dw_s(dim3 grid, hipStream_t st, const float* x, const float* gy, const float* wq, float* gx, float* part,
                        const DwGeom& g, float kws, int ngx, int ngw, const EncArgs* tab, int fmt_act, const ScaleDiv& sd) {
    static const EncArgs kNone{};
    const EncArgs& t = tab ? *tab : kNone;
    if (tab) hipLaunchKernelGGL((k_dw3x3_bwd<S, kEncTabQ>), grid, dim3(kDwThreads), 0, st, x, gy, wq, gx, part, g, kws, ngx, ngw, t, sd);
    else if (fmt_act == kFmtAct8) hipLaunchKernelGGL((k_dw3x3_bwd<S, kFmtAct8>), grid, dim3(kDwThreads), 0, st, x, gy, wq, gx, part, g, kws, ngx, ngw, t, sd);
    else hipLaunchKernelGGL((k_dw3x3_bwd<S, kFmtSfp7>), grid, dim3(kDwThreads), 0, st, x, gy, wq, gx, part, g, kws, ngx, ngw, t, sd);
}

template <int TM, int TN, bool A_KMAJ, int AF>
static void launch_gemm_v(const GemmArgs& a, dim3 grid, hipStream_t st, const EncArgs& t, const ScaleDiv& sd, bool vec) {
    if (vec) hipLaunchKernelGGL((k_gemm_f32<TM, TN, A_KMAJ, AF, true>), grid, dim3(256), 0, st, a, t, sd);
    else hipLaunchKernelGGL((k_gemm_f32<TM, TN, A_KMAJ, AF, false>), grid, dim3(256), 0, st, a, t, sd);
}

template <bool A_KMAJ, int AF>
static void launch_gemm_t(const GemmArgs& a, int tm, int tn, hipStream_t st, const EncArgs& t, const ScaleDiv& sd, bool vec) {
    const dim3 grid((unsigned)ceil_div(a.M, 64 * tm), (unsigned)ceil_div(a.N, 64 * tn), (unsigned)ceil_div(a.K, a.kps));
    if (tm == 2 && tn == 2) launch_gemm_v<2, 2, A_KMAJ, AF>(a, grid, st, t, sd, vec);
    else if (tm == 2) launch_gemm_v<2, 1, A_KMAJ, AF>(a, grid, st, t, sd, vec);
    else if (tn == 2) launch_gemm_v<1, 2, A_KMAJ, AF>(a, grid, st, t, sd, vec);
    else launch_gemm_v<1, 1, A_KMAJ, AF>(a, grid, st, t, sd, vec);
}

static int run_bwd(const slfp_conv2d_desc* d, const float* x, const float* w, const float* gy, float* gx, float* gw,
                   float* gb, void* workspace, void* stream) {
    ConvPlan p;
    int rc = make_plan(d, &p);
    if (rc != SLFP_OK) return rc;
    const BwdKind kind = bwd_kind(*d);
    if (kind == kBwdNone)
        return fail(SLFP_ERR_UNSUPPORTED, "slfp_conv2d_bwd: only 3x3 depthwise (stride 1/2, pad 1) and stride-1 1x1 layers");
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
    static const EncArgs kNone{};

    if (kind == kBwdDw) {
        const DwGeom g = dw_geom(*d, p);
        const int pb = dw_blocks(g);
        float* part = reinterpret_cast<float*>(ws + L.part);
        const bool parts = need_gw;
        const dim3 grid((unsigned)pb, (unsigned)ceil_div(g.C, g.cw));
        if (d->stride_h == 1) launch_dw_s<1>(grid, st, x_n, gy_n, wq, gx_n, part, g, d->kw_scale, need_gx, parts, tab, p.fmt_act, sd);
        else launch_dw_s<2>(grid, st, x_n, gy_n, wq, gx_n, part, g, d->kw_scale, need_gx, parts, tab, p.fmt_act, sd);
        if ((rc = check_launch("slfp depthwise backward kernel")) != SLFP_OK) return rc;
        if (parts) {
            const int64_t ncols = (int64_t)kDwParts * g.C;
            hipLaunchKernelGGL(k_reduce_parts, dim3((unsigned)ceil_div(ncols, kRedCols)), dim3(kRedCols * kRedRows), 0, st, part, pb,
                               ncols, d->ka, g.C, gw, gb);
            if ((rc = check_launch("slfp backward reduction kernel")) != SLFP_OK) return rc;
        }
    } else {
        const PwShape s = pw_shape(*d);
        const bool vec = (Cin % 4) == 0 && (Cout % 4) == 0 && aligned16(gy_n) && (!need_gw || aligned16(x_n)) &&
                         (!need_gx || aligned16(wq));
        if (need_gx) {
            GemmArgs a{gy_n, wq, gx_n, nullptr, (int)s.M, (int)Cin, (int)Cout, Cout, Cin, Cin, (int)Cout, d->kw_scale};
            a.kps = (int)ceil_div(Cout, kGemmBK) * kGemmBK;
            launch_gemm_t<false, kNoEnc>(a, s.tm_x, s.tn_x, st, kNone, sd, vec);
            if ((rc = check_launch("slfp pointwise backward (gx) kernel")) != SLFP_OK) return rc;
        }
        if (need_gw) {
            float* part = s.splits > 1 ? reinterpret_cast<float*>(ws + L.part) : gw;
            float* gbp = reinterpret_cast<float*>(ws + L.gbpart);
            GemmArgs a{gy_n, x_n, part, need_gb ? gbp : nullptr, (int)Cout, (int)Cin, (int)s.M, Cout, Cin, Cin, s.kps,
                       s.splits > 1 ? 1.0f : d->ka};
            if (tab) launch_gemm_t<true, kEncTabQ>(a, s.tm_w, s.tn_w, st, *tab, sd, vec);
            else if (p.fmt_act == kFmtAct8) launch_gemm_t<true, kFmtAct8>(a, s.tm_w, s.tn_w, st, kNone, sd, vec);
            else launch_gemm_t<true, kFmtSfp7>(a, s.tm_w, s.tn_w, st, kNone, sd, vec);
            if ((rc = check_launch("slfp pointwise backward (gw) kernel")) != SLFP_OK) return rc;
            if (s.splits > 1) {
                const int64_t ncols = Cout * Cin;
                hipLaunchKernelGGL(k_reduce_parts, dim3((unsigned)ceil_div(ncols, kRedCols)), dim3(kRedCols * kRedRows), 0, st,
                                   part, s.splits, ncols, d->ka, 0, gw, nullptr);
                if ((rc = check_launch("slfp backward reduction kernel")) != SLFP_OK) return rc;
            }
            if (need_gb) {
                hipLaunchKernelGGL(k_reduce_parts, dim3((unsigned)ceil_div(Cout, kRedCols)), dim3(kRedCols * kRedRows), 0, st,
                                   gbp, s.splits, Cout, 1.0f, 0, gb, nullptr);
                if ((rc = check_launch("slfp backward reduction kernel")) != SLFP_OK) return rc;
            }
        }
    }
    if (need_gx && d->x_layout == SLFP_LAYOUT_NCHW) rc = slfp_nhwc_to_nchw_f32(gx_n, gx, N, Cin, H, W, stream);
    return rc;
}

}  // namespace slfp

using namespace slfp;

extern "C" {

int slfp_conv2d_bwd_supported(const slfp_conv2d_desc* d) {
    ConvPlan p;
    if (!d || make_plan(d, &p) != SLFP_OK) return 0;
    return bwd_kind(*d) != kBwdNone ? 1 : 0;
}

const char* slfp_conv2d_bwd_kernel_name(const slfp_conv2d_desc* d) {
    if (!slfp_conv2d_bwd_supported(d)) return "composite";
    return bwd_kind(*d) == kBwdDw ? "dw3x3_bwd" : "pw_bwd_mfma_f32";
}

size_t slfp_conv2d_bwd_workspace_bytes(const slfp_conv2d_desc* d, int need_gx, int need_gw) {
    ConvPlan p;
    if (!d || make_plan(d, &p) != SLFP_OK) return 0;
    const BwdKind kind = bwd_kind(*d);
    if (kind == kBwdNone) return 0;
    return bwd_layout(*d, p, kind, need_gx != 0, need_gw != 0).total;
}

int slfp_conv2d_bwd(const slfp_conv2d_desc* d, const float* x, const float* w_oihw, const float* gy, float* gx,
                    float* gw_oihw, float* gb, void* workspace, void* stream) {
    if (!d) return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd: null descriptor");
    if ((x && !aligned16(x)) || (w_oihw && !aligned16(w_oihw)) || (gy && !aligned16(gy)) || (gx && !aligned16(gx)) ||
        (gw_oihw && !aligned16(gw_oihw)) || (gb && !aligned16(gb)))
        return fail(SLFP_ERR_ALIGNMENT, "slfp_conv2d_bwd: tensors must be 16-byte aligned");
    return run_bwd(d, x, w_oihw, gy, gx, gw_oihw, gb, workspace, stream);
}

}  // extern "C"
