// conv_bwd_bf16_core.hpp -- what the two bf16x3 backward translation units share (conv_bwd_bf16.hip: the pw family;
// conv_bwd_dense_bf16.hip: the dense family): the exact three-way split, the LDS geometry, the fragment-read + MFMA chunk and
// k_bf16_gemm, the GEMM kernel both instantiate.  The arithmetic is described at the top of conv_bwd_bf16.hip.
//
// k_bf16_gemm<TM, TN, GW, FMT, XF, AR>: 256 threads = 4 waves in a 2 x 2 grid, each owning TM x TN accumulators of 32 x 32 (a 64 x 64
// wave tile at TM = TN = 2: per 16 of k, 12 ds_read_b128 feed 24 MFMAs in t6).  The 64 TM x 64 TN workgroup tile advances kBK = 32 per
// k-step through sA[3][BM][kPitch] and sB[3][BN][kPitch]: one row per output row / column, k contiguous, so that a lane's MFMA
// fragment (8 consecutive k of one row) is one 16-byte LDS read.  The split happens on the way into LDS, never in HBM:
//   gx  A: GY rows, k = c_out contiguous in memory: float4 loads, split, one 8-byte store per plane.
//       B: WQ, quantized into the workspace as on the float32 path, then written once by k_wq_planes as bf16 planes [plane][c_in][k]
//          (k padded to whole k-steps with zeros): a fragment's 8 k are consecutive in memory, the tile is copied 16 bytes at a time.
//   gw  both operands have k = m as their slow axis.  The transpose is made on the store: a thread loads four rows m .. m+3 of four
//       channels (4 float4, or 4 dwords of codes), and stores for each channel the four m as one 8-byte run per plane.  x goes through
//       the layer's threshold table first (XF = kXTab; bit-identical to slfp_quantize_f32), or its code bytes through a 256-entry LDS
//       table of the three pieces of decode(code) (XF = kXCodes, 2 KiB).
//       AR is the row-address policy of gw's B operand: Bf16Args: row m of x is row m of an [M][C_in] matrix (the pw family);
//       Bf16DenseArgs: column group (tap, ci .. ci+3), row m = (n, ho, wo) is the input pixel (ho s_h - pad_h + kh, wo s_w - pad_w + kw)
//       of image n, and a pixel in the padding is an exact zero.  A thread decodes the first of its four m once per k-step (two
//       divisions) and walks the other three.
// kPitch = 40 bf16 (80 bytes): the sixteen rows a quarter wave reads with ds_read_b128 start at 16-byte offsets that are all distinct
// modulo 256, so fragment reads are bank-conflict-free; the gw stores of a half wave (8 m-groups x 4 channel groups) cover every bank
// twice: two passes for 8 bytes per lane, the minimum.
// The next k-step's global loads are in flight under the MFMAs (registers -> LDS after the barrier, as conv_bwd.hip's tile_loop).
// gb: the threads that stage GY^T add their four m per channel in registers; the eight m-groups of a channel meet in LDS once, in a
// fixed order.  No atomics anywhere: the gw splits go through conv_bwd.hip's gw_split / k_reduce_parts.
#pragma once
#include "slfp_device.hpp"
#include "slfp_enc.hpp"
#include "slfp_codes.hpp"
#include "slfp_host.hpp"
#include "conv_bwd_shared.hpp"
#include <type_traits>

namespace slfp {

constexpr int kBK = 32;       // contraction elements per k-step: two MFMAs of 16
constexpr int kPitch = 40;    // bf16 per LDS row
constexpr int kPlanes = 3;    // bf16 pieces of a float32
constexpr int kXBlob = 0;     // XF: B is the prepared bf16 planes of WQ (gx)
constexpr int kXTab = 1;      // XF: B is float32 x, encoded through the threshold table (gw)
constexpr int kXCodes = 2;    // XF: B is the 1-byte codes of xq (gw)

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// a = p1 + p2 + p3 exactly; b1..b3 are float32 bit patterns whose low 16 bits are zero (the bf16 sits in the high half)
__device__ __forceinline__ void split3(float a, uint32_t& b1, uint32_t& b2, uint32_t& b3) {
    b1 = __float_as_uint(a) & 0xFFFF0000u;
    const float r = a - __uint_as_float(b1);
    b2 = __float_as_uint(r) & 0xFFFF0000u;
    b3 = __float_as_uint(r - __uint_as_float(b2));
}
__device__ __forceinline__ uint32_t pack_hi(uint32_t lo, uint32_t hi) { return (lo >> 16) | (hi & 0xFFFF0000u); }

// four consecutive k of one row -> one 8-byte run per plane
__device__ __forceinline__ void split4(float v0, float v1, float v2, float v3, uint2 (&out)[kPlanes]) {
    uint32_t b[4][3];
    split3(v0, b[0][0], b[0][1], b[0][2]);
    split3(v1, b[1][0], b[1][1], b[1][2]);
    split3(v2, b[2][0], b[2][1], b[2][2]);
    split3(v3, b[3][0], b[3][1], b[3][2]);
#pragma unroll
    for (int p = 0; p < 3; ++p) out[p] = make_uint2(pack_hi(b[0][p], b[1][p]), pack_hi(b[2][p], b[3][p]));
}

// the 256-entry table of the code form: {p1 | p2 << 16, p3} of decode(code)
template <int FMT, int NT>
__device__ __forceinline__ void dec3_fill(uint2* sE) {
    for (int i = threadIdx.x; i < 256; i += NT) {
        uint32_t b1, b2, b3;
        split3(__uint_as_float(decode_ext_bits<FMT>((uint32_t)i)), b1, b2, b3);
        sE[i] = make_uint2((b1 >> 16) | b2, b3 >> 16);
    }
}

template <int TM, int TN>
__device__ __forceinline__ void bf16_acc_zero(f32x16 (&acc)[TM][TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
}

// acc += A * B over the staged k-step: per 16 of k the fragments of every plane, then the terms from the lowest order up
template <int TM, int TN, int BM, int BN>
__device__ __forceinline__ void bf16_mfma_step(const uint16_t (&sA)[kPlanes][BM][kPitch], const uint16_t (&sB)[kPlanes][BN][kPitch],
                                               int wm, int wn, int lane, f32x16 (&acc)[TM][TN]) {
#pragma unroll
    for (int s = 0; s < kBK / 16; ++s) {
        const int kk = s * 16 + 8 * (lane >> 5);
        bf16x8 a[kPlanes][TM], b[kPlanes][TN];
#pragma unroll
        for (int p = 0; p < kPlanes; ++p)
#pragma unroll
            for (int i = 0; i < TM; ++i) a[p][i] = *reinterpret_cast<const bf16x8*>(&sA[p][(wm * TM + i) * 32 + (lane & 31)][kk]);
#pragma unroll
        for (int p = 0; p < kPlanes; ++p)
#pragma unroll
            for (int j = 0; j < TN; ++j) b[p][j] = *reinterpret_cast<const bf16x8*>(&sB[p][(wn * TN + j) * 32 + (lane & 31)][kk]);
#pragma unroll
        for (int o = 2; o >= 0; --o)          // order of the term: i + j
#pragma unroll
            for (int pa = o; pa >= 0; --pa) {
                const int pb = o - pa;
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[pa][i], b[pb][j], acc[i][j], 0, 0, 0);
            }
    }
}

struct Bf16Args {
    const float* gy;     // A: gx [M][K] (k contiguous); gw [K][M] (GY^T read from NHWC rows)
    const void* b;       // B: gx the bf16 planes [3][N][kpad]; gw x as float32 or codes, [K][N]
    float* C;            // [z][M][N]
    float* gbpart;       // gw: [z][M] or null
    int M, N, K;         // rows and columns of C, contraction length
    int kpad;            // gx: k pitch of the planes
    int kps;             // K rows per split (blockIdx.z)
    float scale;
};

// gw of a dense layer: N = taps * C_in columns (tap, ci), K = N * Ho * Wo rows, b is NHWC x (float32 or codes)
struct Bf16DenseArgs : Bf16Args {
    DenseGeom g;
};

template <int TM, int TN, bool GW, int FMT, int XF, class AR = Bf16Args>
__global__ __launch_bounds__(256) void k_bf16_gemm(const AR ga, const EncArgs t) {
    constexpr int BM = 64 * TM, BN = 64 * TN, PB = kPlanes;
    constexpr bool DENSE = std::is_same<AR, Bf16DenseArgs>::value;
    static_assert(GW == (XF != kXBlob), "gx reads the planes, gw reads x");
    static_assert(GW || !DENSE, "the dense gx is k_dense_gx_bf16");
    __shared__ __attribute__((aligned(16))) uint16_t sA[3][BM][kPitch];
    __shared__ __attribute__((aligned(16))) uint16_t sB[PB][BN][kPitch];
    __shared__ __attribute__((aligned(16))) uint2 sE[XF == kXTab ? kEncEntries + 1 : (XF == kXCodes ? 256 : 1)];
    if constexpr (XF == kXTab) enc_fill<256>(sE, t);
    if constexpr (XF == kXCodes) dec3_fill<FMT, 256>(sE);
    const unsigned char* tb = reinterpret_cast<const unsigned char*>(sE);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int M = ga.M, N = ga.N;
    const int kb = blockIdx.z * ga.kps;
    const int ke = min(ga.K, kb + ga.kps);
    const bool gb_on = GW && ga.gbpart != nullptr && blockIdx.y == 0;

    // ---- global -> registers.  Everything a thread loads is all there or all absent (both channel counts are multiples of 8, gw's
    // k-steps start at multiples of 16 and its rows are single m), so each load is one guarded 16-byte (codes: 4-byte) access.
    constexpr int AV = GW ? 4 : BM / 32;   // float4 of A per thread
    constexpr int BV = GW ? 4 : BN / 64;   // gw: float4 / code dwords of x; gx: 16-byte chunks per plane
    float4 ra[AV];
    float4 rbf[XF == kXTab ? BV : 1];
    uint32_t rbc[XF == kXCodes ? BV : 1];
    uint4 rbp[XF == kXBlob ? PB : 1][XF == kXBlob ? BV : 1];
    // gw: thread (cg, mg) owns channels 4cg .. 4cg+3 and rows 4mg .. 4mg+3 of the k-step, for A (cg < BM/4) and for B (cg < BN/4)
    const int mg = tid & 7, cg = tid >> 3;
    // dense gw: the thread's B columns are one (tap, ci .. ci+3) group (C_in % 8 == 0 keeps it inside a tap), fixed over the K loop
    int b_kh = 0, b_kw = 0, b_ci = 0;
    if constexpr (DENSE) {
        const int cb = n0 + 4 * cg;
        const int tap = (cb < N ? cb : 0) / ga.g.Cin;
        b_ci = (cb < N ? cb : 0) - tap * ga.g.Cin;
        b_kh = tap / ga.g.KW - ga.g.padh;
        b_kw = tap % ga.g.KW - ga.g.padw;
    }
    auto ld4 = [](const float* p, int64_t off, bool ok) -> float4 {
        const float4 v = *reinterpret_cast<const float4*>(p + (ok ? off : 0));
        return ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    auto load_tiles = [&](int k0) {
        if constexpr (GW) {
            const int ca = m0 + 4 * cg, cb = n0 + 4 * cg;
            const bool oka = cg < BM / 4 && ca < M, okb = cg < BN / 4 && cb < N;
            int dn = 0, dho = 0, dwo = 0;   // dense: (n, ho, wo) of the thread's current m
            if constexpr (DENSE) {
                const int HWo = ga.g.Ho * ga.g.Wo, k = k0 + 4 * mg;
                dn = k / HWo;
                const int rem = k - dn * HWo;
                dho = rem / ga.g.Wo;
                dwo = rem - dho * ga.g.Wo;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = k0 + 4 * mg + r;
                ra[r] = ld4(ga.gy, (int64_t)k * M + ca, oka && k < ke);
                bool ok = okb && k < ke;
                int64_t off;
                if constexpr (DENSE) {
                    const int hi = dho * ga.g.sh + b_kh, wi = dwo * ga.g.sw + b_kw;
                    ok = ok && (unsigned)hi < (unsigned)ga.g.H && (unsigned)wi < (unsigned)ga.g.W;   // padding: an exact zero
                    off = ok ? (((int64_t)dn * ga.g.H + hi) * ga.g.W + wi) * ga.g.Cin + b_ci : 0;
                    if (++dwo == ga.g.Wo) {
                        dwo = 0;
                        if (++dho == ga.g.Ho) { dho = 0; ++dn; }
                    }
                } else {
                    off = ok ? (int64_t)k * N + cb : 0;
                }
                if constexpr (XF == kXTab) {
                    rbf[r] = ld4(reinterpret_cast<const float*>(ga.b), off, ok);
                } else {
                    const uint32_t v = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(ga.b) + off);
                    rbc[r] = ok ? v : 0x01010101u;   // four codes of exact zero (conv_bwd.hip's kCodeZero4)
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < AV; ++i) {
                const int e = tid + i * 256, row = m0 + (e >> 3), k = k0 + (e & 7) * 4;
                ra[i] = ld4(ga.gy, (int64_t)row * ga.K + k, row < M && k < ke);
            }
            const uint16_t* blob = reinterpret_cast<const uint16_t*>(ga.b);
#pragma unroll
            for (int p = 0; p < PB; ++p)
#pragma unroll
                for (int i = 0; i < BV; ++i) {
                    const int e = tid + i * 256, row = n0 + (e >> 2);
                    const bool ok = row < N;   // k0 + 8 (e & 3) + 7 < kpad: the planes are padded to whole k-steps
                    const uint4 v = *reinterpret_cast<const uint4*>(blob + (ok ? ((int64_t)p * N + row) * ga.kpad + k0 + (e & 3) * 8 : 0));
                    rbp[p][i] = ok ? v : make_uint4(0u, 0u, 0u, 0u);
                }
        }
    };
    // ---- registers -> LDS, splitting on the way
    float gbs[4] = {0.f, 0.f, 0.f, 0.f};
    auto store_tiles = [&]() {
        if constexpr (GW) {
            if (cg < BM / 4) {
                const float* a0 = &ra[0].x; const float* a1 = &ra[1].x; const float* a2 = &ra[2].x; const float* a3 = &ra[3].x;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    uint2 o[3];
                    split4(a0[j], a1[j], a2[j], a3[j], o);
#pragma unroll
                    for (int p = 0; p < 3; ++p) *reinterpret_cast<uint2*>(&sA[p][4 * cg + j][4 * mg]) = o[p];
                    if (gb_on) { gbs[j] += a0[j]; gbs[j] += a1[j]; gbs[j] += a2[j]; gbs[j] += a3[j]; }
                }
            }
            if (cg < BN / 4) {
                if constexpr (XF == kXTab) {
                    float4 q[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {   // QA(x / Ka) as conv_bwd.hip's ActEnc: -0 becomes +0, NaN stays NaN
                        q[r] = enc4_f32_raw(rbf[r], t.r1, t.lo, t.hi, tb);
                        q[r].x += 0.0f; q[r].y += 0.0f; q[r].z += 0.0f; q[r].w += 0.0f;
                        enc_fix_nan4(rbf[r], q[r]);
                    }
                    const float* b0 = &q[0].x; const float* b1 = &q[1].x; const float* b2 = &q[2].x; const float* b3 = &q[3].x;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        uint2 o[PB];
                        split4(b0[j], b1[j], b2[j], b3[j], o);
#pragma unroll
                        for (int p = 0; p < PB; ++p) *reinterpret_cast<uint2*>(&sB[p][4 * cg + j][4 * mg]) = o[p];
                    }
                } else if constexpr (XF == kXCodes) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        uint2 e[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) e[r] = sE[(rbc[r] >> (8 * j)) & 0xFFu];
                        *reinterpret_cast<uint2*>(&sB[0][4 * cg + j][4 * mg]) =
                            make_uint2((e[0].x & 0xFFFFu) | (e[1].x << 16), (e[2].x & 0xFFFFu) | (e[3].x << 16));
                        *reinterpret_cast<uint2*>(&sB[1][4 * cg + j][4 * mg]) =
                            make_uint2((e[0].x >> 16) | (e[1].x & 0xFFFF0000u), (e[2].x >> 16) | (e[3].x & 0xFFFF0000u));
                        *reinterpret_cast<uint2*>(&sB[2][4 * cg + j][4 * mg]) =
                            make_uint2((e[0].y & 0xFFFFu) | (e[1].y << 16), (e[2].y & 0xFFFFu) | (e[3].y << 16));
                    }
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < AV; ++i) {
                const int e = tid + i * 256;
                uint2 o[3];
                split4(ra[i].x, ra[i].y, ra[i].z, ra[i].w, o);
#pragma unroll
                for (int p = 0; p < 3; ++p) *reinterpret_cast<uint2*>(&sA[p][e >> 3][(e & 7) * 4]) = o[p];
            }
#pragma unroll
            for (int p = 0; p < PB; ++p)
#pragma unroll
                for (int i = 0; i < BV; ++i) {
                    const int e = tid + i * 256;
                    *reinterpret_cast<uint4*>(&sB[p][e >> 2][(e & 3) * 8]) = rbp[p][i];
                }
        }
    };
    f32x16 acc[TM][TN];
    bf16_acc_zero(acc);

    __syncthreads();   // the table is in LDS
    if (kb < ke) load_tiles(kb);
    for (int k0 = kb; k0 < ke; k0 += kBK) {
        store_tiles();
        __syncthreads();
        if (k0 + kBK < ke) load_tiles(k0 + kBK);
        bf16_mfma_step<TM, TN>(sA, sB, wm, wn, lane, acc);
        __syncthreads();
    }

    // C/D map of the 32x32 MFMA: col = lane & 31, row = (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5)
    float* cz = ga.C + (int64_t)blockIdx.z * M * N;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int row = m0 + (wm * TM + i) * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
            if (row >= M) continue;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int col = n0 + (wn * TN + j) * 32 + (lane & 31);
                if (col < N) cz[(int64_t)row * N + col] = acc[i][j][q] * ga.scale;
            }
        }
    if constexpr (GW) {
        if (!gb_on) return;   // workgroup-uniform
        float* sRed = reinterpret_cast<float*>(&sA[0][0][0]);   // [8][BM]; the K loop ended on a barrier
        if (cg < BM / 4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) sRed[mg * BM + 4 * cg + j] = gbs[j];
        }
        __syncthreads();
        if (tid < BM && m0 + tid < M) {
            float s = 0.f;
#pragma unroll
            for (int g = 0; g < 8; ++g) s += sRed[g * BM + tid];
            ga.gbpart[(int64_t)blockIdx.z * M + m0 + tid] = s;
        }
    }
}

// ---- host side: what both launchers use --------------------------------------------------------------------------------
static inline size_t r256(size_t b) { return (b + 255) & ~(size_t)255; }

template <int V>
using Bf16Int = std::integral_constant<int, V>;
template <class F>
static void bf16_1_or_2(int v, F fn) {
    if (v == 2) fn(Bf16Int<2>{});
    else fn(Bf16Int<1>{});
}

template <bool GW, int XF, int FMT = kFmtAct8, class AR>
static void launch_bf16(const AR& a, int tm, int tn, hipStream_t st, const EncArgs& t) {
    const dim3 grid((unsigned)ceil_div(a.M, 64 * tm), (unsigned)ceil_div(a.N, 64 * tn), (unsigned)ceil_div(a.K, a.kps));
    bf16_1_or_2(tm, [&](auto TM) { bf16_1_or_2(tn, [&](auto TN) {
        hipLaunchKernelGGL((k_bf16_gemm<decltype(TM)::value, decltype(TN)::value, GW, FMT, XF, AR>), grid, dim3(256), 0, st, a, t);
    }); });
}

// gw with x in the form the caller has: codes of either format, or float32 through the layer's threshold table
template <class AR>
static void launch_bf16_gw(const AR& a, int tm, int tn, hipStream_t st, bool codes, int fmt_act, const EncArgs* tab) {
    static const EncArgs kNoTable{};
    if (codes && fmt_act == kFmtAct8) launch_bf16<true, kXCodes, kFmtAct8>(a, tm, tn, st, kNoTable);
    else if (codes) launch_bf16<true, kXCodes, kFmtSfp7>(a, tm, tn, st, kNoTable);
    else launch_bf16<true, kXTab>(a, tm, tn, st, *tab);
}

}  // namespace slfp
