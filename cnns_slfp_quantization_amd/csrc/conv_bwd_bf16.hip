// conv_bwd_bf16.hip -- the pointwise / Linear_Q backward (conv_bwd.hip's `pw` family) on the bf16 matrix cores, float32-equivalent
// through an exact three-way split (include/slfp.h: slfp_conv2d_bwd_bf16; opt-in, options.backward_gemm = "bf16x3").
//
//     gx[M x Cin]    = (GY[M x Cout] * WQ[Cout x Cin]) * Kw          M = N*H*W rows of NHWC
//     gw[Cout x Cin] = (GY^T * XQ[M x Cin]) * Ka, split over M       xq = QA(x / Ka), never materialised
//     gb[Cout]       = sum_m GY                                      float32 VALU adds
//
// A float32 a is p1 + p2 + p3 exactly, each p a bf16: p1 = the top 16 bits of a (truncation), p2 = the top 16 bits of a - p1, p3 = the
// rest (a carries 24 significant bits, each piece at most 8; the subtractions are exact, nothing rounds, nothing overflows).  A product
// of two pieces has at most 16 significant bits and is exact in float32, so v_mfma_f32_32x32x16_bf16 on the pieces accumulates what
// the float32 MFMA of conv_bwd.hip accumulates.  Both operands carry three planes and the six cross terms g_i * x_j with i + j <= 2
// are kept ("t6"; the three dropped ones are below 2 * 2^-24 |g||x| per product): eight k per instruction and six instructions against
// one float32 MFMA per two k.  SLFP<3,4> values 2^(m/16) need all 24 bits.  SFP<3,3> values have 4 significant bits and would fit one
// plane (a three-term form), but both quantizers also emit the class +-1e-10 (sfp_quant.py:43,92), a full 24-bit float32: in one
// plane it would be off by 2^-8, and a gradient element whose terms all come from that class would miss the 1e-5 bar.  So q_bit 7
// takes the six terms too and no three-term instance is built.  Within one MFMA k-step (16) the lowest-order terms are issued first.
//
// k_bf16_gemm<TM, TN, GW, FMT, XF>: 256 threads = 4 waves in a 2 x 2 grid, each owning TM x TN accumulators of 32 x 32 (a 64 x 64 wave
// tile at TM = TN = 2: per 16 of k, 12 ds_read_b128 feed 24 MFMAs in t6).  The 64 TM x 64 TN workgroup tile advances kBK = 32 per
// k-step through sA[3][BM][kPitch] and sB[3][BN][kPitch]: one row per output row / column, k contiguous, so that a lane's MFMA
// fragment (8 consecutive k of one row) is one 16-byte LDS read.  The split happens on the way into LDS, never in HBM:
//   gx  A: GY rows, k = c_out contiguous in memory: float4 loads, split, one 8-byte store per plane.
//       B: WQ, quantized into the workspace as on the float32 path, then written once by k_wq_planes as bf16 planes [plane][c_in][k]
//          (k padded to whole k-steps with zeros): a fragment's 8 k are consecutive in memory, the tile is copied 16 bytes at a time.
//   gw  both operands have k = m as their slow axis.  The transpose is made on the store: a thread loads four rows m .. m+3 of four
//       channels (4 float4, or 4 dwords of codes), and stores for each channel the four m as one 8-byte run per plane.  x goes through
//       the layer's threshold table first (XF = kXTab; bit-identical to slfp_quantize_f32), or its code bytes through a 256-entry LDS
//       table of the three pieces of decode(code) (XF = kXCodes, 2 KiB).
// kPitch = 40 bf16 (80 bytes): the sixteen rows a quarter wave reads with ds_read_b128 start at 16-byte offsets that are all distinct
// modulo 256, so fragment reads are bank-conflict-free; the gw stores of a half wave (8 m-groups x 4 channel groups) cover every bank
// twice: two passes for 8 bytes per lane, the minimum.
// The next k-step's global loads are in flight under the MFMAs (registers -> LDS after the barrier, as conv_bwd.hip's tile_loop).
// gb: the threads that stage GY^T add their four m per channel in registers; the eight m-groups of a channel meet in LDS once, in a
// fixed order.  No atomics anywhere: the gw splits go through conv_bwd.hip's gw_split / k_reduce_parts.
//
// Differences to the float32 kernels: an inf in gy splits into (inf, NaN, NaN), so outputs the float32 kernels make +-inf can be NaN
// here (the set of non-finite elements is the same); pieces below 2^-126 may be flushed by the matrix unit.
#include "slfp_device.hpp"
#include "slfp_enc.hpp"
#include "slfp_codes.hpp"
#include "slfp_host.hpp"
#include "conv_bwd_shared.hpp"
#include <algorithm>
#include <cstdio>
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

template <int TM, int TN, bool GW, int FMT, int XF>
__global__ __launch_bounds__(256) void k_bf16_gemm(const Bf16Args ga, const EncArgs t) {
    constexpr int BM = 64 * TM, BN = 64 * TN, PB = kPlanes;
    static_assert(GW == (XF != kXBlob), "gx reads the planes, gw reads x");
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
    auto ld4 = [](const float* p, int64_t off, bool ok) -> float4 {
        const float4 v = *reinterpret_cast<const float4*>(p + (ok ? off : 0));
        return ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    auto load_tiles = [&](int k0) {
        if constexpr (GW) {
            const int ca = m0 + 4 * cg, cb = n0 + 4 * cg;
            const bool oka = cg < BM / 4 && ca < M, okb = cg < BN / 4 && cb < N;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = k0 + 4 * mg + r;
                ra[r] = ld4(ga.gy, (int64_t)k * M + ca, oka && k < ke);
                const bool ok = okb && k < ke;
                const int64_t off = ok ? (int64_t)k * N + cb : 0;
                if constexpr (XF == kXTab) {
                    rbf[r] = ld4(reinterpret_cast<const float*>(ga.b), off, ok);
                } else {
                    const uint32_t v = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(ga.b) + off);
                    rbc[r] = ok ? v : 0x01010101u;   // four codes of exact zero
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
    // ---- acc += A * B over the staged k-step: per 16 of k the fragments of every plane, then the terms from the lowest order up
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
    auto mfma_step = [&]() {
#pragma unroll
        for (int s = 0; s < kBK / 16; ++s) {
            const int kk = s * 16 + 8 * (lane >> 5);
            bf16x8 a[3][TM], b[PB][TN];
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int i = 0; i < TM; ++i) a[p][i] = *reinterpret_cast<const bf16x8*>(&sA[p][(wm * TM + i) * 32 + (lane & 31)][kk]);
#pragma unroll
            for (int p = 0; p < PB; ++p)
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
    };

    __syncthreads();   // the table is in LDS
    if (kb < ke) load_tiles(kb);
    for (int k0 = kb; k0 < ke; k0 += kBK) {
        store_tiles();
        __syncthreads();
        if (k0 + kBK < ke) load_tiles(k0 + kBK);
        mfma_step();
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

// planes[p][ci][k] = piece p of wq[k][ci] as bf16, k < kpad (zeros from c_out on).  A workgroup transposes a tile of 32 k x 32 ci
// through LDS: the reads are 128-byte rows of wq (ci contiguous), the writes 16-byte chunks of 64-byte rows of the planes (k contiguous).
__global__ __launch_bounds__(256) void k_wq_planes(const float* __restrict__ wq, uint16_t* __restrict__ planes, int Cout, int Cin, int kpad) {
    __shared__ __attribute__((aligned(16))) uint16_t tile[kPlanes][32][kPitch];   // [plane][ci][k]
    const int ci0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
    const int c = threadIdx.x & 31;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = (threadIdx.x >> 5) + 8 * i;
        const bool ok = k0 + r < Cout && ci0 + c < Cin;
        const float v = wq[ok ? (int64_t)(k0 + r) * Cin + ci0 + c : 0];
        uint32_t b[3];
        split3(ok ? v : 0.f, b[0], b[1], b[2]);
#pragma unroll
        for (int p = 0; p < kPlanes; ++p) tile[p][c][r] = (uint16_t)(b[p] >> 16);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < kPlanes * 32 * 4; e += 256) {   // 16-byte chunks: (plane, ci, quarter of the 32 k)
        const int p = e >> 7, cc = (e >> 2) & 31, q = e & 3;
        if (ci0 + cc < Cin)   // k0 + 31 < kpad: the planes are padded to whole k-steps
            *reinterpret_cast<uint4*>(planes + ((int64_t)p * Cin + ci0 + cc) * kpad + k0 + q * 8) = *reinterpret_cast<const uint4*>(&tile[p][cc][q * 8]);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------
static size_t r256(size_t b) { return (b + 255) & ~(size_t)255; }

// What the launch is sized by: the tiles, the planes of the quantized operand, the gw split.  A function of the descriptor only.
struct Bf16Shape {
    int64_t M;        // rows = N*H*W
    int tm_x, tn_x;   // gx tiling
    int tm_w, tn_w;   // gw tiling
    int kpad;         // k pitch of the WQ planes
    int splits, kps;  // gw split of M (gw_split)
};

static Bf16Shape bf16_shape(const slfp_conv2d_desc& d) {
    Bf16Shape s;
    s.M = d.n * d.h * d.w;
    const int64_t cin = d.c_in, cout = d.c_out;
    s.tm_x = s.M >= 128 ? 2 : 1;  s.tn_x = cin >= 128 ? 2 : 1;
    s.tm_w = cout >= 128 ? 2 : 1; s.tn_w = cin >= 128 ? 2 : 1;
    s.kpad = (int)(ceil_div(cout, kBK) * kBK);
    const GwSplit sp = gw_split(s.M, cout, cin, ceil_div(cout, 64 * s.tm_w) * ceil_div(cin, 64 * s.tn_w));
    s.splits = sp.splits; s.kps = sp.kps;
    return s;
}

// The layers the kernels take, whichever way x arrives (what the workspace is sized for): 0 and the reason in slfp_last_error, or 1.
static int bf16_layer_ok(const slfp_conv2d_desc* d) {
    auto no = [](const char* why) { fail(SLFP_ERR_UNSUPPORTED, "slfp_conv2d_bwd_bf16: %s", why); return 0; };
    if (!bwd_is_pw(*d)) return no("only stride-1 1x1 layers (the pw family); depthwise and dense layers stay on slfp_conv2d_bwd_ex");
    if (d->x_layout != SLFP_LAYOUT_NHWC || d->y_layout != SLFP_LAYOUT_NHWC) return no("NHWC only");
    if (d->c_in % 8 != 0 || d->c_out % 8 != 0) return no("C_in and C_out must be multiples of 8");
    if (d->n * d->h * d->w >= 0x7FFFFF00) return no("N*H*W must stay below 2^31");
    // measured not faster than the float32 kernels by more than the spread (profiles/backward_bf16_bench.json), so not taken:
    // (a) the weight planes cost the same at every batch, what the GEMMs save grows with the rows: 25088 -> 4096 loses at 128 rows
    // (0.88x) and wins at 512 (1.24x); 4096 -> 4096 (2^24 elements) wins at 128 already
    if (d->n * d->h * d->w < 512 && d->c_in * d->c_out > ((int64_t)1 << 24))
        return no("fewer than 512 rows under a weight of more than 2^24 elements: the weight planes cost more than the GEMMs save");
    // (b) the HBM-bound layers with a narrow and a wide side at image sizes (64 -> 128, 64 -> 256, 256 -> 64 at 56 x 56, batch 128):
    // 1.01-1.09x, inside the spread in one of two runs; 32 -> 64 and 64 -> 64 stay in (1.18x, 1.02-1.07x beyond the spread in both)
    if (std::min(d->c_in, d->c_out) <= 64 && std::max(d->c_in, d->c_out) >= 128 && d->n * d->h * d->w >= 65536)
        return no("a side of at most 64 channels against one of at least 128 over 65536 rows or more measured level with the float32 kernels");
    return 1;
}

// ... and this operand form: float32 x needs the threshold table (codes are decoded, not encoded; NHWC with C_in % 8 == 0 is codes_ok)
static int bf16_supported(const slfp_conv2d_desc* d, const ConvPlan& p, bool x_codes) {
    if (!bf16_layer_ok(d)) return 0;
    if (!x_codes && !act_table(d->ka, p.fmt_act, kEncF32)) {
        fail(SLFP_ERR_UNSUPPORTED, "slfp_conv2d_bwd_bf16: no threshold table for this Ka (float32 x)");
        return 0;
    }
    return 1;
}

struct Bf16Layout {  // byte offsets into the workspace
    size_t wq, planes, part, gbpart, total;
};

static Bf16Layout bf16_layout(const slfp_conv2d_desc& d, const Bf16Shape& s, bool need_gx, bool need_gw) {
    Bf16Layout L;
    size_t off = 0;
    L.wq = off; if (need_gx) off += r256((size_t)d.c_out * d.c_in * sizeof(float));
    L.planes = off; if (need_gx) off += r256((size_t)kPlanes * d.c_in * s.kpad * sizeof(uint16_t));
    L.part = off; if (need_gw && s.splits > 1) off += r256((size_t)s.splits * d.c_out * d.c_in * sizeof(float));
    L.gbpart = off; if (need_gw) off += r256((size_t)s.splits * d.c_out * sizeof(float));
    L.total = off;
    return L;
}

template <int V>
using Int = std::integral_constant<int, V>;
template <class F>
static void with_1_or_2(int v, F fn) {
    if (v == 2) fn(Int<2>{});
    else fn(Int<1>{});
}

static const EncArgs kNoTable{};

template <bool GW, int XF, int FMT = kFmtAct8>
static void launch_bf16(const Bf16Args& a, int tm, int tn, hipStream_t st, const EncArgs& t) {
    const dim3 grid((unsigned)ceil_div(a.M, 64 * tm), (unsigned)ceil_div(a.N, 64 * tn), (unsigned)ceil_div(a.K, a.kps));
    with_1_or_2(tm, [&](auto TM) { with_1_or_2(tn, [&](auto TN) {
        hipLaunchKernelGGL((k_bf16_gemm<decltype(TM)::value, decltype(TN)::value, GW, FMT, XF>), grid, dim3(256), 0, st, a, t);
    }); });
}

}  // namespace slfp

using namespace slfp;

extern "C" {

int slfp_conv2d_bwd_bf16_supported(const slfp_conv2d_desc* d, unsigned flags, int x_codes) {
    ConvPlan p;
    if (!d || (flags & ~SLFP_BWD_DENSE) || make_plan(d, &p) != SLFP_OK) return 0;
    return bf16_supported(d, p, x_codes != 0);
}

size_t slfp_conv2d_bwd_bf16_workspace_bytes(const slfp_conv2d_desc* d, unsigned flags, int need_gx, int need_gw) {
    ConvPlan p;
    if (!d || (flags & ~SLFP_BWD_DENSE) || make_plan(d, &p) != SLFP_OK || !bf16_layer_ok(d)) return 0;   // the same for x and x_codes
    return bf16_layout(*d, bf16_shape(*d), need_gx != 0, need_gw != 0).total;
}

const char* slfp_debug_bwd_bf16_instance(const slfp_conv2d_desc* d, unsigned flags, int x_codes, int need_gx, int need_gw) {
    static thread_local char buf[160];
    ConvPlan p;
    if (!d || (flags & ~SLFP_BWD_DENSE) || make_plan(d, &p) != SLFP_OK || !bf16_supported(d, p, x_codes != 0)) return "none";
    if (!need_gx && !need_gw) return "none";
    const Bf16Shape s = bf16_shape(*d);
    int n = 0;
    if (need_gx) n += std::snprintf(buf + n, sizeof buf - n, "pwb/gx/tm%dtn%d/t6", s.tm_x, s.tn_x);
    if (need_gw)
        std::snprintf(buf + n, sizeof buf - n, "%spwb/gw/tm%dtn%d/t6/%s/p%dk%d", n ? "+" : "", s.tm_w, s.tn_w,
                      x_codes ? "codes" : "tab", s.splits, s.kps);
    return buf;
}

int slfp_conv2d_bwd_bf16(const slfp_conv2d_desc* d, unsigned flags, const float* x, const uint8_t* x_codes, const float* w_oihw,
                         const float* gy, float* gx, float* gw_oihw, float* gb, void* workspace, void* stream) {
    if (!d) return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd_bf16: null descriptor");
    if (flags & ~SLFP_BWD_DENSE) return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd_bf16: unknown flag bits 0x%x", flags & ~SLFP_BWD_DENSE);
    if ((x != nullptr) == (x_codes != nullptr)) return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd_bf16: exactly one of x and x_codes");
    if ((x && !aligned16(x)) || (w_oihw && !aligned16(w_oihw)) || (gy && !aligned16(gy)) || (gx && !aligned16(gx)) ||
        (gw_oihw && !aligned16(gw_oihw)) || (gb && !aligned16(gb)))
        return fail(SLFP_ERR_ALIGNMENT, "slfp_conv2d_bwd_bf16: tensors must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(x_codes) & 3) return fail(SLFP_ERR_ALIGNMENT, "slfp_conv2d_bwd_bf16: x_codes must be 4-byte aligned");
    ConvPlan p;
    int rc = make_plan(d, &p);
    if (rc != SLFP_OK) return rc;
    const bool codes = x_codes != nullptr;
    if (!bf16_supported(d, p, codes)) return SLFP_ERR_UNSUPPORTED;   // the reason is recorded
    if (!gy) return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd_bf16: null gy");
    if (gx && !w_oihw) return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd_bf16: gx needs the weights");
    if (gb && !gw_oihw) return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd_bf16: gb is computed together with gw");
    const bool need_gx = gx != nullptr, need_gw = gw_oihw != nullptr;
    if (!need_gx && !need_gw) return SLFP_OK;
    const Bf16Shape s = bf16_shape(*d);
    const Bf16Layout L = bf16_layout(*d, s, need_gx, need_gw);
    if (L.total && (!workspace || !aligned16(workspace)))
        return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd_bf16: %zu bytes of 16-byte aligned workspace required (slfp_conv2d_bwd_bf16_workspace_bytes)", L.total);
    unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
    hipStream_t st = as_stream(stream);
    const int Cin = (int)d->c_in, Cout = (int)d->c_out, M = (int)s.M;

    if (need_gx) {
        float* wq = reinterpret_cast<float*>(ws + L.wq);
        uint16_t* planes = reinterpret_cast<uint16_t*>(ws + L.planes);
        if ((rc = launch_quantize(w_oihw, wq, (size_t)Cout * Cin, d->kw_scale, p.fmt_w, st)) != SLFP_OK) return rc;
        hipLaunchKernelGGL(k_wq_planes, dim3((unsigned)ceil_div(Cin, 32), (unsigned)(s.kpad / 32)), dim3(256), 0, st, wq, planes, Cout, Cin, s.kpad);
        if ((rc = check_launch("slfp bf16 backward weight planes kernel")) != SLFP_OK) return rc;
        const Bf16Args a{gy, planes, gx, nullptr, M, Cin, Cout, s.kpad, s.kpad, d->kw_scale};
        launch_bf16<false, kXBlob>(a, s.tm_x, s.tn_x, st, kNoTable);
        if ((rc = check_launch("slfp bf16 pointwise backward (gx) kernel")) != SLFP_OK) return rc;
    }
    if (need_gw) {
        float* part = s.splits > 1 ? reinterpret_cast<float*>(ws + L.part) : gw_oihw;
        float* gbp = reinterpret_cast<float*>(ws + L.gbpart);
        const Bf16Args a{gy, codes ? (const void*)x_codes : (const void*)x, part, gb ? gbp : nullptr, Cout, Cin, M, 0, s.kps,
                         s.splits > 1 ? 1.0f : d->ka};
        if (codes && p.fmt_act == kFmtAct8) launch_bf16<true, kXCodes, kFmtAct8>(a, s.tm_w, s.tn_w, st, kNoTable);
        else if (codes) launch_bf16<true, kXCodes, kFmtSfp7>(a, s.tm_w, s.tn_w, st, kNoTable);
        else launch_bf16<true, kXTab>(a, s.tm_w, s.tn_w, st, *act_table(d->ka, p.fmt_act, kEncF32));
        if ((rc = check_launch("slfp bf16 pointwise backward (gw) kernel")) != SLFP_OK) return rc;
        if (s.splits > 1 && (rc = reduce_parts(st, part, s.splits, (int64_t)Cout * Cin, d->ka, 0, 0, 0, gw_oihw, nullptr)) != SLFP_OK) return rc;
        if (gb && (rc = reduce_gb(st, gbp, s.splits, Cout, gb)) != SLFP_OK) return rc;
    }
    return SLFP_OK;
}

}  // extern "C"
