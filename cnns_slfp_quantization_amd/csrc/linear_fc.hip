// linear_fc.hip -- Linear_Q (utils/conv2d_func.py:60-65) as a weight-streaming skinny GEMM on 1-byte activation codes, gfx950.
//
//   y[M, N] = x[M, K] . W[N, K]^T      M = batch (1 ... a few hundred), K x N = a classifier layer (9216 x 4096, 25088 x 4096, 2048 x 1000)
//
// slfp_linear_fwd_prepared runs such a layer as a 1x1 convolution over `batch` pixels (conv_pw.hip): 64-row x 512-channel tiles, so
// ceil(M/64) x ceil(N/512) workgroups -- 8 for AlexNet's Linear(9216, 4096) at batch <= 64 on a 256-CU part -- each of which streams
// its whole K extent of W with one k-step in flight.  A classifier's cost is the weight stream, not the activation stream; this
// kernel is built around that:
//   * W is the SAME blob (slfp_linear_prepare_weights): one lane-linear 1 KiB fp16 fragment per (16-channel n-tile, 32-deep k-step),
//     n-tile major, so what a wave needs of W is NTW contiguous streams that go straight into registers (no LDS round trip: nothing
//     of W is shared between waves), two chunks of 8 / NTW k-steps deep: 8 KiB per wave in flight under the 8 KiB being multiplied.
//   * A workgroup is ONE wave: NTW n-tiles (1, 2 or 4) x MT row tiles of 16 rows.  The grid is n-groups x row blocks, no split over
//     K, no barrier after the tables are filled.  NTW and MT (1, 2 or 4 each) come from (M, N) by the measured rule of fc_select.
//   * X is 1-byte codes of QA(x / Ka) (float32 X is encoded once into the workspace by slfp_encode_f32): 1/4 of the bytes of float32,
//     and byte -> fp16 operand is a 256-entry LDS lookup (slfp_codes.hpp) instead of the encoder.  Every workgroup re-reads all the
//     rows of its row block from L2; the row blocks of one n-group sit on one XCD (xcd_remap).
// Bit-identity with slfp_linear_fwd_prepared (k_pw_stream for K <= 256, k_pw_tiled above): one output element is ONE accumulator
// chain of v_mfma_f32_16x16x32_f16(W fragment, X fragment, acc) over ascending k-steps from +0, lane (col, kq) feeding
// k = {4 kq .. 4 kq + 3, 16 + 4 kq .. 16 + 4 kq + 3} of each k-step -- the blob's order -- and the epilogue of slfp_epilogue.hpp with
// Linear_Q's scale order (s1 = Kw, s2 = Ka).  The zero-padded k-steps k_pw_tiled also multiplies add +0 to an accumulator that is
// never -0 (sums of exact products from +0), so leaving them out changes no bit.  The tiling is free.
// Output: float32 (optional ReLU), or the reader's codes (the ReLU folded into the quantizer: code4), 4 channels = one dword per lane.
// NaN inputs: the float32 interface propagates them, codes cannot carry them (slfp_encode_f32 gives 0x00): not bit-identical there.
#include <atomic>
#include "slfp_device.hpp"
#include "slfp_enc.hpp"
#include "slfp_codes.hpp"
#include "slfp_host.hpp"
#include "conv_pw_params.hpp"

namespace slfp {

struct FcParams {
    const uint8_t* x;      // [M][K] codes of QA(x / Ka), format fmt
    const _Float16* w;     // the pointwise blob: fragment (n-tile, k-step) at (n-tile * KS + k-step) * 512 halves
    const float* bias;     // [N] or nullptr
    void* y;               // [M][N] float32, or uint8 codes (yc)
    int64_t M;
    int K, N;
    int KS;                // k-steps per n-tile in the blob (k_pad / 32)
    int nks;               // k-steps that hold real channels: K / 32
    int n_tiles;           // 16-channel tiles that hold real channels: ceil(N / 16)
    uint32_t row_blocks;   // ceil(M / (16 MT))
    int fmt;               // format of the input codes (kFmtAct8 | kFmtSfp7)
    float s1, s2, s1x;     // out = ((acc / 256 + bias / s1 / s2) * s1) * s2; s1x = s1 / 256
    int relu;
    int yc;                // y receives the reader's codes
    int fmt_out;           // their format
    EncArgs enc;           // yc: code table of the reader's Ka (kEncCode)
};
static_assert(sizeof(FcParams) <= 4096, "FcParams must fit the 4 KiB kernel-argument segment");

// XW: K is a multiple of 64: a lane loads 16 consecutive codes of its row (two k-steps) and the wave transposes them into fragment
// order, as k_pwc_stream does; otherwise two dword loads per k-step.
template <int NTW, int MT, bool XW>
__global__ __launch_bounds__(64) void k_linear_fc(const FcParams p) {
    constexpr int CH = 8 / NTW;   // k-steps per chunk: 8 KiB of W per wave and chunk
    static_assert(CH % 2 == 0, "a 16-byte code load covers two k-steps");
    __shared__ __attribute__((aligned(16))) uint32_t sdec[256];
    __shared__ __attribute__((aligned(16))) unsigned char senc[kPwTab];
    if (p.fmt == kFmtSfp7) dec_fill<kFmtSfp7, kDecF16D, 64>(sdec);
    else dec_fill<kFmtAct8, kDecF16D, 64>(sdec);
    if (p.yc) enc_fill<64>(reinterpret_cast<uint2*>(senc), p.enc);
    __syncthreads();
    const unsigned char* dtab = reinterpret_cast<const unsigned char*>(sdec);

    const int lane = threadIdx.x;
    const int col = lane & 15, kq = lane >> 4;
    // logical block = n-group * row_blocks + row block: the row blocks that stream the same W are neighbours on one XCD
    const uint32_t b = xcd_remap(blockIdx.x, gridDim.x);
    const uint32_t rbk = b % p.row_blocks, ng = b / p.row_blocks;
    const int64_t m0 = (int64_t)rbk * (16 * MT);
    const int t0 = (int)ng * NTW;

    // every load below is unconditional: n-tiles past the last real one re-read it, rows past M re-read the last row, k-steps past
    // the end re-read the last one -- computed or skipped, never stored
    const _Float16* wj[NTW];
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
        const int t = t0 + j < p.n_tiles ? t0 + j : p.n_tiles - 1;
        wj[j] = p.w + ((size_t)t * p.KS) * 512 + lane * 8;
    }
    const uint8_t* xr[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int64_t m = m0 + i * 16 + col;
        xr[i] = p.x + (size_t)(m < p.M ? m : p.M - 1) * p.K + (XW ? kq * 16 : kq * 4);
    }

    constexpr int XR = XW ? CH / 2 : CH;   // X registers of a chunk: u32x4 per two k-steps, or a dword pair per k-step
    struct Chunk {
        half8 w[CH][NTW];
        u32x4 x[MT][XR];   // !XW: only [0], [1] of each are used
    };
    const int nks = p.nks;
    auto load_chunk = [&](int c, Chunk& q) {
#pragma unroll
        for (int s = 0; s < CH; ++s) {
            const int ks = c * CH + s < nks ? c * CH + s : nks - 1;
#pragma unroll
            for (int j = 0; j < NTW; ++j) q.w[s][j] = *reinterpret_cast<const half8*>(wj[j] + (size_t)ks * 512);
        }
#pragma unroll
        for (int i = 0; i < MT; ++i) {
#pragma unroll
            for (int s = 0; s < XR; ++s) {
                if constexpr (XW) {
                    const int c2 = c * (CH / 2) + s < (nks >> 1) ? c * (CH / 2) + s : (nks >> 1) - 1;
                    q.x[i][s] = *reinterpret_cast<const u32x4*>(xr[i] + c2 * 64);
                } else {
                    const int ks = c * CH + s < nks ? c * CH + s : nks - 1;
                    q.x[i][s][0] = *reinterpret_cast<const uint32_t*>(xr[i] + ks * 32);
                    q.x[i][s][1] = *reinterpret_cast<const uint32_t*>(xr[i] + ks * 32 + 16);
                }
            }
        }
    };

    floatx4 acc[MT][NTW];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NTW; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

    auto mfma_chunk = [&](int c, const Chunk& q) {
        uint32_t cw[MT][CH][2];
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            if constexpr (XW) {
#pragma unroll
                for (int s = 0; s < CH / 2; ++s) {
                    uint32_t a0 = q.x[i][s][0], a1 = q.x[i][s][1], a2 = q.x[i][s][2], a3 = q.x[i][s][3];
                    rows_transpose4(a0, a1, a2, a3);   // lane-quarter kq now holds codes 64 s + 16 r + 4 kq .. of its row in a_r
                    cw[i][2 * s][0] = a0; cw[i][2 * s][1] = a1; cw[i][2 * s + 1][0] = a2; cw[i][2 * s + 1][1] = a3;
                }
            } else {
#pragma unroll
                for (int s = 0; s < CH; ++s) { cw[i][s][0] = q.x[i][s][0]; cw[i][s][1] = q.x[i][s][1]; }
            }
        }
#pragma unroll
        for (int s = 0; s < CH; ++s) {
            if (c * CH + s < nks) {   // wave-uniform: the k-steps past the end were loaded (clamped) and are not multiplied
#pragma unroll
                for (int i = 0; i < MT; ++i) {
                    const uint2 pa = dec4_f16(cw[i][s][0], dtab), pb = dec4_f16(cw[i][s][1], dtab);
                    const half8 xh = __builtin_bit_cast(half8, u32x4{pa.x, pa.y, pb.x, pb.y});
#pragma unroll
                    for (int j = 0; j < NTW; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(q.w[s][j], xh, acc[i][j], 0, 0, 0);
                }
            }
        }
    };

    // two register sets: while one chunk is multiplied the loads of the next (CH k-steps of W) are in flight
    const int nch = (nks + CH - 1) / CH;
    Chunk qa, qb;
    load_chunk(0, qa);
    for (int c = 0; c < nch; c += 2) {
        load_chunk(c + 1, qb);
        mfma_chunk(c, qa);
        load_chunk(c + 2, qa);
        mfma_chunk(c + 1, qb);
    }

    // ---- epilogue: lane (col, kq) holds channels 16 t + 4 kq .. + 3 of row col of every (row tile, n-tile)
    const CodeQuant cq{p.enc.r1, p.enc.lo, p.enc.hi, p.relu ? 0 : 1, p.fmt_out};
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
        const int n = (t0 + j) * 16 + kq * 4;
        const bool n_ok = t0 + j < p.n_tiles && n < p.N;   // N is a multiple of 4: all four channels or none
        const float4 bq = n_ok ? bias_q256(p.bias, n, p.s1, p.s2) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int64_t m = m0 + i * 16 + col;
            float4 r = epilogue(acc[i][j], bq, p.s1x, p.s2);
            if (p.yc) {
                const uint32_t c = code4<false, true>(r, cq, senc);   // the ReLU, if any, is the quantizer's
                if (n_ok && m < p.M) *reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(p.y) + (size_t)m * p.N + n) = c;
            } else {
                if (p.relu) r = relu4(r);
                if (n_ok && m < p.M) *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.y) + (size_t)m * p.N + n) = r;
            }
        }
    }
}

// ---------------------------------------------------------------------------- selection and launch
// slfp_debug_linear_fc_tiles: n-tiles per workgroup / row tiles per workgroup forced for measurements (0: the rule below)
static std::atomic<int> g_force_ntw{0}, g_force_mt{0};

struct FcSel {
    int ntw, mt;
};

// The measured rule (profiles/linear_fc_bench.json; batch 1 ... 1024, N 1000 and 4096, every forced tiling): the
// largest tile per wave that still leaves the grid four waves -- one per SIMD -- for every CU, grown over n first (4, 2, 1 n-tiles:
// fewer re-reads and re-decodes of X) and, only once the n-group is 4 tiles wide, over rows (4, 2, 1 row tiles: fewer passes over W
// from L2).  Below four waves per CU the grid is as wide as the layer allows: one n-tile x 16 rows per wave.
static FcSel fc_select(int64_t M, int64_t N, int cus) {
    const int64_t tiles = ceil_div(N, 16), want = 4 * (int64_t)cus;
    FcSel s{1, 1};
    for (int w = 4; w >= 2; w >>= 1)
        if (ceil_div(tiles, w) * ceil_div(M, 16) >= want) { s.ntw = w; break; }
    if (s.ntw == 4)
        for (int r = 4; r >= 2; r >>= 1)
            if (ceil_div(tiles, 4) * ceil_div(M, 16 * r) >= want) { s.mt = r; break; }
    if (g_force_ntw.load(std::memory_order_relaxed)) s.ntw = g_force_ntw.load(std::memory_order_relaxed);
    if (g_force_mt.load(std::memory_order_relaxed)) s.mt = g_force_mt.load(std::memory_order_relaxed);
    return s;
}

template <int NTW, int MT>
static void (*fc_kernel_x(bool xw))(const FcParams) {
    return xw ? k_linear_fc<NTW, MT, true> : k_linear_fc<NTW, MT, false>;
}
template <int NTW>
static void (*fc_kernel_m(int mt, bool xw))(const FcParams) {
    return mt == 1 ? fc_kernel_x<NTW, 1>(xw) : (mt == 2 ? fc_kernel_x<NTW, 2>(xw) : fc_kernel_x<NTW, 4>(xw));
}
static void (*fc_kernel(const FcSel& s, bool xw))(const FcParams) {
    return s.ntw == 1 ? fc_kernel_m<1>(s.mt, xw) : (s.ntw == 2 ? fc_kernel_m<2>(s.mt, xw) : fc_kernel_m<4>(s.mt, xw));
}

static int y_fmt(int qbits) { return qbits == 7 ? kFmtSfp7 : kFmtAct8; }

// The host-only answer of slfp_linear_fc_supported.  Single-pass operand modes, K whole k-steps, N whole float4s (whole n-tiles with
// code output): such a layer's blob is always the pointwise family's.
static bool fc_supported(int64_t batch, int64_t in_f, int64_t out_f, int qbits, int mfma_passes, const slfp_conv2d_io* io, int relu) {
    if (!io || batch < 1 || in_f < 32 || out_f < 4) return false;
    if (qbits != 8 && qbits != 7) return false;
    if (mfma_passes != SLFP_MFMA_DEFAULT && mfma_passes != SLFP_MFMA_F16X1 && mfma_passes != SLFP_MFMA_F16X3) return false;
    if (qbits == 8 && mfma_passes == SLFP_MFMA_F16X3) return false;   // the float32-equivalent mode has two weight planes
    if (in_f % 32 || out_f % 4 || in_f > 0x7FFFFFFF || out_f > 0x7FFFFFFF) return false;
    if ((relu & ~SLFP_POST_RELU) != 0) return false;
    if ((io->x_codes != 0 && io->x_codes != 1) || (io->y_codes != 0 && io->y_codes != 1)) return false;
    if (long_encode_forced()) return false;   // SLFP_LONG_ENCODE keeps every kernel off the tables, as on the conv code paths
    if (ceil_div(out_f, 16) * ceil_div(batch, 16) > 0x7FFFFFFF) return false;
    if (io->y_codes) {
        if (out_f % 16) return false;
        if ((io->y_qbits != 8 && io->y_qbits != 7) || !(io->y_ka > 0.f) || !scale_div_ok(io->y_ka)) return false;
        if (!enc_table(io->y_ka, y_fmt(io->y_qbits), kEncCode)->valid) return false;
    }
    return true;
}

static size_t fc_workspace_bytes(int64_t batch, int64_t in_f, const slfp_conv2d_io* io) {
    if (!io || io->x_codes || batch < 1 || in_f < 1) return 0;
    return ((size_t)batch * (size_t)in_f + 255) & ~(size_t)255;   // the codes of a float32 x
}

}  // namespace slfp

using namespace slfp;

extern "C" {

int slfp_linear_fc_supported(int64_t batch, int64_t in_f, int64_t out_f, int qbits, int mfma_passes, const slfp_conv2d_io* io,
                             int has_bias, int relu) {
    (void)has_bias;   // with or without
    return fc_supported(batch, in_f, out_f, qbits, mfma_passes, io, relu) ? 1 : 0;
}

size_t slfp_linear_fc_workspace_bytes(int64_t batch, int64_t in_f, int64_t out_f, const slfp_conv2d_io* io) {
    (void)out_f;
    return fc_workspace_bytes(batch, in_f, io);
}

int slfp_debug_linear_fc_tiles(int n_tiles, int row_tiles) {
    const bool n_ok = n_tiles == 0 || n_tiles == 1 || n_tiles == 2 || n_tiles == 4;
    const bool m_ok = row_tiles == 0 || row_tiles == 1 || row_tiles == 2 || row_tiles == 4;
    if (!n_ok || !m_ok) return fail(SLFP_ERR_BAD_ARG, "slfp_debug_linear_fc_tiles: each of the two is 0 (the rule), 1, 2 or 4");
    g_force_ntw.store(n_tiles, std::memory_order_relaxed);
    g_force_mt.store(row_tiles, std::memory_order_relaxed);
    return SLFP_OK;
}

int slfp_linear_fwd_fc(const void* x, const void* wprep, const float* bias, void* y, int64_t batch, int64_t in_f, int64_t out_f,
                       float ka, float kw_scale, int qbits, int mfma_passes, const slfp_conv2d_io* io, int relu, void* workspace,
                       void* stream) {
    if (!io) return fail(SLFP_ERR_BAD_ARG, "slfp_linear_fwd_fc: null io");
    if (!fc_supported(batch, in_f, out_f, qbits, mfma_passes, io, relu))
        return fail(SLFP_ERR_UNSUPPORTED, "slfp_linear_fwd_fc: no weight-streaming kernel for this layer / io combination "
                                          "(slfp_linear_fc_supported); use slfp_linear_fwd_prepared");
    if (!(ka > 0.f) || !(kw_scale > 0.f)) return fail(SLFP_ERR_BAD_ARG, "slfp_linear_fwd_fc: Ka and Kw must be > 0");
    if (!scale_div_ok(ka) || !scale_div_ok(kw_scale)) return fail(SLFP_ERR_UNSUPPORTED, "slfp_linear_fwd_fc: Ka and Kw must be within [1e-30, 1e30]");
    if (!x || !wprep || !y) return fail(SLFP_ERR_BAD_ARG, "slfp_linear_fwd_fc: null pointer");
    if (!io->x_codes && !workspace) return fail(SLFP_ERR_BAD_ARG, "slfp_linear_fwd_fc: a float32 x needs the workspace (slfp_linear_fc_workspace_bytes)");
    if (!aligned16(x) || !aligned16(y) || !aligned16(wprep) || (bias && !aligned16(bias)) || (!io->x_codes && !aligned16(workspace)))
        return fail(SLFP_ERR_ALIGNMENT, "slfp_linear_fwd_fc: pointers must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    const int fmt = y_fmt(qbits);
    const uint8_t* xc = reinterpret_cast<const uint8_t*>(x);
    if (!io->x_codes) {   // input_q = QA(x / Ka) (utils/conv2d_func.py:60), once, as codes
        const int rc = slfp_encode_f32(reinterpret_cast<const float*>(x), reinterpret_cast<uint8_t*>(workspace),
                                       (size_t)batch * (size_t)in_f, ka, fmt | SLFP_FMT_EXT, stream);
        if (rc != SLFP_OK) return rc;
        xc = reinterpret_cast<const uint8_t*>(workspace);
    }
    FcParams p = {};
    p.x = xc; p.w = reinterpret_cast<const _Float16*>(wprep); p.bias = bias; p.y = y;
    p.M = batch; p.K = (int)in_f; p.N = (int)out_f;
    p.KS = (int)(ceil_div(in_f, 64) * 2);   // the blob's K is padded to 64 (make_plan_core)
    p.nks = (int)(in_f / 32);
    p.n_tiles = (int)ceil_div(out_f, 16);
    p.fmt = fmt;
    p.s1 = kw_scale; p.s2 = ka; p.s1x = kw_scale * (1.0f / 256.0f);   // Linear_Q: ((acc + bias / Kw / Ka) * Kw) * Ka
    p.relu = (relu & SLFP_POST_RELU) ? 1 : 0;
    p.yc = io->y_codes ? 1 : 0;
    p.fmt_out = y_fmt(io->y_qbits);
    p.enc.valid = 0;
    if (p.yc) p.enc = *enc_table(io->y_ka, p.fmt_out, kEncCode);
    const FcSel s = fc_select(batch, out_f, device_cu_count());
    p.row_blocks = (uint32_t)ceil_div(batch, 16 * s.mt);
    const int64_t nblocks = ceil_div(p.n_tiles, s.ntw) * (int64_t)p.row_blocks;
    if (nblocks > 0x7FFFFFFF) return fail(SLFP_ERR_UNSUPPORTED, "slfp_linear_fwd_fc: grid too large");
    hipLaunchKernelGGL(fc_kernel(s, in_f % 64 == 0), dim3((unsigned)nblocks), dim3(64), 0, st, p);
    return check_launch("slfp linear (fc) kernel");
}

}  // extern "C"
