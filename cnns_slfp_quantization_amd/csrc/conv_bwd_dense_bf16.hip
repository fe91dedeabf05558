// conv_bwd_dense_bf16.hip -- the dense backward family (conv_bwd.hip's k_dense_gx / k_dense_gw: groups 1, dilation 1, any kernel
// size / stride / padding that is neither pw nor the depthwise 3x3) on the bf16 matrix cores, float32-equivalent through the exact
// three-way split of conv_bwd_bf16.hip (include/slfp.h: slfp_conv2d_bwd_dense_bf16; opt-in, options.backward_gemm = "bf16x3_all").
//
//     gx[(n,h,w)][ci]     = Kw * sum_(tap,co) GY[n, (h+pad_h-kh)/s_h, (w+pad_w-kw)/s_w, co] * WQ[co][ci][tap]
//     gw[z][co][(tap,ci)] = sum_m GY[m][co] * QA(X[n, ho s_h - pad_h + kh, wo s_w - pad_w + kw, ci] / Ka)     m = (n, ho, wo), split over m
//     gb[co]              = sum_m GY                                                                          float32 VALU adds
//
// The arithmetic, the 80-byte LDS pitch, the fragment reads and the six-term issue order are conv_bwd_bf16_core.hpp's; only the
// address arithmetic of the two gathers is new.
//
// gx: k_dense_gx_bf16<TN>, a kernel of its own over the shared chunk (bf16_mfma_step), with k_dense_gx's work split: the 128 rows of
// a workgroup lie in one (h mod s_h, w mod s_w) phase, so a tap reaches every row of the tile or none and the taps that reach none
// are skipped workgroup-uniformly; a phase no tap reaches (1x1 stride 2: three of four) is written as exact zeros.  K runs over
// (tap, co) with each tap's co run padded to whole k-steps of 32, so no k-step straddles a tap.
//   A: a thread owns four rows (32 apart) and four consecutive co of the k-step: a float4 gather from NHWC gy on a clamped address with
//      a select to zero, split in registers, one 8-byte store per plane into sA[3][128][40].  The rows' (n, h, w) are decoded once.
//   B: k_wq_tap_planes writes the quantized weight once per call as bf16 planes [plane][tap][ci][co padded to 32, zeros]: fragment
//      order, so a tile is 16-byte copies with no transpose (it stands where k_oihw_to_tap stands on the float32 path).
// gw: the instances k_bf16_gemm<TM, TN, true, FMT, XF, Bf16DenseArgs> of the shared GEMM kernel: A (GY^T), the gb partial sums, the
// transpose on the store and the splits are the pw form's; the row-address policy Bf16DenseArgs decodes where a row of B comes from.
// The partials go through reduce_parts' dense output map (Cin, T) into OIHW scaled by Ka, also at one split.  No atomics.
//
// Bank pattern of the stores (64 banks of 4 bytes, rows 80 bytes apart): the gx A store of a half wave is 4 rows x 8 lanes of 8 bytes;
// a row's 64 bytes are contiguous and row r starts at bank 20 r mod 64 = 0, 20, 40, 60, so the fourth row wraps onto banks 0-11 of
// the first: partly two-way, the pattern of the pw gx A store (same thread-to-row map); the B copies (16 bytes per lane, 4 lanes per
// row) are the pw gx form.  The gw stores are the pw gw form unchanged: every bank exactly twice per half wave.
//
// Differences to the float32 kernels: those of conv_bwd_bf16.hip (an inf in gy may give NaN where they give +-inf; pieces below 2^-126
// may be flushed; not bit-equal).
#include "conv_bwd_bf16_core.hpp"
#include <algorithm>
#include <cstdio>

namespace slfp {

struct TapStep32 { int t, c0; };   // a k-step of the gx kernel: 32 output channels from c0 of tap t

template <int TN>
__global__ __launch_bounds__(256) void k_dense_gx_bf16(const float* __restrict__ gy, const uint16_t* __restrict__ planes,
                                                        float* __restrict__ gx, const DenseGeom g, const int copad, const float scale) {
    constexpr int TM = 2, BM = 64 * TM, BN = 64 * TN;
    __shared__ __attribute__((aligned(16))) uint16_t sA[kPlanes][BM][kPitch];
    __shared__ __attribute__((aligned(16))) uint16_t sB[kPlanes][BN][kPitch];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int Cin = g.Cin, Cout = g.Cout, Ho = g.Ho, Wo = g.Wo, T = g.KH * g.KW;

    // the workgroup's phase and its row tile inside the phase (workgroup-uniform; the order of dense_gx_tiles)
    int bx = blockIdx.x, ph = 0, pw = 0, Hp = 1, Wp = 1, rows = 0;   // N*H*W < 2^31 (dense_ok)
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

    constexpr int AV = BM / 32, BV = BN / 64;   // float4 of A per thread; 16-byte chunks of B per plane and thread
    float4 ra[AV];
    uint4 rb[kPlanes][BV];
    // the A rows of this thread (tid / 8 + 32 i) and its four co of the k-step: fixed for the whole K loop
    const int kq = (tid & 7) * 4;
    int a_nb[AV], a_h[AV], a_w[AV];
    bool a_ok[AV];
#pragma unroll
    for (int i = 0; i < AV; ++i) {
        const int r = r0 + (tid >> 3) + 32 * i;
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
    auto next_step = [&](TapStep32 s) -> TapStep32 {
        if (s.c0 + kBK < Cout) return TapStep32{s.t, s.c0 + kBK};
        return TapStep32{next_tap(s.t + 1), 0};
    };
    auto load_tiles = [&](TapStep32 s) {
        const int t = s.t, c0 = s.c0;
        const int dh = (ph + g.padh - t / g.KW) / g.sh, dw = (pw + g.padw - t % g.KW) / g.sw;   // exact
        const int co = c0 + kq;   // C_out % 8 == 0: the four are all there or all absent
#pragma unroll
        for (int i = 0; i < AV; ++i) {
            const int ho = a_h[i] + dh, wo = a_w[i] + dw;
            const bool ok = a_ok[i] && co < Cout && (unsigned)ho < (unsigned)Ho && (unsigned)wo < (unsigned)Wo;
            const float4 v = *reinterpret_cast<const float4*>(gy + (ok ? ((int64_t)(a_nb[i] + ho) * Wo + wo) * Cout + co : 0));
            ra[i] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int p = 0; p < kPlanes; ++p)
#pragma unroll
            for (int i = 0; i < BV; ++i) {
                const int e = tid + i * 256, row = n0 + (e >> 2);
                const bool ok = row < Cin;   // c0 + 8 (e & 3) + 7 < copad: a tap's co run is padded to whole k-steps
                const uint4 v = *reinterpret_cast<const uint4*>(planes + (ok ? (((int64_t)p * T + t) * Cin + row) * copad + c0 + (e & 3) * 8 : 0));
                rb[p][i] = ok ? v : make_uint4(0u, 0u, 0u, 0u);
            }
    };
    auto store_tiles = [&]() {
#pragma unroll
        for (int i = 0; i < AV; ++i) {
            uint2 o[kPlanes];
            split4(ra[i].x, ra[i].y, ra[i].z, ra[i].w, o);
#pragma unroll
            for (int p = 0; p < kPlanes; ++p) *reinterpret_cast<uint2*>(&sA[p][(tid >> 3) + 32 * i][kq]) = o[p];
        }
#pragma unroll
        for (int p = 0; p < kPlanes; ++p)
#pragma unroll
            for (int i = 0; i < BV; ++i) {
                const int e = tid + i * 256;
                *reinterpret_cast<uint4*>(&sB[p][e >> 2][(e & 3) * 8]) = rb[p][i];
            }
    };

    f32x16 acc[TM][TN];
    bf16_acc_zero(acc);
    TapStep32 s{next_tap(0), 0};
    if (s.t < T) load_tiles(s);
    while (s.t < T) {   // workgroup-uniform
        store_tiles();
        __syncthreads();
        s = next_step(s);
        if (s.t < T) load_tiles(s);
        bf16_mfma_step<TM, TN>(sA, sB, wm, wn, lane, acc);
        __syncthreads();
    }

    // C/D map of the 32x32 MFMA: col = lane & 31, row = (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5); a row is an input pixel of the phase
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int r = r0 + (wm * TM + i) * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
            if (r >= rows) continue;
            const int n = r / HWp, rem = r - n * HWp;
            const int hh = rem / Wp, ww = rem - hh * Wp;
            float* dst = gx + (((int64_t)n * g.H + ph + hh * g.sh) * g.W + pw + ww * g.sw) * Cin;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int col = n0 + (wn * TN + j) * 32 + (lane & 31);
                if (col < Cin) dst[col] = acc[i][j][q] * scale;
            }
        }
}

// planes[p][tap][ci][k] = piece p of wq[k][ci][tap] as bf16, k < copad (zeros from c_out on).  As k_wq_planes, per tap: a workgroup
// transposes a tile of 32 k x 32 ci through LDS and writes 16-byte chunks of 64-byte rows.  The reads are T floats apart; the T
// workgroups that share their cache lines are neighbours in the grid (blockIdx.x = ci tile * T + tap).
__global__ __launch_bounds__(256) void k_wq_tap_planes(const float* __restrict__ wq, uint16_t* __restrict__ planes, int Cout, int Cin,
                                                        int T, int copad) {
    __shared__ __attribute__((aligned(16))) uint16_t tile[kPlanes][32][kPitch];   // [plane][ci][k]
    const int tap = blockIdx.x % T, ci0 = (blockIdx.x / T) * 32, k0 = blockIdx.y * 32;
    const int c = threadIdx.x & 31;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = (threadIdx.x >> 5) + 8 * i;
        const bool ok = k0 + r < Cout && ci0 + c < Cin;
        const float v = wq[ok ? ((int64_t)(k0 + r) * Cin + ci0 + c) * T + tap : 0];
        uint32_t b[3];
        split3(ok ? v : 0.f, b[0], b[1], b[2]);
#pragma unroll
        for (int p = 0; p < kPlanes; ++p) tile[p][c][r] = (uint16_t)(b[p] >> 16);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < kPlanes * 32 * 4; e += 256) {   // 16-byte chunks: (plane, ci, quarter of the 32 k)
        const int p = e >> 7, cc = (e >> 2) & 31, q = e & 3;
        if (ci0 + cc < Cin)   // k0 + 31 < copad
            *reinterpret_cast<uint4*>(planes + (((int64_t)p * T + tap) * Cin + ci0 + cc) * copad + k0 + q * 8) =
                *reinterpret_cast<const uint4*>(&tile[p][cc][q * 8]);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------
// What the launch is sized by.  A function of the descriptor only.
struct DnbShape {
    int64_t M;        // rows of the gw contraction = N*Ho*Wo
    int64_t ncol;     // gw GEMM columns = taps * C_in
    int T;            // taps
    int tn_x;         // gx tiling (TM = 2)
    int tm_w, tn_w;   // gw tiling
    int copad;        // k pitch of a tap's run in the WQ planes
    int splits, kps;  // gw split of M (gw_split)
};

static DnbShape dnb_shape(const slfp_conv2d_desc& d, const ConvPlan& p) {
    DnbShape s;
    s.M = d.n * p.h_out * p.w_out;
    s.T = (int)(d.kh * d.kw);
    s.ncol = (int64_t)s.T * d.c_in;
    s.tn_x = d.c_in >= 128 ? 2 : 1;
    s.tm_w = d.c_out >= 128 ? 2 : 1; s.tn_w = s.ncol >= 128 ? 2 : 1;
    s.copad = (int)(ceil_div(d.c_out, kBK) * kBK);
    const GwSplit sp = gw_split(s.M, d.c_out, s.ncol, ceil_div(d.c_out, 64 * s.tm_w) * ceil_div(s.ncol, 64 * s.tn_w));
    s.splits = sp.splits; s.kps = sp.kps;
    return s;
}

// The layers the kernels take, whichever way x arrives (what the workspace is sized for): 0 and the reason in slfp_last_error, or 1.
// No geometry class is refused for its speed: every measured layer beat the float32 dense kernels beyond the spread (DESIGN.md
// section 45, profiles/backward_dense_bf16_bench.json).
static int dnb_layer_ok(const slfp_conv2d_desc* d, const ConvPlan& p, unsigned flags) {
    auto no = [](const char* why) { fail(SLFP_ERR_UNSUPPORTED, "slfp_conv2d_bwd_dense_bf16: %s", why); return 0; };
    if (bwd_is_pw(*d)) return no("a stride-1 1x1 layer is the pw family: slfp_conv2d_bwd_bf16");
    if (d->groups != 1) return no("depthwise and grouped layers stay on slfp_conv2d_bwd_ex");
    if (!(flags & SLFP_BWD_DENSE)) return no("the dense family is taken under SLFP_BWD_DENSE only");
    if (!bwd_is_dense(*d, p, flags)) return no("not a dense layer of slfp_conv2d_bwd_ex (dilation 1, its 32-bit limits)");
    if (d->x_layout != SLFP_LAYOUT_NHWC || d->y_layout != SLFP_LAYOUT_NHWC) return no("NHWC only");
    if (d->c_in % 8 != 0 || d->c_out % 8 != 0) return no("C_in and C_out must be multiples of 8");
    // one k-step past the last row stays in 32 bits; the grids' y extents
    if (d->n * p.h_out * p.w_out >= 0x7FFFFF00 || d->kh * d->kw * d->c_in > (int64_t)65535 * 64 || d->c_out > (int64_t)65535 * 32)
        return no("N*Ho*Wo must stay below 2^31 - 256, taps * C_in within 65535 * 64, C_out within 65535 * 32");
    return 1;
}

// ... and this operand form: float32 x needs the threshold table (codes are decoded, not encoded)
static int dnb_supported(const slfp_conv2d_desc* d, const ConvPlan& p, unsigned flags, bool x_codes) {
    if (!dnb_layer_ok(d, p, flags)) return 0;
    if (!x_codes && !act_table(d->ka, p.fmt_act, kEncF32)) {
        fail(SLFP_ERR_UNSUPPORTED, "slfp_conv2d_bwd_dense_bf16: no threshold table for this Ka (float32 x)");
        return 0;
    }
    return 1;
}

struct DnbLayout {  // byte offsets into the workspace
    size_t wq, planes, part, gbpart, total;
};

static DnbLayout dnb_layout(const slfp_conv2d_desc& d, const DnbShape& s, bool need_gx, bool need_gw) {
    DnbLayout L;
    size_t off = 0;
    L.wq = off; if (need_gx) off += r256((size_t)d.c_out * s.ncol * sizeof(float));
    L.planes = off; if (need_gx) off += r256((size_t)kPlanes * s.ncol * s.copad * sizeof(uint16_t));
    L.part = off; if (need_gw) off += r256((size_t)s.splits * d.c_out * s.ncol * sizeof(float));   // [split][co][tap][ci], reduced into OIHW
    L.gbpart = off; if (need_gw) off += r256((size_t)s.splits * d.c_out * sizeof(float));
    L.total = off;
    return L;
}

}  // namespace slfp

using namespace slfp;

extern "C" {

int slfp_conv2d_bwd_dense_bf16_supported(const slfp_conv2d_desc* d, unsigned flags, int x_codes) {
    ConvPlan p;
    if (!d || (flags & ~SLFP_BWD_DENSE) || make_plan(d, &p) != SLFP_OK) return 0;
    return dnb_supported(d, p, flags, x_codes != 0);
}

size_t slfp_conv2d_bwd_dense_bf16_workspace_bytes(const slfp_conv2d_desc* d, unsigned flags, int need_gx, int need_gw) {
    ConvPlan p;
    if (!d || (flags & ~SLFP_BWD_DENSE) || make_plan(d, &p) != SLFP_OK || !dnb_layer_ok(d, p, flags)) return 0;   // the same for x and x_codes
    return dnb_layout(*d, dnb_shape(*d, p), need_gx != 0, need_gw != 0).total;
}

const char* slfp_debug_bwd_dense_bf16_instance(const slfp_conv2d_desc* d, unsigned flags, int x_codes, int need_gx, int need_gw) {
    static thread_local char buf[160];
    ConvPlan p;
    if (!d || (flags & ~SLFP_BWD_DENSE) || make_plan(d, &p) != SLFP_OK || !dnb_supported(d, p, flags, x_codes != 0)) return "none";
    if (!need_gx && !need_gw) return "none";
    const DnbShape s = dnb_shape(*d, p);
    int n = 0;
    if (need_gx) n += std::snprintf(buf + n, sizeof buf - n, "dnb/gx/tn%d/t6", s.tn_x);
    if (need_gw)
        std::snprintf(buf + n, sizeof buf - n, "%sdnb/gw/tm%dtn%d/t6/%s/p%dk%d", n ? "+" : "", s.tm_w, s.tn_w, x_codes ? "codes" : "tab",
                      s.splits, s.kps);
    return buf;
}

int slfp_conv2d_bwd_dense_bf16(const slfp_conv2d_desc* d, unsigned flags, const float* x, const uint8_t* x_codes, const float* w_oihw,
                               const float* gy, float* gx, float* gw_oihw, float* gb, void* workspace, void* stream) {
    if (!d) return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd_dense_bf16: null descriptor");
    if (flags & ~SLFP_BWD_DENSE) return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd_dense_bf16: unknown flag bits 0x%x", flags & ~SLFP_BWD_DENSE);
    if ((x != nullptr) == (x_codes != nullptr)) return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd_dense_bf16: exactly one of x and x_codes");
    if ((x && !aligned16(x)) || (w_oihw && !aligned16(w_oihw)) || (gy && !aligned16(gy)) || (gx && !aligned16(gx)) ||
        (gw_oihw && !aligned16(gw_oihw)) || (gb && !aligned16(gb)))
        return fail(SLFP_ERR_ALIGNMENT, "slfp_conv2d_bwd_dense_bf16: tensors must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(x_codes) & 3) return fail(SLFP_ERR_ALIGNMENT, "slfp_conv2d_bwd_dense_bf16: x_codes must be 4-byte aligned");
    ConvPlan p;
    int rc = make_plan(d, &p);
    if (rc != SLFP_OK) return rc;
    const bool codes = x_codes != nullptr;
    if (!dnb_supported(d, p, flags, codes)) return SLFP_ERR_UNSUPPORTED;   // the reason is recorded
    if (!gy) return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd_dense_bf16: null gy");
    if (gx && !w_oihw) return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd_dense_bf16: gx needs the weights");
    if (gb && !gw_oihw) return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd_dense_bf16: gb is computed together with gw");
    const bool need_gx = gx != nullptr, need_gw = gw_oihw != nullptr;
    if (!need_gx && !need_gw) return SLFP_OK;
    const DnbShape s = dnb_shape(*d, p);
    const DnbLayout L = dnb_layout(*d, s, need_gx, need_gw);
    if (L.total && (!workspace || !aligned16(workspace)))
        return fail(SLFP_ERR_BAD_ARG, "slfp_conv2d_bwd_dense_bf16: %zu bytes of 16-byte aligned workspace required (slfp_conv2d_bwd_dense_bf16_workspace_bytes)", L.total);
    unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
    hipStream_t st = as_stream(stream);
    const DenseGeom g = dense_geom(*d, p);
    const int Cin = g.Cin, Cout = g.Cout;

    if (need_gx) {
        float* wq = reinterpret_cast<float*>(ws + L.wq);
        uint16_t* planes = reinterpret_cast<uint16_t*>(ws + L.planes);
        if ((rc = launch_quantize(w_oihw, wq, (size_t)Cout * s.ncol, d->kw_scale, p.fmt_w, st)) != SLFP_OK) return rc;
        hipLaunchKernelGGL(k_wq_tap_planes, dim3((unsigned)(ceil_div(Cin, 32) * s.T), (unsigned)(s.copad / 32)), dim3(256), 0, st, wq, planes,
                           Cout, Cin, s.T, s.copad);
        if ((rc = check_launch("slfp bf16 dense backward weight planes kernel")) != SLFP_OK) return rc;
        const dim3 grid((unsigned)dense_gx_tiles(g), (unsigned)ceil_div(Cin, 64 * s.tn_x));
        bf16_1_or_2(s.tn_x, [&](auto TN) {
            hipLaunchKernelGGL((k_dense_gx_bf16<decltype(TN)::value>), grid, dim3(256), 0, st, gy, planes, gx, g, s.copad, d->kw_scale);
        });
        if ((rc = check_launch("slfp bf16 dense backward (gx) kernel")) != SLFP_OK) return rc;
    }
    if (need_gw) {
        float* part = reinterpret_cast<float*>(ws + L.part);
        float* gbp = reinterpret_cast<float*>(ws + L.gbpart);
        Bf16DenseArgs a;
        a.gy = gy; a.b = codes ? (const void*)x_codes : (const void*)x; a.C = part; a.gbpart = gb ? gbp : nullptr;
        a.M = Cout; a.N = (int)s.ncol; a.K = (int)s.M; a.kpad = 0; a.kps = s.kps; a.scale = 1.0f;
        a.g = g;
        launch_bf16_gw(a, s.tm_w, s.tn_w, st, codes, p.fmt_act, act_table(d->ka, p.fmt_act, kEncF32));
        if ((rc = check_launch("slfp bf16 dense backward (gw) kernel")) != SLFP_OK) return rc;
        if ((rc = reduce_parts(st, part, s.splits, (int64_t)Cout * s.ncol, d->ka, 0, Cin, s.T, gw_oihw, nullptr)) != SLFP_OK) return rc;
        if (gb && (rc = reduce_gb(st, gbp, s.splits, Cout, gb)) != SLFP_OK) return rc;
    }
    return SLFP_OK;
}

}  // extern "C"
