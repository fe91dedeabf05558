// bn_train.hip -- training-mode BatchNorm2d (+ReLU), forward and backward, float32 NHWC (gfx950, wave64).
//
// nn.BatchNorm2d behind every Conv2d_Q, mostly followed by nn.ReLU(inplace=True) (nets_cifar/mobilenetv1.py:30-45,
// nets_imgnet/mobilenetv1.py:24-41).  x is [M][C] with M = N H W rows; a channel's statistics are sums over a column.  No
// atomics: every result is a pure function of the inputs and of (M, C), and the orders below are the contract of
// include/slfp.h.  The library is built with -ffp-contract=off and without fast-math, so the compiler neither fuses nor
// reassociates any of it.
//
// Geometry (bn_split, a pure function of (M, C)): V = 4 channels per lane (16-byte accesses) if C % 4 == 0, else V = 1.  A
// workgroup is 256 lanes = TX column lanes x TY row lanes, TX the power of two >= min(C / V, 64); it owns one slab of R rows
// (the last slab ragged) and one tile of TX V channels.  Lane (tx, ty) walks rows r0 + ty, r0 + ty + TY, ... of its slab.
//   k_bn_stats         per lane and channel, from +0.0f, rows ascending: d = x - k; s1 = s1 + d; s2 = s2 + d * d, with k the
//                      channel's value in the slab's first row (8 loads issued ahead of their adds).  The TY lane partials meet in
//                      LDS and are added ty = 0, 1, ..., TY - 1.  One (count, k, s1, s2) record per (slab, channel).
//   k_bn_finalize      float64: mean_b = k + s1 / n_b, M2_b = s2 - s1 s1 / n_b per slab, then Chan's update in slab order:
//                      delta = mean_b - mean; mean = mean + delta (n_b / n); M2 = (M2 + M2_b) + (delta delta) (n_a n_b / n).
//                      var = max(M2 / M, 0); save_mean = f32(mean), save_invstd = f32(1 / sqrt(var + eps)), running statistics
//                      in place;
//                      lo = f32(mean - save_mean), the part of the mean float32 cannot hold, goes to the workspace.
//   k_bn_apply         sc = invstd * gamma;  y = (((x - save_mean) - lo) * sc) + beta;  relu: y < 0 ? 0 : y  (a NaN stays a
//                      NaN).  x - save_mean is exact where x is within a factor 2 of the mean, so y keeps float32 accuracy
//                      relative to the CENTRED value even where |mean| >> sigma.
//   k_bn_bwd_reduce    g = relu ? (y > 0 ? gy : 0) : gy;  d = x - save_mean;  sg = sg + g;  sx = sx + g * (d * invstd);  sd = sd + d;
//                      the same lane walk and LDS order as k_bn_stats (4 rows of loads ahead).  One (sg, sx, sd) per (slab,
//                      channel).  The backward is handed the float32 save_mean alone; sd gives it back what that rounding lost.
//   k_bn_bwd_finalize  float64 sums in slab order: SG, SX, SD;  lo = SD / M;  SX = SX - (lo * invstd) * SG  (the sum of g xh for
//                      xh = ((x - save_mean) - lo) * invstd);  gbeta = f32(SG), ggamma = f32(SX), and for the last pass
//                      mb = f32(SG / M), mg = f32(SX / M), f32(lo)
//   k_bn_bwd_dx        a = gamma * invstd;  xh = ((x - save_mean) - lo) * invstd;  gx = a * ((g - mb) - (xh * mg))
// The LUT forms (k_bn_apply, k_bn_bwd_reduce, k_bn_bwd_dx with LUT = true; slfp_bn_lut_train_fwd / _bwd) put the layer-output
// quantizer and the activation behind it into the same passes, for the training blocks [Conv2d_Q, BatchNorm2d,
// layerout_quantize_func, ReLU | Swish | GELU].  After the quantizer a value is one of kLayeroutClasses, so the activation is a
// float32 table over the class (act_table) and its derivative another (dact_table):
//   forward    t = the apply above with relu = 0;  y = act_table[layerout_class(layerout_bits(t))]
//   backward   the class is recomputed from x with the forward's own expression (save_lo is the forward's lo, handed over
//              bit for bit);  g = gy * dact_table[class]  (the quantizer is a straight-through estimator);  the rest as above.
// Each workgroup copies its table (19 712 B) into LDS once; a lookup is one ds_read_b32 at a random address.
// The residual forms (k_bn_apply, k_bn_bwd_dx with RES = true, never with LUT; slfp_bn_res_train_fwd / _bwd) carry the tail of a
// Bottleneck, out = bn3(out); out += identity; out = relu(out) (nets_imgnet/resnet50.py:85-90), in the same passes:
//   forward    t = the apply above with relu = 0;  z = t + res;  relu: y = z < 0 ? 0 : z  (a NaN stays a NaN)
//   backward   g as above, the mask read from y;  gx as above;  gres = g, a second store of the dx pass (skipped when NULL)
// The statistics, both finalize kernels and the reduce pass are the plain ones.
// The code forms (k_bn_apply_codes; k_bn_bwd_reduce, k_bn_bwd_dx with XM = true; slfp_bn_codes_train_fwd / _bwd) hand y to the
// next Conv2d_Q as the 1-byte extended codes of that layer's own quantizer (slfp_codes.hpp), C % 4 == 0:
//   forward    t = the apply above (with its ReLU);  a lane's four channels go through enc4_code_relu (behind a ReLU) or
//              enc4_code_fmt<FMT, true> on the reader's kEncCode table in LDS and leave as one dword;  lo goes to save_lo
//   backward   the ReLU's mask is t > 0 with t recomputed from x through bn_affine (y > 0 exactly where t > 0): no forward output
//              is read;  the rest as the plain form
// The residual-and-codes form (k_bn_apply_res_codes; slfp_bn_res_codes_train_fwd) is the residual forward with a second store: the
// float32 trunk y as the residual form stores it and, next to it, y as the extended codes of the Conv2d_Q layers that read the
// trunk, the four channels of a lane as one dword exactly as the code form stores them (behind the ReLU enc4_code_relu, else
// enc4_code_fmt<FMT, true>).  One pass over x and res, the code form's one barrier (the table); its backward is the residual form's.
// The table-and-codes form (k_bn_apply_lut_codes; slfp_bn_lut_codes_train_fwd) is the LUT forward with the reader's quantizer folded
// into the table: behind the layer-output quantizer, act and the next Conv2d_Q's quantize_act(. / Ka) are ONE byte per class
// (code_table, SLFP_LAYEROUT_LUT_BYTES bytes, built by the caller), C % 4 == 0:
//   forward    t and the class as the LUT form;  byte = code_table[class];  a lane's four bytes leave as one dword, as the code form
//              stores them;  no float32 y is written.  Only the byte table is in LDS (4 928 B, not the float table's 19 712 B).
//   backward   slfp_bn_lut_train_bwd as it is: it recomputes the class from x and reads no forward output.
// The two finalize kernels stage the records of 256 slabs x 8 channels in LDS with all 256 lanes (and the per-slab weights
// n_b / n and n_a n_b / n, which depend on the slab index alone), then one lane per channel runs the serial chain.
// Each of these is written once: bn_walk is the lane's walk over its rows (all five streaming kernels), bn_affine the apply's
// expression (the apply of every form, and through bn_class the backward's recomputed class), bn_g the g of one element
// (reduce, dx and the gres store), bn_forward / bn_backward the refusals and the three launches of a direction; the ten entry
// points state their pointers and the refusals of their own form.
#include "slfp_device.hpp"
#include "slfp_enc.hpp"
#include "slfp_codes.hpp"
#include "slfp_host.hpp"
#include "slfp_layerout_lut.hpp"

#include <algorithm>

namespace slfp {

constexpr int kBnThreads = 256;
constexpr int kBnTargetWgs = 512;    // two workgroups per CU on 256 CUs
constexpr int kBnMaxSlabs = 1024;
constexpr int kBnFinCh = 8;          // channels per finalize workgroup
constexpr int kBnFinChunk = 256;     // slabs staged in LDS at a time
constexpr int kBnTableFloats = SLFP_LAYEROUT_TABLE_FLOATS;   // one float32 per layer-output class, padded
static_assert(kBnTableFloats % 4 == 0 && kBnTableFloats >= kLayeroutClasses, "the table is copied 16 bytes at a time");

struct BnSplit {
    int64_t rows, slabs;   // R, S: R (S - 1) < M <= R S
    int64_t tiles;         // channel tiles of TX V channels
    int tx_log2, vec;
};

// The cut of [M][C] into workgroups: a pure function of (M, C).
static BnSplit bn_split(int64_t M, int64_t C) {
    BnSplit s;
    s.vec = C % 4 == 0 ? 4 : 1;
    const int64_t groups = C / s.vec;
    int lg = 0;
    while (lg < 6 && ((int64_t)1 << lg) < groups) ++lg;
    s.tx_log2 = lg;
    const int64_t tx = (int64_t)1 << lg, ty = kBnThreads / tx;
    s.tiles = ceil_div(groups, tx);
    int64_t want = std::max<int64_t>(1, kBnTargetWgs / s.tiles);
    want = std::min<int64_t>(want, kBnMaxSlabs);
    want = std::min<int64_t>(want, std::max<int64_t>(1, M / (4 * ty)));   // at least 4 rows per lane
    s.rows = ceil_div(M, want);
    s.slabs = ceil_div(M, s.rows);
    return s;
}

static bool bn_supported(int64_t n, int64_t h, int64_t w, int64_t c, int x_layout) {
    if (n < 0 || h < 1 || w < 1 || c < 1 || x_layout != SLFP_LAYOUT_NHWC) return false;
    if (h > 0x7FFFFFFF || w > 0x7FFFFFFF || h * w > 0x7FFFFFFF || c > (1 << 21)) return false;   // grid.y: at most 32768 tiles
    if (n > 0x7FFFFFFF / (h * w)) return false;   // M fits 31 bits (the record's count)
    return n == 0 || n * h * w > 1;               // one value per channel has no variance
}

static size_t bn_gmean_offset(const BnSplit& s, int64_t c) { return (size_t)s.slabs * (size_t)c * sizeof(float4); }

static size_t bn_workspace_bytes(int64_t m, int64_t c) {
    if (m < 1) return 0;
    const BnSplit s = bn_split(m, c);
    // S C records of 16 bytes in either direction; behind them C floats (lo) in the forward, 3 C floats (mb, mg, lo) in the backward
    const size_t bytes = bn_gmean_offset(s, c) + 3 * (size_t)c * sizeof(float);
    return (bytes + 255) & ~(size_t)255;
}

struct BnArgs {
    const float* x;
    const float* y;        // backward: the forward's output (the ReLU mask)
    const float* gy;
    float* out;            // forward: y; backward: gx
    const float* gamma;
    const float* beta;
    const float* mean;
    const float* invstd;
    float4* rec;           // forward workspace: [S][C] (count bits, k, s1, s2)
    float4* part;          // backward workspace: [S][C] (sg, sx, sd, 0)
    float* gmean;          // workspace behind the records: backward [3][C] mb, mg, lo; forward [C] lo = f32(mean - save_mean)
    const float* lo_fwd;   // LUT backward: the forward's lo (save_lo)
    const float* table;    // LUT forms: act_table (forward) / dact_table (backward), kBnTableFloats floats; the table-and-codes
                           // forward: the reader's byte table over the class (bn_code_lds reads it as bytes)
    const float* res;      // residual forward: the operand added behind the affine map
    float* gres;           // residual backward: the residual's gradient g, or null
    uint8_t* codes;        // code forward: y as the reader's extended codes, [M][C] bytes
    int code_fmt;          // code forward: kFmtAct8 | kFmtSfp7, the format of those codes
    int64_t m, c, rows;
    int slabs, tx_log2, relu;
};

template <int V> struct alignas(4 * V) Pack { float v[V]; };

template <int V> __device__ __forceinline__ Pack<V> bn_ld(const float* p) {
    Pack<V> r;
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
    } else {
        r.v[0] = *p;
    }
    return r;
}

template <int V> __device__ __forceinline__ void bn_st(float* p, const Pack<V>& r) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else *p = r.v[0];
}

template <int V> __device__ __forceinline__ Pack<V> bn_fill(float f) {
    Pack<V> r;
#pragma unroll
    for (int e = 0; e < V; ++e) r.v[e] = f;
    return r;
}

// LUT forms: the workgroup's copy of the table in LDS, published by the barrier (every lane of the workgroup calls this).  The
// plain forms get no LDS and a null pointer they never read.
template <bool LUT> __device__ __forceinline__ const float* bn_table_lds(const float* g) {
    if constexpr (LUT) {
        __shared__ __attribute__((aligned(16))) float sTab[kBnTableFloats];
        for (int i = threadIdx.x; i < kBnTableFloats / 4; i += kBnThreads)
            reinterpret_cast<float4*>(sTab)[i] = reinterpret_cast<const float4*>(g)[i];
        __syncthreads();
        return sTab;
    } else {
        return nullptr;
    }
}

// Code forms: the workgroup's copy of the reader's kEncCode threshold table in LDS, published by the barrier (every lane calls this).
template <bool CODES> __device__ __forceinline__ const unsigned char* bn_enc_lds(const EncArgs* enc) {
    if constexpr (CODES) {
        __shared__ __attribute__((aligned(16))) uint2 sEnc[kEncEntries + 1];
        enc_fill<kBnThreads>(sEnc, *enc);
        __syncthreads();
        return reinterpret_cast<const unsigned char*>(sEnc);
    } else {
        return nullptr;
    }
}

// Table-and-codes form: the workgroup's copy of the reader's byte table over the layer-output class in LDS (308 pieces of 16
// bytes), published by the barrier (every lane calls this).
template <bool ON> __device__ __forceinline__ const uint8_t* bn_code_lds(const void* g) {
    if constexpr (ON) {
        static_assert(SLFP_LAYEROUT_LUT_BYTES % 16 == 0 && SLFP_LAYEROUT_LUT_BYTES >= kLayeroutClasses, "copied 16 bytes at a time");
        __shared__ __attribute__((aligned(16))) uint8_t sCode[SLFP_LAYEROUT_LUT_BYTES];
        for (int i = threadIdx.x; i < SLFP_LAYEROUT_LUT_BYTES / 16; i += kBnThreads)
            reinterpret_cast<uint4*>(sCode)[i] = reinterpret_cast<const uint4*>(g)[i];
        __syncthreads();
        return sCode;
    } else {
        return nullptr;
    }
}

// The forward's affine map of a lane's V channels: sc = invstd * gamma; lo is f32(mean - save_mean)
template <int V> struct BnMap { Pack<V> mean, lo, sc, beta; };

// The apply's expression, channel e of the lane.  The backward of the LUT forms recomputes the class through this very function.
template <int V> __device__ __forceinline__ float bn_affine(const float x, const BnMap<V>& m, const int e) {
    return (((x - m.mean.v[e]) - m.lo.v[e]) * m.sc.v[e]) + m.beta.v[e];
}

// LUT forms: the class of one element
template <int V> __device__ __forceinline__ uint32_t bn_class(const float x, const BnMap<V>& m, const int e) {
    return layerout_class(layerout_bits(__float_as_uint(bn_affine<V>(x, m, e))));
}

// Where a lane stands: its first channel, whether that channel exists, its rows [first, r1) with stride nty.
template <int V> struct BnLane {
    int tx, ty, nty;
    int64_t ch, r0, r1, first;
    bool live;
    __device__ __forceinline__ explicit BnLane(const BnArgs& a) {
        tx = threadIdx.x & ((1 << a.tx_log2) - 1);
        ty = threadIdx.x >> a.tx_log2;
        nty = kBnThreads >> a.tx_log2;
        ch = (((int64_t)blockIdx.y << a.tx_log2) + tx) * V;
        live = ch < a.c;
        r0 = (int64_t)blockIdx.x * a.rows;
        r1 = r0 + a.rows < a.m ? r0 + a.rows : a.m;
        first = live ? r0 + ty : r1;   // lanes past C walk no rows; they still meet the barriers
    }
};

// The TY lane partials of a channel group, added ty = 0, 1, ..., TY - 1 by the ty == 0 lane.
template <int V, int K> __device__ __forceinline__ void bn_meet(Pack<V> (&p)[K], const BnLane<V>& l, const int tx_log2) {
    __shared__ Pack<V> sp[K][kBnThreads];
#pragma unroll
    for (int i = 0; i < K; ++i) sp[i][threadIdx.x] = p[i];
    __syncthreads();
    if (l.ty != 0) return;
    for (int j = 1; j < l.nty; ++j) {
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const Pack<V> pj = sp[i][(j << tx_log2) + l.tx];
#pragma unroll
            for (int e = 0; e < V; ++e) p[i].v[e] = p[i].v[e] + pj.v[e];
        }
    }
}

// What a lane loads of one row: N operands of V channels each
template <int V, int N> struct BnRow { Pack<V> p[N]; };

// A lane's walk over rows r, r + st, ... < end of pitch ld: load(offset) of AHEAD rows are all issued before use(offset, row)
// of the first of them; then a one-row tail.  The uses run in row order.
template <int AHEAD, class Load, class Use>
__device__ __forceinline__ void bn_walk(int64_t r, const int64_t end, const int64_t st, const size_t ld, Load load, Use use) {
    for (; r + (AHEAD - 1) * st < end; r += AHEAD * st) {
        decltype(load((size_t)0)) b[AHEAD];
#pragma unroll
        for (int i = 0; i < AHEAD; ++i) b[i] = load((size_t)(r + i * st) * ld);
#pragma unroll
        for (int i = 0; i < AHEAD; ++i) use((size_t)(r + i * st) * ld, b[i]);
    }
    for (; r < end; r += st) {
        const size_t o = (size_t)r * ld;
        use(o, load(o));
    }
}

template <int V> __device__ __forceinline__ void bn_stat_add(Pack<V> (&s)[2], const Pack<V>& v, const Pack<V>& k) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const float d = v.v[e] - k.v[e];
        s[0].v[e] = s[0].v[e] + d;
        s[1].v[e] = s[1].v[e] + d * d;
    }
}

template <int V>
__global__ __launch_bounds__(kBnThreads) void k_bn_stats(const BnArgs a) {
    const BnLane<V> l(a);
    const size_t ld = (size_t)a.c;
    const float* px = a.x + (l.live ? l.ch : 0);
    const Pack<V> k = l.live ? bn_ld<V>(px + (size_t)l.r0 * ld) : bn_fill<V>(0.f);
    Pack<V> s[2] = {bn_fill<V>(0.f), bn_fill<V>(0.f)};   // s1, s2
    // eight loads ahead of the adds of this lane's one chain per channel
    bn_walk<8>(l.first, l.r1, l.nty, ld, [&](const size_t o) { return BnRow<V, 1>{{bn_ld<V>(px + o)}}; },
               [&](const size_t, const BnRow<V, 1>& b) { bn_stat_add<V>(s, b.p[0], k); });
    bn_meet<V, 2>(s, l, a.tx_log2);
    if (l.ty != 0 || !l.live) return;
    const float cnt = __int_as_float((int)(l.r1 - l.r0));
    float4* rec = a.rec + (size_t)blockIdx.x * ld + (size_t)l.ch;
#pragma unroll
    for (int e = 0; e < V; ++e) rec[e] = make_float4(cnt, k.v[e], s[0].v[e], s[1].v[e]);
}

// Stage of both finalize kernels: lane (cl, sl) of 8 x 32 owns channel c0 + cl and slabs sl, sl + 32, ... of the chunk.
struct BnFinLane {
    int cl, sl;
    int64_t c;
    bool live;
    __device__ __forceinline__ explicit BnFinLane(const BnArgs& a) {
        cl = threadIdx.x & (kBnFinCh - 1);
        sl = threadIdx.x / kBnFinCh;
        c = (int64_t)blockIdx.x * kBnFinCh + cl;
        live = c < a.c;
    }
};

__global__ __launch_bounds__(kBnThreads) void k_bn_finalize(const BnArgs a, float* running_mean, float* running_var,
                                                            const float momentum, const float eps, float* save_mean,
                                                            float* save_invstd) {
    __shared__ double smean[kBnFinChunk][kBnFinCh], sm2[kBnFinChunk][kBnFinCh], sw[kBnFinChunk], sq[kBnFinChunk];
    const BnFinLane l(a);
    double mean = 0.0, m2 = 0.0;
    for (int base = 0; base < a.slabs; base += kBnFinChunk) {
        const int lim = a.slabs - base < kBnFinChunk ? a.slabs - base : kBnFinChunk;
        for (int j = l.sl; j < lim; j += kBnThreads / kBnFinCh) {
            const int64_t slab = base + j;
            const double na = (double)(slab * a.rows);   // every slab in front of this one is full
            const double nb = (double)((slab + 1) * a.rows < a.m ? a.rows : a.m - slab * a.rows);
            const double nt = na + nb;
            if (l.cl == 0) { sw[j] = nb / nt; sq[j] = na * nb / nt; }
            if (l.live) {
                const float4 rec = a.rec[(size_t)slab * (size_t)a.c + (size_t)l.c];
                const double cnt = (double)__float_as_int(rec.x), s1 = (double)rec.z, s2 = (double)rec.w;
                smean[j][l.cl] = (double)rec.y + s1 / cnt;
                sm2[j][l.cl] = s2 - s1 * s1 / cnt;
            }
        }
        __syncthreads();
        if (l.sl == 0 && l.live) {
#pragma unroll 4
            for (int j = 0; j < lim; ++j) {
                const double delta = smean[j][l.cl] - mean;
                mean = mean + delta * sw[j];
                m2 = (m2 + sm2[j][l.cl]) + (delta * delta) * sq[j];
            }
        }
        __syncthreads();
    }
    if (l.sl != 0 || !l.live) return;
    const double cnt = (double)a.m;
    double var = m2 / cnt;
    var = var < 0.0 ? 0.0 : var;   // rounding can leave M2 of a constant channel a hair below 0; a NaN stays a NaN
    const float mean_hi = (float)mean;
    save_mean[l.c] = mean_hi;
    a.gmean[l.c] = (float)(mean - (double)mean_hi);
    save_invstd[l.c] = (float)(1.0 / sqrt(var + (double)eps));
    const double mo = (double)momentum;
    if (running_mean) running_mean[l.c] = (float)((1.0 - mo) * (double)running_mean[l.c] + mo * mean);
    if (running_var) running_var[l.c] = (float)((1.0 - mo) * (double)running_var[l.c] + mo * (var * cnt / (cnt - 1.0)));
}

// The apply pass of every form.  CODES (V == 4) without LUT: `enc` is the reader's kEncCode table, copied to LDS.  RES && CODES
// stores both: the float32 pack of the residual form and the dword of the code form, of the same y.  LUT && CODES: a.table is
// the reader's byte table over the class, the only table in LDS; `enc` is null and no float32 is stored.
template <int V, bool LUT, bool RES, bool CODES>
__device__ __forceinline__ void bn_apply(const BnArgs& a, const EncArgs* enc) {
    static_assert(!(LUT && RES), "the residual form has no table");
    static_assert(!CODES || V == 4, "codes leave four channels to a dword");
    const BnLane<V> l(a);
    const float* const sTab = bn_table_lds<LUT && !CODES>(a.table);
    const unsigned char* const sE = bn_enc_lds<CODES && !LUT>(enc);
    const uint8_t* const sCode = bn_code_lds<LUT && CODES>(a.table);
    if (!l.live) return;
    const size_t ld = (size_t)a.c;
    BnMap<V> map = {bn_ld<V>(a.mean + l.ch), bn_ld<V>(a.gmean + l.ch), bn_ld<V>(a.invstd + l.ch), bn_ld<V>(a.beta + l.ch)};
    const Pack<V> gamma = bn_ld<V>(a.gamma + l.ch);
#pragma unroll
    for (int e = 0; e < V; ++e) map.sc.v[e] = map.sc.v[e] * gamma.v[e];
    const float* px = a.x + l.ch;
    const float* pr = RES ? a.res + l.ch : nullptr;
    float* py = CODES && !RES ? nullptr : a.out + l.ch;
    const int relu = a.relu;
    constexpr int N = RES ? 2 : 1;
    bn_walk<4>(l.first, l.r1, l.nty, ld,
               [&](const size_t o) {
                   BnRow<V, N> b;
                   b.p[0] = bn_ld<V>(px + o);
                   if constexpr (RES) b.p[1] = bn_ld<V>(pr + o);
                   return b;
               },
               [&](const size_t o, const BnRow<V, N>& b) {
                   if constexpr (LUT && CODES) {
                       // whole-register shifts and ors: no sub-dword VALU write in front of the store
                       uint32_t d = 0;
#pragma unroll
                       for (int e = 0; e < V; ++e) d = d | ((uint32_t)sCode[bn_class<V>(b.p[0].v[e], map, e)] << (8 * e));
                       *reinterpret_cast<uint32_t*>(a.codes + o + (size_t)l.ch) = d;
                       return;
                   }
                   Pack<V> v;
#pragma unroll
                   for (int e = 0; e < V; ++e) {
                       if constexpr (LUT) {
                           v.v[e] = sTab[bn_class<V>(b.p[0].v[e], map, e)];
                       } else {
                           float t = bn_affine<V>(b.p[0].v[e], map, e);
                           if constexpr (RES) t = t + b.p[1].v[e];   // the add is rounded on its own, the ReLU comes behind it
                           if constexpr (!CODES || RES) {   // codes alone: the code quantizers fold the ReLU (enc4_code_relu)
                               if (relu) t = t < 0.f ? 0.f : t;
                           }
                           v.v[e] = t;
                       }
                   }
                   if constexpr (CODES && !LUT) {
                       const float4 t4 = make_float4(v.v[0], v.v[1], v.v[2], v.v[3]);
                       const float r1 = enc->r1, lo = enc->lo, hi = enc->hi;
                       const uint32_t d = relu ? enc4_code_relu<>(t4, r1, lo, hi, sE)
                                               : (a.code_fmt == kFmtSfp7 ? enc4_code_fmt<kFmtSfp7, true>(t4, r1, lo, hi, sE)
                                                                         : enc4_code_fmt<kFmtAct8, true>(t4, r1, lo, hi, sE));
                       *reinterpret_cast<uint32_t*>(a.codes + o + (size_t)l.ch) = d;
                   }
                   if constexpr (!CODES || RES) bn_st<V>(py + o, v);
               });
}

template <int V, bool LUT = false, bool RES = false>
__global__ __launch_bounds__(kBnThreads) void k_bn_apply(const BnArgs a) {
    bn_apply<V, LUT, RES, false>(a, nullptr);
}

__global__ __launch_bounds__(kBnThreads) void k_bn_apply_codes(const BnArgs a, const EncArgs enc) {
    bn_apply<4, false, false, true>(a, &enc);
}

__global__ __launch_bounds__(kBnThreads) void k_bn_apply_res_codes(const BnArgs a, const EncArgs enc) {
    bn_apply<4, false, true, true>(a, &enc);
}

__global__ __launch_bounds__(kBnThreads) void k_bn_apply_lut_codes(const BnArgs a) {
    bn_apply<4, true, false, true>(a, nullptr);
}

// What the backward loads of one row: x, gy and the forward's y (with relu only: otherwise y is never read; XM: never)
template <int V, bool XM = false>
__device__ __forceinline__ BnRow<V, 3> bn_ld_bwd(const float* px, const float* pg, const float* py, const size_t o, const int relu) {
    BnRow<V, 3> b;
    b.p[0] = bn_ld<V>(px + o);
    b.p[1] = bn_ld<V>(pg + o);
    if constexpr (XM) b.p[2] = b.p[1];
    else b.p[2] = relu ? bn_ld<V>(py + o) : b.p[1];
    return b;
}

// g of channel e of a row.  The ReLU's mask is read from the forward's own output; the LUT forms multiply by the derivative
// table at the class recomputed from x (map: the forward's own mean, lo, sc and beta).  XM (the code forms): the mask is t > 0 with
// t the forward's own expression of x, which holds exactly where the plain forward's y > 0 (a NaN is in neither).
template <int V, bool LUT, bool XM = false>
__device__ __forceinline__ float bn_g(const BnRow<V, 3>& b, const int e, const int relu, const float* sTab, const BnMap<V>& map) {
    const float gy = b.p[1].v[e];
    if constexpr (LUT) return gy * sTab[bn_class<V>(b.p[0].v[e], map, e)];
    else if constexpr (XM) return relu ? (bn_affine<V>(b.p[0].v[e], map, e) > 0.f ? gy : 0.f) : gy;
    else return relu ? (b.p[2].v[e] > 0.f ? gy : 0.f) : gy;
}

template <int V, bool LUT = false, bool XM = false>
__global__ __launch_bounds__(kBnThreads) void k_bn_bwd_reduce(const BnArgs a) {
    static_assert(!(LUT && XM), "the table forms have no ReLU mask");
    const BnLane<V> l(a);
    const float* const sTab = bn_table_lds<LUT>(a.table);
    const size_t ld = (size_t)a.c;
    const size_t c0 = l.live ? (size_t)l.ch : 0;
    const Pack<V> mean = l.live ? bn_ld<V>(a.mean + c0) : bn_fill<V>(0.f);
    const Pack<V> invstd = l.live ? bn_ld<V>(a.invstd + c0) : bn_fill<V>(0.f);
    BnMap<V> map = {mean, bn_fill<V>(0.f), bn_fill<V>(0.f), bn_fill<V>(0.f)};   // LUT, XM: the forward's lo, invstd * gamma, beta
    if constexpr (LUT || XM) {
        if (l.live) {
            const Pack<V> gamma = bn_ld<V>(a.gamma + c0);
            map.lo = bn_ld<V>(a.lo_fwd + c0);
            map.beta = bn_ld<V>(a.beta + c0);
#pragma unroll
            for (int e = 0; e < V; ++e) map.sc.v[e] = invstd.v[e] * gamma.v[e];
        }
    }
    const float* px = a.x + c0;
    const float* pg = a.gy + c0;
    const float* py = a.y + c0;   // read with relu only
    const int relu = a.relu;
    Pack<V> s[3] = {bn_fill<V>(0.f), bn_fill<V>(0.f), bn_fill<V>(0.f)};   // sg, sx, sd
    bn_walk<4>(l.first, l.r1, l.nty, ld, [&](const size_t o) { return bn_ld_bwd<V, XM>(px, pg, py, o, relu); },
               [&](const size_t, const BnRow<V, 3>& b) {
#pragma unroll
                   for (int e = 0; e < V; ++e) {
                       const float g = bn_g<V, LUT, XM>(b, e, relu, sTab, map);
                       const float d = b.p[0].v[e] - mean.v[e];
                       s[0].v[e] = s[0].v[e] + g;
                       s[1].v[e] = s[1].v[e] + g * (d * invstd.v[e]);
                       s[2].v[e] = s[2].v[e] + d;
                   }
               });
    bn_meet<V, 3>(s, l, a.tx_log2);
    if (l.ty != 0 || !l.live) return;
    float4* part = a.part + (size_t)blockIdx.x * ld + (size_t)l.ch;
#pragma unroll
    for (int e = 0; e < V; ++e) part[e] = make_float4(s[0].v[e], s[1].v[e], s[2].v[e], 0.f);
}

__global__ __launch_bounds__(kBnThreads) void k_bn_bwd_finalize(const BnArgs a, float* ggamma, float* gbeta) {
    __shared__ double ssg[kBnFinChunk][kBnFinCh], ssx[kBnFinChunk][kBnFinCh], ssd[kBnFinChunk][kBnFinCh];
    const BnFinLane l(a);
    double sg = 0.0, sx = 0.0, sd = 0.0;
    for (int base = 0; base < a.slabs; base += kBnFinChunk) {
        const int lim = a.slabs - base < kBnFinChunk ? a.slabs - base : kBnFinChunk;
        if (l.live) {
            for (int j = l.sl; j < lim; j += kBnThreads / kBnFinCh) {
                const float4 p = a.part[(size_t)(base + j) * (size_t)a.c + (size_t)l.c];
                ssg[j][l.cl] = (double)p.x;
                ssx[j][l.cl] = (double)p.y;
                ssd[j][l.cl] = (double)p.z;
            }
        }
        __syncthreads();
        if (l.sl == 0 && l.live) {
#pragma unroll 4
            for (int j = 0; j < lim; ++j) {
                sg = sg + ssg[j][l.cl];
                sx = sx + ssx[j][l.cl];
                sd = sd + ssd[j][l.cl];
            }
        }
        __syncthreads();
    }
    if (l.sl != 0 || !l.live) return;
    // lo: what the float32 save_mean misses of the mean; xh below means ((x - save_mean) - lo) * invstd
    const double cnt = (double)a.m;
    const double lo = sd / cnt;
    sx = sx - (lo * (double)a.invstd[l.c]) * sg;
    if (gbeta) gbeta[l.c] = (float)sg;
    if (ggamma) ggamma[l.c] = (float)sx;
    a.gmean[l.c] = (float)(sg / cnt);
    a.gmean[(size_t)a.c + (size_t)l.c] = (float)(sx / cnt);
    a.gmean[2 * (size_t)a.c + (size_t)l.c] = (float)lo;
}

template <int V, bool LUT = false, bool RES = false, bool XM = false>
__global__ __launch_bounds__(kBnThreads) void k_bn_bwd_dx(const BnArgs a) {
    static_assert(!(LUT && RES), "the residual form has no table");
    static_assert(!XM || (!LUT && !RES), "the recomputed mask belongs to the code forms alone");
    const BnLane<V> l(a);
    const float* const sTab = bn_table_lds<LUT>(a.table);
    if (!l.live) return;
    const size_t ld = (size_t)a.c;
    const Pack<V> mean = bn_ld<V>(a.mean + l.ch), invstd = bn_ld<V>(a.invstd + l.ch), gamma = bn_ld<V>(a.gamma + l.ch);
    const Pack<V> mb = bn_ld<V>(a.gmean + l.ch), mg = bn_ld<V>(a.gmean + ld + l.ch), lo = bn_ld<V>(a.gmean + 2 * ld + l.ch);
    BnMap<V> map = {mean, bn_fill<V>(0.f), bn_fill<V>(0.f), bn_fill<V>(0.f)};   // sc = gamma * invstd, the forward's too
#pragma unroll
    for (int e = 0; e < V; ++e) map.sc.v[e] = gamma.v[e] * invstd.v[e];
    if constexpr (LUT || XM) {   // the forward's lo and beta
        map.lo = bn_ld<V>(a.lo_fwd + l.ch);
        map.beta = bn_ld<V>(a.beta + l.ch);
    }
    const float* px = a.x + l.ch;
    const float* pg = a.gy + l.ch;
    const float* py = a.y + l.ch;   // read with relu only
    float* po = a.out + l.ch;
    float* pq = RES && a.gres ? a.gres + l.ch : nullptr;   // the residual's gradient: g itself, stored where gx is
    const int relu = a.relu;
    bn_walk<4>(l.first, l.r1, l.nty, ld, [&](const size_t o) { return bn_ld_bwd<V, XM>(px, pg, py, o, relu); },
               [&](const size_t o, const BnRow<V, 3>& b) {
                   Pack<V> gx, g;
#pragma unroll
                   for (int e = 0; e < V; ++e) {
                       g.v[e] = bn_g<V, LUT, XM>(b, e, relu, sTab, map);
                       const float xh = ((b.p[0].v[e] - mean.v[e]) - lo.v[e]) * invstd.v[e];
                       gx.v[e] = map.sc.v[e] * ((g.v[e] - mb.v[e]) - (xh * mg.v[e]));
                   }
                   bn_st<V>(po + o, gx);
                   if constexpr (RES) {
                       if (pq) bn_st<V>(pq + o, g);
                   }
               });
}

// The refusals both entry points share, in the order of include/slfp.h; *m receives N H W.
// `table`: the LUT entry points' act_table / dact_table (has_table), 16-byte aligned whatever c is.
// `cc`: the code entry points' own part (null for every other form): what their supported set adds, and the forward's y_codes.
struct BnCodeCheck {
    bool ok;             // c % 4 == 0, and in the forward a y_ka and y_qbits with a proven code table (bn_codes_table)
    bool has_codes;      // the forward: y_codes counts among the pointers, 4-byte aligned
    const void* codes;
    const char* query;   // the form's own support query, for the message
    bool by_table;       // the table-and-codes form: the caller's byte table holds the reader's quantizer, c % 4 == 0 is all
};
static int bn_check(const char* fn, int64_t n, int64_t h, int64_t w, int64_t c, int x_layout, int relu, const void* const* big,
                    int nbig, const void* const* small, int nsmall, const void* workspace, size_t ws_bytes, int64_t* m,
                    bool has_table = false, const void* table = nullptr, const BnCodeCheck* cc = nullptr) {
    for (int i = 0; i < nbig; ++i)
        if (!big[i]) return fail(SLFP_ERR_BAD_ARG, "%s: null pointer", fn);
    if (cc && cc->has_codes && !cc->codes) return fail(SLFP_ERR_BAD_ARG, "%s: null pointer (y_codes)", fn);
    for (int i = 0; i < nsmall; ++i)
        if (!small[i]) return fail(SLFP_ERR_BAD_ARG, "%s: null pointer", fn);
    if (has_table && !table) return fail(SLFP_ERR_BAD_ARG, "%s: null pointer (the table)", fn);
    if (x_layout != SLFP_LAYOUT_NHWC && x_layout != SLFP_LAYOUT_NCHW) return fail(SLFP_ERR_BAD_ARG, "%s: bad layout", fn);
    if (relu != 0 && relu != 1) return fail(SLFP_ERR_BAD_ARG, "%s: relu must be 0 or 1", fn);
    if (n < 0 || h < 1 || w < 1 || c < 1) return fail(SLFP_ERR_SHAPE, "%s: bad geometry", fn);
    if (!bn_supported(n, h, w, c, x_layout))
        return fail(SLFP_ERR_UNSUPPORTED, "%s: no kernel for this shape / layout (slfp_bn_train_supported): NHWC only, and more "
                                          "than 1 value per channel", fn);
    if (cc && !cc->ok && cc->by_table)
        return fail(SLFP_ERR_UNSUPPORTED, "%s: no kernel for this shape (%s): c %% 4 == 0", fn, cc->query);
    if (cc && !cc->ok)
        return fail(SLFP_ERR_UNSUPPORTED, "%s: no kernel for this shape / reader (%s): c %% 4 == 0, y_qbits "
                                          "8 or 7, and a y_ka > 0 with a proven code table", fn, cc->query);
    *m = n * h * w;
    const uintptr_t mask = c % 4 == 0 ? 15 : 3;
    for (int i = 0; i < nbig; ++i)
        if (reinterpret_cast<uintptr_t>(big[i]) & mask)
            return fail(SLFP_ERR_ALIGNMENT, "%s: x / y / gy / gx must be %d-byte aligned", fn, (int)mask + 1);
    if (cc && cc->has_codes && (reinterpret_cast<uintptr_t>(cc->codes) & 3))
        return fail(SLFP_ERR_ALIGNMENT, "%s: y_codes must be 4-byte aligned", fn);
    for (int i = 0; i < nsmall; ++i)
        if (reinterpret_cast<uintptr_t>(small[i]) & mask)
            return fail(SLFP_ERR_ALIGNMENT, "%s: the per-channel arrays must be %d-byte aligned", fn, (int)mask + 1);
    if (has_table && !aligned16(table)) return fail(SLFP_ERR_ALIGNMENT, "%s: the table must be 16-byte aligned", fn);
    const size_t need = bn_workspace_bytes(*m, c);
    if (need && (!workspace || ws_bytes < need || !aligned16(workspace)))
        return fail(SLFP_ERR_BAD_ARG, "%s: %zu bytes of 16-byte aligned workspace required (slfp_bn_train_workspace_bytes)", fn, need);
    return SLFP_OK;
}

// The geometry and workspace pointers of a launch, into the entry point's own pointers.  A gmean the entry point has set stays
// (the table forward sends the finalize kernel's lo to the caller's save_lo; the apply reads it there).
static void bn_geometry(BnArgs& a, const BnSplit& s, int64_t m, int64_t c, int relu, void* workspace) {
    a.m = m; a.c = c; a.rows = s.rows;
    a.slabs = (int)s.slabs; a.tx_log2 = s.tx_log2; a.relu = relu;
    a.rec = reinterpret_cast<float4*>(workspace);
    a.part = reinterpret_cast<float4*>(workspace);
    if (!a.gmean) a.gmean = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + bn_gmean_offset(s, c));
}

enum BnForm { kBnPlain, kBnTable, kBnRes, kBnCodes, kBnResCodes, kBnTableCodes };

// What the code forms add to the supported set, host only: the reader's quantizer and a proven table for it.  Returns that table
// (the one the apply is then launched with), or null.
static int bn_code_fmt(int y_qbits) { return y_qbits == 7 ? kFmtSfp7 : kFmtAct8; }
static const EncArgs* bn_codes_table(int64_t c, float y_ka, int y_qbits) {
    if (c % 4 != 0 || (y_qbits != 8 && y_qbits != 7)) return nullptr;
    if (!(y_ka > 0.f) || !scale_div_ok(y_ka) || long_encode_forced()) return nullptr;
    const EncArgs* t = enc_table(y_ka, bn_code_fmt(y_qbits), kEncCode);
    return t->valid ? t : nullptr;
}

// The streaming kernels of a (vec, form); the residual form's statistics and reduce pass are the plain ones, the code form's
// statistics too.  The code forms' apply takes the reader's table by value behind the arguments (apply_codes; V == 4 only); the
// residual-and-codes form has the residual form's backward.  The table-and-codes form (V == 4 only) has an ordinary apply, which
// finds its byte table in the arguments, and the table form's backward.
using BnKernel = void (*)(BnArgs);
using BnCodeKernel = void (*)(BnArgs, EncArgs);
struct BnKernels { BnKernel stats, apply, reduce, dx; BnCodeKernel apply_codes; };
template <int V> static BnKernels bn_kernels(BnForm form) {
    switch (form) {
        case kBnCodes:
            if constexpr (V == 4)
                return {k_bn_stats<V>, nullptr, k_bn_bwd_reduce<V, false, true>, k_bn_bwd_dx<V, false, false, true>, k_bn_apply_codes};
            else
                return {};   // no such kernels: bn_forward / bn_backward refuse a form without them
        case kBnResCodes:
            if constexpr (V == 4)
                return {k_bn_stats<V>, nullptr, k_bn_bwd_reduce<V>, k_bn_bwd_dx<V, false, true>, k_bn_apply_res_codes};
            else
                return {};
        case kBnTableCodes:
            if constexpr (V == 4)
                return {k_bn_stats<V>, k_bn_apply_lut_codes, k_bn_bwd_reduce<V, true>, k_bn_bwd_dx<V, true>, nullptr};
            else
                return {};
        case kBnTable: return {k_bn_stats<V>, k_bn_apply<V, true>, k_bn_bwd_reduce<V, true>, k_bn_bwd_dx<V, true>, nullptr};
        case kBnRes: return {k_bn_stats<V>, k_bn_apply<V, false, true>, k_bn_bwd_reduce<V>, k_bn_bwd_dx<V, false, true>, nullptr};
        default: return {k_bn_stats<V>, k_bn_apply<V>, k_bn_bwd_reduce<V>, k_bn_bwd_dx<V>, nullptr};
    }
}
static BnKernels bn_kernels(int vec, BnForm form) { return vec == 4 ? bn_kernels<4>(form) : bn_kernels<1>(form); }

// The tail of every entry point's argument list.
struct BnCall {
    int64_t n, h, w, c;
    int x_layout;
    void* workspace;
    size_t ws_bytes;
    void* stream;
};

// A failed launch names the entry point, hence the form, and the pass.
static int bn_launched(const char* fn, const char* pass) {
    char what[96];
    snprintf(what, sizeof what, "%s: slfp batch-norm %s kernel", fn, pass);
    return check_launch(what);
}

// The forward of every form.  `a` holds the entry point's pointers (x, out, gamma, beta, res, table; gmean = save_lo in the
// table and code forms; codes and code_fmt in the two code forms); `aliased` is the entry point's own aliasing refusal, or null;
// `y_ka` is the code forms' reader scale (the table-and-codes form has none: its table holds the reader's quantizer).
static int bn_forward(const char* fn, BnForm form, BnArgs a, float* running_mean, float* running_var, float momentum, float eps,
                      int relu, float* save_mean, float* save_invstd, const BnCall& g, const char* aliased, float y_ka = 0.f,
                      int y_qbits = 0) {
    a.mean = save_mean; a.invstd = save_invstd;
    const bool by_table = form == kBnTableCodes;
    const bool res = form == kBnRes || form == kBnResCodes, codes = form == kBnCodes || form == kBnResCodes || by_table;
    const bool has_lo = form == kBnTable || form == kBnCodes || by_table;
    const void* big[] = {a.x, a.out, a.res};
    const void* small[] = {a.gamma, a.beta, save_mean, save_invstd, a.gmean};
    const bool by_enc = codes && !by_table;   // the reader's threshold table travels behind the arguments
    const EncArgs* const enc = by_enc ? bn_codes_table(g.c, y_ka, y_qbits) : nullptr;   // fetched once: checked here, launched below
    const BnCodeCheck cc = {by_table ? g.c % 4 == 0 : enc != nullptr, true, a.codes,
                            by_table ? "slfp_bn_lut_codes_train_supported"
                                     : (form == kBnResCodes ? "slfp_bn_res_codes_train_supported" : "slfp_bn_codes_train_supported"),
                            by_table};
    int64_t m = 0;
    const int rc = bn_check(fn, g.n, g.h, g.w, g.c, g.x_layout, relu, big, res ? 3 : (codes ? 1 : 2), small, has_lo ? 5 : 4,
                            g.workspace, g.ws_bytes, &m, form == kBnTable || by_table, a.table, codes ? &cc : nullptr);
    if (rc != SLFP_OK) return rc;
    if ((running_mean == nullptr) != (running_var == nullptr))
        return fail(SLFP_ERR_BAD_ARG, "%s: running_mean and running_var are given together or not at all", fn);
    if ((reinterpret_cast<uintptr_t>(running_mean) | reinterpret_cast<uintptr_t>(running_var)) & 3)
        return fail(SLFP_ERR_ALIGNMENT, "%s: the running statistics must be 4-byte aligned", fn);
    if (aliased) return fail(SLFP_ERR_BAD_ARG, "%s: %s", fn, aliased);
    if (m == 0) return SLFP_OK;
    const BnSplit s = bn_split(m, g.c);
    bn_geometry(a, s, m, g.c, relu, g.workspace);
    const BnKernels k = bn_kernels(s.vec, form);
    if (!k.stats || !(by_enc ? (k.apply_codes && enc) : (bool)k.apply))
        return fail(SLFP_ERR_UNSUPPORTED, "%s: no kernels of this form for %d channel(s) per lane", fn, s.vec);
    const dim3 grid((unsigned)s.slabs, (unsigned)s.tiles), block(kBnThreads);
    const hipStream_t st = as_stream(g.stream);
    hipLaunchKernelGGL(k.stats, grid, block, 0, st, a);
    int e = bn_launched(fn, "statistics");
    if (e != SLFP_OK) return e;
    hipLaunchKernelGGL(k_bn_finalize, dim3((unsigned)ceil_div(g.c, kBnFinCh)), block, 0, st, a, running_mean, running_var, momentum,
                       eps, save_mean, save_invstd);
    e = bn_launched(fn, "finalize");
    if (e != SLFP_OK) return e;
    if (by_enc) hipLaunchKernelGGL(k.apply_codes, grid, block, 0, st, a, *enc);
    else hipLaunchKernelGGL(k.apply, grid, block, 0, st, a);
    return bn_launched(fn, "apply");
}

// The backward of every form.  `a` holds the entry point's pointers (x, y, gy, out, gamma, mean, invstd, gres; beta, lo_fwd and
// table in the table form, beta and lo_fwd in the code form; the y of both is x: it is never read); `misaligned` and `aliased` are
// the entry point's own refusals, or null.
static int bn_backward(const char* fn, BnForm form, BnArgs a, int relu, float* ggamma, float* gbeta, const BnCall& g,
                       const char* misaligned, const char* aliased) {
    const void* big[] = {a.x, a.y, a.gy, a.out};
    const void* small[] = {a.gamma, a.mean, a.invstd, a.beta, a.lo_fwd};
    const bool codes = form == kBnCodes;
    const BnCodeCheck cc = {g.c % 4 == 0, false, nullptr, "slfp_bn_codes_train_supported", false};
    int64_t m = 0;
    const int rc = bn_check(fn, g.n, g.h, g.w, g.c, g.x_layout, relu, big, 4, small, form == kBnTable || codes ? 5 : 3, g.workspace,
                            g.ws_bytes, &m, form == kBnTable, a.table, codes ? &cc : nullptr);
    if (rc != SLFP_OK) return rc;
    if (misaligned) return fail(SLFP_ERR_ALIGNMENT, "%s: %s", fn, misaligned);
    if ((reinterpret_cast<uintptr_t>(ggamma) | reinterpret_cast<uintptr_t>(gbeta)) & 3)
        return fail(SLFP_ERR_ALIGNMENT, "%s: ggamma and gbeta must be 4-byte aligned", fn);
    if (aliased) return fail(SLFP_ERR_BAD_ARG, "%s: %s", fn, aliased);
    if (m == 0) return SLFP_OK;
    const BnSplit s = bn_split(m, g.c);
    bn_geometry(a, s, m, g.c, relu, g.workspace);
    const BnKernels k = bn_kernels(s.vec, form);
    if (!k.reduce || !k.dx) return fail(SLFP_ERR_UNSUPPORTED, "%s: no kernels of this form for %d channel(s) per lane", fn, s.vec);
    const dim3 grid((unsigned)s.slabs, (unsigned)s.tiles), block(kBnThreads);
    const hipStream_t st = as_stream(g.stream);
    hipLaunchKernelGGL(k.reduce, grid, block, 0, st, a);
    int e = bn_launched(fn, "backward reduce");
    if (e != SLFP_OK) return e;
    hipLaunchKernelGGL(k_bn_bwd_finalize, dim3((unsigned)ceil_div(g.c, kBnFinCh)), block, 0, st, a, ggamma, gbeta);
    e = bn_launched(fn, "backward finalize");
    if (e != SLFP_OK) return e;
    hipLaunchKernelGGL(k.dx, grid, block, 0, st, a);
    return bn_launched(fn, "backward dx");
}

}  // namespace slfp

using namespace slfp;

extern "C" {

int slfp_bn_train_supported(int64_t n, int64_t h, int64_t w, int64_t c, int x_layout) {
    return bn_supported(n, h, w, c, x_layout) ? 1 : 0;
}

size_t slfp_bn_train_workspace_bytes(int64_t n, int64_t h, int64_t w, int64_t c) {
    if (!bn_supported(n, h, w, c, SLFP_LAYOUT_NHWC)) return 0;
    return bn_workspace_bytes(n * h * w, c);
}

int slfp_debug_bn_split(int64_t m, int64_t c, int64_t* rows_per_slab, int64_t* slabs) {
    if (!rows_per_slab || !slabs) return fail(SLFP_ERR_BAD_ARG, "slfp_debug_bn_split: null pointer");
    if (m < 1 || c < 1 || m > 0x7FFFFFFF || c > (1 << 21)) return fail(SLFP_ERR_SHAPE, "slfp_debug_bn_split: bad geometry");
    const BnSplit s = bn_split(m, c);
    *rows_per_slab = s.rows;
    *slabs = s.slabs;
    return SLFP_OK;
}

int slfp_bn_train_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                      float momentum, float eps, int relu, float* y, float* save_mean, float* save_invstd, int64_t n, int64_t h,
                      int64_t w, int64_t c, int x_layout, void* workspace, size_t ws_bytes, void* stream) {
    BnArgs a = {};
    a.x = x; a.out = y; a.gamma = gamma; a.beta = beta;
    return bn_forward("slfp_bn_train_fwd", kBnPlain, a, running_mean, running_var, momentum, eps, relu, save_mean, save_invstd,
                      {n, h, w, c, x_layout, workspace, ws_bytes, stream},
                      x == y ? "y may not alias x (the backward reads both)" : nullptr);
}

int slfp_bn_train_bwd(const float* x, const float* y, const float* gy, const float* gamma, const float* save_mean,
                      const float* save_invstd, int relu, float* gx, float* ggamma, float* gbeta, int64_t n, int64_t h, int64_t w,
                      int64_t c, int x_layout, void* workspace, size_t ws_bytes, void* stream) {
    BnArgs a = {};
    a.x = x; a.y = y; a.gy = gy; a.out = gx; a.gamma = gamma; a.mean = save_mean; a.invstd = save_invstd;
    return bn_backward("slfp_bn_train_bwd", kBnPlain, a, relu, ggamma, gbeta, {n, h, w, c, x_layout, workspace, ws_bytes, stream},
                       nullptr, gx == x || gx == y ? "gx may not alias x or y" : nullptr);
}

int slfp_bn_res_train_fwd(const float* x, const float* res, const float* gamma, const float* beta, float* running_mean,
                          float* running_var, float momentum, float eps, int relu, float* y, float* save_mean, float* save_invstd,
                          int64_t n, int64_t h, int64_t w, int64_t c, int x_layout, void* workspace, size_t ws_bytes, void* stream) {
    BnArgs a = {};
    a.x = x; a.res = res; a.out = y; a.gamma = gamma; a.beta = beta;
    return bn_forward("slfp_bn_res_train_fwd", kBnRes, a, running_mean, running_var, momentum, eps, relu, save_mean, save_invstd,
                      {n, h, w, c, x_layout, workspace, ws_bytes, stream},
                      y == x || y == res ? "y may alias neither x nor res (the backward reads x and y)" : nullptr);
}

int slfp_bn_res_train_bwd(const float* x, const float* y, const float* gy, const float* gamma, const float* save_mean,
                          const float* save_invstd, int relu, float* gx, float* gres, float* ggamma, float* gbeta, int64_t n,
                          int64_t h, int64_t w, int64_t c, int x_layout, void* workspace, size_t ws_bytes, void* stream) {
    BnArgs a = {};
    a.x = x; a.y = y; a.gy = gy; a.out = gx; a.gres = gres; a.gamma = gamma; a.mean = save_mean; a.invstd = save_invstd;
    const char* misaligned = nullptr;
    if (reinterpret_cast<uintptr_t>(gres) & (c % 4 == 0 ? 15 : 3))
        misaligned = c % 4 == 0 ? "gres must be 16-byte aligned" : "gres must be 4-byte aligned";
    const char* aliased = nullptr;
    if (gx == x || gx == y || gx == gy) aliased = "gx may not alias x, y or gy";
    else if (gres && (gres == x || gres == y || gres == gy || gres == gx)) aliased = "gres may not alias x, y, gy or gx";
    return bn_backward("slfp_bn_res_train_bwd", kBnRes, a, relu, ggamma, gbeta, {n, h, w, c, x_layout, workspace, ws_bytes, stream},
                       misaligned, aliased);
}

int slfp_bn_lut_train_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                          float momentum, float eps, const float* act_table, float* y, float* save_mean, float* save_invstd,
                          float* save_lo, int64_t n, int64_t h, int64_t w, int64_t c, int x_layout, void* workspace,
                          size_t ws_bytes, void* stream) {
    BnArgs a = {};
    a.x = x; a.out = y; a.gamma = gamma; a.beta = beta; a.table = act_table;
    a.gmean = save_lo;   // the finalize kernel's lo goes to the caller instead of the workspace; the apply reads it there
    return bn_forward("slfp_bn_lut_train_fwd", kBnTable, a, running_mean, running_var, momentum, eps, 0, save_mean, save_invstd,
                      {n, h, w, c, x_layout, workspace, ws_bytes, stream}, x == y ? "y may not alias x (the backward reads x)" : nullptr);
}

int slfp_bn_lut_train_bwd(const float* x, const float* gy, const float* gamma, const float* beta, const float* save_mean,
                          const float* save_invstd, const float* save_lo, const float* dact_table, float* gx, float* ggamma,
                          float* gbeta, int64_t n, int64_t h, int64_t w, int64_t c, int x_layout, void* workspace,
                          size_t ws_bytes, void* stream) {
    BnArgs a = {};
    a.x = x; a.y = x; a.gy = gy; a.out = gx; a.gamma = gamma; a.beta = beta; a.mean = save_mean; a.invstd = save_invstd;
    a.lo_fwd = save_lo; a.table = dact_table;
    return bn_backward("slfp_bn_lut_train_bwd", kBnTable, a, 0, ggamma, gbeta, {n, h, w, c, x_layout, workspace, ws_bytes, stream},
                       nullptr, gx == x ? "gx may not alias x" : nullptr);
}

int slfp_bn_lut_codes_train_supported(int64_t n, int64_t h, int64_t w, int64_t c, int x_layout) {
    return bn_supported(n, h, w, c, x_layout) && c % 4 == 0 ? 1 : 0;
}

int slfp_bn_lut_codes_train_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                                float momentum, float eps, const uint8_t* code_table, uint8_t* y_codes, float* save_mean,
                                float* save_invstd, float* save_lo, int64_t n, int64_t h, int64_t w, int64_t c, int x_layout,
                                void* workspace, size_t ws_bytes, void* stream) {
    BnArgs a = {};
    a.x = x; a.codes = y_codes; a.gamma = gamma; a.beta = beta;
    a.table = reinterpret_cast<const float*>(code_table);   // read as bytes (bn_code_lds)
    a.gmean = save_lo;   // as the table form: slfp_bn_lut_train_bwd recomputes the class from it
    return bn_forward("slfp_bn_lut_codes_train_fwd", kBnTableCodes, a, running_mean, running_var, momentum, eps, 0, save_mean,
                      save_invstd, {n, h, w, c, x_layout, workspace, ws_bytes, stream},
                      reinterpret_cast<const void*>(x) == reinterpret_cast<const void*>(y_codes)
                          ? "y_codes may not alias x (the backward reads x)" : nullptr);
}

int slfp_bn_codes_train_supported(int64_t n, int64_t h, int64_t w, int64_t c, int x_layout, float y_ka, int y_qbits) {
    return bn_supported(n, h, w, c, x_layout) && bn_codes_table(c, y_ka, y_qbits) ? 1 : 0;
}

int slfp_bn_codes_train_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                            float momentum, float eps, int relu, float y_ka, int y_qbits, uint8_t* y_codes, float* save_mean,
                            float* save_invstd, float* save_lo, int64_t n, int64_t h, int64_t w, int64_t c, int x_layout,
                            void* workspace, size_t ws_bytes, void* stream) {
    BnArgs a = {};
    a.x = x; a.codes = y_codes; a.code_fmt = bn_code_fmt(y_qbits); a.gamma = gamma; a.beta = beta;
    a.gmean = save_lo;   // as the table form: the backward recomputes the forward's t from it
    return bn_forward("slfp_bn_codes_train_fwd", kBnCodes, a, running_mean, running_var, momentum, eps, relu, save_mean, save_invstd,
                      {n, h, w, c, x_layout, workspace, ws_bytes, stream},
                      reinterpret_cast<const void*>(x) == reinterpret_cast<const void*>(y_codes)
                          ? "y_codes may not alias x (the backward reads x)" : nullptr,
                      y_ka, y_qbits);
}

int slfp_bn_codes_train_bwd(const float* x, const float* gy, const float* gamma, const float* beta, const float* save_mean,
                            const float* save_invstd, const float* save_lo, int relu, float* gx, float* ggamma, float* gbeta,
                            int64_t n, int64_t h, int64_t w, int64_t c, int x_layout, void* workspace, size_t ws_bytes,
                            void* stream) {
    BnArgs a = {};
    a.x = x; a.y = x; a.gy = gy; a.out = gx; a.gamma = gamma; a.beta = beta; a.mean = save_mean; a.invstd = save_invstd;
    a.lo_fwd = save_lo;
    return bn_backward("slfp_bn_codes_train_bwd", kBnCodes, a, relu, ggamma, gbeta, {n, h, w, c, x_layout, workspace, ws_bytes, stream},
                       nullptr, gx == x ? "gx may not alias x" : nullptr);
}

int slfp_bn_res_codes_train_supported(int64_t n, int64_t h, int64_t w, int64_t c, int x_layout, float y_ka, int y_qbits) {
    return bn_supported(n, h, w, c, x_layout) && bn_codes_table(c, y_ka, y_qbits) ? 1 : 0;
}

int slfp_bn_res_codes_train_fwd(const float* x, const float* res, const float* gamma, const float* beta, float* running_mean,
                                float* running_var, float momentum, float eps, int relu, float y_ka, int y_qbits, float* y,
                                uint8_t* y_codes, float* save_mean, float* save_invstd, int64_t n, int64_t h, int64_t w, int64_t c,
                                int x_layout, void* workspace, size_t ws_bytes, void* stream) {
    BnArgs a = {};
    a.x = x; a.res = res; a.out = y; a.codes = y_codes; a.code_fmt = bn_code_fmt(y_qbits); a.gamma = gamma; a.beta = beta;
    const char* aliased = nullptr;
    if (y == x || y == res) aliased = "y may alias neither x nor res (the backward reads x and y)";
    const void* const others[] = {x, res, y, gamma, beta, running_mean, running_var, save_mean, save_invstd, workspace};
    for (const void* o : others)
        if (o == reinterpret_cast<const void*>(y_codes)) aliased = "y_codes may alias no other operand";
    return bn_forward("slfp_bn_res_codes_train_fwd", kBnResCodes, a, running_mean, running_var, momentum, eps, relu, save_mean,
                      save_invstd, {n, h, w, c, x_layout, workspace, ws_bytes, stream}, aliased, y_ka, y_qbits);
}

}  // extern "C"
