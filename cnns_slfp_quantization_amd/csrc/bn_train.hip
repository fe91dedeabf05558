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
// The two finalize kernels stage the records of 256 slabs x 8 channels in LDS with all 256 lanes (and the per-slab weights
// n_b / n and n_a n_b / n, which depend on the slab index alone), then one lane per channel runs the serial chain.
#include "slfp_device.hpp"
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
    const float* table;    // LUT forms: act_table (forward) / dact_table (backward), kBnTableFloats floats
    const float* res;      // residual forward: the operand added behind the affine map
    float* gres;           // residual backward: the residual's gradient g, or null
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

// LUT forms: the class of one element, from the forward's own expression (sc = invstd * gamma)
__device__ __forceinline__ uint32_t bn_class(const float x, const float mean, const float lo, const float sc, const float beta) {
    const float t = (((x - mean) - lo) * sc) + beta;
    return layerout_class(layerout_bits(__float_as_uint(t)));
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
    const int64_t st = l.nty;
    int64_t r = l.first;
    for (; r + 7 * st < l.r1; r += 8 * st) {   // eight loads ahead of the adds of this lane's one chain per channel
        Pack<V> v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = bn_ld<V>(px + (size_t)(r + i * st) * ld);
#pragma unroll
        for (int i = 0; i < 8; ++i) bn_stat_add<V>(s, v[i], k);
    }
    for (; r < l.r1; r += st) bn_stat_add<V>(s, bn_ld<V>(px + (size_t)r * ld), k);
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

template <int V, bool LUT = false, bool RES = false>
__global__ __launch_bounds__(kBnThreads) void k_bn_apply(const BnArgs a) {
    static_assert(!(LUT && RES), "the residual form has no table");
    const BnLane<V> l(a);
    const float* const sTab = bn_table_lds<LUT>(a.table);
    if (!l.live) return;
    const size_t ld = (size_t)a.c;
    const Pack<V> mean = bn_ld<V>(a.mean + l.ch), lo = bn_ld<V>(a.gmean + l.ch), beta = bn_ld<V>(a.beta + l.ch);
    Pack<V> sc = bn_ld<V>(a.invstd + l.ch);
    const Pack<V> gamma = bn_ld<V>(a.gamma + l.ch);
#pragma unroll
    for (int e = 0; e < V; ++e) sc.v[e] = sc.v[e] * gamma.v[e];
    const float* px = a.x + l.ch;
    float* py = a.out + l.ch;
    const int relu = a.relu;
    auto f = [&](Pack<V> v) {
#pragma unroll
        for (int e = 0; e < V; ++e) {
            if constexpr (LUT) {
                v.v[e] = sTab[bn_class(v.v[e], mean.v[e], lo.v[e], sc.v[e], beta.v[e])];
            } else {
                float t = (((v.v[e] - mean.v[e]) - lo.v[e]) * sc.v[e]) + beta.v[e];
                if (relu) t = t < 0.f ? 0.f : t;
                v.v[e] = t;
            }
        }
        return v;
    };
    const int64_t st = l.nty;
    int64_t r = l.first;
    if constexpr (RES) {
        const float* pr = a.res + l.ch;
        auto fr = [&](Pack<V> v, const Pack<V>& q) {   // the add is rounded on its own, the ReLU comes behind it
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float t = (((v.v[e] - mean.v[e]) - lo.v[e]) * sc.v[e]) + beta.v[e];
                float z = t + q.v[e];
                if (relu) z = z < 0.f ? 0.f : z;
                v.v[e] = z;
            }
            return v;
        };
        for (; r + 3 * st < l.r1; r += 4 * st) {
            Pack<V> v[4], q[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const size_t o = (size_t)(r + i * st) * ld;
                v[i] = bn_ld<V>(px + o);
                q[i] = bn_ld<V>(pr + o);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) bn_st<V>(py + (size_t)(r + i * st) * ld, fr(v[i], q[i]));
        }
        for (; r < l.r1; r += st) {
            const size_t o = (size_t)r * ld;
            bn_st<V>(py + o, fr(bn_ld<V>(px + o), bn_ld<V>(pr + o)));
        }
    } else {
        for (; r + 3 * st < l.r1; r += 4 * st) {
            Pack<V> v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = bn_ld<V>(px + (size_t)(r + i * st) * ld);
#pragma unroll
            for (int i = 0; i < 4; ++i) bn_st<V>(py + (size_t)(r + i * st) * ld, f(v[i]));
        }
        for (; r < l.r1; r += st) bn_st<V>(py + (size_t)r * ld, f(bn_ld<V>(px + (size_t)r * ld)));
    }
}

// g of one element: the ReLU's mask is read from the forward's own output
__device__ __forceinline__ float bn_g(const float gy, const float y, const int relu) { return relu ? (y > 0.f ? gy : 0.f) : gy; }

template <int V, bool LUT = false>
__global__ __launch_bounds__(kBnThreads) void k_bn_bwd_reduce(const BnArgs a) {
    const BnLane<V> l(a);
    const float* const sTab = bn_table_lds<LUT>(a.table);
    const size_t ld = (size_t)a.c;
    const size_t c0 = l.live ? (size_t)l.ch : 0;
    const Pack<V> mean = l.live ? bn_ld<V>(a.mean + c0) : bn_fill<V>(0.f);
    const Pack<V> invstd = l.live ? bn_ld<V>(a.invstd + c0) : bn_fill<V>(0.f);
    Pack<V> lof = bn_fill<V>(0.f), sc = bn_fill<V>(0.f), beta = bn_fill<V>(0.f);   // LUT: the forward's lo, invstd * gamma, beta
    if constexpr (LUT) {
        if (l.live) {
            const Pack<V> gamma = bn_ld<V>(a.gamma + c0);
            lof = bn_ld<V>(a.lo_fwd + c0);
            beta = bn_ld<V>(a.beta + c0);
#pragma unroll
            for (int e = 0; e < V; ++e) sc.v[e] = invstd.v[e] * gamma.v[e];
        }
    }
    const float* px = a.x + c0;
    const float* pg = a.gy + c0;
    const float* py = a.y + c0;   // read with relu only
    const int relu = a.relu;
    Pack<V> s[3] = {bn_fill<V>(0.f), bn_fill<V>(0.f), bn_fill<V>(0.f)};   // sg, sx, sd
    auto add = [&](const Pack<V>& x, const Pack<V>& gy, const Pack<V>& y) {
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float g;
            if constexpr (LUT) g = gy.v[e] * sTab[bn_class(x.v[e], mean.v[e], lof.v[e], sc.v[e], beta.v[e])];
            else g = bn_g(gy.v[e], y.v[e], relu);
            const float d = x.v[e] - mean.v[e];
            s[0].v[e] = s[0].v[e] + g;
            s[1].v[e] = s[1].v[e] + g * (d * invstd.v[e]);
            s[2].v[e] = s[2].v[e] + d;
        }
    };
    const int64_t st = l.nty;
    int64_t r = l.first;
    for (; r + 3 * st < l.r1; r += 4 * st) {
        Pack<V> x[4], g[4], y[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const size_t o = (size_t)(r + i * st) * ld;
            x[i] = bn_ld<V>(px + o);
            g[i] = bn_ld<V>(pg + o);
            y[i] = relu ? bn_ld<V>(py + o) : g[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) add(x[i], g[i], y[i]);
    }
    for (; r < l.r1; r += st) {
        const size_t o = (size_t)r * ld;
        const Pack<V> g = bn_ld<V>(pg + o);
        add(bn_ld<V>(px + o), g, relu ? bn_ld<V>(py + o) : g);
    }
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

template <int V, bool LUT = false, bool RES = false>
__global__ __launch_bounds__(kBnThreads) void k_bn_bwd_dx(const BnArgs a) {
    static_assert(!(LUT && RES), "the residual form has no table");
    const BnLane<V> l(a);
    const float* const sTab = bn_table_lds<LUT>(a.table);
    if (!l.live) return;
    const size_t ld = (size_t)a.c;
    const Pack<V> mean = bn_ld<V>(a.mean + l.ch), invstd = bn_ld<V>(a.invstd + l.ch), gamma = bn_ld<V>(a.gamma + l.ch);
    const Pack<V> mb = bn_ld<V>(a.gmean + l.ch), mg = bn_ld<V>(a.gmean + ld + l.ch), lo = bn_ld<V>(a.gmean + 2 * ld + l.ch);
    Pack<V> sc;
#pragma unroll
    for (int e = 0; e < V; ++e) sc.v[e] = gamma.v[e] * invstd.v[e];
    Pack<V> lof = bn_fill<V>(0.f), beta = bn_fill<V>(0.f);   // LUT: the forward's lo and beta (its invstd * gamma is sc)
    if constexpr (LUT) {
        lof = bn_ld<V>(a.lo_fwd + l.ch);
        beta = bn_ld<V>(a.beta + l.ch);
    }
    const float* px = a.x + l.ch;
    const float* pg = a.gy + l.ch;
    const float* py = a.y + l.ch;   // read with relu only
    float* po = a.out + l.ch;
    const int relu = a.relu;
    auto f = [&](const Pack<V>& x, const Pack<V>& gy, const Pack<V>& y) {
        Pack<V> o;
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float g;
            if constexpr (LUT) g = gy.v[e] * sTab[bn_class(x.v[e], mean.v[e], lof.v[e], sc.v[e], beta.v[e])];
            else g = bn_g(gy.v[e], y.v[e], relu);
            const float xh = ((x.v[e] - mean.v[e]) - lo.v[e]) * invstd.v[e];
            o.v[e] = sc.v[e] * ((g - mb.v[e]) - (xh * mg.v[e]));
        }
        return o;
    };
    const int64_t st = l.nty;
    int64_t r = l.first;
    if constexpr (RES) {
        float* pq = a.gres ? a.gres + l.ch : nullptr;   // the residual's gradient: g itself, stored where gx is
        auto gq = [&](const Pack<V>& gy, const Pack<V>& y) {
            Pack<V> o;
#pragma unroll
            for (int e = 0; e < V; ++e) o.v[e] = bn_g(gy.v[e], y.v[e], relu);
            return o;
        };
        for (; r + 3 * st < l.r1; r += 4 * st) {
            Pack<V> x[4], g[4], y[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const size_t o = (size_t)(r + i * st) * ld;
                x[i] = bn_ld<V>(px + o);
                g[i] = bn_ld<V>(pg + o);
                y[i] = relu ? bn_ld<V>(py + o) : g[i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const size_t o = (size_t)(r + i * st) * ld;
                bn_st<V>(po + o, f(x[i], g[i], y[i]));
                if (pq) bn_st<V>(pq + o, gq(g[i], y[i]));
            }
        }
        for (; r < l.r1; r += st) {
            const size_t o = (size_t)r * ld;
            const Pack<V> g = bn_ld<V>(pg + o);
            const Pack<V> y = relu ? bn_ld<V>(py + o) : g;
            bn_st<V>(po + o, f(bn_ld<V>(px + o), g, y));
            if (pq) bn_st<V>(pq + o, gq(g, y));
        }
        return;
    }
    for (; r + 3 * st < l.r1; r += 4 * st) {
        Pack<V> x[4], g[4], y[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const size_t o = (size_t)(r + i * st) * ld;
            x[i] = bn_ld<V>(px + o);
            g[i] = bn_ld<V>(pg + o);
            y[i] = relu ? bn_ld<V>(py + o) : g[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) bn_st<V>(po + (size_t)(r + i * st) * ld, f(x[i], g[i], y[i]));
    }
    for (; r < l.r1; r += st) {
        const size_t o = (size_t)r * ld;
        const Pack<V> g = bn_ld<V>(pg + o);
        bn_st<V>(po + o, f(bn_ld<V>(px + o), g, relu ? bn_ld<V>(py + o) : g));
    }
}

// The refusals both entry points share, in the order of include/slfp.h; *m receives N H W.
// `table`: the LUT entry points' act_table / dact_table (has_table), 16-byte aligned whatever c is.
static int bn_check(const char* fn, int64_t n, int64_t h, int64_t w, int64_t c, int x_layout, int relu, const void* const* big,
                    int nbig, const void* const* small, int nsmall, const void* workspace, size_t ws_bytes, int64_t* m,
                    bool has_table = false, const void* table = nullptr) {
    for (int i = 0; i < nbig; ++i)
        if (!big[i]) return fail(SLFP_ERR_BAD_ARG, "%s: null pointer", fn);
    for (int i = 0; i < nsmall; ++i)
        if (!small[i]) return fail(SLFP_ERR_BAD_ARG, "%s: null pointer", fn);
    if (has_table && !table) return fail(SLFP_ERR_BAD_ARG, "%s: null pointer (the table)", fn);
    if (x_layout != SLFP_LAYOUT_NHWC && x_layout != SLFP_LAYOUT_NCHW) return fail(SLFP_ERR_BAD_ARG, "%s: bad layout", fn);
    if (relu != 0 && relu != 1) return fail(SLFP_ERR_BAD_ARG, "%s: relu must be 0 or 1", fn);
    if (n < 0 || h < 1 || w < 1 || c < 1) return fail(SLFP_ERR_SHAPE, "%s: bad geometry", fn);
    if (!bn_supported(n, h, w, c, x_layout))
        return fail(SLFP_ERR_UNSUPPORTED, "%s: no kernel for this shape / layout (slfp_bn_train_supported): NHWC only, and more "
                                          "than 1 value per channel", fn);
    *m = n * h * w;
    const uintptr_t mask = c % 4 == 0 ? 15 : 3;
    for (int i = 0; i < nbig; ++i)
        if (reinterpret_cast<uintptr_t>(big[i]) & mask)
            return fail(SLFP_ERR_ALIGNMENT, "%s: x / y / gy / gx must be %d-byte aligned", fn, (int)mask + 1);
    for (int i = 0; i < nsmall; ++i)
        if (reinterpret_cast<uintptr_t>(small[i]) & mask)
            return fail(SLFP_ERR_ALIGNMENT, "%s: the per-channel arrays must be %d-byte aligned", fn, (int)mask + 1);
    if (has_table && !aligned16(table)) return fail(SLFP_ERR_ALIGNMENT, "%s: the table must be 16-byte aligned", fn);
    const size_t need = bn_workspace_bytes(*m, c);
    if (need && (!workspace || ws_bytes < need || !aligned16(workspace)))
        return fail(SLFP_ERR_BAD_ARG, "%s: %zu bytes of 16-byte aligned workspace required (slfp_bn_train_workspace_bytes)", fn, need);
    return SLFP_OK;
}

static BnArgs bn_args(const BnSplit& s, int64_t m, int64_t c, int relu, void* workspace) {
    BnArgs a = {};
    a.m = m; a.c = c; a.rows = s.rows;
    a.slabs = (int)s.slabs; a.tx_log2 = s.tx_log2; a.relu = relu;
    a.rec = reinterpret_cast<float4*>(workspace);
    a.part = reinterpret_cast<float4*>(workspace);
    a.gmean = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + bn_gmean_offset(s, c));
    return a;
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
    const char* fn = "slfp_bn_train_fwd";
    const void* big[] = {x, y};
    const void* small[] = {gamma, beta, save_mean, save_invstd};
    int64_t m = 0;
    const int rc = bn_check(fn, n, h, w, c, x_layout, relu, big, 2, small, 4, workspace, ws_bytes, &m);
    if (rc != SLFP_OK) return rc;
    if ((running_mean == nullptr) != (running_var == nullptr))
        return fail(SLFP_ERR_BAD_ARG, "%s: running_mean and running_var are given together or not at all", fn);
    if ((reinterpret_cast<uintptr_t>(running_mean) | reinterpret_cast<uintptr_t>(running_var)) & 3)
        return fail(SLFP_ERR_ALIGNMENT, "%s: the running statistics must be 4-byte aligned", fn);
    if (x == y) return fail(SLFP_ERR_BAD_ARG, "%s: y may not alias x (the backward reads both)", fn);
    if (m == 0) return SLFP_OK;
    const BnSplit s = bn_split(m, c);
    BnArgs a = bn_args(s, m, c, relu, workspace);
    a.x = x; a.out = y; a.gamma = gamma; a.beta = beta; a.mean = save_mean; a.invstd = save_invstd;
    const dim3 grid((unsigned)s.slabs, (unsigned)s.tiles), block(kBnThreads);
    const hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(s.vec == 4 ? k_bn_stats<4> : k_bn_stats<1>, grid, block, 0, st, a);
    int e = check_launch("slfp batch-norm statistics kernel");
    if (e != SLFP_OK) return e;
    hipLaunchKernelGGL(k_bn_finalize, dim3((unsigned)ceil_div(c, kBnFinCh)), block, 0, st, a, running_mean, running_var, momentum,
                       eps, save_mean, save_invstd);
    e = check_launch("slfp batch-norm finalize kernel");
    if (e != SLFP_OK) return e;
    hipLaunchKernelGGL(s.vec == 4 ? k_bn_apply<4> : k_bn_apply<1>, grid, block, 0, st, a);
    return check_launch("slfp batch-norm apply kernel");
}

int slfp_bn_train_bwd(const float* x, const float* y, const float* gy, const float* gamma, const float* save_mean,
                      const float* save_invstd, int relu, float* gx, float* ggamma, float* gbeta, int64_t n, int64_t h, int64_t w,
                      int64_t c, int x_layout, void* workspace, size_t ws_bytes, void* stream) {
    const char* fn = "slfp_bn_train_bwd";
    const void* big[] = {x, y, gy, gx};
    const void* small[] = {gamma, save_mean, save_invstd};
    int64_t m = 0;
    const int rc = bn_check(fn, n, h, w, c, x_layout, relu, big, 4, small, 3, workspace, ws_bytes, &m);
    if (rc != SLFP_OK) return rc;
    if ((reinterpret_cast<uintptr_t>(ggamma) | reinterpret_cast<uintptr_t>(gbeta)) & 3)
        return fail(SLFP_ERR_ALIGNMENT, "%s: ggamma and gbeta must be 4-byte aligned", fn);
    if (gx == x || gx == y) return fail(SLFP_ERR_BAD_ARG, "%s: gx may not alias x or y", fn);
    if (m == 0) return SLFP_OK;
    const BnSplit s = bn_split(m, c);
    BnArgs a = bn_args(s, m, c, relu, workspace);
    a.x = x; a.y = y; a.gy = gy; a.out = gx; a.gamma = gamma; a.mean = save_mean; a.invstd = save_invstd;
    const dim3 grid((unsigned)s.slabs, (unsigned)s.tiles), block(kBnThreads);
    const hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(s.vec == 4 ? k_bn_bwd_reduce<4> : k_bn_bwd_reduce<1>, grid, block, 0, st, a);
    int e = check_launch("slfp batch-norm backward reduce kernel");
    if (e != SLFP_OK) return e;
    hipLaunchKernelGGL(k_bn_bwd_finalize, dim3((unsigned)ceil_div(c, kBnFinCh)), block, 0, st, a, ggamma, gbeta);
    e = check_launch("slfp batch-norm backward finalize kernel");
    if (e != SLFP_OK) return e;
    hipLaunchKernelGGL(s.vec == 4 ? k_bn_bwd_dx<4> : k_bn_bwd_dx<1>, grid, block, 0, st, a);
    return check_launch("slfp batch-norm backward dx kernel");
}

int slfp_bn_res_train_fwd(const float* x, const float* res, const float* gamma, const float* beta, float* running_mean,
                          float* running_var, float momentum, float eps, int relu, float* y, float* save_mean, float* save_invstd,
                          int64_t n, int64_t h, int64_t w, int64_t c, int x_layout, void* workspace, size_t ws_bytes, void* stream) {
    const char* fn = "slfp_bn_res_train_fwd";
    const void* big[] = {x, res, y};
    const void* small[] = {gamma, beta, save_mean, save_invstd};
    int64_t m = 0;
    const int rc = bn_check(fn, n, h, w, c, x_layout, relu, big, 3, small, 4, workspace, ws_bytes, &m);
    if (rc != SLFP_OK) return rc;
    if ((running_mean == nullptr) != (running_var == nullptr))
        return fail(SLFP_ERR_BAD_ARG, "%s: running_mean and running_var are given together or not at all", fn);
    if ((reinterpret_cast<uintptr_t>(running_mean) | reinterpret_cast<uintptr_t>(running_var)) & 3)
        return fail(SLFP_ERR_ALIGNMENT, "%s: the running statistics must be 4-byte aligned", fn);
    if (y == x || y == res) return fail(SLFP_ERR_BAD_ARG, "%s: y may alias neither x nor res (the backward reads x and y)", fn);
    if (m == 0) return SLFP_OK;
    const BnSplit s = bn_split(m, c);
    BnArgs a = bn_args(s, m, c, relu, workspace);
    a.x = x; a.res = res; a.out = y; a.gamma = gamma; a.beta = beta; a.mean = save_mean; a.invstd = save_invstd;
    const dim3 grid((unsigned)s.slabs, (unsigned)s.tiles), block(kBnThreads);
    const hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(s.vec == 4 ? k_bn_stats<4> : k_bn_stats<1>, grid, block, 0, st, a);
    int e = check_launch("slfp batch-norm statistics kernel");
    if (e != SLFP_OK) return e;
    hipLaunchKernelGGL(k_bn_finalize, dim3((unsigned)ceil_div(c, kBnFinCh)), block, 0, st, a, running_mean, running_var, momentum,
                       eps, save_mean, save_invstd);
    e = check_launch("slfp batch-norm finalize kernel");
    if (e != SLFP_OK) return e;
    hipLaunchKernelGGL((s.vec == 4 ? k_bn_apply<4, false, true> : k_bn_apply<1, false, true>), grid, block, 0, st, a);
    return check_launch("slfp batch-norm residual apply kernel");
}

int slfp_bn_res_train_bwd(const float* x, const float* y, const float* gy, const float* gamma, const float* save_mean,
                          const float* save_invstd, int relu, float* gx, float* gres, float* ggamma, float* gbeta, int64_t n,
                          int64_t h, int64_t w, int64_t c, int x_layout, void* workspace, size_t ws_bytes, void* stream) {
    const char* fn = "slfp_bn_res_train_bwd";
    const void* big[] = {x, y, gy, gx};
    const void* small[] = {gamma, save_mean, save_invstd};
    int64_t m = 0;
    const int rc = bn_check(fn, n, h, w, c, x_layout, relu, big, 4, small, 3, workspace, ws_bytes, &m);
    if (rc != SLFP_OK) return rc;
    if (reinterpret_cast<uintptr_t>(gres) & (c % 4 == 0 ? 15 : 3))
        return fail(SLFP_ERR_ALIGNMENT, "%s: gres must be %d-byte aligned", fn, c % 4 == 0 ? 16 : 4);
    if ((reinterpret_cast<uintptr_t>(ggamma) | reinterpret_cast<uintptr_t>(gbeta)) & 3)
        return fail(SLFP_ERR_ALIGNMENT, "%s: ggamma and gbeta must be 4-byte aligned", fn);
    if (gx == x || gx == y || gx == gy) return fail(SLFP_ERR_BAD_ARG, "%s: gx may not alias x, y or gy", fn);
    if (gres && (gres == x || gres == y || gres == gy || gres == gx))
        return fail(SLFP_ERR_BAD_ARG, "%s: gres may not alias x, y, gy or gx", fn);
    if (m == 0) return SLFP_OK;
    const BnSplit s = bn_split(m, c);
    BnArgs a = bn_args(s, m, c, relu, workspace);
    a.x = x; a.y = y; a.gy = gy; a.out = gx; a.gres = gres; a.gamma = gamma; a.mean = save_mean; a.invstd = save_invstd;
    const dim3 grid((unsigned)s.slabs, (unsigned)s.tiles), block(kBnThreads);
    const hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(s.vec == 4 ? k_bn_bwd_reduce<4> : k_bn_bwd_reduce<1>, grid, block, 0, st, a);
    int e = check_launch("slfp batch-norm backward reduce kernel");
    if (e != SLFP_OK) return e;
    hipLaunchKernelGGL(k_bn_bwd_finalize, dim3((unsigned)ceil_div(c, kBnFinCh)), block, 0, st, a, ggamma, gbeta);
    e = check_launch("slfp batch-norm backward finalize kernel");
    if (e != SLFP_OK) return e;
    hipLaunchKernelGGL((s.vec == 4 ? k_bn_bwd_dx<4, false, true> : k_bn_bwd_dx<1, false, true>), grid, block, 0, st, a);
    return check_launch("slfp batch-norm residual backward dx kernel");
}

int slfp_bn_lut_train_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                          float momentum, float eps, const float* act_table, float* y, float* save_mean, float* save_invstd,
                          float* save_lo, int64_t n, int64_t h, int64_t w, int64_t c, int x_layout, void* workspace,
                          size_t ws_bytes, void* stream) {
    const char* fn = "slfp_bn_lut_train_fwd";
    const void* big[] = {x, y};
    const void* small[] = {gamma, beta, save_mean, save_invstd, save_lo};
    int64_t m = 0;
    const int rc = bn_check(fn, n, h, w, c, x_layout, 0, big, 2, small, 5, workspace, ws_bytes, &m, true, act_table);
    if (rc != SLFP_OK) return rc;
    if ((running_mean == nullptr) != (running_var == nullptr))
        return fail(SLFP_ERR_BAD_ARG, "%s: running_mean and running_var are given together or not at all", fn);
    if ((reinterpret_cast<uintptr_t>(running_mean) | reinterpret_cast<uintptr_t>(running_var)) & 3)
        return fail(SLFP_ERR_ALIGNMENT, "%s: the running statistics must be 4-byte aligned", fn);
    if (x == y) return fail(SLFP_ERR_BAD_ARG, "%s: y may not alias x (the backward reads x)", fn);
    if (m == 0) return SLFP_OK;
    const BnSplit s = bn_split(m, c);
    BnArgs a = bn_args(s, m, c, 0, workspace);
    a.x = x; a.out = y; a.gamma = gamma; a.beta = beta; a.mean = save_mean; a.invstd = save_invstd; a.table = act_table;
    a.gmean = save_lo;   // the finalize kernel's lo goes to the caller instead of the workspace; the apply reads it there
    const dim3 grid((unsigned)s.slabs, (unsigned)s.tiles), block(kBnThreads);
    const hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(s.vec == 4 ? k_bn_stats<4> : k_bn_stats<1>, grid, block, 0, st, a);
    int e = check_launch("slfp batch-norm statistics kernel");
    if (e != SLFP_OK) return e;
    hipLaunchKernelGGL(k_bn_finalize, dim3((unsigned)ceil_div(c, kBnFinCh)), block, 0, st, a, running_mean, running_var, momentum,
                       eps, save_mean, save_invstd);
    e = check_launch("slfp batch-norm finalize kernel");
    if (e != SLFP_OK) return e;
    hipLaunchKernelGGL((s.vec == 4 ? k_bn_apply<4, true> : k_bn_apply<1, true>), grid, block, 0, st, a);
    return check_launch("slfp batch-norm table apply kernel");
}

int slfp_bn_lut_train_bwd(const float* x, const float* gy, const float* gamma, const float* beta, const float* save_mean,
                          const float* save_invstd, const float* save_lo, const float* dact_table, float* gx, float* ggamma,
                          float* gbeta, int64_t n, int64_t h, int64_t w, int64_t c, int x_layout, void* workspace,
                          size_t ws_bytes, void* stream) {
    const char* fn = "slfp_bn_lut_train_bwd";
    const void* big[] = {x, gy, gx};
    const void* small[] = {gamma, beta, save_mean, save_invstd, save_lo};
    int64_t m = 0;
    const int rc = bn_check(fn, n, h, w, c, x_layout, 0, big, 3, small, 5, workspace, ws_bytes, &m, true, dact_table);
    if (rc != SLFP_OK) return rc;
    if ((reinterpret_cast<uintptr_t>(ggamma) | reinterpret_cast<uintptr_t>(gbeta)) & 3)
        return fail(SLFP_ERR_ALIGNMENT, "%s: ggamma and gbeta must be 4-byte aligned", fn);
    if (gx == x) return fail(SLFP_ERR_BAD_ARG, "%s: gx may not alias x", fn);
    if (m == 0) return SLFP_OK;
    const BnSplit s = bn_split(m, c);
    BnArgs a = bn_args(s, m, c, 0, workspace);
    a.x = x; a.y = x; a.gy = gy; a.out = gx; a.gamma = gamma; a.beta = beta; a.mean = save_mean; a.invstd = save_invstd;
    a.lo_fwd = save_lo; a.table = dact_table;
    const dim3 grid((unsigned)s.slabs, (unsigned)s.tiles), block(kBnThreads);
    const hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL((s.vec == 4 ? k_bn_bwd_reduce<4, true> : k_bn_bwd_reduce<1, true>), grid, block, 0, st, a);
    int e = check_launch("slfp batch-norm table backward reduce kernel");
    if (e != SLFP_OK) return e;
    hipLaunchKernelGGL(k_bn_bwd_finalize, dim3((unsigned)ceil_div(c, kBnFinCh)), block, 0, st, a, ggamma, gbeta);
    e = check_launch("slfp batch-norm backward finalize kernel");
    if (e != SLFP_OK) return e;
    hipLaunchKernelGGL((s.vec == 4 ? k_bn_bwd_dx<4, true> : k_bn_bwd_dx<1, true>), grid, block, 0, st, a);
    return check_launch("slfp batch-norm table backward dx kernel");
}

}  // extern "C"
