// optim.hip -- the reference's quantization-aware SGD step (utils/optimizer.py: DSGD, SSGD, NormalSGD) as one
// multi-tensor HIP pass per launch (gfx950).
//
// The reference runs ~20 full-tensor ATen ops per parameter (clones, two weight quantizers, a masked scale and four
// scalar mul / add passes).  Here every element is loaded once, stepped in registers -- including both SLFP weight
// quantizations, through the same quant_bits<FMT> the codec kernels use (slfp_device.hpp) at unit scale -- and stored
// once: 24 B per element with weight decay and momentum (read p, g, buf; write p, g, buf).  Each line of the step
// (include/slfp.h) is its own float32 rounding, in the reference's order; the a + alpha * b terms
// of ATen's add(alpha=) are one fused multiply-add, which is what ATen's ROCm build runs (measured).
//
// One launch takes up to kOptMaxTensors tensors, passed by value in the kernel arguments (no device allocation, no
// host-to-device copy).  The tensors are cut into chunks of kOptChunk elements; chunk_end[t] is the running chunk
// count, so the (tensor, chunk) pairs of the launch are numbered 0 .. chunk_end[T-1] - 1 and every workgroup walks
// its share of them, grid-stride, with the tensor index found by a wave-uniform forward scan.
#include "slfp_device.hpp"
#include "slfp_host.hpp"

namespace slfp {

constexpr int kOptThreads = 256;
constexpr int kOptMaxTensors = 48;   // 48 x 37 B + 32 B = 1.8 KiB of kernel arguments (limit 4 KiB)
constexpr int64_t kOptChunk = 4096;  // elements per (tensor, chunk) pair: 4 float4 per thread
constexpr uint32_t kOptFirst = 1u;   // flags: buf := g (this is the step that creates the buffer; buf is not read)
constexpr uint32_t kOptVec = 2u;     //        p, g and buf all 16-byte aligned

struct OptHyper {
    float lr, momentum, damp_alpha, weight_decay;
    int32_t use_wd, use_mom, nesterov, reserved;
};

struct OptArgs {
    OptHyper h;
    float* p[kOptMaxTensors];
    float* g[kOptMaxTensors];
    float* buf[kOptMaxTensors];
    int64_t numel[kOptMaxTensors];
    uint32_t chunk_end[kOptMaxTensors];
    uint8_t flags[kOptMaxTensors];
};
static_assert(sizeof(OptArgs) <= 2048, "keep the kernel arguments well under the 4 KiB limit");

constexpr int kRuleSgd = SLFP_OPT_SGD, kRuleDsgd = SLFP_OPT_DSGD, kRuleSsgd = SLFP_OPT_SSGD;
constexpr int kFmtNone = -1;  // qbits 32: Q is the identity

// ATen's `a + alpha * b` (add with alpha): a single rounding.
__device__ __forceinline__ float add_alpha(float a, float alpha, float b) { return __builtin_fmaf(alpha, b, a); }

template <int FMT>
__device__ __forceinline__ float qw(float x, const uint32_t* __restrict__ sT) {
    if constexpr (FMT == kFmtNone) return x;
    else return __uint_as_float(quant_bits<FMT>(__float_as_uint(x), __float_as_uint(x), sT));
}

// One element of the step.  `g` and `b` are updated in place (the caller stores them as the flags say).
template <int RULE, int FMT>
__device__ __forceinline__ float step1(float p, float& g, float& b, bool first, const OptHyper& h,
                                       const uint32_t* __restrict__ sT) {
    if (h.use_wd) g = add_alpha(g, h.weight_decay, p);
    float d = g;
    if (h.use_mom) {
        b = first ? g : add_alpha(b * h.momentum, h.damp_alpha, g);
        d = h.nesterov ? add_alpha(g, h.momentum, b) : b;
    }
    const float t = d * -h.lr;
    if constexpr (RULE == kRuleSgd) {
        return p + t;
    } else {
        float s;
        float wb = 0.f;
        if constexpr (RULE == kRuleDsgd) wb = qw<FMT>(p, sT);
        p = p + t;
        if constexpr (RULE == kRuleDsgd) {
            const float diff = fabsf(wb - qw<FMT>(p, sT));
            // 0 where diff > 1e-4, 2 where diff < 1e-4, and 0 where neither holds (equality, NaN)
            s = diff < 1e-4f ? 2.f : 0.f;
        } else {
            s = fabsf(p) + 1.f;
        }
        return p + t * s;
    }
}

template <int RULE, int FMT>
__device__ __forceinline__ float4 step4(float4 p, float4& g, float4& b, bool first, const OptHyper& h,
                                        const uint32_t* __restrict__ sT) {
    float4 r;
    r.x = step1<RULE, FMT>(p.x, g.x, b.x, first, h, sT);
    r.y = step1<RULE, FMT>(p.y, g.y, b.y, first, h, sT);
    r.z = step1<RULE, FMT>(p.z, g.z, b.z, first, h, sT);
    r.w = step1<RULE, FMT>(p.w, g.w, b.w, first, h, sT);
    return r;
}

template <int RULE, int FMT>
__global__ __launch_bounds__(kOptThreads) void k_sgd_step(const OptArgs a) {
    __shared__ uint32_t sT[16];
    if constexpr (FMT != kFmtNone) {
        lut_fill<FMT>(sT);
        __syncthreads();
    }
    const OptHyper& h = a.h;
    const uint32_t nchunks = a.chunk_end[kOptMaxTensors - 1];
    int t = 0;
    for (uint32_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        while (c >= a.chunk_end[t]) ++t;  // wave-uniform; chunks are visited in increasing order
        const uint32_t c0 = t == 0 ? 0u : a.chunk_end[t - 1];
        const int64_t e0 = (int64_t)(c - c0) * kOptChunk;
        const int64_t n = a.numel[t];
        const int64_t e1 = e0 + kOptChunk < n ? e0 + kOptChunk : n;
        const uint32_t fl = a.flags[t];
        const bool first = fl & kOptFirst;
        float* __restrict__ p = a.p[t];
        float* __restrict__ g = a.g[t];
        float* __restrict__ buf = a.buf[t];
        int64_t i0 = e0;
        if (fl & kOptVec) {
            const int64_t nv = (e1 - e0) >> 2;  // e0 is a multiple of 4
            for (int64_t j = threadIdx.x; j < nv; j += kOptThreads) {
                const int64_t i = e0 + 4 * j;
                const float4 pv = *reinterpret_cast<const float4*>(p + i);
                float4 gv = *reinterpret_cast<const float4*>(g + i);
                float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
                if (h.use_mom && !first) bv = *reinterpret_cast<const float4*>(buf + i);
                const float4 r = step4<RULE, FMT>(pv, gv, bv, first, h, sT);
                *reinterpret_cast<float4*>(p + i) = r;
                if (h.use_wd) *reinterpret_cast<float4*>(g + i) = gv;
                if (h.use_mom) *reinterpret_cast<float4*>(buf + i) = bv;
            }
            i0 = e0 + 4 * nv;
        }
        // scalar tail of the last chunk, or the whole chunk when a pointer is not 16-byte aligned
        for (int64_t i = i0 + threadIdx.x; i < e1; i += kOptThreads) {
            float gv = g[i];
            float bv = (h.use_mom && !first) ? buf[i] : 0.f;
            const float r = step1<RULE, FMT>(p[i], gv, bv, first, h, sT);
            p[i] = r;
            if (h.use_wd) g[i] = gv;
            if (h.use_mom) buf[i] = bv;
        }
    }
}

template <int RULE, int FMT>
static int launch_sgd(const OptArgs& a, int grid, hipStream_t st) {
    hipLaunchKernelGGL((k_sgd_step<RULE, FMT>), dim3(grid), dim3(kOptThreads), 0, st, a);
    return check_launch("slfp sgd step kernel");
}

static int launch_sgd_any(int rule, int qbits, const OptArgs& a, int grid, hipStream_t st) {
    if (rule == kRuleSgd) return launch_sgd<kRuleSgd, kFmtNone>(a, grid, st);
    if (rule == kRuleSsgd) return launch_sgd<kRuleSsgd, kFmtNone>(a, grid, st);
    if (qbits == 8) return launch_sgd<kRuleDsgd, kFmtW8>(a, grid, st);
    if (qbits == 7) return launch_sgd<kRuleDsgd, kFmtSfp7>(a, grid, st);
    return launch_sgd<kRuleDsgd, kFmtNone>(a, grid, st);
}

}  // namespace slfp

using namespace slfp;

extern "C" int slfp_sgd_step_f32(const slfp_sgd_hparams* h, size_t ntensors, float* const* param, float* const* grad,
                                 float* const* momentum_buf, const int64_t* numel, const uint8_t* first_step, void* stream) {
    // every argument is validated before the first HIP call
    if (!h) return fail(SLFP_ERR_BAD_ARG, "slfp_sgd_step_f32: null hparams");
    if (h->rule != SLFP_OPT_SGD && h->rule != SLFP_OPT_DSGD && h->rule != SLFP_OPT_SSGD)
        return fail(SLFP_ERR_BAD_ARG, "slfp_sgd_step_f32: unknown rule %d", h->rule);
    if (h->qbits != 8 && h->qbits != 7 && h->qbits != 32)
        return fail(SLFP_ERR_BAD_ARG, "slfp_sgd_step_f32: qbits must be 8, 7 or 32, got %d", h->qbits);
    if (h->nesterov != 0 && h->nesterov != 1) return fail(SLFP_ERR_BAD_ARG, "slfp_sgd_step_f32: nesterov must be 0 or 1");
    const bool use_mom = h->momentum != 0.f;
    if (h->nesterov && !use_mom) return fail(SLFP_ERR_BAD_ARG, "slfp_sgd_step_f32: nesterov needs a momentum");
    if (ntensors == 0) return SLFP_OK;
    if (!param || !grad || !numel || !first_step) return fail(SLFP_ERR_BAD_ARG, "slfp_sgd_step_f32: null array");
    if (use_mom != (momentum_buf != nullptr))
        return fail(SLFP_ERR_BAD_ARG, "slfp_sgd_step_f32: momentum_buf must be non-NULL exactly when momentum != 0");
    for (size_t i = 0; i < ntensors; ++i) {
        if (numel[i] < 0 || numel[i] > ((int64_t)1 << 40))
            return fail(SLFP_ERR_BAD_ARG, "slfp_sgd_step_f32: numel[%zu] = %lld out of range", i, (long long)numel[i]);
        if (numel[i] == 0) continue;
        if (!param[i] || !grad[i] || (use_mom && !momentum_buf[i]))
            return fail(SLFP_ERR_BAD_ARG, "slfp_sgd_step_f32: null pointer for tensor %zu", i);
    }

    OptArgs a;
    a.h.lr = h->lr;
    a.h.momentum = h->momentum;
    a.h.damp_alpha = h->damp_alpha;
    a.h.weight_decay = h->weight_decay;
    a.h.use_wd = h->weight_decay != 0.f;
    a.h.use_mom = use_mom;
    a.h.nesterov = h->nesterov;
    a.h.reserved = 0;
    hipStream_t st = as_stream(stream);
    const int64_t grid_cap = (int64_t)device_cu_count() * 8;  // 8 workgroups per CU, grid-stride the rest
    size_t i = 0;
    while (i < ntensors) {
        int nt = 0;
        int64_t chunks = 0;
        for (; i < ntensors && nt < kOptMaxTensors; ++i) {
            if (numel[i] == 0) continue;
            const int64_t c = ceil_div(numel[i], kOptChunk);
            if (nt > 0 && chunks + c > (int64_t)INT32_MAX) break;  // chunk numbers stay within 31 bits per launch
            float* b = use_mom ? momentum_buf[i] : nullptr;
            a.p[nt] = param[i];
            a.g[nt] = grad[i];
            a.buf[nt] = b;
            a.numel[nt] = numel[i];
            chunks += c;
            a.chunk_end[nt] = (uint32_t)chunks;
            const bool vec = aligned16(param[i]) && aligned16(grad[i]) && (!b || aligned16(b));
            a.flags[nt] = (uint8_t)((first_step[i] ? kOptFirst : 0u) | (vec ? kOptVec : 0u));
            ++nt;
        }
        if (nt == 0) break;
        for (int k = nt; k < kOptMaxTensors; ++k) {  // unused slots: empty, after the last chunk
            a.p[k] = a.g[k] = a.buf[k] = nullptr;
            a.numel[k] = 0;
            a.chunk_end[k] = (uint32_t)chunks;
            a.flags[k] = 0;
        }
        const int grid = (int)(chunks < grid_cap ? chunks : grid_cap);
        const int rc = launch_sgd_any(h->rule, h->qbits, a, grid, st);
        if (rc != SLFP_OK) return rc;
    }
    return SLFP_OK;
}
