// conv_pw_params.hpp -- what the pointwise (1x1) kernels of conv_pw.hip (and experiments built next to it) share: launch parameters,
// the fp16 tile swizzle and the epilogue arithmetic of Conv2d_Q.forward (utils/conv2d_func.py:23-24).
#pragma once
#include "slfp_device.hpp"
#include "slfp_enc.hpp"
#include "slfp_host.hpp"

namespace slfp {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

struct PwParams {
    const float* x;
    const _Float16* whi;
    const _Float16* wlo;
    const float* bias;
    float* y;
    int64_t M;        // output pixels = N_img * Ho * Wo
    int K, N;         // input / output channels
    int KS;           // number of 32-deep k-steps in the blob (even)
    int n_tiles;      // 16-row tiles in the blob (n_pad / 16)
    int H, W, Ho, Wo, S;  // strided 1x1: input pixel = (oh*S, ow*S)
    ScaleDiv sd;          // divides by Ka/16
    float s1, s2;         // out = ((acc/256 + bias/s1/s2) * s1) * s2 ; s1x = s1/256
    float s1x;
    uint32_t m_blocks, n_blocks, nblocks;
    int rb;               // k_pw_tiled: pixel rows a workgroup really owns (<= BM; the rest of its tile is padding)
    int nt_out;           // staged (whole-line) stores carry the nt hint: outputs too large for the Infinity Cache
    const float* res;     // RES kernels: the residual operand, NHWC like y (y = relu?(affine(conv) + res)); nullptr otherwise
    PostOp post;
    EncArgs enc;          // threshold table of fp16(16 * QA(x / Ka)) (TAB kernels; slfp_enc.hpp)
    EncArgsCompact enc_lo;   // three-pass TAB kernels: the residual plane's table (kEncF16LO) of the same scale;
                             // YC kernels (single-pass): the code table of the consumer's Ka (kEncCode), same compact form
#ifdef SLFP_PW_STAMPS
    unsigned long long* dbg;   // diagnostic builds only (profiles/stamps_tiled.py): 16 x s_memrealtime per workgroup
#endif
    int sgn;              // YC: no ReLU in front of the output quantizer: codes carry a sign
    int fmt_out;          // YC: format of the output codes (kFmtAct8 | kFmtSfp7)
    uint8_t* yc;          // YC kernels (slfp_conv2d_fwd_entry): the uint8 code tensor, NHWC, C_out bytes per pixel; nullptr otherwise
};
// passed by value: the kernel-argument segment holds 4 KiB.  A second full EncArgs (2 KiB) would not fit next to `enc`.
static_assert(sizeof(PwParams) <= 4096, "PwParams must fit the 4 KiB kernel-argument segment");

#ifdef SLFP_PW_STAMPS
#define SLFP_STAMP(i) do { if (p.dbg && threadIdx.x == 0) p.dbg[(size_t)blockIdx.x * 16 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define SLFP_STAMP(i) do { } while (0)
#endif

constexpr int kPwTab = (kEncEntries * 8 + 15) & ~15;   // LDS bytes of the threshold table


// out = ((acc * 2^-8 + bq) * s1) * s2 with the 2^-8 folded: ((acc + 256*bq) * (s1/256)) * s2
__device__ __forceinline__ float4 epilogue(const floatx4 acc, const float4 bq256, const float s1x, const float s2) {
    float4 r;
    r.x = ((acc[0] + bq256.x) * s1x) * s2;
    r.y = ((acc[1] + bq256.y) * s1x) * s2;
    r.z = ((acc[2] + bq256.z) * s1x) * s2;
    r.w = ((acc[3] + bq256.w) * s1x) * s2;
    return r;
}

__device__ __forceinline__ float4 bias_q256(const PwParams& p, int n) {
    if (!p.bias) return make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 bb = *reinterpret_cast<const float4*>(p.bias + n);
    return make_float4(256.f * ((bb.x / p.s1) / p.s2), 256.f * ((bb.y / p.s1) / p.s2),
                       256.f * ((bb.z / p.s1) / p.s2), 256.f * ((bb.w / p.s1) / p.s2));
}

// The residual epilogue (slfp_conv2d_fwd_res): t = r + q, one float32 add AFTER the affine's rounding (the library is built
// with -ffp-contract=off, so the add never merges into the fma in front of it), then the ReLU's max: what torch.add and
// torch.relu compute on the unfused result.
__device__ __forceinline__ float4 res_add(float4 r, const float4 q, const int relu) {
    r.x = r.x + q.x; r.y = r.y + q.y; r.z = r.z + q.z; r.w = r.w + q.w;
    if (relu) { r.x = fmaxf(r.x, 0.f); r.y = fmaxf(r.y, 0.f); r.z = fmaxf(r.z, 0.f); r.w = fmaxf(r.w, 0.f); }
    return r;
}

typedef uint32_t u32x4r __attribute__((ext_vector_type(4)));
// 16 bytes of the residual in the layout of the staged store they pair with: same descriptor bounds, same byte offset (an
// out-of-range offset -- rows past M, channels past N -- reads nothing and returns 0)
__device__ __forceinline__ u32x4r res_load_stg(const __amdgpu_buffer_rsrc_t rr, uint32_t so) {
    asm volatile("" : "+v"(so));
    return __builtin_amdgcn_raw_buffer_load_b128(rr, so, 0, (SLFP_NT_PW_RES & 1) ? 2 : 0);
}
__device__ __forceinline__ u32x4r res_add_stg(const u32x4r v, const u32x4r q, const int relu) {
    const float4 r = res_add(make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3])),
                             make_float4(__uint_as_float(q[0]), __uint_as_float(q[1]), __uint_as_float(q[2]), __uint_as_float(q[3])), relu);
    return u32x4r{__float_as_uint(r.x), __float_as_uint(r.y), __float_as_uint(r.z), __float_as_uint(r.w)};
}

// 128-byte rows (64 fp16); XOR swizzle so that the 16 rows a fragment read touches hit
// 16 distinct 16-byte slots (conflict-free ds_read_b128; cdna guide T2)
__device__ __forceinline__ uint32_t lds_x_off(int row, int chunk16) {
    // 128-byte rows (64 fp16); XOR swizzle so that the 16 rows a fragment read touches hit
    // 16 distinct 16-byte slots (conflict-free ds_read_b128; cdna guide T2)
    return (uint32_t)row * 128u + (uint32_t)((chunk16 ^ (row & 7)) << 4);
}

constexpr int kStgRow = 272;   // 256 B of a row's 64 channels + 16: the 16 rows' float4 writes spread over the banks

}  // namespace slfp
