// conv_pw_params.hpp -- what the pointwise (1x1) kernels of conv_pw.hip (and experiments built next to it) share: launch parameters,
// the fp16 tile swizzle and the staged-store helpers (the epilogue arithmetic itself: slfp_epilogue.hpp).
#pragma once
#include "slfp_device.hpp"
#include "slfp_enc.hpp"
#include "slfp_host.hpp"
#include "slfp_epilogue.hpp"

namespace slfp {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));

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


__device__ __forceinline__ float4 bias_q256(const PwParams& p, int n) { return bias_q256(p.bias, n, p.s1, p.s2); }

// 16 bytes of the residual in the layout of the staged store they pair with: same descriptor bounds, same byte offset (an
// out-of-range offset -- rows past M, channels past N -- reads nothing and returns 0)
__device__ __forceinline__ u32x4 res_load_stg(const __amdgpu_buffer_rsrc_t rr, uint32_t so) {
    asm volatile("" : "+v"(so));
    return __builtin_amdgcn_raw_buffer_load_b128(rr, so, 0, (SLFP_NT_PW_RES & 1) ? 2 : 0);
}
__device__ __forceinline__ u32x4 res_add_stg(const u32x4 v, const u32x4 q, const int relu) {
    const float4 r = res_add(make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3])),
                             make_float4(__uint_as_float(q[0]), __uint_as_float(q[1]), __uint_as_float(q[2]), __uint_as_float(q[3])), relu);
    return u32x4{__float_as_uint(r.x), __float_as_uint(r.y), __float_as_uint(r.z), __float_as_uint(r.w)};
}

// 128-byte rows (64 fp16); XOR swizzle so that the 16 rows a fragment read touches hit
// 16 distinct 16-byte slots (conflict-free ds_read_b128; cdna guide T2)
__device__ __forceinline__ uint32_t lds_x_off(int row, int chunk16) {
    return (uint32_t)row * 128u + (uint32_t)((chunk16 ^ (row & 7)) << 4);
}

constexpr int kStgRow = 272;   // 256 B of a row's 64 channels + 16: the 16 rows' float4 writes spread over the banks

}  // namespace slfp
