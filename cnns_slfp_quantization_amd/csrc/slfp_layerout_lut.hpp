// slfp_layerout_lut.hpp -- the layer-output quantizer's image as a table index (host and device), gfx950.
//
// The blocks of MobileNetV1_swish / VGG16_gelu are [Conv2d_Q, BatchNorm2d, layerout_quantize_func, ReLU | Swish | GELU]
// (nets_cifar/mobilenetv1.py:196-231, nets_cifar/vgg16.py:186-293).  After layerout_bits() (slfp_device.hpp) a float32 has 5
// significant bits and |v| <= 248: a few thousand values per sign.  Everything between that value and the NEXT layer's 1-byte
// code -- a folded ReLU, any elementwise activation module, the reader's quantize_act(. / Ka) -- is a pure function of it, so the
// whole tail of a code-writing epilogue is one byte table:
//     code = T[layerout_class(layerout_bits(affine(conv)))]
// T is built on the host at link time by running the stock modules over layerout_value(i) for every i and encoding the result
// with slfp_encode_f32(., Ka, fmt | SLFP_FMT_EXT) (fusion.link_layerout): bit-identical to the unlinked model for ANY
// elementwise activation, with no device sigmoid / erf and no reader-side threshold table.
//
// Index layout (kLayeroutClasses = 4927 slots, padded to kLayeroutLutBytes = 4928):
//     0                 NaN (layerout of an exact zero, or of a NaN) -- one class whatever the payload
//     k = 1 .. 2463     positive values, by magnitude a = bits & 0x7FFFFFFF:
//         1 .. 31         a = k                       denormals with at most 5 significant bits at the bottom of the field
//         32 .. 319       a = m << sh, k = 16 sh + m   denormals with leading bit 4 + sh (sh = 1 .. 18), m = 16 .. 31: the 5
//                                                      kept bits sit at ANY position, so a >> 19 cannot tell them apart
//         320 .. 2463     a = (k - 304) << 19          normals: a >> 19 = exponent << 4 | 4 mantissa bits = 16 .. 0x86F (248)
//     2463 + k          the same magnitudes with the sign bit set
// layerout_class is injective on the whole image of layerout_bits (slfp_debug_layerout_lut_mismatches sweeps all 2^32 inputs
// on the device); layerout_value is its inverse.  Normals take a shift, an add and the sign; denormals a cold branch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "slfp_device.hpp"
#include "slfp_enc.hpp"

#include "../../include/slfp.h"   // SLFP_LAYEROUT_LUT_BYTES: the table size in bytes (the classes, padded to a multiple of 16)

namespace slfp {

constexpr int kLayeroutSide = 2463;                       // slots per sign
constexpr int kLayeroutClasses = 1 + 2 * kLayeroutSide;   // + the NaN slot
constexpr int kLayeroutLutBytes = SLFP_LAYEROUT_LUT_BYTES;
static_assert(kLayeroutLutBytes % 16 == 0 && kLayeroutLutBytes >= kLayeroutClasses && kLayeroutLutBytes <= 8192, "padded table size");

// index of v = layerout_bits(u); v must lie in the image (any NaN is class 0)
__host__ __device__ __forceinline__ uint32_t layerout_class(uint32_t v) {
    const uint32_t a = v & 0x7FFFFFFFu;
    uint32_t k = (a >> 19) + 304u;
    if (a < 0x00800000u) {   // denormal (rare path)
        k = a;
        if (a >= 32u) {
            const uint32_t sh = (uint32_t)(31 - __builtin_clz(a)) - 4u;
            k = 16u * sh + (a >> sh);
        }
    }
    k += (v >> 31) * (uint32_t)kLayeroutSide;
    return a > 0x7F800000u ? 0u : k;
}

// float32 bits of class i: the inverse of layerout_class; padding slots (i >= kLayeroutClasses) give +0
__host__ __device__ __forceinline__ uint32_t layerout_value(uint32_t i) {
    if (i == 0u) return kBitsQNaN;
    if (i >= (uint32_t)kLayeroutClasses) return 0u;
    const uint32_t s = i > (uint32_t)kLayeroutSide ? 0x80000000u : 0u;
    const uint32_t k = s ? i - (uint32_t)kLayeroutSide : i;
    uint32_t a;
    if (k < 32u) a = k;
    else if (k < 320u) { const uint32_t sh = (k - 16u) >> 4; a = (k - 16u * sh) << sh; }
    else a = (k - 304u) << 19;
    return a | s;
}

// ---- device side: the table epilogue of the code-writing (YC) kernels ------------------------------------------------
// The table reaches a kernel as a device pointer.  The LUT instantiations have no use for the reader's threshold table, so the
// pointer travels in the first entry of the EncArgs / EncArgsCompact the kernel's parameter block already holds: the
// kernel-argument layout of every existing instantiation stays what it was.
template <typename ENC>
inline void enc_carry_ptr(ENC& e, const void* ptr) {
    static_assert(sizeof(e.e[0]) == sizeof(void*), "one table entry holds a pointer");
    __builtin_memcpy(&e.e[0], &ptr, sizeof(void*));
}
typedef const __attribute__((address_space(1))) unsigned char* lut_gptr;   // read through the vector cache (global_load_ubyte)
template <typename ENC>
__device__ __forceinline__ lut_gptr enc_carried_ptr(const ENC& e) {
    const uint64_t v = (uint64_t)e.e[0].x | ((uint64_t)e.e[0].y << 32);
    return (lut_gptr)v;
}

// copies the table into LDS (kLayeroutLutBytes, 16-byte aligned); the caller's next __syncthreads() publishes it
template <int NT>
__device__ __forceinline__ void layerout_lut_fill(unsigned char* sLut, lut_gptr g) {
    typedef uint32_t u32x4l __attribute__((ext_vector_type(4)));
    for (int i = threadIdx.x; i < kLayeroutLutBytes / 16; i += NT)
        reinterpret_cast<u32x4l*>(sLut)[i] = reinterpret_cast<const __attribute__((address_space(1))) u32x4l*>(g)[i];
}

// 4 values after the affine -> layerout, class, one byte load each; packed like enc4_code (byte k = element k).  TAB: an LDS
// array (ds_read_u8) or a lut_gptr.  Whole-register shifts and ors: no sub-dword VALU writes, so no SDWA forwarding hazard.
template <typename TAB>
__device__ __forceinline__ uint32_t lut4_code(const float4 t, TAB tab) {
    const uint32_t b0 = tab[layerout_class(layerout_bits(__float_as_uint(t.x)))];
    const uint32_t b1 = tab[layerout_class(layerout_bits(__float_as_uint(t.y)))];
    const uint32_t b2 = tab[layerout_class(layerout_bits(__float_as_uint(t.z)))];
    const uint32_t b3 = tab[layerout_class(layerout_bits(__float_as_uint(t.w)))];
    return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
}

}  // namespace slfp
