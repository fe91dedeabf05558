// conv_dense_core.hpp -- what the dense k x k translation units share on the device (conv_dense.hip: dilation 1;
// conv_dense_dil.hip: the phase-tiled dilated family): the fragment type, the swizzled halo-tile address and the LDS-DMA piece.
#pragma once
#include "slfp_device.hpp"

namespace slfp {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ uint32_t dn_x_off(int row, int chunk16) {
    // 128-byte rows; a fragment read touches 16 rows base .. base+15 for ANY base (taps shift it).
    // ds_read_b128 is served in lane groups {0-3,12-15,20-27}, ... = 8 lanes of an even lane-quarter
    // (rows +0..3, +12..15) and 8 of the next odd one (rows +4..11): bit 0 of the chunk (= parity of
    // the lane-quarter) is left alone so the two halves of a group never meet; bits 1-2 are rotated
    // by (row >> 1) & 3, which takes 4 distinct values on each half's 4 same-parity rows; (row & 1)
    // picks the 128-byte half of the 256-byte bank line.  16 distinct slots per group (profiles/
    // r01f_vgg16 measured 18 % conflict cycles with the plain (row >> 1) & 7 rotation).
    return (uint32_t)row * 128u + (uint32_t)((chunk16 ^ (((row >> 1) & 3) << 1)) << 4);
}

__device__ __forceinline__ void glds16(const void* g, void* l) {  // 64 lanes x 16 B -> 1 KiB of LDS at (wave-uniform) l
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}

}  // namespace slfp
