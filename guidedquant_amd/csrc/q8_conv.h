// q8_conv.h -- int8 -> fp16 of the int8 lm_head, once for the decode GEMV (head_q8.hip) and the scoring head (head_nll.hip), gfx950.
// 1.75 VALU instructions per weight: one v_xor turns the four bytes of a dword into biased codes q + 128, two v_perm_b32 place each
// under the high byte 0x64 -- the fp16 number 1024 + (q + 128), exact -- and one v_pk_add_f16 of -1152 per pair gives q itself, exact
// again (|q| <= 128, every intermediate an integer below 2048).  The signed value exists BEFORE the product: nothing biased is
// accumulated, no correction term is subtracted from a sum.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wave_util.h"

namespace gqw {

// the signed fp16 pair of bytes (2 * HI, 2 * HI + 1) of a dword of biased codes (b = q ^ 0x80)
template <int HI>
__device__ __forceinline__ h16x2 q8_pair(uint32_t biased) {
    // v_perm_b32: selector bytes 0..3 take the bytes of the second operand, 4..7 those of the first
    const uint32_t p = __builtin_amdgcn_perm(0x64646464u, biased, HI ? 0x04030402u : 0x04010400u);  // (0x64, b1, 0x64, b0): 1024 + b each
    const h16 off = (h16)-1152.0f;
    return __builtin_bit_cast(h16x2, p) + (h16x2){off, off};
}

// 16 codes (one 16-byte load, ascending columns) -> two 16-byte rows of 8 fp16 integers each, in column order
__device__ __forceinline__ void q8_row16(uint4 c, uint4 &lo, uint4 &hi) {
    const uint32_t b0 = c.x ^ 0x80808080u, b1 = c.y ^ 0x80808080u, b2 = c.z ^ 0x80808080u, b3 = c.w ^ 0x80808080u;
    lo = make_uint4(__builtin_bit_cast(uint32_t, q8_pair<0>(b0)), __builtin_bit_cast(uint32_t, q8_pair<1>(b0)),
                    __builtin_bit_cast(uint32_t, q8_pair<0>(b1)), __builtin_bit_cast(uint32_t, q8_pair<1>(b1)));
    hi = make_uint4(__builtin_bit_cast(uint32_t, q8_pair<0>(b2)), __builtin_bit_cast(uint32_t, q8_pair<1>(b2)),
                    __builtin_bit_cast(uint32_t, q8_pair<0>(b3)), __builtin_bit_cast(uint32_t, q8_pair<1>(b3)));
}

}  // namespace gqw
