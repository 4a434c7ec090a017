// decode_util.h -- the fp16 bit casts and the wave reduction that decode.hip (attention, dense GEMV) and sampler.hip share
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gq_dec {

typedef uint32_t u32;
typedef _Float16 h16;

__device__ __forceinline__ float h2f(uint16_t h) { return (float)__builtin_bit_cast(h16, h); }
__device__ __forceinline__ h16 u2h(uint16_t h) { return __builtin_bit_cast(h16, h); }
__device__ __forceinline__ uint16_t h2u(h16 h) { return __builtin_bit_cast(uint16_t, h); }

template <bool MAX>
__device__ __forceinline__ float wave_reduce(float v) {
    auto comb = [](float a, float b) { return MAX ? fmaxf(a, b) : a + b; };
    v = comb(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false)));
    v = comb(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false)));
    v = comb(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, false)));
    v = comb(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, false)));
    // row_bcast15 -> rows 1,3 ; row_bcast31 -> rows 2,3 ; lanes not written keep `old` = identity for the combine
    const float ident = MAX ? -3.0e38f : 0.f;
    v = comb(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, ident), __builtin_bit_cast(int, v), 0x142, 0xA, 0xF, false)));
    v = comb(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, ident), __builtin_bit_cast(int, v), 0x143, 0xC, 0xF, false)));
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

}  // namespace gq_dec
