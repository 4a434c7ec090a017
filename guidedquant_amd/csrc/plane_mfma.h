// plane_mfma.h -- the device pieces of the plane arithmetic (plane_core.h: the algorithm, the index math, host-compilable) that the
// three fast-mode kernels share: ap_plane_kernel, ap_plane_local_kernel (ap_plane.hip) and ap_stream_kernel (ap_stream.hip).
// Device only; what differs between the kernels (hot_step / hot_unit / hot_append, epilogues, image builders, LDS layouts) stays
// in their files.
#pragma once
#include "plane_core.h"
#include "wave_util.h"

namespace gqp {

using gqw::h2v;
using gqw::v4f;
using gqw::v4i;
using gqw::v8i;

// The scaled MFMA with A = FP4 (4 registers; the upper half of the builtin's 8-register vector is ignored for cbsz = 4),
// B = BF8.  Through the BUILTIN, not inline asm: the compiler must see the instruction to insert the MFMA hazard wait
// states.  An asm version with a tied accumulator was tried (the register allocator otherwise lets vDst != SrcC wander):
// no faster, and unsafe -- the compiler copied accumulators between registers right behind an MFMA it could not see.
__device__ __forceinline__ void mfma_f4_bf8(v4f &acc, v4i a, v8i b, int scale_a, int scale_b) {
    const v8i a8 = __builtin_shufflevector(a, a, 0, 1, 2, 3, -1, -1, -1, -1);
    acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8, b, acc, 4, 1, 0, scale_a, 0, scale_b);
}

// The defining step of the mode (plane_core.h "activation pieces"): an fp16 value, already multiplied by the power of two of its
// vector / unit, splits EXACTLY into 4 bf8 pieces by truncate-and-subtract in fp16 arithmetic.
// One value: byte p of the result = piece p.
__device__ __forceinline__ u32 bf8_split(uint16_t xh, uint16_t k16) {  // the pieces of x * 2^k, both as fp16 bit patterns
    _Float16 rem = __builtin_bit_cast(_Float16, xh) * __builtin_bit_cast(_Float16, k16);
    u32 pieces = 0;
#pragma unroll
    for (u32 p = 0; p < 4; p++) {
        const uint16_t pb = __builtin_bit_cast(uint16_t, rem) & 0xFF00u;
        pieces |= (u32)(pb >> 8) << (8u * p);
        rem = rem - __builtin_bit_cast(_Float16, pb);
    }
    return pieces;
}
// ---- extracted ("hot") activations: the elements above GQ_HOT_T x the mean magnitude of their vector (ap_plane.hip) or unit
// (ap_stream.hip) leave the image and are multiplied on their own; the story is told in ap_plane.hip.  An entry: the position
// (the kernel's own key layout) and the 4 bf8 pieces of x * 2^ksh (bf8_split: byte p = piece p).
struct HotEnt {
    u32 key, pieces;
};
#define GQ_HOT_T 64.0f
#ifndef HOT_ABL
#define HOT_ABL 0  // ablation experiments (build-time): 1 no threshold, 2 no detection, 4 no extra MFMA sets
#endif
// threshold of the extraction as an fp16 bit pattern (rounded up): GQ_HOT_T x the mean magnitude, 1 % above it for the roundings of
// the estimate (sum1 = sum |x| over K elements)
__device__ __forceinline__ u32 hot_tau_bits(float sum1, float K) {
#if HOT_ABL & 1
    return 0x7C00u;
#endif
    // the hardware reciprocal (1 ulp) is plenty next to the 1 % margin
    const float tau = GQ_HOT_T * 1.01f * sum1 * __builtin_amdgcn_rcpf(K);
    if (!(tau < 65000.f)) return 0x7C00u;  // nothing exceeds +inf: no extraction
    return (u32)__builtin_bit_cast(uint16_t, (_Float16)tau) + 1u;
}

// F.silu(gate) * up on two packed fp16 pairs -- inference/model.py:266
__device__ __forceinline__ u32 silu_mul2(u32 gw, u32 uw) {
    _Float16 hh[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const float gv = gqw::h2f((uint16_t)(gw >> (16 * k)));
        hh[k] = (_Float16)(gv / (1.0f + __expf(-gv))) * __builtin_bit_cast(_Float16, (uint16_t)(uw >> (16 * k)));
    }
    return (u32)__builtin_bit_cast(uint16_t, hh[0]) | ((u32)__builtin_bit_cast(uint16_t, hh[1]) << 16);
}

}  // namespace gqp
