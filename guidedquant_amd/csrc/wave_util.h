// wave_util.h -- the device helpers every kernel file shares, each defined once: the fp16 bit casts, the vector types, the wave and
// row reductions (one name per contract), the raw-buffer descriptor and the hand-issued vector-memory requests.  Device only.
// Kernel files keep their short spellings through using-declarations (using gqw::h2f; ...) or `using namespace gqw;`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace gqw {

// ------------------------------------------------------------------------------------------------ vector types
typedef _Float16 h16;
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));  // (the same type as v4f: both spellings are in use)
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 h2v __attribute__((ext_vector_type(2)));
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));  // (= h2v)
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));  // (= h16x8)
typedef uint16_t us2 __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------------------------------------ fp16 bit casts
__device__ __forceinline__ float h2f(uint16_t h) { return (float)__builtin_bit_cast(h16, h); }
__device__ __forceinline__ uint16_t f2h(float f) { return __builtin_bit_cast(uint16_t, (h16)f); }
__device__ __forceinline__ h16 u2h(uint16_t h) { return __builtin_bit_cast(h16, h); }
__device__ __forceinline__ uint16_t h2u(h16 h) { return __builtin_bit_cast(uint16_t, h); }
__device__ __forceinline__ h2v u2h2(uint32_t u) { return __builtin_bit_cast(h2v, u); }  // a packed pair
__device__ __forceinline__ uint32_t h22u(h2v h) { return __builtin_bit_cast(uint32_t, h); }

// ------------------------------------------------------------------------------------------------ reductions
// All of them are fixed DPP trees (no LDS round trip, deterministic order).  The forms differ in the `old` operand of their DPP moves
// (what a lane without a source reads) and in who holds the result; they are NOT interchangeable at the instruction level, and
// kernels that must agree bit for bit use the same one.

// wave_reduce_l63: sum or maximum over the 64 lanes; the result is valid in LANE 63 ONLY (lane63() fetches it).  The xor steps
// inside a row of 16 read the lane's own value as `old`; the row_bcast steps read 0 where no row is broadcast.  MAX therefore
// REQUIRES NON-NEGATIVE inputs (magnitudes): 0 is its identity.  Users: ap_plane.hip, ap_stream.hip.
template <bool MAX>
__device__ __forceinline__ float wave_reduce_l63(float v) {
    auto step = [&](auto dpp) {
        float o = __builtin_bit_cast(float, dpp(__builtin_bit_cast(int, v)));
        v = MAX ? fmaxf(v, o) : v + o;
    };
    step([](int x) { return __builtin_amdgcn_update_dpp(x, x, 0xB1, 0xF, 0xF, false); });   // quad_perm [1,0,3,2]
    step([](int x) { return __builtin_amdgcn_update_dpp(x, x, 0x4E, 0xF, 0xF, false); });   // quad_perm [2,3,0,1]
    step([](int x) { return __builtin_amdgcn_update_dpp(x, x, 0x141, 0xF, 0xF, false); });  // row_half_mirror
    step([](int x) { return __builtin_amdgcn_update_dpp(x, x, 0x140, 0xF, 0xF, false); });  // row_mirror
    {   // row_bcast15 into rows 1 and 3, row_bcast31 into rows 2 and 3 (0 elsewhere: the identity of the sum and of a maximum of magnitudes)
        float o = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xA, 0xF, false));
        v = MAX ? fmaxf(v, o) : v + o;
        o = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x143, 0xC, 0xF, false));
        v = MAX ? fmaxf(v, o) : v + o;
    }
    return v;
}
__device__ __forceinline__ float lane63(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63)); }

// wave_reduce_bcast: sum or maximum over the 64 lanes, returned in EVERY lane (a readlane of lane 63: the value is wave-uniform).
// `old` is 0 in the row steps and the identity (-3e38 for MAX, 0 for the sum) in the row_bcast steps: MAX takes inputs of either
// sign, down to -3e38.  Users: decode.hip, sampler.hip.
template <bool MAX>
__device__ __forceinline__ float wave_reduce_bcast(float v) {
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

// wave_allsum: the sum over the 64 lanes, in EVERY lane, without the LDS crossbar and without a readlane: quad_perm / row mirrors (DPP
// operands of the adds) inside a row of 16, v_permlane16_swap / v_permlane32_swap across rows.  (Round 6: six ds_bpermute + wait + add
// per statistic -- what __shfl_xor compiles to -- sat between the activations' arrival and the first normalised value of every RMSNorm
// launch.)  The exact / dq GEMV kernels and the QTIP prologues take their RMSNorm statistic through it (kernels that must agree bit
// for bit do).
__device__ __forceinline__ float wave_allsum(float v) {
    auto dpp = [](float x, auto ctrl) {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), decltype(ctrl)::value, 0xF, 0xF, false));
    };
    v += dpp(v, std::integral_constant<int, 0xB1>{});   // quad_perm [1,0,3,2]
    v += dpp(v, std::integral_constant<int, 0x4E>{});   // quad_perm [2,3,0,1]
    v += dpp(v, std::integral_constant<int, 0x141>{});  // row_half_mirror
    v += dpp(v, std::integral_constant<int, 0x140>{});  // row_mirror
    const uint32_t b16 = __builtin_bit_cast(uint32_t, v);
    auto r16 = __builtin_amdgcn_permlane16_swap(b16, b16, false, false);
    v = __builtin_bit_cast(float, (uint32_t)r16[0]) + __builtin_bit_cast(float, (uint32_t)r16[1]);
    const uint32_t b32 = __builtin_bit_cast(uint32_t, v);
    auto r32 = __builtin_amdgcn_permlane32_swap(b32, b32, false, false);
    return __builtin_bit_cast(float, (uint32_t)r32[0]) + __builtin_bit_cast(float, (uint32_t)r32[1]);
}

// row_sum<LANES>: the sum over each aligned group of LANES = 4, 8 or 16 lanes of a DPP row (xor butterflies: quad_perm, quad_perm,
// row_half_mirror, row_mirror); EVERY lane of the group gets the result -- no row_bcast steps, no readlane.
template <int LANES>
__device__ __forceinline__ float row_sum(float v) {
    static_assert(LANES == 4 || LANES == 8 || LANES == 16, "a group of 4, 8 or 16 lanes");
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false));
    if constexpr (LANES >= 8) v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, false));
    if constexpr (LANES >= 16) v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, false));
    return v;
}

// ------------------------------------------------------------------------------------------------ raw-buffer descriptor
// Raw buffer: stride 0, num_records = bytes; a request at or past `bytes` (the kernels use offset 0x80000000 for "no request")
// returns 0 and touches no memory.  Word 3, the same in every descriptor of the library:
constexpr uint32_t RSRC_FLAGS = 0x00020000u;
typedef __amdgpu_buffer_rsrc_t rsrc_t;
// the descriptor for the compiler's buffer builtins ...
__device__ __forceinline__ rsrc_t make_rsrc(const void *p, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), (short)0, (int)bytes, (int)RSRC_FLAGS);
}
// ... and as four SGPRs for the asm requests below
__device__ __forceinline__ u32x4 make_rsrc4(const void *p, uint32_t bytes) {
    const uint64_t a = (uint64_t)(uintptr_t)p;
    return (u32x4){(uint32_t)a, (uint32_t)(a >> 32) & 0xFFFFu, bytes, RSRC_FLAGS};
}

// ------------------------------------------------------------------------------------------------ hand-issued vector memory
// Why asm.  The compiler's waitcnt pass treats an LDS-DMA load as "may alias every later LDS access" and drains vmcnt before the
// first ds_read / barrier, which would serialise a prologue behind the whole plane stream; and its own counting gives up at a
// loop's control-flow joins and drains the queue (vmcnt(0)) before every unit, which serialises the memory latency with the MFMAs.
// So the loads that must stay in flight are issued from inline asm (invisible to that pass) and waited for with an explicit
// s_waitcnt vmcnt(n): vector memory returns in order, the kernels count their requests.
// Request sites.  ONE request site per register slot: a second site in another branch gets registers of its own and a copy at
// the join -- made before the data lands.
// Register copies.  An asm OUTPUT may be copied by the compiler before the data lands; where that can happen (a destination that
// lives across a loop) the destination is an in-out operand of the request (aload128) and is tied again behind the wait; the
// ties (empty asm, "+v") make the registers depend on the preceding s_waitcnt (volatile asm statements keep their order).
// NT selects the cache policy between two literal statements: `nt` (streamed once: the planes) or plain.

// 16 bytes per lane straight into LDS at lds_base + 16 * lane.  m0 is not otherwise used in these kernels (no compiler-generated
// LDS-DMA / movrel).
template <bool NT>
__device__ __forceinline__ void dma16(u32x4 rsrc, uint32_t lds_base, uint32_t voff) {
    static_assert(NT, "only the streamed form is in use without a scalar offset");
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen nt lds" ::"s"(lds_base), "v"(voff), "s"(rsrc) : "memory");
}
template <bool NT>
__device__ __forceinline__ void dma16(u32x4 rsrc, uint32_t lds_base, uint32_t voff, uint32_t soff) {
    if constexpr (NT)
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen nt lds" ::"s"(lds_base), "v"(voff), "s"(rsrc), "s"(soff) : "memory");
    else
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(lds_base), "v"(voff), "s"(rsrc), "s"(soff) : "memory");
}
// 16 bytes per lane to VGPRs (an output: for destinations used once, behind the wait and a tie)
__device__ __forceinline__ u32x4 bload128(u32x4 rsrc, uint32_t voff, uint32_t soff) {
    u32x4 r;
    asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(r) : "v"(voff), "s"(rsrc), "s"(soff) : "memory");
    return r;
}
// ... into a register slot that lives across the loop (in-out)
template <bool NT>
__device__ __forceinline__ void aload128(u32x4 &dst, u32x4 rsrc, uint32_t voff, uint32_t soff) {
    if constexpr (NT) asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen nt" : "+v"(dst) : "v"(voff), "s"(rsrc), "s"(soff) : "memory");
    else asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "+v"(dst) : "v"(voff), "s"(rsrc), "s"(soff) : "memory");
}
// a zero-extended 16-bit value per lane
__device__ __forceinline__ uint32_t bload16s(u32x4 rsrc, uint32_t voff, uint32_t soff) {
    uint32_t r;
    asm volatile("buffer_load_ushort %0, %1, %2, %3 offen" : "=v"(r) : "v"(voff), "s"(rsrc), "s"(soff) : "memory");
    return r;
}
// ... into a register that stays live until a wait far behind the request (in-out, like aload128)
__device__ __forceinline__ void aload16s(uint32_t &dst, u32x4 rsrc, uint32_t voff, uint32_t soff) {
    asm volatile("buffer_load_ushort %0, %1, %2, %3 offen" : "+v"(dst) : "v"(voff), "s"(rsrc), "s"(soff) : "memory");
}
__device__ __forceinline__ void tie128(u32x4 &r) { asm volatile("" : "+v"(r)); }
__device__ __forceinline__ void tie4(uint32_t (&r)[4]) { asm volatile("" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3])); }
template <int N>
__device__ __forceinline__ void wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// wait until at most n * LPS vector-memory instructions of this wave are outstanding (n wave-uniform, 0..4; more waits for 4 LPS)
template <int LPS>
__device__ __forceinline__ void wait_vm_steps(uint32_t n) {
    switch (n) {
        case 0: wait_vm<0>(); break;
        case 1: wait_vm<LPS>(); break;
        case 2: wait_vm<2 * LPS>(); break;
        case 3: wait_vm<3 * LPS>(); break;
        default: wait_vm<4 * LPS>(); break;
    }
}
// ... at most n * LPU (n wave-uniform, 0..3; more waits for 3 LPU)
template <int LPU>
__device__ __forceinline__ void wait_vm_units(uint32_t n) {
    switch (n) {
        case 0: wait_vm<0>(); break;
        case 1: wait_vm<LPU>(); break;
        case 2: wait_vm<2 * LPU>(); break;
        default: wait_vm<3 * LPU>(); break;
    }
}

// LDS byte address of a pointer into the block's LDS
__device__ __forceinline__ uint32_t lds_addr(const void *p) {
    return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const unsigned char *)reinterpret_cast<const unsigned char *>(p);
}

}  // namespace gqw
