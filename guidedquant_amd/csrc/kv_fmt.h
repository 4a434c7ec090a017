// kv_fmt.h -- the format of a cached K / V row, stated once: the four cache formats (Fmt), what a kernel needs to know of each
// (Traits<F>), what a launch passes beside the caches (Side<F>) and the arithmetic of the formats' write and read rules.  Nothing about
// attention.  Users: attn_roped_kernel (decode.hip), rope_cache_rows_kernel (prefill.hip), prefill_attn_kernel (prefill_attn.hip) over
// every format; attn_kv8.hip and ap_stream.hip::fuse_attn_head take the fp16 / fp8 arithmetic.  A new format is one Traits
// specialisation (and one Side) here, one row of model.KV_FORMATS on the host, and its C entries.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gq_internal.h"
#include "wave_util.h"

namespace gq_kv {
typedef uint32_t u32;

// kv_cache_dtype "fp16" | "fp8" | "fp8_row" | "mxfp4" of the host (model.KV_FORMATS)
enum class Fmt { F16, FP8, FP8_ROW, MX4 };

// ------------------------------------------------------------------------------------------------ fp16 and fp8 (e4m3) rows
__device__ __forceinline__ void unpack8(const uint4 &row, float (&f)[8]) {  // 16 bytes of a K / V / q row: 8 fp16 values
    const u32 w[4] = {row.x, row.y, row.z, row.w};
#pragma unroll
    for (int e = 0; e < 4; e++) {
        f[2 * e] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[e] & 0xFFFF));
        f[2 * e + 1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[e] >> 16));
    }
}
// 8 bytes of an fp8 K / V row: 8 OCP e4m3 codes, converted in hardware (v_cvt_pk_f32_fp8).  Every e4m3 value is an fp16 value, so the
// floats are those unpack8 gives for the fp16 row that holds the same numbers: the arithmetic behind the unpack does not know the format.
__device__ __forceinline__ void unpack8_fp8(const uint2 &row, float (&f)[8]) {
    const u32 w[2] = {row.x, row.y};
#pragma unroll
    for (int e = 0; e < 2; e++) {
        const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[e], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[e], true);
        f[4 * e] = lo[0], f[4 * e + 1] = lo[1], f[4 * e + 2] = hi[0], f[4 * e + 3] = hi[1];
    }
}
// 8 fp16 values (4 words) -> 8 OCP e4m3 codes by THE write rule of the fp8 cache, the only rounding the format adds:
//   code = fp8_rne(clamp(float(x16) * inv, -448, 448))
// inv = 1 / scale of the KV head, an fp32 the host computed (no division here).  The clamp is explicit (v_med3_f32): v_cvt_pk_fp8_f32
// turns a magnitude beyond 448 into NaN, not into 448; +-Inf clamps to +-448.  The host model:
// (x16.float() * inv).clamp(-448, 448).to(torch.float8_e4m3fn).  A NaN must be stored as a NaN code, and the clamp loses it (v_med3_f32
// with a NaN operand returns the smaller of the other two, -448): NAN_PASS puts the NaNs among the products v back behind the clamp.
// Users: the row write (prefill.hip) and the fp8 decode attention that writes its own row (attn_kv8.hip).
template <bool NAN_PASS>
__device__ __forceinline__ uint2 fp8_quant8(const float (&v)[8]) {
    float f[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        f[k] = __builtin_amdgcn_fmed3f(v[k], -448.f, 448.f);
        if constexpr (NAN_PASS) f[k] = v[k] != v[k] ? v[k] : f[k];
    }
    u32 o[2];
#pragma unroll
    for (int e = 0; e < 2; e++) {
        int r = 0;
        r = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * e], f[4 * e + 1], r, false);
        r = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * e + 2], f[4 * e + 3], r, true);
        o[e] = (u32)r;
    }
    return make_uint2(o[0], o[1]);
}
// ------------------------------------------------------------------------------------------------ the per-row scaled fp8 cache
// kv_cache_dtype="fp8_row": e4m3 codes as above, and ONE exponent byte per (KV head, cached row) beside them, uint8 [n_kv_head][max_seq]
// in e8m0: value = fp16(code) * 2^(byte - 127).  No per-head scale, nothing to calibrate: the write puts the row's largest finite
// magnitude at the top of the e4m3 range.  THE exponent rule, on a = the fp16 bits of that magnitude (0 for a row without a finite
// non-zero element; max over magnitudes = max over their bits):
//   t = (a + 0xFF) >> 10      the fp16 exponent field, one more where the mantissa field exceeds 0x300: 448 = 1.75 * 2^8, so that
//                             t - 23 = ceil(log2(amax / 448)) for every normal amax
//   byte = clamp(t, 8, 30) + 104      e = byte - 127 in [-15, 7]: code * 2^e stays an fp16 value (2^-9 * 2^-15 = 2^-24; 448 * 2^7 = 57344)
// Integer arithmetic alone, no log2, no divide; the host model is model.fp8_row_quantize.  Both factors are built from the byte:
__device__ __forceinline__ u32 row_exp_byte(u32 amax_bits) { return min(max((amax_bits + 0xFFu) >> 10, 8u), 30u) + 104u; }
__device__ __forceinline__ float row_exp_scale(u32 byte) { return __builtin_bit_cast(float, byte << 23); }        // 2^e: the read rule
__device__ __forceinline__ float row_exp_inv(u32 byte) { return __builtin_bit_cast(float, (254u - byte) << 23); }  // 2^-e: the write rule
// the largest of a value over each aligned group of 4 or 8 lanes (the thread units that hold one (row, head) of the row write), in every
// lane of the group: the DPP butterflies of row_sum, no LDS round trip.  eight: wave-uniform.  The lanes of a group are active together.
__device__ __forceinline__ u32 group_umax(u32 v, bool eight) {
    v = max(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false));  // quad_perm [1,0,3,2]
    v = max(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false));  // quad_perm [2,3,0,1]
    if (eight) v = max(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false));  // row_half_mirror
    return v;
}
// ------------------------------------------------------------------------------------------------ the MXFP4 cache
// kv_cache_dtype="mxfp4" (OCP microscaling): e2m1 codes, two per byte (element 2j in the low nibble of byte j), uint8
// [n_kv_head][max_seq][head_dim / 2], and ONE e8m0 exponent byte per block of 32 consecutive elements of a head's row, uint8
// [n_kv_head][max_seq][head_dim / 32]: value = e2m1(code) * 2^(byte - 127), magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6.  The scale of the
// per-row fp8 form moved from the row to the block.  THE exponent rule, on a = the largest fp16 magnitude bits of the block's 32 values:
//   t = (a + 0x1FF) >> 10     the fp16 exponent field, one more where the mantissa field exceeds 0x200: 6 = 1.5 * 2^2, so that
//                             t - 17 = ceil(log2(amax / 6)) for every normal amax
//   field = clamp(t, 2, 30) + 110     e = field - 127 in [-15, 13]: code * 2^e stays an fp16 value (0.5 * 2^-15 = 2^-16; 6 * 2^13 = 49152)
//   byte = 0xFF where a >= 0x7C00 (the block holds an Inf or a NaN: every element of it reads back NaN), else field
// The codes are taken at 2^-(field - 127) in both cases (a non-finite block: e = 13, its non-finite elements saturate to +-6).
__device__ __forceinline__ u32 mx4_exp_field(u32 amax_bits) { return min(max((amax_bits + 0x1FFu) >> 10, 2u), 30u) + 110u; }
__device__ __forceinline__ u32 mx4_exp_byte(u32 amax_bits) { return amax_bits >= 0x7C00u ? 0xFFu : mx4_exp_field(amax_bits); }
// one e2m1 code (sign in bit 3) of the fp16 value h at the scale inv = 2^-e, round to nearest, ties to the even mantissa: y = |h| * inv
// is exact in fp32.  y < 1 (the codes 0, 0.5, 1: a grid of 0.5): the fp32 addition y + 2^22 rounds to that grid, ties to even, and leaves
// the code in its two low bits.  y >= 1: one mantissa bit is kept -- the fp32 bits rounded to bit 22, ties to even, make (exponent, bit)
// = code + 252; anything from 7 on (above 6, Inf, NaN) saturates to the code of 6.
__device__ __forceinline__ u32 mx4_code(uint16_t h, float inv) {
    const float y = gqw::h2f((uint16_t)(h & 0x7FFFu)) * inv;
    const u32 b = __builtin_bit_cast(u32, y);
    const u32 sub = __builtin_bit_cast(u32, y + 4194304.0f) & 3u;
    const u32 nrm = min(((b + 0x1FFFFFu + ((b >> 22) & 1u)) >> 22) - 252u, 7u);
    return (y < 1.0f ? sub : nrm) | (((u32)h >> 12) & 8u);
}
// 8 fp16 values (4 words) -> 8 codes in one word, element k in nibble k
__device__ __forceinline__ u32 mx4_quant8(const u32 (&w)[4], float inv) {
    u32 o = 0u;
#pragma unroll
    for (int k = 0; k < 8; k++) o |= mx4_code((uint16_t)(w[k >> 1] >> (16 * (k & 1))), inv) << (4 * k);
    return o;
}
// the read rule: 2^e of a block as fp32, NaN for the byte 0xFF; 4 bytes of codes -> 8 values by v_cvt_scalef32_pk_f32_fp4 at the scale
// 1.0 (the e2m1 magnitudes, exact), times 2^e: every product is an fp16 value, so from here on the floats are those unpack8 gives for an
// fp16 row that holds code * 2^e -- and a NaN scale makes all 8 NaN, zero codes included
__device__ __forceinline__ float mx4_scale(u32 byte) { return byte == 0xFFu ? __builtin_nanf("") : __builtin_bit_cast(float, byte << 23); }
__device__ __forceinline__ void unpack8_mx4(u32 row, float sc, float (&f)[8]) {
    const auto p0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(row, 1.0f, 0), p1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(row, 1.0f, 1);
    const auto p2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(row, 1.0f, 2), p3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(row, 1.0f, 3);
    f[0] = p0[0] * sc, f[1] = p0[1] * sc, f[2] = p1[0] * sc, f[3] = p1[1] * sc;
    f[4] = p2[0] * sc, f[5] = p2[1] * sc, f[6] = p3[0] * sc, f[7] = p3[1] * sc;
}

// ------------------------------------------------------------------------------------------------ what a kernel asks of a format
// Traits<F>: elem, the cache element type; load, the load of a lane's 8 dims of a row; ROW_DIV / LANE, the cache elements of a row
// (head_dim / ROW_DIV) and of a lane's 8 dims; exp_bytes(head_dim), the exponent bytes of a (KV head, row), 0 where there are none;
// head_scale (a scale per KV head: fp8 alone), row_exp (exponent bytes beside the codes), block_exp (one per block of 32 elements, not
// one per row); zero(), and unpack(load, exponent byte, f): the read rule up to the per-head scale, which stays outside the products
// (the byte is ignored where the format has none).
template <Fmt F>
struct Traits {  // F16
    typedef uint16_t elem;
    typedef uint4 load;
    static constexpr u32 ROW_DIV = 1, LANE = 8;
    static constexpr bool head_scale = false, row_exp = false, block_exp = false;
    static constexpr u32 exp_bytes(u32) { return 0u; }
    static __device__ __forceinline__ load zero() { return make_uint4(0, 0, 0, 0); }
    static __device__ __forceinline__ void unpack(const load &r, u32, float (&f)[8]) { unpack8(r, f); }
};
template <>
struct Traits<Fmt::FP8> {
    typedef uint8_t elem;
    typedef uint2 load;
    static constexpr u32 ROW_DIV = 1, LANE = 8;
    static constexpr bool head_scale = true, row_exp = false, block_exp = false;
    static constexpr u32 exp_bytes(u32) { return 0u; }
    static __device__ __forceinline__ load zero() { return make_uint2(0, 0); }
    static __device__ __forceinline__ void unpack(const load &r, u32, float (&f)[8]) { unpack8_fp8(r, f); }
};
template <>
struct Traits<Fmt::FP8_ROW> : Traits<Fmt::FP8> {  // the fp8 codes; fp16(code) * 2^e, exact
    static constexpr bool head_scale = false, row_exp = true;
    static constexpr u32 exp_bytes(u32) { return 1u; }
    static __device__ __forceinline__ void unpack(const load &r, u32 byte, float (&f)[8]) {
        unpack8_fp8(r, f);
        const float sc = row_exp_scale(byte);
#pragma unroll
        for (int e = 0; e < 8; e++) f[e] *= sc;
    }
};
template <>
struct Traits<Fmt::MX4> {
    typedef uint8_t elem;
    typedef u32 load;
    static constexpr u32 ROW_DIV = 2, LANE = 4;
    static constexpr bool head_scale = false, row_exp = true, block_exp = true;
    static constexpr u32 exp_bytes(u32 hd) { return hd / 32u; }
    static __device__ __forceinline__ load zero() { return 0u; }
    static __device__ __forceinline__ void unpack(const load &r, u32 byte, float (&f)[8]) { unpack8_mx4(r, mx4_scale(byte), f); }
};

// what a launch that READS such caches takes beside them: nothing, the per-KV-head scales of an fp8 cache (fp32 [n_kv_head], device
// memory: value = code * scale), or the exponent bytes of the batch slot (uint8 [n_kv_head][max_seq], [n_kv_head][max_seq][head_dim / 32]
// for MXFP4).  Compile-time like gq_attn::AttnWindow: the fp16 instances take an empty argument.
template <Fmt F>
struct Side {};
template <>
struct Side<Fmt::FP8> {
    const float *k_scale, *v_scale;
};
template <>
struct Side<Fmt::FP8_ROW> {
    const uint8_t *k_exp, *v_exp;
};
template <>
struct Side<Fmt::MX4> {
    const uint8_t *k_exp, *v_exp;
};
// the same for the launch that WRITES the rows (rope_cache_rows_kernel): the exponent bytes are stored, the reciprocal scales of an fp8
// cache are plain arguments of every instance (null where the format has none)
template <bool EXP>
struct WriteSide {};
template <>
struct WriteSide<true> {
    uint8_t *k_exp, *v_exp;
};

}  // namespace gq_kv
