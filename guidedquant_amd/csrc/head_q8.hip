// head_q8.hip -- the opt-in int8 lm_head of the fused decode step (weight-only, one fp32 scale per output row), gfx950:
//   out[n] = fp16( scale[n] * sum_k xn[k] * Wq[n][k] ),  fp32 accumulation (v_dot2_f32_f16)
// xn = x, or the RMSNorm of x staged by the text the fp16 head runs (dense_stage.h).  The data flow is dense_gemv_kernel's
// (decode.hip): x once in LDS, one wave = RW rows at a time, 16-byte non-temporal loads with the RW loads of a row group in flight,
// a wave reduction, lane 0 stores.  A 16-byte load holds 16 weights per lane, so a wave covers 1024 columns per step; with
// K % 1024 == 512 the upper half of the wave sits out the last step.
//
// int8 -> fp16 (1.75 VALU instructions per weight; the stream leaves room for about 2): one v_xor turns the four bytes of a dword into
// biased codes q + 128, two v_perm_b32 place each under the high byte 0x64 -- the fp16 number 1024 + (q + 128), exact -- and one
// v_pk_add_f16 of -1152 per pair gives q itself, exact again (|q| <= 128, every intermediate an integer below 2048).  The signed value
// exists BEFORE the product: nothing biased is accumulated, no correction term is subtracted from a sum.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gq_internal.h"
#include "wave_util.h"
#include "dense_stage.h"

namespace {

typedef uint32_t u32;
using gqw::h16;
using gqw::h16x2;
using gqw::h2u;
using gqw::u32x4;
using gqw::wave_reduce_bcast;

// the signed fp16 pair of bytes (2 * HI, 2 * HI + 1) of a dword of biased codes (b = q ^ 0x80)
template <int HI>
__device__ __forceinline__ h16x2 q8_pair(u32 biased) {
    // v_perm_b32: selector bytes 0..3 take the bytes of the second operand, 4..7 those of the first
    const u32 p = __builtin_amdgcn_perm(0x64646464u, biased, HI ? 0x04030402u : 0x04010400u);  // (0x64, b1, 0x64, b0): 1024 + b each
    const h16 off = (h16)-1152.0f;
    return __builtin_bit_cast(h16x2, p) + (h16x2){off, off};
}

template <int RW>
__global__ void __launch_bounds__(256) dense_gemv_i8_kernel(const uint16_t *x, const uint8_t *Wq, const float *scale, uint16_t *out, u32 N, u32 K,
                                                            const uint16_t *normw, float eps, u32 rows_per_block) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint16_t *xs = reinterpret_cast<uint16_t *>(smem);
    float *red = reinterpret_cast<float *>(xs + K);
    const u32 tid = threadIdx.x, w = tid >> 6, l = tid & 63u;
    gq_dense::stage_x(x, normw, eps, K, xs, red, tid, w, l);
    const u32 row_begin = blockIdx.x * rows_per_block;
    const u32 row_end = min(row_begin + rows_per_block, N);
    for (u32 r0 = row_begin + w * RW; r0 < row_end; r0 += 4 * RW) {
        float acc[RW], sc[RW];
#pragma unroll
        for (int r = 0; r < RW; r++) {
            acc[r] = 0.f;
            sc[r] = scale[min(r0 + (u32)r, N - 1u)];  // (requested with the first weights; rows past N read row N - 1 and are not stored)
        }
        for (u32 k0 = l * 16u; k0 < K; k0 += 1024u) {
            const uint4 xa = *reinterpret_cast<const uint4 *>(xs + k0), xb = *reinterpret_cast<const uint4 *>(xs + k0 + 8u);
            const u32 xw[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
            u32x4 wv[RW];
#pragma unroll
            for (int r = 0; r < RW; r++) {
                const u32 row = min(r0 + (u32)r, N - 1u);
                wv[r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(Wq + (size_t)row * K + k0));
            }
#pragma unroll
            for (int r = 0; r < RW; r++) {
#pragma unroll
                for (int d = 0; d < 4; d++) {
                    const u32 b = wv[r][d] ^ 0x80808080u;
                    acc[r] = __builtin_amdgcn_fdot2(q8_pair<0>(b), __builtin_bit_cast(h16x2, xw[2 * d]), acc[r], false);
                    acc[r] = __builtin_amdgcn_fdot2(q8_pair<1>(b), __builtin_bit_cast(h16x2, xw[2 * d + 1]), acc[r], false);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < RW; r++) {
            const float s = wave_reduce_bcast<false>(acc[r]);
            // (the fp32 product is rounded before the conversion, as the contract states it: not one rounding of the exact product)
            if (l == 0 && r0 + (u32)r < row_end) out[r0 + r] = h2u((h16)gq_pin_f32(sc[r] * s));
        }
    }
}

}  // namespace

extern "C" int gq_dense_gemv_i8(const void *x, const void *Wq, const float *scale, void *out, uint32_t N, uint32_t K, const void *norm_weight,
                                float eps, void *stream) {
    if (!x || !Wq || !scale || !out) return gq_fail(GQ_EINVAL, "null pointer argument.");
    if (K == 0 || K % 512u || N == 0) return gq_fail(GQ_EINVAL, "dense int8 GEMV needs N > 0 and K a positive multiple of 512.");
    if ((((uintptr_t)x | (uintptr_t)Wq | (uintptr_t)norm_weight) & 15u)) return gq_fail(GQ_EINVAL, "x, Wq and norm_weight must be 16-byte aligned.");
    if (((uintptr_t)scale & 3u) || ((uintptr_t)out & 1u)) return gq_fail(GQ_EINVAL, "scale must be 4-byte, out 2-byte aligned.");
    const size_t smem = (size_t)K * 2u + 64u;  // (the fp16 activations and the four partial sums, as in gq_dense_gemv_f16)
    if (smem > 160u * 1024u) return gq_fail(GQ_ENOTSUP, "K too large.");
    constexpr int RW = 4;
    const u32 ncu = (u32)gq_cu_count();
    // the fp16 entry's plan: ~3 blocks per CU, every block a multiple of 4 waves * RW rows
    const int bpc_env = gq_env_int("GQ_DENSE_I8_BPC", 3);
    const u32 bpc = bpc_env >= 1 ? (u32)bpc_env : 1u;
    u32 rpb = (N + ncu * bpc - 1u) / (ncu * bpc);
    rpb = ((rpb + 4u * RW - 1u) / (4u * RW)) * (4u * RW);
    {   // (GQ_DENSE_I8_RPB: rows per block directly, a multiple of 16)
        const int rpb_env = gq_env_int("GQ_DENSE_I8_RPB", 0);
        if (rpb_env >= 16 && rpb_env % 16 == 0) rpb = (u32)rpb_env;
    }
    const u32 grid = (N + rpb - 1u) / rpb;
    static GqPerDeviceOnce once;
    GQ_HIP_CHECK(once.max_dynamic_lds(reinterpret_cast<const void *>(dense_gemv_i8_kernel<RW>), 160 * 1024));
    hipLaunchKernelGGL(dense_gemv_i8_kernel<RW>, dim3(grid), dim3(256), smem, (hipStream_t)stream, (const uint16_t *)x, (const uint8_t *)Wq, scale,
                       (uint16_t *)out, N, K, (const uint16_t *)norm_weight, eps, rpb);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}
