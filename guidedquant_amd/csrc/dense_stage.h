// dense_stage.h -- the activation staging of the dense lm_head GEMVs (decode.hip::dense_gemv_kernel, head_q8.hip::dense_gemv_i8_kernel):
// x, or the RMSNorm of x, once into the block's LDS.  One text for both kernels, so that the int8 head normalises with exactly the
// rounding points of the fp16 head: the statistic in fp32, x * scale rounded to fp16, the fp16 product with the weight.  Device only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gq_internal.h"
#include "wave_util.h"

namespace gq_dense {

// blocks of 256 threads (w = wave, l = lane of tid); xs: K fp16 in LDS, red: four floats behind them; K a multiple of 8.  Ends with the
// barrier behind which every thread may read xs.
__device__ __forceinline__ void stage_x(const uint16_t *x, const uint16_t *normw, float eps, uint32_t K, uint16_t *xs, float *red, uint32_t tid,
                                        uint32_t w, uint32_t l) {
    typedef uint32_t u32;
    using gqw::h16;
    using gqw::h2f;
    using gqw::h2u;
    using gqw::u2h;
    using gqw::wave_reduce_bcast;
    float nscale = 1.f;
    // (round 5: x and the norm weights of a thread's first two units are requested together and kept -- the weights are a layer
    // tensor that comes from HBM; requested only behind the sum of squares they cost the launch a second memory round trip)
    constexpr u32 NPRE = 2;
    uint4 xpre[NPRE], npre[NPRE];
    auto sq8 = [&](const uint4 &v, float &ss) {
        const u32 ww[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float a = h2f(ww[i] & 0xFFFF), b = h2f(ww[i] >> 16);
            ss += a * a;
            ss += b * b;
        }
    };
    auto norm8 = [&](uint4 v, const uint4 &nv) {
        u32 ww[4] = {v.x, v.y, v.z, v.w};
        const u32 nw[4] = {nv.x, nv.y, nv.z, nv.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const h16 a = (h16)gq_pin_f32(h2f(ww[i] & 0xFFFF) * nscale) * u2h((uint16_t)(nw[i] & 0xFFFF));
            const h16 b = (h16)gq_pin_f32(h2f(ww[i] >> 16) * nscale) * u2h((uint16_t)(nw[i] >> 16));
            ww[i] = (u32)h2u(a) | ((u32)h2u(b) << 16);
        }
        return make_uint4(ww[0], ww[1], ww[2], ww[3]);
    };
    if (normw) {
        float ss = 0.f;
#pragma unroll
        for (u32 k = 0; k < NPRE; k++) {
            const u32 g = tid + 256u * k;
            xpre[k] = g < K / 8u ? reinterpret_cast<const uint4 *>(x)[g] : make_uint4(0u, 0u, 0u, 0u);
            npre[k] = g < K / 8u ? reinterpret_cast<const uint4 *>(normw)[g] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (u32 k = 0; k < NPRE; k++) sq8(xpre[k], ss);  // (units beyond K are zero)
        for (u32 g = tid + 256u * NPRE; g < K / 8u; g += 256) sq8(reinterpret_cast<const uint4 *>(x)[g], ss);
        ss = wave_reduce_bcast<false>(ss);
        if (l == 0) red[w] = ss;
        __syncthreads();
        nscale = 1.0f / sqrtf((red[0] + red[1] + red[2] + red[3]) / (float)K + eps);
#pragma unroll
        for (u32 k = 0; k < NPRE; k++) {
            const u32 g = tid + 256u * k;
            if (g < K / 8u) reinterpret_cast<uint4 *>(xs)[g] = norm8(xpre[k], npre[k]);
        }
        for (u32 g = tid + 256u * NPRE; g < K / 8u; g += 256)
            reinterpret_cast<uint4 *>(xs)[g] = norm8(reinterpret_cast<const uint4 *>(x)[g], reinterpret_cast<const uint4 *>(normw)[g]);
    } else {
        for (u32 g = tid; g < K / 8u; g += 256) reinterpret_cast<uint4 *>(xs)[g] = reinterpret_cast<const uint4 *>(x)[g];
    }
    __syncthreads();
}

}  // namespace gq_dense
