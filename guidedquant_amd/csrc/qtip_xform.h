// qtip_xform.h -- the element-wise arithmetic of the QTIP transform-in / transform-out, once (device only).
//
// BitshiftLinear.forward (inference/lib/codebook/bitshift.py:415-472) around the trellis matvec:
//   in  (bitshift.py:441):  x = hadamard(x.float() * SU) * n^-1/2 / 32 -> half, with what produces x in the decode step fused in front:
//                           RMSNorm (model.py:281-292) or silu(gate) * up (model.py:266)
//   out (bitshift.py:470):  out = (hadamard(y) * m^-1/2 * (SV * 32)).half()  (+ the residual add of the block, model.py:311-313)
// qtip.hip (the prologue of the fused linear), qtip_xf.hip (the one-block transform kernels) and decode.hip (the q / k / v fold of the
// attention kernel) build their forms of the two from the functions below: the tests compare those forms bit for bit, so a rounding
// point lives here and nowhere else.  DESIGN.md section 3.13 has the contracts as a table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gq_internal.h"
#include "fwht.h"
#include "wave_util.h"

namespace gqq {
typedef uint32_t u32;
using gqw::h16;
using gqw::wave_allsum;

// what produces the input of a transform-in (GQ_QPRO_* of include/gq_hip.h; QPRO_ROWS is internal: gq_qtip_linear_in_rows)
enum { QPRO_NONE = 0, QPRO_RMSNORM = 1, QPRO_SILUMUL = 2, QPRO_PRE = 3, QPRO_ROWS = 4 };

struct QtipOut {
    const float *y32, *SV32;  // SV32 = SV * 32 (fp32)
    const uint16_t *resid;
    uint16_t *out;
    u32 M;
    float mscale;  // (float)M^-1/2
    u32 parts;     // y32 is [parts][M] split-K partial sums, added in this order
};

// fp16 element e of a register run of packed pairs (no rounding)
template <int N>
__device__ __forceinline__ uint16_t h16_of(const u32 (&w)[N], int e) {
    return (uint16_t)(w[e >> 1] >> (16 * (e & 1)));
}

// y32 of a producing linear: its split-K parts added in ascending order, part 0 first (fp32 adds, nothing else)
__device__ __forceinline__ float sum_parts(const float *y32, u32 M, u32 parts, u32 i) {
    float t = y32[i];
    for (u32 p = 1; p < parts; p++) t += y32[(size_t)p * M + i];
    return t;
}
// the same for the 16-byte unit u (elements 4 u .. 4 u + 3; M a multiple of 4, y32 16-byte aligned)
__device__ __forceinline__ float4 sum_parts4(const float *y32, u32 M, u32 parts, u32 u) {
    float4 t = reinterpret_cast<const float4 *>(y32)[u];
    for (u32 p = 1; p < parts; p++) {
        const float4 t2 = reinterpret_cast<const float4 *>(y32 + (size_t)p * M)[u];
        t = make_float4(t.x + t2.x, t.y + t2.y, t.z + t2.z, t.w + t2.w);
    }
    return t;
}

// transform-out element (bitshift.py:470): v = the Hadamard sum.  Roundings: fp32 v * m^-1/2, fp32 * SV32, then fp16 -- the second
// product is pinned so that the conversion is not fused into it (gq_internal.h: gq_pin_f32)
__device__ __forceinline__ h16 xf_out(float v, float mscale, float sv32) { return (h16)gq_pin_f32((v * mscale) * sv32); }
// ... + the residual (model.py:311-313): one fp16 add, residual on the left (the callers branch on the residual pointer)
__device__ __forceinline__ h16 xf_resid(uint16_t resid, h16 y) { return __builtin_bit_cast(h16, resid) + y; }

// transform-in element in front of the Hadamard sum (bitshift.py:441 with the producer fused in): fp16 bits in, fp32 out.
//   QPRO_RMSNORM (model.py:281-292): half(float(x) * nscale) -- the product pinned -- then the fp16 product with the norm weight
//   QPRO_SILUMUL (model.py:266):     half(g / (1 + exp(-g))) in fp32 with the fast exponential, then the fp16 product with up
// and, for every PRO, float(.) * SU in fp32
template <int PRO>
__device__ __forceinline__ float xf_in(uint16_t xb, uint16_t x2b, uint16_t nwb, float nscale, float su) {
    h16 xh = __builtin_bit_cast(h16, xb);
    if constexpr (PRO == QPRO_RMSNORM) xh = (h16)gq_pin_f32((float)xh * nscale) * __builtin_bit_cast(h16, nwb);
    if constexpr (PRO == QPRO_SILUMUL) {
        const float g = (float)xh;
        xh = (h16)(g / (1.0f + __expf(-g))) * __builtin_bit_cast(h16, x2b);
    }
    return (float)xh * su;
}
// the same for one 16-byte unit of 8 activations held in registers (x2q / nwq are read only by the prologue that needs them)
template <int PRO>
__device__ __forceinline__ void xf_in_unit(const uint4 &xq, const uint4 &x2q, const uint4 &nwq, const float4 &s0, const float4 &s1, float nscale,
                                           float (&o)[8]) {
    const u32 xw[4] = {xq.x, xq.y, xq.z, xq.w};
    const u32 x2w[4] = {PRO == QPRO_SILUMUL ? x2q.x : 0u, PRO == QPRO_SILUMUL ? x2q.y : 0u, PRO == QPRO_SILUMUL ? x2q.z : 0u,
                        PRO == QPRO_SILUMUL ? x2q.w : 0u};
    const u32 nw[4] = {PRO == QPRO_RMSNORM ? nwq.x : 0u, PRO == QPRO_RMSNORM ? nwq.y : 0u, PRO == QPRO_RMSNORM ? nwq.z : 0u,
                       PRO == QPRO_RMSNORM ? nwq.w : 0u};
    const float su[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
#pragma unroll
    for (int e = 0; e < 8; e++) o[e] = xf_in<PRO>(h16_of(xw, e), h16_of(x2w, e), h16_of(nw, e), nscale, su[e]);
}

// transform-in element behind the Hadamard sum (bitshift.py:441): fp32 f * K^-1/2, a true fp32 division by 32, then fp16
__device__ __forceinline__ h16 xf_in_h16(float f, float kscale) { return (h16)((f * kscale) / 32.0f); }
__device__ __forceinline__ u32 xf_in_pack(float f0, float f1, float kscale) {
    return (u32)__builtin_bit_cast(uint16_t, xf_in_h16(f0, kscale)) | ((u32)__builtin_bit_cast(uint16_t, xf_in_h16(f1, kscale)) << 16);
}

// sum of squares of a unit of 8 fp16 values, element order, onto ss (the RMSNorm statistic's per-thread part)
__device__ __forceinline__ float ssq_unit(float ss, const uint4 &xq) {
    const u32 w4[4] = {xq.x, xq.y, xq.z, xq.w};
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const float f = (float)__builtin_bit_cast(h16, h16_of(w4, e));
        ss += f * f;
    }
    return ss;
}
// RMSNorm scale of the block's K values from the per-thread sums of squares (model.py:281-292), in EVERY thread: wave_allsum, the
// wave sums through redf[>= waves] and ONE barrier, the same tree over the wave sums (ascending lanes = ascending waves), then
// 1 / sqrtf(t / K + eps).  The order of the additions depends on the block shape only: two kernels with the same threads and the
// same per-thread units get the same bits.
__device__ __forceinline__ float block_rms_scale(float ss, float *redf, u32 K, float eps) {
    const u32 T = blockDim.x, tid = threadIdx.x;
    ss = wave_allsum(ss);
    if ((tid & 63u) == 0) redf[tid >> 6] = ss;
    __syncthreads();
    const float t = wave_allsum((tid & 63u) < (T >> 6) ? redf[tid & 63u] : 0.f);
    return 1.0f / sqrtf(t / (float)K + eps);
}

// Segment combine of H_M = H_(M / HD) (x) H_HD: the HD outputs of segment `seg` are the HD-point transform of
// z[b] = sum_c s(c) y[c HD + b], s(c) = (-1)^popcount(c & seg) (row `seg` of the M / HD-point Sylvester matrix).  Thread tid of T
// takes the 16-byte units tid, tid + T, .. (<= 4: M <= 16 T) of the sums -- Q = HD / 4 units per segment, T a multiple of Q, so all
// its units share the element group tid % Q -- and keeps one signed partial sum; the T / Q partial sums of an element are added in
// ascending order behind a barrier.  The additions of the full transform in another order: equal to it up to fp32 rounding.
__device__ __forceinline__ void seg_load(float4 (&y)[4], const float *y32, u32 M, u32 parts, u32 T) {
    const u32 M4 = M / 4u;
#pragma unroll
    for (u32 k = 0; k < 4; k++) {  // all in flight together; units past the vector hold zeros
        const u32 u = threadIdx.x + k * T;
        y[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (u < M4) {
            float4 t = reinterpret_cast<const float4 *>(y32)[u];
            for (u32 p = 1; p < parts; p++) {  // sum_parts4 with the part stride counted in units
                const float4 t2 = reinterpret_cast<const float4 *>(y32)[(size_t)p * M4 + u];
                t = make_float4(t.x + t2.x, t.y + t2.y, t.z + t2.z, t.w + t2.w);
            }
            y[k] = t;
        }
    }
}
template <u32 Q>
__device__ __forceinline__ float4 seg_signed_sum(const float4 (&y)[4], u32 seg, u32 T) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (u32 k = 0; k < 4; k++) {
        const u32 c = (threadIdx.x + k * T) / Q;
        const float sg = (__builtin_popcount(c & seg) & 1) ? -1.f : 1.f;
        acc = make_float4(acc.x + sg * y[k].x, acc.y + sg * y[k].y, acc.z + sg * y[k].z, acc.w + sg * y[k].w);
    }
    return acc;
}

// Transform-out of one linear by one block: y32 (split-K parts added in ascending order) -> hadamard * m^-1/2 -> * (SV * 32) ->
// fp16 (+ residual).  v: M floats of LDS.  Two arms with the same arithmetic: 16-byte units requested before the transform when the
// buffers are aligned and M <= 8 T, else element by element.  Shared by gq_qtip_linear_out, gq_qtip_linear_out_in and the finishing
// block of gq_qtip_linear: the forms agree bit for bit.
__device__ __forceinline__ void qtip_transform_out(const QtipOut &L, float *v) {
    const u32 T = blockDim.x, tid = threadIdx.x, M = L.M;
    constexpr u32 PRE = 2;  // M <= 8192 at 1024 threads
    const bool vec = !(((uintptr_t)L.y32 | (uintptr_t)L.SV32) & 15u) && !(((uintptr_t)L.resid | (uintptr_t)L.out) & 7u);
    const bool pre = vec && M <= 4u * PRE * T;
    float4 svr[PRE];
    uint2 rsr[PRE];
    if (pre) {  // (one block: nothing else hides the latency of the scales and the residual)
#pragma unroll
        for (u32 k = 0; k < PRE; k++) {
            const u32 u = tid + k * T;
            const bool ok = u < M / 4u;
            float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok) y = sum_parts4(L.y32, M, L.parts, u);
            if (ok) reinterpret_cast<float4 *>(v)[u] = y;
            svr[k] = ok ? reinterpret_cast<const float4 *>(L.SV32)[u] : make_float4(0.f, 0.f, 0.f, 0.f);
            rsr[k] = (ok && L.resid) ? reinterpret_cast<const uint2 *>(L.resid)[u] : make_uint2(0u, 0u);
        }
    } else {
        for (u32 i = tid; i < M; i += T) v[i] = sum_parts(L.y32, M, L.parts, i);
    }
    __syncthreads();
    gq_fwht::fwht_lds(v, M);
    const float sc = L.mscale;
    if (pre) {
#pragma unroll
        for (u32 k = 0; k < PRE; k++) {
            const u32 u = tid + k * T;
            if (u < M / 4u) {
                const float4 f = reinterpret_cast<const float4 *>(v)[u];
                const float fv[4] = {f.x, f.y, f.z, f.w}, sv[4] = {svr[k].x, svr[k].y, svr[k].z, svr[k].w};
                const u32 rw[2] = {rsr[k].x, rsr[k].y};
                uint16_t o[4];
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    h16 y = xf_out(fv[e], sc, sv[e]);
                    if (L.resid) y = xf_resid(h16_of(rw, e), y);
                    o[e] = __builtin_bit_cast(uint16_t, y);
                }
                reinterpret_cast<uint2 *>(L.out)[u] = make_uint2((u32)o[0] | ((u32)o[1] << 16), (u32)o[2] | ((u32)o[3] << 16));
            }
        }
        return;
    }
    for (u32 i = tid; i < M; i += T) {
        h16 y = xf_out(v[i], sc, L.SV32[i]);
        if (L.resid) y = xf_resid(L.resid[i], y);
        L.out[i] = __builtin_bit_cast(uint16_t, y);
    }
}
}  // namespace gqq
