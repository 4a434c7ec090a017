// qtip_xf.hip -- the transform side of the fused QTIP linear for gfx950: the one-block kernels around the trellis matvec of
// qtip.hip (transform-out, transform-out + the consumers' transform-in, the segmented transform-out, the transforms of widths with a
// Hadamard factor, the middle of a factor-width MLP) and gq_hadamard, y = scale * x @ H_n for n a power of two
// (fast_hadamard_transform as used by inference/lib/utils/matmul_had.py:96-106).  The element-wise arithmetic is qtip_xform.h's.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gq_internal.h"
#include "fwht.h"
#include "qtip_xform.h"
#include "wave_util.h"

namespace {
typedef uint32_t u32;
using gq_fwht::fwht_lds;
using gqq::QtipOut;
using gqw::h16;
using gqw::make_rsrc;
using gqw::rsrc_t;
using gqw::u32x4;

struct QtipOutArgs {
    QtipOut lin[3];
};
__global__ void __launch_bounds__(1024) qtip_linear_out_kernel(QtipOutArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    gqq::qtip_transform_out(a.lin[blockIdx.x], reinterpret_cast<float *>(smem));
}

// Round 5: transform-out of ONE linear (o or down, residual added) followed by the transform-IN of the linears that consume its
// output (gate / up, or the next layer's q / k / v) -- block j of the launch repeats the transform-out (only block 0 stores the hidden
// state) and then runs RMSNorm -> * SU_j -> Hadamard -> * K^-1/2 / 32 -> fp16 for consumer j, leaving that linear's PRE-TRANSFORMED
// input in memory.  The matvec launch that follows takes it as is (GQ_QPRO_PRETRANSFORMED with one vector per linear): its 256
// blocks no longer repeat RMSNorm . SU . H each (~5 us of a 15 us launch, profiles/r04_qtip_decode_kernel_trace.txt).  Same
// element-wise operations (qtip_xform.h), the same butterfly network and the same summation order of the mean of squares (1024
// threads, the per-thread unit order of qtip_linear_in_kernel's prologue): the pre-transformed vectors are what that prologue builds.
struct QtipOutInArgs {
    QtipOut prev;
    const uint16_t *normw;
    float eps, kscale;
    const float *SU[3];
    uint16_t *xt[3];
};
__global__ void __launch_bounds__(1024) qtip_out_in_kernel(QtipOutInArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ float redf[17];
    const u32 K = a.prev.M, T = blockDim.x, tid = threadIdx.x, j = blockIdx.x;
    float *v = reinterpret_cast<float *>(smem);                       // [K] fp32 transform buffer
    uint16_t *hs = reinterpret_cast<uint16_t *>(smem + (size_t)K * 4u);  // [K] fp16: the hidden state this launch produces
    // the consumer's vectors are requested with the sums (one block: nothing else hides their latency)
    constexpr u32 NU = 2;  // 8-element units per thread (K <= 16384)
    float4 su0[NU], su1[NU];
    uint4 nwq[NU];
#pragma unroll
    for (u32 k = 0; k < NU; k++) {
        const u32 u = tid + k * T;
        const bool ok = u < K / 8u;
        su0[k] = ok ? reinterpret_cast<const float4 *>(a.SU[j])[2u * u] : make_float4(0.f, 0.f, 0.f, 0.f);
        su1[k] = ok ? reinterpret_cast<const float4 *>(a.SU[j])[2u * u + 1u] : make_float4(0.f, 0.f, 0.f, 0.f);
        nwq[k] = ok ? reinterpret_cast<const uint4 *>(a.normw)[u] : make_uint4(0u, 0u, 0u, 0u);
    }
    {   // transform-out into LDS; the global store only by block 0
        QtipOut P = a.prev;
        P.out = hs;
        gqq::qtip_transform_out(P, v);
        __syncthreads();
        if (j == 0u && a.prev.out)
            for (u32 u = tid; u < K / 4u; u += T) reinterpret_cast<uint2 *>(a.prev.out)[u] = reinterpret_cast<const uint2 *>(hs)[u];
    }
    // transform-in of consumer j: the prologue of qtip_linear_in_kernel<QPRO_RMSNORM>, unit by unit
    float ss = 0.f;
    for (u32 u = tid; u < K / 8u; u += T) ss = gqq::ssq_unit(ss, reinterpret_cast<const uint4 *>(hs)[u]);
    const float nscale = gqq::block_rms_scale(ss, redf, K, a.eps);
#pragma unroll
    for (u32 k = 0; k < NU; k++) {
        const u32 u = tid + k * T;
        if (u < K / 8u) {
            float o[8];
            gqq::xf_in_unit<gqq::QPRO_RMSNORM>(reinterpret_cast<const uint4 *>(hs)[u], nwq[k], nwq[k], su0[k], su1[k], nscale, o);
            reinterpret_cast<float4 *>(v)[2u * u] = make_float4(o[0], o[1], o[2], o[3]);
            reinterpret_cast<float4 *>(v)[2u * u + 1u] = make_float4(o[4], o[5], o[6], o[7]);
        }
    }
    __syncthreads();
    fwht_lds(v, K);
#pragma unroll
    for (u32 k = 0; k < NU; k++) {
        const u32 u = tid + k * T;
        if (u < K / 8u) {
            const float4 f0 = reinterpret_cast<const float4 *>(v)[2u * u], f1 = reinterpret_cast<const float4 *>(v)[2u * u + 1u];
            reinterpret_cast<uint4 *>(a.xt[j])[u] = make_uint4(gqq::xf_in_pack(f0.x, f0.y, a.kscale), gqq::xf_in_pack(f0.z, f0.w, a.kscale),
                                                               gqq::xf_in_pack(f1.x, f1.y, a.kscale), gqq::xf_in_pack(f1.z, f1.w, a.kscale));
        }
    }
}

// The same transform-out spread over M / 128 blocks per linear (gq_qtip_linear_out_seg).  H_M = H_(M / 128) (x) H_128: block `seg`
// combines the M / 128 segments of the sums with the signs of row `seg` of the Sylvester matrix (qtip_xform.h: seg_load /
// seg_signed_sum) and runs ONE 128-point transform: no block repeats work another one does (the segment combination is what the last
// log2(M / 128) stages of the full transform do for this segment), and the launch ends after one load round trip and seven butterfly
// stages instead of twelve stages of a single block.  Equal to qtip_transform_out up to fp32 rounding, not bit for bit (decode.hip's
// attention prologue does the same for q / k / v).
constexpr u32 QSEG = 128u, QSEG_T = 512u;
__global__ void __launch_bounds__(QSEG_T) qtip_linear_out_seg_kernel(QtipOutArgs a) {
    __shared__ __attribute__((aligned(16))) float ps[QSEG_T / (QSEG / 4u) * QSEG];  // [thread group][128] partial sums
    __shared__ __attribute__((aligned(16))) float tv[QSEG];
    const QtipOut L = a.lin[blockIdx.y];
    const u32 tid = threadIdx.x, seg = blockIdx.x;
    if (seg * QSEG >= L.M) return;
    constexpr u32 Q = QSEG / 4u, G = QSEG_T / Q;
    // scale and residual of this thread's output element: requested before the sums (nothing else hides their latency)
    float sv = 0.f;
    uint16_t rs = 0;
    if (tid < QSEG) {
        sv = L.SV32[seg * QSEG + tid];
        if (L.resid) rs = L.resid[seg * QSEG + tid];
    }
    float4 y[4];  // M <= 8192: at most 4 units per thread
    gqq::seg_load(y, L.y32, L.M, L.parts, QSEG_T);
    reinterpret_cast<float4 *>(ps + (size_t)(tid / Q) * QSEG)[tid % Q] = gqq::seg_signed_sum<Q>(y, seg, QSEG_T);
    __syncthreads();
    if (tid < QSEG) {
        float z = 0.f;
#pragma unroll
        for (u32 gi = 0; gi < G; gi++) z += ps[(size_t)gi * QSEG + tid];
        tv[tid] = z;
    }
    __syncthreads();
    fwht_lds(tv, QSEG);
    if (tid < QSEG) {
        h16 y = gqq::xf_out(tv[tid], L.mscale, sv);
        if (L.resid) y = gqq::xf_resid(rs, y);
        L.out[seg * QSEG + tid] = __builtin_bit_cast(uint16_t, y);
    }
}

// ------------------------------------------------------------------------------------------------ transform with a Hadamard factor
// Widths n = Kf * P with a non-power-of-two Hadamard factor Kf (matmul_had.py:13-67; Llama-2's 11008 = 172 * 64): the
// transform is the P-point Sylvester transform of every row of the [Kf][P] view followed by hadK @ (or hadK^T @) over
// the rows (matmul_hadU / matmul_hadUt, matmul_had.py:69-94).  The Kf x Kf product is too much work to repeat in every
// band block of the matvec, so these widths run transform -> gq_qtip_matvec -> transform: this kernel is either side.
// Block b owns RB rows of the result; every block loads the vector and does the (cheap) row transforms itself.
//   IN : v = pro(x) * SU            -> rows, hadK^T -> out16 = half(val * n^-1/2 / 32)          (input of the matvec)
//   OUT: v = y32                    -> rows, hadK   -> out16 = half(val * n^-1/2 * SV32) (+ resid)
struct QtipXfLin {
    const float *y32, *vec, *hadK;  // vec = SU (IN) or SV * 32 (OUT); hadK fp32 [Kf][Kf]
    const uint16_t *resid;
    uint16_t *out;
};
struct QtipXfArgs {
    const uint16_t *x, *x2, *normw;
    QtipXfLin lin[3];   // blockIdx.y (linears that share the source / the launch)
    float eps, nscale;  // nscale = (float)n^-1/2
    u32 n, Kf, P, RB, in, pro, transpose;
};
__global__ void __launch_bounds__(1024) qtip_transform_kernel(QtipXfArgs a) {
    __shared__ float redf[17];
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const u32 n = a.n, T = blockDim.x, tid = threadIdx.x;
    const u32 P = a.P, Kf = a.Kf, RB = a.RB, r0 = blockIdx.x * RB;
    float *v = reinterpret_cast<float *>(smem);  // [n]
    float *hs = v + n;                           // [Kf][4]: element k of the (up to 4) factor rows this block multiplies with
    float *ps = hs + 4u * Kf;                    // [KQ][RB][P] partial sums of the factor product
    const QtipXfLin L = a.lin[blockIdx.y];
    // this block's rows of hadK (columns for the transposed product), requested first; k-major so that one 16-byte LDS read
    // serves the 4 rows
    for (u32 e = tid; e < 4u * Kf; e += T) {
        const u32 k = e >> 2, rr = e & 3u, kr = r0 + rr;
        hs[e] = (rr < RB && kr < Kf) ? (a.transpose ? L.hadK[(size_t)k * Kf + kr] : L.hadK[(size_t)kr * Kf + k]) : 0.f;
    }
    if (a.in) {
        float rs = 0.f;
        if (a.pro == gqq::QPRO_RMSNORM) {
            float ss = 0.f;
            for (u32 i = tid; i < n; i += T) {
                const float f = (float)__builtin_bit_cast(h16, a.x[i]);
                ss += f * f;
            }
            rs = gqq::block_rms_scale(ss, redf, n, a.eps);
        }
        for (u32 u = tid; u < n / 8u; u += T) {  // 8 activations per 16-byte load
            const uint4 xq = reinterpret_cast<const uint4 *>(a.x)[u];
            uint4 x2q = make_uint4(0u, 0u, 0u, 0u), nwq = x2q;
            if (a.pro == gqq::QPRO_SILUMUL) x2q = reinterpret_cast<const uint4 *>(a.x2)[u];
            if (a.pro == gqq::QPRO_RMSNORM) nwq = reinterpret_cast<const uint4 *>(a.normw)[u];
            const float4 s0 = reinterpret_cast<const float4 *>(L.vec)[2u * u], s1 = reinterpret_cast<const float4 *>(L.vec)[2u * u + 1u];
            float o[8];
            if (a.pro == gqq::QPRO_RMSNORM) gqq::xf_in_unit<gqq::QPRO_RMSNORM>(xq, x2q, nwq, s0, s1, rs, o);
            else if (a.pro == gqq::QPRO_SILUMUL) gqq::xf_in_unit<gqq::QPRO_SILUMUL>(xq, x2q, nwq, s0, s1, rs, o);
            else gqq::xf_in_unit<gqq::QPRO_NONE>(xq, x2q, nwq, s0, s1, rs, o);
            reinterpret_cast<float4 *>(v)[2u * u] = make_float4(o[0], o[1], o[2], o[3]);
            reinterpret_cast<float4 *>(v)[2u * u + 1u] = make_float4(o[4], o[5], o[6], o[7]);
        }
    } else {
        for (u32 i = tid; i < n / 4u; i += T) reinterpret_cast<float4 *>(v)[i] = reinterpret_cast<const float4 *>(L.y32)[i];
    }
    __syncthreads();
    fwht_lds(v, n, P);  // every row of the [Kf][P] view
    // (hadamard() scales by n^-1/2 before the factor product, matmul_had.py:88-90; here the factor entries are +-1, the
    // scale is applied to the sum -- one rounding less, one pass over the vector less)
    // factor product: thread (p, kq) adds its share of the k range into the (up to 4) rows of column p -- one LDS read of
    // the activation and one 16-byte read of the 4 factor entries per 4 multiply-adds --; the KQ partial sums are added in
    // a fixed order
    const u32 KQ = T >= P ? T / P : 1u, kper = (Kf + KQ - 1u) / KQ, NO = RB * P;
    for (u32 pb = 0; pb < P; pb += T) {
        const u32 p = pb + (T >= P ? tid % P : tid), kq = T >= P ? tid / P : 0u;
        if (p < P && kq < KQ) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            const u32 k1 = min((kq + 1u) * kper, Kf);
            for (u32 k = kq * kper; k < k1; k++) {
                const float4 h4 = *reinterpret_cast<const float4 *>(hs + 4u * k);
                const float xv = v[k * P + p];
                acc[0] += h4.x * xv;
                acc[1] += h4.y * xv;
                acc[2] += h4.z * xv;
                acc[3] += h4.w * xv;
            }
            for (u32 rr = 0; rr < RB; rr++) ps[(kq * RB + rr) * P + p] = acc[rr];
        }
    }
    __syncthreads();
    for (u32 o = tid; o < NO; o += T) {
        const u32 rr = o / P, kr = r0 + rr, p = o % P;
        if (kr >= Kf) continue;
        float acc = 0.f;
        for (u32 q = 0; q < KQ; q++) acc += ps[(q * RB + rr) * P + p];
        const u32 i = kr * P + p;
        h16 y;
        if (a.in) y = gqq::xf_in_h16(acc, a.nscale);
        else {
            y = gqq::xf_out(acc, a.nscale, L.vec[i]);
            if (L.resid) y = gqq::xf_resid(L.resid[i], y);
        }
        L.out[i] = __builtin_bit_cast(uint16_t, y);
    }
}

// ------------------------------------------------------------------------------------------------ middle of a gated MLP with a factor width
// gate / up leave their sums y32 [n]; down wants half(H(silu(g) * u * SU) * n^-1/2 / 32) with g, u = half(H(y32) * n^-1/2 * SV32),
// n = Kf * P (Llama-2: 11008 = 172 * 64).  As two gq_qtip_transform launches (out, then in) that is 2 x 6.9 us of a 78 us layer.
// H = hadK (x) H_P acts on the [Kf][P] view as  hadK @ X @ H_P: the two sides commute.  So
//     out:  rows first, then the factor product      (the order of gq_qtip_transform: g and u come out bit-identical to it)
//     in :  the factor product first, then the rows  (the other order: equal up to fp32 rounding)
// and everything between the two row passes -- out product, scales, fp16 roundings, silu * up, SU, in product -- is local to a
// COLUMN of the view.  Block j owns column j: it computes that column of the row transforms itself (a 64-term sum in butterfly
// order per row), both factor products and the element-wise middle, and stores column j of the fp32 vector whose row transforms the
// matvec launch of down runs in its prologue (QPRO_ROWS: one in-register pass per block).  One launch of P blocks instead of two
// launches of Kf / 4 blocks that each stage the whole vector.
// Every block needs both Kf x Kf tables: they come as fp16 (+-1 is exact; 2 x 59 KB per block instead of 2 x 118 KB -- the first
// version with fp32 tables and one row per thread spent 16 us, most of it in 96 four-byte loads per thread) in [k][r] order, wave w
// owns the k group w (the 16 groups of qtip_transform_kernel) and lane L the rows 4 L .. 4 L + 3: 8-byte loads, coalesced, requested
// before anything else -- they do not depend on the previous launch and arrive while its sums are still on their way --, kept in
// registers and multiplied by v_fma_mix_f32 (fp16 x fp32 + fp32: with +-1 entries the product is exact, so the fused form
// rounds like the multiply-add of qtip_transform_kernel).
struct QtipMidArgs {
    const float *y32g, *y32u, *sv32g, *sv32u, *su_down;
    const uint16_t *hadT_out, *had_in;  // fp16 [Kf][Kf]
    float *z32;
    uint16_t *gout, *uout;  // optional fp16 copies of gate / up (null: not stored)
    u32 parts, n, Kf, kper;
    float nscale;
    unsigned long long *dbg;  // phase stamps of block 32 (tools/qtip_mid_timing.py)
};
constexpr u32 MID_R = 256u, MID_T = 1024u, MID_KP = 12u;  // Kf <= 192 (3 rounds of 64 rows in stage 1), kper = ceil(Kf / 16) <= 12
__global__ void __launch_bounds__(MID_T) qtip_mlp_mid_kernel(QtipMidArgs a) {
    // dynamic LDS: both tables (fp16 [Kf][Kf], flat copies), then xr [256][gate, up] (column j of the row transforms), ps [16][gate,
    // up][256] (partial sums of the out product; the in product's [16][256] re-use it), vin [256]
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const u32 tbytes = a.Kf * a.Kf * 2u;  // (a multiple of 16: Kf % 4 == 0)
    const unsigned char *tabO = smem, *tabI = smem + tbytes;
    float *xr = reinterpret_cast<float *>(smem + 2u * tbytes);
    float *ps = xr + MID_R * 2u, *ps2 = ps;
    float *vin = ps + 16u * 2u * MID_R;
    constexpr u32 P = 64u;
    const u32 tid = threadIdx.x, j = blockIdx.x, Kf = a.Kf, kper = a.kper;
    const u32 w = __builtin_amdgcn_readfirstlane(tid >> 6), r0 = 4u * (tid & 63u);
    u32 nst = 0;
    auto stamp = [&]() {
        if (GQ_STAMPS && a.dbg && blockIdx.x == 32u && (tid & 63u) == 0u && nst < 8u) a.dbg[w * 8u + nst++] = __builtin_readcyclecounter();
    };
    stamp();
    // ---- requests.  First what stage 1 needs (the sums of the previous launch: the long latency), then the constants.
    // A row of the view is 256 bytes: 16 lanes x 16 bytes, so a wave instruction reads 4 whole rows (one row per thread -- 128
    // bytes at a 256-byte stride -- touched 64 cache lines per instruction: 11 us for the launch).  Rounds 0..2: gate rows
    // (tid / 16) + 64 i, rounds 3..5: up (the source of a round is uniform).
    const u32 c16 = tid & 15u, rq = tid >> 4;
    u32x4 xq[6];
    {
        const rsrc_t rg = make_rsrc(a.y32g, a.parts * a.n * 4u);
        const rsrc_t ru = make_rsrc(a.y32u, a.parts * a.n * 4u);
#pragma unroll
        for (u32 i = 0; i < 3; i++) {
            const u32 row = rq + 64u * i;
            const u32 off = row < Kf ? (row * P + 4u * c16) * 4u : 0x80000000u;  // (rows beyond Kf: out of range -> zeros)
            xq[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rg, (int)off, 0, 0));
            xq[3 + i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(ru, (int)off, 0, 0));
        }
    }
    // the tables: flat 16-byte units, 4 per thread and table (a wave instruction moves 1 KiB: 8 instead of 32 requests per wave)
    u32x4 tq[8];
    {
        const rsrc_t ro = make_rsrc(a.hadT_out, tbytes);
        const rsrc_t ri = make_rsrc(a.had_in, tbytes);
#pragma unroll
        for (u32 i = 0; i < 4; i++) {
            tq[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(ro, (int)((tid + MID_T * i) * 16u), 0, 0));
            tq[4 + i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(ri, (int)((tid + MID_T * i) * 16u), 0, 0));
        }
    }
    float svg = 0.f, svu = 0.f, sud = 0.f;
    if (tid < Kf) svg = a.sv32g[tid * P + j], svu = a.sv32u[tid * P + j], sud = a.su_down[tid * P + j];
    auto h4 = [](uint2 hw, u32 i) -> float { return (float)__builtin_bit_cast(h16, (uint16_t)((i >> 1 ? hw.y : hw.x) >> (16u * (i & 1u)))); };
    // ---- 1. column j of the row transforms: out_j = the butterfly tree of fwht_lds for output index j -- at the stage of bit m
    // the pair (lo, hi) becomes lo + hi (bit m of j clear) or lo - hi = lo + (-hi) (set): the same additions, bit for bit.
    // Bits 0, 1 inside the lane's 4 elements, bits 2..5 across the 16 lanes of the row (DPP butterflies: every lane ends with the sum)
    {
        auto flip = [](float v, u32 sm) { return __builtin_bit_cast(float, __builtin_bit_cast(u32, v) ^ sm); };
        const u32 s0 = (j & 1u) << 31, s1 = ((j >> 1) & 1u) << 31;
#pragma unroll
        for (u32 i = 0; i < 6; i++) {
            float e[4];
#pragma unroll
            for (u32 c = 0; c < 4; c++) {  // (through a scalar: this hipcc folds __builtin_bit_cast(float, vector[c]) to element 0)
                const u32 t = xq[i][c];
                e[c] = __builtin_bit_cast(float, t);
            }
            if (a.parts > 1u) {  // split-K parts, ascending: mirrors gqq::sum_parts4 (part 0 came through the buffer load above)
                const float *src = (i < 3u ? a.y32g : a.y32u);
                const u32 row = rq + 64u * (i % 3u);
                for (u32 p = 1; p < a.parts; p++)
                    if (row < Kf) {
                        const float4 t = *reinterpret_cast<const float4 *>(src + (size_t)p * a.n + row * P + 4u * c16);
                        e[0] += t.x, e[1] += t.y, e[2] += t.z, e[3] += t.w;
                    }
            }
            float t = (e[0] + flip(e[1], s0)) + flip(e[2] + flip(e[3], s0), s1);
#pragma unroll
            for (u32 m = 2; m < 6; m++) {
                int o = __builtin_bit_cast(int, t);
                if (m == 2u) o = __builtin_amdgcn_update_dpp(0, o, 0xB1, 0xF, 0xF, false);       // lane ^ 1
                else if (m == 3u) o = __builtin_amdgcn_update_dpp(0, o, 0x4E, 0xF, 0xF, false);  // lane ^ 2
                else if (m == 4u) {                                                              // lane ^ 4 = (^ 3) then (^ 7)
                    o = __builtin_amdgcn_update_dpp(0, o, 0x1B, 0xF, 0xF, false);
                    o = __builtin_amdgcn_update_dpp(0, o, 0x141, 0xF, 0xF, false);
                } else {                                                                         // lane ^ 8 = (^ 15) then (^ 7)
                    o = __builtin_amdgcn_update_dpp(0, o, 0x140, 0xF, 0xF, false);
                    o = __builtin_amdgcn_update_dpp(0, o, 0x141, 0xF, 0xF, false);
                }
                const float of = __builtin_bit_cast(float, o);
                const bool upper = (c16 >> (m - 2u)) & 1u;
                const float lo = upper ? of : t, hi = upper ? t : of;
                t = lo + flip(hi, ((j >> m) & 1u) << 31);
            }
            const u32 row = rq + 64u * (i % 3u);
            if (c16 == 0u && row < MID_R) xr[row * 2u + (i < 3u ? 0u : 1u)] = t;  // (rows beyond Kf: zeros)
        }
    }
    stamp();
#pragma unroll
    for (u32 i = 0; i < 4; i++) {
        const u32 u = tid + MID_T * i;
        if (u * 16u < tbytes) {
            *reinterpret_cast<u32x4 *>(smem + u * 16u) = tq[i];
            *reinterpret_cast<u32x4 *>(smem + tbytes + u * 16u) = tq[4 + i];
        }
    }
    __syncthreads();
    stamp();
    // ---- 2. out product, in the order of qtip_transform_kernel at P = 64: 16 k groups of kper terms, each summed from 0.f.
    // Branch-free: every LDS read of the group is issued before the first multiply (with a branch per k the compiler waits for each
    // read where it is used: 4,200 cycles for 11 terms); a term outside the group gets the factor 0 at a clamped address -- acc + 0 * x
    {
        float2 xk[MID_KP];
        uint2 hk[MID_KP];
#pragma unroll
        for (u32 kk = 0; kk < MID_KP; kk++) {
            const u32 k = w * kper + kk;
            const bool ok = kk < kper && k < Kf;
            const u32 kc = ok ? k : 0u;
            xk[kk] = *reinterpret_cast<const float2 *>(xr + 2u * kc);
            const uint2 hw = *reinterpret_cast<const uint2 *>(tabO + (kc * Kf + r0) * 2u);  // (lanes beyond Kf: inside the allocation, unused)
            hk[kk] = (ok && r0 < Kf) ? hw : make_uint2(0u, 0u);
        }
        float ag[4] = {0.f, 0.f, 0.f, 0.f}, au[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (u32 kk = 0; kk < MID_KP; kk++)
#pragma unroll
            for (u32 i = 0; i < 4; i++) {
                const float h = h4(hk[kk], i);
                ag[i] = __builtin_fmaf(h, xk[kk].x, ag[i]);
                au[i] = __builtin_fmaf(h, xk[kk].y, au[i]);
            }
        *reinterpret_cast<float4 *>(ps + (w * 2u + 0u) * MID_R + r0) = make_float4(ag[0], ag[1], ag[2], ag[3]);
        *reinterpret_cast<float4 *>(ps + (w * 2u + 1u) * MID_R + r0) = make_float4(au[0], au[1], au[2], au[3]);
    }
    __syncthreads();
    stamp();
    // ---- 3. the element-wise middle for row r = tid of column j: transform-out of gate and up, silu * up, transform-in element
    if (tid < MID_R) {
        float pg[16], pu[16];
#pragma unroll
        for (u32 q = 0; q < 16; q++) pg[q] = ps[(q * 2u + 0u) * MID_R + tid], pu[q] = ps[(q * 2u + 1u) * MID_R + tid];
        float yg = 0.f, yu = 0.f;
#pragma unroll
        for (u32 q = 0; q < 16; q++) yg += pg[q], yu += pu[q];
        const uint16_t g16 = __builtin_bit_cast(uint16_t, gqq::xf_out(yg, a.nscale, svg)), u16 = __builtin_bit_cast(uint16_t, gqq::xf_out(yu, a.nscale, svu));
        if (tid < Kf) {
            if (a.gout) a.gout[tid * P + j] = g16;
            if (a.uout) a.uout[tid * P + j] = u16;
        }
        vin[tid] = tid < Kf ? gqq::xf_in<gqq::QPRO_SILUMUL>(g16, u16, 0, 0.f, sud) : 0.f;
    }
    __syncthreads();
    stamp();
    // ---- 4. in product (hadK^T @, matmul_hadUt): z[r] = sum_k had[k][r] * vin[k], the 16 k groups added in ascending order
    {
        float xk[MID_KP];
        uint2 hk[MID_KP];
#pragma unroll
        for (u32 kk = 0; kk < MID_KP; kk++) {
            const u32 k = w * kper + kk;
            const bool ok = kk < kper && k < Kf;
            const u32 kc = ok ? k : 0u;
            xk[kk] = vin[kc];
            const uint2 hw = *reinterpret_cast<const uint2 *>(tabI + (kc * Kf + r0) * 2u);
            hk[kk] = (ok && r0 < Kf) ? hw : make_uint2(0u, 0u);
        }
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (u32 kk = 0; kk < MID_KP; kk++)
#pragma unroll
            for (u32 i = 0; i < 4; i++) acc[i] = __builtin_fmaf(h4(hk[kk], i), xk[kk], acc[i]);
        *reinterpret_cast<float4 *>(ps2 + w * MID_R + r0) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }
    __syncthreads();
    stamp();
    if (tid < Kf) {
        float z = 0.f;
#pragma unroll
        for (u32 g = 0; g < 16; g++) z += ps2[g * MID_R + tid];
        a.z32[tid * P + j] = z;
    }
    stamp();
}

// ------------------------------------------------------------------------------------------------ Hadamard (FWHT)
__global__ void __launch_bounds__(1024) fwht_kernel(const float *x, float *y, u32 n, float scale) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *v = reinterpret_cast<float *>(smem);
    const u32 T = blockDim.x, tid = threadIdx.x;
    const float *xr = x + (size_t)blockIdx.x * n;
    float *yr = y + (size_t)blockIdx.x * n;
    for (u32 i = tid; i < n; i += T) v[i] = xr[i];
    __syncthreads();
    fwht_lds(v, n);
    for (u32 i = tid; i < n; i += T) yr[i] = v[i] * scale;
}

bool pow2(u32 n) { return n && !(n & (n - 1u)); }
}  // namespace

unsigned long long *g_qdbg = nullptr;  // optional per-wave phase stamps of the middle block (tools/qtip_phase_timing.py)
extern "C" void gq_debug_set_qtip_timing_buffer(void *p) { g_qdbg = (unsigned long long *)p; }

float gq_inv_sqrt_f(uint32_t n) { return (float)pow((double)n, -0.5); }

GqQtipOutErr gq_qtip_out_desc(const GqQtipOut &g, bool need_out, gqq::QtipOut &o) {
    if (!g.y32 || !g.SV32 || (need_out && !g.out)) return GQ_QOUT_NULL;
    if (g.parts > 4u) return GQ_QOUT_PARTS;
    o = QtipOut{g.y32, g.SV32, (const uint16_t *)g.resid, (uint16_t *)g.out, g.M, gq_inv_sqrt_f(g.M), g.parts ? g.parts : 1u};
    return GQ_QOUT_OK;
}

extern "C" int gq_qtip_mlp_mid(const GqQtipMid *m, uint32_t parts, uint32_t n, uint32_t Kf, void *stream) {
    if (!m || !m->y32_gate || !m->y32_up || !m->SV32_gate || !m->SV32_up || !m->hadT_right16 || !m->SU_down || !m->had_left_down16 || !m->z32)
        return gq_fail(GQ_EINVAL, "gq_qtip_mlp_mid: null pointer argument.");
    if (Kf < 2u || n == 0 || n % Kf) return gq_fail(GQ_EINVAL, "gq_qtip_mlp_mid: n a multiple of Kf.");
    if (n / Kf != 64u || Kf > 176u || Kf % 4u)  // (both fp16 tables in LDS: 4 Kf^2 + 35 KiB <= 160 KiB)
        return gq_fail(GQ_ENOTSUP, "gq_qtip_mlp_mid: serves n = Kf * 64 with Kf <= 176, Kf % 4 == 0 (other widths: two gq_qtip_transform launches).");
    if (parts < 1u || parts > 4u) return gq_fail(GQ_EINVAL, "gq_qtip_mlp_mid: parts must be 1..4.");
    if (((uintptr_t)m->y32_gate | (uintptr_t)m->y32_up) & 15u) return gq_fail(GQ_EINVAL, "gq_qtip_mlp_mid: the sums must be 16-byte aligned.");
    if (((uintptr_t)m->hadT_right16 | (uintptr_t)m->had_left_down16) & 7u) return gq_fail(GQ_EINVAL, "gq_qtip_mlp_mid: the tables must be 8-byte aligned.");
    QtipMidArgs a{};
    a.y32g = m->y32_gate, a.y32u = m->y32_up, a.sv32g = m->SV32_gate, a.sv32u = m->SV32_up;
    a.hadT_out = (const uint16_t *)m->hadT_right16, a.had_in = (const uint16_t *)m->had_left_down16;
    a.su_down = m->SU_down, a.z32 = m->z32;
    a.gout = (uint16_t *)m->gate_out, a.uout = (uint16_t *)m->up_out;
    a.parts = parts, a.n = n, a.Kf = Kf;
    a.kper = (Kf + 15u) / 16u;  // (qtip_transform_kernel: KQ = 1024 / 64 = 16 k groups)
    a.nscale = gq_inv_sqrt_f(n);
    a.dbg = g_qdbg;
    const size_t smem = 2u * (size_t)Kf * Kf * 2u + (MID_R * 2u + 16u * 2u * MID_R + MID_R) * 4u;
    static GqPerDeviceOnce once;
    GQ_HIP_CHECK(once.max_dynamic_lds(reinterpret_cast<const void *>(qtip_mlp_mid_kernel), 160 * 1024));
    hipLaunchKernelGGL(qtip_mlp_mid_kernel, dim3(64u), dim3(MID_T), smem, (hipStream_t)stream, a);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}

extern "C" int gq_qtip_linear_out(int n, const GqQtipOut *lin, void *stream) {
    if (!lin || n < 1 || n > 3) return gq_fail(GQ_EINVAL, "gq_qtip_linear_out: 1..3 linears.");
    QtipOutArgs a{};
    u32 maxM = 0;
    for (int i = 0; i < n; i++) {
        const GqQtipOutErr e = gq_qtip_out_desc(lin[i], true, a.lin[i]);
        if (e == GQ_QOUT_NULL) return gq_fail(GQ_EINVAL, "gq_qtip_linear_out: null pointer argument.");
        if (!pow2(lin[i].M) || lin[i].M < 32u || lin[i].M > 32768u)
            return gq_fail(GQ_ENOTSUP, "fused QTIP linear: M must be a power of two in 32..32768.");
        if (e == GQ_QOUT_PARTS) return gq_fail(GQ_EINVAL, "gq_qtip_linear_out: parts must be 0..4.");
        if (lin[i].M > maxM) maxM = lin[i].M;
    }
    const size_t smem = (size_t)maxM * 4u;
    static GqPerDeviceOnce once;
    GQ_HIP_CHECK(once.max_dynamic_lds(reinterpret_cast<const void *>(qtip_linear_out_kernel), 160 * 1024));
    hipLaunchKernelGGL(qtip_linear_out_kernel, dim3((u32)n), dim3(1024), smem, (hipStream_t)stream, a);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}

extern "C" int gq_qtip_linear_out_in(const GqQtipOut *prev, const void *norm_weight, float eps, int n_next, const float *const *SU_next,
                                     void *const *xt_next, void *stream) {
    if (!prev || !norm_weight || !SU_next || !xt_next || n_next < 1 || n_next > 3) return gq_fail(GQ_EINVAL, "gq_qtip_linear_out_in: 1..3 consumers, no null pointers.");
    const u32 K = prev->M;
    if (!pow2(K) || K < 256u || K > 8192u) return gq_fail(GQ_ENOTSUP, "gq_qtip_linear_out_in: width must be a power of two in 256..8192.");
    QtipOutInArgs a{};
    if (gq_qtip_out_desc(*prev, false, a.prev) != GQ_QOUT_OK) return gq_fail(GQ_EINVAL, "gq_qtip_linear_out_in: producing linear (y32, SV32, parts <= 4).");
    if (((uintptr_t)prev->y32 | (uintptr_t)prev->SV32 | (uintptr_t)norm_weight) & 15u || ((uintptr_t)prev->resid | (uintptr_t)prev->out) & 7u)
        return gq_fail(GQ_EINVAL, "gq_qtip_linear_out_in: buffers must be 16-byte (fp16 vectors: 8-byte) aligned.");
    a.normw = (const uint16_t *)norm_weight;
    a.eps = eps;
    a.kscale = a.prev.mscale;  // (the consumers' width is the producer's)
    for (int i = 0; i < n_next; i++) {
        if (!SU_next[i] || !xt_next[i] || (((uintptr_t)SU_next[i] | (uintptr_t)xt_next[i]) & 15u)) return gq_fail(GQ_EINVAL, "gq_qtip_linear_out_in: consumer vectors (16-byte aligned).");
        a.SU[i] = SU_next[i];
        a.xt[i] = (uint16_t *)xt_next[i];
    }
    hipLaunchKernelGGL(qtip_out_in_kernel, dim3((unsigned)n_next), dim3(1024), (size_t)K * 6u, (hipStream_t)stream, a);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}

extern "C" int gq_qtip_linear_out_seg(int n, const GqQtipOut *lin, void *stream) {
    if (!lin || n < 1 || n > 3) return gq_fail(GQ_EINVAL, "gq_qtip_linear_out_seg: 1..3 linears.");
    QtipOutArgs a{};
    u32 maxM = 0;
    for (int i = 0; i < n; i++) {
        const GqQtipOutErr e = gq_qtip_out_desc(lin[i], true, a.lin[i]);
        if (e == GQ_QOUT_NULL) return gq_fail(GQ_EINVAL, "gq_qtip_linear_out_seg: null pointer argument.");
        if (!pow2(lin[i].M) || lin[i].M < QSEG || lin[i].M > 16u * QSEG_T)
            return gq_fail(GQ_ENOTSUP, "gq_qtip_linear_out_seg: M must be a power of two in 128..8192 (else gq_qtip_linear_out).");
        if (e == GQ_QOUT_PARTS) return gq_fail(GQ_EINVAL, "gq_qtip_linear_out_seg: parts must be 0..4.");
        if (((uintptr_t)lin[i].y32) & 15u) return gq_fail(GQ_EINVAL, "gq_qtip_linear_out_seg: the sums must be 16-byte aligned.");
        if (lin[i].M > maxM) maxM = lin[i].M;
    }
    hipLaunchKernelGGL(qtip_linear_out_seg_kernel, dim3(maxM / QSEG, (u32)n), dim3(QSEG_T), 0, (hipStream_t)stream, a);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}

extern "C" int gq_qtip_transform(int input_side, const void *x, const void *x2, const void *norm_weight, float eps, int prologue,
                                 int n_lin, const GqQtipXf *lin, uint32_t n, uint32_t Kf, int transpose, void *stream) {
    if (!lin || n_lin < 1 || n_lin > 3 || Kf < 2u || n == 0 || n % Kf) return gq_fail(GQ_EINVAL, "gq_qtip_transform: 1..3 linears; n a multiple of Kf.");
    const u32 P = n / Kf;
    if (!pow2(P) || P < 64u || n > 32768u) return gq_fail(GQ_ENOTSUP, "gq_qtip_transform: n / Kf must be a power of two >= 64, n <= 32768.");
    if (input_side && (!x || (prologue == GQ_QPRO_RMSNORM && !norm_weight) || (prologue == GQ_QPRO_SILU_MUL && !x2) || prologue < 0 || prologue > 2))
        return gq_fail(GQ_EINVAL, "gq_qtip_transform: source operand missing.");
    if (((uintptr_t)x | (uintptr_t)x2 | (uintptr_t)norm_weight) & 15u) return gq_fail(GQ_EINVAL, "gq_qtip_transform: buffers must be 16-byte aligned.");
    QtipXfArgs a{};
    a.x = (const uint16_t *)x;
    a.x2 = (const uint16_t *)x2;
    a.normw = (const uint16_t *)norm_weight;
    for (int i = 0; i < n_lin; i++) {
        if (((uintptr_t)lin[i].y32 | (uintptr_t)lin[i].vec) & 15u) return gq_fail(GQ_EINVAL, "gq_qtip_transform: buffers must be 16-byte aligned.");
        if (!lin[i].vec || !lin[i].out || !lin[i].hadK || (!input_side && !lin[i].y32)) return gq_fail(GQ_EINVAL, "gq_qtip_transform: null pointer argument.");
        a.lin[i] = QtipXfLin{lin[i].y32, lin[i].vec, lin[i].hadK, (const uint16_t *)lin[i].resid, (uint16_t *)lin[i].out};
    }
    a.eps = eps;
    a.nscale = gq_inv_sqrt_f(n);
    a.n = n;
    a.Kf = Kf;
    a.P = P;
    a.RB = (u32)gq_env_int("GQ_QTIP_XF_RB", P >= 256u ? 1 : (P >= 128u ? 2 : 4));  // rows of the result per block (<= 4)
    if (a.RB < 1u || a.RB > 4u) a.RB = 1u;
    a.in = input_side ? 1u : 0u;
    a.pro = input_side ? (u32)prologue : 0u;
    a.transpose = transpose ? 1u : 0u;
    const u32 KQ = P >= 1024u ? 1u : 1024u / P;
    const size_t smem = ((size_t)n + 4u * (size_t)Kf + (size_t)KQ * a.RB * P) * 4u;
    if (smem > 150u * 1024u) return gq_fail(GQ_ENOTSUP, "gq_qtip_transform: n too large.");
    static GqPerDeviceOnce once;
    GQ_HIP_CHECK(once.max_dynamic_lds(reinterpret_cast<const void *>(qtip_transform_kernel), 156 * 1024));
    hipLaunchKernelGGL(qtip_transform_kernel, dim3((Kf + a.RB - 1u) / a.RB, (u32)n_lin), dim3(1024), smem, (hipStream_t)stream, a);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}

extern "C" int gq_hadamard(const float *x, float *y, uint32_t rows, uint32_t n, float scale, void *stream) {
    if (!x || !y) return gq_fail(GQ_EINVAL, "null pointer argument.");
    if (n == 0 || (n & (n - 1u))) return gq_fail(GQ_EINVAL, "hadamard: the last dimension must be a power of two.");
    if (rows == 0) return GQ_OK;
    const size_t smem = (size_t)n * 4u;
    if (smem > 160u * 1024u) return gq_fail(GQ_ENOTSUP, "hadamard: n too large (<= 32768).");
    static GqPerDeviceOnce once;
    GQ_HIP_CHECK(once.max_dynamic_lds(reinterpret_cast<const void *>(fwht_kernel), 160 * 1024));
    const u32 T = n / 2u >= 1024u ? 1024u : (n / 2u >= 64u ? n / 2u : 64u);
    hipLaunchKernelGGL(fwht_kernel, dim3(rows), dim3(T), smem, (hipStream_t)stream, x, y, n, scale);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}
