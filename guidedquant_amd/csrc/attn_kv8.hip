// attn_kv8.hip -- gq_attn_decode_split_kv8: the gq_attn_decode_split family (decode.hip, attn_decode_kernel: plain / _qknorm / _bias,
// each with a window form) over an fp8 (e4m3) KV cache.  ONE launch behind the plain wqkv GEMV takes the packed q | k | v vector, adds
// the bias or applies the per-head norm, rotates, QUANTISES k and v of the current token by the write rule, writes the cache row and
// attends -- what gq_rope_cache_rows_kv8 (S = 1) -> gq_attn_decode_roped_kv8 do in two launches, bit for bit (include/gq_hip.h).
//
// How the work is split.  The block of a (head, split) has GQ_ATTN_WAVES waves.  The current token is prepared by HD / 16 lanes each of
// three waves -- wave 0: q of the head, wave 1: k of its KV group, wave 2: v -- in the units of the row write (prefill.hip,
// rope_cache_rows_kernel): a lane owns elements d .. d + 7 and d + HD / 2 .. of its vector, two 16-byte loads, so the rotation partners
// are its own registers, the QK-norm statistic is the row write's (16 squares per lane in element order, then an xor butterfly over the
// HD / 16 lanes: the same sum bit for bit, which a sum in another order is not), and the 8 codes of a unit are one 8-byte store.  The three
// waves run side by side; the other waves wait at the barrier.  LDS takes the rotated q and, for k and v, the DEQUANTISED codes
// (float(code), exact: every e4m3 value is an fp16 value), so every block that attends position *pos attends what the cache will hold
// whether or not the row has landed, and the result is a function of the cache alone.  Behind the barrier: the position streams of
// attn_core.h over 8-byte cached rows (K scale folded into the score factor), the merge of attn_roped_kernel (factors e^(m_i - M) once
// per stream through LDS, streams of a head in ascending order), V scale on the merged sum in front of the division / the workspace.
//
// A translation unit of its own: it is compiled with packed fp32 math off (csrc/Makefile), which decode.hip's kernels are not, and they
// keep their instructions.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gq_internal.h"
#include "attn_core.h"
#include "kv_fmt.h"
#include "wave_util.h"

namespace {

typedef uint32_t u32;
using gqw::h16;
using gqw::h2f;
using gqw::h2u;
using gqw::u2h;
using gq_attn::AttnGeom;
using gq_attn::AttnWindow;
using gq_attn::window_lo;

constexpr int ATTN_WAVES = GQ_ATTN_WAVES;

// the optional forms, compile-time like decode.hip's: an instance without the form takes an empty argument
template <bool QKN>
struct Kv8QkNorm {};
template <>
struct Kv8QkNorm<true> {
    const uint16_t *qw, *kw;  // q_norm / k_norm weights, fp16 [HD]
    float eps;
};
template <bool QB>
struct Kv8Bias {};
template <>
struct Kv8Bias<true> {
    const uint16_t *qkv;  // fp16 [(H + 2 Hkv) * HD], laid out like the packed vector
};
struct Kv8Scales {
    const float *k_inv, *v_inv, *k_scale, *v_scale;  // fp32 [Hkv] each: the write rule's reciprocals, the read rule's scales
};

// KV group of query head h (decode.hip, kv_group_of: shifts for the group sizes of every Llama, the quotient otherwise)
__device__ __forceinline__ u32 kv_group_of(u32 h, u32 H, u32 Hkv) {
    if (H == Hkv) return h;
    if (H == 4u * Hkv) return h >> 2;
    if (H == 8u * Hkv) return h >> 3;
    if (H == 2u * Hkv) return h >> 1;
    return h / (H / Hkv);
}
__device__ __forceinline__ void words(const uint4 &v, u32 (&w)[4]) { w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w; }
// 8 floats of a unit into LDS (two 16-byte stores: d is a multiple of 8)
__device__ __forceinline__ void stage8(float *dst, const float (&f)[8]) {
    reinterpret_cast<float4 *>(dst)[0] = make_float4(f[0], f[1], f[2], f[3]);
    reinterpret_cast<float4 *>(dst)[1] = make_float4(f[4], f[5], f[6], f[7]);
}

template <int HD, bool QKN, bool QB, bool WIN>
__global__ void __launch_bounds__(64 * ATTN_WAVES) attn_decode_kv8_kernel(const uint16_t *qkv, const int *pos_ptr, const uint16_t *cos_t,
                                                                          const uint16_t *sin_t, uint8_t *kc, uint8_t *vc, Kv8Scales k8,
                                                                          uint16_t *out, u32 H, u32 Hkv, u32 max_seq, float scale, u32 nsplit,
                                                                          float *ws, Kv8QkNorm<QKN> nm, Kv8Bias<QB> bs, AttnWindow<WIN> wn) {
    static_assert(!(QKN && QB), "the norm form and the bias form do not combine");
    static_assert(ATTN_WAVES >= 3, "q, k and v of the current token take a wave each");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using Geo = AttnGeom<HD>;
    using L = gq_attn::DecodeLds<HD>;
    constexpr u32 NW = Geo::NW, NS = Geo::NS, UPR = HD / 16;
    constexpr int LPP = Geo::LPP, PPW = Geo::PPW, U = Geo::U;
    static_assert(4 * HD + 2 * NW >= NS + 1, "the merge factors take the place of the norm scratch");
    float *lds = reinterpret_cast<float *>(smem);
    float *sc = lds + L::sc, *qs = lds + L::qs, *kcur = lds + L::kcur, *vcur = lds + L::vcur, *fl = lds + L::red, *red2 = lds + L::red2;
    const u32 tid = threadIdx.x, w = tid >> 6, l = tid & 63u;
    const u32 h = blockIdx.x, g = kv_group_of(h, H, Hkv), sp = blockIdx.y;
    // the current token: wave 0 q, wave 1 k, wave 2 v; lane u < UPR owns elements 8 u .. and 8 u + HD / 2 .. (the lanes behind repeat the
    // loads of lane u % UPR, so that whole waves run the butterfly below, and write nothing).  Nothing here depends on the position: the
    // loads go out before it is read.
    const u32 d = 8u * (l % UPR);
    const u32 hh = w == 0u ? h : (w == 1u ? H + g : H + Hkv + g);  // the head of the packed vector (and of the bias)
    u32 x1[4] = {0, 0, 0, 0}, x2[4] = {0, 0, 0, 0};
    float inv = 0.f;
    if (w < 3u) {
        const uint16_t *src = qkv + (size_t)hh * HD;
        words(*reinterpret_cast<const uint4 *>(src + d), x1);
        words(*reinterpret_cast<const uint4 *>(src + d + HD / 2), x2);
        if constexpr (QB) {  // ONE fp16 add on q, k and v in front of the rotation (decode.hip, AttnBias)
            const uint16_t *br = bs.qkv + (size_t)hh * HD;
            u32 b1[4], b2[4];
            words(*reinterpret_cast<const uint4 *>(br + d), b1);
            words(*reinterpret_cast<const uint4 *>(br + d + HD / 2), b2);
#pragma unroll
            for (int e = 0; e < 4; e++) {
                u32 r1 = 0, r2 = 0;
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const u32 sh = 16u * (u32)k;
                    r1 |= (u32)h2u(u2h((uint16_t)(x1[e] >> sh)) + u2h((uint16_t)(b1[e] >> sh))) << sh;
                    r2 |= (u32)h2u(u2h((uint16_t)(x2[e] >> sh)) + u2h((uint16_t)(b2[e] >> sh))) << sh;
                }
                x1[e] = r1, x2[e] = r2;
            }
        }
        if (w > 0u) inv = (w == 1u ? k8.k_inv : k8.v_inv)[g];
    }
    scale *= k8.k_scale[g];  // (block-uniform: the K scale is one factor of every score)
    const u32 pos = (u32)pos_ptr[0];
    if (pos >= max_seq) {  // decoding past the cache: nothing is written to it, the head's output is poisoned (NaN logits)
        if (sp == 0u && tid < HD) out[(size_t)h * HD + tid] = 0x7e00u;
        return;
    }
    uint8_t *kcg = kc + (size_t)g * max_seq * HD, *vcg = vc + (size_t)g * max_seq * HD;
    // the rows [p0, p1) of this block (attn_core.h: the solo rule, the rows of a split)
    const u32 lo = window_lo(pos, wn), n = pos + 1u - lo;
    if (gq_attn::attn_solo<HD>(n, nsplit)) {
        if (sp > 0u) return;
        nsplit = 1u;
    }
    const u32 per = gq_attn::attn_per<HD>(n, nsplit);
    const u32 p0 = lo + sp * per, p1 = min(pos + 1u, p0 + per);
    const bool has_cur = p0 <= pos && pos < p1;  // the split that covers the current token ...
    const bool writes = has_cur && h == g * (H / Hkv);  // ... and of its blocks the first head of the KV group: the owner of the cache row
    if (w < 3u) {
        if constexpr (QKN) {
            if (w < 2u) {  // (wave-uniform; v is not normed)
                // the statistic of the row write: 16 squares per lane in element order, then the butterfly over the UPR lanes of the head
                float ss = 0.f;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const float f0 = h2f((uint16_t)(x1[e] & 0xFFFF)), f1 = h2f((uint16_t)(x1[e] >> 16));
                    ss += f0 * f0;
                    ss += f1 * f1;
                }
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const float f0 = h2f((uint16_t)(x2[e] & 0xFFFF)), f1 = h2f((uint16_t)(x2[e] >> 16));
                    ss += f0 * f0;
                    ss += f1 * f1;
                }
#pragma unroll
                for (u32 sh = 1u; sh < UPR; sh <<= 1) ss += __shfl_xor(ss, (int)sh, 64);
                const float rs = rsqrtf(ss / (float)HD + nm.eps);
                const uint16_t *wn16 = w == 0u ? nm.qw : nm.kw;
                u32 w1[4], w2[4];
                words(*reinterpret_cast<const uint4 *>(wn16 + d), w1);
                words(*reinterpret_cast<const uint4 *>(wn16 + d + HD / 2), w2);
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    u32 r1 = 0, r2 = 0;
#pragma unroll
                    for (int k = 0; k < 2; k++) {  // (x.float() * rsqrt(..)).half() * weight
                        const u32 sh = 16u * (u32)k;
                        // (the product pinned in fp32: two roundings, as the row write and the tensor expression make them -- folded into
                        // the conversion it would be rounded once, gq_internal.h)
                        const h16 v1 = (h16)gq_pin_f32(h2f((uint16_t)(x1[e] >> sh)) * rs) * u2h((uint16_t)(w1[e] >> sh));
                        const h16 v2 = (h16)gq_pin_f32(h2f((uint16_t)(x2[e] >> sh)) * rs) * u2h((uint16_t)(w2[e] >> sh));
                        r1 |= (u32)h2u(v1) << sh;
                        r2 |= (u32)h2u(v2) << sh;
                    }
                    x1[e] = r1, x2[e] = r2;
                }
            }
        }
        if (w < 2u) {  // apply_rotary_pos_emb on the unit: (x * cos) + (rotate_half(x) * sin), three fp16 operations per element
            const uint16_t *cr = cos_t + (size_t)pos * HD, *sr = sin_t + (size_t)pos * HD;
            u32 c1[4], c2[4], s1[4], s2[4];
            words(*reinterpret_cast<const uint4 *>(cr + d), c1);
            words(*reinterpret_cast<const uint4 *>(cr + d + HD / 2), c2);
            words(*reinterpret_cast<const uint4 *>(sr + d), s1);
            words(*reinterpret_cast<const uint4 *>(sr + d + HD / 2), s2);
#pragma unroll
            for (int e = 0; e < 4; e++) {
                u32 r1 = 0, r2 = 0;
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const u32 sh = 16u * (u32)k;
                    const h16 a1 = u2h((uint16_t)(x1[e] >> sh)), a2 = u2h((uint16_t)(x2[e] >> sh));
                    // first half:  x1 * cos + (-x2) * sin ;  second half:  x2 * cos + x1 * sin   (rotate_half = cat(-x2, x1))
                    const h16 f = (a1 * u2h((uint16_t)(c1[e] >> sh))) + ((-a2) * u2h((uint16_t)(s1[e] >> sh)));
                    const h16 gg = (a2 * u2h((uint16_t)(c2[e] >> sh))) + (a1 * u2h((uint16_t)(s2[e] >> sh)));
                    r1 |= (u32)h2u(f) << sh;
                    r2 |= (u32)h2u(gg) << sh;
                }
                x1[e] = r1, x2[e] = r2;
            }
        }
        // x1 / x2 now hold the fp16 values the fp16 path would attend (q) or store (k, v)
        float f1[8], f2[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            f1[k] = h2f((uint16_t)(x1[k >> 1] >> (16 * (k & 1))));
            f2[k] = h2f((uint16_t)(x2[k >> 1] >> (16 * (k & 1))));
        }
        if (w == 0u) {
            if (l < UPR) stage8(qs + d, f1), stage8(qs + d + HD / 2, f2);
        } else {
            // the write rule, then the read rule's conversion: what LDS holds is what the cache row holds
#pragma unroll
            for (int k = 0; k < 8; k++) f1[k] *= inv, f2[k] *= inv;
            const uint2 q1 = gq_kv::fp8_quant8<true>(f1), q2 = gq_kv::fp8_quant8<true>(f2);
            gq_kv::unpack8_fp8(q1, f1);
            gq_kv::unpack8_fp8(q2, f2);
            if (l < UPR) {
                float *cur = w == 1u ? kcur : vcur;
                stage8(cur + d, f1), stage8(cur + d + HD / 2, f2);
                if (writes) {  // (off the critical path; 8 codes of a unit = one 8-byte store, a row = one line)
                    uint8_t *row = (w == 1u ? kcg : vcg) + (size_t)pos * HD;
                    *reinterpret_cast<uint2 *>(row + d) = q1;
                    *reinterpret_cast<uint2 *>(row + d + HD / 2) = q2;
                }
            }
        }
    }
    __syncthreads();
    // One pass, online softmax per position stream (attn_core.h); the K and the V rows of a batch are requested together
    const u32 sub = l / LPP, ld = l % LPP;
    float qreg[8];
#pragma unroll
    for (int e = 0; e < 8; e++) qreg[e] = qs[ld * 8 + e];
    float m_run = -3.0e38f, s_run = 0.f, acc[8];
#pragma unroll
    for (int e = 0; e < 8; e++) acc[e] = 0.f;
    for (u32 t0 = p0 + w * PPW * U; t0 < p1; t0 += NW * PPW * U) {
        uint2 kv[U], vv[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const u32 t = t0 + (u32)u * PPW + sub;
            const bool cached = t < pos && t < p1;  // (t < p1 <= pos + 1 <= max_seq: inside the cache)
            kv[u] = cached ? *reinterpret_cast<const uint2 *>(kcg + (size_t)t * HD + ld * 8) : make_uint2(0, 0);
            vv[u] = cached ? *reinterpret_cast<const uint2 *>(vcg + (size_t)t * HD + ld * 8) : make_uint2(0, 0);
        }
        float pu[U], vfu[U][8];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const u32 t = t0 + (u32)u * PPW + sub;
            float kf[8];
            gq_kv::unpack8_fp8(kv[u], kf);
            gq_kv::unpack8_fp8(vv[u], vfu[u]);
            if (t == pos) {  // (the current token: staged in LDS above, its cache row may not have landed)
#pragma unroll
                for (int e = 0; e < 8; e++) kf[e] = kcur[ld * 8 + e], vfu[u][e] = vcur[ld * 8 + e];
            }
            float p = 0.f;
#pragma unroll
            for (int e = 0; e < 8; e++) p += qreg[e] * kf[e];
            p = gq_attn::row_sum<LPP>(p);  // (every lane takes part: in front of the select)
            pu[u] = t < p1 ? p * scale : -3.0e38f;
        }
        gq_attn::softmax_update<U>(m_run, s_run, acc, pu, vfu);
    }
    const u32 stream = w * PPW + sub;
#pragma unroll
    for (int e = 0; e < 8; e++) red2[stream * HD + ld * 8 + e] = acc[e];
    if (ld == 0) {
        sc[stream] = m_run;
        sc[NS + stream] = s_run;
    }
    __syncthreads();
    // the merge of attn_core.h, as attn_roped_kernel spells it: the factors and the maximum of the head to fl [NS] + [1] ..
    const u32 ng = gq_attn::merge_groups<HD>(p1 - p0);
    if (tid < NS) {
        float M = -3.0e38f;
        for (u32 g8 = 0; g8 < ng; g8++)
#pragma unroll
            for (u32 k = 0; k < 8u; k++) M = fmaxf(M, sc[8u * g8 + k]);
        fl[tid] = __expf(sc[tid] - M);
        if (tid == 0u) fl[NS] = M;
    }
    __syncthreads();
    if (tid < HD) {  // .. then thread dd: the streams merged in ascending order
        const float M = fl[NS];
        float o = 0.f, sum = 0.f;
        for (u32 g8 = 0; g8 < ng; g8++)
#pragma unroll
            for (u32 k = 0; k < 8u; k++) gq_attn::merge_step<HD>(sc, red2, fl, 8u * g8 + k, tid, o, sum);
        o *= k8.v_scale[g];  // (the V scale: in front of the division and the one fp16 rounding, or of the workspace)
        if (nsplit > 1u) {
            float *wp = ws + ((size_t)h * nsplit + sp) * (HD + 2u);
            wp[tid] = o;
            if (tid == 0) {
                wp[HD] = M;
                wp[HD + 1] = sum;
            }
        } else {
            out[(size_t)h * HD + tid] = h2u((h16)(o / sum));
        }
    }
}

template <bool QKN, bool QB, bool WIN>
int kv8_launch(const void *qkv, const int *pos, const void *cos_table, const void *sin_table, void *k_cache, void *v_cache, const Kv8Scales &k8,
               void *out, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq, float scale, uint32_t n_split, float *workspace,
               const void *q_norm_weight, const void *k_norm_weight, float eps, const void *qkv_bias, uint32_t window, hipStream_t s) {
    Kv8QkNorm<QKN> nm{};
    if constexpr (QKN) nm = Kv8QkNorm<true>{(const uint16_t *)q_norm_weight, (const uint16_t *)k_norm_weight, eps};
    Kv8Bias<QB> bs{};
    if constexpr (QB) bs = Kv8Bias<true>{(const uint16_t *)qkv_bias};
    AttnWindow<WIN> wn{};
    if constexpr (WIN) wn = AttnWindow<true>{window};
    const dim3 grid(n_head, n_split);
#define GQ_LAUNCH_KV8(HD_)                                                                                                                  \
    do {                                                                                                                                    \
        static GqPerDeviceOnce once;                                                                                                        \
        GQ_HIP_CHECK(once.max_dynamic_lds(reinterpret_cast<const void *>(attn_decode_kv8_kernel<HD_, QKN, QB, WIN>), 160 * 1024));          \
        hipLaunchKernelGGL((attn_decode_kv8_kernel<HD_, QKN, QB, WIN>), grid, dim3(64 * ATTN_WAVES), gq_attn::DecodeLds<HD_>::bytes(false), s, \
                           (const uint16_t *)qkv, pos, (const uint16_t *)cos_table, (const uint16_t *)sin_table, (uint8_t *)k_cache,        \
                           (uint8_t *)v_cache, k8, (uint16_t *)out, n_head, n_kv_head, max_seq, scale, n_split, workspace, nm, bs, wn);     \
    } while (0)
    if (head_dim == 128) GQ_LAUNCH_KV8(128);
    else GQ_LAUNCH_KV8(64);
#undef GQ_LAUNCH_KV8
    return GQ_OK;
}
}  // namespace

extern "C" int gq_attn_decode_split_kv8(const void *qkv, const int *pos, const void *cos_table, const void *sin_table, void *k_cache,
                                        void *v_cache, const float *k_inv, const float *v_inv, const float *k_scale, const float *v_scale,
                                        void *out, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq, float scale,
                                        uint32_t n_split, float *workspace, const void *q_norm_weight, const void *k_norm_weight, float eps,
                                        const void *qkv_bias, uint32_t window, void *stream) {
    const bool qkn = q_norm_weight || k_norm_weight;
    if (qkn && (!q_norm_weight || !k_norm_weight)) return gq_fail(GQ_EINVAL, "gq_attn_decode_split_kv8: both norm weights or none.");
    if (qkn && qkv_bias) return gq_fail(GQ_EINVAL, "gq_attn_decode_split_kv8: the norm form and the bias form do not combine.");
    const bool any_null = !qkv || !pos || !cos_table || !sin_table || !k_cache || !v_cache || !k_inv || !v_inv || !k_scale || !v_scale || !out;
    // (16-byte units of the packed vector, the tables, the weights and the bias; 8-byte units of the cache rows)
    const char *misaligned = (((uintptr_t)qkv | (uintptr_t)cos_table | (uintptr_t)sin_table | (uintptr_t)k_cache | (uintptr_t)v_cache |
                               (uintptr_t)q_norm_weight | (uintptr_t)k_norm_weight | (uintptr_t)qkv_bias) & 15u)
                                 ? "gq_attn_decode_split_kv8: 16-byte aligned pointers."
                                 : nullptr;
    if (const int rc = gq_attn_check_args(any_null, misaligned, n_head, n_kv_head, head_dim, n_split, workspace)) return rc;
    const Kv8Scales k8 = {k_inv, v_inv, k_scale, v_scale};
    hipStream_t s = (hipStream_t)stream;
    int rc;
#define GQ_KV8_FORM(QKN_, QB_)                                                                                                          \
    rc = window ? kv8_launch<QKN_, QB_, true>(qkv, pos, cos_table, sin_table, k_cache, v_cache, k8, out, n_head, n_kv_head, head_dim, max_seq, \
                                              scale, n_split, workspace, q_norm_weight, k_norm_weight, eps, qkv_bias, window, s)       \
                : kv8_launch<QKN_, QB_, false>(qkv, pos, cos_table, sin_table, k_cache, v_cache, k8, out, n_head, n_kv_head, head_dim, max_seq, \
                                               scale, n_split, workspace, q_norm_weight, k_norm_weight, eps, qkv_bias, 0u, s)
    if (qkn) GQ_KV8_FORM(true, false);
    else if (qkv_bias) GQ_KV8_FORM(false, true);
    else GQ_KV8_FORM(false, false);
#undef GQ_KV8_FORM
    if (rc) return rc;
    if (n_split > 1u) gq_attn_combine_launch(workspace, out, n_head, head_dim, n_split, pos, max_seq, window, stream);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}
