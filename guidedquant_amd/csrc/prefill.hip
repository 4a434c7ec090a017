// prefill.hip -- the element-wise steps of the PROMPT pass (seq_len > 1) between the fused prefill GEMMs (ap_gemm.hip), one
// launch each instead of the ~45 eager tensor ops per layer of the module forward (inference/model.py:121-266 semantics:
// `Transformer.forward` -> `TransformerBlock.forward` -> `Attention.forward` / `FeedForward.forward`).  At S = 128 the
// module forward of the 8B model spends 10 of its 14.5 ms in launch overhead of those ops; the GEMMs take 4.2 ms.
// Every kernel keeps the fp16 rounding points of the tensor expressions it replaces:
//   gq_rmsnorm_rows     RMSNorm.forward (model.py:84-96):  (x.float() * rsqrt(mean(x^2) + eps)).half() * weight, optionally
//                       behind the residual add in front of it (TransformerBlock.forward, model.py:311-313: h = x + attn(..))
//   gq_rope_cache_rows  apply_rotary_pos_emb (model.py:336-341) on q and k -- (q * cos) + (rotate_half(q) * sin), three fp16
//                       operations -- and KVCache.update (model.py:69-79): k, v written at their positions
//   gq_silu_mul_rows    FeedForward.forward (model.py:266):  F.silu(w1(x)) * w3(x), silu rounded to fp16 before the product
// All of them are HBM-bound streams over [S][D] fp16 rows; 16-byte accesses, one block per row (norm) / grid-stride.
#include <hip/hip_runtime.h>

#include "gq_internal.h"
#include "wave_util.h"

namespace {
using u32 = uint32_t;
using gqw::f2h;
using gqw::h16;
using gqw::h2f;
using gqw::h2u;
using gqw::u2h;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) v += __shfl_xor(v, sh, 64);
    return v;
}

// one block (256 threads) per row; the row stays in registers between the two passes (D <= 256 * 8 * 8 = 16384)
// delta != null: the residual add of the block in front (x = x + delta, one fp16 rounding, written back) rides along
__global__ void __launch_bounds__(256) rmsnorm_rows_kernel(uint16_t *__restrict__ x, const uint16_t *__restrict__ delta, const uint16_t *__restrict__ w,
                                                           uint16_t *__restrict__ out, u32 D, float eps) {
    __shared__ float red[4];
    const u32 tid = threadIdx.x, row = blockIdx.x, nu = D / 8u;  // 16-byte units of the row
    uint4 *xr = reinterpret_cast<uint4 *>(x + (size_t)row * D);
    const uint4 *dr = delta ? reinterpret_cast<const uint4 *>(delta + (size_t)row * D) : nullptr;
    uint4 v[8];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const u32 u = tid + 256u * (u32)i;
        v[i] = u < nu ? xr[u] : make_uint4(0u, 0u, 0u, 0u);
        if (delta && u < nu) {
            const uint4 dv = dr[u];
            const u32 xa[4] = {v[i].x, v[i].y, v[i].z, v[i].w}, da[4] = {dv.x, dv.y, dv.z, dv.w};
            u32 r[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const h16 lo = u2h((uint16_t)(xa[e] & 0xFFFF)) + u2h((uint16_t)(da[e] & 0xFFFF)), hi = u2h((uint16_t)(xa[e] >> 16)) + u2h((uint16_t)(da[e] >> 16));
                r[e] = (u32)h2u(lo) | ((u32)h2u(hi) << 16);
            }
            v[i] = make_uint4(r[0], r[1], r[2], r[3]);
            xr[u] = v[i];
        }
        const u32 ww[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const float a = h2f((uint16_t)(ww[e] & 0xFFFF)), b = h2f((uint16_t)(ww[e] >> 16));
            ss += a * a;
            ss += b * b;
        }
    }
    ss = wave_sum(ss);
    if ((tid & 63u) == 0u) red[tid >> 6] = ss;
    __syncthreads();
    const float rs = rsqrtf((red[0] + red[1] + red[2] + red[3]) / (float)D + eps);
    uint4 *orow = reinterpret_cast<uint4 *>(out + (size_t)row * D);
    const uint4 *wr = reinterpret_cast<const uint4 *>(w);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const u32 u = tid + 256u * (u32)i;
        if (u >= nu) continue;
        const uint4 wv = wr[u];
        const u32 xx[4] = {v[i].x, v[i].y, v[i].z, v[i].w}, ww[4] = {wv.x, wv.y, wv.z, wv.w};
        u32 o[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            // (x.float() * rs).half(), then the fp16 product with the weight
            const h16 n0 = (h16)(h2f((uint16_t)(xx[e] & 0xFFFF)) * rs), n1 = (h16)(h2f((uint16_t)(xx[e] >> 16)) * rs);
            const h16 p0 = n0 * u2h((uint16_t)(ww[e] & 0xFFFF)), p1 = n1 * u2h((uint16_t)(ww[e] >> 16));
            o[e] = (u32)h2u(p0) | ((u32)h2u(p1) << 16);
        }
        orow[u] = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// apply_rotary_pos_emb on one thread's unit: a = elements d .. d + 7, b = elements d + HD / 2 .. of a head, at cache position p
__device__ __forceinline__ void rope_unit(const uint4 a, const uint4 b, const uint16_t *__restrict__ cos_t, const uint16_t *__restrict__ sin_t, u32 p,
                                          u32 max_seq, u32 HD, u32 d, u32 (&o1)[4], u32 (&o2)[4]) {
    const uint16_t *cr = cos_t + (size_t)min(p, max_seq - 1u) * HD, *sr = sin_t + (size_t)min(p, max_seq - 1u) * HD;
    const uint4 c1 = *reinterpret_cast<const uint4 *>(cr + d), c2 = *reinterpret_cast<const uint4 *>(cr + d + HD / 2u);
    const uint4 s1 = *reinterpret_cast<const uint4 *>(sr + d), s2 = *reinterpret_cast<const uint4 *>(sr + d + HD / 2u);
    const u32 x1[4] = {a.x, a.y, a.z, a.w}, x2[4] = {b.x, b.y, b.z, b.w};
    const u32 cc1[4] = {c1.x, c1.y, c1.z, c1.w}, cc2[4] = {c2.x, c2.y, c2.z, c2.w}, ss1[4] = {s1.x, s1.y, s1.z, s1.w}, ss2[4] = {s2.x, s2.y, s2.z, s2.w};
#pragma unroll
    for (int e = 0; e < 4; e++) {
        u32 r1 = 0, r2 = 0;
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const u32 sh = 16u * (u32)k;
            const h16 a1 = u2h((uint16_t)(x1[e] >> sh)), a2 = u2h((uint16_t)(x2[e] >> sh));
            // first half:  x1 * cos + (-x2) * sin ;  second half:  x2 * cos + x1 * sin   (rotate_half = cat(-x2, x1))
            const h16 f = (a1 * u2h((uint16_t)(cc1[e] >> sh))) + ((-a2) * u2h((uint16_t)(ss1[e] >> sh)));
            const h16 g = (a2 * u2h((uint16_t)(cc2[e] >> sh))) + (a1 * u2h((uint16_t)(ss2[e] >> sh)));
            r1 |= (u32)h2u(f) << sh;
            r2 |= (u32)h2u(g) << sh;
        }
        o1[e] = r1, o2[e] = r2;
    }
}

// 8 fp16 values (4 words) -> 8 OCP e4m3 codes by THE write rule of the fp8 cache, the only rounding the format adds:
//   code = fp8_rne(clamp(float(x16) * inv, -448, 448))
// inv = 1 / scale of the KV head, an fp32 the host computed (no division here).  The clamp is explicit (v_med3_f32): v_cvt_pk_fp8_f32
// turns a magnitude beyond 448 into NaN, not into 448; +-Inf clamps to +-448.  The host model:
// (x16.float() * inv).clamp(-448, 448).to(torch.float8_e4m3fn).  A NaN must be stored as a NaN code, and the clamp loses it (v_med3_f32
// with a NaN operand returns the smaller of the other two, -448): NAN_PASS puts the NaNs among the products v back behind the clamp.
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

// a thread's two units (elements d .. d + 7 and d + HD / 2 .. of a head's row `dst`): as they are into an fp16 row (q_out, an fp16
// cache), by fp8_quant8 with the reciprocal scale of the KV head into a row of one byte per element.  The fp8 row is stored by the clamp
// alone first; the test for a NaN -- a chain of fused multiply-adds through the 16 products, which a NaN survives, and one unordered
// compare -- runs behind the stores, off their path, and a thread that finds one stores its 16 bytes again with the NaNs in place (the
// same thread, the same addresses: in order).  A compare and a select per value in front of the store cost the S = 4096 launch 2 %.
template <typename E>
__device__ __forceinline__ void store_units(E *dst, u32 d, u32 HD, const u32 (&w1)[4], const u32 (&w2)[4], float inv) {
    if constexpr (sizeof(E) == 1) {
        float v1[8], v2[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            v1[k] = h2f((uint16_t)(w1[k >> 1] >> (16 * (k & 1)))) * inv;
            v2[k] = h2f((uint16_t)(w2[k >> 1] >> (16 * (k & 1)))) * inv;
        }
        *reinterpret_cast<uint2 *>(dst + d) = fp8_quant8<false>(v1);
        *reinterpret_cast<uint2 *>(dst + d + HD / 2u) = fp8_quant8<false>(v2);
        // a NaN among the 16 products makes t a NaN, or is v2[7] (Infs may do so too: the pass below is right for any input)
        float t = __builtin_fmaf(v1[0], v1[1], v1[2]);
        t = __builtin_fmaf(v1[3], v1[4], t);
        t = __builtin_fmaf(v1[5], v1[6], t);
        t = __builtin_fmaf(v1[7], v2[0], t);
        t = __builtin_fmaf(v2[1], v2[2], t);
        t = __builtin_fmaf(v2[3], v2[4], t);
        t = __builtin_fmaf(v2[5], v2[6], t);
        const bool nan = __builtin_isunordered(t, v2[7]);
        if (nan) {
            *reinterpret_cast<uint2 *>(dst + d) = fp8_quant8<true>(v1);
            *reinterpret_cast<uint2 *>(dst + d + HD / 2u) = fp8_quant8<true>(v2);
        }
    } else {
        *reinterpret_cast<uint4 *>(dst + d) = make_uint4(w1[0], w1[1], w1[2], w1[3]);
        *reinterpret_cast<uint4 *>(dst + d + HD / 2u) = make_uint4(w2[0], w2[1], w2[2], w2[3]);
    }
}

template <bool KV8>
struct CacheElem {
    typedef uint16_t type;
};
template <>
struct CacheElem<true> {
    typedef uint8_t type;
};

// THE row write of the prompt pass (and of the fp8 decode step, S = 1), one kernel for every layout:
//   qkv [S][(H + 2 Hkv) HD] -> q_out [H][S][HD] (rotated), k_cache / v_cache [Hkv][max_seq][HD] at pos[s] (k rotated).
// One thread per (token, head of q | k | v, 8 elements of the FIRST half): it owns elements d .. d + 7 and d + HD / 2 ..
// KV8: caches of one byte per element -- the same fp16 values up to the store (q_out is bit for bit what the fp16 form writes), k / v
//   stored by fp8_quant8 with the reciprocal scale of their KV head (k_inv / v_inv: read in this form only).
// QKN: Qwen3's per-head RMSNorm of q and k in front of the rotation (modeling_qwen3.Qwen3Attention.forward: q_norm / k_norm =
//   Qwen3RMSNorm over head_dim, weights [HD] shared by the heads): the HD / 16 threads of a (token, head) are neighbouring lanes of one
//   wave; each adds the squares of its 16 values in fp32, an xor butterfly over the group gives every lane the same sum, then
//   (x.float() * rsqrt(ssq / HD + eps)).half() * weight -- the rounding points of gq_rmsnorm_rows -- and the rotation.  v is not normed.
// QB: the bias of the q / k / v linears (fp16, laid out like a qkv row), ONE fp16 add in front of the rotation (decode.hip, AttnBias).
//   Only the fp8 decode step has it: the prompt pass's linears add the bias themselves, so no fp16 form is instantiated.
// PKD (gq_rope_cache_rows_packed: several sequences as one run of rows): the cache row is tail.row[s], apart from the RoPE position
//   pos[s] inside the row's own sequence.  Every other form has the empty tail and writes row pos[s].
// The loop bound is block-uniform in every form (QKN needs it: whole groups are active or idle together, total is a multiple of HD / 16).
template <bool PKD>
struct RowsTail {};
template <>
struct RowsTail<true> {
    const int *row;
};

template <bool QKN, bool QB, bool KV8, bool PKD = false>
__global__ void __launch_bounds__(256) rope_cache_rows_kernel(const uint16_t *__restrict__ qkv, const int *__restrict__ pos,
                                                              const uint16_t *__restrict__ cos_t, const uint16_t *__restrict__ sin_t,
                                                              uint16_t *__restrict__ q_out, typename CacheElem<KV8>::type *__restrict__ kc,
                                                              typename CacheElem<KV8>::type *__restrict__ vc, const float *__restrict__ k_inv,
                                                              const float *__restrict__ v_inv, const uint16_t *__restrict__ qnw,
                                                              const uint16_t *__restrict__ knw, float eps, const uint16_t *__restrict__ bias, u32 S,
                                                              u32 H, u32 Hkv, u32 HD, u32 max_seq, RowsTail<PKD> tail) {
    const u32 upr = HD / 16u, heads = H + 2u * Hkv, total = S * heads * upr;  // units of 8 in the first half
    for (u32 base = blockIdx.x * 256u; base < total; base += gridDim.x * 256u) {
        const u32 i = base + threadIdx.x;
        const bool active = i < total;
        const u32 ic = active ? i : 0u;
        const u32 u = ic % upr, hh = (ic / upr) % heads, s = ic / (upr * heads), d = 8u * u;
        const u32 p = (u32)pos[s];
        u32 cr = p;  // the cache row
        if constexpr (PKD) cr = (u32)tail.row[s];
        const uint16_t *src = qkv + (size_t)s * heads * HD + (size_t)hh * HD;
        uint4 a = *reinterpret_cast<const uint4 *>(src + d), b = *reinterpret_cast<const uint4 *>(src + d + HD / 2u);
        u32 x1[4] = {a.x, a.y, a.z, a.w}, x2[4] = {b.x, b.y, b.z, b.w};
        if constexpr (QB) {
            const uint16_t *br = bias + (size_t)hh * HD;
            const uint4 b1 = *reinterpret_cast<const uint4 *>(br + d), b2 = *reinterpret_cast<const uint4 *>(br + d + HD / 2u);
            const u32 bb1[4] = {b1.x, b1.y, b1.z, b1.w}, bb2[4] = {b2.x, b2.y, b2.z, b2.w};
#pragma unroll
            for (int e = 0; e < 4; e++) {
                u32 r1 = 0, r2 = 0;
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const u32 sh = 16u * (u32)k;
                    r1 |= (u32)h2u(u2h((uint16_t)(x1[e] >> sh)) + u2h((uint16_t)(bb1[e] >> sh))) << sh;
                    r2 |= (u32)h2u(u2h((uint16_t)(x2[e] >> sh)) + u2h((uint16_t)(bb2[e] >> sh))) << sh;
                }
                x1[e] = r1, x2[e] = r2;
            }
        }
        float ss = 0.f;
        if constexpr (QKN) {
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
            for (u32 sh = 1u; sh < upr; sh <<= 1) ss += __shfl_xor(ss, (int)sh, 64);  // (upr is wave-uniform: 4 or 8 lanes, aligned)
        }
        if (!active) continue;
        if (hh >= H + Hkv) {  // v: stored as it is
            if (cr < max_seq) {
                const u32 g = hh - H - Hkv;
                float inv = 0.f;
                if constexpr (KV8) inv = v_inv[g];
                store_units(vc + ((size_t)g * max_seq + cr) * HD, d, HD, x1, x2, inv);
            }
            continue;
        }
        if constexpr (QKN) {
            const float rs = rsqrtf(ss / (float)HD + eps);
            const uint16_t *wn = hh < H ? qnw : knw;
            const uint4 w1 = *reinterpret_cast<const uint4 *>(wn + d), w2 = *reinterpret_cast<const uint4 *>(wn + d + HD / 2u);
            const u32 ww1[4] = {w1.x, w1.y, w1.z, w1.w}, ww2[4] = {w2.x, w2.y, w2.z, w2.w};
#pragma unroll
            for (int e = 0; e < 4; e++) {
                u32 r1 = 0, r2 = 0;
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const u32 sh = 16u * (u32)k;
                    const h16 v1 = (h16)(h2f((uint16_t)(x1[e] >> sh)) * rs) * u2h((uint16_t)(ww1[e] >> sh));
                    const h16 v2 = (h16)(h2f((uint16_t)(x2[e] >> sh)) * rs) * u2h((uint16_t)(ww2[e] >> sh));
                    r1 |= (u32)h2u(v1) << sh;
                    r2 |= (u32)h2u(v2) << sh;
                }
                x1[e] = r1, x2[e] = r2;
            }
        }
        a = make_uint4(x1[0], x1[1], x1[2], x1[3]);
        b = make_uint4(x2[0], x2[1], x2[2], x2[3]);
        u32 o1[4], o2[4];
        rope_unit(a, b, cos_t, sin_t, p, max_seq, HD, d, o1, o2);
        if (hh < H) {
            store_units(q_out + ((size_t)hh * S + s) * HD, d, HD, o1, o2, 0.f);
        } else if (cr < max_seq) {
            const u32 g = hh - H;
            float inv = 0.f;
            if constexpr (KV8) inv = k_inv[g];
            store_units(kc + ((size_t)g * max_seq + cr) * HD, d, HD, o1, o2, inv);
        }
    }
}

// y [S][2 I] -> out [S][I]; paired: (gate_i, up_i) adjacent (the decode step's row order), else gate = y[:, :I], up = y[:, I:]
__global__ void __launch_bounds__(256) silu_mul_rows_kernel(const uint16_t *__restrict__ y, uint16_t *__restrict__ out, u32 S, u32 I, u32 paired) {
    const u32 upr = I / 8u, total = S * upr;
    for (u32 i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const u32 u = i % upr, s = i / upr;
        const uint16_t *row = y + (size_t)s * 2u * I;
        u32 gw[4], uw[4];
        if (paired) {
            const uint4 a = *reinterpret_cast<const uint4 *>(row + 16u * u), b = *reinterpret_cast<const uint4 *>(row + 16u * u + 8u);
            const u32 pw[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};  // word = gate | up << 16
#pragma unroll
            for (int e = 0; e < 4; e++) {
                gw[e] = (pw[2 * e] & 0xFFFFu) | (pw[2 * e + 1] << 16);
                uw[e] = (pw[2 * e] >> 16) | (pw[2 * e + 1] & 0xFFFF0000u);
            }
        } else {
            const uint4 a = *reinterpret_cast<const uint4 *>(row + 8u * u), b = *reinterpret_cast<const uint4 *>(row + I + 8u * u);
            gw[0] = a.x, gw[1] = a.y, gw[2] = a.z, gw[3] = a.w;
            uw[0] = b.x, uw[1] = b.y, uw[2] = b.z, uw[3] = b.w;
        }
        u32 o[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            u32 r = 0;
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const u32 sh = 16u * (u32)k;
                const float gf = h2f((uint16_t)(gw[e] >> sh));
                const h16 sl = (h16)(gf / (1.0f + expf(-gf)));  // F.silu on fp16: computed in fp32, rounded
                r |= (u32)h2u(sl * u2h((uint16_t)(uw[e] >> sh))) << sh;
            }
            o[e] = r;
        }
        *reinterpret_cast<uint4 *>(out + (size_t)s * I + 8u * u) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// what the three entries of the row write do not share behind their null checks: the head_dims served and the texts of the failures
// (literals: callers compare gq_last_error)
struct RowsEntry {
    bool any_hd16;  // every head_dim % 16 == 0 (no group of lanes adds a statistic), else 64 and 128
    const char *bad_hd, *unaligned, *too_large;
};

// the checks from `S == 0` on, the grid rule and the launch of rope_cache_rows_kernel<QKN, QB, KV8>: the norm form with norm weights,
// the bias form with a bias, the fp8 form with `kv8` (k_inv / v_inv are read by that form only)
int rope_cache_rows(const RowsEntry &e, bool kv8, const void *qkv, const int *pos, const void *cos_table, const void *sin_table, void *q_out, void *k_cache,
                    void *v_cache, const float *k_inv, const float *v_inv, u32 S, u32 n_head, u32 n_kv_head, u32 head_dim, u32 max_seq,
                    const void *q_norm_weight, const void *k_norm_weight, float eps, const void *qkv_bias, void *stream, const int *row = nullptr) {
    if (S == 0) return GQ_OK;
    // (QKN: the statistic of a head is added inside an aligned group of head_dim / 16 lanes: a power of two, within one wave)
    const bool hd_ok = e.any_hd16 ? (head_dim != 0 && head_dim % 16u == 0) : (head_dim == 64u || head_dim == 128u);
    if (!hd_ok || n_head == 0 || n_kv_head == 0 || max_seq == 0) return gq_fail(GQ_ENOTSUP, e.bad_hd);
    if (((uintptr_t)qkv | (uintptr_t)cos_table | (uintptr_t)sin_table | (uintptr_t)q_out | (uintptr_t)k_cache | (uintptr_t)v_cache |
         (uintptr_t)q_norm_weight | (uintptr_t)k_norm_weight | (uintptr_t)qkv_bias) & 15u)
        return gq_fail(GQ_EINVAL, e.unaligned);
    const uint64_t total = (uint64_t)S * (n_head + 2u * n_kv_head) * (head_dim / 16u);
    if (total >= 0x7FFFFFFFull) return gq_fail(GQ_ENOTSUP, e.too_large);
    const u32 nb = (u32)((total + 255u) / 256u);
    const dim3 grid(nb > 65535u ? 65535u : nb), block(256);
#define GQ_LAUNCH_ROWS(QKN_, QB_, KV8_, PKD_, TAIL_)                                                                                          \
    hipLaunchKernelGGL((rope_cache_rows_kernel<QKN_, QB_, KV8_, PKD_>), grid, block, 0, (hipStream_t)stream, (const uint16_t *)qkv, pos,      \
                       (const uint16_t *)cos_table, (const uint16_t *)sin_table, (uint16_t *)q_out, (CacheElem<KV8_>::type *)k_cache,         \
                       (CacheElem<KV8_>::type *)v_cache, k_inv, v_inv, (const uint16_t *)q_norm_weight, (const uint16_t *)k_norm_weight, eps, \
                       (const uint16_t *)qkv_bias, S, n_head, n_kv_head, head_dim, max_seq, TAIL_)
    const RowsTail<false> none = {};
    const RowsTail<true> rows = {row};
    if (row) {  // (the packed pass: fp16 caches)
        if (q_norm_weight) GQ_LAUNCH_ROWS(true, false, false, true, rows);
        else GQ_LAUNCH_ROWS(false, false, false, true, rows);
    } else if (kv8) {
        if (q_norm_weight) GQ_LAUNCH_ROWS(true, false, true, false, none);
        else if (qkv_bias) GQ_LAUNCH_ROWS(false, true, true, false, none);
        else GQ_LAUNCH_ROWS(false, false, true, false, none);
    } else if (q_norm_weight) {
        GQ_LAUNCH_ROWS(true, false, false, false, none);
    } else {
        GQ_LAUNCH_ROWS(false, false, false, false, none);
    }
#undef GQ_LAUNCH_ROWS
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}
}  // namespace

extern "C" int gq_rmsnorm_rows(void *x, const void *delta, const void *weight, void *out, uint32_t S, uint32_t D, float eps, void *stream) {
    if (!x || !weight || !out) return gq_fail(GQ_EINVAL, "null pointer argument.");
    if ((uintptr_t)delta & 15u) return gq_fail(GQ_EINVAL, "gq_rmsnorm_rows: 16-byte aligned pointers.");
    if (S == 0) return GQ_OK;
    if (D == 0 || D % 8u || D > 16384u) return gq_fail(GQ_ENOTSUP, "gq_rmsnorm_rows: D must be a multiple of 8, <= 16384.");
    if (((uintptr_t)x | (uintptr_t)weight | (uintptr_t)out) & 15u) return gq_fail(GQ_EINVAL, "gq_rmsnorm_rows: 16-byte aligned pointers.");
    hipLaunchKernelGGL(rmsnorm_rows_kernel, dim3(S), dim3(256), 0, (hipStream_t)stream, (uint16_t *)x, (const uint16_t *)delta, (const uint16_t *)weight, (uint16_t *)out, D, eps);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}

extern "C" int gq_rope_cache_rows(const void *qkv, const int *pos, const void *cos_table, const void *sin_table, void *q_out, void *k_cache,
                                  void *v_cache, uint32_t S, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq, void *stream) {
    if (!qkv || !pos || !cos_table || !sin_table || !q_out || !k_cache || !v_cache) return gq_fail(GQ_EINVAL, "null pointer argument.");
    static const RowsEntry e = {true, "gq_rope_cache_rows: head_dim must be a multiple of 16.", "gq_rope_cache_rows: 16-byte aligned pointers.",
                                "gq_rope_cache_rows: problem too large."};
    return rope_cache_rows(e, false, qkv, pos, cos_table, sin_table, q_out, k_cache, v_cache, nullptr, nullptr, S, n_head, n_kv_head, head_dim, max_seq,
                           nullptr, nullptr, 0.f, nullptr, stream);
}

extern "C" int gq_qknorm_rope_cache_rows(const void *qkv, const int *pos, const void *cos_table, const void *sin_table, void *q_out, void *k_cache,
                                         void *v_cache, uint32_t S, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq,
                                         const void *q_norm_weight, const void *k_norm_weight, float eps, void *stream) {
    if (!qkv || !pos || !cos_table || !sin_table || !q_out || !k_cache || !v_cache || !q_norm_weight || !k_norm_weight)
        return gq_fail(GQ_EINVAL, "null pointer argument.");
    static const RowsEntry e = {false, "gq_qknorm_rope_cache_rows: head_dim must be 64 or 128.", "gq_qknorm_rope_cache_rows: 16-byte aligned pointers.",
                                "gq_qknorm_rope_cache_rows: problem too large."};
    return rope_cache_rows(e, false, qkv, pos, cos_table, sin_table, q_out, k_cache, v_cache, nullptr, nullptr, S, n_head, n_kv_head, head_dim, max_seq,
                           q_norm_weight, k_norm_weight, eps, nullptr, stream);
}

extern "C" int gq_rope_cache_rows_kv8(const void *qkv, const int *pos, const void *cos_table, const void *sin_table, void *q_out, void *k_cache,
                                      void *v_cache, const float *k_inv, const float *v_inv, uint32_t S, uint32_t n_head, uint32_t n_kv_head,
                                      uint32_t head_dim, uint32_t max_seq, const void *q_norm_weight, const void *k_norm_weight, float eps,
                                      const void *qkv_bias, void *stream) {
    if (!qkv || !pos || !cos_table || !sin_table || !q_out || !k_cache || !v_cache || !k_inv || !v_inv) return gq_fail(GQ_EINVAL, "null pointer argument.");
    const bool qkn = q_norm_weight || k_norm_weight;
    if (qkn && (!q_norm_weight || !k_norm_weight)) return gq_fail(GQ_EINVAL, "gq_rope_cache_rows_kv8: both norm weights or none.");
    if (qkn && qkv_bias) return gq_fail(GQ_EINVAL, "gq_rope_cache_rows_kv8: the norm form and the bias form do not combine.");
    static const RowsEntry e = {false, "gq_rope_cache_rows_kv8: head_dim must be 64 or 128.", "gq_rope_cache_rows_kv8: 16-byte aligned pointers.",
                                "gq_rope_cache_rows_kv8: problem too large."};
    return rope_cache_rows(e, true, qkv, pos, cos_table, sin_table, q_out, k_cache, v_cache, k_inv, v_inv, S, n_head, n_kv_head, head_dim, max_seq, q_norm_weight,
                           k_norm_weight, eps, qkv_bias, stream);
}

extern "C" int gq_rope_cache_rows_packed(const void *qkv, const int *pos, const int *row, const void *cos_table, const void *sin_table, void *q_out,
                                         void *k_cache, void *v_cache, uint32_t S, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq,
                                         const void *q_norm_weight, const void *k_norm_weight, float eps, void *stream) {
    if (!qkv || !pos || !row || !cos_table || !sin_table || !q_out || !k_cache || !v_cache) return gq_fail(GQ_EINVAL, "null pointer argument.");
    const bool qkn = q_norm_weight || k_norm_weight;
    if (qkn && (!q_norm_weight || !k_norm_weight)) return gq_fail(GQ_EINVAL, "gq_rope_cache_rows_packed: both norm weights or none.");
    // (the head_dims of the entry each form restates: any multiple of 16 without the norm, 64 and 128 with it)
    static const RowsEntry plain = {true, "gq_rope_cache_rows_packed: head_dim must be a multiple of 16.", "gq_rope_cache_rows_packed: 16-byte aligned pointers.",
                                    "gq_rope_cache_rows_packed: problem too large."};
    static const RowsEntry norm = {false, "gq_rope_cache_rows_packed: head_dim must be 64 or 128 with the norm weights.",
                                   "gq_rope_cache_rows_packed: 16-byte aligned pointers.", "gq_rope_cache_rows_packed: problem too large."};
    return rope_cache_rows(qkn ? norm : plain, false, qkv, pos, cos_table, sin_table, q_out, k_cache, v_cache, nullptr, nullptr, S, n_head, n_kv_head, head_dim,
                           max_seq, q_norm_weight, k_norm_weight, eps, nullptr, stream, row);
}

extern "C" int gq_silu_mul_rows(const void *y, void *out, uint32_t S, uint32_t inter, int paired, void *stream) {
    if (!y || !out) return gq_fail(GQ_EINVAL, "null pointer argument.");
    if (S == 0) return GQ_OK;
    if (inter == 0 || inter % 8u) return gq_fail(GQ_ENOTSUP, "gq_silu_mul_rows: the intermediate size must be a multiple of 8.");
    if (((uintptr_t)y | (uintptr_t)out) & 15u) return gq_fail(GQ_EINVAL, "gq_silu_mul_rows: 16-byte aligned pointers.");
    const uint64_t total = (uint64_t)S * (inter / 8u);
    if (total >= 0x7FFFFFFFull) return gq_fail(GQ_ENOTSUP, "gq_silu_mul_rows: problem too large.");
    const u32 blocks = (u32)((total + 255u) / 256u);
    hipLaunchKernelGGL(silu_mul_rows_kernel, dim3(blocks > 65535u ? 65535u : blocks), dim3(256), 0, (hipStream_t)stream, (const uint16_t *)y, (uint16_t *)out, S,
                       inter, (u32)(paired != 0));
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}
