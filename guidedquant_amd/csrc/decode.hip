// decode.hip -- the non-quantized pieces of one bs=1 decode step, gfx950:
//   * token embedding lookup                      (inference/model.py:123 tok_embeddings)
//   * RoPE + KV-cache update + single-query attention  (inference/model.py:206-241, 336-341, 63-79)
//   * dense fp16 GEMV with optional RMSNorm prologue   (final norm + lm_head `output`, inference/model.py:93-94,128-129)
// All entry points read the token id / position from DEVICE memory so a captured hipGraph can be replayed for
// every token without re-recording.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gq_internal.h"
#include "attn_core.h"
#include "dense_stage.h"
#include "wave_util.h"
#include "fwht.h"
#include "qtip_xform.h"

namespace {

typedef uint32_t u32;
using gqw::h16;
using gqw::h16x2;
using gqw::h2f;
using gqw::h2u;
using gqw::u2h;
using gqw::u32x4;
using gqw::wave_reduce_bcast;
using gq_attn::AttnGeom;
using gq_attn::AttnWindow;
using gq_attn::window_lo;

// KV group of query head h: h / (H / Hkv).  Both divisions sit in front of the first load of an attention launch (the cache base
// needs g) -- ~25 scalar / vector instructions each on this chip (no integer divide); the group size is a power of two for every
// Llama (1, 4, 8): shifts then, the general quotient otherwise.  (Scalar: H, Hkv are kernel arguments, h is wave-uniform.)
__device__ __forceinline__ u32 kv_group_of(u32 h, u32 H, u32 Hkv) {
    if (H == Hkv) return h;
    if (H == 4u * Hkv) return h >> 2;
    if (H == 8u * Hkv) return h >> 3;
    if (H == 2u * Hkv) return h >> 1;
    return h / (H / Hkv);
}

// ------------------------------------------------------------------------------------------------ embedding
__global__ void embed_kernel(const int *tok, const uint16_t *table, uint16_t *out, u32 D, u32 V) {
    u32 t = (u32)tok[0];
    if (t >= V) t = 0;
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < D / 8u; i += gridDim.x * blockDim.x)
        reinterpret_cast<uint4 *>(out)[i] = reinterpret_cast<const uint4 *>(table + (size_t)t * D)[i];
}

// the same with the statistics hand-over for the RMSNorm prologue of layer 0's first launch (include/gq_hip.h, GQ_SSQ_SLOTS): one
// block, thread t leaves the sum of squares of the 16-byte units it copied in slot t
__global__ void __launch_bounds__(GQ_SSQ_SLOTS) embed_ssq_kernel(const int *tok, const uint16_t *table, uint16_t *out, u32 D, u32 V, float *ssq) {
    u32 t = (u32)tok[0];
    if (t >= V) t = 0;
    float acc = 0.f;
    for (u32 i = threadIdx.x; i < D / 8u; i += (u32)GQ_SSQ_SLOTS) {
        const uint4 v = reinterpret_cast<const uint4 *>(table + (size_t)t * D)[i];
        gq_store_wt(reinterpret_cast<uint4 *>(out) + i, v);
        const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float a = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[k] & 0xFFFFu)), b = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[k] >> 16));
            acc += a * a;
            acc += b * b;
        }
    }
    gq_store_wt(ssq + threadIdx.x, acc);
}

// ------------------------------------------------------------------------------------------------ attention
// One block per query head.  RoPE exactly as apply_rotary_pos_emb on fp16 tensors (inference/model.py:336-341):
//   q_embed = (q * cos) + (rotate_half(q) * sin)   -- three fp16-rounded operations, cos/sin are fp16 tables
// built by the host from fp32 (LlamaRotaryEmbedding.forward, model.py:379-405).  The rotated k and the v of this
// token are written to the cache at `pos` (KVCache.update, model.py:69-79) by the first head of each KV group.
// Scores / softmax / weighted sum run in fp32 from the fp16 operands; the output is rounded to fp16 once.  The split geometry, the
// arithmetic of a cached row and of the online softmax, and the LDS layout are those of attn_core.h.
constexpr int ATTN_WAVES = GQ_ATTN_WAVES;
// QT (QTIP models): q / k / v are not read as fp16 vectors but rebuilt from the trellis matvecs' fp32 sums -- the transform-out of
// BitshiftLinear.forward (inference/lib/codebook/bitshift.py:470: hadamard(y) * m^-1/2 * (SV * 32) -> fp16), i.e. what
// gq_qtip_linear_out computes in a launch of its own.  A head needs HD of the M outputs of each vector and the Sylvester matrix
// factors, H_M = H_(M / HD) (x) H_HD: combine the M / HD segments with the signs of the head's row first, then ONE HD-point
// transform.  (Keeping the order of the full transform -- segment-local stages of ALL segments first, then a tree over the
// segments: bit-identical -- was built and measured: every head block repeats 7/12 of the whole vector's butterflies with half
// the threads gq_qtip_linear_out has per vector, 366 vs 385 tokens/s.)
struct AttnQt {
    const float *y32[3], *sv32[3];  // q, k, v: sums [parts][M] and SV * 32 [M]
    u32 M[3], parts[3];
    float mscale[3];                // (float)M^-1/2
};
// QKN (Qwen3: modeling_qwen3.Qwen3Attention.forward, q_norm / k_norm = Qwen3RMSNorm over head_dim in front of the rotation): the block
// normalises its q head and its KV group's k head before it rotates them -- sum of squares of the HD fp16 values in fp32 (one wave at
// HD = 64, two waves added in wave order at HD = 128), x * rsqrt(ssq / HD + eps) rounded to fp16, then the fp16 product with the
// weight: Qwen3RMSNorm's rounding points (= RMSNorm.forward of model.py).  v is untouched.  Every split block normalises q; the
// block that owns the current position writes the normalised, rotated k.  A compile-time form: the QKN = false instances take
// an empty argument behind the old ones and keep the instructions they had.
template <bool QKN>
struct AttnQkNorm {};  // (nothing to pass: the instances without the norm keep their arguments)
template <>
struct AttnQkNorm<true> {
    const uint16_t *qw, *kw;  // q_norm / k_norm weights, fp16 [HD]
    float eps;
};
// QB (Qwen2 / Qwen2.5: modeling_qwen2.Qwen2Attention, q_proj / k_proj / v_proj = nn.Linear(bias=True); the quantized linears add the
// bias as ONE fp16 add behind the fp16-rounded GEMV result, any_precision/modules/AnyPrecisionLinear.py `output += bias`): thread
// d < HD adds the bias of its q / k / v element (and of the rotation partners) in fp16 right behind the loads, in front of the
// rotation -- bit for bit what the module forward rotates and caches.  The bias is laid out like the packed q | k | v vector; its loads
// go out with the q / k / v loads, in front of the position read.  A compile-time form like QKN: the QB = false instances take an
// empty argument and keep the instructions they had.
template <bool QB>
struct AttnBias {};  // (nothing to pass)
template <>
struct AttnBias<true> {
    const uint16_t *qkv;  // fp16 [(H + 2 Hkv) * HD]
};
// WIN: the sliding-window form (attn_core.h, AttnWindow).
template <int HD, bool QT, bool QKN = false, bool QB = false, bool WIN = false>
__global__ void __launch_bounds__(64 * ATTN_WAVES) attn_decode_kernel(const uint16_t *qkv, const int *pos_ptr, const uint16_t *cos_t,
                                                          const uint16_t *sin_t, uint16_t *kc, uint16_t *vc, uint16_t *out,
                                                          u32 H, u32 Hkv, u32 max_seq, float scale, u32 nsplit, float *ws, AttnQt qt,
                                                          AttnQkNorm<QKN> nm, AttnBias<QB> bs, AttnWindow<WIN> wn) {
    static_assert(!(QB && (QT || QKN)), "the bias form is the plain fp16 q / k / v form plus the add");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using Geo = AttnGeom<HD>;
    using L = gq_attn::DecodeLds<HD>;
    constexpr u32 NW = Geo::NW, NS = Geo::NS;
    constexpr int LPP = Geo::LPP, PPW = Geo::PPW, U = Geo::U;
    float *lds = reinterpret_cast<float *>(smem);
    float *sc = lds + L::sc, *qs = lds + L::qs, *kcur = lds + L::kcur, *vcur = lds + L::vcur, *red = lds + L::red, *red2 = lds + L::red2;
    const u32 tid = threadIdx.x, w = tid >> 6, l = tid & 63u;
    const u32 h = blockIdx.x, g = kv_group_of(h, H, Hkv);
    const uint16_t *q = qkv + (size_t)h * HD;
    const uint16_t *k = qkv + (size_t)H * HD + (size_t)g * HD;
    const uint16_t *v = qkv + (size_t)(H + Hkv) * HD + (size_t)g * HD;
    if constexpr (QT) {
        float *tv = lds + L::tv;
        uint16_t *res16 = reinterpret_cast<uint16_t *>(lds + L::res16);
        // H_M = H_(M / HD) (x) H_HD: the HD outputs of segment `seg` are the HD-point transform of  z[b] = sum_c s(c) y[c HD + b],
        // s(c) = (-1)^popcount(c & seg)  (row `seg` of the M / HD-point Sylvester matrix): 4096 signed additions and ONE short
        // transform instead of the whole vector's butterflies.  The additions are those of the full transform in another order
        // (segments first): the result equals gq_qtip_linear_out's up to fp32 rounding, not bit for bit.
        // every thread takes 16-byte units of the three vectors (all loads of a thread in flight together: one round trip to L2):
        // unit u of a vector = segment c = u / (HD / 4), elements 4 (u % (HD / 4)) ..; a thread's units of one vector share the
        // element group (T is a multiple of HD / 4), so it keeps one signed partial sum per vector; the T / (HD / 4) partial sums
        // of an element are added in a fixed order behind the barrier.  gqq::seg_load / seg_signed_sum (qtip_xform.h), written out: as calls
        // the kernel's scalar loads of `qt` come out in another order
        {
            constexpr u32 Q = HD / 4u;
            const u32 T = blockDim.x, G = T / Q;  // G thread groups per element group
            float *ps = lds + L::ps;  // [3][G][HD] partial sums
            float4 y[3][4];
#pragma unroll
            for (u32 vi = 0; vi < 3; vi++) {
                const u32 M4 = qt.M[vi] / 4u;
#pragma unroll
                for (u32 k = 0; k < 4; k++) {
                    const u32 u = tid + k * T;
                    y[vi][k] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (u < M4) {
                        float4 t = reinterpret_cast<const float4 *>(qt.y32[vi])[u];
                        for (u32 p = 1; p < qt.parts[vi]; p++) {  // split-K parts, ascending
                            const float4 t2 = reinterpret_cast<const float4 *>(qt.y32[vi])[(size_t)p * M4 + u];
                            t = make_float4(t.x + t2.x, t.y + t2.y, t.z + t2.z, t.w + t2.w);
                        }
                        y[vi][k] = t;
                    }
                }
            }
#pragma unroll
            for (u32 vi = 0; vi < 3; vi++) {
                const u32 seg = vi == 0u ? h : g;
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (u32 k = 0; k < 4; k++) {
                    const u32 c = (tid + k * T) / Q;
                    const float sg = (__builtin_popcount(c & seg) & 1) ? -1.f : 1.f;  // (units past the vector hold zeros)
                    acc = make_float4(acc.x + sg * y[vi][k].x, acc.y + sg * y[vi][k].y, acc.z + sg * y[vi][k].z, acc.w + sg * y[vi][k].w);
                }
                reinterpret_cast<float4 *>(ps + ((size_t)vi * G + tid / Q) * HD)[tid % Q] = acc;
            }
            __syncthreads();
            if (tid < 3u * HD) {
                const u32 vi = tid / HD, b = tid % HD;
                float z = 0.f;
                for (u32 gi = 0; gi < G; gi++) z += ps[((size_t)vi * G + gi) * HD + b];
                tv[tid] = z;
            }
        }
        __syncthreads();
        gq_fwht::fwht_lds(tv, 3u * HD, (u32)HD);  // the three HD-point transforms (barrier behind)
        if (tid < 3u * HD) {
            const u32 vi = tid / HD, b = tid % HD, seg = vi == 0u ? h : g;
            res16[tid] = h2u(gqq::xf_out(tv[tid], qt.mscale[vi], qt.sv32[vi][(size_t)seg * HD + b]));
        }
        __syncthreads();
        q = res16, k = res16 + HD, v = res16 + 2 * HD;
    }
    // q / k / v do not depend on the position: their loads are issued before the position is read, so the two
    // dependent round trips (position -> cos / sin rows) overlap with them
    uint16_t qd_b = 0, kd_b = 0, qr_b = 0, kr_b = 0, vd_b = 0;
    if (tid < HD) {
        const u32 d = tid, dr = d < HD / 2 ? d + HD / 2 : d - HD / 2;
        qd_b = q[d];
        kd_b = k[d];
        qr_b = q[dr];
        kr_b = k[dr];
        vd_b = v[d];
        if constexpr (QB) {
            // (the same offsets into the bias as into the packed vector; all ten loads in flight together)
            const uint16_t *bq = bs.qkv + (q - qkv), *bk = bs.qkv + (k - qkv), *bv = bs.qkv + (v - qkv);
            const uint16_t bqd = bq[d], bkd = bk[d], bqr = bq[dr], bkr = bk[dr], bvd = bv[d];
            qd_b = h2u(u2h(qd_b) + u2h(bqd));
            kd_b = h2u(u2h(kd_b) + u2h(bkd));
            qr_b = h2u(u2h(qr_b) + u2h(bqr));
            kr_b = h2u(u2h(kr_b) + u2h(bkr));
            vd_b = h2u(u2h(vd_b) + u2h(bvd));
        }
    }
    u32 pos = (u32)pos_ptr[0];
    if (pos >= max_seq) {  // decoding past the cache: nothing is written to it, the head's output is poisoned (NaN logits)
        if (blockIdx.y == 0 && tid < HD) out[(size_t)h * HD + tid] = 0x7e00u;
        return;
    }
    uint16_t *kcg = kc + (size_t)g * max_seq * HD;
    uint16_t *vcg = vc + (size_t)g * max_seq * HD;
    // the rows [p0, p1) of this block (attn_core.h: the solo rule, the rows of a split)
    const u32 sp = blockIdx.y;
    const u32 lo = window_lo(pos, wn), n = pos + 1u - lo;  // (WIN = false: lo = 0, n = pos + 1)
    if (gq_attn::attn_solo<HD>(n, nsplit)) {
        if (sp > 0u) return;
        nsplit = 1u;
    }
    const u32 per = gq_attn::attn_per<HD>(n, nsplit);
    const u32 p0 = lo + sp * per, p1 = min(pos + 1u, p0 + per);
    const bool has_cur = p0 <= pos && pos < p1;  // the split that covers the current token
    if constexpr (QKN) {
        // per-head statistics: thread d < HD holds element d of q and of k (the other waves add zeros); fixed order
        const float qf = h2f(qd_b), kf = h2f(kd_b);  // (0 for tid >= HD)
        float sq = wave_reduce_bcast<false>(qf * qf), sk = wave_reduce_bcast<false>(kf * kf);
        if constexpr (HD > 64) {
            if (l == 0u && w < (u32)(HD / 64)) red[w] = sq, red[HD / 64 + w] = sk;
            __syncthreads();  // (block-uniform: behind the position checks above)
            sq = 0.f, sk = 0.f;
#pragma unroll
            for (int i = 0; i < HD / 64; i++) sq += red[i], sk += red[HD / 64 + i];
        }
        const float rq = rsqrtf(sq / (float)HD + nm.eps), rk = rsqrtf(sk / (float)HD + nm.eps);
        if (tid < HD) {
            const u32 d = tid, dr = d < HD / 2 ? d + HD / 2 : d - HD / 2;
            // (x.float() * rsqrt(..)).half() * weight -- for the element and for its rotation partner
            qd_b = h2u((h16)(qf * rq) * u2h(nm.qw[d]));
            kd_b = h2u((h16)(kf * rk) * u2h(nm.kw[d]));
            qr_b = h2u((h16)(h2f(qr_b) * rq) * u2h(nm.qw[dr]));
            kr_b = h2u((h16)(h2f(kr_b) * rk) * u2h(nm.kw[dr]));
        }
    }
    if (tid < HD) {
        const u32 d = tid;
        const h16 c = u2h(cos_t[(size_t)pos * HD + d]), s = u2h(sin_t[(size_t)pos * HD + d]);
        const h16 qd = u2h(qd_b), kd = u2h(kd_b);
        const h16 qr = d < HD / 2 ? -u2h(qr_b) : u2h(qr_b);
        const h16 kr = d < HD / 2 ? -u2h(kr_b) : u2h(kr_b);
        const h16 qe = (h16)(qd * c) + (h16)(qr * s);
        const h16 ke = (h16)(kd * c) + (h16)(kr * s);
        qs[d] = (float)qe;
        kcur[d] = (float)ke;
        vcur[d] = h2f(vd_b);
        if (h == g * (H / Hkv) && has_cur) {  // (the first head of its KV group; off the critical path)
            kcg[(size_t)pos * HD + d] = h2u(ke);
            vcg[(size_t)pos * HD + d] = vd_b;
        }
    }
    __syncthreads();
    // One pass, online softmax per position stream (attn_core.h).  The K and the V rows of a batch are requested together (one memory
    // round trip instead of two); the NS streams of the block are combined once, through LDS.
    const u32 sub = l / LPP, ld = l % LPP;
    float qreg[8];
#pragma unroll
    for (int e = 0; e < 8; e++) qreg[e] = qs[ld * 8 + e];
    float m_run = -3.0e38f, s_run = 0.f, acc[8];
#pragma unroll
    for (int e = 0; e < 8; e++) acc[e] = 0.f;
    for (u32 t0 = p0 + w * PPW * U; t0 < p1; t0 += NW * PPW * U) {
        uint4 kv[U], vv[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const u32 t = t0 + (u32)u * PPW + sub;
            const bool cached = t < pos && t < p1;
            kv[u] = cached ? *reinterpret_cast<const uint4 *>(kcg + (size_t)t * HD + ld * 8) : make_uint4(0, 0, 0, 0);
            vv[u] = cached ? *reinterpret_cast<const uint4 *>(vcg + (size_t)t * HD + ld * 8) : make_uint4(0, 0, 0, 0);
        }
        float pu[U], vfu[U][8];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const u32 t = t0 + (u32)u * PPW + sub;
            const u32 kw[4] = {kv[u].x, kv[u].y, kv[u].z, kv[u].w}, vw[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
            float p = 0.f;
            if (t == pos) {  // (the current token: staged in LDS above, its cache row may not have landed)
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    p += qreg[e] * kcur[ld * 8 + e];
                    vfu[u][e] = vcur[ld * 8 + e];
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    p += qreg[2 * e] * h2f((uint16_t)(kw[e] & 0xFFFF));
                    p += qreg[2 * e + 1] * h2f((uint16_t)(kw[e] >> 16));
                    vfu[u][2 * e] = h2f((uint16_t)(vw[e] & 0xFFFF));
                    vfu[u][2 * e + 1] = h2f((uint16_t)(vw[e] >> 16));
                }
            }
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
    // (not attn_core.h's merge: one exponential per thread and stream over all NS streams -- another instruction sequence, kept for its speed)
    if (tid < HD) {
        float M = -3.0e38f;
#pragma unroll
        for (u32 i = 0; i < NS; i++) M = fmaxf(M, sc[i]);
        float o = 0.f, sum = 0.f;
#pragma unroll
        for (u32 i = 0; i < NS; i++) {
            const float f = __expf(sc[i] - M);  // streams without a position: exp(-3e38 - M) = 0
            sum += sc[NS + i] * f;
            o += red2[i * HD + tid] * f;
        }
        if (nsplit > 1u) {  // partial result of this split: weighted sum and sum relative to its own maximum M
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

// ------------------------------------------------------------------------------------------------ attention, q / k rotated upstream
// Round 4: the wqkv GEMV of the decode step applies RoPE in its epilogue and writes k / v of the current token straight into the
// caches (ap_stream.hip, gq_anyprec_gemv_qkv_rope), so this launch starts at q k^T: no cos / sin round trip behind the position, no
// rotation, no LDS staging of the current token, no barrier in front of the position streams.  And the first batch of cached rows
// does not wait for the position either: the rows [0, PASS) are requested together with q and the position (one memory round trip
// instead of two); which of them are valid (t <= pos) is decided when they have landed.  Rows past the position hold whatever
// an earlier sequence left (finite or not): their scores are replaced and their V rows zeroed before use.
// The arithmetic is attn_core.h's, shared with attn_decode_kernel (fp32 scores / softmax / weighted sum from fp16 operands, one fp16 rounding).
#ifndef GQ_ATTN_SPEC
#define GQ_ATTN_SPEC 32  // cached rows requested before the position is known (a multiple of 16)
#endif
// QH = 1: one query head per block (grid n_head x n_split).  QH > 1 (grouped-query models, long caches): the QH query heads of a
// KV group share a block (grid n_head / QH x n_split), every cached row is loaded ONCE and multiplied with all of them -- at
// 4096 positions the per-head form reads each K / V row four times and waits a full memory round trip per 128-position pass
// (19 us per layer on Llama-3-8B); here the next pass is requested before the current one is multiplied.  Per head the
// arithmetic, the position -> stream assignment and the merge order are those of the QH = 1 form: bit-identical outputs.
// A short context (the `solo` rule) is finished by ONE block per head: block (hq, sp < QH) takes head hq * QH + sp alone.
// WIN: the window form (attn_core.h, AttnWindow).  The rows requested ahead of the position are usable only when lo == 0; with lo > 0 they
// are dropped (p0 >= lo > 0 below) and the first batch is requested once lo is known.
// KV8: the caches hold OCP e4m3 codes (gq_attn_decode_roped_kv8): a row is one 8-byte load per lane and unpack8_fp8, the K scale of the
// head's KV group is folded into the score factor, the V scale multiplies the merged weighted sum (the final one in front of the
// division, a split's partial one in front of the workspace, so that attn_combine_kernel serves as it is).  Everything else is shared.
template <int HD, int QH, bool WIN = false, bool KV8 = false>
__global__ void __launch_bounds__(64 * ATTN_WAVES) attn_roped_kernel(const uint16_t *q, const int *pos_ptr, const typename gq_attn::CacheFmt<KV8>::elem *kc,
                                                                     const typename gq_attn::CacheFmt<KV8>::elem *vc, uint16_t *out, u32 H, u32 Hkv,
                                                                     u32 max_seq, float scale, u32 nsplit, float *ws, AttnWindow<WIN> wn,
                                                                     gq_attn::AttnKv8<KV8> k8) {
    using Fmt = gq_attn::CacheFmt<KV8>;
    using Row = typename Fmt::row;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using Geo = AttnGeom<HD>;
    using L = gq_attn::RopedLds<HD, QH>;
    constexpr u32 NW = Geo::NW, NS = Geo::NS;
    constexpr int LPP = Geo::LPP, PPW = Geo::PPW, U = Geo::U;
    // (the merge and the NaN poisoning below index the block's QH * HD outputs by thread id: a build with fewer waves would silently
    // leave the upper heads of a group unwritten)
    static_assert(64 * ATTN_WAVES >= QH * HD, "attn_roped_kernel: the block must have a thread per output of its QH heads (GQ_ATTN_WAVES)");
    float *lds = reinterpret_cast<float *>(smem);
    float *sc = lds + L::sc, *red2 = lds + L::red2;
    const u32 tid = threadIdx.x, w = tid >> 6, l = tid & 63u;
#ifdef GQ_ATTN_PROBE  // timing probe (tools/r5): blockIdx.y = identical copies of the whole-group form, every copy writes the same outputs
    const u32 h0 = blockIdx.x * QH, g = kv_group_of(h0, H, Hkv), sp = 0u;
#else
    const u32 h0 = blockIdx.x * QH, g = kv_group_of(h0, H, Hkv), sp = blockIdx.y;
#endif
    const u32 sub = l / LPP, ld = l % LPP;
    const typename Fmt::elem *kcg = kc + (size_t)g * max_seq * HD, *vcg = vc + (size_t)g * max_seq * HD;
    // requests that do not depend on the position: q, and (blocks that may start at row 0) the first batch of cached rows
    uint4 q4[QH];
#pragma unroll
    for (int qh = 0; qh < QH; qh++) q4[qh] = *reinterpret_cast<const uint4 *>(q + (size_t)(h0 + qh) * HD + ld * 8);
    Row kv[U], vv[U];
    u32 t0 = w * PPW * U;
#pragma unroll
    for (int u = 0; u < U; u++) {
        const u32 t = t0 + (u32)u * PPW + sub;
        // (only the first GQ_ATTN_SPEC rows: every row requested ahead of the position is HBM traffic whether it is needed or not --
        // 128 rows x 32 heads = 2 MiB per layer, which costs what the saved round trip gains)
        const bool in = sp < (u32)QH && t < max_seq && t < (u32)GQ_ATTN_SPEC;
        kv[u] = in ? *reinterpret_cast<const Row *>(kcg + (size_t)t * HD + ld * 8) : Fmt::zero();
        vv[u] = in ? *reinterpret_cast<const Row *>(vcg + (size_t)t * HD + ld * 8) : Fmt::zero();
    }
    if constexpr (KV8) scale *= k8.k_scale[g];  // (block-uniform: one scalar load next to the position's)
    const u32 pos = (u32)pos_ptr[0];
    if (pos >= max_seq) {  // decoding past the cache: the head's output is poisoned (NaN logits), like attn_decode_kernel
        if (sp == 0u && tid < (u32)QH * HD) out[(size_t)h0 * HD + tid] = 0x7e00u;
        return;
    }
    const u32 lo = window_lo(pos, wn), n = pos + 1u - lo;  // (WIN = false: lo = 0, n = pos + 1)
    const bool solo = gq_attn::attn_solo<HD>(n, nsplit);
    u32 nh = QH, hb = h0;  // heads of this block: [hb, hb + nh)
    if (solo) {  // (every block sp < QH finishes a head)
        if (sp >= (u32)QH) return;
        if (QH > 1) nh = 1u, hb = h0 + sp;
        nsplit = 1u;
    }
    const u32 spx = solo ? 0u : sp;
    const u32 per = gq_attn::attn_per<HD>(n, nsplit);
    const u32 p0 = lo + spx * per, p1 = min(pos + 1u, p0 + per);
    float qreg[QH][8];
#pragma unroll
    for (int qh = 0; qh < QH; qh++) {
        uint4 qq = q4[qh];
        if (QH > 1 && solo) {  // (the one head of this block: q of head h0 + sp)
#pragma unroll
            for (int j = 1; j < QH; j++)
                if (sp == (u32)j) qq = q4[j];
        }
        gq_attn::unpack8(qq, qreg[qh]);
    }
    float m_run[QH], s_run[QH], acc[QH][8];
#pragma unroll
    for (int qh = 0; qh < QH; qh++) {
        m_run[qh] = -3.0e38f, s_run[qh] = 0.f;
#pragma unroll
        for (int e = 0; e < 8; e++) acc[qh][e] = 0.f;
    }
    auto request = [&](Row (&kd)[U], Row (&vd)[U], u32 tb) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const u32 t = tb + (u32)u * PPW + sub;
            const bool in = t < p1;
            kd[u] = in ? *reinterpret_cast<const Row *>(kcg + (size_t)t * HD + ld * 8) : Fmt::zero();
            vd[u] = in ? *reinterpret_cast<const Row *>(vcg + (size_t)t * HD + ld * 8) : Fmt::zero();
        }
    };
    t0 = p0 + w * PPW * U;
    const bool have = p0 == 0u && t0 + PPW * U <= (u32)GQ_ATTN_SPEC;  // the batch at t0 is already in registers
    if (!have && t0 < p1) request(kv, vv, t0);
    for (; t0 < p1; t0 += NW * PPW * U) {
        Row kn[U], vn[U];
        const bool more = QH > 1 && t0 + NW * PPW * U < p1;  // (QH > 1: the next pass is on its way while this one is multiplied)
        if (more) request(kn, vn, t0 + NW * PPW * U);
        float pu[QH][U], vfu[U][8];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const u32 t = t0 + (u32)u * PPW + sub;
            const bool valid = t < p1;
            float kf[8];
            Fmt::unpack(kv[u], kf);
            if constexpr (KV8) {
                float vf[8];
                Fmt::unpack(vv[u], vf);
#pragma unroll
                for (int e = 0; e < 8; e++) vfu[u][e] = valid ? vf[e] : 0.f;
            } else {
                const u32 vw[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    vfu[u][2 * e] = valid ? h2f((uint16_t)(vw[e] & 0xFFFF)) : 0.f;
                    vfu[u][2 * e + 1] = valid ? h2f((uint16_t)(vw[e] >> 16)) : 0.f;
                }
            }
#pragma unroll
            for (int qh = 0; qh < QH; qh++) {
                if (QH > 1 && (u32)qh >= nh) continue;
                float p = 0.f;
#pragma unroll
                for (int e = 0; e < 8; e++) p += qreg[qh][e] * kf[e];
                p = gq_attn::row_sum<LPP>(p);
                pu[qh][u] = valid ? p * scale : -3.0e38f;  // (a stale row past the position may have produced anything, NaN included)
            }
        }
#pragma unroll
        for (int qh = 0; qh < QH; qh++) {
            if (QH > 1 && (u32)qh >= nh) continue;  // (wave-uniform: a solo block multiplies one head)
            gq_attn::softmax_update<U>(m_run[qh], s_run[qh], acc[qh], pu[qh], vfu);
        }
        if (QH > 1) {
#pragma unroll
            for (int u = 0; u < U; u++) kv[u] = kn[u], vv[u] = vn[u];
        } else if (t0 + NW * PPW * U < p1) {
            request(kv, vv, t0 + NW * PPW * U);
        }
    }
    const u32 stream = w * PPW + sub;
#pragma unroll
    for (int qh = 0; qh < QH; qh++) {
        if (QH > 1 && (u32)qh >= nh) continue;
#pragma unroll
        for (int e = 0; e < 8; e++) red2[((size_t)qh * NS + stream) * HD + ld * 8 + e] = acc[qh][e];
        if (ld == 0) {
            sc[qh * 2u * NS + stream] = m_run[qh];
            sc[qh * 2u * NS + NS + stream] = s_run[qh];
        }
    }
    __syncthreads();
    // the merge of attn_core.h (spelled out here and in ap_stream.hip::fuse_attn_head): the factors and the maximum of a head to fl ..
    float *fl = lds + L::fl;  // [QH][NS] factors, [QH] maxima behind them
    const u32 ng = gq_attn::merge_groups<HD>(p1 - p0);
    if (tid < nh * NS) {
        const u32 qh = tid / NS, i = tid % NS;
        const float *scq = sc + qh * 2u * NS;
        float M = -3.0e38f;
        for (u32 g8 = 0; g8 < ng; g8++)
#pragma unroll
            for (u32 k = 0; k < 8u; k++) M = fmaxf(M, scq[8u * g8 + k]);
        fl[qh * NS + i] = __expf(scq[i] - M);
        if (i == 0u) fl[(u32)QH * NS + qh] = M;
    }
    __syncthreads();
    if (tid < nh * HD) {  // .. then thread (head, dim): the streams of the head merged in ascending order
        const u32 qh = tid / HD, dd = tid % HD, h = hb + qh;
        const float *scq = sc + qh * 2u * NS, *rq = red2 + (size_t)qh * NS * HD, *fq = fl + qh * NS;
        const float M = fl[(u32)QH * NS + qh];
        float o = 0.f, sum = 0.f;
        for (u32 g8 = 0; g8 < ng; g8++)
#pragma unroll
            for (u32 k = 0; k < 8u; k++) gq_attn::merge_step<HD>(scq, rq, fq, 8u * g8 + k, dd, o, sum);
        if constexpr (KV8) o *= k8.v_scale[g];
        if (nsplit > 1u) {
            float *wp = ws + ((size_t)h * nsplit + sp) * (HD + 2u);
            wp[dd] = o;
            if (dd == 0) {
                wp[HD] = M;
                wp[HD + 1] = sum;
            }
        } else {
            out[(size_t)h * HD + dd] = h2u((h16)(o / sum));
        }
    }
}

// split-KV combine: out[h] = sum_s o_s e^(M_s - M) / sum_s l_s e^(M_s - M)
template <int HD, bool WIN = false>
__global__ void __launch_bounds__(HD) attn_combine_kernel(const float *ws, uint16_t *out, u32 nsplit, const int *pos_ptr, u32 max_seq, AttnWindow<WIN> wn) {
    const u32 h = blockIdx.x, tid = threadIdx.x;
    {   // (a short context was finished by the blocks of split 0)
        const u32 pos = (u32)pos_ptr[0];  // (the solo rule: n_split > 1 here; two spellings that keep each instance's instructions)
        if constexpr (WIN) {
            if (pos >= max_seq || gq_attn::attn_short<HD>(pos + 1u - window_lo(pos, wn))) return;
        } else {
            const bool done = gq_attn::attn_short<HD>(pos + 1u);
            if (pos >= max_seq || done) return;
        }
    }
    const float *wp = ws + (size_t)h * nsplit * (HD + 2u);
    // Every load of this kernel reads what another CU has just written (an L2 miss each): a loop with one dependent load per split
    // costs n_split memory round trips (measured: 19 -> 45 us per layer from 8 to 64 splits).  Lane s of every wave takes (M_s, l_s)
    // in one round trip, the partial outputs come 8 splits per round trip; the sums keep the ascending split order.
    const u32 l = tid & 63u;
    const float Ms = l < nsplit ? wp[l * (HD + 2u) + HD] : -3.0e38f;  // (n_split <= 64; empty splits: M_s = -3e38, l_s = 0, o_s = 0)
    const float ls = l < nsplit ? wp[l * (HD + 2u) + HD + 1] : 0.f;
    // (the partial outputs of the first 32 splits are requested in the same round trip as the scalars)
    float ov[32];
#pragma unroll
    for (u32 k = 0; k < 32; k++) ov[k] = k < nsplit ? wp[k * (HD + 2u) + tid] : 0.f;
    float M = Ms;
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) M = fmaxf(M, __shfl_xor(M, sh, 64));
    const float fs = __expf(Ms - M);
    float o = 0.f, sum = 0.f;
#pragma unroll
    for (u32 k = 0; k < 32; k++)
        if (k < nsplit) {  // (uniform)
            const float f = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, fs), (int)k));
            sum += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ls), (int)k)) * f;
            o += ov[k] * f;
        }
    for (u32 s0 = 32u; s0 < nsplit; s0 += 8u) {
        float ow[8];
#pragma unroll
        for (u32 k = 0; k < 8; k++) ow[k] = s0 + k < nsplit ? wp[(s0 + k) * (HD + 2u) + tid] : 0.f;
#pragma unroll
        for (u32 k = 0; k < 8; k++)
            if (s0 + k < nsplit) {
                const float f = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, fs), (int)(s0 + k)));
                sum += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ls), (int)(s0 + k))) * f;
                o += ow[k] * f;
            }
    }
    out[(size_t)h * HD + tid] = h2u((h16)(o / sum));
}

// ------------------------------------------------------------------------------------------------ dense fp16 GEMV
// out[n] = sum_k x[k] * W[n][k], fp32 accumulation (v_dot2_f32_f16), fp16 output -- what nn.Linear(fp16) gives at M = 1.
// Optional RMSNorm prologue on x (final norm before lm_head).  One wave = RW rows at a time, 16-byte loads,
// all K/512 * RW loads of a row group in flight.
template <int RW>
__global__ void __launch_bounds__(256) dense_gemv_kernel(const uint16_t *x, const uint16_t *W, uint16_t *out, u32 N, u32 K,
                                                         const uint16_t *normw, float eps, u32 rows_per_block) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint16_t *xs = reinterpret_cast<uint16_t *>(smem);
    float *red = reinterpret_cast<float *>(xs + K);
    const u32 tid = threadIdx.x, w = tid >> 6, l = tid & 63u;
    gq_dense::stage_x(x, normw, eps, K, xs, red, tid, w, l);  // (dense_stage.h: shared with the int8 head, head_q8.hip)
    const u32 row_begin = blockIdx.x * rows_per_block;
    const u32 row_end = min(row_begin + rows_per_block, N);
    for (u32 r0 = row_begin + w * RW; r0 < row_end; r0 += 4 * RW) {
        float acc[RW];
#pragma unroll
        for (int r = 0; r < RW; r++) acc[r] = 0.f;
        for (u32 k0 = l * 8u; k0 < K; k0 += 512u) {
            const uint4 xv = *reinterpret_cast<const uint4 *>(xs + k0);
            uint4 wv[RW];
#pragma unroll
            for (int r = 0; r < RW; r++) {
                const u32 row = min(r0 + (u32)r, N - 1u);
                const u32x4 t4 = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(W + (size_t)row * K + k0));
                wv[r] = make_uint4(t4.x, t4.y, t4.z, t4.w);
            }
#pragma unroll
            for (int r = 0; r < RW; r++) {
                acc[r] = __builtin_amdgcn_fdot2(__builtin_bit_cast(h16x2, wv[r].x), __builtin_bit_cast(h16x2, xv.x), acc[r], false);
                acc[r] = __builtin_amdgcn_fdot2(__builtin_bit_cast(h16x2, wv[r].y), __builtin_bit_cast(h16x2, xv.y), acc[r], false);
                acc[r] = __builtin_amdgcn_fdot2(__builtin_bit_cast(h16x2, wv[r].z), __builtin_bit_cast(h16x2, xv.z), acc[r], false);
                acc[r] = __builtin_amdgcn_fdot2(__builtin_bit_cast(h16x2, wv[r].w), __builtin_bit_cast(h16x2, xv.w), acc[r], false);
            }
        }
#pragma unroll
        for (int r = 0; r < RW; r++) {
            const float s = wave_reduce_bcast<false>(acc[r]);
            if (l == 0 && r0 + (u32)r < row_end) out[r0 + r] = h2u((h16)s);
        }
    }
}


}  // namespace

extern "C" int gq_embed_lookup(const int *token, const void *table, void *out, uint32_t dim, uint32_t vocab, void *stream) {
    if (!token || !table || !out) return gq_fail(GQ_EINVAL, "null pointer argument.");
    if (dim % 8u) return gq_fail(GQ_EINVAL, "embedding dim must be a multiple of 8.");
    hipLaunchKernelGGL(embed_kernel, dim3((dim / 8u + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, token,
                       (const uint16_t *)table, (uint16_t *)out, dim, vocab);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}
extern "C" int gq_embed_lookup_ho(const int *token, const void *table, void *out, uint32_t dim, uint32_t vocab, float *ssq_out, void *stream) {
    if (!ssq_out) return gq_embed_lookup(token, table, out, dim, vocab, stream);
    if (!token || !table || !out) return gq_fail(GQ_EINVAL, "null pointer argument.");
    if (dim % 8u) return gq_fail(GQ_EINVAL, "embedding dim must be a multiple of 8.");
    hipLaunchKernelGGL(embed_ssq_kernel, dim3(1), dim3(GQ_SSQ_SLOTS), 0, (hipStream_t)stream, token, (const uint16_t *)table, (uint16_t *)out, dim,
                       vocab, ssq_out);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}

namespace {
// the argument checks every attention launch shares, in the order they have always been made (any_null: one of the launch's own pointer
// arguments is null; misaligned: the message of the launch's own alignment check where it failed and comes in front of the sizes)
int attn_check_args(bool any_null, const char *misaligned, bool win, uint32_t window, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim,
                    uint32_t n_split, const float *workspace) {
    if (win && window == 0u) return gq_fail(GQ_EINVAL, "window must be at least 1 (the query attends itself).");
    if (any_null) return gq_fail(GQ_EINVAL, "null pointer argument.");
    if (misaligned) return gq_fail(GQ_EINVAL, misaligned);
    if (n_kv_head == 0 || n_head % n_kv_head) return gq_fail(GQ_EINVAL, "n_head must be a multiple of n_kv_head.");
    if (head_dim != 64 && head_dim != 128) return gq_fail(GQ_ENOTSUP, "head_dim must be 64 or 128.");
    if (n_split < 1u || n_split > 64u || (n_split > 1u && !workspace)) return gq_fail(GQ_EINVAL, "n_split in 1..64, with a workspace when > 1.");
    return GQ_OK;
}

template <bool QT, bool QKN = false, bool QB = false, bool WIN = false>
int attn_launch(const void *qkv, const AttnQt &qt, const int *pos, const void *cos_table, const void *sin_table, void *k_cache, void *v_cache,
                void *out, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq, float scale, uint32_t n_split,
                float *workspace, void *stream, const void *q_norm_weight = nullptr, const void *k_norm_weight = nullptr, float eps = 0.f,
                const void *qkv_bias = nullptr, uint32_t window = 0u) {
    static_assert(!(QT && QKN), "the QK-norm form reads fp16 q / k / v");
    static_assert(!(QT && WIN), "the QTIP form has no window form");
    static_assert(!(QB && (QT || QKN)), "the bias form does not combine with the QTIP or the QK-norm form");
    const bool any_null = (!QT && !qkv) || !pos || !cos_table || !sin_table || !k_cache || !v_cache || !out ||
                          (QKN && (!q_norm_weight || !k_norm_weight)) || (QB && !qkv_bias);
    const char *misaligned = QB && ((uintptr_t)qkv_bias & 15u) ? "gq_attn_decode_split_bias: 16-byte aligned bias." : nullptr;
    if (const int rc = attn_check_args(any_null, misaligned, WIN, window, n_head, n_kv_head, head_dim, n_split, workspace)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(n_head, n_split);
#define GQ_LAUNCH_ATTN(HD_)                                                                                                                   \
    do {                                                                                                                                      \
        static GqPerDeviceOnce once;                                                                                                          \
        GQ_HIP_CHECK(once.max_dynamic_lds(reinterpret_cast<const void *>(attn_decode_kernel<HD_, QT, QKN, QB, WIN>), 160 * 1024));            \
        hipLaunchKernelGGL((attn_decode_kernel<HD_, QT, QKN, QB, WIN>), grid, dim3(64 * ATTN_WAVES), gq_attn::DecodeLds<HD_>::bytes(QT), s,   \
                           (const uint16_t *)qkv, pos, (const uint16_t *)cos_table, (const uint16_t *)sin_table, (uint16_t *)k_cache, (uint16_t *)v_cache, \
                           (uint16_t *)out, n_head, n_kv_head, max_seq, scale, n_split, workspace, qt, nm, bs, wn);                           \
        if (n_split > 1u)                                                                                                                     \
            hipLaunchKernelGGL((attn_combine_kernel<HD_, WIN>), dim3(n_head), dim3(HD_), 0, s, workspace, (uint16_t *)out, n_split, pos,      \
                               max_seq, wn);                                                                                                  \
    } while (0)
    AttnWindow<WIN> wn{};
    if constexpr (WIN) wn = AttnWindow<true>{window};
    AttnQkNorm<QKN> nm{};
    if constexpr (QKN) nm = AttnQkNorm<true>{(const uint16_t *)q_norm_weight, (const uint16_t *)k_norm_weight, eps};
    AttnBias<QB> bs{};
    if constexpr (QB) bs = AttnBias<true>{(const uint16_t *)qkv_bias};
    if (head_dim == 128) GQ_LAUNCH_ATTN(128);
    else GQ_LAUNCH_ATTN(64);
#undef GQ_LAUNCH_ATTN
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}
}  // namespace

extern "C" int gq_attn_decode_split(const void *qkv, const int *pos, const void *cos_table, const void *sin_table, void *k_cache,
                                    void *v_cache, void *out, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq,
                                    float scale, uint32_t n_split, float *workspace, void *stream) {
    return attn_launch<false>(qkv, AttnQt{}, pos, cos_table, sin_table, k_cache, v_cache, out, n_head, n_kv_head, head_dim, max_seq, scale, n_split,
                              workspace, stream);
}

// Qwen3 layers: gq_attn_decode_split with the per-head RMSNorm of q and k (weights fp16 [head_dim], shared by all heads) in front of
// the rotation, inside the same launch
extern "C" int gq_attn_decode_split_qknorm(const void *qkv, const int *pos, const void *cos_table, const void *sin_table, void *k_cache,
                                           void *v_cache, void *out, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq,
                                           float scale, uint32_t n_split, float *workspace, const void *q_norm_weight,
                                           const void *k_norm_weight, float eps, void *stream) {
    return attn_launch<false, true>(qkv, AttnQt{}, pos, cos_table, sin_table, k_cache, v_cache, out, n_head, n_kv_head, head_dim, max_seq, scale,
                                    n_split, workspace, stream, q_norm_weight, k_norm_weight, eps);
}

// Qwen2 / Qwen2.5 layers: gq_attn_decode_split with the bias of the q / k / v linears (fp16 [(n_head + 2 n_kv_head) * head_dim], laid out
// like the packed q | k | v vector, 16-byte aligned) added in fp16 in front of the rotation, inside the same launch
extern "C" int gq_attn_decode_split_bias(const void *qkv, const int *pos, const void *cos_table, const void *sin_table, void *k_cache,
                                         void *v_cache, void *out, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq,
                                         float scale, uint32_t n_split, float *workspace, const void *qkv_bias, void *stream) {
    return attn_launch<false, false, true>(qkv, AttnQt{}, pos, cos_table, sin_table, k_cache, v_cache, out, n_head, n_kv_head, head_dim, max_seq,
                                           scale, n_split, workspace, stream, nullptr, nullptr, 0.f, qkv_bias);
}

// Sliding-window layers (Mistral, Qwen2 / Qwen3 with use_sliding_window): the three forms above over the cached rows (*pos - window, *pos]
// only -- the geometry of the launch without a window at position n - 1, shifted by lo (attn_core.h, AttnWindow)
extern "C" int gq_attn_decode_split_window(const void *qkv, const int *pos, const void *cos_table, const void *sin_table, void *k_cache,
                                           void *v_cache, void *out, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq,
                                           float scale, uint32_t n_split, float *workspace, uint32_t window, void *stream) {
    return attn_launch<false, false, false, true>(qkv, AttnQt{}, pos, cos_table, sin_table, k_cache, v_cache, out, n_head, n_kv_head, head_dim,
                                                  max_seq, scale, n_split, workspace, stream, nullptr, nullptr, 0.f, nullptr, window);
}
extern "C" int gq_attn_decode_split_qknorm_window(const void *qkv, const int *pos, const void *cos_table, const void *sin_table, void *k_cache,
                                                  void *v_cache, void *out, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim,
                                                  uint32_t max_seq, float scale, uint32_t n_split, float *workspace, const void *q_norm_weight,
                                                  const void *k_norm_weight, float eps, uint32_t window, void *stream) {
    return attn_launch<false, true, false, true>(qkv, AttnQt{}, pos, cos_table, sin_table, k_cache, v_cache, out, n_head, n_kv_head, head_dim,
                                                 max_seq, scale, n_split, workspace, stream, q_norm_weight, k_norm_weight, eps, nullptr, window);
}
extern "C" int gq_attn_decode_split_bias_window(const void *qkv, const int *pos, const void *cos_table, const void *sin_table, void *k_cache,
                                                void *v_cache, void *out, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq,
                                                float scale, uint32_t n_split, float *workspace, const void *qkv_bias, uint32_t window,
                                                void *stream) {
    return attn_launch<false, false, true, true>(qkv, AttnQt{}, pos, cos_table, sin_table, k_cache, v_cache, out, n_head, n_kv_head, head_dim,
                                                 max_seq, scale, n_split, workspace, stream, nullptr, nullptr, 0.f, qkv_bias, window);
}

// QTIP models: the same attention with the transform-out of the q, k and v linears folded in (qkv_lin[0..2]: the GqQtipOut
// descriptors gq_qtip_linear_out would take; resid / out unused).  Equal to gq_qtip_linear_out + gq_attn_decode_split up to fp32
// rounding (the segments are combined first: the additions of the full transform in another order), not bit for bit.
extern "C" int gq_attn_decode_qtip(const GqQtipOut *qkv_lin, const int *pos, const void *cos_table, const void *sin_table, void *k_cache,
                                   void *v_cache, void *out, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq,
                                   float scale, uint32_t n_split, float *workspace, void *stream) {
    if (!qkv_lin) return gq_fail(GQ_EINVAL, "null pointer argument.");
    AttnQt qt{};
    for (int i = 0; i < 3; i++) {
        const uint32_t want = (i == 0 ? n_head : n_kv_head) * head_dim, M = qkv_lin[i].M;
        if (M != want || (M & (M - 1u)) || !qkv_lin[i].y32 || !qkv_lin[i].SV32 || (((uintptr_t)qkv_lin[i].y32 | (uintptr_t)qkv_lin[i].SV32) & 15u) ||
            qkv_lin[i].parts > 4u || M > 16u * 64u * ATTN_WAVES)
            return gq_fail(GQ_ENOTSUP, "gq_attn_decode_qtip: q / k / v widths must be n_head (n_kv_head) * head_dim, powers of two, 16-byte aligned sums.");
        qt.y32[i] = qkv_lin[i].y32;
        qt.sv32[i] = qkv_lin[i].SV32;
        qt.M[i] = M;
        qt.parts[i] = qkv_lin[i].parts ? qkv_lin[i].parts : 1u;
        qt.mscale[i] = (float)pow((double)M, -0.5);
    }
    return attn_launch<true>(nullptr, qt, pos, cos_table, sin_table, k_cache, v_cache, out, n_head, n_kv_head, head_dim, max_seq, scale, n_split,
                             workspace, stream);
}


// Attention of the decode step when the wqkv launch has already rotated q / k and written k / v of the current token into the
// caches (gq_anyprec_gemv_qkv_rope): q fp16 [n_head * head_dim] rotated; the caches hold every position <= *pos.
namespace {
template <bool WIN, bool KV8 = false>
int roped_launch(const void *q, const int *pos, const void *k_cache, const void *v_cache, void *out, uint32_t n_head, uint32_t n_kv_head,
                 uint32_t head_dim, uint32_t max_seq, float scale, uint32_t n_split, float *workspace, uint32_t window, void *stream,
                 const float *k_scale = nullptr, const float *v_scale = nullptr) {
    using CE = typename gq_attn::CacheFmt<KV8>::elem;
    const bool any_null = !q || !pos || !k_cache || !v_cache || !out || (KV8 && (!k_scale || !v_scale));
    if (const int rc = attn_check_args(any_null, nullptr, WIN, window, n_head, n_kv_head, head_dim, n_split, workspace)) return rc;
    AttnWindow<WIN> wn{};
    if constexpr (WIN) wn = AttnWindow<true>{window};
    gq_attn::AttnKv8<KV8> k8{};
    if constexpr (KV8) k8 = gq_attn::AttnKv8<true>{k_scale, v_scale};
    if (((uintptr_t)q | (uintptr_t)k_cache | (uintptr_t)v_cache) & 15u) return gq_fail(GQ_EINVAL, "buffers must be 16-byte aligned.");
    hipStream_t s = (hipStream_t)stream;
    // grouped-query models with a split cache: the 4 query heads of a KV group in one block (every cached row loaded once)
    const bool gqa = n_split >= 4u && (n_head / n_kv_head) % 4u == 0u && gq_env_int("GQ_ATTN_GQA", 1);  // (8 heads per group: two blocks of 4)
#ifdef GQ_ATTN_PROBE
    const u32 copies = (u32)gq_env_int("GQ_ATTN_PROBE_COPIES", 0);
    const bool gqa_p = copies > 0u;
    const u32 qh = gqa_p || gqa ? 4u : 1u;
    const dim3 grid(n_head / qh, gqa_p ? copies : n_split);
    if (gqa_p && !WIN) {
        static GqPerDeviceOnce once;
        GQ_HIP_CHECK(once.max_dynamic_lds(reinterpret_cast<const void *>(attn_roped_kernel<128, 4, false, KV8>), 160 * 1024));
        hipLaunchKernelGGL((attn_roped_kernel<128, 4, false, KV8>), grid, dim3(64 * ATTN_WAVES), (gq_attn::RopedLds<128, 4>::bytes()), s, (const uint16_t *)q, pos,
                           (const CE *)k_cache, (const CE *)v_cache, (uint16_t *)out, n_head, n_kv_head, max_seq, scale, 1u, workspace,
                           AttnWindow<false>{}, k8);
        GQ_HIP_CHECK(hipGetLastError());
        return GQ_OK;
    }
#else
    const u32 qh = gqa ? 4u : 1u;
    const dim3 grid(n_head / qh, n_split);
#endif
#define GQ_LAUNCH_ROPED(HD_, QH_)                                                                                                    \
    do {                                                                                                                             \
        static GqPerDeviceOnce once;                                                                                                 \
        GQ_HIP_CHECK(once.max_dynamic_lds(reinterpret_cast<const void *>(attn_roped_kernel<HD_, QH_, WIN, KV8>), 160 * 1024));        \
        hipLaunchKernelGGL((attn_roped_kernel<HD_, QH_, WIN, KV8>), grid, dim3(64 * ATTN_WAVES), (gq_attn::RopedLds<HD_, QH_>::bytes()), s, \
                           (const uint16_t *)q, pos, (const CE *)k_cache, (const CE *)v_cache, (uint16_t *)out, n_head,               \
                           n_kv_head, max_seq, scale, n_split, workspace, wn, k8);                                                   \
        if (n_split > 1u)                                                                                                            \
            hipLaunchKernelGGL((attn_combine_kernel<HD_, WIN>), dim3(n_head), dim3(HD_), 0, s, workspace, (uint16_t *)out, n_split,   \
                               pos, max_seq, wn);                                                                                    \
    } while (0)
    if (head_dim == 128) {
        if (gqa) GQ_LAUNCH_ROPED(128, 4);
        else GQ_LAUNCH_ROPED(128, 1);
    } else {
        if (gqa) GQ_LAUNCH_ROPED(64, 4);
        else GQ_LAUNCH_ROPED(64, 1);
    }
#undef GQ_LAUNCH_ROPED
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}
}  // namespace

extern "C" int gq_attn_decode_roped(const void *q, const int *pos, const void *k_cache, const void *v_cache, void *out, uint32_t n_head,
                                    uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq, float scale, uint32_t n_split, float *workspace,
                                    void *stream) {
    return roped_launch<false>(q, pos, k_cache, v_cache, out, n_head, n_kv_head, head_dim, max_seq, scale, n_split, workspace, 0u, stream);
}
// the window form (the caches hold every row of (*pos - window, *pos]; rows below stay in the cache and are not read)
extern "C" int gq_attn_decode_roped_window(const void *q, const int *pos, const void *k_cache, const void *v_cache, void *out, uint32_t n_head,
                                           uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq, float scale, uint32_t n_split,
                                           float *workspace, uint32_t window, void *stream) {
    return roped_launch<true>(q, pos, k_cache, v_cache, out, n_head, n_kv_head, head_dim, max_seq, scale, n_split, workspace, window, stream);
}
// the fp8 (e4m3) cache form of the two entries above (window 0: the whole context): the same launches over caches of one byte per
// element, scales fp32 [n_kv_head] in device memory
extern "C" int gq_attn_decode_roped_kv8(const void *q, const int *pos, const void *k_cache, const void *v_cache, const float *k_scale,
                                        const float *v_scale, void *out, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq,
                                        float scale, uint32_t n_split, float *workspace, uint32_t window, void *stream) {
    if (window)
        return roped_launch<true, true>(q, pos, k_cache, v_cache, out, n_head, n_kv_head, head_dim, max_seq, scale, n_split, workspace, window, stream,
                                        k_scale, v_scale);
    return roped_launch<false, true>(q, pos, k_cache, v_cache, out, n_head, n_kv_head, head_dim, max_seq, scale, n_split, workspace, 0u, stream,
                                     k_scale, v_scale);
}

extern "C" int gq_attn_decode(const void *qkv, const int *pos, const void *cos_table, const void *sin_table, void *k_cache,
                              void *v_cache, void *out, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq,
                              float scale, void *stream) {
    return gq_attn_decode_split(qkv, pos, cos_table, sin_table, k_cache, v_cache, out, n_head, n_kv_head, head_dim, max_seq, scale, 1u,
                                nullptr, stream);
}

extern "C" int gq_dense_gemv_f16(const void *x, const void *W, void *out, uint32_t N, uint32_t K, const void *norm_weight,
                                 float eps, void *stream) {
    if (!x || !W || !out) return gq_fail(GQ_EINVAL, "null pointer argument.");
    if (K == 0 || K % 512u || N == 0) return gq_fail(GQ_EINVAL, "dense GEMV needs N > 0 and K a positive multiple of 512.");
    if ((((uintptr_t)x | (uintptr_t)W | (uintptr_t)norm_weight) & 15u)) return gq_fail(GQ_EINVAL, "buffers must be 16-byte aligned.");
    const size_t smem = (size_t)K * 2u + 64u;
    if (smem > 160u * 1024u) return gq_fail(GQ_ENOTSUP, "K too large.");
    constexpr int RW = 4;
    const u32 ncu = (u32)gq_cu_count();
    // ~3 blocks per CU (measured over 2 .. 16 on the 128256 x 4096 lm_head inside the decode step: 3 is 0.4 % of the token faster than 4,
    // 6 is 0.7 % slower), every block a multiple of 4 waves * RW rows
    const int bpc_env = gq_env_int("GQ_DENSE_BPC", 3);
    const u32 bpc = bpc_env >= 1 ? (u32)bpc_env : 1u;
    u32 rpb = (N + ncu * bpc - 1u) / (ncu * bpc);
    rpb = ((rpb + 4u * RW - 1u) / (4u * RW)) * (4u * RW);
    {   // (GQ_DENSE_RPB: rows per block directly, a multiple of 16 -- the sweep of profiles/r05_knob_sweep.txt)
        const int rpb_env = gq_env_int("GQ_DENSE_RPB", 0);
        if (rpb_env >= 16 && rpb_env % 16 == 0) rpb = (u32)rpb_env;
    }
    const u32 grid = (N + rpb - 1u) / rpb;
    static GqPerDeviceOnce once;
    GQ_HIP_CHECK(once.max_dynamic_lds(reinterpret_cast<const void *>(dense_gemv_kernel<RW>), 160 * 1024));
    hipLaunchKernelGGL(dense_gemv_kernel<RW>, dim3(grid), dim3(256), smem, (hipStream_t)stream, (const uint16_t *)x,
                       (const uint16_t *)W, (uint16_t *)out, N, K, (const uint16_t *)norm_weight, eps, rpb);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}
