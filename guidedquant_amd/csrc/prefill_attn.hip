// prefill_attn.hip -- the attention of the PROMPT pass: a flash-attention forward for gfx950 over one batch slot of the KV cache,
// causal, with an offset (a later chunk of a prompt attends the cached chunks in front of it), a sliding window, grouped heads.
//   q    fp16 [n_head][S][head_dim]            (what gq_rope_cache_rows / gq_qknorm_rope_cache_rows write)
//   k, v fp16 [n_kv_head][max_seq][head_dim]   (one batch slot of KVCache; rows [0, start + S) written)
//   out  fp16 [S][n_head * head_dim]           (the rows wo reads)
// Query row i sits at position p = start + i and attends the cache rows t <= p, with a window also t > p - window
// (model.py window_mask).
//
// One block of 4 waves per (tile of BQ = 64 query rows, head); wave w owns 16 query rows.  Key tiles of BK = 64 rows go through LDS,
// row-major for K and for V, the next tile's global loads in flight (in registers) while the current one is computed.  Both
// products run on v_mfma_f32_16x16x32_f16 and are TRANSPOSED, so that the query is the accumulator's column (its lane, l & 15) in
// both and the softmax statistics never leave their lane group:
//   S^T = K Q^T    A = K rows (ds_read_b128), B = Q^T from registers.  The 16 MFMA rows of score block b are the tile's keys
//                  32 (b >> 1) + 8 (row >> 2) + 4 (b & 1) + (row & 3): lane group g = l >> 4 then holds, in blocks 2c and 2c + 1, the
//                  EIGHT CONSECUTIVE keys 32 c + 8 g .. + 7 of its query -- exactly the B fragment of k-step c of the second product.
//   O^T = V^T P^T  A = V^T through ds_read_b64_tr_b16 on the row-major image (two reads of 4 keys x 16 columns per fragment),
//                  B = P^T = exp2 of the scores, rounded to fp16 AT THE SCALE 2^PK, straight from the accumulators.
// The online softmax is fp32 with scale * log2(e) folded into one multiply and v_exp_f32; a masked score is REPLACED (select), a
// masked P is exactly 0, and a row that has seen only masked keys so far keeps sum 0 (its running maximum stays at NEG, finite).
// P = exp2(s - m) <= 1 is taken as exp2(s - (m - PK)) = P 2^PK <= 32768 (PK = 15: one subtraction per tile), the numerator AND the
// normaliser accumulate the scaled weights, and o / l is what it was: a power of two moves through every step exactly.  Unscaled, a
// weight under 2^-14 was an fp16 subnormal and one under 2^-25 exactly 0 in the numerator while the fp32 normaliser kept it: behind a
// large first key (an attention sink) T keys of weight just under 2^-25 lost T 2^-25 of the softmax with one sign -- 0.4 % of max|V|
// at 2^17 keys, twice that at 2^18, where the decode kernels (fp32 weights, attn_core.h) lose nothing.  Scaled, the flush sits at
// 2^-40 relative to the row maximum and every weight above 2^-29 is a normal fp16 number.
// Error against float64, elementwise, over T keys: (4 2^-11 + (T / 32 + T / 64) 2^-24) max|V| -- P's fp16 rounding in the numerator
// (2^-11 relative) and at most as much in the normaliser, the output's own fp16 rounding, one fp32 rounding of the accumulator per MFMA
// (32 keys) and one of a lane's normaliser share per tile, taken with one sign (tests/prefill_attn_model.py error_bound).  The sums
// stay far inside fp32: l <= 2^15 T / 4 per lane, |o| <= 2^15 T max|V|, T <= 2^30.
// Tiles wholly above the diagonal or below the window are never visited by the block, a wave skips the visited ones it has no
// key in, and only tiles astride an edge evaluate the element mask.  Rows >= start + S of a tile are not read: they are staged as
// zeros (0 x NaN inside an MFMA is NaN), so nothing at or behind row max_seq is touched.  The tile loops hold no integer division.
#include <hip/hip_runtime.h>

#include "gq_internal.h"
#include "wave_util.h"

namespace {
using u32 = uint32_t;
using gqw::f32x4;
using gqw::h16;
using gqw::h16x8;
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr u32 BQ = GQ_PREFILL_ATTN_BQ, BK = GQ_PREFILL_ATTN_BK;
static_assert(BQ == 64 && BK == 64, "4 waves x 16 query rows; 4 score blocks of 16 keys");
constexpr float NEG = -1.0e30f;  // a masked score: finite, so NEG - NEG = 0 and never Inf - Inf
constexpr float PK = 15.0f;      // P is rounded to fp16 as P 2^PK (<= 32768 < 65504)

__device__ __forceinline__ h16x4 lds_read_tr(const h16 *p) {
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    return __builtin_bit_cast(h16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)p));
}

// the cache format of an instance.  fp8 (gq_attn_prefill_kv8): a chunk of 8 elements is 8 bytes of OCP e4m3 codes, converted to fp16 --
// exactly: every e4m3 value is an fp16 value -- between the global load and the LDS store, so the LDS image, the fragments and both
// products are those of the fp16 instance on the same numbers; the scales (fp32 per KV head, device memory) stay outside the products
template <bool KV8>
struct TileFmt {
    typedef uint16_t elem;
    typedef uint4 chunk;
    struct Scales {};
    static __device__ __forceinline__ chunk zero() { return make_uint4(0u, 0u, 0u, 0u); }
    static __device__ __forceinline__ uint4 to_f16(const chunk &v) { return v; }
};
template <>
struct TileFmt<true> {
    typedef uint8_t elem;
    typedef uint2 chunk;
    struct Scales {
        const float *k_scale, *v_scale;
    };
    static __device__ __forceinline__ chunk zero() { return make_uint2(0u, 0u); }
    static __device__ __forceinline__ uint4 to_f16(const chunk &v) {
        const u32 w[2] = {v.x, v.y};
        u32 o[4];
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[e], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[e], true);
            o[2 * e] = (u32)__builtin_bit_cast(uint16_t, (h16)lo[0]) | ((u32)__builtin_bit_cast(uint16_t, (h16)lo[1]) << 16);
            o[2 * e + 1] = (u32)__builtin_bit_cast(uint16_t, (h16)hi[0]) | ((u32)__builtin_bit_cast(uint16_t, (h16)hi[1]) << 16);
        }
        return make_uint4(o[0], o[1], o[2], o[3]);
    }
};

// the kernel's last argument: the scales of an fp8 cache, or -- PACKED, fp16 caches -- the segment begins (an instance that is neither
// keeps the empty struct it had: its arguments and its code are those of the kernel without the flag)
template <bool KV8, bool PACKED>
struct TailArg {
    typedef typename TileFmt<KV8>::Scales type;
};
template <>
struct TailArg<false, true> {
    struct type {
        const int *seg_begin;
    };
};

// PACKED: the first key row `i` attends: its segment's begin, clamped to i (a malformed array never leaves rows [0, S)), or the window's
__device__ __forceinline__ u32 packed_lo(const int *__restrict__ seg_begin, u32 i, u32 window) {
    const u32 sb = min((u32)seg_begin[i], i);
    return (window && i + 1u > window) ? max(sb, i + 1u - window) : sb;
}

// PACKED (gq_attn_prefill_packed): N sequences as one run of S rows from cache row 0.  Row i attends max(seg_begin[i], i + 1 - window)
// <= t <= i.  Both bounds are non-decreasing in i, so the block's first tile comes from its first row, a wave's rows attend one run of
// keys [lo of its first row, its last row], and a tile every row of the wave attends whole lies inside ONE segment.  Every other visited
// tile is an edge tile: the element mask gets the term t >= lo(i), and the second product runs once per segment among the wave's 16
// rows, with the V fragment's keys outside [that segment's begin, its last row in the wave] replaced by zeros and the result kept by
// that segment's rows only -- P = 0 alone does not keep another sequence's rows out: 0 x NaN inside an MFMA is NaN.  For a row the
// products and their order are those of the one-sequence kernel (a masked key adds +-0 either way), so row i is bit for bit row i of
// gq_attn_prefill(S = i + 1, start = 0, window = min(i - seg_begin[i] + 1, window)).
template <int HD, bool KV8 = false, bool PACKED = false>
__global__ void __launch_bounds__(256) prefill_attn_kernel(const uint16_t *__restrict__ q, const typename TileFmt<KV8>::elem *__restrict__ kc,
                                                           const typename TileFmt<KV8>::elem *__restrict__ vc, uint16_t *__restrict__ out, u32 S,
                                                           u32 start, u32 H, u32 group, u32 max_seq, float c, u32 window,
                                                           typename TailArg<KV8, PACKED>::type sc) {
    static_assert(!(KV8 && PACKED), "the packed pass has fp16 caches");
    using Fmt = TileFmt<KV8>;
    using Chunk = typename Fmt::chunk;
    constexpr u32 LD = HD + 8;             // halves per LDS row: 16 bytes of padding
    constexpr u32 CH = HD / 8;             // 16-byte chunks per row
    constexpr u32 NCH = BK * CH / 256;     // chunks per thread and matrix
    constexpr u32 KS = HD / 32, DB = HD / 16;
    __shared__ __attribute__((aligned(16))) h16 sK[BK * LD];
    __shared__ __attribute__((aligned(16))) h16 sV[BK * LD];

    const u32 tid = threadIdx.x, w = tid >> 6, l = tid & 63u, g = l >> 4, li = l & 15u;
    const u32 head = blockIdx.y, kvh = head / group;  // (once per block)
    const u32 q0 = (gridDim.x - 1u - blockIdx.x) * BQ;  // the long rows of the triangle first
    const u32 T = start + S;
    const typename Fmt::elem *kbase = kc + (size_t)kvh * max_seq * HD, *vbase = vc + (size_t)kvh * max_seq * HD;
    if constexpr (KV8) c *= sc.k_scale[kvh];  // (the K scale: one factor of the scores)

    // the block's key range: [klo, khi] covers every key one of its rows attends
    const u32 p_lo = start + q0, khi = start + min(q0 + BQ - 1u, S - 1u);
    u32 klo;
    if constexpr (PACKED) klo = packed_lo(sc.seg_begin, q0, window);  // (start == 0: a position is a row)
    else klo = (window && p_lo + 1u > window) ? p_lo + 1u - window : 0u;
    const u32 kt0 = klo / BK, kt1 = khi / BK;

    // the wave's rows (rows >= S repeat row S - 1 and are not stored)
    const u32 wq0 = q0 + 16u * w;
    const bool wave_active = wq0 < S;
    const u32 qrow = wq0 + li, qi = min(qrow, S - 1u), p = start + qi;
    const u32 pmin = start + min(wq0, S - 1u), pmax = start + min(wq0 + 15u, S - 1u);
    // PACKED: the row's own first key and segment begin; the first keys of the wave's first and last row (lanes 0 and 15)
    u32 lo = 0u, sb = 0u, lo_min = 0u, lo_max = 0u;
    if constexpr (PACKED) {
        lo = packed_lo(sc.seg_begin, qi, window);
        sb = min((u32)sc.seg_begin[qi], qi);
        lo_min = (u32)__builtin_amdgcn_readlane((int)lo, 0);
        lo_max = (u32)__builtin_amdgcn_readlane((int)lo, 15);
    }

    h16x8 qf[KS];
    {
        const uint16_t *qr = q + ((size_t)head * S + qi) * HD + 8u * g;
#pragma unroll
        for (u32 ks = 0; ks < KS; ks++) qf[ks] = __builtin_bit_cast(h16x8, *reinterpret_cast<const uint4 *>(qr + 32u * ks));
    }

    Chunk kreg[NCH], vreg[NCH];
    auto load_tile = [&](u32 kt) {
#pragma unroll
        for (u32 i = 0; i < NCH; i++) {
            const u32 id = tid + 256u * i, row = id / CH, col = id % CH, t = kt * BK + row;  // (CH: a power of two)
            if (t < T) {
                kreg[i] = *reinterpret_cast<const Chunk *>(kbase + (size_t)t * HD + 8u * col);
                vreg[i] = *reinterpret_cast<const Chunk *>(vbase + (size_t)t * HD + 8u * col);
            } else {
                kreg[i] = Fmt::zero();
                vreg[i] = Fmt::zero();
            }
        }
    };

    f32x4 o[DB];
#pragma unroll
    for (u32 d = 0; d < DB; d++) o[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = NEG, l_run = 0.f;  // l_run: this lane's share of the row sum of P 2^PK (the four lane groups of a query are added at the end)

    load_tile(kt0);
    for (u32 kt = kt0; kt <= kt1; kt++) {
        __syncthreads();  // every wave is through with the tile in LDS
#pragma unroll
        for (u32 i = 0; i < NCH; i++) {
            const u32 id = tid + 256u * i, row = id / CH, col = id % CH;
            *reinterpret_cast<uint4 *>(&sK[row * LD + 8u * col]) = Fmt::to_f16(kreg[i]);
            *reinterpret_cast<uint4 *>(&sV[row * LD + 8u * col]) = Fmt::to_f16(vreg[i]);
        }
        __syncthreads();
        if (kt < kt1) load_tile(kt + 1u);  // in flight under the products below

        const u32 tb = kt * BK;
        // (wave-uniform: EXEC stays full for the transposed reads)
        bool edge;
        if constexpr (PACKED) {
            if (!(wave_active && tb <= pmax && tb + (BK - 1u) >= lo_min)) continue;
            edge = tb + (BK - 1u) > pmin || tb < lo_max;
        } else {
            if (!(wave_active && tb <= pmax && (window == 0u || tb + (BK - 1u) + window > pmin))) continue;
            edge = tb + (BK - 1u) > pmin || (window != 0u && tb + window <= pmax);
        }

        f32x4 s[4];
#pragma unroll
        for (u32 b = 0; b < 4; b++) {
            s[b] = f32x4{0.f, 0.f, 0.f, 0.f};
            const u32 krow = 32u * (b >> 1) + 8u * (li >> 2) + 4u * (b & 1u) + (li & 3u);
#pragma unroll
            for (u32 ks = 0; ks < KS; ks++) {
                const h16x8 a = *reinterpret_cast<const h16x8 *>(&sK[krow * LD + 32u * ks + 8u * g]);
                s[b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, qf[ks], s[b], 0, 0, 0);
            }
        }
        // scores in the exp2 domain; the masked ones replaced
        bool ok[4][4];
        float mloc = NEG;
#pragma unroll
        for (u32 b = 0; b < 4; b++) {
#pragma unroll
            for (u32 r = 0; r < 4; r++) {
                const u32 t = tb + 32u * (b >> 1) + 8u * g + 4u * (b & 1u) + r;
                if constexpr (PACKED) ok[b][r] = !edge || (t <= p && t >= lo);
                else ok[b][r] = !edge || (t <= p && (window == 0u || t + window > p));
                const float x = s[b][r] * c;
                s[b][r] = ok[b][r] ? x : NEG;
                mloc = fmaxf(mloc, s[b][r]);
            }
        }
        mloc = fmaxf(mloc, __shfl_xor(mloc, 16, 64));
        mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
        const float m_new = fmaxf(m_run, mloc);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        m_run = m_new;
        const float m_pk = m_new - PK;  // (NEG - PK = NEG: a row of masked keys only is unchanged)
        float psum = 0.f;
        h16x8 pf[2];
#pragma unroll
        for (u32 b = 0; b < 4; b++) {
#pragma unroll
            for (u32 r = 0; r < 4; r++) {
                const float pe = ok[b][r] ? __builtin_amdgcn_exp2f(s[b][r] - m_pk) : 0.f;
                psum += pe;
                pf[b >> 1][4u * (b & 1u) + r] = (h16)pe;
            }
        }
        l_run = l_run * alpha + psum;
        if constexpr (PACKED) {
            if (edge) {
#pragma unroll
                for (u32 d = 0; d < DB; d++) o[d] *= alpha;
                unsigned long long todo = 0xFFFFull;  // the wave's 16 queries (lanes 0 .. 15 hold one each), a segment at a time
                while (todo) {
                    const u32 sfirst = (u32)__builtin_amdgcn_readlane((int)sb, __builtin_ctzll(todo));
                    const bool mine = sb == sfirst;
                    const unsigned long long members = __ballot(mine) & 0xFFFFull;  // (never empty: the lane read from is one)
                    todo &= ~members;
                    const u32 slast = (u32)__builtin_amdgcn_readlane((int)p, 63 - __builtin_clzll(members));
#pragma unroll
                    for (u32 d = 0; d < DB; d++) {
#pragma unroll
                        for (u32 cc = 0; cc < 2; cc++) {
                            const h16 *vp = &sV[(32u * cc + 8u * g + (li >> 2)) * LD + 16u * d + 4u * (li & 3u)];
                            const h16x4 vlo = lds_read_tr(vp), vhi = lds_read_tr(vp + 4u * LD);
                            h16x8 a = __builtin_shufflevector(vlo, vhi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
                            for (u32 j = 0; j < 8; j++) {
                                const u32 t = tb + 32u * cc + 8u * g + j;
                                a[j] = (t >= sfirst && t <= slast) ? a[j] : (h16)0.f;
                            }
                            const f32x4 on = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, pf[cc], o[d], 0, 0, 0);
#pragma unroll
                            for (u32 r = 0; r < 4; r++) o[d][r] = mine ? on[r] : o[d][r];
                        }
                    }
                }
                continue;
            }
        }
#pragma unroll
        for (u32 d = 0; d < DB; d++) {
            o[d] *= alpha;
#pragma unroll
            for (u32 cc = 0; cc < 2; cc++) {
                // lane 4 q + p of a group of 16 addresses row q, columns 4 p .. 4 p + 3 of a block of 4 keys x 16 columns
                const h16 *vp = &sV[(32u * cc + 8u * g + (li >> 2)) * LD + 16u * d + 4u * (li & 3u)];
                const h16x4 lo = lds_read_tr(vp), hi = lds_read_tr(vp + 4u * LD);
                const h16x8 a = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                o[d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, pf[cc], o[d], 0, 0, 0);
            }
        }
    }

    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
    if (qrow < S) {
        float inv = 1.0f / l_run;
        if constexpr (KV8) inv *= sc.v_scale[kvh];  // (the V scale: on the output, in front of its one fp16 rounding)
        uint16_t *orow = out + (size_t)qrow * H * HD + (size_t)head * HD + 4u * g;
#pragma unroll
        for (u32 d = 0; d < DB; d++) {
            const h16x4 v = {(h16)(o[d][0] * inv), (h16)(o[d][1] * inv), (h16)(o[d][2] * inv), (h16)(o[d][3] * inv)};
            *reinterpret_cast<uint2 *>(orow + 16u * d) = __builtin_bit_cast(uint2, v);
        }
    }
}
}  // namespace

extern "C" int gq_attn_prefill_supported(uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim) {
    return (head_dim == 64u || head_dim == 128u) && n_head != 0u && n_kv_head != 0u && n_head % n_kv_head == 0u && n_head <= 65535u;
}

namespace {
template <bool KV8, bool PACKED = false>
int prefill_attn_launch(const void *q, const void *k_cache, const void *v_cache, void *out, uint32_t S, uint32_t start, uint32_t n_head,
                        uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq, float scale, uint32_t window, void *stream,
                        typename TailArg<KV8, PACKED>::type sc) {
    using CE = typename TileFmt<KV8>::elem;
    if (!gq_attn_prefill_supported(n_head, n_kv_head, head_dim))
        return gq_fail(GQ_ENOTSUP, "gq_attn_prefill: head_dim 64 or 128, n_head a multiple of n_kv_head.");
    if (!q || !k_cache || !v_cache || !out) return gq_fail(GQ_EINVAL, "null pointer argument.");
    if constexpr (PACKED) {
        if (!sc.seg_begin) return gq_fail(GQ_EINVAL, "null pointer argument.");
        if (S == 0) return gq_fail(GQ_EINVAL, "gq_attn_prefill_packed: no rows.");
    }
    if (((uintptr_t)q | (uintptr_t)k_cache | (uintptr_t)v_cache | (uintptr_t)out) & 15u) return gq_fail(GQ_EINVAL, "gq_attn_prefill: 16-byte aligned pointers.");
    const uint64_t T = (uint64_t)start + S;
    if (T > max_seq) return gq_fail(GQ_EINVAL, "gq_attn_prefill: start + S exceeds max_seq.");
    if (max_seq > 0x40000000u) return gq_fail(GQ_ENOTSUP, "gq_attn_prefill: max_seq beyond 2^30.");
    if (S == 0) return GQ_OK;
    if (window >= T) window = 0u;  // a window no row outgrows
    const float c = scale * 1.4426950408889634f;
    const dim3 grid((S + BQ - 1u) / BQ, n_head), block(256);
    const uint32_t group = n_head / n_kv_head;
    if (head_dim == 64u)
        hipLaunchKernelGGL((prefill_attn_kernel<64, KV8, PACKED>), grid, block, 0, (hipStream_t)stream, (const uint16_t *)q, (const CE *)k_cache, (const CE *)v_cache,
                           (uint16_t *)out, S, start, n_head, group, max_seq, c, window, sc);
    else
        hipLaunchKernelGGL((prefill_attn_kernel<128, KV8, PACKED>), grid, block, 0, (hipStream_t)stream, (const uint16_t *)q, (const CE *)k_cache, (const CE *)v_cache,
                           (uint16_t *)out, S, start, n_head, group, max_seq, c, window, sc);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}
}  // namespace

extern "C" int gq_attn_prefill(const void *q, const void *k_cache, const void *v_cache, void *out, uint32_t S, uint32_t start, uint32_t n_head,
                               uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq, float scale, uint32_t window, void *stream) {
    return prefill_attn_launch<false>(q, k_cache, v_cache, out, S, start, n_head, n_kv_head, head_dim, max_seq, scale, window, stream, {});
}

extern "C" int gq_attn_prefill_kv8(const void *q, const void *k_cache, const void *v_cache, const float *k_scale, const float *v_scale, void *out,
                                   uint32_t S, uint32_t start, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq, float scale,
                                   uint32_t window, void *stream) {
    if (!k_scale || !v_scale) return gq_fail(GQ_EINVAL, "null pointer argument.");
    return prefill_attn_launch<true>(q, k_cache, v_cache, out, S, start, n_head, n_kv_head, head_dim, max_seq, scale, window, stream, {k_scale, v_scale});
}

extern "C" int gq_attn_prefill_packed(const void *q, const void *k_cache, const void *v_cache, const int *seg_begin, void *out, uint32_t S,
                                      uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq, float scale, uint32_t window,
                                      void *stream) {
    return prefill_attn_launch<false, true>(q, k_cache, v_cache, out, S, 0u, n_head, n_kv_head, head_dim, max_seq, scale, window, stream, {seg_begin});
}
