// topn.hip -- the top-n alternatives of a draw with their log-probabilities, gfx950: gq_sample_topk_lp_topn and the launch pair behind
// gq_sample_full_topn (include/gq_hip.h has the contract, tests/topn_model.py the exact host model).
//
// The selection is a launch pair of its own BEHIND the sampler's launches -- the sampler's kernels are not touched, and an entry point
// without the request launches what it launched:
//   topn_stage1  128 blocks  the sampler's slices (<= 1024 logits per block up to 131072, <= 2048 up to 262144).  Every wave keeps the best n
//                            of its share by n rounds of a wave-wide maximum over unique 32-bit keys (value image, inverted position), wave
//                            0 then the best n of the 4 * n survivors: (image, token id) of rank j at cand[block * 20 + j], 0 where the
//                            slice has fewer tokens that are no NaN.
//   topn_merge   1 block     the best n of the 128 * n candidates the same way.  Slices hold ascending ids and a block's list is in the raw
//                            order, so among equal images the candidate with the lower slot number has the lower id: the key is (image,
//                            inverted slot) in 28 bits.  Wave 1 meanwhile combines the sampler's 128 log-sum-exp partials -- the words its
//                            own last launch combined, in the same fixed butterfly: the same (M, log Z) bit for bit -- and lanes j < n of
//                            wave 0 store id and (v - M) - log Z, the expression lp_raw is.
// The row is read from device memory (*pos_io as the sampler left it: the slot of the token it has just stored), the grids depend on
// nothing but the build, no host read-back: a captured graph replays the pair.  Integer maxima only; no atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gq_internal.h"
#include "sampler_core.h"
#include "wave_util.h"

namespace {

using namespace gqs;  // the value images and the log-sum-exp merge: the sampler's own, so a list's order and its log Z are the sampler's
using gqw::h2f;

constexpr int TB = 128, TT = 256, TN = GQ_TOPN_MAX;  // blocks, threads, candidate slots per block
constexpr size_t WS_HEAD = 16;                      // {M, log Z} of the last call (the test hook), then uint2 cand[TB * TN]
static_assert(GQ_TOPN_WS_BYTES == WS_HEAD + (size_t)TB * TN * 8, "the workspace of include/gq_hip.h");
static_assert(GQ_SAMPLER_MAX_VOCAB == 2048 * TB && TB * TN < 4096, "slices of <= 2048 logits; a slot number is 12 bits of the merge key");

// the maximum of an unsigned word over the 64 lanes, in every lane: wave_reduce_bcast's DPP tree with 0, the identity, wherever a lane
// has no source
__device__ __forceinline__ u32 wave_umax(u32 v) {
    auto dpp = [](u32 old, u32 x, auto ctrl, auto rows) {
        return (u32)__builtin_amdgcn_update_dpp((int)old, (int)x, decltype(ctrl)::value, decltype(rows)::value, 0xF, false);
    };
    typedef std::integral_constant<int, 0xF> all;
    v = max(v, dpp(0u, v, std::integral_constant<int, 0xB1>{}, all{}));   // quad_perm [1,0,3,2]
    v = max(v, dpp(0u, v, std::integral_constant<int, 0x4E>{}, all{}));   // quad_perm [2,3,0,1]
    v = max(v, dpp(0u, v, std::integral_constant<int, 0x141>{}, all{}));  // row_half_mirror
    v = max(v, dpp(0u, v, std::integral_constant<int, 0x140>{}, all{}));  // row_mirror
    v = max(v, dpp(0u, v, std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xA>{}));  // row_bcast15 -> rows 1, 3
    v = max(v, dpp(0u, v, std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xC>{}));  // row_bcast31 -> rows 2, 3
    return (u32)__builtin_amdgcn_readlane((int)v, 63);
}

// The n largest of the wave's 64 * EPT keys, largest first: round j takes the largest key below round j - 1's (keys are unique but for
// 0 = no key, which ends the list) and hands it to `put(j, key)` in every lane.
template <int EPT, typename Put>
__device__ __forceinline__ void wave_top_n(const u32 (&key)[EPT], int n, Put put) {
    u32 prev = 0xFFFFFFFFu;
#pragma unroll 1
    for (int j = 0; j < n; j++) {
        u32 m = 0u;
#pragma unroll
        for (int e = 0; e < EPT; e++) m = max(m, key[e] < prev ? key[e] : 0u);
        prev = wave_umax(m);
        put(j, prev);
    }
}

// stage 1: EPT = 4, LB = 10 (vocab <= 131072) or EPT = 8, LB = 11.  key = image << LB | (2^LB - 1 - position in the slice); a NaN of
// either sign has no key.  Nothing but the logits enters: no ban list, no token set, no penalty.
template <int EPT, int LB>
__global__ void __launch_bounds__(TT) topn_stage1(const uint16_t *logits, u32 V, int n, uint2 *cand) {
    static_assert(TT * EPT == 1 << LB && 16 + LB <= 32 && 2 * 64 >= 4 * TN, "one position per key of the block; wave 0 holds the survivors two per lane");
    constexpr u32 LMASK = (1u << LB) - 1u;
    __shared__ u32 surv[4 * TN];
    const u32 per = (V + TB - 1) / TB;  // <= 256 * EPT
    const u32 lo = min(blockIdx.x * per, V), hi = min(lo + per, V);
    const u32 tid = threadIdx.x, w = tid >> 6, l = tid & 63u;
    u32 key[EPT];
#pragma unroll
    for (int e = 0; e < EPT; e++) {
        const u32 li = tid * (u32)EPT + (u32)e, gi = lo + li;
        const uint16_t hb = gi < hi ? logits[gi] : (uint16_t)0x7E00u;  // (the NaN pattern: no key)
        key[e] = is_nan16(hb) ? 0u : ((ordered_key16(hb) << LB) | (LMASK - li));
    }
    wave_top_n<EPT>(key, n, [&](int j, u32 k) {
        if (l == 0) surv[w * TN + j] = k;
    });
    __syncthreads();
    if (w != 0) return;
    u32 ks[2];
    {   // survivor s = wave * n + rank, s < 4 * n <= 80: lane l takes s = l and s = 64 + l
        const u32 s0 = l, s1 = 64u + l, tot = 4u * (u32)n;
        ks[0] = s0 < tot ? surv[s0 / (u32)n * TN + s0 % (u32)n] : 0u;
        ks[1] = s1 < tot ? surv[s1 / (u32)n * TN + s1 % (u32)n] : 0u;
    }
    u32 mine = 0u;
    wave_top_n<2>(ks, n, [&](int j, u32 k) {
        if ((int)l == j) mine = k;
    });
    if ((int)l < n) {  // (slots n .. TN - 1 of a block are never read)
        const u32 li = LMASK - (mine & LMASK);
        cand[blockIdx.x * TN + l] = mine ? make_uint2(mine >> LB, lo + li) : make_uint2(0u, 0u);
    }
}

// merge: one block.  Slot c = block * TN + rank; thread tid looks at c = tid + 256 * e.  key = image << 12 | (4095 - c).
__global__ void __launch_bounds__(TT) topn_merge(const uint2 *cand, int n, const float *lse_part, const int *pos_io, int *top_ids, float *top_lps,
                                                 u32 cap, float *head) {
    static_assert(TB == 128 && TT == 256 && TB * TN == 10 * TT, "two partials per lane of wave 1; ten slots per thread");
    __shared__ u32 surv[4 * TN];
    __shared__ float lpM, lpLogZ;
    const u32 tid = threadIdx.x, w = tid >> 6, l = tid & 63u;
    u32 key[10];
#pragma unroll
    for (int e = 0; e < 10; e++) {
        const u32 c = tid + (u32)TT * (u32)e;
        const u32 img = (int)(c % (u32)TN) < n ? cand[c].x : 0u;
        key[e] = img ? ((img << 12) | (4095u - c)) : 0u;
    }
    wave_top_n<10>(key, n, [&](int j, u32 k) {
        if (l == 0) surv[w * TN + j] = k;
    });
    // (M, log Z) by the function sample_stage2 / full_finish formed theirs with, from the same words
    if (w == 1) lse_merge128(lse_part[l], lse_part[64u + l], lse_part[TB + l], lse_part[TB + 64u + l], l, lpM, lpLogZ);
    __syncthreads();
    if (w != 0) return;
    u32 ks[2];
    {
        const u32 s0 = l, s1 = 64u + l, tot = 4u * (u32)n;
        ks[0] = s0 < tot ? surv[s0 / (u32)n * TN + s0 % (u32)n] : 0u;
        ks[1] = s1 < tot ? surv[s1 / (u32)n * TN + s1 % (u32)n] : 0u;
    }
    u32 mine = 0u;
    wave_top_n<2>(ks, n, [&](int j, u32 k) {
        if ((int)l == j) mine = k;
    });
    const int p = pos_io ? pos_io[0] : 0;  // (behind the sampler's increment: the slot of the token it stored)
    if (l == 0) {
        head[0] = lpM;
        head[1] = lpLogZ;
    }
    if ((int)l < n && (u32)p < cap) {
        int id = -1;
        float lp = NINF;
        if (mine) {  // v_tok - lse as (v_tok - M) - log Z: lp_raw's expression
            id = (int)cand[4095u - (mine & 4095u)].y;
            lp = (h2f(unordered_key16(mine >> 12)) - lpM) - lpLogZ;
        }
        top_ids[(size_t)p * (size_t)n + l] = id;
        top_lps[(size_t)p * (size_t)n + l] = lp;
    }
}

}  // namespace

int gq_topn_check(uint32_t vocab, int n, const void *top_ids, const void *top_lps, const void *ws, const void *lse_source) {
    if (int rc = gqs::sample_vocab_ok(vocab)) return rc;
    if (n < 1 || n > GQ_TOPN_MAX) return gq_fail(GQ_EINVAL, "top_n must be in 1..20.");
    if (!top_ids || !top_lps || !ws) return gq_fail(GQ_EINVAL, "top-n: top_ids, top_lps and topn_ws must not be NULL.");
    if ((uintptr_t)ws & 7u) return gq_fail(GQ_EINVAL, "top-n: topn_ws must be 8-byte aligned.");
    if (!lse_source) return gq_fail(GQ_EINVAL, "top-n: lp_raw (and its workspace) must not be NULL -- the list is normalised by lp_raw's log-sum-exp.");
    return GQ_OK;
}

int gq_topn_launch(const void *logits, uint32_t vocab, int n, const float *lse_part, const int *pos_io, int *top_ids, float *top_lps, uint32_t cap,
                   void *ws, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    uint2 *cand = (uint2 *)((unsigned char *)ws + WS_HEAD);
    if (vocab <= 131072u) hipLaunchKernelGGL((topn_stage1<4, 10>), dim3(TB), dim3(TT), 0, s, (const uint16_t *)logits, vocab, n, cand);
    else hipLaunchKernelGGL((topn_stage1<8, 11>), dim3(TB), dim3(TT), 0, s, (const uint16_t *)logits, vocab, n, cand);
    hipLaunchKernelGGL(topn_merge, dim3(1), dim3(TT), 0, s, (const uint2 *)cand, n, lse_part, pos_io, top_ids, top_lps, cap, (float *)ws);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}

extern "C" int gq_sample_topk_lp_topn(const void *logits, uint32_t vocab, int top_k, float top_p, float temperature, uint32_t seed, int *counter,
                                      float *work_val, int *work_idx, int *tok_io, int *pos_io, int *next_tok, const int *ban, int *seq_out,
                                      uint32_t seq_cap, const void *embed_table, void *x_out, uint32_t dim, float *ssq_out, float repetition_penalty,
                                      uint32_t *seen, const uint32_t *suppress, float *lp_ws, float *lp_raw, float *lp_drawn, uint32_t lp_cap,
                                      int top_n, int *top_ids, float *top_lps, void *topn_ws, void *stream) {
    if (int rc = gq_topn_check(vocab, top_n, top_ids, top_lps, topn_ws, lp_raw && lp_ws ? lp_ws : nullptr)) return rc;
    if (int rc = gq_sample_topk_lp(logits, vocab, top_k, top_p, temperature, seed, counter, work_val, work_idx, tok_io, pos_io, next_tok, ban, seq_out,
                                   seq_cap, embed_table, x_out, dim, ssq_out, repetition_penalty, seen, suppress, lp_ws, lp_raw, lp_drawn, lp_cap, stream))
        return rc;
    return gq_topn_launch(logits, vocab, top_n, lp_ws, pos_io, top_ids, top_lps, lp_cap, topn_ws, stream);
}
