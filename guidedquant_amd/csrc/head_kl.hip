// head_kl.hip -- the KL head of the prompt pass: how far the next-token distributions of TWO models with one lm_head are apart, per
// row, in one pass over the vocabulary and without a logit of either reaching global memory (include/gq_hip.h: gq_head_kl).
//   xp      fp16 [S][D]   the rows behind the final RMSNorm of the REFERENCE model (P)
//   xq      fp16 [S][D]   the same rows of the model under TEST (Q)
//   W       fp16 [V][D]   output.weight as stored: one head, both models
// lp[s][v] = fp16(sum_k xp[s][k] W[v][k]) and lq likewise from xq -- gq_head_nll's logit: fp32 accumulation, ONE rounding -- and per row
//   kl = sum_v exp(lp - lse_p) (lp - lq) - lse_p + lse_q,   top1_p / top1_q = the lowest id among the largest logits of each model.
//
// Why one kernel and not two passes of head_nll: the head is bound by the stream of W (1.05 GB at 128256 x 4096) and by the LDS reads of
// its fragments.  Here a block stages a W tile ONCE per K step, beside the two activation tiles, and a wave reads each W fragment from
// LDS ONCE and issues two MFMAs with it -- one against the xp fragment, one against the xq fragment -- so the second model costs matrix
// instructions and 18 KB of LDS, no second stream.  And KL needs both logits of a token in the same lane at the same time, which two
// passes could only have through memory.
//
// The split and the lane layout are head_nll.hip's (head_tile.h holds what the two files agree on): one block of 4 waves per (tile of
// BS = 128 sequence rows, vocabulary range of whole BV = 128-row tiles); the product is transposed, logits^T = W x^T on
// v_mfma_f32_16x16x32_f16, so a sequence row is an accumulator COLUMN (lane l & 15) and lane group g = l >> 4 holds the vocabulary rows
// 16 a + 4 g + r of score block a.  Wave w owns 32 rows (two B fragments per model) against all 128 vocabulary rows (eight A fragments):
// 2 x 16 accumulators = 128 registers, which with the 12 staging registers of a K step, the rounded logits (kept IN the accumulators)
// and the state below stays inside the 512 registers of a block of 4 waves per CU -- head_nll's plain instance is built for one block
// per CU as well, so the 128 x 128 tile stays and W is fetched as rarely per sequence row as there.
// Per lane and column the state is {m_p, s_p, a, m_q, s_q} and the two best (value, id) pairs:
//   s_p = sum exp(lp - m_p),  a = sum exp(lp - m_p) (lp - lq),  s_q = sum exp(lq - m_q)
// over the lane's share of the vocabulary; a and s_p are rescaled by the SAME factor whenever m_p moves.  A column behind V is replaced
// by NEG in both models and adds exactly 0 to all three sums.  The four lane groups of a column are folded once, at the end; each block
// writes one partial of nine words per (row, range) -- a range without a tile writes the neutral element -- and head_kl_merge_kernel folds
// a row's partials in ascending range order: kl = a / s_p - (m_p + log s_p) + (m_q + log s_q), not clamped.  Where xp == xq bit for bit
// every lp - lq is 0, so a is 0, and the two log-sum-exps go through the same instructions on the same bits: kl is exactly 0.0f.
// Rows >= S and vocabulary rows >= V are loaded from the last valid row instead (never stored, masked): nothing outside the arrays is
// read.  No float atomics, no grid barrier, no register array under a run-time index, no integer division in the tile loop.
#include <hip/hip_runtime.h>

#include "gq_internal.h"
#include "wave_util.h"
#include "head_tile.h"

namespace {
using u32 = uint32_t;
using gqw::f32x4;
using gqw::h16;
using gqw::h16x8;
using gqh::BKK, gqh::BS, gqh::BV, gqh::LD, gqh::LOG2E, gqh::MAX_SPLITS, gqh::NEG, gqh::NO_ID;

constexpr u32 NCH = BV * (BKK / 8) / 256;  // 16-byte chunks per thread and matrix
static_assert(BS == BV && NCH == 4, "one chunk map for the three tiles");

// the partials of a (range, row): nine planes [splits][S]
struct KlPartials {
    float *mp, *sp, *a, *mq, *sq, *bvp, *bvq;
    int *bip, *biq;
};

__device__ __forceinline__ float ex(float d) { return __builtin_amdgcn_exp2f(d * LOG2E); }  // exp(d): v_exp_f32, log2(e) in one multiply

// the lowest id among the largest: (ov, oi) replaces (bv, bi) when it is larger, or as large under a lower id
__device__ __forceinline__ void best(float &bv, int &bi, float ov, int oi) {
    if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
}

__global__ void __launch_bounds__(256, 1) head_kl_kernel(const uint16_t *__restrict__ xp, const uint16_t *__restrict__ xq, const uint16_t *__restrict__ W, u32 S,
                                                         u32 V, u32 D, u32 tiles_per_split, KlPartials ws) {
    __shared__ __attribute__((aligned(16))) h16 sW[BV * LD];
    __shared__ __attribute__((aligned(16))) h16 sP[BS * LD];
    __shared__ __attribute__((aligned(16))) h16 sQ[BS * LD];

    const u32 tid = threadIdx.x, w = tid >> 6, l = tid & 63u, g = l >> 4, li = l & 15u;
    const u32 s0 = blockIdx.x * BS, split = blockIdx.y;
    const u32 ntiles = (V + BV - 1u) / BV;  // (once per block)
    const u32 t0 = min(split * tiles_per_split, ntiles), t1 = min(t0 + tiles_per_split, ntiles);

    // the chunks this thread stages: row id >> 3, columns 8 (id & 7) .. + 7 of a step; the same map for W, xp and xq
    u32 xoff[NCH], srow[NCH];
#pragma unroll
    for (u32 i = 0; i < NCH; i++) {
        const u32 id = tid + 256u * i, row = id >> 3, col = id & 7u;
        srow[i] = row * LD + 8u * col;
        xoff[i] = min(s0 + row, S - 1u) * D + 8u * col;  // (S * D < 2^32: checked by the host)
    }

    // one K step ahead in named registers (arrays written under a condition inside the loop nest end up in scratch memory)
    uint4 w0, w1, w2, w3, p0, p1, p2, p3, q0, q1, q2, q3;
#define GQ_KL_LOAD(i_, w_, p_, q_, vt_, kc_)                                                      \
    {                                                                                             \
        const u32 id_ = tid + 256u * (i_), v_ = min((vt_) * BV + (id_ >> 3), V - 1u);             \
        w_ = *reinterpret_cast<const uint4 *>(W + (size_t)v_ * D + (kc_) + 8u * (id_ & 7u));      \
        p_ = *reinterpret_cast<const uint4 *>(xp + xoff[i_] + (kc_));                             \
        q_ = *reinterpret_cast<const uint4 *>(xq + xoff[i_] + (kc_));                             \
    }
#define GQ_KL_LOAD_STEP(vt_, kc_) \
    GQ_KL_LOAD(0, w0, p0, q0, vt_, kc_) GQ_KL_LOAD(1, w1, p1, q1, vt_, kc_) GQ_KL_LOAD(2, w2, p2, q2, vt_, kc_) GQ_KL_LOAD(3, w3, p3, q3, vt_, kc_)
#define GQ_KL_STAGE(i_, w_, p_, q_)                     \
    *reinterpret_cast<uint4 *>(&sW[srow[i_]]) = w_;     \
    *reinterpret_cast<uint4 *>(&sP[srow[i_]]) = p_;     \
    *reinterpret_cast<uint4 *>(&sQ[srow[i_]]) = q_;

    // the wave's two columns per lane: rows s0 + 32 w + 16 b + li
    float mp[2], sp[2], ak[2], mq[2], sq[2], bvp[2], bvq[2];
    int bip[2], biq[2];
#pragma unroll
    for (u32 b = 0; b < 2; b++) {
        mp[b] = NEG, sp[b] = 0.f, ak[b] = 0.f, mq[b] = NEG, sq[b] = 0.f;
        bvp[b] = NEG, bip[b] = NO_ID, bvq[b] = NEG, biq[b] = NO_ID;
    }

    if (t0 < t1) {
        GQ_KL_LOAD_STEP(t0, 0u)
    }
    for (u32 vt = t0; vt < t1; vt++) {
        f32x4 accp[8][2], accq[8][2];
#pragma unroll
        for (u32 a = 0; a < 8; a++)
#pragma unroll
            for (u32 b = 0; b < 2; b++) accp[a][b] = f32x4{0.f, 0.f, 0.f, 0.f}, accq[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

        for (u32 kc = 0; kc < D; kc += BKK) {
            __syncthreads();  // every wave is through with the step in LDS
            GQ_KL_STAGE(0, w0, p0, q0) GQ_KL_STAGE(1, w1, p1, q1) GQ_KL_STAGE(2, w2, p2, q2) GQ_KL_STAGE(3, w3, p3, q3)
            __syncthreads();
            {  // the next step, of this tile or the first of the next one, in flight under the products below
                u32 nk = kc + BKK, nt = vt;
                if (nk == D) nk = 0u, nt = vt + 1u;
                if (nt < t1) {
                    GQ_KL_LOAD_STEP(nt, nk)
                }
            }
#pragma unroll
            for (u32 ks = 0; ks < BKK / 32u; ks++) {
                h16x8 pb[2], qb[2];
#pragma unroll
                for (u32 b = 0; b < 2; b++) {
                    const u32 o = (32u * w + 16u * b + li) * LD + 32u * ks + 8u * g;
                    pb[b] = *reinterpret_cast<const h16x8 *>(&sP[o]);
                    qb[b] = *reinterpret_cast<const h16x8 *>(&sQ[o]);
                }
#pragma unroll
                for (u32 a = 0; a < 8; a++) {  // one read of the W fragment, four products
                    const h16x8 wa = *reinterpret_cast<const h16x8 *>(&sW[(16u * a + li) * LD + 32u * ks + 8u * g]);
#pragma unroll
                    for (u32 b = 0; b < 2; b++) {
                        accp[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa, pb[b], accp[a][b], 0, 0, 0);
                        accq[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa, qb[b], accq[a][b], 0, 0, 0);
                    }
                }
            }
        }

        // the tile's 128 logit pairs of each column.  First sweep: the ONE fp16 rounding of each, written back into the accumulators
        // (NEG behind V), the tile's maxima and the best pairs; second sweep: the three sums against the new maxima.
        const u32 vb = vt * BV + 4u * g;
#pragma unroll
        for (u32 b = 0; b < 2; b++) {
            float mlp = NEG, mlq = NEG;
#pragma unroll
            for (u32 a = 0; a < 8; a++) {
#pragma unroll
                for (u32 r = 0; r < 4; r++) {
                    const u32 v = vb + 16u * a + r;
                    const float lp = v < V ? (float)(h16)accp[a][b][r] : NEG, lq = v < V ? (float)(h16)accq[a][b][r] : NEG;
                    accp[a][b][r] = lp, accq[a][b][r] = lq;
                    mlp = fmaxf(mlp, lp), mlq = fmaxf(mlq, lq);
                    if (lp > bvp[b]) bvp[b] = lp, bip[b] = (int)v;  // ascending v: the lowest id of the largest stays
                    if (lq > bvq[b]) bvq[b] = lq, biq[b] = (int)v;
                }
            }
            const float mnp = fmaxf(mp[b], mlp), mnq = fmaxf(mq[b], mlq);
            float psum = 0.f, asum = 0.f, qsum = 0.f;
#pragma unroll
            for (u32 a = 0; a < 8; a++) {
#pragma unroll
                for (u32 r = 0; r < 4; r++) {
                    const bool in = vb + 16u * a + r < V;
                    const float lp = accp[a][b][r], lq = accq[a][b][r];
                    const float e = ex(lp - mnp);
                    psum += in ? e : 0.f;
                    asum += in ? e * (lp - lq) : 0.f;
                    qsum += in ? ex(lq - mnq) : 0.f;
                }
            }
            const float cp = ex(mp[b] - mnp);  // a and s_p move together
            sp[b] = sp[b] * cp + psum;
            ak[b] = ak[b] * cp + asum;
            sq[b] = sq[b] * ex(mq[b] - mnq) + qsum;
            mp[b] = mnp, mq[b] = mnq;
        }
    }
#undef GQ_KL_LOAD_STEP
#undef GQ_KL_LOAD
#undef GQ_KL_STAGE

    // the four lane groups of a column, then one partial per (row, range)
#pragma unroll
    for (u32 b = 0; b < 2; b++) {
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {
            const float omp = __shfl_xor(mp[b], off, 64), osp = __shfl_xor(sp[b], off, 64), oa = __shfl_xor(ak[b], off, 64);
            const float omq = __shfl_xor(mq[b], off, 64), osq = __shfl_xor(sq[b], off, 64);
            const float ovp = __shfl_xor(bvp[b], off, 64), ovq = __shfl_xor(bvq[b], off, 64);
            const int oip = __shfl_xor(bip[b], off, 64), oiq = __shfl_xor(biq[b], off, 64);
            const float mnp = fmaxf(mp[b], omp), mnq = fmaxf(mq[b], omq);
            const float c0 = ex(mp[b] - mnp), c1 = ex(omp - mnp);
            sp[b] = sp[b] * c0 + osp * c1;
            ak[b] = ak[b] * c0 + oa * c1;
            sq[b] = sq[b] * ex(mq[b] - mnq) + osq * ex(omq - mnq);
            mp[b] = mnp, mq[b] = mnq;
            best(bvp[b], bip[b], ovp, oip);
            best(bvq[b], biq[b], ovq, oiq);
        }
        const u32 row = s0 + 32u * w + 16u * b + li;
        if (g == 0u && row < S) {
            const size_t o = (size_t)split * S + row;
            ws.mp[o] = mp[b], ws.sp[o] = sp[b], ws.a[o] = ak[b];
            ws.mq[o] = mq[b], ws.sq[o] = sq[b];
            ws.bvp[o] = bvp[b], ws.bip[o] = bip[b];
            ws.bvq[o] = bvq[b], ws.biq[o] = biq[b];
        }
    }
}

__global__ void __launch_bounds__(256) head_kl_merge_kernel(KlPartials ws, u32 S, u32 splits, float *__restrict__ kl, float *__restrict__ lse_p,
                                                            float *__restrict__ lse_q, int *__restrict__ top1_p, int *__restrict__ top1_q) {
    const u32 row = blockIdx.x * 256u + threadIdx.x;
    if (row >= S) return;
    float mp = NEG, sp = 0.f, a = 0.f, mq = NEG, sq = 0.f, bvp = NEG, bvq = NEG;
    int bip = NO_ID, biq = NO_ID;
    for (u32 r = 0; r < splits; r++) {  // ascending: one order of the fp32 sums
        const size_t o = (size_t)r * S + row;
        const float omp = ws.mp[o], omq = ws.mq[o], mnp = fmaxf(mp, omp), mnq = fmaxf(mq, omq);
        const float c0 = expf(mp - mnp), c1 = expf(omp - mnp);
        sp = sp * c0 + ws.sp[o] * c1;
        a = a * c0 + ws.a[o] * c1;
        sq = sq * expf(mq - mnq) + ws.sq[o] * expf(omq - mnq);
        mp = mnp, mq = mnq;
        best(bvp, bip, ws.bvp[o], ws.bip[o]);
        best(bvq, biq, ws.bvq[o], ws.biq[o]);
    }
    const float zp = mp + logf(sp), zq = mq + logf(sq);
    kl[row] = (a / sp - zp) + zq;  // (not clamped: 0 - z + z where the two models are one)
    if (lse_p) lse_p[row] = zp;
    if (lse_q) lse_q[row] = zq;
    if (top1_p) top1_p[row] = bip;
    if (top1_q) top1_q[row] = biq;
}
}  // namespace

extern "C" size_t gq_head_kl_ws_bytes(uint32_t S, uint32_t V, uint32_t D, uint32_t splits) {
    (void)D;
    if (S == 0 || V == 0) return 0;
    return (size_t)gqh::pick_splits(S, V, splits) * S * 9u * sizeof(float);
}

extern "C" int gq_head_kl(const void *xp, const void *xq, const void *W, uint32_t S, uint32_t V, uint32_t D, float *kl, float *lse_p, float *lse_q, int *top1_p,
                          int *top1_q, uint32_t splits, void *ws, size_t ws_bytes, void *stream) {
    if (D == 0 || D % 64u != 0) return gq_fail(GQ_ENOTSUP, "gq_head_kl: D must be a multiple of 64.");
    if (S == 0 || V == 0) return gq_fail(GQ_EINVAL, "gq_head_kl: S >= 1 and V >= 1.");
    if (!xp || !xq || !W || !kl || !ws) return gq_fail(GQ_EINVAL, "null pointer argument.");
    if (((uintptr_t)xp | (uintptr_t)xq | (uintptr_t)W) & 15u) return gq_fail(GQ_EINVAL, "gq_head_kl: 16-byte aligned xp, xq and W.");
    if (((uintptr_t)kl | (uintptr_t)lse_p | (uintptr_t)lse_q | (uintptr_t)top1_p | (uintptr_t)top1_q | (uintptr_t)ws) & 3u)
        return gq_fail(GQ_EINVAL, "gq_head_kl: 4-byte aligned outputs and workspace.");
    if (V > 0x7FFFFF00u || (uint64_t)S * D > 0xFFFFFFFFull) return gq_fail(GQ_ENOTSUP, "gq_head_kl: V below 2^31, S * D below 2^32.");
    if (splits > MAX_SPLITS) return gq_fail(GQ_EINVAL, "gq_head_kl: at most 65535 splits.");
    const u32 ns = gqh::pick_splits(S, V, splits);
    const size_t plane = (size_t)ns * S;
    if (ws_bytes < plane * 9u * sizeof(float)) return gq_fail(GQ_EINVAL, "gq_head_kl: workspace smaller than gq_head_kl_ws_bytes.");
    float *f = (float *)ws;
    const KlPartials p = {f, f + plane, f + 2 * plane, f + 3 * plane, f + 4 * plane, f + 5 * plane, f + 6 * plane, (int *)(f + 7 * plane), (int *)(f + 8 * plane)};
    const u32 ntiles = (V + BV - 1u) / BV, tps = (ntiles + ns - 1u) / ns;
    hipLaunchKernelGGL(head_kl_kernel, dim3((S + BS - 1u) / BS, ns), dim3(256), 0, (hipStream_t)stream, (const uint16_t *)xp, (const uint16_t *)xq,
                       (const uint16_t *)W, S, V, D, tps, p);
    GQ_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(head_kl_merge_kernel, dim3((S + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, p, S, ns, kl, lse_p, lse_q, top1_p, top1_q);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}
