// head_nll.hip -- the SCORING head of the prompt pass: lm_head GEMM + log-softmax + gather + argmax in one pass over the vocabulary,
// without the logits ever reaching global memory (include/gq_hip.h: gq_head_nll).
//   xn      fp16 [S][D]   the rows behind the final RMSNorm
//   W       fp16 [V][D]   output.weight as stored
//   target  int  [S]      the token each row is scored on (negative: ignored)
// logit[s][v] = fp16(sum_k xn[s][k] W[v][k]), fp32 accumulation and ONE rounding -- the point at which an fp16 lm_head rounds in front
// of the loss's upcast -- and per row lse = log sum_v exp(logit), logprob = logit[target] - lse, top1 = the lowest id among the largest.
//
// The layout follows prefill_attn.hip.  The product runs on v_mfma_f32_16x16x32_f16 and is TRANSPOSED, logits^T = W xn^T: A = rows of W
// (the vocabulary), B = rows of xn, so the sequence row is the accumulator's column (its lane, l & 15) and lane group g = l >> 4 holds
// the vocabulary rows 16 a + 4 g + r of score block a.  A row's running maximum, sum, target logit and best (value, id) pair live in
// the lanes of its column across every vocabulary tile of the block (each lane keeps the statistics of its own share of the
// vocabulary; the four lane groups are merged once, at the end): the online softmax of the attention kernel with a finite NEG, fp32,
// exp through v_exp_f32 with log2(e) folded into one multiply; a column behind V is REPLACED by NEG and adds exactly 0.
// One block of 4 waves per (tile of BS = 128 sequence rows, vocabulary split); wave w owns 32 rows (two B fragments) against all
// BV = 128 vocabulary rows of a tile (eight A fragments): 16 accumulators.  Tiles of W and xn go through LDS in steps of BKK = 64
// columns, row-major with 16 bytes of padding, the next step's global loads in flight (in registers) under the products.  Rows >= S
// and vocabulary rows >= V are loaded from the last valid row instead (never stored, masked): nothing outside the arrays is read.
// Each block writes one partial {max, sum, target logit, best value, best id} per (row, split); a split without a tile writes the
// neutral element.  head_nll_merge_kernel folds the partials of a row in ascending split order: deterministic.
// The tile loops hold no integer division.
#include <hip/hip_runtime.h>

#include "gq_internal.h"
#include "wave_util.h"

namespace {
using u32 = uint32_t;
using gqw::f32x4;
using gqw::h16;
using gqw::h16x8;

constexpr u32 BS = 128, BV = 128, BKK = 64;
constexpr u32 LD = BKK + 8;          // halves per LDS row: 16 bytes of padding
constexpr u32 NCH = BV * (BKK / 8) / 256;  // 16-byte chunks per thread and matrix
static_assert(BS == BV && NCH == 4, "one chunk map for both tiles");
constexpr float NEG = -1.0e30f;      // below every fp16 value and finite: NEG - NEG = 0, never Inf - Inf
constexpr float LOG2E = 1.4426950408889634f;
constexpr int NO_ID = 0x7FFFFFFF;
constexpr u32 MAX_SPLITS = 65535u;

// the partials of a (split, row): five planes [splits][S]
struct Partials {
    float *m, *sum, *tgt, *bestv;
    int *besti;
};

__device__ __forceinline__ void fold(float &m, float &sum, float &tl, float &bv, int &bi, float om, float os, float ot, float ov, int oi) {
    const float mn = fmaxf(m, om);
    sum = sum * __builtin_amdgcn_exp2f((m - mn) * LOG2E) + os * __builtin_amdgcn_exp2f((om - mn) * LOG2E);
    m = mn;
    tl = fmaxf(tl, ot);
    if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
    }
}

__global__ void __launch_bounds__(256) head_nll_kernel(const uint16_t *__restrict__ xn, const uint16_t *__restrict__ W, const int *__restrict__ target,
                                                       u32 S, u32 V, u32 D, u32 tiles_per_split, Partials ws) {
    __shared__ __attribute__((aligned(16))) h16 sW[BV * LD];
    __shared__ __attribute__((aligned(16))) h16 sX[BS * LD];

    const u32 tid = threadIdx.x, w = tid >> 6, l = tid & 63u, g = l >> 4, li = l & 15u;
    const u32 s0 = blockIdx.x * BS, split = blockIdx.y;
    const u32 ntiles = (V + BV - 1u) / BV;  // (once per block)
    const u32 t0 = min(split * tiles_per_split, ntiles), t1 = min(t0 + tiles_per_split, ntiles);

    // the chunks this thread stages: row id >> 3, columns 8 (id & 7) .. + 7 of a step
    u32 xoff[NCH], srow[NCH];
#pragma unroll
    for (u32 i = 0; i < NCH; i++) {
        const u32 id = tid + 256u * i, row = id >> 3, col = id & 7u;
        srow[i] = row * LD + 8u * col;
        xoff[i] = min(s0 + row, S - 1u) * D + 8u * col;  // (S * D < 2^32: checked by the host)
    }

    // (named registers, not arrays: indexed ones written under a condition inside the loop nest were left in scratch memory)
    uint4 w0, w1, w2, w3, x0, x1, x2, x3;
#define GQ_HEAD_LOAD(i_, w_, x_, vt_, kc_)                                                        \
    {                                                                                             \
        const u32 id_ = tid + 256u * (i_), v_ = min((vt_) * BV + (id_ >> 3), V - 1u);             \
        w_ = *reinterpret_cast<const uint4 *>(W + (size_t)v_ * D + (kc_) + 8u * (id_ & 7u));      \
        x_ = *reinterpret_cast<const uint4 *>(xn + xoff[i_] + (kc_));                             \
    }
#define GQ_HEAD_LOAD_STEP(vt_, kc_) \
    GQ_HEAD_LOAD(0, w0, x0, vt_, kc_) GQ_HEAD_LOAD(1, w1, x1, vt_, kc_) GQ_HEAD_LOAD(2, w2, x2, vt_, kc_) GQ_HEAD_LOAD(3, w3, x3, vt_, kc_)
#define GQ_HEAD_STAGE(i_, w_, x_)                           \
    *reinterpret_cast<uint4 *>(&sW[srow[i_]]) = w_;         \
    *reinterpret_cast<uint4 *>(&sX[srow[i_]]) = x_;

    // the wave's two columns per lane: rows s0 + 32 w + 16 b + li
    int tg[2];
    float m_run[2], l_run[2], t_run[2], bv[2];
    int bi[2];
#pragma unroll
    for (u32 b = 0; b < 2; b++) {
        tg[b] = target[min(s0 + 32u * w + 16u * b + li, S - 1u)];
        // (the target logit's neutral element is -inf, not NEG: a target whose logit IS -inf then scores -inf, not -1e30.  A target that
        // matches no column -- target >= V, the caller's error by the header -- now scores -inf as well, where it scored -1e30 - lse.
        // The fold of the target logit is fmaxf and drops a NaN; a NaN target logit still gives a NaN logprob, through lse: the same
        // NaN logit is in the row's sum.)
        m_run[b] = NEG, l_run[b] = 0.f, t_run[b] = -__builtin_inff(), bv[b] = NEG, bi[b] = NO_ID;
    }

    if (t0 < t1) {
        GQ_HEAD_LOAD_STEP(t0, 0u)
    }
    for (u32 vt = t0; vt < t1; vt++) {
        f32x4 acc[8][2];
#pragma unroll
        for (u32 a = 0; a < 8; a++)
#pragma unroll
            for (u32 b = 0; b < 2; b++) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

        for (u32 kc = 0; kc < D; kc += BKK) {
            __syncthreads();  // every wave is through with the step in LDS
            GQ_HEAD_STAGE(0, w0, x0) GQ_HEAD_STAGE(1, w1, x1) GQ_HEAD_STAGE(2, w2, x2) GQ_HEAD_STAGE(3, w3, x3)
            __syncthreads();
            {  // the next step, of this tile or the first of the next one, in flight under the products below
                u32 nk = kc + BKK, nt = vt;
                if (nk == D) nk = 0u, nt = vt + 1u;
                if (nt < t1) {
                    GQ_HEAD_LOAD_STEP(nt, nk)
                }
            }
#pragma unroll
            for (u32 ks = 0; ks < BKK / 32u; ks++) {
                h16x8 xb[2];
#pragma unroll
                for (u32 b = 0; b < 2; b++) xb[b] = *reinterpret_cast<const h16x8 *>(&sX[(32u * w + 16u * b + li) * LD + 32u * ks + 8u * g]);
#pragma unroll
                for (u32 a = 0; a < 8; a++) {
                    const h16x8 wa = *reinterpret_cast<const h16x8 *>(&sW[(16u * a + li) * LD + 32u * ks + 8u * g]);
#pragma unroll
                    for (u32 b = 0; b < 2; b++) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa, xb[b], acc[a][b], 0, 0, 0);
                }
            }
        }

        // the tile's 128 logits of each column: rounded to fp16 once, then the online softmax, the target and the best pair
        const u32 vb = vt * BV + 4u * g;
#pragma unroll
        for (u32 b = 0; b < 2; b++) {
            float x[8][4];
            float mloc = NEG;
#pragma unroll
            for (u32 a = 0; a < 8; a++) {
#pragma unroll
                for (u32 r = 0; r < 4; r++) {
                    const u32 v = vb + 16u * a + r;
                    const float lg = (float)(h16)acc[a][b][r];
                    x[a][r] = v < V ? lg : NEG;
                    mloc = fmaxf(mloc, x[a][r]);
                    if ((int)v == tg[b]) t_run[b] = x[a][r];  // (a negative target matches no column; v < V <= 2^31 - 1)
                    if (x[a][r] > bv[b]) bv[b] = x[a][r], bi[b] = (int)v;  // ascending v: the lowest id of the largest stays
                }
            }
            const float m_new = fmaxf(m_run[b], mloc);
            float psum = 0.f;
#pragma unroll
            for (u32 a = 0; a < 8; a++) {
#pragma unroll
                for (u32 r = 0; r < 4; r++) {
                    const u32 v = vb + 16u * a + r;
                    psum += v < V ? __builtin_amdgcn_exp2f((x[a][r] - m_new) * LOG2E) : 0.f;
                }
            }
            l_run[b] = l_run[b] * __builtin_amdgcn_exp2f((m_run[b] - m_new) * LOG2E) + psum;
            m_run[b] = m_new;
        }
    }

#undef GQ_HEAD_LOAD_STEP
#undef GQ_HEAD_LOAD
#undef GQ_HEAD_STAGE
    // the four lane groups of a column, then one partial per (row, split)
#pragma unroll
    for (u32 b = 0; b < 2; b++) {
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {
            const float om = __shfl_xor(m_run[b], off, 64), os = __shfl_xor(l_run[b], off, 64), ot = __shfl_xor(t_run[b], off, 64);
            const float ov = __shfl_xor(bv[b], off, 64);
            const int oi = __shfl_xor(bi[b], off, 64);
            fold(m_run[b], l_run[b], t_run[b], bv[b], bi[b], om, os, ot, ov, oi);
        }
        const u32 row = s0 + 32u * w + 16u * b + li;
        if (g == 0u && row < S) {
            const size_t o = (size_t)split * S + row;
            ws.m[o] = m_run[b];
            ws.sum[o] = l_run[b];
            ws.tgt[o] = t_run[b];
            ws.bestv[o] = bv[b];
            ws.besti[o] = bi[b];
        }
    }
}

__global__ void __launch_bounds__(256) head_nll_merge_kernel(Partials ws, const int *__restrict__ target, u32 S, u32 splits, float *__restrict__ logprob,
                                                             float *__restrict__ lse, int *__restrict__ top1) {
    const u32 row = blockIdx.x * 256u + threadIdx.x;
    if (row >= S) return;
    float m = NEG, sum = 0.f, tl = -__builtin_inff(), bv = NEG;
    int bi = NO_ID;
    for (u32 sp = 0; sp < splits; sp++) {  // ascending: one order of the fp32 sums
        const size_t o = (size_t)sp * S + row;
        const float om = ws.m[o], mn = fmaxf(m, om);
        sum = sum * expf(m - mn) + ws.sum[o] * expf(om - mn);
        m = mn;
        tl = fmaxf(tl, ws.tgt[o]);
        const float ov = ws.bestv[o];
        const int oi = ws.besti[o];
        if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
    }
    const float z = m + logf(sum);
    logprob[row] = target[row] < 0 ? 0.0f : tl - z;
    if (lse) lse[row] = z;
    if (top1) top1[row] = bi;
}

// the vocabulary splits of a launch: the caller's, or enough blocks for two per compute unit with at least 8 tiles each
u32 pick_splits(u32 S, u32 V, u32 splits) {
    if (splits) return splits;
    const u32 row_tiles = (S + BS - 1u) / BS, ntiles = (V + BV - 1u) / BV;
    const u32 want = (2u * (u32)gq_cu_count() + row_tiles - 1u) / row_tiles;
    return max(1u, min(min(want, ntiles / 8u), MAX_SPLITS));
}
}  // namespace

extern "C" size_t gq_head_nll_ws_bytes(uint32_t S, uint32_t V, uint32_t D, uint32_t splits) {
    (void)D;
    if (S == 0 || V == 0) return 0;
    return (size_t)pick_splits(S, V, splits) * S * 5u * sizeof(float);
}

extern "C" int gq_head_nll(const void *xn, const void *W, const int *target, uint32_t S, uint32_t V, uint32_t D, float *logprob, float *lse, int *top1,
                           uint32_t splits, void *ws, size_t ws_bytes, void *stream) {
    if (D == 0 || D % 64u != 0) return gq_fail(GQ_ENOTSUP, "gq_head_nll: D must be a multiple of 64.");
    if (S == 0 || V == 0) return gq_fail(GQ_EINVAL, "gq_head_nll: S >= 1 and V >= 1.");
    if (!xn || !W || !target || !logprob || !ws) return gq_fail(GQ_EINVAL, "null pointer argument.");
    if (((uintptr_t)xn | (uintptr_t)W) & 15u) return gq_fail(GQ_EINVAL, "gq_head_nll: 16-byte aligned xn and W.");
    if (((uintptr_t)target | (uintptr_t)logprob | (uintptr_t)lse | (uintptr_t)top1 | (uintptr_t)ws) & 3u)
        return gq_fail(GQ_EINVAL, "gq_head_nll: 4-byte aligned target, outputs and workspace.");
    if (V > 0x7FFFFF00u || (uint64_t)S * D > 0xFFFFFFFFull) return gq_fail(GQ_ENOTSUP, "gq_head_nll: V below 2^31, S * D below 2^32.");
    if (splits > MAX_SPLITS) return gq_fail(GQ_EINVAL, "gq_head_nll: at most 65535 splits.");
    const u32 ns = pick_splits(S, V, splits);
    const size_t plane = (size_t)ns * S;
    if (ws_bytes < plane * 5u * sizeof(float)) return gq_fail(GQ_EINVAL, "gq_head_nll: workspace smaller than gq_head_nll_ws_bytes.");
    float *f = (float *)ws;
    const Partials p = {f, f + plane, f + 2 * plane, f + 3 * plane, (int *)(f + 4 * plane)};
    const u32 ntiles = (V + BV - 1u) / BV, tps = (ntiles + ns - 1u) / ns;
    hipLaunchKernelGGL(head_nll_kernel, dim3((S + BS - 1u) / BS, ns), dim3(256), 0, (hipStream_t)stream, (const uint16_t *)xn, (const uint16_t *)W, target, S,
                       V, D, tps, p);
    GQ_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(head_nll_merge_kernel, dim3((S + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, p, target, S, ns, logprob, lse, top1);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}
