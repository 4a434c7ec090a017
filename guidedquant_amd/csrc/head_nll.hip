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
//
// gq_head_nll_topn is the same pass with the n <= 20 best (fp16 logit, id) pairs of every row next to it: head_nll_kernel<true>.
//   * where the lists live: a row's n best so far, sorted (value descending, id ascending), in LDS -- 128 rows x 20 x {float, int} =
//     20 KB beside sW / sX, and only the rows of the wave that owns them: no barrier guards them.  Every lane keeps its row's n-th pair
//     (the threshold) in two registers.
//   * per tile a lane compares its 2 x 32 fresh logits with the threshold: a 4-bit mask per score block a, one ballot per mask.  Only
//     where a ballot is not empty does the wave leave the fast path, and then it inserts the candidates ONE AT A TIME, wave-uniformly:
//     the candidate goes to scalar registers (v_readlane from its lane), lane j reads entry j of the row's list, a ballot of "entry j
//     stays in front" counts the position, the lanes behind it move their entry down one slot, and the row's four lanes take the new
//     threshold.  A candidate that an earlier insert of the same tile has overtaken finds position n and writes nothing.  An insert is
//     rare behind a split's first tiles -- about n ln(tiles x 128 / n) per row and split -- so it is allowed to be serial.
//     The order is total on (value, id), so a list does not depend on the order of the inserts.  A NaN compares false and never enters;
//     a column >= V is masked; an empty slot is (-inf, NO_ID), which every token -- a -inf logit included -- overtakes.
//   * per (row, split) the block writes its list behind the five planes; head_nll_merge_kernel runs UNCHANGED on the five planes, and
//     head_nll_topn_merge_kernel (one wave per row) folds the lists in ascending split order: each lane ranks its entry of the merged
//     list and of the split's list among the 2 n by counting (v_readlane over the other list), the first n go through LDS to their
//     rank, and lane j stores id_j and fp32(logit_j) - lse -- the subtraction logprob is made by, against the same lse.
// No float atomics, no register array under a run-time index, no integer division in the tile loop.
//
// gq_head_nll_i8 / gq_head_nll_i8_topn score the int8 lm_head of the decode step (W8A16: head_q8.hip's model) through the SAME kernel
// text, head_nll_kernel<TOPN, true>: logit = fp16(fl32(scale[v] * sum_k xn[s][k] q[v][k])).  Only the operand path and one multiply differ:
//   * a step's W tile is 128 rows x 64 BYTES: two 16-byte loads per thread (row id >> 2, 16 codes each) where the fp16 tile takes four,
//     one step ahead in two named registers, like the fp16 loads;
//   * between the load and the LDS store every code becomes the fp16 integer it is (q8_conv.h: xor, two v_perm_b32, v_pk_add_f16 -- once
//     per block and element), so sW holds fp16 numbers and the LDS reads and the MFMA loop are the fp16 instance's.  The products of
//     fp16 integers with fp16 activations are exact in the fp32 accumulator's multiplier, as in the decode GEMV;
//   * the tile's 128 fp32 scales (scale[min(v, V - 1)]) are requested with the tile's first step by threads 0..127, stored to LDS with it
//     (512 bytes) and read as one float4 per score block in the epilogue: no scale lives in a register across the K loop.  The
//     accumulators are multiplied in place, in fp32, in front of the ONE fp16 rounding; the top-n candidates and the softmax then read
//     the same rounded logits, and everything behind them -- lists, partials, both merge kernels, the splits rule -- is shared.
// The int8 MFMA is not used: it would want int8 activations, another model than the decode step's.
#include <hip/hip_runtime.h>

#include "gq_internal.h"
#include "wave_util.h"
#include "q8_conv.h"
#include "head_tile.h"

namespace {
using u32 = uint32_t;
using gqw::f32x4;
using gqw::h16;
using gqw::h16x8;

using gqh::BKK, gqh::BS, gqh::BV, gqh::LD, gqh::LOG2E, gqh::MAX_SPLITS, gqh::NEG, gqh::NO_ID;  // (head_tile.h: shared with head_kl.hip)
using gqh::pick_splits;
constexpr u32 NCH = BV * (BKK / 8) / 256;  // 16-byte chunks per thread and matrix
static_assert(BS == BV && NCH == 4, "one chunk map for both tiles");
constexpr u32 TN = 20;              // list slots per row (GQ_TOPN_MAX of include/gq_hip.h)
static_assert(TN == GQ_TOPN_MAX, "the list stride is the largest top_n");

// the partials of a (split, row): five planes [splits][S]
struct Partials {
    float *m, *sum, *tgt, *bestv;
    int *besti;
};

// the top-n instance's lists: planes [splits][S][n] behind the partials (nothing in the plain instance)
template <bool TOPN>
struct Lists {};
template <>
struct Lists<true> {
    u32 n;
    float *val;
    int *id;
};

// the int8 instances' fp32 scale per vocabulary row [V] (nothing in the fp16 instances)
template <bool Q8>
struct RowScale {};
template <>
struct RowScale<true> {
    const float *scale;
};

// (value, id) a in front of (value, id) b: the order of every list
__device__ __forceinline__ bool in_front(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }
__device__ __forceinline__ float lane_f(float x, u32 lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), (int)lane)); }
__device__ __forceinline__ int lane_i(int x, u32 lane) { return __builtin_amdgcn_readlane(x, (int)lane); }

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

// (two blocks per CU for the top-n instance by request: left to itself the compiler took 308 registers for it, one block per CU; the
// plain instance keeps the bounds, and the code, it always had)
// Q8: W is the int8 head, BV x BKK BYTES per step (two 16-byte loads per thread: row id >> 2, columns 16 (id & 3) .. + 15), turned into
// fp16 integers between the load and the LDS store; q8.scale rides through LDS beside the tile and meets the accumulators once per tile.
template <bool TOPN, bool Q8>
__global__ void __launch_bounds__(256, TOPN ? 2 : 1) head_nll_kernel(const uint16_t *__restrict__ xn, const uint16_t *__restrict__ W, const int *__restrict__ target,
                                                       u32 S, u32 V, u32 D, u32 tiles_per_split, Partials ws, Lists<TOPN> top, RowScale<Q8> q8) {
    __shared__ __attribute__((aligned(16))) h16 sW[BV * LD];
    __shared__ __attribute__((aligned(16))) h16 sX[BS * LD];
    __shared__ uint2 sL[TOPN ? BS * TN : 1];  // {value bits, id} [row][slot]; rows 32 w .. 32 w + 31 are wave w's alone
    __shared__ __attribute__((aligned(16))) float sS[Q8 ? BV : 4];  // the tile's row scales (the int8 instances)

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
    // the int8 step: 16 codes per load (w0, w1), the four xn chunks as above, and with a tile's first step its 128 scales (sc, tid < BV)
    float sc = 0.f;
#define GQ_HEAD_LOADQ(i_, w_, vt_, kc_)                                                                                                  \
    {                                                                                                                                    \
        const u32 id_ = tid + 256u * (i_), v_ = min((vt_) * BV + (id_ >> 2), V - 1u);                                                    \
        w_ = *reinterpret_cast<const uint4 *>(reinterpret_cast<const uint8_t *>(W) + (size_t)v_ * D + (kc_) + 16u * (id_ & 3u));         \
    }
#define GQ_HEAD_LOADX(i_, x_, kc_) x_ = *reinterpret_cast<const uint4 *>(xn + xoff[i_] + (kc_));
#define GQ_HEAD_LOAD_STEP(vt_, kc_)                                                                                                          \
    if constexpr (Q8) {                                                                                                                      \
        GQ_HEAD_LOADQ(0, w0, vt_, kc_) GQ_HEAD_LOADQ(1, w1, vt_, kc_)                                                                        \
        GQ_HEAD_LOADX(0, x0, kc_) GQ_HEAD_LOADX(1, x1, kc_) GQ_HEAD_LOADX(2, x2, kc_) GQ_HEAD_LOADX(3, x3, kc_)                              \
        if ((kc_) == 0u && tid < BV) sc = q8.scale[min((vt_) * BV + tid, V - 1u)];                                                           \
    } else {                                                                                                                                 \
        GQ_HEAD_LOAD(0, w0, x0, vt_, kc_) GQ_HEAD_LOAD(1, w1, x1, vt_, kc_) GQ_HEAD_LOAD(2, w2, x2, vt_, kc_) GQ_HEAD_LOAD(3, w3, x3, vt_, kc_) \
    }
#define GQ_HEAD_STAGE(i_, w_, x_)                           \
    *reinterpret_cast<uint4 *>(&sW[srow[i_]]) = w_;         \
    *reinterpret_cast<uint4 *>(&sX[srow[i_]]) = x_;
#define GQ_HEAD_STAGEQ(i_, w_)                                                           \
    {                                                                                    \
        const u32 id_ = tid + 256u * (i_), o_ = (id_ >> 2) * LD + 16u * (id_ & 3u);      \
        uint4 lo_, hi_;                                                                  \
        gqw::q8_row16(w_, lo_, hi_);                                                     \
        *reinterpret_cast<uint4 *>(&sW[o_]) = lo_;                                       \
        *reinterpret_cast<uint4 *>(&sW[o_ + 8u]) = hi_;                                  \
    }
#define GQ_HEAD_STAGEX(i_, x_) *reinterpret_cast<uint4 *>(&sX[srow[i_]]) = x_;

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
    // the threshold of the lane's two rows: the n-th pair of the list
    float tv[2] = {-__builtin_inff(), -__builtin_inff()};
    int ti[2] = {NO_ID, NO_ID};
    if constexpr (TOPN) {
        for (u32 i = l; i < 32u * TN; i += 64u) sL[32u * w * TN + i] = make_uint2((u32)__float_as_int(-__builtin_inff()), (u32)NO_ID);
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
            if constexpr (Q8) {  // (the barrier above is also behind the previous tile's epilogue, the last reader of sS)
                GQ_HEAD_STAGEQ(0, w0) GQ_HEAD_STAGEQ(1, w1)
                GQ_HEAD_STAGEX(0, x0) GQ_HEAD_STAGEX(1, x1) GQ_HEAD_STAGEX(2, x2) GQ_HEAD_STAGEX(3, x3)
                if (kc == 0u && tid < BV) sS[tid] = sc;
            } else {
                GQ_HEAD_STAGE(0, w0, x0) GQ_HEAD_STAGE(1, w1, x1) GQ_HEAD_STAGE(2, w2, x2) GQ_HEAD_STAGE(3, w3, x3)
            }
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
        if constexpr (Q8) {  // scale[v] * acc in fp32, in place: the ONE fp16 rounding below is then the model's (include/gq_hip.h)
#pragma unroll
            for (u32 a = 0; a < 8; a++) {
                const float4 s4 = *reinterpret_cast<const float4 *>(&sS[16u * a + 4u * g]);
#pragma unroll
                for (u32 b = 0; b < 2; b++) {
                    acc[a][b][0] *= s4.x, acc[a][b][1] *= s4.y, acc[a][b][2] *= s4.z, acc[a][b][3] *= s4.w;
                }
            }
        }
        if constexpr (TOPN) {  // (from the accumulators, in front of the softmax, four logits at a time)
#pragma unroll
            for (u32 b = 0; b < 2; b++) {
#pragma unroll
                for (u32 a = 0; a < 8; a++) {
                    float x4[4];
                    u32 pm = 0u;  // the lane's logits of score block a in front of its row's threshold
#pragma unroll
                    for (u32 r = 0; r < 4; r++) {
                        const u32 v = vb + 16u * a + r;
                        x4[r] = (float)(h16)acc[a][b][r];
                        pm |= (v < V && in_front(x4[r], (int)v, tv[b], ti[b])) ? (1u << r) : 0u;
                    }
                    for (unsigned long long bal = __ballot(pm != 0u); bal != 0ull; bal = __ballot(pm != 0u)) {
                        const u32 cl = (u32)__builtin_amdgcn_readfirstlane((int)__builtin_ctzll(bal));  // the candidate's lane
                        const u32 r = (u32)__builtin_ctz(pm | 16u);
                        const float mine = r == 0u ? x4[0] : r == 1u ? x4[1] : r == 2u ? x4[2] : x4[3];
                        const float cv = lane_f(mine, cl);
                        const int ci = (int)(vt * BV + 16u * a + 4u * (cl >> 4) + (u32)lane_i((int)r, cl));
                        const u32 base = (32u * w + 16u * b + (cl & 15u)) * TN;
                        const uint2 e = sL[base + min(l, top.n - 1u)];
                        const float ev = __int_as_float((int)e.x);
                        const u32 pos = (u32)__popcll(__ballot(l < top.n && in_front(ev, (int)e.y, cv, ci)));  // (sorted: a prefix)
                        if (pos < top.n) {
                            if (l >= pos && l + 1u < top.n) sL[base + l + 1u] = e;
                            if (l == pos) sL[base + pos] = make_uint2((u32)__float_as_int(cv), (u32)ci);
                            // the row's new n-th pair: the candidate, or what stood at n - 2
                            const u32 src = top.n >= 2u ? top.n - 2u : 0u;
                            const float nv = pos + 1u == top.n ? cv : lane_f(ev, src);
                            const int ni = pos + 1u == top.n ? ci : lane_i((int)e.y, src);
                            if (li == (cl & 15u)) tv[b] = nv, ti[b] = ni;
                        }
                        if (l == cl) pm &= pm - 1u;
                    }
                }
            }
        }
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
#undef GQ_HEAD_LOADQ
#undef GQ_HEAD_LOADX
#undef GQ_HEAD_STAGEQ
#undef GQ_HEAD_STAGEX
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
    if constexpr (TOPN) {
        for (u32 rr = 0; rr < 32u; rr++) {
            const u32 row = s0 + 32u * w + rr;
            if (row < S && l < top.n) {
                const uint2 e = sL[(32u * w + rr) * TN + l];
                const size_t o = ((size_t)split * S + row) * top.n + l;
                top.val[o] = __int_as_float((int)e.x);
                top.id[o] = (int)e.y;
            }
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

// One wave per row.  Lane j < n holds entry j of the merged list (m) and of the next split's (s); both are sorted and, but for empty
// slots, hold different ids.  rank(m_j) = j + #{s in front of m_j}, rank(s_j) = j + #{m not behind s_j}: a permutation of 0 .. 2 n - 1
// (equal pairs -- empty slots -- keep m first), and ranks below n are the new list.
__global__ void __launch_bounds__(256) head_nll_topn_merge_kernel(const float *__restrict__ val, const int *__restrict__ id, u32 S, u32 splits, u32 n,
                                                                  const float *__restrict__ lse, int *__restrict__ top_ids, float *__restrict__ top_lps) {
    __shared__ uint2 sm[4][TN];
    const u32 w = threadIdx.x >> 6, l = threadIdx.x & 63u, row = blockIdx.x * 4u + w;
    if (row >= S) return;  // (a whole wave; the kernel has no block barrier)
    float mv = -__builtin_inff();
    int mi = NO_ID;
    for (u32 sp = 0; sp < splits; sp++) {
        const size_t o = ((size_t)sp * S + row) * n + l;
        const float sv = l < n ? val[o] : -__builtin_inff();
        const int si = l < n ? id[o] : NO_ID;
        u32 rm = l, rs = l;
        for (u32 k = 0; k < n; k++) {
            rm += in_front(lane_f(sv, k), lane_i(si, k), mv, mi) ? 1u : 0u;
            rs += in_front(sv, si, lane_f(mv, k), lane_i(mi, k)) ? 0u : 1u;
        }
        if (l < n && rm < n) sm[w][rm] = make_uint2((u32)__float_as_int(mv), (u32)mi);
        if (l < n && rs < n) sm[w][rs] = make_uint2((u32)__float_as_int(sv), (u32)si);
        __builtin_amdgcn_wave_barrier();
        if (l < n) {
            const uint2 e = sm[w][l];
            mv = __int_as_float((int)e.x), mi = (int)e.y;
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (l < n) {
        const size_t o = (size_t)row * n + l;
        top_ids[o] = mi == NO_ID ? -1 : mi;
        top_lps[o] = mi == NO_ID ? -__builtin_inff() : mv - lse[row];
    }
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
    hipLaunchKernelGGL((head_nll_kernel<false, false>), dim3((S + BS - 1u) / BS, ns), dim3(256), 0, (hipStream_t)stream, (const uint16_t *)xn,
                       (const uint16_t *)W, target, S, V, D, tps, p, Lists<false>{}, RowScale<false>{});
    GQ_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(head_nll_merge_kernel, dim3((S + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, p, target, S, ns, logprob, lse, top1);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}

// the workspace of the top-n form: the five planes, a row of lse (for a caller that asks for none), then the lists' two planes
extern "C" size_t gq_head_nll_topn_ws_bytes(uint32_t S, uint32_t V, uint32_t D, uint32_t splits, int top_n) {
    (void)D;
    if (S == 0 || V == 0 || top_n < 1 || top_n > (int)TN) return 0;
    const size_t plane = (size_t)pick_splits(S, V, splits) * S;
    return (plane * 5u + S + plane * (size_t)top_n * 2u) * sizeof(float);
}

extern "C" int gq_head_nll_topn(const void *xn, const void *W, const int *target, uint32_t S, uint32_t V, uint32_t D, float *logprob, float *lse, int *top1,
                                int top_n, int *top_ids, float *top_lps, uint32_t splits, void *ws, size_t ws_bytes, void *stream) {
    if (top_n < 1 || top_n > (int)TN) return gq_fail(GQ_EINVAL, "gq_head_nll_topn: top_n must be in 1..20.");
    if (D == 0 || D % 64u != 0) return gq_fail(GQ_ENOTSUP, "gq_head_nll_topn: D must be a multiple of 64.");
    if (S == 0 || V == 0) return gq_fail(GQ_EINVAL, "gq_head_nll_topn: S >= 1 and V >= 1.");
    if (!xn || !W || !target || !logprob || !top_ids || !top_lps || !ws) return gq_fail(GQ_EINVAL, "null pointer argument.");
    if (((uintptr_t)xn | (uintptr_t)W) & 15u) return gq_fail(GQ_EINVAL, "gq_head_nll_topn: 16-byte aligned xn and W.");
    if (((uintptr_t)target | (uintptr_t)logprob | (uintptr_t)lse | (uintptr_t)top1 | (uintptr_t)top_ids | (uintptr_t)top_lps | (uintptr_t)ws) & 3u)
        return gq_fail(GQ_EINVAL, "gq_head_nll_topn: 4-byte aligned target, outputs and workspace.");
    if (V > 0x7FFFFF00u || (uint64_t)S * D > 0xFFFFFFFFull) return gq_fail(GQ_ENOTSUP, "gq_head_nll_topn: V below 2^31, S * D below 2^32.");
    if (splits > MAX_SPLITS) return gq_fail(GQ_EINVAL, "gq_head_nll_topn: at most 65535 splits.");
    const u32 ns = pick_splits(S, V, splits), n = (u32)top_n;
    const size_t plane = (size_t)ns * S;
    if (ws_bytes < (plane * 5u + S + plane * n * 2u) * sizeof(float))
        return gq_fail(GQ_EINVAL, "gq_head_nll_topn: workspace smaller than gq_head_nll_topn_ws_bytes.");
    float *f = (float *)ws;
    const Partials p = {f, f + plane, f + 2 * plane, f + 3 * plane, (int *)(f + 4 * plane)};
    float *z = lse ? lse : f + 5 * plane;
    const Lists<true> lists = {n, f + 5 * plane + S, (int *)(f + 5 * plane + S + plane * n)};
    const u32 ntiles = (V + BV - 1u) / BV, tps = (ntiles + ns - 1u) / ns;
    hipLaunchKernelGGL((head_nll_kernel<true, false>), dim3((S + BS - 1u) / BS, ns), dim3(256), 0, (hipStream_t)stream, (const uint16_t *)xn,
                       (const uint16_t *)W, target, S, V, D, tps, p, lists, RowScale<false>{});
    GQ_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(head_nll_merge_kernel, dim3((S + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, p, target, S, ns, logprob, z, top1);
    GQ_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(head_nll_topn_merge_kernel, dim3((S + 3u) / 4u), dim3(256), 0, (hipStream_t)stream, (const float *)lists.val, (const int *)lists.id, S,
                       ns, n, (const float *)z, top_ids, top_lps);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}

// the int8 head: both entries, top_n == 0 the plain one.  The checks, the workspaces and the launches behind the pass are the fp16 entries'.
static int head_nll_i8(const void *xn, const void *Wq, const float *scale, const int *target, u32 S, u32 V, u32 D, float *logprob, float *lse, int *top1,
                       int top_n, int *top_ids, float *top_lps, u32 splits, void *ws, size_t ws_bytes, void *stream) {
    if (D == 0 || D % 64u != 0) return gq_fail(GQ_ENOTSUP, "gq_head_nll_i8: D must be a multiple of 64.");
    if (S == 0 || V == 0) return gq_fail(GQ_EINVAL, "gq_head_nll_i8: S >= 1 and V >= 1.");
    if (!xn || !Wq || !scale || !target || !logprob || !ws || (top_n && (!top_ids || !top_lps))) return gq_fail(GQ_EINVAL, "null pointer argument.");
    if (((uintptr_t)xn | (uintptr_t)Wq) & 15u) return gq_fail(GQ_EINVAL, "gq_head_nll_i8: 16-byte aligned xn and Wq.");
    if (((uintptr_t)scale | (uintptr_t)target | (uintptr_t)logprob | (uintptr_t)lse | (uintptr_t)top1 | (uintptr_t)top_ids | (uintptr_t)top_lps | (uintptr_t)ws) & 3u)
        return gq_fail(GQ_EINVAL, "gq_head_nll_i8: 4-byte aligned scale, target, outputs and workspace.");
    if (V > 0x7FFFFF00u || (uint64_t)S * D > 0xFFFFFFFFull) return gq_fail(GQ_ENOTSUP, "gq_head_nll_i8: V below 2^31, S * D below 2^32.");
    if (splits > MAX_SPLITS) return gq_fail(GQ_EINVAL, "gq_head_nll_i8: at most 65535 splits.");
    const u32 ns = pick_splits(S, V, splits), n = (u32)top_n;
    const size_t plane = (size_t)ns * S;
    if (ws_bytes < (plane * 5u + (n ? S + plane * n * 2u : 0u)) * sizeof(float))
        return gq_fail(GQ_EINVAL, "gq_head_nll_i8: workspace smaller than gq_head_nll_ws_bytes / gq_head_nll_topn_ws_bytes.");
    float *f = (float *)ws;
    const Partials p = {f, f + plane, f + 2 * plane, f + 3 * plane, (int *)(f + 4 * plane)};
    float *z = (lse || !n) ? lse : f + 5 * plane;
    const Lists<true> lists = {n, f + 5 * plane + S, (int *)(f + 5 * plane + S + plane * n)};
    const u32 ntiles = (V + BV - 1u) / BV, tps = (ntiles + ns - 1u) / ns;
    const dim3 grid((S + BS - 1u) / BS, ns);
    if (n)
        hipLaunchKernelGGL((head_nll_kernel<true, true>), grid, dim3(256), 0, (hipStream_t)stream, (const uint16_t *)xn, (const uint16_t *)Wq, target, S, V, D,
                           tps, p, lists, RowScale<true>{scale});
    else
        hipLaunchKernelGGL((head_nll_kernel<false, true>), grid, dim3(256), 0, (hipStream_t)stream, (const uint16_t *)xn, (const uint16_t *)Wq, target, S, V, D,
                           tps, p, Lists<false>{}, RowScale<true>{scale});
    GQ_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(head_nll_merge_kernel, dim3((S + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, p, target, S, ns, logprob, z, top1);
    GQ_HIP_CHECK(hipGetLastError());
    if (n) {
        hipLaunchKernelGGL(head_nll_topn_merge_kernel, dim3((S + 3u) / 4u), dim3(256), 0, (hipStream_t)stream, (const float *)lists.val, (const int *)lists.id,
                           S, ns, n, (const float *)z, top_ids, top_lps);
        GQ_HIP_CHECK(hipGetLastError());
    }
    return GQ_OK;
}

extern "C" int gq_head_nll_i8(const void *xn, const void *Wq, const float *scale, const int *target, uint32_t S, uint32_t V, uint32_t D, float *logprob,
                              float *lse, int *top1, uint32_t splits, void *ws, size_t ws_bytes, void *stream) {
    return head_nll_i8(xn, Wq, scale, target, S, V, D, logprob, lse, top1, 0, nullptr, nullptr, splits, ws, ws_bytes, stream);
}

extern "C" int gq_head_nll_i8_topn(const void *xn, const void *Wq, const float *scale, const int *target, uint32_t S, uint32_t V, uint32_t D, float *logprob,
                                   float *lse, int *top1, int top_n, int *top_ids, float *top_lps, uint32_t splits, void *ws, size_t ws_bytes,
                                   void *stream) {
    if (top_n < 1 || top_n > (int)TN) return gq_fail(GQ_EINVAL, "gq_head_nll_i8_topn: top_n must be in 1..20.");
    return head_nll_i8(xn, Wq, scale, target, S, V, D, logprob, lse, top1, top_n, top_ids, top_lps, splits, ws, ws_bytes, stream);
}
