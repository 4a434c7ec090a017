// attn_core.h -- what the decode attention kernels share, each stated once: the split geometry, the arithmetic of one cached row and of
// one online-softmax step, the hand-over of the position streams through LDS with its merge, and the LDS layouts.  Users:
// attn_decode_kernel, attn_roped_kernel and attn_combine_kernel (decode.hip) and the head blocks of the wqkv launch
// (ap_stream.hip::fuse_attn_head).  Their outputs are pinned bit for bit against each other and against tests/attn_probes.py, which
// mirrors the geometry below: a change here reaches every kernel at once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gq_internal.h"
#include "wave_util.h"

namespace gq_attn {
typedef uint32_t u32;
using gqw::row_sum;  // the score of a cached row: the sum over the LPP lanes that share it, in every one of them

// ------------------------------------------------------------------------------------------------ geometry
// A block has NW waves.  LPP lanes share a cached row (8 dims = one 16-byte load per lane: a K / V row is one coalesced line pair),
// PPW rows per wave instruction, U independent rows in flight per lane group.  The lane group (wave, sub) is a position STREAM with
// its own running (max, sum, weighted V); the NS streams of a block cover PASS consecutive rows per pass.
template <int HD>
struct AttnGeom {
    static constexpr u32 NW = GQ_ATTN_WAVES;  // 8 waves x 4 rows x 4 in flight = 128 rows per pass (HD = 128)
    static constexpr int LPP = HD / 8;        // 16 (HD = 128) or 8 (HD = 64)
    static constexpr int PPW = 64 / LPP;
    static constexpr int U = 4;
    static constexpr u32 NS = NW * PPW;
    static constexpr u32 PASS = NS * U;
};

// WIN (sliding-window layers: transformers' masking_utils.sliding_window_overlay on top of the causal mask): the query at position pos
// attends the cached rows (pos - W, pos] -- lo = max(0, pos + 1 - W), n = pos + 1 - lo rows.  The geometry of a launch is that of the
// launch without a window at position n - 1, shifted by lo: the solo rule and the split length are taken from n, split s covers
// [lo + s per, ..), row t takes the (pass, wave, u, sub) slot row t - lo has there; merge and combine order as they are.  No row below lo
// is requested behind the position read (they hold real rows of the sequence).  A compile-time form: the WIN = false instances take an
// empty argument and keep the instructions they had.  W >= 1 (checked by the host), so lo <= pos: nothing underflows.
template <bool WIN>
struct AttnWindow {};  // (nothing to pass)
template <>
struct AttnWindow<true> {
    u32 w;  // rows a query attends, itself included
};
template <bool WIN>
__device__ __forceinline__ u32 window_lo(u32 pos, const AttnWindow<WIN> &wn) {
    if constexpr (WIN) return pos + 1u > wn.w ? pos + 1u - wn.w : 0u;
    else return 0u;
}

// split-KV (long contexts): block (head, sp) of an n_split launch takes the rows [p0, p1) of the n = pos + 1 - lo attended ones, in
// whole passes of a block (one head per block leaves all but H CUs idle: 51 us at 4096 positions).  A short context (up to two
// passes) is not worth splitting -- `solo`: the blocks of split 0 do it all and write the result themselves, the other blocks and the
// combine launch return at once.
template <int HD>
__device__ __forceinline__ bool attn_short(u32 n) {
    return n <= 2u * AttnGeom<HD>::PASS;
}
template <int HD>
__device__ __forceinline__ bool attn_solo(u32 n, u32 nsplit) {
    return nsplit > 1u && attn_short<HD>(n);
}
// the rows of a split: split sp of nsplit (a solo block: split 0 of 1) takes [p0, p1), p0 = lo + sp per, p1 = min(pos + 1, p0 + per).
// p0 >= p1: nothing to do, a neutral partial result is written.  (The two sums stay with the kernels: computed in here, behind the
// min, the compiler orders the scalar tests of attn_decode_kernel's current-token split another way.)
template <int HD>
__device__ __forceinline__ u32 attn_per(u32 n, u32 nsplit) {
    constexpr u32 PASS = AttnGeom<HD>::PASS;
    return nsplit > 1u ? (((n - 1u + nsplit) / nsplit + PASS - 1u) / PASS) * PASS : n;
}

// ------------------------------------------------------------------------------------------------ one cached row
__device__ __forceinline__ void unpack8(const uint4 &row, float (&f)[8]) {  // 16 bytes of a K / V / q row: 8 fp16 values
    const u32 w[4] = {row.x, row.y, row.z, row.w};
#pragma unroll
    for (int e = 0; e < 4; e++) {
        f[2 * e] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[e] & 0xFFFF));
        f[2 * e + 1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[e] >> 16));
    }
}
// 8 bytes of an fp8 K / V row: 8 OCP e4m3 codes, converted in hardware (v_cvt_pk_f32_fp8).  Every e4m3 value is an fp16 value, so the
// floats are those unpack8 gives for the fp16 row that holds the same numbers: the arithmetic behind the unpack does not know the format.
__device__ __forceinline__ void unpack8_fp8(const uint2 &row, float (&f)[8]) {
    const u32 w[2] = {row.x, row.y};
#pragma unroll
    for (int e = 0; e < 2; e++) {
        const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[e], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[e], true);
        f[4 * e] = lo[0], f[4 * e + 1] = lo[1], f[4 * e + 2] = hi[0], f[4 * e + 3] = hi[1];
    }
}
// the cache format of a launch: element type, the load of a lane's 8 dims of a row (16 bytes of fp16, 8 bytes of fp8), its unpack
template <bool KV8>
struct CacheFmt {
    typedef uint16_t elem;
    typedef uint4 row;
    static __device__ __forceinline__ row zero() { return make_uint4(0, 0, 0, 0); }
    static __device__ __forceinline__ void unpack(const row &r, float (&f)[8]) { unpack8(r, f); }
};
template <>
struct CacheFmt<true> {
    typedef uint8_t elem;
    typedef uint2 row;
    static __device__ __forceinline__ row zero() { return make_uint2(0, 0); }
    static __device__ __forceinline__ void unpack(const row &r, float (&f)[8]) { unpack8_fp8(r, f); }
};
// the per-KV-head scales of an fp8 cache (fp32 [n_kv_head], device memory): value = code * scale.  Compile-time like AttnWindow: the
// fp16 instances take an empty argument.
template <bool KV8>
struct AttnKv8 {};
template <>
struct AttnKv8<true> {
    const float *k_scale, *v_scale;
};
// the online softmax of one stream over a batch of U rows (scores pu, -3e38 = no row; V rows vfu): the rows share ONE rescale of the
// running (max, sum, weighted V) -- one exp for the old maximum and one per row
template <int U>
__device__ __forceinline__ void softmax_update(float &m_run, float &s_run, float (&acc)[8], const float (&pu)[U], const float (&vfu)[U][8]) {
    float m_new = m_run;
#pragma unroll
    for (int u = 0; u < U; u++) m_new = fmaxf(m_new, pu[u]);
    const float resc = __expf(m_run - m_new);
    s_run *= resc;
#pragma unroll
    for (int e = 0; e < 8; e++) acc[e] *= resc;
#pragma unroll
    for (int u = 0; u < U; u++) {
        // (not `pu > -2e38`: a NaN score compares false and would be dropped with weight 0 -- it must poison the head)
        const float wgt = !(pu[u] <= -2.0e38f) ? __expf(pu[u] - m_new) : 0.f;
        s_run += wgt;
#pragma unroll
        for (int e = 0; e < 8; e++) acc[e] += wgt * vfu[u][e];
    }
    m_run = m_new;
}

// ------------------------------------------------------------------------------------------------ the streams of a head, through LDS
// Behind the last pass a stream leaves its state in LDS -- sc [2 NS]: running max, then running sum; red2 [NS][HD]: weighted sums --
// and the block merges the streams of a head in ascending order.  attn_roped_kernel and fuse_attn_head first take the factors
// e^(m_i - M) once per head and stream (fl [NS], M = the maximum of the running maxima) instead of once per output element: the same
// values, 32 exponentials less on the tail of every thread.  (The stores and the loops of the merge are spelled out in the kernels:
// behind a call the compiler indexes the stores and unrolls the loops another way.)
// Streams that saw no row (a short context: wave w starts at row p0 + PPW U w) hold m = -3e38, l = 0, o = 0: their factor is exactly 0
// and they add exactly 0 -- a merge over the groups of 8 streams that can hold something gives the same sums bit for bit (at the 50
// positions of an average bench step: 16 of the 32 streams)
template <int HD>
__device__ __forceinline__ u32 merge_groups(u32 rows) {
    using G = AttnGeom<HD>;
    const u32 nw_act = min(G::NW, (rows + (u32)(G::PPW * G::U) - 1u) / (u32)(G::PPW * G::U));
    return (nw_act * (u32)G::PPW + 7u) >> 3;
}
// stream i joins output element dd of its head (o / sum is the result, (o, M, sum) a split's partial one)
template <int HD>
__device__ __forceinline__ void merge_step(const float *sc, const float *red2, const float *fl, u32 i, u32 dd, float &o, float &sum) {
    const float f = fl[i];
    sum += sc[AttnGeom<HD>::NS + i] * f;
    o += red2[i * HD + dd] * f;
}

// ------------------------------------------------------------------------------------------------ LDS layouts (offsets in floats)
// attn_decode_kernel<HD, QT>, a block of 64 NW threads
template <int HD>
struct DecodeLds {
    using G = AttnGeom<HD>;
    static constexpr u32 sc = 0;                         // [2 NS] running max / sum of the streams
    static constexpr u32 qs = sc + 2u * G::NS;           // [HD] the rotated q
    static constexpr u32 kcur = qs + HD;                 // [HD] k of the current token
    static constexpr u32 vcur = kcur + HD;               // [HD] v of the current token
    static constexpr u32 red = vcur + HD;                // [4 HD + 2 NW] scratch of the QK-norm statistics
    static constexpr u32 red2 = red + 4 * HD + 2u * G::NW;  // [NS][HD] partial outputs
    // QT only: the combined segments, the fp16 results, the partial sums of the 64 NW / (HD / 4) thread groups of an element group
    static constexpr u32 tv = red2 + G::NS * HD;         // [3][HD]
    static constexpr u32 res16 = tv + 3 * HD;            // [3][HD] fp16
    static constexpr u32 ps = res16 + 3 * HD / 2;        // [3][64 NW / (HD / 4)][HD]
    static constexpr u32 qt_end = ps + 3u * (64u * G::NW / (HD / 4u)) * HD;
    static constexpr size_t bytes(bool qt) { return ((size_t)(qt ? qt_end : tv) + 16u) * 4u; }  // (16 floats to spare, as ever)
};
// attn_roped_kernel<HD, QH>, and with QH = 1 the head blocks of the wqkv launch (fuse_attn_head)
template <int HD, int QH>
struct RopedLds {
    using G = AttnGeom<HD>;
    static constexpr u32 sc = 0;                          // [QH][2 NS]
    static constexpr u32 red2 = sc + QH * 2u * G::NS;     // [QH][NS][HD]
    static constexpr u32 fl = red2 + QH * G::NS * HD;     // [QH][NS] merge factors, then [QH] maxima
    static constexpr size_t bytes() { return ((size_t)fl + QH * G::NS + QH) * 4u; }
};

}  // namespace gq_attn
