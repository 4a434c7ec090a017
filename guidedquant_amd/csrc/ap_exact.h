// ap_exact.h -- device code shared by the Any-Precision GEMV kernels that decode with ap_core.h: the launch arguments, the fused
// prologues (their arithmetic, the RMSNorm statistic, the item loop of the image builders, the natural-order staging), the plane-word
// and LUT-row request, and the ordered reduction + epilogues with the gate/up pair output.  Each stands here once (DESIGN.md section
// 3.15; tests/test_csrc_single_definition_cpu.py).  Included by ap_gemv.hip (ap_gemv_quad_kernel, ap_gemv_pt2_kernel), ap_wide.hip
// (ap_gemv_wide_kernel, bits 5..8) -- the kernels that keep the reference's fp16 order -- and ap_dq.hip (ap_gemv_dq_kernel, fast mode).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ap_core.h"
#include "ap_dispatch.h"
#include "wave_util.h"

namespace {
using namespace gq;
using gqw::f2h;
using gqw::h2f;
using gqw::make_rsrc;
using gqw::rsrc_t;
using gqw::u32x4;
using gqw::wave_allsum;

struct ApArgs {
    const u32 *qw;         // [bits][N][K/32]
    const uint16_t *lut;   // [N][2^bits]
    const uint16_t *x;     // [M][K]
    uint16_t *out;         // [M][N] (or [M][N/2] with SILU_MUL)
    const uint16_t *normw; // [K] or null
    const uint16_t *resid; // [N] or null
    u32 N, K;
    u32 RS;                // row slots per block step = blockDim.x / Q
    u32 SPB;               // row steps per block
    u32 epilogue;
    float eps;
    void *ws;              // optional caller workspace (gq_anyprec_gemv_fused_ws) and its size
    size_t ws_bytes;
    const float *ssq_in;   // statistics hand-over (gq_anyprec_gemv_fused_ho): partial sums of squares of x / of the outputs
    float *ssq_out;
    unsigned long long *dbg = nullptr;  // GQ_STAMPS builds: the debug buffer of gq_debug_set_timing_buffer (tools/r6/exact_stamps.py)
};
// the kernel arguments of a launch on a plan of RS row slots and SPB row steps per block (the workspace and the hand-over are not these kernels')
inline ApArgs ap_args(const ApLaunch &L, u32 RS, u32 SPB) {
    ApArgs a{};
    a.qw = L.qweight, a.lut = L.lut, a.x = L.x, a.out = L.out, a.normw = L.normw, a.resid = L.resid;
    a.N = L.N, a.K = L.K, a.RS = RS, a.SPB = SPB, a.epilogue = L.epilogue, a.eps = L.eps;
    return a;
}

__device__ __forceinline__ uint4 ld16(const void *p) { return *reinterpret_cast<const uint4 *>(p); }
__device__ __forceinline__ uint4 ld16_nt(const void *p) {
    u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}

// Fused prologues, with the same fp16 rounding points as the reference's separate kernels.  Their arithmetic stands here once; the
// kernels differ only in which 16-byte units a thread takes and where the words go in LDS (stage_items, stage_x_natural below):
//   PRO_RMSNORM: y = (x.float() * rsqrt(mean(x^2) + eps)).half() * w        (inference/model.py:281-292)
//   PRO_SILUMUL: y = silu(g) * u with g = x[0:K], u = x[K:2K]                (inference/model.py:266)

// F.silu on an fp16 value evaluates x / (1 + exp(-x)) in fp32 and rounds to fp16; then an fp16 multiply (the gate/up pair outputs too)
__device__ __forceinline__ _Float16 silu_pair(_Float16 gate, _Float16 up) {
    const float gv = (float)gate;
    return (_Float16)(gv / (1.0f + __expf(-gv))) * up;
}
__device__ __forceinline__ u32 silu_mul_pk(u32 g, u32 u) {  // (silu_pair on both halves, spelled out: through it the SiLU * up kernels grow by six s_nop)
    float g0 = h2f(g & 0xFFFF), g1 = h2f(g >> 16);
    _Float16 s0 = (_Float16)(g0 / (1.0f + __expf(-g0)));
    _Float16 s1 = (_Float16)(g1 / (1.0f + __expf(-g1)));
    _Float16 r0 = s0 * __builtin_bit_cast(_Float16, (uint16_t)(u & 0xFFFF));
    _Float16 r1 = s1 * __builtin_bit_cast(_Float16, (uint16_t)(u >> 16));
    return (u32)__builtin_bit_cast(uint16_t, r0) | ((u32)__builtin_bit_cast(uint16_t, r1) << 16);
}
// the normalise of a packed fp16 pair: (x.float() * scale).half() * w
__device__ __forceinline__ u32 norm_pk(u32 x, u32 w, float scale) {
    const uint16_t a = f2h(gq_pin_f32(h2f(x & 0xFFFF) * scale)), b = f2h(gq_pin_f32(h2f(x >> 16) * scale));
    const _Float16 ra = __builtin_bit_cast(_Float16, a) * __builtin_bit_cast(_Float16, (uint16_t)(w & 0xFFFF));
    const _Float16 rb = __builtin_bit_cast(_Float16, b) * __builtin_bit_cast(_Float16, (uint16_t)(w >> 16));
    return (u32)__builtin_bit_cast(uint16_t, ra) | ((u32)__builtin_bit_cast(uint16_t, rb) << 16);
}

// A staging work item is 32 activations: four 16-byte units.  Item idx = (quad q = idx / 4, sub-item s = idx % 4) starts at activation
// e0 = Lay::base(G, q, s), and its unit c of a vector p is at Lay::unit(p, e0, c).  The sums of the statistic are fp32 and their order
// is part of the result, so the partition of the vector into items belongs to the kernel (its layout type):
//   QuadItems (here): item = (quad idx / 4, byte idx % 4), 64 contiguous bytes -- both exact kernels, so that they normalise with the
//                     same fp32 statistic bit for bit;
//   DqImage (ap_dq.hip): item = (quad, word), units 512 bytes apart.
struct QuadItems {
    __device__ __forceinline__ static u32 base(const RowGeom &G, u32 q, u32 c) { return G.xindex(q, 0u, c, 0u); }
    __device__ __forceinline__ static const uint16_t *unit(const uint16_t *p, u32 e0, int v) { return p + e0 + 8 * v; }
};
struct FirstItem {  // the activations and norm weights of a thread's first item
    u32 in[4][4], nw[4][4];
};
// The RMSNorm statistic: rsqrt(mean(x^2) + eps) over the stager threads' items (thread tid takes items tid, tid + T, ..), the wave sums
// exchanged through red[] (>= 16 floats of LDS) behind one barrier.
// KEEP -- ONE memory round trip (round 5): a stager thread requests the activations AND the norm weights of its first item (4 + 4
// sixteen-byte loads) up front, takes the sum of squares from those registers, and normalises from them behind the barrier.  The first
// version read x, reduced, and only then requested x again together with the norm weights -- a layer weight that comes from HBM: two
// extra round trips, +2.1 us (3 bits) / +3.3 us (4 bits) on the 8B wqkv launch against the plain one (bench.py roofline_by_shape,
// round 5).  Items beyond the first (K > 16 T) are re-read.
template <bool KEEP, typename Lay>
__device__ __forceinline__ float rms_scale(const RowGeom &G, const uint16_t *x, const uint16_t *normw, float eps, float *red,
                                           bool stager, u32 T, FirstItem *first) {
    const u32 tid = threadIdx.x, idx0 = stager ? tid : 4u * G.Q;
    float ss = 0.f;
    for (u32 idx = idx0; idx < 4u * G.Q; idx += T) {
        const u32 e0 = Lay::base(G, idx >> 2, idx & 3u);
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const uint4 t4 = ld16(Lay::unit(x, e0, v));
            const u32 w[4] = {t4.x, t4.y, t4.z, t4.w};
            if constexpr (KEEP) {
                if (idx == idx0) {
                    const uint4 n4 = ld16(Lay::unit(normw, e0, v));
                    first->in[v][0] = t4.x, first->in[v][1] = t4.y, first->in[v][2] = t4.z, first->in[v][3] = t4.w;
                    first->nw[v][0] = n4.x, first->nw[v][1] = n4.y, first->nw[v][2] = n4.z, first->nw[v][3] = n4.w;
                }
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const float a = h2f(w[i] & 0xFFFF), b = h2f(w[i] >> 16);
                ss += a * a;
                ss += b * b;
            }
        }
    }
    ss = wave_allsum(ss);
    if ((tid & 63u) == 0 && stager) red[tid >> 6] = ss;
    __syncthreads();
    // (the stager waves' sums: one LDS round trip + the same register tree, instead of one dependent ds_read per wave)
    const float tot = wave_allsum((tid & 63u) < (T + 63u) / 64u ? red[tid & 63u] : 0.f);
    return 1.0f / sqrtf(tot / (float)G.K + eps);
}

// The item loop of the two image builders (ap_gemv.hip::QuadImage, ap_dq.hip::DqImage): load the item's four units, apply the
// prologue, and hand the 4 x 4 words to Lay::put, which permutes them into the kernel's LDS image.
template <int PRO, typename Lay>
__device__ __forceinline__ void stage_items(const RowGeom &G, const uint16_t *x, const uint16_t *normw, float eps, uint16_t *xlds,
                                            float *red /* >= 16 floats of LDS */, bool stager, u32 T) {
    const u32 idx0 = stager ? threadIdx.x : 4u * G.Q;
    float scale = 0.f;
    FirstItem first;
    if constexpr (PRO == PRO_RMSNORM) scale = rms_scale<true, Lay>(G, x, normw, eps, red, stager, T, &first);
    for (u32 idx = idx0; idx < 4u * G.Q; idx += T) {
        const u32 q = idx >> 2, s = idx & 3u;
        const u32 e0 = Lay::base(G, q, s);
        u32 in[4][4];
#pragma unroll
        for (int v = 0; v < 4; v++) {
            if constexpr (PRO == PRO_RMSNORM) {
                u32 nw[4];
                if (idx == idx0) {
#pragma unroll
                    for (int i = 0; i < 4; i++) in[v][i] = first.in[v][i], nw[i] = first.nw[v][i];
                } else {
                    const uint4 t4 = ld16(Lay::unit(x, e0, v)), n4 = ld16(Lay::unit(normw, e0, v));
                    in[v][0] = t4.x, in[v][1] = t4.y, in[v][2] = t4.z, in[v][3] = t4.w;
                    nw[0] = n4.x, nw[1] = n4.y, nw[2] = n4.z, nw[3] = n4.w;
                }
#pragma unroll
                for (int i = 0; i < 4; i++) in[v][i] = norm_pk(in[v][i], nw[i], scale);
            } else {
                const uint4 t4 = ld16(Lay::unit(x, e0, v));
                in[v][0] = t4.x, in[v][1] = t4.y, in[v][2] = t4.z, in[v][3] = t4.w;
                if constexpr (PRO == PRO_SILUMUL) {
                    const uint4 u4 = ld16(Lay::unit(x + G.K, e0, v));
                    const u32 uw[4] = {u4.x, u4.y, u4.z, u4.w};
#pragma unroll
                    for (int i = 0; i < 4; i++) in[v][i] = silu_mul_pk(in[v][i], uw[i]);
                }
            }
        }
        Lay::put(G, xlds, q, s, in);
    }
}

// The plane words and the LUT row of one (row, quad), requested with raw buffer loads into the caller's registers.  A dead request
// (!ok: a row past the end, an idle lane) gets an out-of-range offset, which the hardware answers with zeros and no memory traffic: no
// divergent control flow, and the compiler's vmcnt bookkeeping stays exact.
template <int BITS>
__device__ __forceinline__ void request_row(rsrc_t rq, rsrc_t rl, bool ok, u32 row, u32 quad, u32 wpr, u32 plane_bytes, u32x4 (&P)[BITS],
                                            u32 (&lraw)[(1 << BITS) / 2]) {
    constexpr int NRAW = (1 << BITS) / 2;
    constexpr u32 OOB = 0x80000000u;
    const u32 off = ok ? (row * wpr + 4u * quad) * 4u : OOB;
#pragma unroll
    for (int p = 0; p < BITS; p++) P[p] = __builtin_amdgcn_raw_buffer_load_b128(rq, ok ? off + (u32)p * plane_bytes : OOB, 0, 2 /* nt */);
    const u32 loff = ok ? row * (u32)NRAW * 4u : OOB;
    if constexpr (NRAW == 2) {
        auto v = __builtin_amdgcn_raw_buffer_load_b64(rl, loff, 0, 0);
        lraw[0] = v[0];
        lraw[1] = v[1];
    } else {
#pragma unroll
        for (int i = 0; i < NRAW; i += 4) {
            u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rl, ok ? loff + (u32)i * 4u : OOB, 0, 0);
            lraw[i] = v.x;
            lraw[i + 1] = v.y;
            lraw[i + 2] = v.z;
            lraw[i + 3] = v.w;
        }
    }
}

// ----------------------------------------------------------------------------------------------
// Final reduction of one row from its per-(chunk, virtual lane) fp16 partials in LDS:
// chunks in ascending order per lane (anyprec.cu:505), then the 16,8,4,2,1 shuffle tree (anyprec.cu:363-370).
// Called by 32 consecutive lanes (t = lane & 31).  Returns the row value in lane t == 0.
// ----------------------------------------------------------------------------------------------
// The chain is what the reference computes; how the values travel is this chip's: the partials of four chunks are read from LDS in
// one round trip, the 16-lane step is one v_permlane16_swap (rows 0 / 1 of the wave exchanged in registers), the 8 / 4 / 2 / 1 steps are
// DPP operands of the adds (row_ror:8, row_shl:4, quad_perm) -- lane t < sh receives lane t + sh exactly as __shfl_down(.., sh, 32) hands
// it over, the other lanes' values are never used.  (Round 6: with one ds_read / ds_bpermute round trip per add the epilogue of a block
// was 0.6 us per pass of T / 32 rows -- 2.8 of the 12.7 us of a w1w3 block; tools/r6/exact_stamps.py.)
__device__ __forceinline__ uint16_t h_add_dpp16(uint16_t p) {  // p[t] + p[t + 16], t < 16 of every 32
    const u32 v = p;
    auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);  // r[0] = rows (0, 0, 2, 2), r[1] = rows (1, 1, 3, 3)
    return h_add((uint16_t)r[0], (uint16_t)r[1]);
}
template <int CTRL>
__device__ __forceinline__ uint16_t h_add_dpp(uint16_t p) {
    return h_add(p, (uint16_t)__builtin_amdgcn_update_dpp(0, (int)(u32)p, CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ uint16_t reduce_tree(uint16_t p) {
    p = h_add_dpp16(p);
    p = h_add_dpp<0x128>(p);  // row_ror:8   lane t <- t + 8 (mod 16)
    p = h_add_dpp<0x104>(p);  // row_shl:4   lane t <- t + 4
    p = h_add_dpp<0x4E>(p);   // quad_perm [2,3,0,1]
    p = h_add_dpp<0xB1>(p);   // quad_perm [1,0,3,2]
    return p;
}
__device__ __forceinline__ uint16_t reduce_row(const RowGeom &G, const uint16_t *sv, u32 t, u32 c0, u32 c1) {
    uint16_t p = 0;
    for (u32 i0 = c0; i0 < c1; i0 += 4u) {
        uint16_t v[4];
        bool ok[4];
#pragma unroll
        for (u32 j = 0; j < 4u; j++) {
            const u32 i = i0 + j;
            ok[j] = i < c1 && !(i == G.nfull && t >= G.eff);  // (the lanes past the end of a partial last chunk hold no partial: no add)
            v[j] = sv[(ok[j] ? i : c0) * 32u + t];
        }
#pragma unroll
        for (u32 j = 0; j < 4u; j++) p = ok[j] ? h_add(p, v[j]) : p;
    }
    return reduce_tree(p);
}

// NCH > 0: rows of exactly NCH full chunks (no predicates, one LDS round trip for all partials of a row)
template <int NCH>
__device__ __forceinline__ uint16_t reduce_row_n(const RowGeom &G, const uint16_t *sv, u32 t) {
    if constexpr (NCH == 0) return reduce_row(G, sv, t, 0u, G.nchunks);
    else {
        uint16_t v[NCH];
#pragma unroll
        for (int i = 0; i < NCH; i++) v[i] = sv[(u32)i * 32u + t];
        uint16_t p = 0;
#pragma unroll
        for (int i = 0; i < NCH; i++) p = h_add(p, v[i]);
        return reduce_tree(p);
    }
}

// Ordered reduction + epilogue of the R rows of a block, 32 lanes per row, TWO rows per 32-lane group and trip (their LDS round trips
// and add chains are independent: the compiler interleaves them); the residual is requested before the row's partials are read.
// KS: the reference's K-split (anyprec.cu:611, bits >= 7 and K > 4096 at one batch row): groups of 4 chunks, each through the chunk
// sum and the tree, added in ascending order into a zeroed fp16 cell (ap_wide.hip)
__device__ __forceinline__ uint16_t reduce_row_ksplit(const RowGeom &G, const uint16_t *sv, u32 t) {
    uint16_t total = 0;
    for (u32 c0 = 0; c0 < G.nchunks; c0 += 4u) total = h_add(total, reduce_row(G, sv, t, c0, c0 + 4u < G.nchunks ? c0 + 4u : G.nchunks));
    return total;
}

template <int NCH, bool KS = false>
__device__ __forceinline__ void rows_epilogue_n(const RowGeom &G, const ApArgs &a, const uint16_t *sv, u32 svrow, u32 R, u32 row0, u32 m,
                                                u32 tid, u32 T) {
    const u32 t = tid & 31u, stride = T >> 5;
    const bool pairs = a.epilogue & GQ_EPI_SILU_PAIRS;
    for (u32 r0 = tid >> 5; r0 < R; r0 += 2u * stride) {
        const u32 r1 = r0 + stride;
        const bool has1 = r1 < R;
        const u32 row[2] = {row0 + r0, row0 + r1};
        const bool live[2] = {true, has1};
        uint16_t res[2] = {0, 0};
        if (!pairs && a.resid) {
#pragma unroll
            for (int e = 0; e < 2; e++)
                if (live[e] && row[e] < a.N) res[e] = a.resid[(size_t)m * a.N + row[e]];
        }
        uint16_t y[2];
        if constexpr (KS) {
            y[0] = reduce_row_ksplit(G, sv + (size_t)r0 * svrow, t);
            y[1] = reduce_row_ksplit(G, sv + (size_t)(has1 ? r1 : r0) * svrow, t);
        } else {
            y[0] = reduce_row_n<NCH>(G, sv + (size_t)r0 * svrow, t);
            y[1] = reduce_row_n<NCH>(G, sv + (size_t)(has1 ? r1 : r0) * svrow, t);
        }
#pragma unroll
        for (int e = 0; e < 2; e++) {
            if (pairs) {
                // rows (2i, 2i+1) = (gate_i, up_i) sit in the two halves of the wave: F.silu(gate) * up on fp16 values
                // (inference/model.py:266), written to out[i]
                const u32 yy = y[e];
                auto sw = __builtin_amdgcn_permlane32_swap(yy, yy, false, false);  // sw[1]: lanes 32..63 of y in both halves
                const uint16_t yo = (uint16_t)sw[1];
                if (live[e] && t == 0 && !(tid & 32u) && row[e] + 1u < a.N) {
                    const _Float16 o = silu_pair(__builtin_bit_cast(_Float16, y[e]), __builtin_bit_cast(_Float16, yo));
                    a.out[(size_t)m * (a.N >> 1) + (row[e] >> 1)] = __builtin_bit_cast(uint16_t, o);
                }
            } else if (live[e] && t == 0 && row[e] < a.N) {
                if (a.resid) y[e] = h_add(res[e], y[e]);
                a.out[(size_t)m * a.N + row[e]] = y[e];
            }
        }
    }
}
template <bool KS = false>
__device__ __forceinline__ void rows_epilogue(const RowGeom &G, const ApArgs &a, const uint16_t *sv, u32 svrow, u32 R, u32 row0, u32 m, u32 tid,
                                              u32 T) {
    if constexpr (KS) {
        rows_epilogue_n<0, true>(G, a, sv, svrow, R, row0, m, tid, T);
        return;
    }
    // (compiled-in chunk counts of the Llama rows: K = 4096, 8192, 14336; everything else -- partial last chunks too -- on the general one)
    const u32 nch = G.eff ? 0u : G.nchunks;
    if (nch == 4u) rows_epilogue_n<4>(G, a, sv, svrow, R, row0, m, tid, T);
    else if (nch == 8u) rows_epilogue_n<8>(G, a, sv, svrow, R, row0, m, tid, T);
    else if (nch == 14u) rows_epilogue_n<14>(G, a, sv, svrow, R, row0, m, tid, T);
    else rows_epilogue_n<0>(G, a, sv, svrow, R, row0, m, tid, T);
}

// ----------------------------------------------------------------------------------------------
// The activation image in LDS in x's natural order (a lane's 8 activations of (word v, byte c) are 16 contiguous bytes): a flat loop over
// the 16-byte units, behind the shared statistic in QuadItems' order.
// ----------------------------------------------------------------------------------------------
template <int PRO>
__device__ __forceinline__ void stage_x_natural(const RowGeom &G, const uint16_t *x, const uint16_t *normw, float eps, uint16_t *xlds, float *red,
                                                bool stager, u32 T) {
    const u32 tid = threadIdx.x, nun = G.K / 8u;
    float scale = 0.f;
    if constexpr (PRO == PRO_RMSNORM) scale = rms_scale<false, QuadItems>(G, x, normw, eps, red, stager, T, nullptr);
    for (u32 u = stager ? tid : nun; u < nun; u += T) {
        uint4 t4 = ld16(x + 8u * u);
        u32 in[4] = {t4.x, t4.y, t4.z, t4.w};
        if constexpr (PRO == PRO_RMSNORM) {
            const uint4 n4 = ld16(normw + 8u * u);
            const u32 nw[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
            for (int i = 0; i < 4; i++) in[i] = norm_pk(in[i], nw[i], scale);
        }
        if constexpr (PRO == PRO_SILUMUL) {
            const uint4 u4 = ld16(x + G.K + 8u * u);
            const u32 uw[4] = {u4.x, u4.y, u4.z, u4.w};
#pragma unroll
            for (int i = 0; i < 4; i++) in[i] = silu_mul_pk(in[i], uw[i]);
        }
        *reinterpret_cast<uint4 *>(xlds + 8u * u) = make_uint4(in[0], in[1], in[2], in[3]);
    }
}

}  // namespace
