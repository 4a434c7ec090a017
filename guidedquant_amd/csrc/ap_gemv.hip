// ap_gemv.hip -- Any-Precision LUT-GEMV / dequant kernels for gfx950 (MI355X) and their launchers.
//
// Replaces inference/ap_gemv/anyprec.cu (matmul_kbit_32, dequant_kbit_store) of the reference.  Not a
// translation: the reference is a warp-32 program with an LDS pair table; this is a wave-64 program that
//   * streams the bit-planes with one 16-byte load per lane per plane ("quad" = 4 of the reference's lanes),
//     RT rows in flight per lane, every row of a wave contiguous in memory (1 KiB per wave-load),
//   * decodes with v_perm_b32 byte lookups out of VGPR-resident LUT pools (no LDS on the weight path),
//   * keeps the activations of the lane's quad in 64 VGPRs for all its rows (staged once through LDS in a
//     bank-conflict-free, lane-linear image),
//   * accumulates in packed fp16 FMAs in EXACTLY the reference's per-lane order, so results are
//     bit-identical to the CUDA kernel (see ap_core.h and DESIGN.md),
//   * reduces through LDS in the reference's chunk order + 16/8/4/2/1 tree.
// Here: the v_perm kernel (ap_gemv_quad_kernel) with its INREG instance, the 2-bit pair-table kernel (ap_gemv_pt2_kernel), the
// reference-shaped generic kernel, the dequantiser, the exact-order planner and the plan entry points.  What these kernels share with
// ap_wide.hip and ap_dq.hip is in ap_exact.h; the fast mode's decode-to-fp16 matrix-core kernel is ap_dq.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "ap_core.h"
#include "ap_exact.h"
#include "gq_internal.h"

using namespace gq;

namespace {

// ----------------------------------------------------------------------------------------------
// The activation vector in LDS in the lane-linear image of ap_core.h::xlds_pos, built by ap_exact.h::stage_items (which has the fused
// prologues).  Work item = (quad q, byte c): 4 virtual lanes x 8 activations = 64 contiguous bytes of x, regrouped with 16 v_perm_b32
// into the 4 sixteen-byte slots (c, jj) of quad q.
// ----------------------------------------------------------------------------------------------
struct QuadImage : QuadItems {
    __device__ __forceinline__ static void put(const RowGeom &G, uint16_t *xlds, u32 q, u32 c, const u32 (&in)[4][4]) {
#pragma unroll
        for (u32 mth = 0; mth < 4; mth++) {
            uint4 o;
            o.x = perm(in[1][mth], in[0][mth], 0x05040100u);  // (v0,v1) @ j = 2m
            o.y = perm(in[3][mth], in[2][mth], 0x05040100u);  // (v2,v3) @ j = 2m
            o.z = perm(in[1][mth], in[0][mth], 0x07060302u);  // (v0,v1) @ j = 2m+1
            o.w = perm(in[3][mth], in[2][mth], 0x07060302u);  // (v2,v3) @ j = 2m+1
            *reinterpret_cast<uint4 *>(xlds + (((c * 4u + mth) * G.Q + q) << 3)) = o;
        }
    }
};

// ----------------------------------------------------------------------------------------------
// Fast path: BITS in {2,3,4}, K % 128 == 0, Q = K/128 <= blockDim.x.
//
// A block owns SPB consecutive "row steps" (one step = RS = blockDim/Q consecutive rows, one item per lane,
// a wave-load is 1 KiB of contiguous plane bytes).  The plane words + LUT of D steps ahead sit in a register
// ring, loaded with raw buffer loads: rows past the end get an out-of-range offset, which the hardware
// answers with zeros and no memory traffic, so the loop has no divergent control flow and the compiler's
// vmcnt bookkeeping stays exact.  The lane's activations stay in 64 VGPRs for the whole loop.
// ----------------------------------------------------------------------------------------------
// ----------------------------------------------------------------------------------------------
// INREG (rows of 4096 weights: Q = 32, a row is one half of a wave): the ordered reduction of a row step stays in registers.
// Lane hl = q of the half-wave holds the packed chunk partials of CUDA lanes t = 4 (q % 8) + v, v = 0..3, of chunk q / 8.  The chunk
// sums of anyprec.cu:505 (chunks ascending, starting from +0) meet in lanes hl < 8: own value, lane + 8 (row_shl:8), lane + 16
// (v_permlane16_swap), lane + 24 (row_shl:8 of that); the shuffle tree of anyprec.cu:363-370 is t + 16 = lane + 4 (row_shl:4), t + 8
// = lane ^ 2, t + 4 = lane ^ 1 (quad_perm), t + 2 = the second register, t + 1 = the upper half -- the same additions in the same
// order, ~30 VALU per step instead of the LDS partials + block barrier + reduction pass (1.2 of the 11.6 us of a w1w3 block,
// 0.6 of the 3.4 us of a wo block: profiles/r06_exact_epilogue.txt).  The row's value lands in lane hl = 0.
// ----------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ u32 mov_dpp(u32 v) { return (u32)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true); }
__device__ __forceinline__ u32 inreg_chunk_sum4(u32 s) {
    const u32 c1 = mov_dpp<0x108>(s);  // row_shl:8
    auto sw = __builtin_amdgcn_permlane16_swap(s, s, false, false);
    const u32 c2 = sw[1];
    const u32 c3 = mov_dpp<0x108>(c2);
    u32 p = pk_add(0u, s);
    p = pk_add(p, c1);
    p = pk_add(p, c2);
    return pk_add(p, c3);
}
__device__ __forceinline__ uint16_t inreg_reduce_row(u32 s01, u32 s23) {
    u32 p01 = inreg_chunk_sum4(s01), p23 = inreg_chunk_sum4(s23);
    p01 = pk_add(p01, mov_dpp<0x104>(p01)), p23 = pk_add(p23, mov_dpp<0x104>(p23));  // t + 16: row_shl:4
    p01 = pk_add(p01, mov_dpp<0x4E>(p01)), p23 = pk_add(p23, mov_dpp<0x4E>(p23));    // t + 8: quad_perm [2,3,0,1]
    p01 = pk_add(p01, mov_dpp<0xB1>(p01)), p23 = pk_add(p23, mov_dpp<0xB1>(p23));    // t + 4: quad_perm [1,0,3,2]
    const u32 pp = pk_add(p01, p23);                                                // t + 2
    return h_add((uint16_t)(pp & 0xFFFFu), (uint16_t)(pp >> 16));                  // t + 1
}

// Waves per SIMD the instances are compiled for (their amdgpu_waves_per_eu attributes), read by the planner and the plan entry points
// too: a planner that believed in more resident blocks than the attribute allows cost 8B w2 a second round of blocks.
// Register budget (tests/test_kernel_resources_cpu.py checks that no instance the dispatcher can pick spills): D = 1 fits 3 waves per
// SIMD at 2 / 3 bits (<= 168 VGPRs), and the INREG instance 4 at 2 bits, 3 at 4 bits; deeper rings and 4 bits are compiled for 2.
constexpr int quad_wpe(int bits, int D, bool inreg) { return inreg && bits == 2 ? 4 : ((bits <= 3 || inreg) && D == 1 ? 3 : 2); }
constexpr int PT2_WPE = 4;  // the pair-table kernel (105 VGPRs)

template <int BITS, int D, int PRO, bool INREG = false>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(quad_wpe(BITS, D, INREG)))) ap_gemv_quad_kernel(ApArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    RowGeom G;
    G.init(a.K);
    uint16_t *xlds = reinterpret_cast<uint16_t *>(smem);
    uint16_t *sv = xlds + G.K;  // [SPB*RS][nchunks*32]
    const u32 svrow = G.nchunks * 32u;
    float *red = reinterpret_cast<float *>(sv);  // scratch for the RMSNorm reduction (before sv is used)

    const u32 T = blockDim.x, tid = threadIdx.x;
    const u32 RS = a.RS, SPB = a.SPB;
    const u32 row0 = blockIdx.x * SPB * RS;
    const u32 m = blockIdx.y;
    const bool active = tid < RS * G.Q;
    const u32 rs = active ? tid / G.Q : 0u;
    const u32 q = active ? tid - rs * G.Q : 0u;
    // (GQ_STAMPS builds: s_memrealtime per wave of the middle block -- start, x in registers, after every step, loop barrier, end)
    // (GQ_STAMPS == 2: start / end of EVERY block instead -- wave 0 of block b writes dbg[2 b], dbg[2 b + 1]: the dispatch ramp of a launch)
    unsigned long long *qdbg = (GQ_STAMPS == 1 && a.dbg && blockIdx.x == gridDim.x / 2u && (tid & 63u) == 0u) ? a.dbg + (size_t)(tid >> 6) * 32u
                               : ((GQ_STAMPS == 2 && a.dbg && tid == 0u && blockIdx.y == 0u) ? a.dbg + 2u * (size_t)blockIdx.x : nullptr);
    u32 nst = 0;
    auto qstamp = [&]() {
        if (GQ_STAMPS == 1 && qdbg && nst < 32u) qdbg[nst++] = __builtin_amdgcn_s_memrealtime();
    };
    qstamp();
    if (GQ_STAMPS == 2 && qdbg) qdbg[0] = __builtin_amdgcn_s_memrealtime();

    constexpr int NRAW = (1 << BITS) / 2;
    const u32 plane_bytes = a.N * G.wpr * 4u;
    rsrc_t rq = make_rsrc(a.qw, plane_bytes * (u32)BITS);
    rsrc_t rl = make_rsrc(a.lut, a.N * (u32)NRAW * 4u);

    u32x4 P[D][BITS];
    u32 lraw[D][NRAW];
    auto issue = [&](int d, u32 step) {
        const u32 row = row0 + step * RS + rs;
        request_row<BITS>(rq, rl, active && step < SPB && row < a.N, row, q, G.wpr, plane_bytes, P[d], lraw[d]);
    };

    // 1. vector-memory results return in order: waves that stage x must not have plane loads queued in front of
    //    their x loads.  Upper half of the waves: fill the ring now; lower half: stage x first, then fill.
    const u32 nw = T >> 6, wv = tid >> 6;
    const bool stager = nw < 2u || wv < nw / 2u;
    if (!stager) {
#pragma unroll
        for (int d = 0; d < D; d++) issue(d, (u32)d);
    }
    // 2. activations -> LDS (lane-linear image) -> 64 VGPRs
    stage_items<PRO, QuadImage>(G, a.x + (size_t)m * (PRO == PRO_SILUMUL ? 2u * G.K : G.K), a.normw, a.eps, xlds, red, stager,
                     nw < 2u ? T : (nw / 2u) * 64u);
    if (stager) {
#pragma unroll
        for (int d = 0; d < D; d++) issue(d, (u32)d);
    }
    __syncthreads();
    XRegs xr;
#pragma unroll
    for (u32 c = 0; c < 4; c++)
#pragma unroll
        for (u32 jj = 0; jj < 4; jj++) {
            uint4 v = *reinterpret_cast<const uint4 *>(xlds + (((c * 4u + jj) * G.Q + q) << 3));
            xr.r[c][jj][0] = v.x;
            xr.r[c][jj][1] = v.y;
            xr.r[c][jj][2] = v.z;
            xr.r[c][jj][3] = v.w;
        }
    if (GQ_STAMPS == 1) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        qstamp();
    }

    // 3. decode + packed fp16 FMA chains, one item per step
    u32 chunk, t0, tpw;
    G.quad(q, chunk, t0, tpw);
    uint16_t *svp = sv + (size_t)rs * svrow + chunk * 32u + t0;
    for (u32 i = 0; i < SPB; i += D) {
#pragma unroll
        for (int d = 0; d < D; d++) {
            if (GQ_STAMPS == 1) {  // (words in hand)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                qstamp();
            }
            u32 Pw[BITS][4];
#pragma unroll
            for (int p = 0; p < BITS; p++) {
                Pw[p][0] = P[d][p].x;
                Pw[p][1] = P[d][p].y;
                Pw[p][2] = P[d][p].z;
                Pw[p][3] = P[d][p].w;
            }
            LutPools<BITS> L;
            L.build(lraw[d]);
            issue(d, i + (u32)d + (u32)D);  // refill this ring slot (its registers are now copied out)
            const u32 row = row0 + (i + (u32)d) * RS + rs;
            const bool rvalid = i + (u32)d < SPB && row < a.N;
            uint16_t res = 0;
            if constexpr (INREG) {
                if (a.resid && !(a.epilogue & GQ_EPI_SILU_PAIRS) && rvalid) res = a.resid[(size_t)m * a.N + row];
            }
            u32 s01, s23;
            Item<BITS>::run(Pw, L, xr, s01, s23);
            if constexpr (INREG) {
                uint16_t y = inreg_reduce_row(s01, s23);
                const bool lead = (tid & 31u) == 0u;
                if (a.epilogue & GQ_EPI_SILU_PAIRS) {
                    // rows (2i, 2i+1) = (gate_i, up_i) sit in the two halves of the wave: F.silu(gate) * up on fp16 values
                    // (inference/model.py:266), written to out[i]
                    const u32 yy = y;
                    auto sw = __builtin_amdgcn_permlane32_swap(yy, yy, false, false);  // sw[1]: lanes 32..63 of y in both halves
                    if (lead && !(tid & 32u) && rvalid && row + 1u < a.N) {
                        const _Float16 o = silu_pair(__builtin_bit_cast(_Float16, y), __builtin_bit_cast(_Float16, (uint16_t)sw[1]));
                        a.out[(size_t)m * (a.N >> 1) + (row >> 1)] = __builtin_bit_cast(uint16_t, o);
                    }
                } else if (lead && rvalid) {
                    if (a.resid) y = h_add(res, y);
                    a.out[(size_t)m * a.N + row] = y;
                }
            } else {
                if (active && i + (u32)d < SPB)
                    *reinterpret_cast<uint2 *>(svp + (size_t)(i + (u32)d) * RS * svrow) = make_uint2(s01, s23);
            }
            if (GQ_STAMPS) qstamp();
        }
    }
    if constexpr (INREG) {
        if (GQ_STAMPS) qstamp();
        if (GQ_STAMPS == 2 && qdbg) qdbg[1] = __builtin_amdgcn_s_memrealtime();
        return;
    }
    __syncthreads();
    if (GQ_STAMPS) qstamp();

    // 4. ordered reduction + epilogue
    rows_epilogue(G, a, sv, svrow, SPB * RS, row0, m, tid, T);
    if (GQ_STAMPS) qstamp();
    if (GQ_STAMPS == 2 && qdbg) qdbg[1] = __builtin_amdgcn_s_memrealtime();
}

// ----------------------------------------------------------------------------------------------
// Round 6 -- exact mode, 2 bits: the reference's LDS PAIR TABLE (anyprec.cu:397-419,454-490) on wave64.
//
// ap_gemv_quad_kernel decodes with v_perm_b32 out of VGPR byte pools: 2.25 VALU operations per weight, the kernel is VALU-bound
// (DESIGN.md section 3.1).  The reference looks a PAIR of weights up in a per-row table of 2^b x 2^b half2 entries in shared memory:
// one load per two weights, and the entry IS the hfma2 operand (even weight, odd weight).  Here the same table -- 16 entries of 4
// bytes per row at 2 bits -- lives in LDS per (wave, row of the wave: the lanes of a wave span at most two rows), rebuilt per row
// step by 32 lanes with one v_perm and one ds_write each; a lane (row slot, quad) forms the sixteen 4-bit indices of a plane-word
// pair with two v_bfi (M1 / M2 below), and per pair issues one v_lshrrev + one v_and_or (byte address) + one ds_read_b32 + one
// v_pk_fma_f16: 3.25 VALU per PAIR instead of 4.5, the look-ups on the LDS pipe (16 words of one table sit in 16 different banks,
// equal addresses broadcast: conflict-free).  The fp16 chains are the reference's own: per word (CUDA lane) ONE half2 accumulator
// (even chain, odd chain), byte c = 3..0, pair k = 0..3 (anyprec.cu:495-504), then sum.x + sum.y -- bit-identical to
// ap_gemv_quad_kernel and to the order-faithful oracle (tests/test_ap_gemv_gpu.py runs both kernels over every exact-mode case).
// The activation image in LDS is x in its natural order (a lane's 8 activations of (word v, byte c) are 16 contiguous bytes).
// ----------------------------------------------------------------------------------------------

template <int PRO>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(PT2_WPE))) ap_gemv_pt2_kernel(ApArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int BITS = 2, NRAW = 2;
    RowGeom G;
    G.init(a.K);
    uint16_t *xlds = reinterpret_cast<uint16_t *>(smem);
    uint16_t *sv = xlds + G.K;  // [SPB*RS][nchunks*32]
    const u32 svrow = G.nchunks * 32u;
    float *red = reinterpret_cast<float *>(sv);
    const u32 T = blockDim.x, tid = threadIdx.x, l = tid & 63u, wv = tid >> 6;
    const u32 RS = a.RS, SPB = a.SPB;
    const u32 row0 = blockIdx.x * SPB * RS;
    const u32 m = blockIdx.y;
    const bool active = tid < RS * G.Q;
    const u32 rs = active ? tid / G.Q : 0u;
    const u32 q = active ? tid - rs * G.Q : 0u;
    // pair tables of this wave: [2 rows of the wave][16 entries] words, behind sv
    u32 *tabs = reinterpret_cast<u32 *>(smem + (((size_t)G.K * 2u + (size_t)SPB * RS * svrow * 2u + 63u) & ~(size_t)63u)) + wv * 32u;
    const u32 plane_bytes = a.N * G.wpr * 4u;
    rsrc_t rq = make_rsrc(a.qw, plane_bytes * (u32)BITS);
    rsrc_t rl = make_rsrc(a.lut, a.N * (u32)NRAW * 4u);
    u32x4 P[BITS];
    u32 lraw[NRAW];
    auto issue = [&](u32 step) {
        const u32 row = row0 + step * RS + rs;
        request_row<BITS>(rq, rl, active && step < SPB && row < a.N, row, q, G.wpr, plane_bytes, P, lraw);
    };
    const u32 nw = T >> 6;
    const bool stager = nw < 2u || wv < nw / 2u;
    if (!stager) issue(0u);
    stage_x_natural<PRO>(G, a.x + (size_t)m * (PRO == PRO_SILUMUL ? 2u * G.K : G.K), a.normw, a.eps, xlds, red, stager, nw < 2u ? T : (nw / 2u) * 64u);
    if (stager) issue(0u);
    __syncthreads();
    // the lane's activations: xr[v][c] = the 8 activations of (word v, byte c) = 4 half2 operands (pair k = 0..3)
    u32 chunk, t0, tpw;
    G.quad(q, chunk, t0, tpw);
    uint4 xr[4][4];
#pragma unroll
    for (u32 v = 0; v < 4; v++)
#pragma unroll
        for (u32 c = 0; c < 4; c++) xr[v][c] = *reinterpret_cast<const uint4 *>(xlds + 1024u * chunk + 8u * tpw * c + 8u * (t0 + v));
    // table builders: lanes 0..15 build the table of the row of lane 0, lanes 16..31 that of the row of lane 63; entry i = (h_even,
    // h_odd, l_even, l_odd) -> half2(lut[2 h_even + l_even], lut[2 h_odd + l_odd]): the selector of the lane's entry is a constant
    const u32 ei = l & 15u;
    const u32 ce = ((ei >> 3) & 1u) * 2u + ((ei >> 1) & 1u), co = ((ei >> 2) & 1u) * 2u + (ei & 1u);
    const u32 esel = (2u * ce) | ((2u * ce + 1u) << 8) | ((2u * co) << 16) | ((2u * co + 1u) << 24);
    // which of the wave's two tables this lane reads: the row slot of lane 0 -> table 0, else table 1 (byte offset 64)
    // (the last ACTIVE lane of the wave carries its second row; a wave without active lanes builds tables nobody reads)
    const unsigned long long act = __builtin_amdgcn_ballot_w64(active);
    const u32 hi_lane = act ? 63u - (u32)__builtin_clzll(act) : 0u;
    const u32 rs_lo = (u32)__builtin_amdgcn_readfirstlane((int)rs);
    const u32 tbase = (u32)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)reinterpret_cast<unsigned char *>(tabs) + (rs == rs_lo ? 0u : 64u);
    uint16_t *svp = sv + (size_t)rs * svrow + chunk * 32u + t0;
    for (u32 i = 0; i < SPB; i++) {
        u32 Pw[BITS][4];
#pragma unroll
        for (int p = 0; p < BITS; p++) {
            Pw[p][0] = P[p].x;
            Pw[p][1] = P[p].y;
            Pw[p][2] = P[p].z;
            Pw[p][3] = P[p].w;
        }
        // this step's tables (the LDS serves a wave's operations in order: the previous step's look-ups are behind us)
        {
            const u32 lo0 = (u32)__builtin_amdgcn_readlane((int)lraw[0], 0), lo1 = (u32)__builtin_amdgcn_readlane((int)lraw[1], 0);
            const u32 hi0 = (u32)__builtin_amdgcn_readlane((int)lraw[0], (int)hi_lane), hi1 = (u32)__builtin_amdgcn_readlane((int)lraw[1], (int)hi_lane);
            const u32 ent = l < 16u ? perm(lo1, lo0, esel) : perm(hi1, hi0, esel);
            if (l < 32u) tabs[l] = ent;
        }
        issue(i + 1u);
        u32 s[4];
#pragma unroll
        for (int v = 0; v < 4; v++) {
            // nibble n of M1: bits (4 n + 3, 4 n + 2) of H and L; of M2: bits (4 n + 1, 4 n).  Byte c of a word = bits 8 (3 - c) ..;
            // pair k of byte c = bits (7 - 2 k, 6 - 2 k): k = 0, 2 from M1 (upper, lower nibble of the byte), k = 1, 3 from M2
            const u32 M1 = bfi(0xCCCCCCCCu, Pw[0][v], Pw[1][v] >> 2), M2 = bfi(0xCCCCCCCCu, Pw[0][v] << 2, Pw[1][v]);
            u32 acc = 0u;
#pragma unroll
            for (int c = 3; c >= 0; c--) {
                const u32 xw[4] = {xr[v][c].x, xr[v][c].y, xr[v][c].z, xr[v][c].w};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const u32 Mk = (k & 1) ? M2 : M1;
                    const int nib = 2 * (3 - c) + ((k & 2) ? 0 : 1);  // nibble index inside the word
                    const int sh = 4 * nib - 2;                       // bring the nibble to bits 5..2 (= index * 4)
                    const u32 addr = ((sh >= 0 ? (Mk >> sh) : (Mk << 2)) & 0x3Cu) | tbase;
                    // (an LDS-address-space load of the byte offset: through the generic `smem + addr` every look-up paid a v_add for the base)
                    const u32 w2 = *(const __attribute__((address_space(3))) u32 *)(uintptr_t)addr;
                    acc = pk_fma(w2, xw[k], acc);
                }
            }
            s[v] = (u32)h_add((uint16_t)(acc & 0xFFFFu), (uint16_t)(acc >> 16));
        }
        if (active) *reinterpret_cast<uint2 *>(svp + (size_t)i * RS * svrow) = make_uint2(s[0] | (s[1] << 16), s[2] | (s[3] << 16));
    }
    __syncthreads();
    // ordered reduction + epilogue: as ap_gemv_quad_kernel
    rows_epilogue(G, a, sv, svrow, SPB * RS, row0, m, tid, T);
}


// ----------------------------------------------------------------------------------------------
// Generic path: any 2 <= BITS <= 8, any K % 32 == 0.  32 lanes per row exactly like the reference warp
// (lane = virtual lane), LUT in LDS, 4-byte plane loads.  Slow; exists for API completeness (K % 128 != 0,
// M > 1 at bits 5..8) and as an on-device cross-check of the fast paths (GQ_AP_FORCE_GENERIC=1).
// ----------------------------------------------------------------------------------------------
template <int BITS>
__global__ void __launch_bounds__(256) ap_gemv_generic_kernel(ApArgs a, int ksplit) {
    __shared__ uint16_t lutl[8][1 << BITS];
    RowGeom G;
    G.init(a.K);
    const u32 tid = threadIdx.x, t = tid & 31u, g = tid >> 5;
    const u32 row = blockIdx.x * 8u + g;
    const u32 m = blockIdx.y;
    const bool ok = row < a.N;
    if (ok)
        for (u32 i = t; i < (1u << BITS); i += 32u) lutl[g][i] = a.lut[(size_t)row * (1u << BITS) + i];
    __syncthreads();
    const uint16_t *x = a.x + (size_t)m * G.K;
    const u32 ngroups = ksplit ? (G.nchunks + 3u) / 4u : 1u;
    uint16_t total = 0, result = 0;
    for (u32 grp = 0; grp < ngroups; grp++) {
        const u32 c0 = ksplit ? grp * 4u : 0u;
        const u32 c1 = ksplit ? min(c0 + 4u, G.nchunks) : G.nchunks;
        uint16_t partial = 0;
        for (u32 i = c0; i < c1 && ok; i++) {
            u32 tpw = 32u;
            if (i == G.nfull) {
                tpw = G.eff;
                if (t >= G.eff) break;
            }
            u32 P[BITS];
#pragma unroll
            for (int p = 0; p < BITS; p++) P[p] = a.qw[((size_t)p * a.N + row) * G.wpr + i * 32u + t];
            u32 acc = 0;  // (even chain, odd chain)
#pragma unroll
            for (int c = 3; c >= 0; c--) {
                const uint16_t *xs = x + 1024u * i + 8u * tpw * (u32)c + 8u * t;
                uint4 xv = ld16(xs);
                const u32 xw[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    u32 ce = 0, co = 0;
#pragma unroll
                    for (int p = 0; p < BITS; p++) {
                        ce = (ce << 1) | ((P[p] >> (31 - (8 * c + 2 * k))) & 1u);
                        co = (co << 1) | ((P[p] >> (30 - (8 * c + 2 * k))) & 1u);
                    }
                    u32 w = (u32)lutl[g][ce] | ((u32)lutl[g][co] << 16);
                    acc = pk_fma(w, xw[k], acc);
                }
            }
            partial = h_add(partial, h_add((uint16_t)(acc & 0xFFFF), (uint16_t)(acc >> 16)));
        }
#pragma unroll
        for (int sh = 16; sh >= 1; sh >>= 1) partial = h_add(partial, (uint16_t)__shfl_down((int)partial, sh, 32));
        if (ksplit)
            total = h_add(total, partial);
        else
            result = partial;
    }
    if (t == 0 && ok) {
        uint16_t y = ksplit ? total : result;
        if (a.resid) y = h_add(a.resid[row], y);
        a.out[(size_t)m * a.N + row] = y;
    }
}

// ----------------------------------------------------------------------------------------------
// Dequantise: W[n][e] = lut[n][code(n,e)]  (anyprec.cu:294-359).  One lane per plane word (32 weights):
// reads BITS words, writes four 16-byte runs (one per byte c) -- the reference's store pattern
// (anyprec.cu:355-357), 64 lanes wide.
// ----------------------------------------------------------------------------------------------
template <int BITS>
__global__ void __launch_bounds__(256) ap_dequant_kernel(const u32 *qw, const uint16_t *lut, uint16_t *W, u32 N, u32 K) {
    __shared__ uint16_t lutl[4][1 << BITS];
    RowGeom G;
    G.init(K);
    const u32 tid = threadIdx.x, g = tid >> 6, l = tid & 63u;
    const u32 row = blockIdx.x * 4u + g;
    const bool ok = row < N;
    if (ok)
        for (u32 i = l; i < (1u << BITS); i += 64u) lutl[g][i] = lut[(size_t)row * (1u << BITS) + i];
    __syncthreads();
    if (!ok) return;
    for (u32 w = l; w < G.wpr; w += 64u) {
        u32 chunk, t, tpw;
        if (w < 32u * G.nfull) {
            chunk = w / 32u;
            t = w % 32u;
            tpw = 32u;
        } else {
            chunk = G.nfull;
            t = w - 32u * G.nfull;
            tpw = G.eff;
        }
        u32 P[BITS];
#pragma unroll
        for (int p = 0; p < BITS; p++) P[p] = qw[((size_t)p * N + row) * G.wpr + w];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            u32 o[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                u32 ce = 0, co = 0;
#pragma unroll
                for (int p = 0; p < BITS; p++) {
                    ce = (ce << 1) | ((P[p] >> (31 - (8 * c + 2 * k))) & 1u);
                    co = (co << 1) | ((P[p] >> (30 - (8 * c + 2 * k))) & 1u);
                }
                o[k] = (u32)lutl[g][ce] | ((u32)lutl[g][co] << 16);
            }
            uint16_t *dst = W + (size_t)row * K + 1024u * chunk + 8u * tpw * (u32)c + 8u * t;
            *reinterpret_cast<uint4 *>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
        }
    }
}

// ----------------------------------------------------------------------------------------------
// Launchers
// ----------------------------------------------------------------------------------------------
struct QuadCfg {
    u32 T, RS, SPB, D, grid;
    size_t smem;
};

// the shapes the INREG instance serves: rows of 4096 weights (a row is one half of a wave) at ring depth 1
bool inreg_shape(u32 K, const QuadCfg &c) { return c.D == 1u && K == 4096u && c.T % 64u == 0u && c.RS * 32u == c.T; }
// .. and whether a launch on the plan takes it
bool inreg_plan(u32 K, const QuadCfg &c) { return inreg_shape(K, c) && gq_env_int("GQ_AP_INREG", 1) != 0; }

// `pt2`: the configuration is for the 2-bit pair-table kernel (4 waves per SIMD); `pairs`: the launch has the SiLU-pairs epilogue
bool pick_quad_cfg(u32 N, u32 K, int bits, QuadCfg &c, int pro = PRO_NONE, bool pt2 = false, bool pairs = false) {
    if (K % 128u) return false;
    const u32 Q = K / 128u;
    if (Q > 512u) return false;
    // block size: multiple of 64 in [192, 512] wasting the fewest lanes; ties -> 256, then the listed order
    u32 bestT = 0;
    double bestw = 2.0;
    const u32 cand[] = {256, 192, 320, 384, 448, 512};
    for (u32 T : cand) {
        if (T < Q) continue;
        double w = double(T - (T / Q) * Q) / double(T);
        if (w < bestw - 1e-9) {
            bestw = w;
            bestT = T;
        }
    }
    // rows of more than 8192 weights: the widest block with the same row slots per step -- the spare waves shorten the activation
    // staging and the ordered reduction (8B w2, K = 14336: 448 -> 512 threads, 10.9 -> 10.1 us per launch in exact mode)
    // (and rows of exactly 8192: 512 threads = 8 row slots instead of 4 -- Llama-3.3-70B's wqkv 12.4 vs 15.2 us, wo 8.7 vs 10.5, w1w3 41.7 vs 45.9)
    if (bestT && (Q == 64u || (Q > 64u && 512u / Q == bestT / Q))) bestT = 512u;
    const int envT = gq_env_int("GQ_AP_T", 0);
    if (envT >= 64 && envT <= 512 && envT % 64 == 0 && (u32)envT >= Q) bestT = (u32)envT;
    if (!bestT) return false;
    c.T = bestT;
    c.RS = bestT / Q;
    const u32 steps = (N + c.RS - 1) / c.RS;
    // ring depth D (steps of plane words + LUT row in flight per lane): the register budget is quad_wpe's; at 2 waves per SIMD (256
    // VGPRs) 4 bits fits D <= 3
    int d = gq_env_int("GQ_AP_D", 0);
    if (d < 1 || d > 4) d = bits <= 3 ? 1 : 2;
    if (bits == 4 && d > 3) d = 3;
    // persistent-style grid: about `bpc` blocks per CU (what the kernel's occupancy allows), every block the same number of steps
    const u32 cus = (u32)gq_cu_count();
    u32 bpc_def = bits <= 3 && d == 1 ? 3u : 2u;
    // a block of an RMSNorm launch normalises the whole vector before its first step: with ONE step per block (few rows: wqkv) the
    // 2-3 resident blocks of a CU repeat that side by side -- one block per CU then (measured, 8B wqkv: 3-bit 8.8 -> 8.4 us, 4-bit
    // 11.9 -> 11.0; the large matrices keep the deeper grid: w1w3 exact 2-bit 17.2 vs 21.9 us with one block per CU)
    if (pro == PRO_RMSNORM && steps <= cus * bpc_def) bpc_def = 1u;
    // never more blocks per CU than the instance's occupancy holds at once (round 6, per-block start stamps: 8B w2 in exact mode, 512-thread
    // blocks of a 3-waves-per-SIMD kernel = ONE resident block per CU, was launched as 512 blocks -- two rounds of 5 us each;
    // profiles/r06_exact_epilogue.txt).
    // (Known quirk, kept: the cap takes the INREG instance's occupancy from the shape alone -- under GQ_AP_INREG=0 the launch goes to the
    // plain instance, which at 2 bits holds 3 waves per SIMD, not 4.  tests/golden/exact_plans.json pins the plans as they are.)
    c.D = (u32)d;  // (the depth asked for: capped by SPB below)
    const u32 wpe = pt2 ? (u32)PT2_WPE : (u32)quad_wpe(bits, d, inreg_shape(K, c));
    const u32 bpc_max = std::max(1u, wpe * 4u / ((c.T + 63u) / 64u));
    if (bpc_def > bpc_max) bpc_def = bpc_max;
    u32 bpc = (u32)gq_env_int("GQ_AP_BPC", (int)bpc_def);
    if (bpc < 1) bpc = 1;
    u32 target = cus * bpc;
    u32 spb = (steps + target - 1) / target;
    if (spb < 1) spb = 1;
    const u32 nchunks = K / 1024u + ((K % 1024u) ? 1u : 0u);
    // LDS: x image + one fp16 partial per (row, chunk, virtual lane)
    auto smem_for = [&](u32 s) { return (size_t)K * 2u + (size_t)s * c.RS * nchunks * 64u + 64u; };
    while (spb > 1 && smem_for(spb) > 150u * 1024u) spb--;
    if (smem_for(spb) > 160u * 1024u) return false;
    // the SiLU-pairs epilogue combines rows (2i, 2i + 1) inside one block (rows_epilogue_n: the two halves of a wave), so a block must
    // start on an even row and hold an even number of rows.  An odd row step (K = 4608: 256 threads, RS = 7; K = 11008: RS = 5) with an
    // odd SPB would leave the pair at every block boundary split: SPB goes up by one, or down by one where the partials would not fit.
    if (pairs && ((spb * c.RS) & 1u)) {
        if (spb > 1u && smem_for(spb + 1u) > 150u * 1024u) spb--;
        else spb++;
        if (smem_for(spb) > 160u * 1024u) return false;
    }
    c.SPB = spb;
    c.grid = (steps + spb - 1) / spb;
    if ((u32)d > spb) d = (int)spb;
    c.D = (u32)d;
    c.smem = smem_for(spb);
    return true;
}

template <int BITS, int D, int PRO>
int launch_quad_inst(const ApArgs &a, const QuadCfg &c, u32 M, hipStream_t s) {
    dim3 grid(c.grid, M), block(c.T);
    ApArgs ad = a;
    if (GQ_STAMPS) ad.dbg = gq_debug_timing_buffer();
    // rows of 4096 weights at the shipped ring depth: the ordered reduction in registers (INREG above)
    if constexpr (D == 1) {
        if (inreg_plan(a.K, c)) {
            if (gq_ap_route(GQ_AP_ROUTE_EXACT, 1u, 1u)) return GQ_OK;
            static GqPerDeviceOnce once_r;
            auto kern_r = ap_gemv_quad_kernel<BITS, D, PRO, true>;
            GQ_HIP_CHECK(once_r.max_dynamic_lds(reinterpret_cast<const void *>(kern_r), (int)(160u * 1024u)));
            hipLaunchKernelGGL(kern_r, grid, block, c.smem, s, ad);
            GQ_HIP_CHECK(hipGetLastError());
            return GQ_OK;
        }
    }
    if (gq_ap_route(GQ_AP_ROUTE_EXACT, 1u, 0u)) return GQ_OK;
    static GqPerDeviceOnce once;
    auto kern = ap_gemv_quad_kernel<BITS, D, PRO>;
    GQ_HIP_CHECK(once.max_dynamic_lds(reinterpret_cast<const void *>(kern), (int)(160u * 1024u)));
    hipLaunchKernelGGL(kern, grid, block, c.smem, s, ad);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}

template <int BITS, int PRO>
int launch_quad_d(const ApArgs &a, const QuadCfg &c, u32 M, hipStream_t s) {
    switch (c.D) {
        case 1: return launch_quad_inst<BITS, 1, PRO>(a, c, M, s);
        case 2: return launch_quad_inst<BITS, 2, PRO>(a, c, M, s);
        case 3: return launch_quad_inst<BITS, 3, PRO>(a, c, M, s);
        default:
            if constexpr (BITS <= 3) return launch_quad_inst<BITS, 4, PRO>(a, c, M, s);
            else return launch_quad_inst<BITS, 3, PRO>(a, c, M, s);  // (pick_quad_cfg never asks for more at 4 bits: D = 4 would spill)
    }
}

template <int BITS>
int launch_quad(const ApArgs &a, const QuadCfg &c, u32 M, int pro, hipStream_t s) {
    switch (pro) {
        case PRO_RMSNORM: return launch_quad_d<BITS, PRO_RMSNORM>(a, c, M, s);
        case PRO_SILUMUL: return launch_quad_d<BITS, PRO_SILUMUL>(a, c, M, s);
        default: return launch_quad_d<BITS, PRO_NONE>(a, c, M, s);
    }
}

// the 2-bit pair-table kernel: asked for by GQ_AP_PT (0 never -- the default --, 1 rows of >= 8192 weights, 2 every shape it serves)
bool pt2_wanted(int bits, u32 K) {
    const int pt = gq_env_int("GQ_AP_PT", 0);
    return bits == 2 && (pt >= 2 || (pt == 1 && K >= 8192u));
}
size_t pt2_smem(u32 K, const QuadCfg &c) {
    const u32 nchunks = K / 1024u + ((K % 1024u) ? 1u : 0u);
    return (((size_t)K * 2u + (size_t)c.SPB * c.RS * nchunks * 64u + 63u) & ~(size_t)63u) + (size_t)(c.T / 64u) * 128u + 64u;
}
// ... and the plans it serves: a wave spans at most two rows (64 or more quads per row, or exactly 32) and the tables fit
bool pt2_serves(u32 K, const QuadCfg &c) {
    const u32 Q = K / 128u;
    return (Q == 32u || Q >= 64u) && !(c.T & 63u) && pt2_smem(K, c) <= 160u * 1024u;
}

// the exact-order launch the dispatcher makes for a shape (kernel: 0 v_perm kernel, 1 its INREG instance, 2 the pair-table kernel)
bool exact_plan(u32 N, u32 K, int bits, int pro, bool pairs, QuadCfg &c, u32 &kernel) {
    if (!pick_quad_cfg(N, K, bits, c, pro, false, pairs)) return false;
    kernel = inreg_plan(K, c) ? 1u : 0u;
    QuadCfg cp;
    if (pt2_wanted(bits, K) && pick_quad_cfg(N, K, bits, cp, pro, true, pairs) && pt2_serves(K, cp)) c = cp, kernel = 2u;
    return true;
}

}  // namespace
extern "C" int gq_debug_exact_plan_ex(uint32_t N, uint32_t K, int bits, int prologue, uint32_t epilogue, uint32_t *plan) {
    QuadCfg c;
    u32 kernel = 0;
    if (!plan || bits < 2 || bits > 4 || !exact_plan(N, K, bits, prologue, (epilogue & GQ_EPI_SILU_PAIRS) != 0, c, kernel)) return GQ_ENOTSUP;
    const u32 wpe = kernel == 2u ? (u32)PT2_WPE : (u32)quad_wpe(bits, (int)c.D, kernel == 1u);
    plan[0] = c.T, plan[1] = c.RS, plan[2] = c.SPB, plan[3] = c.D, plan[4] = c.grid, plan[5] = std::max(1u, wpe * 4u / ((c.T + 63u) / 64u));
    plan[6] = kernel;
    return GQ_OK;
}
extern "C" int gq_debug_exact_plan(uint32_t N, uint32_t K, int bits, int prologue, uint32_t *plan) {
    uint32_t p[7];
    const int rc = plan ? gq_debug_exact_plan_ex(N, K, bits, prologue, GQ_EPI_NONE, p) : GQ_ENOTSUP;
    if (rc == GQ_OK)
        for (int i = 0; i < 6; i++) plan[i] = p[i];
    return rc;
}
namespace {
// the 2-bit pair-table kernel on the quad kernel's configuration (+ the waves' tables behind the partial sums); GQ_ENOTSUP where it does
// not serve the plan (pt2_serves)
int launch_pt2(const ApArgs &a, const QuadCfg &c, u32 M, int pro, hipStream_t s) {
    if (!pt2_serves(a.K, c)) return GQ_ENOTSUP;
    if (gq_ap_route(GQ_AP_ROUTE_PAIR_TABLE, 1u, 2u)) return GQ_OK;
    const size_t smem = pt2_smem(a.K, c);
    dim3 grid(c.grid, M), block(c.T);
#define GQ_PT2(PRO_)                                                                                                            \
    do {                                                                                                                        \
        static GqPerDeviceOnce once;                                                                                            \
        GQ_HIP_CHECK(once.max_dynamic_lds(reinterpret_cast<const void *>(ap_gemv_pt2_kernel<PRO_>), (int)(160u * 1024u)));        \
        hipLaunchKernelGGL(ap_gemv_pt2_kernel<PRO_>, grid, block, smem, s, a);                                                  \
    } while (0)
    switch (pro) {
        case PRO_RMSNORM: GQ_PT2(PRO_RMSNORM); break;
        case PRO_SILUMUL: GQ_PT2(PRO_SILUMUL); break;
        default: GQ_PT2(PRO_NONE); break;
    }
#undef GQ_PT2
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}

template <int BITS>
int launch_generic(const ApArgs &a, u32 M, hipStream_t s) {
    const int ksplit = (M == 1 && a.K > 4096 && BITS >= 7) ? 1 : 0;  // anyprec.cu:611
    if (gq_ap_route(GQ_AP_ROUTE_GENERIC, 1u)) return GQ_OK;
    dim3 grid((a.N + 7) / 8, M), block(256);
    hipLaunchKernelGGL(ap_gemv_generic_kernel<BITS>, grid, block, 0, s, a, ksplit);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}

}  // namespace

namespace {
// the launches the fp16-order kernels serve, and the v_perm kernel's plan for them
bool exact_serves(const ApLaunch &L, QuadCfg &c) {
    return L.bits >= 2 && L.bits <= 4 && L.qbytes() < 0x7FFFFFFFull && pick_quad_cfg(L.N, L.K, L.bits, c, L.pro, false, L.pairs) && !L.unaligned16();
}
}  // namespace
int gq_ap_pair_table_try(const ApLaunch &L) {
    QuadCfg c, cp;
    if (!pt2_wanted(L.bits, L.K) || !exact_serves(L, c) || !pick_quad_cfg(L.N, L.K, L.bits, cp, L.pro, true, L.pairs)) return GQ_ENOTSUP;
    return launch_pt2(ap_args(L, cp.RS, cp.SPB), cp, L.M, L.pro, L.stream);
}
int gq_ap_exact_try(const ApLaunch &L) {
    QuadCfg c;
    if (!exact_serves(L, c)) return GQ_ENOTSUP;
    return gq_with_bits<2, 4>(L.bits, [&](auto B) { return launch_quad<B()>(ap_args(L, c.RS, c.SPB), c, L.M, L.pro, L.stream); });
}
int gq_ap_generic(const ApLaunch &L) {
    return gq_with_bits<2, 8>(L.bits, [&](auto B) { return launch_generic<B()>(ap_args(L, 0u, 0u), L.M, L.stream); });
}

extern "C" int gq_anyprec_dequant(const uint32_t *qweight, const void *lut, void *W, uint32_t N, uint32_t K, int bits,
                                  void *stream) {
    if (bits < 2 || bits > 8) return gq_fail(GQ_EINVAL, "Bitwidth must be between 2 and 8.");
    if (K == 0 || K % 32u || N == 0) return gq_fail(GQ_EINVAL, "bad shape: need N > 0 and K a positive multiple of 32.");
    if (!qweight || !lut || !W) return gq_fail(GQ_EINVAL, "null pointer argument.");
    if ((uintptr_t)W & 15u) return gq_fail(GQ_EINVAL, "output must be 16-byte aligned.");
    dim3 grid((N + 3) / 4), block(256);
    hipStream_t s = (hipStream_t)stream;
    const uint16_t *l = (const uint16_t *)lut;
    uint16_t *w = (uint16_t *)W;
    gq_with_bits<2, 8>(bits, [&](auto B) {
        hipLaunchKernelGGL(ap_dequant_kernel<B()>, grid, block, 0, s, qweight, l, w, N, K);
        return GQ_OK;
    });
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}
