// ap_dq.hip -- "decode to fp16, accumulate on the matrix cores": the fast-mode Any-Precision GEMV for 2 to 4 bits and one batch row
// (round 6), with its planner, launchers and dispatch entry gq_ap_dq_try (ap_dispatch.h).  NOT one of the bit-identical kernels: those
// are ap_gemv.hip's and ap_wide.hip's.  It shares their decode (ap_core.h) and the fused prologues' arithmetic (ap_exact.h).
//
// The plane-MFMA kernels (ap_plane.hip / ap_stream.hip) multiply 2^b - 1 BINARY matrices per b-bit LUT: 3 at 2 bits, 7 at 3, 15
// at 4 -- 24 / 56 / 120 FP4 x BF8 MFMAs of 32 cycles per 16 rows x 1024 weights, with ~8 VALU instructions per MFMA to build the
// operands: at 4 bits ~1,040 instructions per block, instruction-issue-bound at 2.3 x the matrix floor (w1w3 24 us, 0.30 of the
// HBM roofline).  The decode of the exact kernels (ap_core.h: v_perm_b32 look-ups in the row's LUT held as VGPR byte pools) grows far
// more slowly with b -- 1.6 / 2.2 / 3.9 VALU operations per weight -- and what it yields, packed fp16 pairs of four weights at one bit
// position, IS an A fragment of v_mfma_f32_16x16x32_f16: lane (row r = l % 16, quad g = l / 16) holds 8 weights of row r, and the K
// index of a matrix-core product is only a label -- any 8 weights do, as long as the B fragment of lane (column, g) holds the 8
// activations that belong to them: one 16-byte slot of an activation image staged in LDS in the decode's own order (the first version
// used the exact kernels' image, ap_core.h::xlds_pos, and their byte transpose of the quad; the second -- DqItem / DqImage below --
// drops the transpose: profiles/r06_dq_kernel.txt).  So:
//   * A = two look-ups (4 VGPRs), B = one ds_read_b128 of the staged image (column 0 reads it, columns 1..15 read zeros from
//     outside the block's LDS allocation -- idle columns fed real data cost 8 % in clocks), one MFMA
//     of 16 cycles per 16 rows x 32 weights: 32 per 16 x 1024 block instead of 56 / 120, no bf8 pieces, no image build, no
//     extraction of large activations, no Moebius coefficients;
//   * products of fp16 values are exact in the fp32 accumulator, sums in fp32, one fp16 rounding: the fast-mode envelope
//     (tests/ap_helpers.py::_check_fast) -- not the reference's fp16 accumulation order (that is the exact mode);
//   * prologues (RMSNorm, SiLU * up) from ap_exact.h::stage_items, with the reference's rounding points; plain / residual / gate-up pair epilogues.
// Work: item = (16-row group, unit of 4 quads = 512 weights per row); wave w of a 16-wave block takes items w, w + 16, ..; the
// K-split partial sums of a row group meet in LDS and are added in unit order (deterministic).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ap_core.h"
#include "ap_exact.h"
#include "gq_internal.h"

using namespace gq;

namespace {
using gqw::f16x8;
using gqw::f32x4;

template <int BITS>
struct DqItem;  // run(P, L, emit): emit(v, k, w01 @ 2 k, w23 @ 2 k, w01 @ 2 k + 1, w23 @ 2 k + 1) for word v = 0..3, pair k = 0..3
// NO byte transpose of the quad (ap_core.h::transpose_quad, 8 v_perm per plane): the exact kernels need it to keep the reference's
// chain order, a matrix-core product does not care which 8 weights share an operand.  A selector taken from ONE word holds the codes
// of the same bit position j of its four bytes c = 3, 2, 1, 0 (byte 0 = c 3: pack.py's byte order); the look-up returns
// w01 = (w[c3], w[c2]), w23 = (w[c1], w[c0]) at that j -- the activation image (DqImage) keeps the matching order.
template <>
struct DqItem<2> {
    template <typename E>
    __device__ __forceinline__ static void run(const u32 P[2][4], const LutPools<2> &L, E emit) {
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const u32 Cm = bfi(0xAAAAAAAAu, P[0][v], P[1][v] >> 1), Dm = bfi(0xAAAAAAAAu, P[0][v] << 1, P[1][v]);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                u32 a01, a23, b01, b23;
                lookup4<2>(L, (Cm >> (6 - 2 * k)) & 0x03030303u, 0u, a01, a23);
                lookup4<2>(L, (Dm >> (6 - 2 * k)) & 0x03030303u, 0u, b01, b23);
                emit(v, k, a01, a23, b01, b23);
            }
        }
    }
};
template <>
struct DqItem<3> {
    template <typename E>
    __device__ __forceinline__ static void run(const u32 P[3][4], const LutPools<3> &L, E emit) {
#pragma unroll
        for (int v = 0; v < 4; v++) {
            u32 nib[4];
#pragma unroll
            for (int r = 0; r < 4; r++) nib[r] = bfi(0x44444444u, shl(P[0][v], 2 - r), bfi(0x22222222u, shl(P[1][v], 1 - r), P[2][v] >> r));
#pragma unroll
            for (int k = 0; k < 4; k++) {
                u32 w[2][2];
#pragma unroll
                for (int par = 0; par < 2; par++) {
                    const int s = 7 - (2 * k + par);
                    const u32 S = ((s & 4) ? (nib[s & 3] >> 4) : nib[s & 3]) & 0x07070707u;
                    lookup4<3>(L, S, 0u, w[par][0], w[par][1]);
                }
                emit(v, k, w[0][0], w[0][1], w[1][0], w[1][1]);
            }
        }
    }
};
template <>
struct DqItem<4> {
    template <typename E>
    __device__ __forceinline__ static void run(const u32 P[4][4], const LutPools<4> &L, E emit) {
#pragma unroll
        for (int v = 0; v < 4; v++) {
            u32 nib[4];
#pragma unroll
            for (int r = 0; r < 4; r++) nib[r] = bfi(0x44444444u, shl(P[1][v], 2 - r), bfi(0x22222222u, shl(P[2][v], 1 - r), P[3][v] >> r));
#pragma unroll
            for (int k = 0; k < 4; k++) {
                u32 w[2][2];
#pragma unroll
                for (int par = 0; par < 2; par++) {
                    const int s = 7 - (2 * k + par);
                    const u32 S = ((s & 4) ? (nib[s & 3] >> 4) : nib[s & 3]) & 0x07070707u;
                    // the MSB plane picks the pool: 0x00 / 0xFF per byte as x * 255 = (x << 8) - x (mod 2^32: exact for bytes of 0 / 1) -- two
                    // VOP2 operations instead of ap_core.h's selector OR + v_perm.  (A 24-bit multiply by 255 is one operation and WRONG: it
                    // drops byte 3 -- 531 tokens/s and 11 failed tests.)
                    const u32 mb = (P[0][v] >> s) & 0x01010101u;
                    const u32 m = (mb << 8) - mb;
                    const u32 lo = bfi(m, perm(L.lo[3], L.lo[2], S), perm(L.lo[1], L.lo[0], S));
                    const u32 hi = bfi(m, perm(L.hi[3], L.hi[2], S), perm(L.hi[1], L.hi[0], S));
                    w[par][0] = perm(hi, lo, 0x05010400u);
                    w[par][1] = perm(hi, lo, 0x07030602u);
                }
                emit(v, k, w[0][0], w[0][1], w[1][0], w[1][1]);
            }
        }
    }
};

// The activation image of the dq kernel: 16-byte slot (v * 4 + k) * Q + q = the 8 activations that meet the A operand of (quad q,
// word v, pair k): [x(c3, 2k), x(c2, 2k), x(c1, 2k), x(c0, 2k), x(c3, 2k+1), x(c2, 2k+1), x(c1, 2k+1), x(c0, 2k+1)], x(c, j) =
// x[G.xindex(q, v, c, j)].  Work item = (quad q, word v): four 16-byte loads (one per byte c), four v_perm per slot; the loop and the
// prologues are ap_exact.h::stage_items'.
struct DqImage {
    // (K % 1024 == 0 for this kernel: whole chunks only -- item idx = 4 q + v = (quad q, word v) starts at activation
    // 1024 (q / 8) + 8 (4 (q % 8) + v) = 1024 (idx / 32) + 8 (idx % 32); byte c adds 256)
    __device__ __forceinline__ static u32 base(const RowGeom &, u32 q, u32 v) {
        const u32 idx = 4u * q + v;
        return 1024u * (idx >> 5) + 8u * (idx & 31u);
    }
    __device__ __forceinline__ static const uint16_t *unit(const uint16_t *p, u32 e0, u32 c) { return p + (e0 + 256u * c); }
    __device__ __forceinline__ static void put(const RowGeom &G, uint16_t *xlds, u32 q, u32 v, const u32 (&in)[4][4]) {  // in[c][k]: (x(c, 2k), x(c, 2k+1))
#pragma unroll
        for (u32 k = 0; k < 4; k++) {
            uint4 o;
            o.x = perm(in[2][k], in[3][k], 0x05040100u);  // (x(c3, 2k), x(c2, 2k))
            o.y = perm(in[0][k], in[1][k], 0x05040100u);  // (x(c1, 2k), x(c0, 2k))
            o.z = perm(in[2][k], in[3][k], 0x07060302u);  // (x(c3, 2k+1), x(c2, 2k+1))
            o.w = perm(in[0][k], in[1][k], 0x07060302u);  // (x(c1, 2k+1), x(c0, 2k+1))
            *reinterpret_cast<uint4 *>(xlds + (((v * 4u + k) * G.Q + q) << 3)) = o;
        }
    }
};

struct DqArgs {
    ApArgs a;
    u32 RGB;      // 16-row groups per block
    u32 NU;       // units (512 weights) per row
    u32 part_off; // LDS offset of the partial sums
    unsigned long long *dbg;  // GQ_STAMPS builds: the debug buffer of gq_debug_set_timing_buffer
};
constexpr u32 DQ_WAVES = 16;  // waves per block
// One item's plane words in flight per wave: the next item's are requested while this one is decoded.  More measured SLOWER, as a
// register ring and as slots behind explicit waits, and so did 8-wave blocks at 3 / 4 per CU (DESIGN.md section 3.15 has the numbers;
// profiles/r06_dq_kernel.txt): issuing a load blocks the wave once the CU's memory pipe is full, and every slot of a ring is another
// copy of the ~600 instructions (5 KB) of an item's unrolled decode in the instruction cache.
#ifndef DQ_KO
#define DQ_KO 0  // build-time knock-outs, WRONG numerics, timing only (bit mask): 1 no B reads, 2 no MFMAs, 4 no plane loads
#endif
// occupancy the instances are compiled for (waves per SIMD): the decode is a dependent chain (selectors -> look-ups -> MFMA), so more
// resident waves = fewer idle issue slots; ONE 16-wave block per CU is the fastest form.  Read by the attribute and by pick_dq_cfg.
constexpr int dq_wpe(int /* bits: one figure for 2 to 4 bits today */) { return 4; }

// QT: quads per row compiled in (32: K = 4096, 112: K = 14336 -- the 8B widths; 0: read from the launch): the sixteen B-fragment
// addresses of an item are then immediate offsets of ONE base register instead of sixteen v_add (7 % of the 3-bit item's VALU)
template <int BITS, int PRO, int QT>
__global__ void __launch_bounds__(64 * DQ_WAVES) __attribute__((amdgpu_waves_per_eu(dq_wpe(BITS)))) ap_gemv_dq_kernel(DqArgs da) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const ApArgs &a = da.a;
    RowGeom G;
    G.init(a.K);
    uint16_t *xlds = reinterpret_cast<uint16_t *>(smem);
    float *part = reinterpret_cast<float *>(smem + da.part_off);
    float *red = part;  // (RMSNorm reduction scratch: before the partial sums exist)
    const u32 tid = threadIdx.x, l = tid & 63u, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const u32 r = l & 15u, g = l >> 4;
    const u32 rg0 = blockIdx.x * da.RGB, NU = da.NU;
    const u32 RGt = (a.N + 15u) >> 4;
    const u32 rgb = min(da.RGB, RGt - rg0);  // row groups of this block
    const u32 nitems = rgb * NU;
    constexpr int NRAW = (1 << BITS) / 2;
    const u32 plane_bytes = a.N * G.wpr * 4u;
    rsrc_t rq = make_rsrc(a.qw, plane_bytes * (u32)BITS);
    rsrc_t rl = make_rsrc(a.lut, a.N * (u32)NRAW * 4u);
    u32x4 P[BITS];
    u32 lraw[NRAW];
    // (item it = (row group rgl, unit u) = (it / NU, it % NU): the loop below carries the pair along -- an integer division is ~30
    // instructions on this chip, and NU = 28 for the 14336-wide rows)
    auto issue = [&](u32 it, u32 rgl, u32 u) {
        const u32 row = (rg0 + rgl) * 16u + r;
        const bool ok = it < nitems && row < a.N && !(DQ_KO & 4);  // (knock-out 4: no plane loads)
        request_row<BITS>(rq, rl, ok, row, 4u * u + g, G.wpr, plane_bytes, P, lraw);
    };
    // the waves that stage x (the lower half) request their first item behind the activations, the others at once (the CU's
    // memory pipe serves requests in order)
    const bool stager = w < DQ_WAVES / 2u;
    if (!stager) issue(w, w / NU, w % NU);
    stage_items<PRO, DqImage>(G, a.x, a.normw, a.eps, xlds, red, stager, DQ_WAVES / 2u * 64u);
    if (stager) issue(w, w / NU, w % NU);
    __syncthreads();
    // B fragments: column 0 reads the image, the other columns read zeros from beyond the block's LDS allocation (192 KiB up)
    const u32 Q = QT ? (u32)QT : G.Q;
    auto decode_item = [&](u32 it, u32 u, const u32 (&Pw)[BITS][4], const u32 (&lw)[NRAW]) {
        LutPools<BITS> L;
        L.build(lw);
        const u32 q = 4u * u + g;
        const unsigned char *bb = r == 0u ? reinterpret_cast<const unsigned char *>(xlds) + (size_t)q * 16u
                                          : reinterpret_cast<const unsigned char *>(smem) + 0x30000u;
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        DqItem<BITS>::run(Pw, L, [&](int v, int jj, u32 a01, u32 a23, u32 b01, u32 b23) {
            const u32x4 av = {a01, a23, b01, b23};
#if DQ_KO & 1  // (timing knock-out, WRONG numerics: no B reads)
            const u32x4 bvv = {(u32)v, (u32)jj, q, Q};
#else
            const uint4 bv = *reinterpret_cast<const uint4 *>(bb + (size_t)((u32)(v * 4 + jj) * Q) * 16u);
            const u32x4 bvv = {bv.x, bv.y, bv.z, bv.w};
#endif
#if DQ_KO & 2  // (no MFMAs)
            acc0[0] += __builtin_bit_cast(float, av[0] ^ av[1] ^ av[2] ^ av[3] ^ bvv[0]);
#else
            if (jj & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, av), __builtin_bit_cast(f16x8, bvv), acc1, 0, 0, 0);
            else acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, av), __builtin_bit_cast(f16x8, bvv), acc0, 0, 0, 0);
#endif
        });
        // D[row 4 g + e][column r]: column 0 holds the sums
        if (r == 0u) *reinterpret_cast<f32x4 *>(part + (size_t)it * 16u + 4u * g) = acc0 + acc1;
    };
    // (GQ_STAMPS builds: s_memrealtime per wave of the middle block -- kernel start, then per item {top, plane words in hand, next item
    // requested, decoded}: tools/r6/dq_stamps.py)
    unsigned long long *dqdbg = (GQ_STAMPS && da.dbg && blockIdx.x == gridDim.x / 2u && l == 0u) ? da.dbg + (size_t)w * 32u : nullptr;
    u32 nst = 0;
    auto dstamp = [&]() {
        if (GQ_STAMPS && dqdbg && nst < 32u) dqdbg[nst++] = __builtin_amdgcn_s_memrealtime();
    };
    dstamp();
    const u32 step_rg = DQ_WAVES / NU, step_u = DQ_WAVES - step_rg * NU;  // one division per launch
    const u32 w_rg = w / NU;
    u32 c_u = w - w_rg * NU;                                                // the unit of the item being decoded
    u32 n_rg = w_rg + step_rg, n_u = c_u + step_u;                          // (row group, unit) of the one being requested
    if (n_u >= NU) n_u -= NU, n_rg++;
    for (u32 it = w; it < nitems; it += DQ_WAVES) {
        dstamp();
        u32 Pw[BITS][4];
#pragma unroll
        for (int p = 0; p < BITS; p++) {
            Pw[p][0] = P[p].x;
            Pw[p][1] = P[p].y;
            Pw[p][2] = P[p].z;
            Pw[p][3] = P[p].w;
        }
        u32 lw[NRAW];
#pragma unroll
        for (int i = 0; i < NRAW; i++) lw[i] = lraw[i];
        if (GQ_STAMPS) {
#pragma unroll
            for (int p = 0; p < BITS; p++) asm volatile("" : "+v"(Pw[p][0]), "+v"(Pw[p][3]));  // (the wait for the plane words sits here)
            dstamp();
        }
        issue(it + DQ_WAVES, n_rg, n_u);  // (the registers are copied out: the next item's words travel while this one is decoded)
        if (GQ_STAMPS) dstamp();
        const u32 u_now = c_u;
        c_u = n_u;
        n_rg += step_rg, n_u += step_u;
        if (n_u >= NU) n_u -= NU, n_rg++;
        decode_item(it, u_now, Pw, lw);
        if (GQ_STAMPS) dstamp();
    }
    __syncthreads();
    // ordered K-split sum + epilogue: one thread per row of the block.  The residual is requested BEFORE the sums are read, and the
    // partial sums of eight units come in one LDS round trip (added in unit order as before): with one dependent ds_read per unit and the
    // residual behind the sum, the tail of a w2 launch (28 units) was 28 LDS round trips + one memory round trip long.
    const bool pairs = (a.epilogue & GQ_EPI_SILU_PAIRS) != 0u;
    for (u32 rl = tid; rl < rgb * 16u; rl += 64u * DQ_WAVES) {
        const u32 row = rg0 * 16u + rl;
        uint16_t res = 0;
        if (!pairs && a.resid && row < a.N) res = a.resid[row];
        const float *pp = part + (size_t)(rl >> 4) * NU * 16u + (rl & 15u);
        float y = 0.f;
        u32 u = 0;
        for (; u + 8u <= NU; u += 8u) {
            float v[8];
#pragma unroll
            for (u32 j = 0; j < 8u; j++) v[j] = pp[(size_t)(u + j) * 16u];
#pragma unroll
            for (u32 j = 0; j < 8u; j++) y += v[j];
        }
        for (; u < NU; u++) y += pp[(size_t)u * 16u];
        _Float16 yh = (_Float16)y;
        if (pairs) {
            // rows (2 i, 2 i + 1) = (gate_i, up_i): F.silu(gate) * up on fp16 values (inference/model.py:266), written to out[i]
            const uint16_t yo = (uint16_t)__builtin_amdgcn_update_dpp(0, (int)__builtin_bit_cast(uint16_t, yh), 0xB1, 0xF, 0xF, true);  // lane ^ 1
            if (!(rl & 1u) && row + 1u < a.N) {
                const _Float16 o = silu_pair(yh, __builtin_bit_cast(_Float16, yo));
                gq_store_wt(a.out + (row >> 1), __builtin_bit_cast(uint16_t, o));
            }
        } else if (row < a.N) {
            if (a.resid) yh = __builtin_bit_cast(_Float16, res) + yh;
            gq_store_wt(a.out + row, __builtin_bit_cast(uint16_t, yh));
        }
    }
}

struct DqCfg {
    u32 grid, RGB, NU, part_off;
    size_t smem;
};
bool pick_dq_cfg(u32 N, u32 K, int bits, DqCfg &c) {
    if (bits < 2 || bits > 4 || K % 1024u || K > 32768u || N < 16u) return false;
    const u32 RGt = (N + 15u) / 16u, cus = (u32)gq_cu_count();
    c.NU = K / 512u;
    // blocks per CU the instance's occupancy allows (waves per SIMD x 4 SIMDs / waves per block)
    u32 bpc = (u32)gq_env_int("GQ_DQ_BPC", 0);
    if (!bpc) bpc = (u32)dq_wpe(bits) * 4u / DQ_WAVES;
    if (bpc < 1u) bpc = 1u;
    c.RGB = (RGt + cus * bpc - 1u) / (cus * bpc);
    c.grid = (RGt + c.RGB - 1u) / c.RGB;
    c.part_off = (K * 2u + 255u) / 256u * 256u;
    c.smem = (size_t)c.part_off + (size_t)c.RGB * c.NU * 64u + 64u;
    return c.smem <= 150u * 1024u;
}
template <int BITS, int PRO, int QT>
int launch_dq_q(const DqArgs &da, const DqCfg &c, hipStream_t s) {
    if (gq_ap_route(GQ_AP_ROUTE_DQ, 1u)) return GQ_OK;
    static GqPerDeviceOnce once;
    auto kern = ap_gemv_dq_kernel<BITS, PRO, QT>;
    GQ_HIP_CHECK(once.max_dynamic_lds(reinterpret_cast<const void *>(kern), (int)(160u * 1024u)));
    hipLaunchKernelGGL(kern, dim3(c.grid), dim3(64u * DQ_WAVES), c.smem, s, da);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}
template <int BITS, int PRO>
int launch_dq_inst(const DqArgs &da, const DqCfg &c, hipStream_t s) {
    switch (da.a.K) {
        case 4096u: return launch_dq_q<BITS, PRO, 32>(da, c, s);
        case 14336u: return launch_dq_q<BITS, PRO, 112>(da, c, s);
        default: return launch_dq_q<BITS, PRO, 0>(da, c, s);
    }
}
template <int BITS>
int launch_dq(const DqArgs &da, const DqCfg &c, int pro, hipStream_t s) {
    switch (pro) {
        case PRO_RMSNORM: return launch_dq_inst<BITS, PRO_RMSNORM>(da, c, s);
        case PRO_SILUMUL: return launch_dq_inst<BITS, PRO_SILUMUL>(da, c, s);
        default: return launch_dq_inst<BITS, PRO_NONE>(da, c, s);
    }
}
}  // namespace
// GQ_ENOTSUP when the shape is not served (the caller goes on to the plane / exact kernels)
int gq_ap_dq_try(const ApLaunch &L) {
    DqCfg c;
    if (L.M != 1u || !pick_dq_cfg(L.N, L.K, L.bits, c)) return GQ_ENOTSUP;
    if (L.qbytes() >= 0x7FFFFFFFull) return GQ_ENOTSUP;
    if (L.unaligned16()) return GQ_ENOTSUP;
    if (L.pairs && (L.N & 1u)) return GQ_ENOTSUP;
    DqArgs da{ap_args(L, 0u, 0u), c.RGB, c.NU, c.part_off, GQ_STAMPS ? gq_debug_timing_buffer() : nullptr};
    return gq_with_bits<2, 4>(L.bits, [&](auto B) { return launch_dq<B()>(da, c, L.pro, L.stream); });
}
