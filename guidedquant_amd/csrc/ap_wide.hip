// ap_wide.hip -- the Any-Precision GEMV at 5 to 8 bits, one batch row (the decode step's launches), in the reference's fp16 order.
//
// Below 5 bits the exact kernels look codes up in v_perm byte pools held in VGPRs (ap_core.h::LutPools); 2^BITS fp16 centroids are 16 /
// 32 / 64 / 128 VGPRs per row at 5 / 6 / 7 / 8 bits, which does not fit beside the activations and the plane ring.  Here the row's LUT
// is a table in LDS (256-byte slots, 512 at 8 bits), one ds_read_u16 per weight.  The rest is ap_gemv_pt2_kernel's frame (ap_exact.h):
//   * lane = (row slot rs, quad q): 4 CUDA lanes (words) x 32 weights of one row per step, one 16-byte load per plane, RS rows per step;
//   * the lane's activations stay in 64 VGPRs (natural-order LDS image, the fused prologues of stage_x_natural);
//   * per word ONE half2 accumulator (even chain, odd chain), byte c = 3..0, pair k = 0..3, then sum.x + sum.y (anyprec.cu:495-505);
//   * the per-(row, chunk, word) partials meet in LDS and go through rows_epilogue: chunks ascending, the 16/8/4/2/1 tree, and at
//     bits >= 7 with K > 4096 the reference's K-split (groups of 4 chunks, anyprec.cu:611); plain, residual and gate/up pair epilogues.
// So every result is bit-identical to ap_gemv_generic_kernel, which served these widths before (GQ_AP_FORCE_GENERIC=1 still picks it).
//
// Code formation: a selector word S[s] of one plane word set holds in byte (3 - c) the code of the weight at bit s of byte c (the
// DqItem trick of ap_dq.hip: no byte transpose), built with one shift + one and-or per plane; below 8 bits the code is formed
// already doubled (the byte offset of its fp16 entry), so one v_perm with the table's 256-aligned base is the LDS address.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "ap_core.h"
#include "ap_exact.h"

using namespace gq;

namespace {

typedef gqw::h2v f16x2;

using gqw::lds_addr;
__device__ __forceinline__ _Float16 lds_f16(u32 addr) { return *(const __attribute__((address_space(3))) _Float16 *)(uintptr_t)addr; }

template <int BITS>
struct WideGeom {
    static constexpr u32 NC = 1u << BITS;                 // centroids per row
    static constexpr u32 NW = NC / 2u;                    // LUT words per row
    static constexpr u32 TS = BITS <= 7 ? 256u : 512u;    // table slot (bytes): 256-aligned, so that byte 0 of a slot base is 0
    static constexpr u32 LW = (8u * NW + 255u) / 256u;    // LUT words a lane loads per step (RS <= 8 rows, blockDim >= 256)
    static constexpr int SH = BITS <= 7 ? 1 : 0;          // codes formed doubled (byte offsets) below 8 bits
};

template <int BITS, int PRO, bool KS>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2))) ap_gemv_wide_kernel(ApArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using WG = WideGeom<BITS>;
    RowGeom G;
    G.init(a.K);
    uint16_t *xlds = reinterpret_cast<uint16_t *>(smem);
    uint16_t *sv = xlds + G.K;  // [SPB*RS][nchunks*32]
    const u32 svrow = G.nchunks * 32u;
    float *red = reinterpret_cast<float *>(sv);  // scratch for the RMSNorm reduction (before sv is used)
    const u32 T = blockDim.x, tid = threadIdx.x;
    const u32 RS = a.RS, SPB = a.SPB;
    const u32 row0 = blockIdx.x * SPB * RS;
    const bool active = tid < RS * G.Q;
    const u32 rs = active ? tid / G.Q : 0u;
    const u32 q = active ? tid - rs * G.Q : 0u;
    // the LUT tables: two buffers (steps alternate) of RS slots behind sv, at a 256-byte aligned LDS address
    const u32 sbase = lds_addr(smem);
    const u32 tab0 = (sbase + G.K * 2u + SPB * RS * svrow * 2u + 255u) & ~255u;
    unsigned char *tabp = smem + (tab0 - sbase);

    constexpr u32 OOB = 0x80000000u;
    const u32 plane_bytes = a.N * G.wpr * 4u;
    rsrc_t rq = make_rsrc(a.qw, plane_bytes * (u32)BITS);
    rsrc_t rl = make_rsrc(a.lut, a.N * WG::NC * 2u);
    // the lane's share of a step's LUT rows (RS consecutive rows = one contiguous run of RS * NW words): words w0 .. w0 + LW - 1
    const u32 w0 = tid * WG::LW, lr = w0 / WG::NW;
    u32x4 P[BITS];
    u32 lw[WG::LW];
    auto issue = [&](u32 step) {
        const u32 row = row0 + step * RS + rs;
        const bool ok = active && step < SPB && row < a.N;
        const u32 off = (row * G.wpr + 4u * q) * 4u;
#pragma unroll
        for (int p = 0; p < BITS; p++) P[p] = __builtin_amdgcn_raw_buffer_load_b128(rq, ok ? off + (u32)p * plane_bytes : OOB, 0, 2 /* nt */);
        const bool lok = step < SPB && lr < RS && row0 + step * RS + lr < a.N;
        const u32 loff = lok ? ((row0 + step * RS) * WG::NW + w0) * 4u : OOB;
        if constexpr (WG::LW == 1) {
            lw[0] = __builtin_amdgcn_raw_buffer_load_b32(rl, loff, 0, 0);
        } else if constexpr (WG::LW == 2) {
            auto v = __builtin_amdgcn_raw_buffer_load_b64(rl, loff, 0, 0);
            lw[0] = v[0], lw[1] = v[1];
        } else {
            u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rl, loff, 0, 0);
            lw[0] = v.x, lw[1] = v.y, lw[2] = v.z, lw[3] = v.w;
        }
    };

    // activations -> LDS (natural image, prologue applied) -> 64 VGPRs; the waves that do not stage queue their first loads in front
    const u32 nw = T >> 6, wv = tid >> 6;
    const bool stager = nw < 2u || wv < nw / 2u;
    if (!stager) issue(0u);
    stage_x_natural<PRO>(G, a.x, a.normw, a.eps, xlds, red, stager, nw < 2u ? T : (nw / 2u) * 64u);
    if (stager) issue(0u);
    __syncthreads();
    u32 chunk, t0, tpw;
    G.quad(q, chunk, t0, tpw);
    uint4 xr[4][4];  // xr[v][c]: the 8 activations of (word v, byte c) = the half2 operands of pairs k = 0..3
#pragma unroll
    for (u32 v = 0; v < 4; v++)
#pragma unroll
        for (u32 c = 0; c < 4; c++) xr[v][c] = *reinterpret_cast<const uint4 *>(xlds + 1024u * chunk + 8u * tpw * c + 8u * (t0 + v));
    uint16_t *svp = sv + (size_t)rs * svrow + chunk * 32u + t0;

    for (u32 i = 0; i < SPB; i++) {
        u32 Pw[BITS][4];
#pragma unroll
        for (int p = 0; p < BITS; p++) Pw[p][0] = P[p].x, Pw[p][1] = P[p].y, Pw[p][2] = P[p].z, Pw[p][3] = P[p].w;
        // this step's tables into buffer i & 1 (its readers of step i - 2 passed the barrier of step i - 1)
        const u32 buf = (i & 1u) * RS * WG::TS;
        if (lr < RS) {
            unsigned char *dst = tabp + buf + lr * WG::TS + (w0 % WG::NW) * 4u;
            if constexpr (WG::LW == 1) *reinterpret_cast<u32 *>(dst) = lw[0];
            else if constexpr (WG::LW == 2) *reinterpret_cast<uint2 *>(dst) = make_uint2(lw[0], lw[1]);
            else *reinterpret_cast<uint4 *>(dst) = make_uint4(lw[0], lw[1], lw[2], lw[3]);
        }
        issue(i + 1u);
        __syncthreads();
        const u32 tb = tab0 + buf + rs * WG::TS;
        u32 s[4];
#pragma unroll
        for (int v = 0; v < 4; v++) {
            // S[b]: byte (3 - c) = code (doubled below 8 bits) of the weight at bit b of byte c -- plane p (0 = MSB) to bit BITS - 1 - p + SH
            u32 S[8];
#pragma unroll
            for (int b = 0; b < 8; b++) {
                S[b] = 0u;
#pragma unroll
                for (int p = 0; p < BITS; p++) {
                    const int dst = BITS - 1 - p + WG::SH;
                    S[b] |= shl(Pw[p][v], dst - b) & (0x01010101u << dst);
                }
            }
            u32 acc = 0u;
#pragma unroll
            for (int c = 3; c >= 0; c--) {
                const u32 xw[4] = {xr[v][c].x, xr[v][c].y, xr[v][c].z, xr[v][c].w};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const u32 Se = S[7 - 2 * k], So = S[6 - 2 * k];  // weight j = 2k (bit 7 - 2k of byte c), j = 2k + 1
                    u32 ae, ao;
                    if constexpr (BITS <= 7) {
                        const u32 sel = 0x07060500u | (u32)(3 - c);  // byte 0 = the doubled code, bytes 1..3 = the slot base's
                        ae = perm(tb, Se, sel), ao = perm(tb, So, sel);
                    } else {
                        // (a slot base is 256-aligned only: the 9-bit byte offset is added, not or-ed in)
                        ae = tb + (((Se >> (8 * (3 - c))) & 0xFFu) << 1), ao = tb + (((So >> (8 * (3 - c))) & 0xFFu) << 1);
                    }
                    const f16x2 w = {lds_f16(ae), lds_f16(ao)};
                    acc = pk_fma(__builtin_bit_cast(u32, w), xw[k], acc);
                }
            }
            s[v] = (u32)h_add((uint16_t)(acc & 0xFFFFu), (uint16_t)(acc >> 16));
        }
        if (active) *reinterpret_cast<uint2 *>(svp + (size_t)i * RS * svrow) = make_uint2(s[0] | (s[1] << 16), s[2] | (s[3] << 16));
    }
    __syncthreads();
    rows_epilogue<KS>(G, a, sv, svrow, SPB * RS, row0, 0u, tid, T);
}

struct WideCfg {
    u32 T, RS, SPB, grid;
    size_t smem;
};

// rows of up to 32768 weights in whole quads: RS row slots of Q = K / 128 lanes, blocks of 256 (512 past 128 quads) threads -- RS even,
// so that a block holds whole gate / up pairs; about two blocks per CU, every block the same number of steps
bool wide_plan(u32 N, u32 K, int bits, WideCfg &c) {
    if (K % 128u || K == 0u || K > 32768u) return false;
    const u32 Q = K / 128u;
    c.RS = Q <= 32u ? 8u : (Q <= 64u ? 4u : 2u);
    c.T = Q <= 128u ? 256u : 512u;
    const u32 nchunks = K / 1024u + ((K % 1024u) ? 1u : 0u);
    const u32 ts = bits <= 7 ? 256u : 512u;
    auto smem_for = [&](u32 spb) { return (((size_t)K * 2u + (size_t)spb * c.RS * nchunks * 64u + 255u) & ~(size_t)255u) + 2u * c.RS * ts + 256u; };
    const u32 steps = (N + c.RS - 1u) / c.RS;
    const u32 target = (u32)gq_cu_count() * 2u;
    u32 spb = std::max(1u, (steps + target - 1u) / target);
    while (spb > 1u && smem_for(spb) > 80u * 1024u) spb--;
    if (smem_for(spb) > 160u * 1024u) return false;
    c.SPB = spb;
    c.grid = (steps + spb - 1u) / spb;
    c.smem = smem_for(spb);
    return true;
}

template <int BITS, int PRO, bool KS>
int launch_wide_inst(const ApArgs &a, const WideCfg &c, hipStream_t s) {
    if (gq_ap_route(GQ_AP_ROUTE_WIDE, 1u)) return GQ_OK;
    static GqPerDeviceOnce once;
    auto kern = ap_gemv_wide_kernel<BITS, PRO, KS>;
    GQ_HIP_CHECK(once.max_dynamic_lds(reinterpret_cast<const void *>(kern), (int)(160u * 1024u)));
    hipLaunchKernelGGL(kern, dim3(c.grid), dim3(c.T), c.smem, s, a);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}

template <int BITS, int PRO>
int launch_wide_pro(const ApArgs &a, const WideCfg &c, hipStream_t s) {
    if constexpr (BITS >= 7) {
        if (a.K > 4096u) return launch_wide_inst<BITS, PRO, true>(a, c, s);  // anyprec.cu:611
    }
    return launch_wide_inst<BITS, PRO, false>(a, c, s);
}

template <int BITS>
int launch_wide(const ApArgs &a, const WideCfg &c, int pro, hipStream_t s) {
    switch (pro) {
        case PRO_RMSNORM: return launch_wide_pro<BITS, PRO_RMSNORM>(a, c, s);
        case PRO_SILUMUL: return launch_wide_pro<BITS, PRO_SILUMUL>(a, c, s);
        default: return launch_wide_pro<BITS, PRO_NONE>(a, c, s);
    }
}

}  // namespace

// the dispatcher's rung at bits 5..8 (ap_dispatch.hip): GQ_ENOTSUP where the kernel does not serve the launch (M > 1, K % 128 != 0 or K > 32768,
// misaligned buffers) -- the generic kernel takes the plain form of those
int gq_ap_wide_try(const ApLaunch &L) {
    if (L.bits < 5 || L.bits > 8 || L.M != 1u) return GQ_ENOTSUP;
    if (L.qbytes() >= 0x7FFFFFFFull || (uint64_t)L.N * (2u << L.bits) >= 0x7FFFFFFFull) return GQ_ENOTSUP;
    if (L.unaligned16()) return GQ_ENOTSUP;
    if (L.pairs && (L.N & 1u)) return GQ_ENOTSUP;
    WideCfg c;
    if (!wide_plan(L.N, L.K, L.bits, c)) return GQ_ENOTSUP;
    return gq_with_bits<5, 8>(L.bits, [&](auto B) { return launch_wide<B()>(ap_args(L, c.RS, c.SPB), c, L.pro, L.stream); });
}
