// qtip.hip -- QTIP trellis-decoded matvec and the Sylvester Hadamard transform for gfx950.
//
// Replaces kernel_decompress_matvec<16,9,R,1,M,1,K> (qtip/qtip-kernels/src/inference.cu:168-425) -- an mma.sync
// program with a 32x-replicated shared-memory codebook, inline-PTX streaming loads and 73 compile-time shapes -- by
// one runtime-shaped wave-64 kernel:
//   * a wave walks 2x2 tile blocks (32 rows x 32 columns, 128*R contiguous bytes); lane (a4 = lane/32, s = lane%32)
//     owns the 4 trellis states 4s..4s+3 of the tiles of tile-row parity a4, i.e. rows a, a+8 (a = s/4) and
//     columns 2b, 2b+1, 2b+8, 2b+9 (b = s%4) -- the A-fragment slot order of the format (finetune.py:291-296);
//   * the 16-bit sliding window needs the next lane's stream unit (one ds_bpermute per tile);
//   * state -> (state*(state+1)) >> 6 & 511 -> fp16 pair from a 2 KiB LDS table, sign bit folded in with one XOR
//     (quantlut_sym, bitshift.py:72-80); v_dot2_f32_f16 accumulates in fp32;
//   * the K range of a 32-row band is split over the waves of the block and combined in LDS in a fixed order.
// This file is the trellis side: the band engine, the bare matvec and the fused linear's matvec launch with its transform-in
// prologue.  The one-block transform kernels around it and gq_hadamard are qtip_xf.hip, the arithmetic both share qtip_xform.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <type_traits>

#include "gq_internal.h"
#include "fwht.h"
#include "qtip_xform.h"
#include "wave_util.h"

namespace {
typedef uint32_t u32;
using gqq::QPRO_NONE;
using gqq::QPRO_PRE;
using gqq::QPRO_RMSNORM;
using gqq::QPRO_ROWS;
using gqq::QPRO_SILUMUL;
using gqq::QtipOut;
using gqw::f32x4;
using gqw::h16;
using gqw::h16x2;
using gqw::h16x8;
using gqw::make_rsrc;
using gqw::rsrc_t;
using gqw::u32x2;
using gqw::u32x4;

// ------------------------------------------------------------------------------------------------ the band engine
// Round 2 redesign (round 1: one v_dot2 per state, one 2 KiB codebook with ~3.5-way bank conflicts, 8 VALU per state).
//
// Lane <-> trellis mapping.  The format hands lane s = 4 a + b of a 16x16 tile the states of rows a, a + 8 and columns
// 2b, 2b+1, 2b+8, 2b+9 -- the A fragment of the reference's mma.sync.  v_mfma_f32_16x16x32_f16 wants lane (g = l / 16,
// r = l % 16) to hold 8 k-slots of ONE row r, all 16 rows of a lane group g agreeing on the columns.  Which global bytes a
// lane loads is free, so lane l = 16 b + 8 a4 + a takes stream unit s = 4 a + b of tile row a4 (the two 16-row halves of
// the band are the two halves of the 16 logical rows), for BOTH column tiles a3 = 0, 1 of the 32-column tile block:
//   A operand "rows a"     = states i = 0, 2 of a3 = 0, 1  -> columns 2g + {0,1}, 16 + 2g + {0,1}, 8 + 2g + {0,1}, 24 + 2g + {0,1}
//   A operand "rows a + 8" = states i = 1, 3                (same columns),
//   B operand (all 16 columns equal) = those 8 activations: ONE ds_read_b128 of a copy of x stored in that order.
// Two MFMAs per 32 x 32 tile block replace 8 v_dot2 per lane and the cross-lane sums; fp32 accumulation as before.
//
// State arithmetic, R = 2 (two states per register; halves = column tiles a3 = 0 / 1):
//   pack  = {unit(a3 = 1), unit(a3 = 0)} (one v_perm), npack = the neighbour lane's pack (one ds_bpermute);
//   P_i   = 16-bit windows at bit offset 4 i of {pack : npack} per half (i = 0: pack itself; 7 ops for i = 1..3);
//   M_i   = v_pk_mad_u16(P_i, P_i, P_i) = st (st + 1) mod 2^16 per half: bits 6..14 = codebook entry, bit 15 = sign;
//   entry address = ((M & 0xFFC0) << 1) | 4 (lane % 32): the codebook is held 32 times, entry-major (128 bytes per entry,
//   lane l reads copy l % 32: ds_read_b32 is banked (a / 4) % 32 per 32-lane group, so every lookup is conflict-free), and
//   sign-expanded (1024 entries; entry 512 + e = entry e with the low half negated) when the 128 KiB fit beside the
//   activations (SX = 1), else 512 entries + 3 ops per register for the sign (SX = 0).
// R = 3, 4 build the same P_i registers through 64-bit shifts (generic path).
//
// Work distribution: `nitems` items = (32-row band, K range); block b walks items b, b + gridDim, ... with ONE codebook
// fill and ONE activation prologue; the 16 waves of a block split an item's tile blocks (K2 = k2lo + w, + W, ...), their
// register prefetch queue (PF tile blocks per wave) runs across item boundaries.  The sum of a band is formed in a fixed
// order: tile blocks in ascending order within a wave (MFMA accumulator), waves in ascending order through LDS.
template <int SX>
struct QtipTab {
    static constexpr u32 ENT = SX ? 1024u : 512u;
    static constexpr u32 WORDS = ENT * 32u;
};

// Codebook fill.  Lane c % 8 of a group of 8 writes 16-byte chunk c % 8 of entry c / 8: a wave-instruction covers 1 KiB of
// contiguous LDS (entry-per-lane stores -- stride 128 bytes -- put all lanes on the same 4 banks: measured 8,500 cycles for
// the fill, 5x).  With 1024 threads chunk tid + 1024 k belongs to entry tid / 8 + 128 k: four words per thread, REQUESTED
// BEFORE the first tile blocks (vector memory returns in order: behind them the words would arrive after ~4,000 cycles), the
// sign-expanded upper half of the table from the same four registers.
struct QtipTabRegs {
    u32 w[4];
};
__device__ __forceinline__ void qtip_table_request(QtipTabRegs &r, const uint16_t *tlut) {
    if (blockDim.x == 1024u) {
#pragma unroll
        for (u32 k = 0; k < 4; k++) r.w[k] = reinterpret_cast<const u32 *>(tlut)[(threadIdx.x >> 3) + 128u * k];
    }
}
template <int SX>
__device__ __forceinline__ void qtip_fill_table(u32 *tab, const uint16_t *tlut, const QtipTabRegs &r) {
    const u32 T = blockDim.x, tid = threadIdx.x;
    if (T == 1024u) {
#pragma unroll
        for (u32 k = 0; k < 4; k++) {
            const u32 wv = r.w[k];
            reinterpret_cast<u32x4 *>(tab)[tid + 1024u * k] = u32x4{wv, wv, wv, wv};
            if (SX) {
                const u32 ws = wv ^ 0x8000u;
                reinterpret_cast<u32x4 *>(tab)[tid + 1024u * (k + 4u)] = u32x4{ws, ws, ws, ws};
            }
        }
        return;
    }
    for (u32 c = tid; c < QtipTab<SX>::ENT * 8u; c += T) {
        const u32 e = c >> 3;
        u32 wv = reinterpret_cast<const u32 *>(tlut)[e & 511u];
        if (SX && (e & 512u)) wv ^= 0x8000u;
        reinterpret_cast<u32x4 *>(tab)[c] = u32x4{wv, wv, wv, wv};
    }
}

// Position of activation k inside the permuted copy: tile block K2 = k / 32, pair q = (k % 32) / 2 -> lane group g = q % 4, slot
// {0, 2, 1, 3}[q / 4] (the order of the A registers above), element k % 2.
// 8 consecutive activations (k = 8 u .. 8 u + 7, packed as 4 words) -> the permuted copy (4 ds_write_b32)
__device__ __forceinline__ void qtip_store_x8(uint16_t *xsp, u32 u, const u32 (&o)[4]) {
    u32 *dst = reinterpret_cast<u32 *>(xsp) + (u >> 2) * 16u;
    const u32 qc = u & 3u, slot = ((qc & 1u) << 1) | (qc >> 1);
#pragma unroll
    for (u32 e = 0; e < 4; e++) dst[e * 4u + slot] = o[e];
}

struct QtItem {
    u32 boff;    // byte offset of the band inside the linear's trellis tensor
    float *out;  // 32 sums
    u32 k2lo, k2hi;
};

// The trellis stream is requested in CHUNKS of CH consecutive tile blocks, one wave-instruction of LW bytes per lane each
// (R = 2: 4 tile blocks = 64 x 16 bytes; R = 3: 2 = 64 x 12; R = 4: 2 = 64 x 16).  Measured (tools/ubench/qtip_stream.hip):
// 8 bytes per lane -- one tile block per instruction, what this kernel did before -- streams the 12.6 MB of q/k/v in 6.1 us,
// 16 bytes per lane in 3.9 us, whatever the queue depth.  The loaded rows are then in "loader order" (lane = tile block x
// row of units); a 1 KiB LDS slot per wave turns them into the MFMA lane order: the loader lane stores its 16 bytes (R = 2:
// already as the four {column tile 1 : column tile 0} packs of its two unit rows and both 16-row halves), each consumer lane
// reads its own and its neighbour's (one dword each at R = 2).  LDS operations of ONE wave are served in order, so the slot
// needs no barrier and no second buffer: the reads of a chunk are issued before the store of the next one.
template <int R>
struct QtChunk {
    static constexpr u32 CH = R == 2 ? 4u : 2u;
    static constexpr u32 LD = R == 3 ? 3u : 4u;          // dwords per lane and load
    static constexpr u32 BYTES = CH * 128u * (u32)R;     // = 64 * 4 * LD
};
constexpr u32 PF = 2;  // chunks per wave in flight (the engine's register prefetch queue)

template <int R>
__device__ __forceinline__ void qtip_load_chunk(u32 (&d)[QtChunk<R>::LD], rsrc_t rs, u32 voff, u32 soff) {
    if constexpr (R == 3) {
        const auto v = __builtin_amdgcn_raw_buffer_load_b96(rs, voff, soff, 2 /* nt */);
        d[0] = v[0], d[1] = v[1], d[2] = v[2];
    } else {
        const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 2);
        d[0] = v[0], d[1] = v[1], d[2] = v[2], d[3] = v[3];
    }
}

// comp / comp_bytes: the trellis tensor the items of this block index into (one linear per block).
// stg: [waves] 1 KiB slots.  Items' K ranges start at multiples of CH tile blocks.
// WC: waves per block if known at compile time (16: the activation reads of a loop use immediate offsets), 0: blockDim / 64.
template <int R, int SX, int WC, class ItemFn, class F>
__device__ __forceinline__ void qtip_engine(const u32 *tab, const uint16_t *xsp, float *part, unsigned char *stg, const u32 *comp, u32 comp_bytes,
                                            u32 nitems, ItemFn item_of, F between, unsigned long long *dbg = nullptr) {
    constexpr u32 CH = QtChunk<R>::CH, LD = QtChunk<R>::LD, CB = QtChunk<R>::BYTES;
    const u32 T = blockDim.x, tid = threadIdx.x, W = WC ? (u32)WC : T >> 6, l = tid & 63u;
    const u32 w = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));  // (wave-uniform: the loop tests stay on the scalar unit)
    const u32 g = l >> 4, a4 = (l >> 3) & 1u, a = l & 7u, s = 4u * a + g;
    const u32 sn = (s + 1u) & 31u;  // the window of unit s ends in unit s + 1 of the same tile (cyclic)
    const u32 lane4 = (l & 31u) * 4u, voff = l * (4u * LD);
    const u32 sel3a = a4 ? 0x0C050403u : 0x0C020100u, sel3b = a4 ? 0x0C070605u : 0x0C040302u;  // (R = 3 unit selectors)
    const unsigned char *tabb = reinterpret_cast<const unsigned char *>(tab);
    unsigned char *slot = stg + w * 1024u;
    // R = 2: the slot holds, per loader lane (tile block tb = lane / 16, unit rows 2 j, 2 j + 1), 16 bytes
    // {pack(2j, half 0), pack(2j + 1, half 0), pack(2j, half 1), pack(2j + 1, half 1)} at 256 tb + 16 j
    // R = 4: raw rows of four dword units; this lane wants units a4 and 2 + a4 (column tiles 0 / 1) of its row and the neighbour's
    const unsigned char *own_p = slot + (R == 2 ? 16u * (s >> 1) + 8u * a4 + 4u * (s & 1u) : s * (4u * R) + (R == 4 ? 4u * a4 : 0u));
    const unsigned char *nbr_p = slot + (R == 2 ? 16u * (sn >> 1) + 8u * a4 + 4u * (sn & 1u) : sn * (4u * R) + (R == 4 ? 4u * a4 : 0u));
    const rsrc_t rs = make_rsrc(comp, comp_bytes);
    u32 dq[PF][LD];
    u32 nstamp = 0;
    // The five stamp sites of the band engine stay compiled IN (switched off at run time by the null debug pointer) while every other
    // kernel's sites are out (GQ_STAMPS): without them the bare matvec ran 4-5 % slower (profiles/r06_qtip_matvec_regression.txt;
    // 4096^2 6.1 vs 5.8 us, 11008 x 4096 9.3 vs 8.85) -- the branch around a site ends a basic block, which changes what the scheduler
    // hoists; scheduling barriers at the same places did not reproduce it.
    auto stamp = [&]() {
        if (dbg && blockIdx.x == gridDim.x / 2 && l == 0 && nstamp < 8u) dbg[w * 8u + nstamp++] = __builtin_readcyclecounter();
    };
    stamp();
    u32 j = blockIdx.x;
    if (j >= nitems) return;  // (whole block)
    u32 ord = 0;  // ordinal of the block's current item (item_of takes it: no division to recover it from j)
    QtItem cur = item_of(j, 0u);
    // Queue refill without vector ALU work: the lane part of the address is a constant VGPR, the chunk a scalar offset.
    // A slot with nothing left to fetch re-reads the last chunk of the item (a cache hit, never used).
    auto fetch = [&](u32 p, const QtItem &it, u32 c) {
        const u32 chi = (it.k2hi + CH - 1u) / CH, cc = c < chi ? c : chi - 1u;
        qtip_load_chunk<R>(dq[p], rs, voff, it.boff + cc * CB);
    };
#pragma unroll
    for (u32 p = 0; p < PF; p++) fetch(p, cur, cur.k2lo / CH + w + p * W);
    stamp();
    between();
    stamp();
    f32x4 accA[2], accB[2];  // even / odd tile blocks: no MFMA waits for the one before it
    const u32 emask = SX ? 0xFFC0FFC0u : 0x7FC07FC0u;
    auto lookup2 = [&](u32 P, u32 &wlo, u32 &whi) {
        u32 m;
        u32 alo, ahi;
        asm("v_pk_mad_u16 %0, %1, %1, %1" : "=v"(m) : "v"(P));
        const u32 y = m & emask;
        // byte address = 2 * (entry << 6) + 4 * (lane % 32), per 16-bit half (v_mad_u32_u16: half select, times 2, plus lane)
        asm("v_mad_u32_u16 %0, %1, 2, %2 op_sel:[0,0,0,0]" : "=v"(alo) : "v"(y), "v"(lane4));
        asm("v_mad_u32_u16 %0, %1, 2, %2 op_sel:[1,0,0,0]" : "=v"(ahi) : "v"(y), "v"(lane4));
        wlo = *reinterpret_cast<const u32 *>(tabb + alo);
        whi = *reinterpret_cast<const u32 *>(tabb + ahi);
        if (!SX) {
            const u32 sg = m & 0x80008000u;
            wlo ^= sg & 0xFFFFu;
            whi ^= sg >> 16;
        }
    };
    // A chunk and its tile blocks in stages, so that the LDS round trips of several tile blocks are in flight:
    //   chunk_in: the loaded registers -> the wave's LDS slot (the queue slot is refilled right away);
    //   stage_a : this lane's units and its neighbour's (both column tiles) out of the slot;
    //   stage_b : the four state-pair registers -> 8 codebook lookups + the activations (ds_read);
    //   stage_c : two MFMAs.
    struct TbA {
        u32 own[R == 2 ? 1 : 2], nbr[R == 2 ? 1 : 2];
    };
    struct TbB {
        u32x4 wa, wb, xb;
    };
    auto chunk_store = [&](const u32 (&d)[LD]) {
        if constexpr (R == 2) {
            const u32x4 q = {__builtin_amdgcn_perm(d[1], d[0], 0x05040100u), __builtin_amdgcn_perm(d[3], d[2], 0x05040100u),
                             __builtin_amdgcn_perm(d[1], d[0], 0x07060302u), __builtin_amdgcn_perm(d[3], d[2], 0x07060302u)};
            *reinterpret_cast<u32x4 *>(slot + l * 16u) = q;
        } else {
#pragma unroll
            for (u32 i = 0; i < LD; i++) reinterpret_cast<u32 *>(slot + l * (4u * LD))[i] = d[i];
        }
    };
    auto stage_a = [&](u32 tbk, TbA &t) {
        if constexpr (R == 2) {
            t.own[0] = *reinterpret_cast<const u32 *>(own_p + tbk * 256u);
            t.nbr[0] = *reinterpret_cast<const u32 *>(nbr_p + tbk * 256u);
        } else if constexpr (R == 4) {
            const u32 *po = reinterpret_cast<const u32 *>(own_p + tbk * 512u), *pn = reinterpret_cast<const u32 *>(nbr_p + tbk * 512u);
            t.own[0] = po[0], t.own[1] = po[2], t.nbr[0] = pn[0], t.nbr[1] = pn[2];  // (one ds_read2_b32 each)
        } else {
            // R = 3: a row is 12 bytes, unit j its bytes 3j .. 3j + 2; this lane wants units a4 and 2 + a4: one v_perm each with a
            // per-lane selector (0x0C = zero byte)
            u32 d0[R], d1[R];
#pragma unroll
            for (int i = 0; i < R; i++) {
                d0[i] = reinterpret_cast<const u32 *>(own_p + tbk * (128u * R))[i];
                d1[i] = reinterpret_cast<const u32 *>(nbr_p + tbk * (128u * R))[i];
            }
            t.own[0] = __builtin_amdgcn_perm(d0[1], d0[0], sel3a), t.own[1] = __builtin_amdgcn_perm(d0[2], d0[1], sel3b);
            t.nbr[0] = __builtin_amdgcn_perm(d1[1], d1[0], sel3a), t.nbr[1] = __builtin_amdgcn_perm(d1[2], d1[1], sel3b);
        }
    };
    auto stage_b = [&](const TbA &t, const uint16_t *xrow, TbB &o) {
        u32 P[4];
        if constexpr (R == 2) {
            // windows at bit offsets 4 i of {pack : npack}, both halves at once: (pack << 4 i) | (npack >> (16 - 4 i)) under a
            // per-half mask (one 3-input bit operation; shifts are 4-byte encodings: half the issue cost of VOP3 forms)
            const u32 pack = t.own[0], npack = t.nbr[0];
            P[0] = pack;
            P[1] = ((pack << 4) & 0xFFF0FFF0u) | ((npack >> 12) & 0x000F000Fu);
            P[2] = __builtin_amdgcn_perm(pack, npack, 0x06030401u);
            P[3] = ((pack << 12) & 0xF000F000u) | ((npack >> 4) & 0x0FFF0FFFu);
        } else if constexpr (R == 4) {
            // byte-aligned windows of {unit : neighbour's unit}: states 0..2 inside the unit, state 3 = its last byte + the
            // neighbour's first: six v_perm for both column tiles
            const u32 u0 = t.own[0], u1 = t.own[1];
            P[0] = __builtin_amdgcn_perm(u1, u0, 0x07060302u);
            P[1] = __builtin_amdgcn_perm(u1, u0, 0x06050201u);
            P[2] = __builtin_amdgcn_perm(u1, u0, 0x05040100u);
            const u32 lo = __builtin_amdgcn_perm(u1, u0, 0x04040000u), hi = __builtin_amdgcn_perm(t.nbr[1], t.nbr[0], 0x07070303u);
            P[3] = __builtin_amdgcn_perm(lo, hi, 0x07020500u);
        } else {
            // R = 3: the 48-bit window {unit : neighbour's unit}; V = its bits 47..16, V2 = bits 39..8 (one v_perm each); the states
            // are bits 47..32, 41..26, 35..20, 29..14 = V[31:16], V[25:10], V[19:4], V2[21:6]: a shift per column tile and a
            // v_perm that pairs the two 16-bit results
            const u32 V0 = __builtin_amdgcn_perm(t.own[0], t.nbr[0], 0x06050402u), V1 = __builtin_amdgcn_perm(t.own[1], t.nbr[1], 0x06050402u);
            const u32 W0 = __builtin_amdgcn_perm(t.own[0], t.nbr[0], 0x05040201u), W1 = __builtin_amdgcn_perm(t.own[1], t.nbr[1], 0x05040201u);
            P[0] = __builtin_amdgcn_perm(V1, V0, 0x07060302u);
            P[1] = __builtin_amdgcn_perm(V1 >> 10, V0 >> 10, 0x05040100u);
            P[2] = __builtin_amdgcn_perm(V1 >> 4, V0 >> 4, 0x05040100u);
            P[3] = __builtin_amdgcn_perm(W1 >> 6, W0 >> 6, 0x05040100u);
        }
        u32 t0, t1;
        lookup2(P[0], t0, t1);
        o.wa[0] = t0, o.wa[1] = t1;
        lookup2(P[2], t0, t1);
        o.wa[2] = t0, o.wa[3] = t1;
        lookup2(P[1], t0, t1);
        o.wb[0] = t0, o.wb[1] = t1;
        lookup2(P[3], t0, t1);
        o.wb[2] = t0, o.wb[3] = t1;
        o.xb = *reinterpret_cast<const u32x4 *>(xrow);
    };
    auto stage_c = [&](const TbB &o, u32 par) {
        accA[par] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16x8, o.wa), __builtin_bit_cast(h16x8, o.xb), accA[par], 0, 0, 0);
        accB[par] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16x8, o.wb), __builtin_bit_cast(h16x8, o.xb), accB[par], 0, 0, 0);
    };
    // this lane group's 8 activations of tile block K2: xg + 32 K2.  Only column 0 of the B operand carries them; the lanes of
    // columns 1..15 read from 192 KiB above -- outside the LDS allocation, where ds_read returns zeros (tools/ubench/lds_oob.hip;
    // capi.hip's self-check refuses to start where it does not): 15 equal copies of the activations in the matrix cores cost power,
    // and with it clock (ap_plane.hip: the idle MFMA columns)
    const uint16_t *xg = xsp + 8u * g + ((l & 15u) ? 0x18000u : 0u);
    u32 flip = 0;
    for (;;) {
        const u32 jn = j + gridDim.x;
        const bool has_next = jn < nitems;
        const QtItem nxt = has_next ? item_of(jn, ord + 1u) : cur;
        const u32 chi = (cur.k2hi + CH - 1u) / CH, first = cur.k2lo / CH + w;
        const u32 cnt = first < chi ? (chi - first + W - 1u) / W : 0u;  // chunks of this wave in this item
        const u32 nl = (cnt + PF - 1u) / PF;
#pragma unroll
        for (u32 q = 0; q < 2; q++) accA[q] = f32x4{0.f, 0.f, 0.f, 0.f}, accB[q] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (u32 i = 0; i < nl; i++) {
            const u32 cb = first + i * PF * W;  // chunk of slot 0 in this loop; slot p: cb + p W
            const bool lastloop = i + 1u == nl;
            // what the slots are refilled with: the next loop of this item, or the first loop of the block's next item
            const QtItem &ft = lastloop ? nxt : cur;
            const u32 fc = lastloop ? nxt.k2lo / CH + w : cb + PF * W;
            const uint16_t *xrow = xg + 32u * CH * cb;
            // slots p < nv hold chunks of this item (nv = PF except in its last loop); tile block k of slot p exists if
            // CH (cb + p W) + k < k2hi (a K range may end inside its last chunk).  The stages of consecutive tile blocks overlap:
            // the lookups of tile block t + 1 are issued before the MFMAs of t, a chunk enters its LDS slot ahead of that.
            const u32 rem = cnt - i * PF, nv = rem < PF ? rem : PF;
            auto exists = [&](u32 p, u32 k) { return p < nv && CH * (cb + p * W) + k < cur.k2hi; };
            TbA ta[2][CH];
            TbB tb[2];
            auto chunk_in = [&](u32 p) {
                if (p < nv) chunk_store(dq[p]);
                fetch(p, ft, fc + p * W);
                if (p < nv) {
#pragma unroll
                    for (u32 k = 0; k < CH; k++) stage_a(k, ta[p & 1u][k]);
                }
            };
            chunk_in(0);
            stage_b(ta[0][0], xrow, tb[0]);
#pragma unroll
            for (u32 t = 0; t < PF * CH; t++) {
                const u32 p = t / CH, k = t % CH, tn = t + 1u, pn = tn / CH, kn = tn % CH;
                if (tn < PF * CH) {
                    if (kn == 0u) chunk_in(pn);
                    if (exists(pn, kn)) stage_b(ta[pn & 1u][kn], xrow + 32u * (CH * pn * W + kn), tb[tn & 1u]);
                }
                if (exists(p, k)) stage_c(tb[t & 1u], t & 1u);
            }
        }
        if (nl == 0u && has_next) {  // (a wave without chunks in this item still feeds its queue)
#pragma unroll
            for (u32 p = 0; p < PF; p++) fetch(p, nxt, nxt.k2lo / CH + w + p * W);
        }
        stamp();
        // D layout: lane (gq = l / 16, n = l % 16) holds logical rows 4 gq + 0..3 of column n (all columns are equal):
        // lanes n < 4 store element n of "rows a", lanes 4 <= n < 8 element n - 4 of "rows a + 8"
        {
            const f32x4 sa = accA[0] + accA[1], sb = accB[0] + accB[1];
            float *pw = part + flip * (W * 32u) + w * 32u;
            if ((l & 15u) == 0u) {  // column 0 holds the sums: its lane of each group stores the 4 + 4 rows
#pragma unroll
                for (u32 e = 0; e < 4u; e++) {
                    const u32 r = 4u * g + e;
                    pw[16u * (r >> 3) + (r & 7u)] = sa[e];
                    pw[16u * (r >> 3) + (r & 7u) + 8u] = sb[e];
                }
            }
        }
        __syncthreads();
        if (tid < 32u) {
            const float *pr = part + flip * (W * 32u);
            float t = 0.f;
            for (u32 i = 0; i < W; i++) t += pr[i * 32u + tid];
            cur.out[tid] = t;
        }
        stamp();
        flip ^= 1u;
        if (!has_next) break;
        cur = nxt;
        j = jn;
        ord++;
    }
}

template <int R, int SX, int WC>
__global__ void __launch_bounds__(1024) qtip_matvec_kernel(float *out, const u32 *comp, const uint16_t *x, const uint16_t *tlut,
                                                          u32 M, u32 K, unsigned long long *dbg) {
    __shared__ __attribute__((aligned(128))) u32 tab[QtipTab<SX>::WORDS];
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint16_t *xsp = reinterpret_cast<uint16_t *>(smem);          // [K] permuted copy
    float *part = reinterpret_cast<float *>(xsp + K);            // [2][waves][32 rows]
    unsigned char *stg = reinterpret_cast<unsigned char *>(part + 2u * (blockDim.x >> 6) * 32u);  // [waves] 1 KiB chunk slots
    const u32 T = blockDim.x, tid = threadIdx.x, nK2 = K / 32u;
    auto item_of = [&](u32 j, u32) {
        return QtItem{j * nK2 * 128u * R, out + (size_t)j * 32u, 0u, nK2};
    };
    // codebook words and activations first, the tile blocks behind them (in-order return)
    QtipTabRegs tr;
    qtip_table_request(tr, tlut);
    constexpr u32 NX = 2;  // 8-element units per thread held in registers (K <= 16 T)
    const bool xin = K <= 8u * NX * T;
    uint4 xq[NX];
    if (xin) {
#pragma unroll
        for (u32 k = 0; k < NX; k++) {
            const u32 u = tid + k * T;
            xq[k] = u < K / 8u ? reinterpret_cast<const uint4 *>(x)[u] : make_uint4(0u, 0u, 0u, 0u);
        }
    }
    auto prologue = [&]() {
        qtip_fill_table<SX>(tab, tlut, tr);
        if (xin) {
#pragma unroll
            for (u32 k = 0; k < NX; k++) {
                const u32 u = tid + k * T;
                const u32 o[4] = {xq[k].x, xq[k].y, xq[k].z, xq[k].w};
                if (u < K / 8u) qtip_store_x8(xsp, u, o);
            }
        } else {
            for (u32 u = tid; u < K / 8u; u += T) {
                const uint4 q = reinterpret_cast<const uint4 *>(x)[u];
                const u32 o[4] = {q.x, q.y, q.z, q.w};
                qtip_store_x8(xsp, u, o);
            }
        }
        __syncthreads();
    };
    qtip_engine<R, SX, WC>(tab, xsp, part, stg, comp, (M / 32u) * nK2 * 128u * R, M / 32u, item_of, prologue, dbg);
}

// ------------------------------------------------------------------------------------------------ fused QTIP linear
// BitshiftLinear.forward (inference/lib/codebook/bitshift.py:415-472, eval, one row, no tensor-parallel Hadamard split):
//   x32 = x.float() * SU;  x = hadamard(x32) * n^-1/2 / 32;  y = decompress_matvec(trellis, x.half(), tlut)       [kernel A]
//   y = hadamard(y) * m^-1/2;  out = (y * (SV * 32)).half()  (+ the residual add of the block, model.py:311-313)       [kernel B]
// Kernel A fuses what produces x in the decode step -- RMSNorm (model.py:281-292) or silu(gate) * up (model.py:266) --
// and serves up to 3 linears that share the input (q/k/v, gate/up) in one launch; every 32-row band block repeats the
// K-point transform (K log K / 2 butterflies: small next to its 32 x K trellis decode).
struct QtipIn {
    const u32 *comp;
    const float *SU;
    const uint16_t *tlut;
    float *y32;
    u32 blk0, nblk;  // the blocks [blk0, blk0 + nblk) walk the items (band, K range) of this linear
    u32 M;
};
struct QtipInArgs {
    const uint16_t *x, *x2, *normw;
    float eps, kscale;  // kscale = (float)K^-1/2, rounded from double like the scale argument of hadamard()
    u32 K, n;
    u32 P;       // QPRO_ROWS: length of the row transforms (K = Kf * P)
    u32 ksplit;  // 1..4 K ranges per band; range ks of a band writes its sums to y32 + ks * M
    QtipIn lin[3];
    u32 nprev;          // 1 / 2: x (and x2) are the outputs of the linears prev[] whose transform-out is done here (M == K)
    QtipOut prev[2];
    u32 xs_off, stg_off, part_off, xp_off;  // byte offsets inside the dynamic LDS (host: qtip_in_layout)
    // gq_qtip_linear: the block that finishes a linear LAST (device-scope counter) also runs its transform-out
    QtipOut fin[3];
    u32 *fin_ctr;  // [n] zero before the first launch; the finishing block resets its counter
    unsigned long long *dbg;
};
// dynamic LDS (offsets from the host, qtip_in_layout): v fp32 [K] at 0, dead once the transform is done -- the chunk slots
// (and, from K = 8192 on, the permuted fp16 copy xs too) re-use it --, xs, part [2][W][32], xp fp16 [nprev][K];
// pre-transformed input: xs | part | slots
template <int R, int PRO, int SX, int WC>
__global__ void __launch_bounds__(1024) qtip_linear_in_kernel(QtipInArgs a) {
    __shared__ __attribute__((aligned(128))) u32 tab[QtipTab<SX>::WORDS];
    __shared__ float redf[17];
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const u32 K = a.K, T = blockDim.x, tid = threadIdx.x;
    float *v = reinterpret_cast<float *>(smem);                 // [K] fp32 transform buffer (none for a pre-transformed input)
    uint16_t *xs = reinterpret_cast<uint16_t *>(smem + a.xs_off);  // [K] fp16 matvec input, permuted (qtip_store_x8)
    float *part = reinterpret_cast<float *>(smem + a.part_off);    // [2][waves][32]
    unsigned char *stg = smem + a.stg_off;                          // [waves] 1 KiB chunk slots
    u32 li = 0;
    if (a.n > 1 && blockIdx.x >= a.lin[1].blk0) li = 1;
    if (a.n > 2 && blockIdx.x >= a.lin[2].blk0) li = 2;
    const QtipIn L = a.lin[li];
    // Folded transform-out of the producing linear(s): what gq_qtip_linear_out would have written is rebuilt in LDS by
    // every block (same arithmetic, same order) and stored once, by block 0, for the kernels that need it later
    // (the residual stream).  One launch and one global round trip less per linear.
    const uint16_t *xg = a.x, *x2g = a.x2;
    if (PRO == QPRO_PRE && !a.x) xg = reinterpret_cast<const uint16_t *>(L.SU);  // (one pre-transformed vector per linear: gq_qtip_linear_out_in)
    if (a.nprev) {
        uint16_t *xp = reinterpret_cast<uint16_t *>(smem + a.xp_off);  // [nprev][K] fp16
        for (u32 r = 0; r < a.nprev; r++) {  // the scalar arm of gqq::qtip_transform_out, written out (put-backs)
            const QtipOut P = a.prev[r];
            for (u32 i = tid; i < K; i += T) v[i] = gqq::sum_parts(P.y32, K, P.parts, i);
            __syncthreads();
            gq_fwht::fwht_lds(v, K);
            for (u32 i = tid; i < K; i += T) {
                h16 y = gqq::xf_out(v[i], P.mscale, P.SV32[i]);
                if (P.resid) y = gqq::xf_resid(P.resid[i], y);
                xp[r * K + i] = __builtin_bit_cast(uint16_t, y);
                if (blockIdx.x == 0 && P.out) P.out[i] = __builtin_bit_cast(uint16_t, y);
            }
            __syncthreads();
        }
        xg = xp;
        x2g = xp + K;
    }
    // The input vectors are requested first (registers), the first tile blocks of the band behind them, and the prologue
    // runs while those are on their way from HBM (vector memory returns in order: requested the other way round, the
    // first use of x would wait for the tiles).
    QtipTabRegs tr;
    qtip_table_request(tr, L.tlut);
    constexpr u32 NU = 2;  // 8-element units per thread held in registers (K <= 16 T)
    const bool inreg = !a.nprev && K <= 8u * NU * T && PRO != QPRO_PRE && PRO != QPRO_ROWS &&
                       !(((uintptr_t)xg | (uintptr_t)x2g | (uintptr_t)a.normw | (uintptr_t)L.SU) & 15u);
    // the first pass of the Sylvester transform fused into the element-wise stage: units of whole waves (K / 8 a multiple of 64, or
    // fewer than 64: the first lanes of wave 0), every unit of a wave in the same loop trip, K >= 64
    const bool fused_first = inreg && K >= 64u && ((K / 8u) % 64u == 0u || K / 8u < 64u);
    uint4 xq[NU], x2q[NU], nwq[NU];
    float4 su0[NU], su1[NU];
    // QPRO_ROWS: x is the fp32 vector gq_qtip_mlp_mid left -- the Kf x Kf factor product of the transform-in is done (column by
    // column, so it commutes with the row transforms); what is left is cheap enough to repeat in every block: the P-point
    // Sylvester transform of every row, * K^-1/2 / 32, fp16.  Requested with the other inputs (<= 4 x 16 bytes per thread).
    constexpr u32 NZ = 4;
    float4 zq[NZ];
    if constexpr (PRO == QPRO_ROWS) {
#pragma unroll
        for (u32 k = 0; k < NZ; k++) {
            const u32 u = tid + k * T;
            zq[k] = u < K / 4u ? reinterpret_cast<const float4 *>(xg)[u] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    if (inreg) {
#pragma unroll
        for (u32 k = 0; k < NU; k++) {
            const u32 u = tid + k * T;
            const bool ok = u < K / 8u;
            xq[k] = ok ? reinterpret_cast<const uint4 *>(xg)[u] : make_uint4(0u, 0u, 0u, 0u);
            su0[k] = ok ? reinterpret_cast<const float4 *>(L.SU)[2u * u] : make_float4(0.f, 0.f, 0.f, 0.f);
            su1[k] = ok ? reinterpret_cast<const float4 *>(L.SU)[2u * u + 1u] : make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (PRO == QPRO_RMSNORM) nwq[k] = ok ? reinterpret_cast<const uint4 *>(a.normw)[u] : make_uint4(0u, 0u, 0u, 0u);
            if constexpr (PRO == QPRO_SILUMUL) x2q[k] = ok ? reinterpret_cast<const uint4 *>(x2g)[u] : make_uint4(0u, 0u, 0u, 0u);
        }
    }
    // (prologue stamps of GQ_STAMPS builds: kept in registers and written out behind the engine -- a global store per stamp sits in vmcnt
    // and turns the next wait for a load into a wait for the store's acknowledgement, ~1,000 cycles each)
    u32 pst = 0;
    unsigned long long pstv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto pstamp = [&]() {
        if (GQ_STAMPS && a.dbg && blockIdx.x == gridDim.x / 2) {
            const unsigned long long now = __builtin_readcyclecounter();
#pragma unroll
            for (u32 i = 0; i < 8u; i++)
                if (i == pst) pstv[i] = now;
            pst++;
        }
    };
    auto prologue = [&]() {
        pstamp();
        qtip_fill_table<SX>(tab, L.tlut, tr);
        pstamp();
        if constexpr (PRO == QPRO_PRE) {  // x is the transformed fp16 input already (gq_qtip_transform): K need not be a power of two
            for (u32 u = tid; u < K / 8u; u += T) {
                const uint4 q = reinterpret_cast<const uint4 *>(xg)[u];
                const u32 o[4] = {q.x, q.y, q.z, q.w};
                qtip_store_x8(xs, u, o);
            }
            __syncthreads();
            return;
        }
        float nscale = 0.f;
        if constexpr (PRO == QPRO_RMSNORM) {
            float ss = 0.f;
            if (inreg) {
#pragma unroll
                for (u32 k = 0; k < NU; k++) {  // gqq::ssq_unit, written out (units beyond K are zero)
                    const u32 w4[4] = {xq[k].x, xq[k].y, xq[k].z, xq[k].w};
#pragma unroll
                    for (int e = 0; e < 8; e++) {
                        const float f = (float)__builtin_bit_cast(h16, gqq::h16_of(w4, e));
                        ss += f * f;
                    }
                }
            } else {  // same elements per thread, same order (the two forms give the same sum bit for bit)
                for (u32 u = tid; u < K / 8u; u += T)
#pragma unroll
                    for (u32 e = 0; e < 8; e++) {
                        const float f = (float)__builtin_bit_cast(h16, xg[8u * u + e]);
                        ss += f * f;
                    }
            }
            // gqq::block_rms_scale, written out (as a call the branches around the statistic come out in another order: DESIGN.md 3.13)
            ss = gqq::wave_allsum(ss);
            if ((tid & 63u) == 0) redf[tid >> 6] = ss;
            __syncthreads();
            {
                const float t = gqq::wave_allsum((tid & 63u) < (T >> 6) ? redf[tid & 63u] : 0.f);
                nscale = 1.0f / sqrtf(t / (float)K + a.eps);
            }
        }
        pstamp();
        if constexpr (PRO == QPRO_ROWS) {
#pragma unroll
            for (u32 k = 0; k < NZ; k++) {
                const u32 u = tid + k * T;
                if (u < K / 4u) reinterpret_cast<float4 *>(v)[u] = zq[k];
            }
            for (u32 u = tid + NZ * T; u < K / 4u; u += T) reinterpret_cast<float4 *>(v)[u] = reinterpret_cast<const float4 *>(xg)[u];
        } else if (inreg) {
#pragma unroll
            for (u32 k = 0; k < NU; k++) {
                const u32 u = tid + k * T;
                if (u < K / 8u) {
                    float o[8];
                    gqq::xf_in_unit<PRO>(xq[k], x2q[k], nwq[k], su0[k], su1[k], nscale, o);
                    // (round 6) unit u IS work item u of the transform's first pass: its register / cross-lane stages run on the
                    // values where they are -- one LDS round trip and one barrier less than store, barrier, fwht_first_pass
                    if (fused_first) gq_fwht::fwht_item_stages<8u>(o, u, gq_fwht::fwht_mmax<8u>(K));
                    reinterpret_cast<float4 *>(v)[2u * u] = make_float4(o[0], o[1], o[2], o[3]);
                    reinterpret_cast<float4 *>(v)[2u * u + 1u] = make_float4(o[4], o[5], o[6], o[7]);
                }
            }
        } else {
            for (u32 i = tid; i < K; i += T)
                v[i] = gqq::xf_in<PRO>(xg[i], PRO == QPRO_SILUMUL ? x2g[i] : (uint16_t)0, PRO == QPRO_RMSNORM ? a.normw[i] : (uint16_t)0, nscale, L.SU[i]);
        }
        __syncthreads();
        pstamp();
        {
            const u32 Pt = PRO == QPRO_ROWS ? a.P : K;
            const u32 hnext = fused_first ? 16u * gq_fwht::fwht_mmax<8u>(K) : gq_fwht::fwht_first_pass(v, K, Pt);
            if (GQ_STAMPS) pstamp();
            gq_fwht::fwht_rest(v, K, Pt, hnext);
        }
        pstamp();
        // fp32 -> fp16, IN PLACE (xs is the front half of v): every thread takes its (<= NU) units of 8 values into
        // registers, one barrier, then the permuted stores (the host checks K <= 16 T)
        const float sc = a.kscale;
        u32 o[NU][4];
#pragma unroll
        for (u32 k = 0; k < NU; k++) {
            const u32 u = tid + k * T;
            if (u < K / 8u) {
                const float4 f0 = reinterpret_cast<const float4 *>(v)[2u * u], f1 = reinterpret_cast<const float4 *>(v)[2u * u + 1u];
                const float f[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
#pragma unroll
                for (int e = 0; e < 4; e++) o[k][e] = gqq::xf_in_pack(f[2 * e], f[2 * e + 1], sc);
            }
        }
        __syncthreads();
#pragma unroll
        for (u32 k = 0; k < NU; k++) {
            const u32 u = tid + k * T;
            if (u < K / 8u) qtip_store_x8(xs, u, o[k]);
        }
        __syncthreads();
    };
    constexpr u32 CH = QtChunk<R>::CH;
    const u32 nK2 = K / 32u, nch = (nK2 + CH - 1u) / CH, kpart = ((nch + a.ksplit - 1u) / a.ksplit) * CH, bl = blockIdx.x - L.blk0;
    // item t of this linear = (band t / ksplit, K range t % ksplit); this block takes t = bl, bl + nblk, ...
    // (no integer divide on this chip, and the item feeds the addresses of the NEXT item's first chunks at every item boundary: the
    // ordinal r comes from the engine, the K range by shifts / a constant divisor)
    auto item_of = [&](u32, u32 r) {  // item r of this block: jj = blockIdx.x + r * gridDim.x  ->  t = bl + r * nblk
        const u32 t = bl + r * L.nblk;
        u32 band, ks;
        if (a.ksplit == 1u) band = t, ks = 0u;
        else if (a.ksplit == 2u) band = t >> 1, ks = t & 1u;
        else if (a.ksplit == 4u) band = t >> 2, ks = t & 3u;
        else band = t / 3u, ks = t - 3u * band;
        const u32 lo = ks * kpart, hi = lo + kpart < nK2 ? lo + kpart : nK2;
        return QtItem{band * nK2 * 128u * R, L.y32 + (size_t)ks * L.M + (size_t)band * 32u, lo, hi};
    };
    // number of items of this block, expressed in the engine's index space (j = blockIdx.x + r * gridDim.x < nitems)
    const u32 total = (L.M / 32u) * a.ksplit, mine = bl < total ? (total - bl + L.nblk - 1u) / L.nblk : 0u;
    qtip_engine<R, SX, WC>(tab, xs, part, stg, L.comp, (L.M / 32u) * nK2 * 128u * R, mine ? blockIdx.x + (mine - 1u) * gridDim.x + 1u : 0u, item_of, prologue, a.dbg);
    if (GQ_STAMPS && a.dbg && blockIdx.x == gridDim.x / 2 && (tid & 63u) == 0) {
#pragma unroll
        for (u32 i = 0; i < 8u; i++)
            if (pstv[i]) a.dbg[128u + (tid >> 6) * 8u + i] = pstv[i];
    }
    if (a.fin_ctr) {
        // Every sum of this block is written (by wave 0, in program order before this point).  Release them to the device,
        // count the block in; the block that completes the count acquires the others' sums and transforms them.  No block
        // waits for another one: this is not a grid barrier, the last arrival simply carries on.
        __shared__ u32 is_last;
        __syncthreads();
        if (tid == 0) {
            __threadfence();
            const u32 old = atomicAdd(a.fin_ctr + li, 1u);
            is_last = old == L.nblk - 1u ? 1u : 0u;
            if (is_last) a.fin_ctr[li] = 0u;  // (nobody touches it again before the next launch)
        }
        __syncthreads();
        if (!is_last) return;
        __threadfence();
        gqq::qtip_transform_out(a.fin[li], reinterpret_cast<float *>(tab));  // the codebook is dead: its LDS holds the M floats
    }
}

}  // namespace

namespace {
// waves per block: the chunks of every K range are dealt out to them (a range shorter than the block still works: the
// surplus waves only take part in the barriers), 16 = four per SIMD for the usual widths
u32 qtip_waves(u32 min_range) {  // min_range: chunks in the shortest K range
    u32 wv = 1;
    while (wv < 16u && wv < min_range) wv *= 2u;
    return wv;
}
constexpr size_t QT_LDS = 160u * 1024u, QT_STATIC_SLACK = 256u;  // (redf + alignment)
bool qtip_sx_fits(size_t dyn) { return dyn + (size_t)QtipTab<1>::WORDS * 4u + QT_STATIC_SLACK <= QT_LDS; }
bool qtip_fits(size_t dyn) { return dyn + (size_t)QtipTab<0>::WORDS * 4u + QT_STATIC_SLACK <= QT_LDS; }
constexpr u32 qtip_chunk(int R) { return R == 2 ? QtChunk<2>::CH : (R == 3 ? QtChunk<3>::CH : QtChunk<4>::CH); }  // the engine's load unit

// The instance of a band-engine kernel for the runtime (R, SX, waves == 16): `launch` is a generic lambda that takes the three as
// std::integral_constants, raises its instance's dynamic-LDS limit through qtip_max_lds and launches it.
template <class F>
int qtip_instance(int R, int sx, u32 waves, F launch) {
    auto with_w = [&](auto r, auto s) {
        return waves == 16u ? launch(r, s, std::integral_constant<int, 16>{}) : launch(r, s, std::integral_constant<int, 0>{});
    };
    auto with_sx = [&](auto r) { return sx ? with_w(r, std::integral_constant<int, 1>{}) : with_w(r, std::integral_constant<int, 0>{}); };
    return R == 2 ? with_sx(std::integral_constant<int, 2>{}) : (R == 3 ? with_sx(std::integral_constant<int, 3>{}) : with_sx(std::integral_constant<int, 4>{}));
}
template <int SX>
hipError_t qtip_max_lds(GqPerDeviceOnce &once, const void *kernel) {  // once per device: what the static table leaves of the LDS
    return once.max_dynamic_lds(kernel, (int)(QT_LDS - (size_t)QtipTab<SX>::WORDS * 4u - QT_STATIC_SLACK));
}
}  // namespace

extern "C" int gq_qtip_matvec(float *out, const uint32_t *compressed, const void *x, const void *codebook, uint32_t M,
                              uint32_t K, int R, void *stream) {
    if (!out || !compressed || !x || !codebook) return gq_fail(GQ_EINVAL, "null pointer argument.");
    if (R < 2 || R > 4) return gq_fail(GQ_ENOTSUP, "R (bits per weight) must be 2, 3 or 4 (kernel_check.py:1-14).");
    if (M == 0 || K == 0 || M % 32u || K % 32u) return gq_fail(GQ_EINVAL, "M and K must be positive multiples of 32.");
    if (((uintptr_t)x | (uintptr_t)compressed | (uintptr_t)codebook) & 15u) return gq_fail(GQ_EINVAL, "buffers must be 16-byte aligned.");
    const u32 nK2 = K / 32u, ch = qtip_chunk(R), waves = qtip_waves((nK2 + ch - 1u) / ch), bands = M / 32u;
    const size_t smem = (size_t)K * 2u + (size_t)waves * 2u * 32u * 4u + (size_t)waves * 1024u;
    if (!qtip_fits(smem)) return gq_fail(GQ_ENOTSUP, "K too large.");
    const int sx = qtip_sx_fits(smem) && gq_env_int("GQ_QTIP_SX", 1) ? 1 : 0;
    const u32 cus = (u32)gq_cu_count();
    hipStream_t s = (hipStream_t)stream;
    dim3 grid(bands < cus ? bands : cus), block(waves * 64u);
    return qtip_instance(R, sx, waves, [&](auto r, auto sxc, auto wc) {
        const auto kernel = qtip_matvec_kernel<decltype(r)::value, decltype(sxc)::value, decltype(wc)::value>;
        static GqPerDeviceOnce once;
        GQ_HIP_CHECK(qtip_max_lds<decltype(sxc)::value>(once, reinterpret_cast<const void *>(kernel)));
        hipLaunchKernelGGL(kernel, grid, block, smem, s, out, compressed, (const uint16_t *)x, (const uint16_t *)codebook, M, K, g_qdbg);
        GQ_HIP_CHECK(hipGetLastError());
        return (int)GQ_OK;
    });
}

namespace {
bool pow2(u32 n) { return n && !(n & (n - 1u)); }

// blocks per linear: the `cus` blocks of a launch are shared out in proportion to the bands (every block serves ONE linear:
// its prologue multiplies by that linear's SU); returns the largest number of rounds (items per block) of any linear
u32 qtip_share_blocks(int n, const u32 *bands, u32 ksplit, u32 cus, u32 *nblk) {
    u32 total = 0, items = 0;
    for (int i = 0; i < n; i++) total += bands[i], items += bands[i] * ksplit;
    if (items <= cus) {
        for (int i = 0; i < n; i++) nblk[i] = bands[i] * ksplit;
        return 1u;
    }
    u32 used = 0;
    for (int i = 0; i < n; i++) {
        nblk[i] = (u32)((unsigned long long)cus * bands[i] / total);
        if (nblk[i] == 0u) nblk[i] = 1u;
        used += nblk[i];
    }
    while (used < cus) {  // leftover blocks to the linear with the most items per block
        int best = 0;
        double worst = -1.0;
        for (int i = 0; i < n; i++) {
            const double load = (double)bands[i] * ksplit / nblk[i];
            if (load > worst) worst = load, best = i;
        }
        nblk[best]++, used++;
    }
    u32 rounds = 0;
    for (int i = 0; i < n; i++) {
        const u32 r = (bands[i] * ksplit + nblk[i] - 1u) / nblk[i];
        if (r > rounds) rounds = r;
    }
    return rounds;
}
}  // namespace

extern "C" int gq_qtip_plan_ksplit(int n, const uint32_t *M, uint32_t K, int max_ksplit) {
    if (n < 1 || n > 3 || !M || K < 32u) return 1;
    if (max_ksplit > 4) max_ksplit = 4;
    const u32 cus = (u32)gq_cu_count(), nK2 = K / 32u;
    u32 bands[3], nblk[3];
    for (int i = 0; i < n; i++) bands[i] = M[i] / 32u;
    int best = 1;
    double best_cost = 1e30;
    for (int ks = 1; ks <= max_ksplit; ks++) {
        if (ks > 1 && nK2 / 4u / (u32)ks < 16u) break;  // every K range keeps the 16 waves of a block busy (one 4-tile-block chunk each)
        const u32 rounds = qtip_share_blocks(n, bands, (u32)ks, cus, nblk);
        // time ~ rounds of 1 / ks band each, plus a small price per extra part (its flush and the consumer's extra read)
        const double cost = (double)rounds / ks * (1.0 + 0.02 * (ks - 1));
        if (cost < best_cost - 1e-9) best_cost = cost, best = ks;
    }
    return best;
}

namespace {
int qtip_linear_in_impl(const void *x, const void *x2, const void *norm_weight, float eps, int prologue, uint32_t K, int R, int n,
                        const GqQtipIn *lin, int n_prev, const GqQtipOut *prev, int ksplit, const GqQtipOut *fin, void *counters, void *stream,
                        uint32_t rows_P = 0) {
    if (ksplit < 1 || ksplit > 4) return gq_fail(GQ_EINVAL, "gq_qtip_linear_in: ksplit must be 1..4.");
    if (!lin || n < 1 || n > 3) return gq_fail(GQ_EINVAL, "gq_qtip_linear_in: 1..3 linears.");
    if (n_prev < 0 || n_prev > 2 || (n_prev && !prev)) return gq_fail(GQ_EINVAL, "gq_qtip_linear_in: 0..2 producing linears.");
    if (n_prev == 0 && !x && prologue != GQ_QPRO_PRETRANSFORMED) return gq_fail(GQ_EINVAL, "gq_qtip_linear_in: x is null.");
    if (n_prev && n_prev != (prologue == GQ_QPRO_SILU_MUL ? 2 : 1))
        return gq_fail(GQ_EINVAL, "gq_qtip_linear_in: one producing linear per input vector (two for SILU_MUL).");
    if (R < 2 || R > 4) return gq_fail(GQ_ENOTSUP, "R (bits per weight) must be 2, 3 or 4 (kernel_check.py:1-14).");
    if (prologue == GQ_QPRO_PRETRANSFORMED) {
        if (K == 0 || K % 32u || K > 32768u || n_prev) return gq_fail(GQ_EINVAL, "gq_qtip_linear_in: pre-transformed input: K a multiple of 32, no folding.");
    } else if (prologue == QPRO_ROWS) {  // (gq_qtip_linear_in_rows: checked there)
        if (!rows_P || n_prev || fin) return gq_fail(GQ_EINVAL, "gq_qtip_linear_in: prologue 4 is reached through gq_qtip_linear_in_rows.");
    } else if (!pow2(K) || K < 32u || K > 16384u)
        return gq_fail(GQ_ENOTSUP, "fused QTIP linear: K must be a power of two in 32..16384.");
    if ((prologue == GQ_QPRO_RMSNORM && !norm_weight) || (prologue == GQ_QPRO_SILU_MUL && !x2 && !n_prev) || prologue < 0 || prologue > QPRO_ROWS)
        return gq_fail(GQ_EINVAL, "gq_qtip_linear_in: prologue operand missing.");
    const u32 nK2 = K / 32u;
    if ((u32)ksplit > nK2) return gq_fail(GQ_EINVAL, "gq_qtip_linear_in: more K ranges than tile blocks.");
    QtipInArgs a{};
    a.x = (const uint16_t *)x;
    a.x2 = (const uint16_t *)x2;
    a.normw = (const uint16_t *)norm_weight;
    a.eps = eps;
    a.kscale = gq_inv_sqrt_f(K);
    a.K = K;
    a.n = (u32)n;
    a.P = rows_P;
    u32 bands[3] = {0, 0, 0}, nblk[3] = {0, 0, 0};
    for (int i = 0; i < n; i++) {
        if (!lin[i].trellis || (!lin[i].SU && prologue != GQ_QPRO_PRETRANSFORMED && prologue != QPRO_ROWS) || !lin[i].tlut || !lin[i].y32 || lin[i].M == 0 || lin[i].M % 32u)
            return gq_fail(GQ_EINVAL, "gq_qtip_linear_in: null pointer or M not a multiple of 32.");
        if (prologue == GQ_QPRO_PRETRANSFORMED && !x && (!lin[i].SU || ((uintptr_t)lin[i].SU & 15u)))
            return gq_fail(GQ_EINVAL, "gq_qtip_linear_in: pre-transformed input without x: every linear's SU field must point to ITS fp16 vector (16-byte aligned).");
        if (((uintptr_t)lin[i].trellis | (uintptr_t)lin[i].tlut) & 15u) return gq_fail(GQ_EINVAL, "buffers must be 16-byte aligned.");
        bands[i] = lin[i].M / 32u;
    }
    qtip_share_blocks(n, bands, (u32)ksplit, (u32)gq_cu_count(), nblk);
    u32 blocks = 0;
    for (int i = 0; i < n; i++) {
        a.lin[i] = QtipIn{lin[i].trellis, lin[i].SU, (const uint16_t *)lin[i].tlut, lin[i].y32, blocks, nblk[i], lin[i].M};
        blocks += nblk[i];
    }
    // K ranges in chunks (the engine's load unit: 4 tile blocks at R = 2, else 2)
    const u32 ch = qtip_chunk(R), nch = (nK2 + ch - 1u) / ch, cpart = (nch + (u32)ksplit - 1u) / (u32)ksplit;
    if (cpart * ((u32)ksplit - 1u) >= nch) return gq_fail(GQ_EINVAL, "gq_qtip_linear_in: an empty K range (ksplit too large for K).");
    const u32 clast = nch - ((u32)ksplit - 1u) * cpart;
    u32 waves = qtip_waves(clast < cpart ? clast : cpart);
    if (waves < 4u) waves = 4u;  // the transform wants threads
    if (prologue != GQ_QPRO_PRETRANSFORMED && K > 16u * waves * 64u) waves = 16u;  // (the in-place fp16 conversion: <= 2 units per thread)
    a.ksplit = (u32)ksplit;
    a.dbg = g_qdbg;
    a.fin_ctr = nullptr;
    if (fin) {
        if (!counters || ((uintptr_t)counters & 3u)) return gq_fail(GQ_EINVAL, "gq_qtip_linear: counters (u32 [n], zeroed once) missing.");
        for (int i = 0; i < n; i++) {
            GqQtipOut f = fin[i];  // (the sums and their parts are the launch's own)
            f.y32 = lin[i].y32, f.parts = (u32)ksplit;
            if (gq_qtip_out_desc(f, true, a.fin[i]) != GQ_QOUT_OK || fin[i].M != lin[i].M)
                return gq_fail(GQ_EINVAL, "gq_qtip_linear: finish descriptor (SV32, out, M) does not match the linear.");
            if (!pow2(fin[i].M) || fin[i].M < 32u || fin[i].M > 16384u)
                return gq_fail(GQ_ENOTSUP, "gq_qtip_linear: M must be a power of two in 32..16384 (other widths: gq_qtip_linear_in + gq_qtip_transform).");
        }
        a.fin_ctr = (u32 *)counters;
    }
    a.nprev = (u32)n_prev;
    for (int i = 0; i < n_prev; i++) {
        const GqQtipOutErr e = gq_qtip_out_desc(prev[i], false, a.prev[i]);
        if (e == GQ_QOUT_NULL || prev[i].M != K) return gq_fail(GQ_EINVAL, "gq_qtip_linear_in: producing linear must have M == K.");
        if (e == GQ_QOUT_PARTS) return gq_fail(GQ_EINVAL, "gq_qtip_linear_in: parts must be 0..4.");
    }
    // LDS layout: the transform buffer v (K floats at 0) is dead when the matvec starts: the chunk slots re-use it, and so does
    // the fp16 copy xs when both fit (K >= 8192; the conversion is staged through registers)
    const size_t slots = (size_t)waves * 1024u, pbytes = (size_t)waves * 2u * 32u * 4u;
    size_t end;
    if (prologue == GQ_QPRO_PRETRANSFORMED) {
        a.xs_off = 0, a.part_off = K * 2u, a.stg_off = (u32)(K * 2u + pbytes), end = (size_t)K * 2u + pbytes + slots;
    } else if ((size_t)K * 2u + slots <= (size_t)K * 4u) {
        a.xs_off = 0, a.stg_off = K * 2u, a.part_off = K * 4u, end = (size_t)K * 4u + pbytes;
    } else {
        const size_t va = (size_t)K * 4u > slots ? (size_t)K * 4u : slots;
        a.stg_off = 0, a.xs_off = (u32)va, a.part_off = (u32)(va + (size_t)K * 2u), end = va + (size_t)K * 2u + pbytes;
    }
    // the rebuilt input vector(s) of a folded transform-out: one vector fits the (not yet written) xs region when that is
    // not inside v; otherwise behind everything
    const bool xp_in_xs = n_prev == 1 && a.xs_off != 0u;
    a.xp_off = xp_in_xs ? a.xs_off : (u32)end;
    const size_t smem = xp_in_xs ? end : end + (size_t)n_prev * K * 2u;
    if (!qtip_fits(smem)) return gq_fail(GQ_ENOTSUP, "gq_qtip_linear_in: K too large.");
    const int sx = qtip_sx_fits(smem) && gq_env_int("GQ_QTIP_SX", 1) ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    dim3 grid(blocks), block(waves * 64u);
    auto with_pro = [&](auto pro) {
        return qtip_instance(R, sx, waves, [&](auto r, auto sxc, auto wc) {
            const auto kernel = qtip_linear_in_kernel<decltype(r)::value, decltype(pro)::value, decltype(sxc)::value, decltype(wc)::value>;
            static GqPerDeviceOnce once;
            GQ_HIP_CHECK(qtip_max_lds<decltype(sxc)::value>(once, reinterpret_cast<const void *>(kernel)));
            hipLaunchKernelGGL(kernel, grid, block, smem, s, a);
            GQ_HIP_CHECK(hipGetLastError());
            return (int)GQ_OK;
        });
    };
    switch (prologue) {
        case GQ_QPRO_RMSNORM: return with_pro(std::integral_constant<int, QPRO_RMSNORM>{});
        case GQ_QPRO_SILU_MUL: return with_pro(std::integral_constant<int, QPRO_SILUMUL>{});
        case GQ_QPRO_PRETRANSFORMED: return with_pro(std::integral_constant<int, QPRO_PRE>{});
        case QPRO_ROWS: return with_pro(std::integral_constant<int, QPRO_ROWS>{});
        default: return with_pro(std::integral_constant<int, QPRO_NONE>{});
    }
}
}  // namespace

extern "C" int gq_qtip_linear_in(const void *x, const void *x2, const void *norm_weight, float eps, int prologue, uint32_t K, int R,
                                 int n, const GqQtipIn *lin, int n_prev, const GqQtipOut *prev, int ksplit, void *stream) {
    return qtip_linear_in_impl(x, x2, norm_weight, eps, prologue, K, R, n, lin, n_prev, prev, ksplit, nullptr, nullptr, stream);
}

extern "C" int gq_qtip_linear(const void *x, const void *x2, const void *norm_weight, float eps, int prologue, uint32_t K, int R, int n,
                              const GqQtipIn *lin, const GqQtipOut *finish, int ksplit, void *counters, void *stream) {
    if (!finish) return gq_fail(GQ_EINVAL, "gq_qtip_linear: finish descriptors missing.");
    return qtip_linear_in_impl(x, x2, norm_weight, eps, prologue, K, R, n, lin, 0, nullptr, ksplit, finish, counters, stream);
}

extern "C" int gq_qtip_linear_in_rows(const float *z32, uint32_t K, uint32_t P, int R, int n, const GqQtipIn *lin, int ksplit, void *stream) {
    if (!z32 || ((uintptr_t)z32 & 15u)) return gq_fail(GQ_EINVAL, "gq_qtip_linear_in_rows: z32 null or not 16-byte aligned.");
    if (P < 2u || !pow2(P) || K == 0 || K % P || K % 32u || K > 16384u) return gq_fail(GQ_EINVAL, "gq_qtip_linear_in_rows: K = Kf * P <= 16384, P a power of two, K % 32 == 0.");
    return qtip_linear_in_impl(z32, nullptr, nullptr, 0.f, QPRO_ROWS, K, R, n, lin, 0, nullptr, ksplit, nullptr, nullptr, stream, P);
}
