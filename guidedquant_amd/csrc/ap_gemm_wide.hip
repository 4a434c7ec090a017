// ap_gemm_wide.hip -- the fused-dequant prefill GEMM of ap_gemm.hip at 5 to 8 bits.
//
//   out[s][n] = sum_k x[s][k] * lut[n][code(n, k)]          x fp16 [S][K], out fp16 [S][N], S > 1 rows (a prompt)
//
// Same contract as the 2..4-bit kernel: the bit-plane words (packed file format, pack.py:304-321) are the only weight bytes read from
// memory, nothing dense is written to global memory, products on v_mfma_f32_32x32x16_f16, fp32 accumulation over all of K and one
// rounding to fp16; K % 64 == 0 (tail chunks of 64 .. 960 weights), any N >= 1, any S >= 1; rows past N / tokens past S are computed
// on clamped indices and never stored.
//
// What differs is where the row LUTs live.  2^BITS fp16 per row are 16 / 32 / 64 / 128 VGPRs as v_perm byte pools (ap_core.h::LutPools),
// so the tile's 128 tables sit in LDS (64 B .. 512 B per row, 8 .. 64 KiB per tile) and a weight costs one ds_read_u16.  Each table
// slot is 2^BITS * 2 + 4 bytes: the 4-byte skew moves consecutive rows one bank on (a 256- or 512-byte stride would start every row in
// bank 0, and the 64 lanes of a lookup hold 64 different rows).
//
// Organisation: the BLOCK decodes, not the wave.  Counted per weight, the decode is
//     code formation   BITS / 2 VALU   (selector words as in ap_wide.hip: one shift + one and-or per plane and bit position, 4 codes each)
//     lookup           2 VALU (extract the code byte, add the row's table base) + 1 ds_read_u16
//     fp16 pairing     ~0.5
// = 5.5 (5 bits) .. 7 (8 bits) instructions, against 1.4 (2 bits) .. 3.3 (4 bits) of the register decode of ap_gemm.hip.  A wave that
// decodes its own A fragments (that kernel's organisation) pays this once per token tile it multiplies with, and its 32 rows' tables
// have to be resident per WAVE: 8 waves x 32 rows x 512 B = 128 KiB at 8 bits, which leaves no room for the x tiles.  Decoding the
// 128 x 64 weight tile of a K stage to fp16 in LDS once per block costs one extra ds_write_b128 per 8 weights and one ds_read_b128
// per A fragment (both conflict-free, below), needs the tables of 128 rows only (64 KiB at 8 bits), and lets the waves tile the
// block 2 x 2 (64 rows x 64 tokens each): per K-step 2 A reads + 2 B reads feed 4 MFMAs, where 1 x 4 fragments per wave would read 5.
// Per stage a thread then issues ~32 * 6 decode instructions for the NEXT stage beside its 16 MFMAs of this one -- independent work
// in one instruction stream, which was meant to keep the matrix core busy under the decode.
// MEASURED (profiles/prefill_gemm_bits_5_to_8.json): it does not.  A block takes ~2 us per 64-weight stage (127 us for K = 4096 at 5
// bits, 158 at 8) whatever S is, about 5 x the instruction count above: 0.09-0.17 of the fp16 MFMA peak at S = 2048 against 0.35-0.43
// for the 2..4-bit kernel, and 0.21-0.86 of the speed of dequantise + hipBLASLt on every 8B shape.  With one block of four waves
// per CU (two at 5 bits) nothing hides the chain lookup -> pack -> ds_write -> barrier -> fragment read -> MFMA of a stage.  The
// kernel is correct and is what GQ_PREFILL_FUSED=1 reaches; the default dispatch keeps the two steps at these widths.
//
// Block = 256 threads, tile 128 weight rows x 128 tokens, K stage = 64 weights.  Thread (row = tid & 127, h = tid >> 7) owns the plane
// words t = hw h + q0 .. q0 + 3 of its row for a group of 4 stages (hw = half the words of the chunk's row, q0 = 0, 4, ..): byte lane
// c = 0..3 of those words is stage c of the group (byte c of word t holds the weights 8 tpw c + 8 t + 0..7 of the chunk, MSB first).
// MFMA lane (r, g) of K-step q therefore multiplies k = chunk base + 8 tpw c + 8 (hw g + q0 + q) + 0..7: the same fragment mapping as
// ap_gemm.hip's first kernel, with groups of 4 words.  The selector words of a group (32 VGPRs) are formed once and serve its 4
// stages; the next group's plane words are requested (16-byte loads) when the group starts.
// LDS: two x stages and two W stages of [128][128 B], 16-byte slot sl of row i at physical slot sl ^ ((i >> 1) & 7) (the 16 lanes
// of a ds_read_b128 / ds_write_b128 phase cover every 16-byte column of the 256-byte bank row once), then the tables.
// One __syncthreads per stage.  No split K and one tile shape: gq_anyprec_gemm_ws_bytes is 0 at these widths.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ap_core.h"
#include "ap_dispatch.h"
#include "wave_util.h"

namespace {
using gq::u32;
using gqw::f16x8;
using gqw::f32x16;
using gqw::lds_addr;

constexpr u32 BS = 128, BN = 128, ROWB = 128;  // token tile, weight-row tile, bytes per tile row of a stage (64 fp16)
constexpr u32 STAGE_BYTES = BS * ROWB;

template <int BITS>
struct GemmWideGeom {
    static constexpr u32 NC = 1u << BITS;        // centroids per row
    static constexpr u32 TS = NC * 2u + 4u;      // table slot (bytes): one bank of skew per row
    static constexpr int SH = BITS <= 7 ? 1 : 0; // codes formed doubled (byte offsets) while they fit a byte
    static constexpr size_t SMEM = 4u * STAGE_BYTES + BN * TS;
};

__device__ __forceinline__ u32 lds_u16(u32 addr) { return *(const __attribute__((address_space(3))) uint16_t *)(uintptr_t)addr; }

template <int BITS>
__global__ void __launch_bounds__(256, 2) ap_gemm_wide_kernel(const uint16_t *__restrict__ x, uint16_t *__restrict__ out,
                                                               const u32 *__restrict__ qw, const uint16_t *__restrict__ lut, u32 S, u32 N,
                                                               u32 K) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];  // x[2], W[2] stages, tables
    using WG = GemmWideGeom<BITS>;
    unsigned char *xs_base = smem, *ws_base = smem + 2u * STAGE_BYTES, *tab = smem + 4u * STAGE_BYTES;
    const u32 tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u, r = lane & 31u, g = lane >> 5;
    const u32 n0 = blockIdx.x * BN, s0 = blockIdx.y * BS;
    const u32 wpr = K / 32u, nfull = K / 1024u, eff = (K % 1024u) / 32u, nchunks = nfull + (eff ? 1u : 0u);
    const size_t plane_stride = (size_t)N * wpr;

    // decode role: row drow of the tile, word half dh
    const u32 drow = tid & 127u, dh = tid >> 7;
    const u32 dn = min(n0 + drow, N - 1u);  // rows past N are computed on a clamped row and never stored
    const u32 tb = lds_addr(tab) + drow * WG::TS;
    const u32 dswz = (drow >> 1) & 7u;
    // MFMA role: wave (wr, wc) multiplies rows 64 wr + 32 f + r with tokens 64 wc + 32 j + r
    const u32 wr = wave & 1u, wc = wave >> 1;
    const u32 mswz = (r >> 1) & 7u;

    // the tile's tables: row i at tab + i TS
    for (u32 i = tid; i < BN * (WG::NC / 2u); i += 256u) {
        const u32 row = i / (WG::NC / 2u), wd = i % (WG::NC / 2u);
        const u32 n = min(n0 + row, N - 1u);
        *reinterpret_cast<u32 *>(tab + row * WG::TS + 4u * wd) = reinterpret_cast<const u32 *>(lut + (size_t)n * WG::NC)[wd];
    }

    f32x16 acc[2][2];
#pragma unroll
    for (int f = 0; f < 2; f++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[f][j][e] = 0.f;

    // stage sequence: chunk -> group of up to 4 K-steps (q0) -> byte lane c; the plane words of a (chunk, q0) group serve 4 stages
    struct Cursor {
        u32 chunk, q0, c;
    };
    auto stage_geom = [&](const Cursor &cu, u32 &kseg0, u32 &kseg1, u32 &nq) {
        const u32 tpw = cu.chunk < nfull ? 32u : eff, hw = tpw >> 1;
        nq = min(4u, hw - cu.q0);
        const u32 base = 1024u * cu.chunk + 8u * tpw * cu.c;
        kseg0 = base + 8u * cu.q0;
        kseg1 = base + 8u * (hw + cu.q0);
    };
    auto advance = [&](Cursor &cu) {
        if (++cu.c < 4u) return;
        cu.c = 0;
        const u32 hw = (cu.chunk < nfull ? 32u : eff) >> 1;
        cu.q0 += 4u;
        if (cu.q0 < hw) return;
        cu.q0 = 0;
        cu.chunk++;
    };

    // x stage copy: 128 tokens x 8 pieces of 16 B (slot sl = 4 g + q) = 1024 pieces, 4 per thread; piece p = tid + 256 i
    uint4 pre[4];
    auto load_stage = [&](const Cursor &cu) {
        u32 kseg0, kseg1, nq;
        stage_geom(cu, kseg0, kseg1, nq);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const u32 p = tid + 256u * (u32)i, tok = p >> 3, sl = p & 7u, part = sl & 3u;
            const u32 s = s0 + tok;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (s < S && part < nq) v = *reinterpret_cast<const uint4 *>(x + (size_t)s * K + ((sl >> 2) ? kseg1 : kseg0) + 8u * part);
            pre[i] = v;
        }
    };
    auto store_stage = [&](u32 buf) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const u32 p = tid + 256u * (u32)i, tok = p >> 3, sl = p & 7u;
            *reinterpret_cast<uint4 *>(xs_base + buf * STAGE_BYTES + tok * ROWB + ((sl ^ ((tok >> 1) & 7u)) * 16u)) = pre[i];
        }
    };

    // plane words t = hw dh + q0 .. + nq - 1 of the thread's row (one 16-byte load per plane where the group is whole and aligned)
    u32 wn[BITS][4];
    auto fetch_words = [&](const Cursor &cu) {
        const u32 tpw = cu.chunk < nfull ? 32u : eff, hw = tpw >> 1, nq = min(4u, hw - cu.q0);
        const u32 *base = qw + (size_t)dn * wpr + 32u * cu.chunk + hw * dh + cu.q0;
#pragma unroll
        for (int p = 0; p < BITS; p++) {
            const u32 *pp = base + (size_t)p * plane_stride;
            if (nq == 4u && (hw & 3u) == 0u && (wpr & 3u) == 0u) {
                const uint4 a = *reinterpret_cast<const uint4 *>(pp);
                wn[p][0] = a.x, wn[p][1] = a.y, wn[p][2] = a.z, wn[p][3] = a.w;
            } else {
#pragma unroll
                for (int q = 0; q < 4; q++) wn[p][q] = (u32)q < nq ? pp[q] : 0u;
            }
        }
    };
    // selector words: byte (3 - c) of sel[q][b] = the code (doubled below 8 bits) of the weight at bit b of byte c of word q --
    // plane p (0 = most significant) goes to bit BITS - 1 - p + SH
    u32 sel[4][8];
    auto form_selectors = [&]() {
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int b = 0; b < 8; b++) {
                u32 v = 0u;
#pragma unroll
                for (int p = 0; p < BITS; p++) {
                    const int dst = BITS - 1 - p + WG::SH;
                    v |= gq::shl(wn[p][q], dst - b) & (0x01010101u << dst);
                }
                sel[q][b] = v;
            }
    };
    auto group_after = [&](Cursor cu) {
        cu.c = 3u;
        advance(cu);
        return cu;
    };
    // byte lane cu.c of the group's words -> fp16 in W stage `buf`: slot 4 dh + q of the thread's row holds the 8 weights of word q
    auto decode_stage = [&](const Cursor &cu, u32 buf) {
        const u32 hw = (cu.chunk < nfull ? 32u : eff) >> 1, nq = min(4u, hw - cu.q0);
        const u32 sh = 24u - 8u * cu.c;
        unsigned char *wrow = ws_base + buf * STAGE_BYTES + drow * ROWB;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if ((u32)q < nq) {
                u32 e[8];
#pragma unroll
                for (int j = 0; j < 8; j++) {  // weight j of the byte sits at bit 7 - j
                    const u32 code = (sel[q][7 - j] >> sh) & 0xFFu;
                    e[j] = lds_u16(tb + (code << (1 - WG::SH)));
                }
                v = make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
            }
            *reinterpret_cast<uint4 *>(wrow + (((4u * dh + (u32)q) ^ dswz) * 16u)) = v;
        }
    };

    Cursor cur{0u, 0u, 0u};
    fetch_words(cur);
    form_selectors();
    {
        const Cursor ng = group_after(cur);
        if (ng.chunk < nchunks) fetch_words(ng);
    }
    load_stage(cur);
    store_stage(0);
    __syncthreads();  // the tables
    decode_stage(cur, 0);
    __syncthreads();
    u32 buf = 0;
    while (cur.chunk < nchunks) {
        u32 k0, k1, nq;
        stage_geom(cur, k0, k1, nq);
        Cursor nx = cur;
        advance(nx);
        const bool more = nx.chunk < nchunks;
        if (more) {
            load_stage(nx);  // in flight during the decode and the MFMAs below
            if (nx.c == 0u) {  // a new group: its words were requested when the last one started
                form_selectors();
                const Cursor ng = group_after(nx);
                if (ng.chunk < nchunks) fetch_words(ng);
            }
            decode_stage(nx, buf ^ 1u);
        }
        const unsigned char *xs = xs_base + buf * STAGE_BYTES + (64u * wc + r) * ROWB;
        const unsigned char *as = ws_base + buf * STAGE_BYTES + (64u * wr + r) * ROWB;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if ((u32)q < nq) {
                const u32 slot = ((4u * g + (u32)q) ^ mswz) * 16u;
                f16x8 a[2], b[2];
#pragma unroll
                for (int f = 0; f < 2; f++) a[f] = *reinterpret_cast<const f16x8 *>(as + (u32)f * 32u * ROWB + slot);
#pragma unroll
                for (int j = 0; j < 2; j++) b[j] = *reinterpret_cast<const f16x8 *>(xs + (u32)j * 32u * ROWB + slot);
#pragma unroll
                for (int f = 0; f < 2; f++)
#pragma unroll
                    for (int j = 0; j < 2; j++) acc[f][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[f], b[j], acc[f][j], 0, 0, 0);
            }
        }
        if (more) store_stage(buf ^ 1u);
        __syncthreads();
        buf ^= 1u;
        cur = nx;
    }

    // D layout: col j = lane & 31 (token), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (weight row)
#pragma unroll
    for (int f = 0; f < 2; f++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const u32 s = s0 + 64u * wc + 32u * (u32)j + r;
            if (s >= S) continue;
#pragma unroll
            for (int rg = 0; rg < 4; rg++) {
                const u32 nn = n0 + 64u * wr + 32u * (u32)f + 8u * (u32)rg + 4u * g;
                if (nn >= N) continue;
                uint16_t h[4];
#pragma unroll
                for (int e = 0; e < 4; e++) h[e] = __builtin_bit_cast(uint16_t, (_Float16)acc[f][j][4 * rg + e]);
                uint16_t *dst = out + (size_t)s * N + nn;
                if (nn + 3u < N && (N & 3u) == 0u) {
                    *reinterpret_cast<uint2 *>(dst) = make_uint2((u32)h[0] | ((u32)h[1] << 16), (u32)h[2] | ((u32)h[3] << 16));
                } else {
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        if (nn + (u32)e < N) dst[e] = h[e];
                }
            }
        }
}

template <int BITS>
int launch_gemm_wide(const void *x, void *out, const uint32_t *qw, const void *lut, u32 S, u32 N, u32 K, hipStream_t s) {
    static GqPerDeviceOnce once;
    auto kern = ap_gemm_wide_kernel<BITS>;
    const size_t smem = GemmWideGeom<BITS>::SMEM;
    GQ_HIP_CHECK(once.max_dynamic_lds(reinterpret_cast<const void *>(kern), (int)smem));
    dim3 grid((N + BN - 1u) / BN, (S + BS - 1u) / BS), block(256);
    hipLaunchKernelGGL(kern, grid, block, smem, s, (const uint16_t *)x, (uint16_t *)out, qw, (const uint16_t *)lut, S, N, K);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}
}  // namespace

// gq_anyprec_gemm / gq_anyprec_gemm_ws (ap_gemm.hip) at 5..8 bits; the arguments were checked there
int gq_ap_gemm_wide(const void *x, void *out, const uint32_t *qweight, const void *lut, uint32_t S, uint32_t N, uint32_t K, int bits,
                    hipStream_t stream) {
    if ((S + BS - 1u) / BS > 65535u) return gq_fail(GQ_ENOTSUP, "gq_anyprec_gemm: more than 65535 token tiles.");
    switch (bits) {
        case 5: return launch_gemm_wide<5>(x, out, qweight, lut, S, N, K, stream);
        case 6: return launch_gemm_wide<6>(x, out, qweight, lut, S, N, K, stream);
        case 7: return launch_gemm_wide<7>(x, out, qweight, lut, S, N, K, stream);
        case 8: return launch_gemm_wide<8>(x, out, qweight, lut, S, N, K, stream);
        default: return gq_fail(GQ_ENOTSUP, "gq_anyprec_gemm: this kernel serves 5 to 8 bits.");
    }
}
