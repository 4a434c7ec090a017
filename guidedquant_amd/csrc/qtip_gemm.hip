// qtip_gemm.hip -- the prompt path of a QTIP linear: trellis decode fused into a matrix-core GEMM, and the decode alone.
//
//   gq_qtip_gemm:        out[s][m] = sum_k decode(compressed)[m][k] * x[s][k]   x fp16 [S][K], out fp32 [S][M] (written)
//   gq_qtip_decompress:  W[m][k] = decode(compressed)[m][k]                       W fp16 [M][K] (written)
//
// Replace the bs > 8 branch of BitshiftLinear.forward (qtip/lib/codebook/bitshift.py:466-470 -> bitshift_linear_kernel,
// qtip/lib/utils/kernel_decompress.py:82-91): decode_compressed (kernel_decompress.py:5-55) writes a dense fp16 hatW to HBM,
// torch.matmul reads it back and rounds z to fp16.  Here the trellis bytes are the only weight bytes that move, and the output
// stays fp32 -- a DELIBERATE DEVIATION from the reference's bs > 8 branch, which rounds z to fp16 before the Hadamard
// transform: the products are exact (fp16 x fp16), the sums fp32, so 8 rows (the matvec loop, which keeps z in fp32) and
// 9 rows are the same arithmetic class, equal up to the fp32 summation order.
//
// Trellis format (the one qtip.hip reads; oracle/gq_oracle.c states it): a 2 x 2 tile block (32 rows x 32 columns) is 128 R
// contiguous bytes, 32 "s-rows" of 4 R bytes; s-row s holds the R-byte little-endian units of stream position s of its four
// 16 x 16 tiles, unit j = 2 a3 + a4 for tile row parity a4 and tile column parity a3.  The big-endian bit stream of a tile is
// its 32 units in order; state p is the 16-bit window at bit offset 2 R p (cyclic) -- inside units p / 4 and p / 4 + 1 -- so
// any state decodes from two units, without a sequential dependency.  State p = 4 (4 a + b) + 2 cc + d holds the fp16 pair of
// row a + 8 d, columns 2 b + 8 cc + {0, 1} (the m16n8k16 A-fragment slot); value = quantlut_sym(state) (bitshift.py:72-80).
//
// GEMM mapping (v_mfma_f32_32x32x16_f16: lane = 32 g + r holds A[i = r][8 g .. 8 g + 7] and B[8 g .. 8 g + 7][j = r]):
//   i = weight row, j = token.  A 32 x 16 A-fragment is one tile column (a3) of a 32-row band's tile block: lane (r, g) is
//   row r = 16 a4 + a + 8 d and takes units b = 2 g, 2 g + 1 of its tile, states d and d + 2 of each -- k-slot
//   t = 8 g + 4 bb + 2 cc + el (b = 2 g + bb) is column c = 4 g + 2 bb + 8 cc + el of the 16.  An MFMA product does not care
//   which 8 k share an operand, so the weights are used in that order and x is stored in LDS in it (xpos below): the B
//   fragment stays one ds_read_b128.  Each lane decodes 4 states per A-fragment (the 256 pairs of a 32 x 16 fragment over 64
//   lanes: no lane decodes what another does) from the 3 s-rows 4 a + 2 g .. + 2 it loads from global memory.
// Block = 256 threads = 4 waves, tile 128 weight rows x 32 CF tokens (wave: one 32-row band x CF token fragments); the codebook
// (512 fp16 pairs) is a 2 KiB LDS table per block; x is staged in LDS 64 columns (32 at CF = 8) at a time, double-buffered through registers
// together with the next stage's trellis words; the weights are decoded once per (row tile, token tile).
// Short grids (fewer output tiles than compute units): K is split over up to 16 ranges of tile blocks, each range's fp32
// partial sums go to a caller workspace and a second launch adds them in ascending K order (deterministic, no atomics).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gq_internal.h"
#include "wave_util.h"

namespace {
typedef uint32_t u32;
typedef unsigned long long u64;
using gqw::f16x8;
using gqw::f32x16;
using gqw::u32x4;

constexpr u32 WAVES = 4, BM = 32u * WAVES;  // weight rows per block
// tile blocks (32 columns each) per x stage: 2, or 1 beside the 128 accumulator registers of 8 token fragments
template <int CF>
constexpr u32 tb_of() { return CF == 8 ? 1u : 2u; }
// bytes per token row of an x stage: 64 per tile block + a 16-byte pad (the 16-byte slots of a B read are conflict-free)
template <int CF>
constexpr u32 rowb_of() { return 64u * tb_of<CF>() + 16u; }
constexpr u32 MAX_KSPLIT = 16;

// unit j = 2 a3 + a4 of an s-row (R dwords, R-byte little-endian units) -- with a4 a per-lane value and a3 a
// compile-time one
template <int R>
__device__ __forceinline__ u32 unit_sel(const u32 (&d)[R], u32 a3, u32 a4) {
    if constexpr (R == 2) {
        return (d[a3] >> (16u * a4)) & 0xFFFFu;
    } else if constexpr (R == 3) {  // units at bits 0, 24, 48, 72 of the 96-bit row
        if (a3 == 0u) return __builtin_amdgcn_alignbit(d[1], d[0], 24u * a4) & 0xFFFFFFu;
        return a4 ? d[2] >> 8 : __builtin_amdgcn_alignbit(d[2], d[1], 16u) & 0xFFFFFFu;
    } else {
        return a4 ? d[2u * a3 + 1u] : d[2u * a3];
    }
}

// state i (0..3) of unit u, whose successor in the tile's stream is un: the 16-bit window at bit offset 2 R i of {u : un}
template <int R>
__device__ __forceinline__ u32 state_of(u32 u, u32 un, u32 i) {
    const u64 v = ((u64)u << (8u * R)) | un;
    return (u32)(v >> (16u * R - 16u - 2u * R * i)) & 0xFFFFu;
}

// quantlut_sym: st (st + 1) mod 2^32, entry (idx >> 6) & 511, bit 15 flips the sign of the first value of the pair
__device__ __forceinline__ u32 lookup(const u32 *tab, u32 st) {
    const u32 idx = __umul24(st, st + 1u);
    return tab[(idx >> 6) & 511u] ^ (idx & 0x8000u);
}

__device__ __forceinline__ void fill_table(u32 *tab, const uint16_t *tlut) {
    for (u32 e = threadIdx.x; e < 512u; e += blockDim.x) tab[e] = reinterpret_cast<const u32 *>(tlut)[e];
}

template <int R>
__device__ __forceinline__ void load_srow(u32 (&d)[R], const u32 *p) {
#pragma unroll
    for (int q = 0; q < R; q++) d[q] = p[q];
}

// ------------------------------------------------------------------------------------------------ decompress
// one thread per (tile block, s-row): s-rows s and s + 1 give the 16 states of stream position s of the four tiles
template <int R>
__global__ void __launch_bounds__(256) qtip_decompress_kernel(uint16_t *__restrict__ W, const u32 *__restrict__ comp,
                                                              const uint16_t *__restrict__ tlut, u32 M, u32 K) {
    __shared__ u32 tab[512];
    fill_table(tab, tlut);
    __syncthreads();
    const u32 ktb = K / 32u, ntb = (M / 32u) * ktb;
    const u32 gid = blockIdx.x * blockDim.x + threadIdx.x, blk = gid >> 5, s = gid & 31u;
    if (blk >= ntb) return;
    const u32 bm = blk / ktb, kt = blk - bm * ktb;
    const u32 *base = comp + (size_t)blk * 32u * R;
    u32 d0[R], d1[R];
    load_srow<R>(d0, base + s * R);
    load_srow<R>(d1, base + ((s + 1u) & 31u) * R);
    const u32 a = s >> 2, b = s & 3u;
#pragma unroll
    for (u32 a3 = 0; a3 < 2; a3++)
#pragma unroll
        for (u32 a4 = 0; a4 < 2; a4++) {
            const u32 u = unit_sel<R>(d0, a3, a4), un = unit_sel<R>(d1, a3, a4);
#pragma unroll
            for (u32 i = 0; i < 4; i++) {
                const u32 row = 32u * bm + 16u * a4 + a + 8u * (i & 1u), col = 32u * kt + 16u * a3 + 2u * b + 8u * (i >> 1);
                *reinterpret_cast<u32 *>(W + (size_t)row * K + col) = lookup(tab, state_of<R>(u, un, i));
            }
        }
}

// ------------------------------------------------------------------------------------------------ GEMM
// position of column c (0..15) of a 16-column group inside the staged x row: slot t = 8 c2 + 4 c1 + 2 c3 + c0 (the A slot
// order above).  A group arrives as 8 fp16 pairs P[p] (p = c >> 1) and is staged as P0 P4 P1 P5 P2 P6 P3 P7.
// dst: out, or the workspace of the split-K form (range z at dst + z * zstride).
template <int R, int CF>
__global__ void __launch_bounds__(256, 2) qtip_gemm_kernel(float *__restrict__ dst, size_t zstride, const u32 *__restrict__ comp,
                                                           const uint16_t *__restrict__ x, const uint16_t *__restrict__ tlut, u32 S,
                                                           u32 M, u32 K, u32 ktb_per_split) {
    constexpr u32 TB = tb_of<CF>(), ROWB = rowb_of<CF>();
    constexpr u32 BS = 32u * CF;                 // tokens per block
    constexpr u32 STAGE = BS * ROWB;
    constexpr u32 GROUPS = 2u * TB;              // 16-column groups per token row and stage
    constexpr u32 PIECES = BS * GROUPS / 256u;   // 32-byte x pieces per thread and stage
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];  // [2][BS][ROWB] x stages, then the codebook
    u32 *tab = reinterpret_cast<u32 *>(smem + 2u * STAGE);
    const u32 tid = threadIdx.x, lane = tid & 63u, r = lane & 31u, g = lane >> 5;
    const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const u32 nbands = M / 32u, ktb = K / 32u;
    const u32 band_raw = blockIdx.x * WAVES + wave, band = min(band_raw, nbands - 1u);  // (a band past M computes, never stores)
    const u32 s0 = blockIdx.y * BS;
    const u32 kt0 = blockIdx.z * ktb_per_split, kt1 = min(ktb, kt0 + ktb_per_split);
    const u32 nst = (kt1 - kt0 + TB - 1u) / TB;

    // lane geometry: row r = 16 a4 + a + 8 d of the band; s-rows 4 a + 2 g, + 1, + 2 (cyclic) of each tile block
    const u32 a4 = r >> 4, a = r & 7u, d = (r >> 3) & 1u;
    const u32 sA = 4u * a + 2u * g, sB = sA + 1u, sC = (sA + 2u) & 31u;
    const u32 *band_p = comp + (size_t)band * ktb * 32u * R;

    fill_table(tab, tlut);

    f32x16 acc[CF];
#pragma unroll
    for (int j = 0; j < CF; j++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[j][e] = 0.f;

    u32 tw[TB][3][R];      // trellis s-rows of the next stage
    u32x4 xp[PIECES][2];   // x pieces of the next stage
    auto load_stage = [&](u32 st) {
        const u32 ktS = kt0 + TB * st;
#pragma unroll
        for (u32 tb = 0; tb < TB; tb++) {
            const u32 kt = min(ktS + tb, kt1 - 1u);  // (a tile block past the range is loaded again and never used)
            const u32 *p = band_p + (size_t)kt * 32u * R;
            load_srow<R>(tw[tb][0], p + sA * R);
            load_srow<R>(tw[tb][1], p + sB * R);
            load_srow<R>(tw[tb][2], p + sC * R);
        }
#pragma unroll
        for (u32 i = 0; i < PIECES; i++) {
            const u32 pc = tid + 256u * i, tok = pc / GROUPS, gi = pc % GROUPS, s = s0 + tok;
            xp[i][0] = xp[i][1] = u32x4{0u, 0u, 0u, 0u};
            if (s < S && ktS + gi / 2u < kt1) {
                const u32x4 *src = reinterpret_cast<const u32x4 *>(x + (size_t)s * K + 32u * ktS + 16u * gi);
                xp[i][0] = src[0];
                xp[i][1] = src[1];
            }
        }
    };
    auto store_stage = [&](u32 buf) {
#pragma unroll
        for (u32 i = 0; i < PIECES; i++) {
            const u32 pc = tid + 256u * i, tok = pc / GROUPS, gi = pc % GROUPS;
            u32x4 *q = reinterpret_cast<u32x4 *>(smem + buf * STAGE + tok * ROWB + gi * 32u);
            const u32x4 lo = xp[i][0], hi = xp[i][1];
            q[0] = u32x4{lo[0], hi[0], lo[1], hi[1]};
            q[1] = u32x4{lo[2], hi[2], lo[3], hi[3]};
        }
    };

    load_stage(0);
    store_stage(0);
    __syncthreads();
    u32 buf = 0;
    for (u32 st = 0; st < nst; st++) {
        // decode the stage's A fragments first: the trellis registers are then free for the next stage's loads
        f16x8 A[TB][2];
#pragma unroll
        for (u32 tb = 0; tb < TB; tb++)
#pragma unroll
            for (u32 a3 = 0; a3 < 2; a3++) {
                const u32 uA = unit_sel<R>(tw[tb][0], a3, a4), uB = unit_sel<R>(tw[tb][1], a3, a4), uC = unit_sel<R>(tw[tb][2], a3, a4);
                const u32x4 w = {lookup(tab, state_of<R>(uA, uB, d)), lookup(tab, state_of<R>(uA, uB, d + 2u)),
                                 lookup(tab, state_of<R>(uB, uC, d)), lookup(tab, state_of<R>(uB, uC, d + 2u))};
                A[tb][a3] = __builtin_bit_cast(f16x8, w);
            }
        const bool more = st + 1u < nst;
        if (more) load_stage(st + 1u);  // in flight during the MFMAs below
        const unsigned char *xs = smem + buf * STAGE + r * ROWB + g * 16u;
        const u32 ntb = min(TB, kt1 - kt0 - TB * st);  // (the last stage of a range may hold fewer tile blocks)
#pragma unroll
        for (u32 tb = 0; tb < TB; tb++) {
            if (tb < ntb) {
#pragma unroll
                for (u32 a3 = 0; a3 < 2; a3++)
#pragma unroll
                    for (u32 j = 0; j < (u32)CF; j++) {
                        const f16x8 B = *reinterpret_cast<const f16x8 *>(xs + j * 32u * ROWB + (tb * 32u + a3 * 16u) * 2u);
                        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[tb][a3], B, acc[j], 0, 0, 0);
                    }
            }
        }
        if (more) store_stage(buf ^ 1u);
        __syncthreads();
        buf ^= 1u;
    }

    // D layout: token j = lane & 31, weight row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    if (band_raw >= nbands) return;
    float *o = dst + blockIdx.z * zstride;
#pragma unroll
    for (u32 j = 0; j < (u32)CF; j++) {
        const u32 s = s0 + 32u * j + r;
        if (s >= S) continue;
#pragma unroll
        for (u32 rg = 0; rg < 4; rg++) {
            const u32 m = 32u * band + 8u * rg + 4u * g;
            *reinterpret_cast<float4 *>(o + (size_t)s * M + m) =
                make_float4(acc[j][4 * rg], acc[j][4 * rg + 1], acc[j][4 * rg + 2], acc[j][4 * rg + 3]);
        }
    }
}

// out[i] = sum over the K ranges z = 0, 1, ... of ws[z][i], in that order (n4 = S M / 4 float4s)
__global__ void __launch_bounds__(256) qtip_gemm_reduce_kernel(float4 *__restrict__ out, const float4 *__restrict__ ws, u32 n4, u32 nks) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    float4 v = ws[i];
    for (u32 z = 1; z < nks; z++) {
        const float4 t = ws[(size_t)z * n4 + i];
        v.x += t.x, v.y += t.y, v.z += t.z, v.w += t.w;
    }
    out[i] = v;
}

// token fragments per wave: 8 (256 tokens per block, half the decode per MFMA) from 256 tokens on; GQ_QTIP_GEMM_CF = 4 | 8 forces one
int gemm_cf(u32 S) {
    const int env = gq_env_int("GQ_QTIP_GEMM_CF", 0);
    if (env == 4 || env == 8) return env;
    return S >= 256u ? 8 : 4;
}

// K ranges of a short grid: about two blocks per CU, each range at least 8 tile blocks (256 columns), at most 16 ranges;
// GQ_QTIP_GEMM_KSPLIT forces the range count (1: no split)
u32 gemm_plan_ksplit(u32 S, u32 M, u32 K, int cf) {
    const u32 ktb = K / 32u, tiles = ((M + BM - 1u) / BM) * ((S + 32u * cf - 1u) / (32u * cf));
    const int env = gq_env_int("GQ_QTIP_GEMM_KSPLIT", -1);
    u32 want;
    if (env >= 0) {
        want = (u32)env;
    } else {
        const u32 cus = (u32)gq_cu_count();
        if (tiles >= cus) return 1u;
        want = (2u * cus + tiles - 1u) / tiles;
    }
    u32 cap = ktb / 8u;
    if (cap > MAX_KSPLIT) cap = MAX_KSPLIT;
    if (want > cap) want = cap;
    if (want <= 1u) return 1u;
    const u32 per = (ktb + want - 1u) / want;
    return (ktb + per - 1u) / per;
}

template <int R, int CF>
int launch_gemm(float *out, const u32 *comp, const uint16_t *x, const uint16_t *tlut, u32 S, u32 M, u32 K, u32 nks, float *ws,
                hipStream_t st) {
    static GqPerDeviceOnce once;
    auto kern = qtip_gemm_kernel<R, CF>;
    const size_t smem = 2u * (32u * CF) * rowb_of<CF>() + 512u * 4u;
    GQ_HIP_CHECK(once.max_dynamic_lds(reinterpret_cast<const void *>(kern), (int)smem));
    const u32 ktb = K / 32u, per = (ktb + nks - 1u) / nks;
    dim3 grid((M / 32u + WAVES - 1u) / WAVES, (S + 32u * CF - 1u) / (32u * CF), nks), block(256);
    const bool split = nks > 1u;
    hipLaunchKernelGGL(kern, grid, block, smem, st, split ? ws : out, split ? (size_t)S * M : (size_t)0, comp, x, tlut, S, M, K, per);
    GQ_HIP_CHECK(hipGetLastError());
    if (split) {
        const u32 n4 = S * M / 4u;
        hipLaunchKernelGGL(qtip_gemm_reduce_kernel, dim3((n4 + 255u) / 256u), dim3(256), 0, st, reinterpret_cast<float4 *>(out),
                           reinterpret_cast<const float4 *>(ws), n4, nks);
        GQ_HIP_CHECK(hipGetLastError());
    }
    return GQ_OK;
}

template <int R>
int launch_gemm_r(float *out, const u32 *comp, const uint16_t *x, const uint16_t *tlut, u32 S, u32 M, u32 K, u32 nks, float *ws, int cf,
                  hipStream_t st) {
    return cf == 8 ? launch_gemm<R, 8>(out, comp, x, tlut, S, M, K, nks, ws, st) : launch_gemm<R, 4>(out, comp, x, tlut, S, M, K, nks, ws, st);
}

int check_shape(const char *who, u32 M, u32 K, int R) {
    (void)who;
    if (R < 2 || R > 4) return gq_fail(GQ_ENOTSUP, "gq_qtip: R must be 2, 3 or 4.");
    if (M == 0 || K == 0 || M % 32u || K % 32u) return gq_fail(GQ_ENOTSUP, "gq_qtip: M and K must be positive multiples of 32.");
    if ((uint64_t)M * K >= (1ull << 32)) return gq_fail(GQ_ENOTSUP, "gq_qtip: M * K must be below 2^32.");
    return GQ_OK;
}
}  // namespace

extern "C" int gq_qtip_decompress(void *W, const void *compressed, const void *codebook, uint32_t M, uint32_t K, int R, void *stream) {
    if (int rc = check_shape("gq_qtip_decompress", M, K, R)) return rc;
    if (!W || !compressed || !codebook) return gq_fail(GQ_EINVAL, "null pointer argument.");
    if (((uintptr_t)W | (uintptr_t)compressed | (uintptr_t)codebook) & 3u)
        return gq_fail(GQ_EINVAL, "gq_qtip_decompress: W, compressed and codebook must be 4-byte aligned.");
    hipStream_t st = (hipStream_t)stream;
    const u32 threads = (M / 32u) * (K / 32u) * 32u;
    const dim3 grid((threads + 255u) / 256u), block(256);
    auto w = (uint16_t *)W;
    auto c = (const u32 *)compressed;
    auto t = (const uint16_t *)codebook;
    switch (R) {
        case 2: hipLaunchKernelGGL(qtip_decompress_kernel<2>, grid, block, 0, st, w, c, t, M, K); break;
        case 3: hipLaunchKernelGGL(qtip_decompress_kernel<3>, grid, block, 0, st, w, c, t, M, K); break;
        default: hipLaunchKernelGGL(qtip_decompress_kernel<4>, grid, block, 0, st, w, c, t, M, K); break;
    }
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}

extern "C" size_t gq_qtip_gemm_ws_bytes(uint32_t S, uint32_t M, uint32_t K, int R) {
    if (R < 2 || R > 4 || S == 0 || M == 0 || K == 0 || M % 32u || K % 32u) return 0;
    const u32 nks = gemm_plan_ksplit(S, M, K, gemm_cf(S));
    return nks > 1u ? (size_t)nks * S * M * 4u : 0;
}

extern "C" int gq_qtip_gemm_ws(void *out, const void *compressed, const void *x, const void *codebook, uint32_t S, uint32_t M, uint32_t K,
                               int R, void *workspace, size_t ws_bytes, void *stream) {
    if (int rc = check_shape("gq_qtip_gemm", M, K, R)) return rc;
    if (S == 0) return gq_fail(GQ_EINVAL, "gq_qtip_gemm: empty problem.");
    if ((uint64_t)S * M >= (1ull << 32) / 4u) return gq_fail(GQ_ENOTSUP, "gq_qtip_gemm: S * M too large.");
    if (!out || !compressed || !x || !codebook) return gq_fail(GQ_EINVAL, "null pointer argument.");
    if (((uintptr_t)out | (uintptr_t)x) & 15u || ((uintptr_t)compressed | (uintptr_t)codebook) & 3u)
        return gq_fail(GQ_EINVAL, "gq_qtip_gemm: out / x must be 16-byte, compressed / codebook 4-byte aligned.");
    if (workspace && ((uintptr_t)workspace & 15u)) return gq_fail(GQ_EINVAL, "gq_qtip_gemm_ws: workspace must be 16-byte aligned.");
    const int cf = gemm_cf(S);
    u32 nks = workspace ? gemm_plan_ksplit(S, M, K, cf) : 1u;
    if (nks > 1u && ws_bytes < (size_t)nks * S * M * 4u) nks = 1u;  // (too small a workspace: the single pass)
    hipStream_t st = (hipStream_t)stream;
    auto o = (float *)out;
    auto c = (const u32 *)compressed;
    auto xx = (const uint16_t *)x;
    auto t = (const uint16_t *)codebook;
    auto ws = (float *)workspace;
    switch (R) {
        case 2: return launch_gemm_r<2>(o, c, xx, t, S, M, K, nks, ws, cf, st);
        case 3: return launch_gemm_r<3>(o, c, xx, t, S, M, K, nks, ws, cf, st);
        default: return launch_gemm_r<4>(o, c, xx, t, S, M, K, nks, ws, cf, st);
    }
}

extern "C" int gq_qtip_gemm(void *out, const void *compressed, const void *x, const void *codebook, uint32_t S, uint32_t M, uint32_t K,
                            int R, void *stream) {
    return gq_qtip_gemm_ws(out, compressed, x, codebook, S, M, K, R, nullptr, 0, stream);
}
