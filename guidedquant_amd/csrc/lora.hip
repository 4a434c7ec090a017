// lora.hip -- a LoRA adapter beside the quantized base of the fused decode step, gfx950 (include/gq_hip.h: gq_lora_down, gq_lora_up).
//   t = A xh (fp32),  d = fp16(s B t),  out = fp16(base + d)
// A site's contribution is a two-stage skinny product: A is [R][K] with R <= 192, B is [N][rank <= 64].  Neither stage has the bytes to be
// bandwidth-bound (rank 16 at K = 4096: 128 KiB of A); both are bound by the latency of one dependent memory round trip, so the design
// spends its effort on having every byte requested at once and nothing handed over inside a launch.
//
// gq_lora_down.  K is cut into at most 64 slices of whole 64-element chunks, one block of four waves per slice.  A work item is
// (16 rows of A) x (one 64-element chunk): lane (row r = l % 16, quad g = l / 16) requests the 32 contiguous bytes A[row][chunk + 16 g ..
// + 15] -- 128 contiguous bytes per row and item -- which ARE two A fragments of v_mfma_f32_16x16x32_f16 (the K index of a matrix-core
// product is only a label, ap_dq.hip): the B fragments of lanes (column 0, g) are the matching 16 activations, read from the slice of xh
// staged in LDS, columns 1..15 are zeros.  The items of a block go round the four waves; an item's sums (column 0 of D: rows 4 g + e in
// lanes 0, 16, 32, 48) go to LDS, and after one barrier thread j < R adds the chunks of its row in ascending order and stores the block's
// partial.  No accumulator lives across items, so nothing is indexed dynamically (no scratch) and the requests of an item do not wait for
// the MFMAs of the one before.  The RMSNorm statistic is the dense head's (dense_stage.h): per block, from all of x (an L2 read), then only
// the block's slice is normalised.
//
// gq_lora_up.  64 output rows per block, four lanes per row.  First t: with Q = 256 / R thread groups, thread (q, j) adds the partials
// [q C, (q + 1) C) of element j in ascending order, and the Q subtotals are added in ascending order -- a fixed association of the
// ascending order, so a replay is bit-equal, and the chain of dependent L2 reads is n_partials / Q long instead of n_partials.  Then lane
// `sub` of a row's four takes the 16-byte pieces sub, sub + 4 of the row of B (rank <= 64: two at most), multiplies in fp32 with t from
// LDS, a xor butterfly over the four lanes (row_sum<4>) adds them, lane 0 scales, rounds once to fp16, adds the base in fp16 and stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gq_internal.h"
#include "wave_util.h"

namespace {

typedef uint32_t u32;
using gqw::f16x8;
using gqw::f32x4;
using gqw::h16;
using gqw::h2f;
using gqw::h2u;
using gqw::row_sum;
using gqw::u2h;
using gqw::wave_reduce_bcast;

constexpr u32 LORA_MAX_PARTIALS = 64;  // slices of K = blocks of gq_lora_down = partial sums every block of gq_lora_up adds
constexpr u32 LORA_MAX_CHUNKS = 16;    // 64-element chunks per slice: K <= 64 * 16 * 64
constexpr u32 LORA_MAX_R = 192;
constexpr u32 LORA_UP_ROWS = 64;       // output rows per block of gq_lora_up

// chunks per slice and slices of a K (a multiple of 64)
__host__ __device__ inline u32 lora_chunks_per_slice(u32 K) { return (K / 64u + LORA_MAX_PARTIALS - 1u) / LORA_MAX_PARTIALS; }

__global__ void __launch_bounds__(256) lora_down_kernel(const uint16_t *x, const uint16_t *normw, float eps, const uint16_t *A, u32 R, u32 K,
                                                        float *partials) {
    __shared__ __attribute__((aligned(16))) uint16_t xs[LORA_MAX_CHUNKS * 64u];
    __shared__ __attribute__((aligned(16))) float items[LORA_MAX_R / 16u * LORA_MAX_CHUNKS * 16u];
    __shared__ float red[4];
    const u32 tid = threadIdx.x, w = tid >> 6, l = tid & 63u;
    const u32 per = lora_chunks_per_slice(K);
    const u32 k0 = blockIdx.x * per * 64u;
    const u32 nkc = min(per, K / 64u - blockIdx.x * per);  // (the last slice may be short)
    float nscale = 1.f;
    if (normw) {
        float ss = 0.f;
        for (u32 u = tid; u < K / 8u; u += 256u) {
            const uint4 v = reinterpret_cast<const uint4 *>(x)[u];
            const u32 ww[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const float a = h2f(ww[i] & 0xFFFF), b = h2f(ww[i] >> 16);
                ss += a * a;
                ss += b * b;
            }
        }
        ss = wave_reduce_bcast<false>(ss);
        if (l == 0) red[w] = ss;
        __syncthreads();
        nscale = 1.0f / sqrtf((red[0] + red[1] + red[2] + red[3]) / (float)K + eps);
    }
    for (u32 u = tid; u < nkc * 8u; u += 256u) {  // the slice of xh: 8 fp16 per thread and turn
        uint4 v = reinterpret_cast<const uint4 *>(x + k0)[u];
        if (normw) {
            const uint4 nv = reinterpret_cast<const uint4 *>(normw + k0)[u];
            u32 ww[4] = {v.x, v.y, v.z, v.w};
            const u32 nw[4] = {nv.x, nv.y, nv.z, nv.w};
#pragma unroll
            for (int i = 0; i < 4; i++) {  // fp16(fp32(x * rs)), then the fp16 product with the weight (dense_stage.h::norm8)
                const h16 a = (h16)gq_pin_f32(h2f(ww[i] & 0xFFFF) * nscale) * u2h((uint16_t)(nw[i] & 0xFFFF));
                const h16 b = (h16)gq_pin_f32(h2f(ww[i] >> 16) * nscale) * u2h((uint16_t)(nw[i] >> 16));
                ww[i] = (u32)h2u(a) | ((u32)h2u(b) << 16);
            }
            v = make_uint4(ww[0], ww[1], ww[2], ww[3]);
        }
        reinterpret_cast<uint4 *>(xs)[u] = v;
    }
    __syncthreads();
    const u32 r = l & 15u, g = l >> 4;
    const u32 nitems = (R / 16u) * nkc;
    for (u32 it = w; it < nitems; it += 4u) {
        const u32 rg = it / nkc, kc = it - rg * nkc;
        const uint4 *ap = reinterpret_cast<const uint4 *>(A + (size_t)(rg * 16u + r) * K + k0 + kc * 64u + 16u * g);
        const uint4 a0 = ap[0], a1 = ap[1];
        uint4 b0 = make_uint4(0u, 0u, 0u, 0u), b1 = b0;
        if (r == 0u) {
            const uint4 *bp = reinterpret_cast<const uint4 *>(xs + kc * 64u + 16u * g);
            b0 = bp[0];
            b1 = bp[1];
        }
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a0), __builtin_bit_cast(f16x8, b0), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a1), __builtin_bit_cast(f16x8, b1), acc, 0, 0, 0);
        // D[row 4 g + e][column r]: column 0 holds the sums
        if (r == 0u) *reinterpret_cast<f32x4 *>(items + (size_t)it * 16u + 4u * g) = acc;
    }
    __syncthreads();
    if (tid < R) {
        const float *p = items + (size_t)(tid >> 4) * nkc * 16u + (tid & 15u);
        float s = 0.f;
        for (u32 kc = 0; kc < nkc; kc++) s += p[kc * 16u];
        partials[(size_t)blockIdx.x * R + tid] = s;
    }
}

struct LoraSegs {
    GqLoraSeg s[3];
    u32 n;
};

__global__ void __launch_bounds__(256) lora_up_kernel(const float *partials, u32 n_partials, u32 R, const uint16_t *B, LoraSegs segs,
                                                      const uint16_t *base, uint16_t *out, u32 N) {
    __shared__ float sub[256];
    __shared__ float t[LORA_MAX_R];
    const u32 tid = threadIdx.x;
    {   // t: Q groups of R threads, group q adds its run of partials in ascending order
        const u32 Q = 256u / R, C = (n_partials + Q - 1u) / Q;
        const u32 q = tid / R, j = tid - q * R;
        if (q < Q) {
            float s = 0.f;
            const u32 p1 = min((q + 1u) * C, n_partials);
            for (u32 p = q * C; p < p1; p++) s += partials[(size_t)p * R + j];
            sub[tid] = s;
        }
        __syncthreads();
        if (tid < R) {
            float s = sub[tid];
            for (u32 qq = 1; qq < Q; qq++) s += sub[qq * R + tid];
            t[tid] = s;
        }
        __syncthreads();
    }
    const u32 row = blockIdx.x * LORA_UP_ROWS + (tid >> 2), part = tid & 3u;
    const u32 rown = min(row, N - 1u);  // (the lanes of rows past N run along for the butterfly and store nothing)
    u32 rb = 0u, rank = 0u, tb = 0u, bo = 0u;
    float sc = 0.f;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        if ((u32)i < segs.n && rown >= segs.s[i].row_begin && rown < segs.s[i].row_end) {
            rb = segs.s[i].row_begin;
            rank = segs.s[i].rank;
            tb = segs.s[i].t_begin;
            bo = segs.s[i].b_offset;
            sc = segs.s[i].scale;
        }
    }
    float acc = 0.f;
    const uint16_t *brow = B + (size_t)bo + (size_t)(rown - rb) * rank;
    for (u32 j = 8u * part; j < rank; j += 32u) {
        const uint4 v = *reinterpret_cast<const uint4 *>(brow + j);
        const u32 ww[4] = {v.x, v.y, v.z, v.w};
        const float *tp = t + tb + j;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            acc = fmaf(h2f(ww[i] & 0xFFFF), tp[2 * i], acc);
            acc = fmaf(h2f(ww[i] >> 16), tp[2 * i + 1], acc);
        }
    }
    acc = row_sum<4>(acc);
    if (part == 0u && row < N) {
        const h16 d = (h16)gq_pin_f32(sc * acc);
        // (a zero d leaves the base as it is, a -0 included: x + (+0) would turn it into +0)
        out[row] = base ? (d == (h16)0.f ? base[row] : h2u(u2h(base[row]) + d)) : h2u(d);
    }
}

}  // namespace

extern "C" uint32_t gq_lora_n_partials(uint32_t K) {
    if (K == 0 || K % 64u || K > 64u * LORA_MAX_CHUNKS * LORA_MAX_PARTIALS) return 0;
    const u32 per = lora_chunks_per_slice(K);
    return (K / 64u + per - 1u) / per;
}

extern "C" int gq_lora_down(const void *x, const void *norm_weight, float eps, const void *A, uint32_t R, uint32_t K, float *partials,
                            void *stream) {
    if (!x || !A || !partials) return gq_fail(GQ_EINVAL, "gq_lora_down: null pointer argument.");
    if (K == 0 || K % 64u) return gq_fail(GQ_EINVAL, "gq_lora_down: K must be a positive multiple of 64.");
    if (R == 0 || R % 16u) return gq_fail(GQ_EINVAL, "gq_lora_down: R must be a positive multiple of 16 (every rank padded to 16).");
    if (((uintptr_t)x | (uintptr_t)norm_weight | (uintptr_t)A | (uintptr_t)partials) & 15u)
        return gq_fail(GQ_EINVAL, "gq_lora_down: x, norm_weight, A and partials must be 16-byte aligned.");
    if (R > LORA_MAX_R) return gq_fail(GQ_ENOTSUP, "gq_lora_down: R above 192.");
    const u32 grid = gq_lora_n_partials(K);
    if (!grid) return gq_fail(GQ_ENOTSUP, "gq_lora_down: K above 65536.");
    hipLaunchKernelGGL(lora_down_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const uint16_t *)x, (const uint16_t *)norm_weight, eps,
                       (const uint16_t *)A, R, K, partials);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}

extern "C" int gq_lora_up(const float *partials, uint32_t n_partials, uint32_t R, const void *B, const GqLoraSeg *segments, uint32_t n_segments,
                          const void *base, void *out, uint32_t N, void *stream) {
    if (!partials || !B || !segments || !out) return gq_fail(GQ_EINVAL, "gq_lora_up: null pointer argument.");
    if (N == 0 || n_partials == 0 || n_partials > LORA_MAX_PARTIALS) return gq_fail(GQ_EINVAL, "gq_lora_up: N > 0 and 1 .. 64 partial sums.");
    if (R == 0 || R % 16u) return gq_fail(GQ_EINVAL, "gq_lora_up: R must be a positive multiple of 16.");
    if (n_segments == 0 || n_segments > 3u) return gq_fail(GQ_EINVAL, "gq_lora_up: 1 .. 3 segments.");
    if ((((uintptr_t)partials | (uintptr_t)B) & 15u) || (((uintptr_t)base | (uintptr_t)out) & 1u))
        return gq_fail(GQ_EINVAL, "gq_lora_up: partials and B must be 16-byte, base and out 2-byte aligned.");
    if (R > LORA_MAX_R) return gq_fail(GQ_ENOTSUP, "gq_lora_up: R above 192.");
    LoraSegs segs = {};
    segs.n = n_segments;
    u32 row = 0;
    for (u32 i = 0; i < n_segments; i++) {
        const GqLoraSeg &s = segments[i];
        if (s.row_begin < row || s.row_end <= s.row_begin || s.row_end > N)
            return gq_fail(GQ_EINVAL, "gq_lora_up: segments must be ascending, disjoint, non-empty and inside the N rows.");
        if (s.rank == 0 || s.rank % 16u || s.rank > 64u || s.t_begin % 16u || s.t_begin + s.rank > R || s.b_offset % 8u)
            return gq_fail(GQ_EINVAL, "gq_lora_up: a segment's rank is 16 .. 64 padded to 16, inside t, its B rows 16-byte aligned.");
        row = s.row_end;
        segs.s[i] = s;
    }
    const u32 grid = (N + LORA_UP_ROWS - 1u) / LORA_UP_ROWS;
    hipLaunchKernelGGL(lora_up_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, partials, n_partials, R, (const uint16_t *)B, segs,
                       (const uint16_t *)base, (uint16_t *)out, N);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}
