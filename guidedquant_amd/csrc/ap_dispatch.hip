// ap_dispatch.hip -- which kernel family serves an Any-Precision GEMV launch: the argument checks, the mode, the route record, the
// ordered list of "try this family under this condition" (ap_serve; DESIGN.md, "Dispatch order") and the entry points of include/gq_hip.h
// that are nothing but that.  No GEMV kernel lives here: the families are ap_gemv.hip (exact, pair-table, generic), ap_dq.hip (dq), ap_plane.hip
// (plane, plane-local, plane-chain), ap_stream.hip (stream, stream-ksplit) and ap_wide.hip (wide), behind the entries of ap_dispatch.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ap_exact.h"

#ifndef GQ_DQ_DEFAULT
#define GQ_DQ_DEFAULT 6  // (bit mask over the bit widths 2, 3, 4 the decode-to-fp16 kernel may take: 3 and 4)
#endif

namespace {

int g_ap_mode = -1;  // -1: unset (env GQ_AP_MODE or default fast), 0: fast (plane-MFMA), 1: exact (fp16-order)

// Stand-alone producer of the hand-over statistics: GQ_SSQ_SLOTS partial sums of squares of an fp16 vector (slot t: elements t, t + 1024,
// ..).  What a GEMV launch without the in-epilogue form is followed by when the caller asked for ssq_out; also gq_ssq_rows.
__global__ void __launch_bounds__(GQ_SSQ_SLOTS) ssq_rows_kernel(const uint16_t *x, u32 n, float *ssq) {
    float acc = 0.f;
    for (u32 i = threadIdx.x; i < n; i += (u32)GQ_SSQ_SLOTS) {
        const float v = h2f(x[i]);
        acc += v * v;
    }
    gq_store_wt(ssq + threadIdx.x, acc);
}

// the route record (gq_internal.h: gq_ap_route) of the calling thread, and whether its dispatch is a dry run
thread_local uint32_t t_route[3] = {GQ_AP_ROUTE_NONE, 0u, 0u};
thread_local bool t_dry = false;
}  // namespace
bool gq_ap_exact_mode() {
    if (g_ap_mode >= 0) return g_ap_mode == 1;
    return gq_env_int("GQ_AP_EXACT", 0) != 0;
}
bool gq_ap_route(uint32_t family, uint32_t launches, uint32_t variant) {
    t_route[0] = family, t_route[1] = launches, t_route[2] = variant;
    return t_dry;
}
namespace {

// what every entry point refuses, real or dry: the launch forms first, then shape and pointers
int ap_validate(const ApLaunch &L) {
    if (L.M != 1u && (L.normw || L.epilogue || L.ws_bytes)) return gq_fail(GQ_EINVAL, "prologue / epilogue / workspace: M = 1 only.");
    if ((L.epilogue & GQ_EPI_RESIDUAL) && !L.resid) return gq_fail(GQ_EINVAL, "RESIDUAL epilogue needs a residual pointer.");
    if ((L.epilogue & GQ_PRO_SILU_MUL) && L.normw) return gq_fail(GQ_EINVAL, "RMSNorm and SiLU-mul prologues are exclusive.");
    if (L.pairs && ((L.epilogue & GQ_EPI_RESIDUAL) || (L.N & 1u)))
        return gq_fail(GQ_EINVAL, "SILU_PAIRS epilogue needs an even N and excludes the residual epilogue.");
    if (L.ho && L.ho->ssq_out && (L.pairs || L.M != 1u)) return gq_fail(GQ_EINVAL, "ssq_out: plain / residual epilogue, M = 1 only.");
    if (L.bits < 2 || L.bits > 8) return gq_fail(GQ_EINVAL, "Bitwidth must be between 2 and 8.");
    if (L.M < 1 || L.M > 8) return gq_fail(GQ_EINVAL, "batch size M must be between 1 and 8 (anyprec.cu:602).");
    if (L.K == 0 || L.K % 32u) return gq_fail(GQ_EINVAL, "input_feat (K) must be a positive multiple of 32.");
    if (L.N == 0) return gq_fail(GQ_EINVAL, "output_feat (N) must be positive.");
    if (!L.x || !L.out || !L.qweight || !L.lut) return gq_fail(GQ_EINVAL, "null pointer argument.");
    return GQ_OK;
}

// round 6: decode-to-fp16 on the matrix cores (ap_gemv_dq_kernel) where it measured faster than the other kernels
// (profiles/r06_dq_kernel.txt, 8B shapes, decode-graph launch forms, same box): at 4 bits every matrix of >= 16 M weights -- wqkv 9.1
// vs 10.3 us, wo 6.6 vs 6.8 (exact kernel), w1w3 22.9 vs 24.4, w2 13.9 vs 15.0 --, at 3 bits the matrices of 16 .. 32 M weights (wqkv
// 6.5 vs 7.2, wo 4.9 vs 5.3; Llama-2-7B's wqkv 50 M 8.1 vs 9.5, w1w3 90 M 12.7 vs 14.2) up to 100 M, and the long-row launches
// without the RMSNorm prologue at any size (8B w2 9.35 vs 9.65, 70B w2 235 M 26.5 vs 34.8; 70B wqkv 84 M 13.2 vs 14.8); the big
// RMSNorm + pair launches stay on the plane kernel (70B w1w3 470 M 45.7 vs 43.0; 8B w1w3 117 M was 15.3 vs 14.8 and, with the item
// loop's divisions gone, is 14.6 vs 14.8 alone and 13.5 vs 14.0 in the decode graph: 3-bit decode 720 -> 736 tokens/s -- the bound moved
// from 100 M to 200 M); never at 2 bits
// (8B w1w3 11.6 vs 8.5, 70B w1w3 37 vs 25).
// GQ_DQ: bit mask of the widths it may take (bit b - 2; 0 = never), GQ_DQ_MIN_MWEIGHTS >= 0: every matrix of at least that many
// million weights at those widths.
bool dq_gate(const ApLaunch &L) {
    const int dq_mask = gq_env_int("GQ_DQ", GQ_DQ_DEFAULT), dq_min = gq_env_int("GQ_DQ_MIN_MWEIGHTS", -1);
    const uint64_t nk = (uint64_t)L.N * L.K;
    const bool dq_shape = dq_min >= 0 ? nk >= (uint64_t)dq_min * 1000000ull
                                      // (and at least one 16-row group per CU: Llama-3.2-1B's w2, 2048 x 8192 = 128 blocks, is faster on the
                                      // exact kernel -- 4-bit 1B decode 1555 vs 1508 tokens/s; Llama-3.3-70B at 4 bits: 72 -> 86 tokens/s here)
                                      : (L.N >= 4096u &&
                                         (L.bits == 4 ? nk >= 16000000ull
                                                      : (L.bits == 3 && nk >= 16000000ull &&
                                                         (nk < 200000000ull || (L.pro != PRO_RMSNORM && L.K >= 8192u)))));
    return L.bits <= 4 && ((dq_mask >> (L.bits - 2)) & 1) && dq_shape;
}

// fast mode serves the shapes on which the plane-MFMA kernel beats the exact kernel (measured):
// 2-bit matrices of >= 20 M weights (wqkv, w1w3, w2 of the 8B / 70B models), 3- and 4-bit matrices of >= 32 M weights
// (w1w3, w2); everything else runs the exact kernels, whose results are bit-identical to the reference.
// GQ_PL_MIN_MWEIGHTS overrides the threshold for every bit width, GQ_PL_MAX_BITS the widest plane-served width.
bool plane_gate(const ApLaunch &L) {
    const int env_min = gq_env_int("GQ_PL_MIN_MWEIGHTS", -1);
    // (matrices of <= 16 rows per CU without the RMSNorm prologue run the local-image variant, which needs no block-wide
    // activation pass: >= 16 M weights at 2 and 3 bits -- wo)
    const bool local = L.pro != PRO_RMSNORM && L.bits <= 3 && gq_plane_local_shape(L.N, L.K, L.bits);
    // (round 5: behind the RMSNorm prologue the plane kernel wins from 20 M weights at 3 and 4 bits too -- 8B wqkv, 25 M: 7.2 vs 8.4 us
    // at 3 bits, 10.2 vs 12.0 at 4 -- the exact kernel normalises the whole vector in every block in front of its first row step;
    // without the prologue the 32 M threshold stands: wo at 4 bits 6.6 exact vs 7.6 plane.  profiles/r05_dispatch_3_4_bits.txt)
    const int def_min = local ? 16 : ((L.bits == 2 || L.pro == PRO_RMSNORM) ? 20 : 32);
    const uint64_t min_w = (uint64_t)(env_min >= 0 ? env_min : def_min) * 1000000ull;
    const int max_bits = gq_env_int("GQ_PL_MAX_BITS", 4);
    return L.bits <= max_bits && (uint64_t)L.N * L.K >= min_w;
}

// the stream kernel (ap_stream.hip) first where it measured faster (profiles/r04_stream_kernel.txt): the RMSNorm-prologue
// launches of the widths up to 4096 at 2 bits (8B wqkv / w1w3); GQ_ST = 0 never, 2 every shape it serves, 3 every prologue too
bool stream_first(const ApLaunch &L) {
    const int st = gq_env_int("GQ_ST", 1);
    // (and the 70B attention output projection, 8192 x 8192 without a prologue: 7.6 vs 7.9 us)
    return st >= 3 || (st == 2 && L.pro == PRO_RMSNORM) || (st == 1 && L.pro == PRO_RMSNORM && L.bits == 2 && L.K <= 4096u) ||
           (st == 1 && L.pro == PRO_NONE && !L.pairs && L.bits == 2 && L.K == 8192u && L.N >= 8192u && L.M == 1u) ||
           // (round 5: and the plain launch -- the reference's own operator -- of the 8B gate / up matrix: 8.39 vs 9.26 us; wqkv, wo
           // and w2 stay on the plane kernels: 4.95 / 4.03 / 6.44 vs 5.26 / 4.68 / 7.62.  profiles/r05_plain_launch_dispatch.txt)
           (st == 1 && L.pro == PRO_NONE && L.bits == 2 && L.K <= 4096u && (uint64_t)L.N * L.K >= 100000000ull && L.M == 1u);
}

// rows of 16384 < K <= 32768 (the 70B down projection) with a workspace: K split over blocks, one fp16 rounding (ap_stream.hip);
// without one they are ap_plane.hip's chain of two launches, which rounds twice.  Plain and residual epilogues only.
bool ksplit_first(const ApLaunch &L) {
    return L.K > 16384u && L.K <= 32768u && L.K % 256u == 0u && L.pro == PRO_NONE && !L.pairs && L.ws && L.M == 1u;
}

// The dispatch order: the first family whose condition holds and whose try entry does not answer GQ_ENOTSUP serves the launch.
int ap_serve(const ApLaunch &L) {
    const bool force_generic = gq_env_int("GQ_AP_FORCE_GENERIC", 0) != 0;
    const bool fast = !force_generic && !gq_ap_exact_mode();
    int rc = GQ_ENOTSUP;
    if (fast && dq_gate(L)) rc = gq_ap_dq_try(L);
    if (rc == GQ_ENOTSUP && fast && plane_gate(L)) {
        if (stream_first(L)) rc = gq_stream_gemv_try(L);
        if (rc == GQ_ENOTSUP && ksplit_first(L)) rc = gq_stream_gemv_ksplit(L);
        if (rc == GQ_ENOTSUP) rc = gq_plane_gemv_try(L);
    }
    // round 6: the pair-table kernel (GQ_AP_PT: 0 never -- the default --, 1 rows of >= 8192 weights, 2 every shape it serves).  It had
    // measured faster on 8B w2 (11.3 vs 12.7 us) while BOTH kernels ran that launch in two rounds of blocks (pick_quad_cfg: blocks per
    // CU beyond the occupancy); in one round the v_perm kernel is the faster one on every Llama shape (8B w2 8.9 vs 9.9 us; 70B w2 26.0
    // vs 33.6, wqkv 12.4 vs 13.5, wo 8.7 vs 10.0) except 70B w1w3 (41.7 vs 38.1): profiles/r06_exact_pair_table.txt, r06_exact_epilogue.txt
    if (rc == GQ_ENOTSUP && !force_generic) rc = gq_ap_pair_table_try(L);
    if (rc == GQ_ENOTSUP && !force_generic) rc = gq_ap_exact_try(L);
    // bits 5..8, one batch row, both modes: the LDS-table kernel (ap_wide.hip), in the reference's order like the generic kernel
    if (rc == GQ_ENOTSUP && !force_generic && L.bits >= 5) rc = gq_ap_wide_try(L);
    if (rc != GQ_ENOTSUP) return rc;
    if (L.pro != PRO_NONE || L.pairs)
        return gq_fail(GQ_ENOTSUP, "fused prologue / pair epilogue needs K % 128 == 0 (<= 32768 at 5..8 bits) and 16-byte aligned buffers.");
    if ((uintptr_t)L.x & 15u) return gq_fail(GQ_EINVAL, "input must be 16-byte aligned.");
    return gq_ap_generic(L);
}

int ssq_rows_launch(const uint16_t *x, u32 n, float *ssq_out, hipStream_t s) {
    hipLaunchKernelGGL(ssq_rows_kernel, dim3(1), dim3(GQ_SSQ_SLOTS), 0, s, x, n, ssq_out);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}

// One dispatch, real or dry (gq_ap_route: a dry one takes every decision of a real one and launches nothing)
int ap_dispatch(ApLaunch L, bool dry) {
    gq_ap_route(GQ_AP_ROUTE_NONE, 0u);  // (until a launch site records what it launches)
    L.derive();
    int rc = ap_validate(L);
    if (rc != GQ_OK) return rc;
    t_dry = dry;
    rc = ap_serve(L);
    t_dry = false;
    if (rc == GQ_OK && !dry && L.ho && L.ho->ssq_out && !L.ho->ssq_written) {  // the kernel that served the shape has no in-epilogue form: one small launch more
        rc = ssq_rows_launch(L.out, L.N, L.ho->ssq_out, L.stream);
        if (rc == GQ_OK) t_route[1]++;
    }
    return rc;
}

alignas(16) unsigned char g_stand_in[16];  // (a 16-byte aligned stand-in for every pointer of a dry dispatch: never dereferenced)
// a dry dispatch of the launch form: M rows, the RMSNorm prologue, the epilogue flags and the workspace as given
int ap_dry_dispatch(u32 N, u32 K, int bits, u32 M, bool has_norm, u32 epilogue, size_t ws_bytes, GqHandover *ho) {
    const uint16_t *al = (const uint16_t *)(void *)g_stand_in;
    ApLaunch L{};
    L.x = L.lut = al, L.out = (uint16_t *)g_stand_in, L.qweight = (const u32 *)(void *)g_stand_in;
    L.normw = has_norm ? al : nullptr;
    L.resid = (epilogue & GQ_EPI_RESIDUAL) ? al : nullptr;
    L.ws = ws_bytes ? g_stand_in : nullptr;
    L.ws_bytes = ws_bytes;
    L.N = N, L.K = K, L.M = M, L.bits = bits, L.epilogue = epilogue, L.ho = ho;
    return ap_dispatch(L, true);
}

}  // namespace

extern "C" int gq_set_ap_mode(int mode) {
    if (mode < -1 || mode > 1) return gq_fail(GQ_EINVAL, "mode must be -1 (default), 0 (fast) or 1 (exact)");
    g_ap_mode = mode;
    return GQ_OK;
}

extern "C" int gq_anyprec_gemv(const void *x, void *out, const uint32_t *qweight, const void *lut, uint32_t M, uint32_t N,
                               uint32_t K, int bits, int dtype, void *stream) {
    if (dtype != GQ_DTYPE_F16) return gq_fail(GQ_ENOTSUP, "only fp16 is implemented (as in the reference, gemv.cu:46-49).");
    GqHandover ho;
    ApLaunch L{};
    L.x = (const uint16_t *)x, L.out = (uint16_t *)out, L.qweight = qweight, L.lut = (const uint16_t *)lut;
    L.M = M, L.N = N, L.K = K, L.bits = bits, L.epilogue = GQ_EPI_NONE, L.stream = (hipStream_t)stream, L.ho = &ho;
    return ap_dispatch(L, false);
}

extern "C" size_t gq_anyprec_gemv_fused_ws_bytes(uint32_t N, uint32_t K, int bits, uint32_t epilogue) {
    if ((epilogue & (GQ_PRO_SILU_MUL | GQ_EPI_SILU_PAIRS)) || gq_ap_exact_mode()) return 0;
    return gq_stream_ksplit_ws_bytes(N, K, bits);
}
extern "C" int gq_anyprec_gemv_fused(const void *x, void *out, const uint32_t *qweight, const void *lut, uint32_t N,
                                     uint32_t K, int bits, const void *norm_weight, float eps, const void *residual,
                                     uint32_t epilogue, void *stream) {
    return gq_anyprec_gemv_fused_ws(x, out, qweight, lut, N, K, bits, norm_weight, eps, residual, epilogue, nullptr, 0, stream);
}
extern "C" int gq_anyprec_gemv_fused_ws(const void *x, void *out, const uint32_t *qweight, const void *lut, uint32_t N,
                                        uint32_t K, int bits, const void *norm_weight, float eps, const void *residual,
                                        uint32_t epilogue, void *workspace, size_t workspace_bytes, void *stream) {
    return gq_anyprec_gemv_fused_ho(x, out, qweight, lut, N, K, bits, norm_weight, eps, residual, epilogue, workspace, workspace_bytes, nullptr,
                                    nullptr, stream);
}
extern "C" int gq_anyprec_gemv_fused_ho(const void *x, void *out, const uint32_t *qweight, const void *lut, uint32_t N,
                                        uint32_t K, int bits, const void *norm_weight, float eps, const void *residual,
                                        uint32_t epilogue, void *workspace, size_t workspace_bytes, const float *ssq_in, float *ssq_out,
                                        void *stream) {
    GqHandover ho;
    ho.ssq_in = norm_weight ? ssq_in : nullptr;
    ho.ssq_out = ssq_out;
    ApLaunch L{};
    L.x = (const uint16_t *)x, L.out = (uint16_t *)out, L.qweight = qweight, L.lut = (const uint16_t *)lut;
    L.normw = (const uint16_t *)norm_weight;
    L.resid = (epilogue & GQ_EPI_RESIDUAL) ? (const uint16_t *)residual : nullptr;
    L.eps = eps;
    L.M = 1u, L.N = N, L.K = K, L.bits = bits, L.epilogue = epilogue;
    L.ws = workspace;
    L.ws_bytes = workspace ? workspace_bytes : 0;
    L.stream = (hipStream_t)stream, L.ho = &ho;
    return ap_dispatch(L, false);
}

extern "C" int gq_anyprec_handover_plan(uint32_t N, uint32_t K, int bits, int has_norm, uint32_t epilogue) {
    // which kernel would serve the launch, without launching: 1 = its RMSNorm prologue reads ssq_in, 2 = its epilogue writes ssq_out
    GqHandover ho;
    ho.ssq_in = (const float *)(void *)g_stand_in;
    ho.ssq_out = (epilogue & GQ_EPI_SILU_PAIRS) ? nullptr : (float *)(void *)g_stand_in;
    if (ap_dry_dispatch(N, K, bits, 1u, has_norm != 0, epilogue, 0, &ho) != GQ_OK) return 0;
    return (ho.ssq_consumed ? 1 : 0) | (ho.ssq_written ? 2 : 0);
}
extern "C" int gq_debug_ap_plan_route(uint32_t N, uint32_t K, int bits, uint32_t M, int has_norm, uint32_t epilogue, size_t ws_bytes,
                                      uint32_t *route) {
    if (!route) return gq_fail(GQ_EINVAL, "null pointer argument.");
    GqHandover ho;
    const int rc = ap_dry_dispatch(N, K, bits, M, has_norm != 0, epilogue, ws_bytes, &ho);
    for (int i = 0; i < 3; i++) route[i] = t_route[i];
    return rc;
}
extern "C" int gq_debug_ap_last_route(uint32_t *route) {
    if (!route) return gq_fail(GQ_EINVAL, "null pointer argument.");
    for (int i = 0; i < 3; i++) route[i] = t_route[i];
    return GQ_OK;
}
extern "C" int gq_ssq_rows(const void *x, uint32_t n, float *ssq_out, void *stream) {
    if (!x || !ssq_out || n == 0) return gq_fail(GQ_EINVAL, "null pointer argument / empty vector.");
    return ssq_rows_launch((const uint16_t *)x, n, ssq_out, (hipStream_t)stream);
}
