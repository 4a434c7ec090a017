// ap_dispatch.h -- the interface between the translation units of the Any-Precision GEMV: one launch descriptor, and every function one
// of them defines for another.  ap_dispatch.hip decides which kernel family serves a launch ("Dispatch order"); a kernel file
// (ap_gemv.hip, ap_dq.hip, ap_plane.hip, ap_stream.hip, ap_wide.hip) only serves the launch it is handed, or returns GQ_ENOTSUP.
#pragma once
#include <type_traits>

#include "gq_internal.h"

// the fused prologue of a launch (a template parameter of every GEMV kernel)
enum { PRO_NONE = 0, PRO_RMSNORM = 1, PRO_SILUMUL = 2 };

// One AP-GEMV launch as the entry points received it.  ApArgs, PlaneArgs and StreamArgs are what a kernel file makes of it for its kernel.
struct ApLaunch {
    const uint16_t *x;      // [M][K] ([M][2K] behind the SiLU-mul prologue)
    uint16_t *out;          // [M][N] ([N/2] with the SiLU-pairs epilogue)
    const uint32_t *qweight;  // [bits][N][K/32]
    const uint16_t *lut;    // [N][2^bits]
    const uint16_t *normw;  // [K]: the RMSNorm prologue's weight, or null
    const uint16_t *resid;  // [N]: the residual epilogue's addend, or null
    float eps;
    uint32_t M, N, K;
    int bits;
    int pro;                // PRO_*, and ...
    bool pairs;             // ... GQ_EPI_SILU_PAIRS: both follow from normw and epilogue, in derive() and nowhere else
    uint32_t epilogue;      // the GQ_EPI_* / GQ_PRO_* flags
    void *ws;               // optional caller workspace (gq_anyprec_gemv_fused_ws) and its size
    size_t ws_bytes;
    hipStream_t stream;
    GqHandover *ho;         // statistics hand-over (gq_anyprec_gemv_fused_ho), or null

    void derive() {
        pro = normw ? PRO_RMSNORM : ((epilogue & GQ_PRO_SILU_MUL) ? PRO_SILUMUL : PRO_NONE);
        pairs = (epilogue & GQ_EPI_SILU_PAIRS) != 0;
    }
    bool unaligned16() const { return (((uintptr_t)qweight | (uintptr_t)x | (uintptr_t)normw | (uintptr_t)lut) & 15u) != 0; }
    uint64_t qbytes() const { return (uint64_t)bits * N * (K / 8u); }  // (the kernels index the planes with 32-bit byte offsets)
};

// f(std::integral_constant<int, B>) for the B in [LO, HI] that equals bits; GQ_ENOTSUP for a width outside the range
template <int LO, int HI, class F>
int gq_with_bits(int bits, F &&f) {
    if constexpr (LO > HI) return GQ_ENOTSUP;
    else return bits == LO ? f(std::integral_constant<int, LO>{}) : gq_with_bits<LO + 1, HI>(bits, f);
}

// ---- ap_dispatch.hip
bool gq_ap_exact_mode();  // gq_set_ap_mode / GQ_AP_EXACT: the fp16-order kernels only

// ---- the kernel files: serve the launch, or GQ_ENOTSUP (shape, bit width, alignment: each checks what its kernels need)
int gq_ap_dq_try(const ApLaunch &L);          // ap_dq.hip: decode-to-fp16 on the matrix cores, bits 2..4, M = 1
int gq_ap_pair_table_try(const ApLaunch &L);  // ap_gemv.hip: the 2-bit LDS pair-table kernel, where GQ_AP_PT asks for it
int gq_ap_exact_try(const ApLaunch &L);       // ap_gemv.hip: the fp16-order v_perm kernel, bits 2..4
int gq_ap_generic(const ApLaunch &L);         // ap_gemv.hip: the reference-shaped kernel, plain launches only (the caller checks)
int gq_ap_wide_try(const ApLaunch &L);        // ap_wide.hip: the LDS-table kernel, bits 5..8, M = 1
int gq_plane_gemv_try(const ApLaunch &L);     // ap_plane.hip: plane-MFMA kernels; rows of 16384 < K <= 32768 as a chain of two launches
bool gq_plane_local_shape(uint32_t N, uint32_t K, int bits);
int gq_stream_gemv_try(const ApLaunch &L);     // ap_stream.hip: M = 1
int gq_stream_gemv_ksplit(const ApLaunch &L);  // ap_stream.hip: K split over blocks into L.ws, plain / residual epilogue
size_t gq_stream_ksplit_ws_bytes(uint32_t N, uint32_t K, int bits);
unsigned long long *gq_debug_timing_buffer();  // ap_plane.hip (gq_debug_set_timing_buffer): every kernel file stamps into the same buffer
// ap_gemm_wide.hip: gq_anyprec_gemm / gq_anyprec_gemm_ws (ap_gemm.hip) at 5..8 bits
int gq_ap_gemm_wide(const void *x, void *out, const uint32_t *qweight, const void *lut, uint32_t S, uint32_t N, uint32_t K, int bits,
                    hipStream_t stream);
