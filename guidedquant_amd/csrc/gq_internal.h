// gq_internal.h -- error plumbing shared by the translation units of libgq_hip.so
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <type_traits>

#include "../../include/gq_hip.h"

int gq_fail(int code, const char *msg);            // records msg (thread-local) and returns code
int gq_fail_hip(hipError_t e, const char *where);  // records the HIP error string, returns GQ_EHIP
int gq_env_int(const char *name, int dflt);        // cached getenv -> int (tuning knobs)
int gq_cu_count();                                 // compute units of the CURRENT device (cached per device)

// Statistics hand-over between the launches of a decode step (include/gq_hip.h: gq_anyprec_gemv_fused_ho): what the caller asked for,
// and whether the GEMV kernel that ran wrote the partial sums itself (else the dispatcher adds gq_ssq_rows)
struct GqHandover {
    const float *ssq_in = nullptr;
    float *ssq_out = nullptr;
    bool ssq_written = false;   // the GEMV kernel writes ssq_out in its epilogue
    bool ssq_consumed = false;  // the GEMV kernel's RMSNorm prologue reads ssq_in
};

// The route record of the AP-GEMV dispatch (include/gq_hip.h: gq_debug_ap_last_route, ap_dispatch.hip).  Every terminal launch site of the
// dispatch calls gq_ap_route right in front of its launch, and launches nothing when it returns true: the dispatch is a dry run
// (gq_anyprec_handover_plan, gq_debug_ap_plan_route), which takes every decision a real one takes.
bool gq_ap_route(uint32_t family, uint32_t launches, uint32_t variant = 0u);

// One-time per-DEVICE actions (function attributes such as the > 64 KiB dynamic-LDS opt-in are per device: a process that
// drives several GPUs -- reference-style sequential sharding, device_map -- must repeat them on each one).
struct GqPerDeviceOnce {
    std::atomic<unsigned long long> done[4] = {{0}, {0}, {0}, {0}};
    // raise the kernel's dynamic-LDS limit once per device.  A device is marked only AFTER the call succeeded: a failure (a sticky
    // error, a call during capture) is reported and retried by the next launch instead of leaving the opt-in undone for good.
    // Racing threads may both make the call: it is idempotent.
    hipError_t max_dynamic_lds(const void *func, int bytes) {
        int dev = 0;
        const bool known = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 256;
        const unsigned long long bit = 1ull << (dev & 63);
        if (known && (done[dev >> 6].load(std::memory_order_acquire) & bit)) return hipSuccess;
        const hipError_t e = hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e == hipSuccess && known) done[dev >> 6].fetch_or(bit, std::memory_order_release);
        return e;
    }
};

// The top-n selection behind a sampler's launches (topn.hip; the entry points are gq_sample_topk_lp_topn there and gq_sample_full_topn in
// sampler_full.hip, which knows where its partials lie).  gq_topn_check: the refusals of include/gq_hip.h, nothing launched; lse_source: the
// sampler's log-sum-exp partials as the request will leave them, NULL when it asks for no lp_raw.  gq_topn_launch: the launch pair;
// lse_part = 2 * 128 floats, (m_b) then (z_b), as the sampler's own last launch reads them.
int gq_topn_check(uint32_t vocab, int n, const void *top_ids, const void *top_lps, const void *ws, const void *lse_source);
int gq_topn_launch(const void *logits, uint32_t vocab, int n, const float *lse_part, const int *pos_io, int *top_ids, float *top_lps, uint32_t cap,
                   void *ws, void *stream);

// Host pieces the two QTIP translation units share (qtip.hip: the trellis side, qtip_xf.hip: the transform side, which defines them).
extern unsigned long long *g_qdbg;  // optional per-wave phase stamps (gq_debug_set_qtip_timing_buffer; tools/qtip_phase_timing.py)
float gq_inv_sqrt_f(uint32_t n);    // (float)n^-1/2, rounded from double like the scale argument of hadamard()
namespace gqq {
struct QtipOut;  // csrc/qtip_xform.h: the kernels' form of a GqQtipOut
}
// What every entry point asks of a GqQtipOut -- sums and scales (need_out: and the output) not null, parts <= 4 -- and its kernel
// form (mscale = M^-1/2, parts 0 -> 1).  Widths, alignments and the error texts stay with the entry points.
enum GqQtipOutErr { GQ_QOUT_OK = 0, GQ_QOUT_NULL, GQ_QOUT_PARTS };
GqQtipOutErr gq_qtip_out_desc(const GqQtipOut &g, bool need_out, gqq::QtipOut &o);

// Phase stamps (tools/phase_timing.py, qtip_phase_timing.py, qtip_mid_timing.py: per-wave shader-clock timestamps into a debug buffer)
// are compiled OUT of the shipped library: even switched off at run time every stamp site costs a wave two or three scalar
// instructions and a branch on its critical path (the stream kernel's prologue alone had ~20 sites).  A library with the sites:
//   tools/build_variant.sh stamps ap_stream.hip -DGQ_STAMPS=1   (one translation unit per variant; select with GQ_LIB_PATH)
#ifndef GQ_STAMPS
#define GQ_STAMPS 0
#endif

// waves of an attention block (decode.hip; the head blocks inside the wqkv launch, ap_stream.hip::ap_qkv_attn_kernel, run the same code)
#ifndef GQ_ATTN_WAVES
#define GQ_ATTN_WAVES 8
#endif

#if defined(__HIPCC__)
// `(half)(a * b)` on floats: the compiler folds the conversion into v_fma_mixlo_f16, which rounds the EXACT product once.
// The reference's torch ops round the fp32 product first and convert then (two roundings; they differ on fp16 ties of the
// fp32 value).  Pinning the product in a register keeps the two-step rounding.
__device__ __forceinline__ float gq_pin_f32(float v) {
    asm volatile("" : "+v"(v));
    return v;
}

// Hand-off stores: what a launch of the decode step writes is read by the NEXT launch, mostly from other XCDs.  A plain store
// leaves the line dirty in the writer's XCD L2 until the end-of-kernel write-back; a write-through store (sc1) puts it in
// memory at once.  Used where it measured faster -- the outputs of the plane GEMV kernels (four of the five launches of a layer,
// 8 .. 28 KiB each): 8B decode 828 -> 843 tokens/s, same box, alternating, three rounds.  Measured neutral or slower and left
// plain: the attention output, the 128 K two-byte logits of the lm_head (one fabric write each), the sampler / embedding
// outputs, the fp32 sums of the QTIP engine, the outputs of the exact-mode GEMV kernels (564-566 vs 568-570 tokens/s).  GQ_WT_STORES=0 at build time brings the plain stores back.
#ifndef GQ_WT_STORES
#define GQ_WT_STORES 1
#endif
__device__ __forceinline__ void gq_store_wt(uint16_t *p, uint16_t v) {
#if GQ_WT_STORES
    asm volatile("global_store_short %0, %1, off sc1" ::"v"(p), "v"((uint32_t)v) : "memory");
#else
    *p = v;
#endif
}
__device__ __forceinline__ void gq_store_wt(uint32_t *p, uint32_t v) {
#if GQ_WT_STORES
    asm volatile("global_store_dword %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
#else
    *p = v;
#endif
}
__device__ __forceinline__ void gq_store_wt(int *p, int v) { gq_store_wt(reinterpret_cast<uint32_t *>(p), (uint32_t)v); }
__device__ __forceinline__ void gq_store_wt(float *p, float v) { gq_store_wt(reinterpret_cast<uint32_t *>(p), __builtin_bit_cast(uint32_t, v)); }
__device__ __forceinline__ void gq_store_wt(uint2 *p, uint2 v) {
#if GQ_WT_STORES
    typedef uint32_t gq_u32x2 __attribute__((ext_vector_type(2)));
    const gq_u32x2 t = {v.x, v.y};
    asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"(p), "v"(t) : "memory");
#else
    *p = v;
#endif
}
__device__ __forceinline__ void gq_store_wt(uint4 *p, uint4 v) {
#if GQ_WT_STORES
    typedef uint32_t gq_u32x4 __attribute__((ext_vector_type(4)));
    const gq_u32x4 t = {v.x, v.y, v.z, v.w};
    asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(t) : "memory");
#else
    *p = v;
#endif
}
#endif

#define GQ_STR2(x) #x
#define GQ_STR(x) GQ_STR2(x)
#define GQ_HIP_CHECK(expr)                                                        \
    do {                                                                          \
        hipError_t e__ = (expr);                                                  \
        if (e__ != hipSuccess) return gq_fail_hip(e__, __FILE__ ":" GQ_STR(__LINE__)); \
    } while (0)
