// sampler_full.hip -- the fused sampler over the WHOLE vocabulary, gfx950: gq_sample_full (include/gq_hip.h has the contract).  No limit of
// 64 candidates: top_k == 0 (no filter) or any top_k >= 1, a nucleus over the top-k survivors, min_p, with gq_sample_topk_rep's penalty
// and token sets, gq_sample_topk_lp's two log-probabilities and the same race, counter, publishing and embedding fold.
//
// The passes are ordered by kernel boundaries only; their grids depend on nothing but the build:
//   full_zero    128 blocks  the two count histograms are cleared
//   full_hist    128 blocks  every live token counts in the bin of its RAW fp16 logit: histogram P (not penalised) or N (penalised).  A bin
//                            of P holds one value v, a bin of N one value pen(v) -- and pen is monotone, so both histograms are sorted by
//                            their bin index.  Integer atomics: the counts do not depend on the order.  (lp_raw: the slice's (max, sum exp).)
//                            One integer atomic per wave leaves the image of the first token of the order.
//   full_scan    1 block     suffix sums of count and of mass (count * w(value) in fixed point, w * 2^44 in 64 bits: exact integer sums) over
//                            both histograms; wave 0 then finds the three cuts by 64-way searches on the 32-bit value image -- the number
//                            of tokens / the mass at or above an image is one look-up per histogram, the bin found by bisecting the
//                            image function in registers -- and leaves ONE cut (image Kc, rc = how many of the tokens AT Kc stay, lowest
//                            ids first) and the report.
//   full_ties    128 blocks  the number of live tokens at Kc per slice (slices hold consecutive ids: the rank by id inside the value Kc
//                            is a prefix over these counts); nothing to do when every token at Kc stays.
//   full_race    128 blocks  the exponential race over the slice's candidates: the best (score, id) per block.
//   full_finish  1 block     the best of the 128, the log-probabilities, publishing, the embedding fold.
// gq_sample_full_topn (at the end of the file): the same six launches, then topn.hip's pair, which reads the partials full_hist left at WS_LP.
// gq_sample_full_fsm: gq_sample_full_adj's launches with a token-level state machine: the forbidden set of the machine's state (a row of
// its masks, chosen by a device word) stands in for `suppress` in the three passes that read it, full_finish makes the transition.
// gq_sample_full_adj: the same six launches with the ADJ instances of the four kernels that read tokens -- a member token's adjusted fp16
// pattern (gqs::adjust16) stands in for its logit in liveness, the histogram bin, the value s, the ties and the race; the log-probability
// partials and lp_raw keep the raw pattern; full_finish counts the drawn token.
// The value images, the penalty, the ban list, the race, the log-sum-exp merge, publishing and the embedding fold are sampler_core.h's: the
// functions sampler.hip's kernels are built from, so the two samplers agree bit for bit where their contracts say so.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "gq_internal.h"
#include "sampler_core.h"
#include "wave_util.h"

namespace {

using namespace gqs;
using gqw::h2f;

constexpr int FB = 128, FT = 256, EPT = 8;  // blocks, threads, consecutive tokens per thread: slices of <= 2048 logits
static_assert((u32)FB * FT * EPT == GQ_SAMPLER_MAX_VOCAB, "one slice position per thread and element");
constexpr u32 NBIN = 65536u, SPN = 65600u;  // bins of a histogram; entries of a suffix array (NBIN + 1, padded)
constexpr u32 OLO = 0x03FFu, OHI = 0xFC00u;  // the bins of -inf and +inf: the ones outside hold NaN patterns and stay empty
constexpr double WONE = 17592186044416.0;    // 2^44: the fixed-point unit of a mass (262144 tokens of w <= 1: sums < 2^63)
constexpr u32 ALL = 0xFFFFFFFFu;

// workspace (bytes): the report, the cut, the per-block partials, the histograms and their suffix arrays
constexpr size_t WS_CUT = 32, WS_MAXKEY = 56, WS_TIES = 64, WS_BEST = WS_TIES + 4 * FB, WS_LP = WS_BEST + 8 * FB, WS_HIST = 4096;
constexpr size_t WS_SPC = WS_HIST + 2 * 4 * (size_t)NBIN, WS_SPM = WS_SPC + 2 * 4 * (size_t)SPN, WS_BYTES = WS_SPM + 2 * 8 * (size_t)SPN;
static_assert(WS_LP + 8 * FB <= WS_HIST && WS_SPM % 16 == 0, "layout");
struct Report {  // the first 24 bytes of the workspace (the documented test hook)
    u32 n, n_k;
    double Z_k, Z_kept;
};
struct Cut {  // at WS_CUT
    u32 Kc, rc, gc;  // candidates: image > Kc, and the first rc (by id) of the gc tokens at Kc
    float m;         // a of the first token of the order
    u64 zkept;       // sum of w over the candidates, fixed point
};

__device__ __forceinline__ u32 image_of(float s) {
    return ordered_key32(__builtin_bit_cast(u32, s));
}
// the images of bin o of the two histograms
__device__ __forceinline__ u32 bin_image(u32 o, bool pen, float rp) {
    const float v = h2f(unordered_key16(o));
    return image_of(pen ? penalise(v, rp) : v);
}

// what every pass knows of the tokens
struct Toks {
    const uint16_t *logits;
    u32 V;
    const int *ban, *pos_io;
    float rp;  // 1: nobody is penalised
    const u32 *seen, *suppress;
};
// (gq_sample_full_adj) the same with the adjustment behind it: the kernels that read tokens are built twice, and the instances of
// gq_sample_full take the argument list they had
struct ToksAdj : Toks {
    SampleAdj adj;
};
template <bool ADJ>
using ToksOf = std::conditional_t<ADJ, ToksAdj, Toks>;
struct Slice {
    u32 lo, hi;
    int bid[4] = {-1, -1, -1, -1};
};
__device__ __forceinline__ Slice slice_of(const Toks &t) {
    Slice s;
    const u32 per = (t.V + FB - 1) / FB;
    s.lo = min(blockIdx.x * per, t.V);
    s.hi = min(s.lo + per, t.V);
    ban_ids(t.ban, t.pos_io, s.bid);
    return s;
}
// token gi of the slice: live or not, its raw pattern, whether the penalty applies, its value s -- and (ToksAdj) the adjusted pattern ha
// that stands in for the logit everywhere but in the raw log-probabilities: liveness, the histogram bin and s are taken from it
template <bool ADJ>
struct TokOf {
    bool live, pen;
    uint16_t h;
    float s;
};
template <>
struct TokOf<true> {
    bool live, pen;
    uint16_t h;
    float s;
    uint16_t ha;
};
template <bool ADJ>
__device__ __forceinline__ uint16_t binned(const TokOf<ADJ> k) {
    if constexpr (ADJ) return k.ha;
    else return k.h;
}
// (the adjusted pattern of token gi alone: full_finish asks for the drawn token's)
__device__ __forceinline__ uint16_t adjusted(const Toks &, u32, uint16_t h) { return h; }
__device__ __forceinline__ uint16_t adjusted(const ToksAdj &t, u32 gi, uint16_t h) {
    const u32 bit = 1u << (gi & 31u);
    return adjust_token(h, gi, t.adj.bias_set && (t.adj.bias_set[gi >> 5] & bit), t.adj.out_set && (t.adj.out_set[gi >> 5] & bit), t.adj);
}
template <typename TK>
__device__ __forceinline__ auto tok_of(const TK &t, const Slice &sl, u32 gi) {
    constexpr bool ADJ = std::is_same_v<TK, ToksAdj>;
    TokOf<ADJ> k{false, false, (uint16_t)0xFC00u, NINF};
    if constexpr (ADJ) k.ha = (uint16_t)0xFC00u;
    if (gi >= sl.hi) return k;
    k.h = t.logits[gi];
    const u32 bit = 1u << (gi & 31u);
    const bool sup = t.suppress && (t.suppress[gi >> 5] & bit);
    uint16_t hv = k.h;
    if constexpr (ADJ) hv = k.ha = adjusted(t, gi, k.h);
    k.live = !is_banned(gi, sl.bid) && !sup && !is_nan16(hv);
    k.pen = t.rp != 1.0f && t.seen && (t.seen[gi >> 5] & bit);
    const float v = h2f(hv);
    k.s = k.pen ? penalise(v, t.rp) : v;
    return k;
}

__global__ void __launch_bounds__(FT) full_zero(uint4 *hist, u32 n16, u32 *maxkey) {
    for (u32 i = blockIdx.x * FT + threadIdx.x; i < n16; i += FB * FT) hist[i] = make_uint4(0u, 0u, 0u, 0u);
    if (blockIdx.x == 0 && threadIdx.x == 0) maxkey[0] = 0u;
}

template <bool ADJ>
__global__ void __launch_bounds__(FT) full_hist(ToksOf<ADJ> t, u32 *hist, u32 *maxkey, float *lp_part) {
    __shared__ float red[FT / 64];
    if constexpr (ADJ) t.suppress = fsm_suppress(t.adj.fsm, t.suppress);  // (_fsm) the forbidden set of the machine's state stands in for the set
    const Slice sl = slice_of(t);
    const u32 tid = threadIdx.x;
    float raw[EPT];
    u32 top = 0u;
#pragma unroll
    for (int e = 0; e < EPT; e++) {
        const auto k = tok_of(t, sl, sl.lo + tid * EPT + e);
        raw[e] = h2f(k.h);  // (-inf past the end; the RAW pattern, adjusted or not)
        if (k.live) {
            atomicAdd(hist + (k.pen ? NBIN : 0u) + ordered_key16(binned(k)), 1u);
            top = max(top, image_of(k.s));
        }
    }
    // the image of the first token of the order: one integer atomic per wave (0: no live token)
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) top = max(top, (u32)__shfl_xor(top, sh, 64));
    if ((tid & 63u) == 0 && top) atomicMax(maxkey, top);
    if (lp_part) {  // (m_b, sum exp(v - m_b)) over the RAW logits of the slice, gq_sample_topk_lp's partials: fmaxf drops a NaN, the sum keeps it
        float mt = raw[0];
#pragma unroll
        for (int e = 1; e < EPT; e++) mt = fmaxf(mt, raw[e]);
        mt = gqw::wave_reduce_bcast<true>(fmaxf(mt, -3.0e38f));
        if ((tid & 63u) == 0) red[tid >> 6] = mt;
        __syncthreads();
        float mb = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        if (mb <= -3.0e38f) mb = NINF;  // (a slice of -inf only, or past the end)
        float zt = 0.f;
#pragma unroll
        for (int e = 0; e < EPT; e++) zt += raw[e] == NINF ? 0.f : expf(raw[e] - mb);
        zt = gqw::wave_reduce_bcast<false>(zt);
        __syncthreads();
        if ((tid & 63u) == 0) red[tid >> 6] = zt;
        __syncthreads();
        if (tid == 0) {
            lp_part[blockIdx.x] = mb;
            lp_part[FB + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
        }
    }
}

// ---- full_scan ----
struct ScanArgs {
    int top_k;
    float top_p, min_p, T, rp;
    int rep;  // histogram N is in use
};
struct Look {  // tokens of histogram h in the bins >= o: spc[h][o % 64][o / 64] (inside the 64 bins of one thread of the scan) + tc[h][o / 64]; spm, tm: their mass
    const u32 *spc;
    const u64 *spm;
    const u32 *tc;
    const u64 *tm;
    float rp;
    int rep;
};
// the lowest bin of histogram `pen` whose image is >= K (OHI + 1: none)
__device__ __forceinline__ u32 bin_at(u32 K, bool pen, float rp) {
    u32 lo = OLO, hi = OHI + 1u;
#pragma unroll 1
    for (int i = 0; i < 16; i++) {
        const u32 mid = (lo + hi) >> 1;
        if (lo < hi) {
            if (bin_image(mid, pen, rp) >= K) hi = mid;
            else lo = mid + 1u;
        }
    }
    return lo;
}
__device__ __forceinline__ void at_or_above(const Look &L, u32 K, u32 &c, u64 &m) {
    const u32 ip = bin_at(K, false, 1.0f);
    c = L.spc[(ip & 63u) * 1024u + (ip >> 6)] + L.tc[ip >> 6];
    m = L.spm[(ip & 63u) * 1024u + (ip >> 6)] + L.tm[ip >> 6];
    if (L.rep) {
        const u32 in = bin_at(K, true, L.rp);
        c += L.spc[SPN + (in & 63u) * 1024u + (in >> 6)] + L.tc[1024u + (in >> 6)];
        m += L.spm[SPN + (in & 63u) * 1024u + (in >> 6)] + L.tm[1024u + (in >> 6)];
    }
}
__device__ __forceinline__ u32 count_ge(const Look &L, u32 K) { u32 c; u64 m; at_or_above(L, K, c, m); return c; }
__device__ __forceinline__ u64 mass_ge(const Look &L, u32 K) { u32 c; u64 m; at_or_above(L, K, c, m); return m; }
// w of the value with image K, as the race forms a: a = fl32(value / T), w = exp(a - m), 1 for a == m (the first token, infinite or not)
__device__ __forceinline__ float w_of(u32 K, float T, float m) {
    const float a = __builtin_bit_cast(float, unordered_key32(K)) / T;
    return a == m ? 1.0f : expf(a - m);
}
__device__ __forceinline__ u64 wfix(float w) { return w > 0.f ? (u64)((double)fminf(w, 1.0f) * WONE) : 0ull; }
// the largest K with pred(K), for a pred that holds up to some K and fails above it (and holds at 0): six rounds of 64 lanes
template <typename P>
__device__ __forceinline__ u32 search_max(u32 l, P pred) {
    u32 t = 0u;
#pragma unroll 1
    for (int shift = 26; shift >= -4; shift -= 6) {
        const int sh = shift < 0 ? 0 : shift;
        const u32 cand = t | (l << sh);
        const bool ok = (shift >= 0 || l < 4u) && pred(cand);
        const int c = __popcll(__builtin_amdgcn_ballot_w64(ok));
        t |= (u32)(c > 0 ? c - 1 : 0) << sh;
    }
    return t;
}

__global__ void __launch_bounds__(1024) full_scan(unsigned char *ws, ScanArgs A) {
    __shared__ u32 tc[2][1024];
    __shared__ u64 tm[2][1024];
    __shared__ u32 wc[2][16];
    __shared__ u64 wm[2][16];
    __shared__ u32 tot_c[2];
    __shared__ u64 tot_m[2];
    const u32 *hist = reinterpret_cast<const u32 *>(ws + WS_HIST);
    u32 *spc = reinterpret_cast<u32 *>(ws + WS_SPC);
    u64 *spm = reinterpret_cast<u64 *>(ws + WS_SPM);
    const u32 tid = threadIdx.x, w = tid >> 6, l = tid & 63u;
    const int NH = A.rep ? 2 : 1;
    const float T = fmaxf(A.T, 1e-5f);
    const u32 maxkey = *reinterpret_cast<const u32 *>(ws + WS_MAXKEY);  // (0: no live token)
    const float m = maxkey ? __builtin_bit_cast(float, unordered_key32(maxkey)) / T : 0.f;
    // without a filter nobody looks a bin up: the totals are the report, and every live token is a candidate
    const bool fine = A.top_k != 0 || A.top_p < 1.0f || A.min_p > 0.f;
    // this thread's 64 bins, highest first: the suffix sums INSIDE the thread go to the arrays, its totals to LDS
    for (int h = 0; h < NH; h++) {
        u32 ec = 0u;
        u64 em = 0ull;
        const uint4 *src = reinterpret_cast<const uint4 *>(hist + h * NBIN + tid * 64u);
        // (bin 64 * tid + j at [j][tid]: the lanes of a wave store side by side)
        u32 *dc = spc + h * SPN + tid;
        u64 *dm = spm + h * SPN + tid;
#pragma unroll 1
        for (int g = 3; g >= 0; g--) {
            uint4 c4[4];
#pragma unroll
            for (int q = 0; q < 4; q++) c4[q] = src[g * 4 + q];
#pragma unroll
            for (int q = 3; q >= 0; q--) {
                const u32 cn[4] = {c4[q].x, c4[q].y, c4[q].z, c4[q].w};
#pragma unroll
                for (int e = 3; e >= 0; e--) {
                    const u32 j = (u32)(g * 16 + q * 4 + e);
                    if (cn[e]) {
                        ec += cn[e];
                        em += (u64)cn[e] * wfix(w_of(bin_image(tid * 64u + j, h == 1, A.rp), T, m));
                    }
                    if (fine) {
                        dc[j * 1024u] = ec;
                        dm[j * 1024u] = em;
                    }
                }
            }
        }
        tc[h][tid] = ec;
        tm[h][tid] = em;
    }
    __syncthreads();
    // exclusive suffix over the threads (threads of higher bins first): inside the wave, then over the waves; it replaces the totals
    for (int h = 0; h < NH; h++) {
        const u32 c0 = tc[h][tid];
        const u64 m0 = tm[h][tid];
        u32 c = c0;
        u64 ms = m0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u32 oc = __shfl_down(c, d, 64);
            const u64 om = __shfl_down(ms, d, 64);
            if (l + d < 64u) {
                c += oc;
                ms += om;
            }
        }
        if (l == 0) {
            wc[h][w] = c;
            wm[h][w] = ms;
        }
        __syncthreads();
        u32 ec = c - c0;
        u64 em = ms - m0;
        for (u32 x = w + 1; x < 16u; x++) {
            ec += wc[h][x];
            em += wm[h][x];
        }
        tc[h][tid] = ec;
        tm[h][tid] = em;
        if (tid == 0) {
            tot_c[h] = ec + c0;
            tot_m[h] = em + m0;
        }
    }
    __threadfence();
    __syncthreads();
    if (w != 0) return;
    const Look L{spc, spm, &tc[0][0], &tm[0][0], A.rp, A.rep};
    Report *rep = reinterpret_cast<Report *>(ws);
    Cut *cut = reinterpret_cast<Cut *>(ws + WS_CUT);
    if (!fine) {  // the totals: thread 0's own bins and everything above them
        if (l == 0) {
            u32 live = 0u;
            u64 Z = 0ull;
            for (int h = 0; h < NH; h++) {
                live += tot_c[h];
                Z += tot_m[h];
            }
            const double Zd = (double)Z * (1.0 / WONE);
            *rep = Report{live, live, Zd, Zd};
            *cut = Cut{0u, 0u, 0u, m, Z};  // (every image of a live token is > 0)
        }
        return;
    }
    const u32 live = count_ge(L, 0u);
    if (live == 0u) {
        if (l == 0) {
            *rep = Report{0u, 0u, 0.0, 0.0};
            *cut = Cut{ALL, 0u, 0u, 0.f, 0ull};
        }
        return;
    }
    // top_k: the image Kk of the last survivor and how many of the tokens at it survive
    const u32 n_k = A.top_k == 0 ? live : min((u32)A.top_k, live);
    u32 Kk = 0u, rk = ALL;
    u64 Zk = mass_ge(L, 0u);
    if (A.top_k != 0) {
        Kk = search_max(l, [&](u32 K) { return count_ge(L, K) >= n_k; });
        u32 cgt;
        u64 mgt;
        at_or_above(L, Kk + 1u, cgt, mgt);
        rk = n_k - cgt;
        Zk = mgt + (u64)rk * wfix(w_of(Kk, T, m));
    }
    u32 Kc = Kk, rc = rk;
    // nucleus: rank j stays while the mass in front of it is < Zk - floor((1 - top_p) Zk)   (its tail is then > (1 - top_p) Zk)
    if (A.top_p < 1.0f) {
        const u64 thr = (u64)((double)(1.0f - A.top_p) * (double)Zk);
        u64 Am = Zk - min(thr, Zk);
        if (Am < 1ull) Am = 1ull;  // (the first token always stays)
        const u32 Kp = search_max(l, [&](u32 K) { return mass_ge(L, K) >= Am; });
        u32 cgt, cge;
        u64 mgt, mge;
        at_or_above(L, Kp + 1u, cgt, mgt);
        at_or_above(L, Kp, cge, mge);
        const u32 g = cge - cgt;
        const u64 wp = g ? (mge - mgt) / g : 0ull;
        u32 rp_ = g;
        if (wp) {
            const u64 need = (Am - mgt + wp - 1ull) / wp;  // tokens at Kp with mgt + q * wp < Am
            if (need < (u64)g) rp_ = (u32)need;
        }
        if (Kp > Kc || (Kp == Kc && rp_ < rc)) {
            Kc = Kp;
            rc = rp_;
        }
    }
    // min_p: a token goes when w < min_p -- the lowest image that stays
    if (A.min_p > 0.f) {
        const u32 Kg = search_max(l, [&](u32 K) { return K < maxkey && !(w_of(K, T, m) >= A.min_p); });
        const u32 Km = Kg + 1u;
        if (Km > Kc) {
            Kc = Km;
            rc = ALL;
        }
    }
    u32 cgt, cge;
    u64 mgt, mge;
    at_or_above(L, Kc + 1u, cgt, mgt);
    at_or_above(L, Kc, cge, mge);
    const u32 gc = cge - cgt;
    rc = min(rc, gc);
    const u64 zkept = mgt + (rc ? (u64)rc * ((mge - mgt) / gc) : 0ull);
    if (l == 0) {
        *rep = Report{cgt + rc, n_k, (double)Zk * (1.0 / WONE), (double)zkept * (1.0 / WONE)};
        *cut = Cut{Kc, rc, gc, m, zkept};
    }
}

template <bool ADJ>
__global__ void __launch_bounds__(FT) full_ties(ToksOf<ADJ> t, const unsigned char *ws, u32 *ties) {
    __shared__ u32 red[FT / 64];
    if constexpr (ADJ) t.suppress = fsm_suppress(t.adj.fsm, t.suppress);  // (_fsm) the forbidden set of the machine's state stands in for the set
    const Cut cut = *reinterpret_cast<const Cut *>(ws + WS_CUT);
    const u32 tid = threadIdx.x;
    u32 c = 0u;
    if (cut.rc < cut.gc) {  // (block-uniform) only a cut INSIDE the tokens of one value needs their ranks
        const Slice sl = slice_of(t);
#pragma unroll
        for (int e = 0; e < EPT; e++) {
            const auto k = tok_of(t, sl, sl.lo + tid * EPT + e);
            c += (k.live && image_of(k.s) == cut.Kc) ? 1u : 0u;
        }
    }
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) c += __shfl_xor(c, sh, 64);
    if ((tid & 63u) == 0) red[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) ties[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

template <bool ADJ>
__global__ void __launch_bounds__(FT) full_race(ToksOf<ADJ> t, const unsigned char *ws, const u32 *ties, float temperature, u32 seed, const int *counter,
                                                 float *best_score, int *best_tok) {
    __shared__ u32 wt[FT / 64];
    __shared__ float rs[FT / 64];
    __shared__ int rt[FT / 64];
    if constexpr (ADJ) t.suppress = fsm_suppress(t.adj.fsm, t.suppress);  // (_fsm) the forbidden set of the machine's state stands in for the set
    const Cut cut = *reinterpret_cast<const Cut *>(ws + WS_CUT);
    const Slice sl = slice_of(t);
    const u32 tid = threadIdx.x, w = tid >> 6, l = tid & 63u;
    const float T = fmaxf(temperature, 1e-5f);
    const u32 ctr = (u32)counter[0];
    const bool inside = cut.rc < cut.gc;  // (block-uniform)
    TokOf<ADJ> k[EPT];
    u32 mine = 0u;
#pragma unroll
    for (int e = 0; e < EPT; e++) {
        k[e] = tok_of(t, sl, sl.lo + tid * EPT + e);
        mine += (k[e].live && image_of(k[e].s) == cut.Kc) ? 1u : 0u;
    }
    u32 rank = 0u;  // of this thread's first token at Kc among all tokens at Kc, by id
    if (inside) {
        u32 base = 0u;  // the slices in front of this one: two per lane
        base += l < blockIdx.x ? ties[l] : 0u;
        base += 64u + l < blockIdx.x ? ties[64u + l] : 0u;
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) base += __shfl_xor(base, sh, 64);
        u32 inc = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u32 o = __shfl_up(inc, d, 64);
            if (l >= (u32)d) inc += o;
        }
        if (l == 63u) wt[w] = inc;
        __syncthreads();
        rank = base + inc - mine;
        for (u32 x = 0; x < w; x++) rank += wt[x];
    }
    float score = -3.0e38f;
    int tokc = NO_TOKEN;
#pragma unroll
    for (int e = 0; e < EPT; e++) {
        const u32 gi = sl.lo + tid * EPT + e, img = image_of(k[e].s);
        bool cand = k[e].live && img >= cut.Kc;
        if (k[e].live && img == cut.Kc) {
            cand = rank < cut.rc;
            rank++;
        }
        if (cand) {
            const float sc = race_score(k[e].s, T, race_u(seed, ctr, gi));
            if (tokc == NO_TOKEN || sc > score) {  // (ids ascend: an equal score keeps the lower id; a NaN score never replaces one)
                score = sc;
                tokc = (int)gi;
            }
        }
    }
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) {
        const float os = __shfl_xor(score, sh, 64);
        const int ot = __shfl_xor(tokc, sh, 64);
        if (better(os, ot, score, tokc)) { score = os; tokc = ot; }
    }
    if (l == 0) {
        rs[w] = score;
        rt[w] = tokc;
    }
    __syncthreads();
    if (tid == 0) {
        for (int x = 1; x < FT / 64; x++)
            if (better(rs[x], rt[x], score, tokc)) { score = rs[x]; tokc = rt[x]; }
        best_score[blockIdx.x] = score;
        best_tok[blockIdx.x] = tokc;
    }
}

struct FinishArgs {
    int *counter, *tok_io, *pos_io, *next_tok;
    SampleEx ex;  // (ban and top_p are not read here: Toks and the scan have them)
    u32 *seen_out;
    float *lp_raw, *lp_drawn;
    u32 lp_cap;
    float temperature;
};

template <bool ADJ>
__global__ void __launch_bounds__(1024) full_finish(ToksOf<ADJ> t, const unsigned char *ws, const float *best_score, const int *best_tok, const float *lp_part,
                                                     FinishArgs F) {
    __shared__ int chosen;
    __shared__ float lpM, lpLogZ;
    const u32 tid = threadIdx.x, w = tid >> 6, l = tid & 63u;
    // the slices' partials -> (M, log Z), the numbers topn_merge forms from the same words
    if (w == 1 && F.lp_raw) lse_merge128(lp_part[l], lp_part[64u + l], lp_part[FB + l], lp_part[FB + 64u + l], l, lpM, lpLogZ);
    __syncthreads();
    if (w == 0) {
        float score = best_score[l];
        int tokc = best_tok[l];
        {
            const float os = best_score[64u + l];
            const int ot = best_tok[64u + l];
            if (better(os, ot, score, tokc)) { score = os; tokc = ot; }
        }
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) {
            const float os = __shfl_xor(score, sh, 64);
            const int ot = __shfl_xor(tokc, sh, 64);
            if (better(os, ot, score, tokc)) { score = os; tokc = ot; }
        }
        if (l == 0) {
            const Cut cut = *reinterpret_cast<const Cut *>(ws + WS_CUT);
            const u32 ctr = (u32)F.counter[0];
            const int p = F.pos_io ? F.pos_io[0] : 0;
            float lraw = __builtin_nanf(""), ldrawn = __builtin_nanf("");
            if ((u32)tokc < t.V) {  // (read before the token joins `seen`)
                const float v = h2f(t.logits[tokc]);
                const bool pen = t.rp != 1.0f && t.seen && (t.seen[(u32)tokc >> 5] & (1u << ((u32)tokc & 31u)));
                // (ADJ) the race saw the adjusted pattern; lp_raw below keeps the raw one
                const float va = ADJ ? h2f(adjusted(t, (u32)tokc, t.logits[tokc])) : v;
                const float a = (pen ? penalise(va, t.rp) : va) / fmaxf(F.temperature, 1e-5f);
                if (F.lp_raw) lraw = (v - lpM) - lpLogZ;
                // a_tok - log sum_C exp(a_c) as (a_tok - m) - log(sum_C w): the candidates' mass is the exact integer sum of the scan
                // (a == m: the first token's own value, infinite or not -- the difference is 0, as w_of has w = 1)
                if (F.lp_drawn) ldrawn = (float)((double)(a == cut.m ? 0.f : a - cut.m) - log((double)cut.zkept * (1.0 / WONE)));
            }
            sample_publish(tokc, ctr, F.counter, F.tok_io, F.pos_io, F.next_tok, F.ex, F.seen_out, t.V);
            if constexpr (ADJ) {
                sample_count(tokc, t.V, t.adj);
                sample_fsm_step(tokc, t.V, t.adj.fsm);  // (_fsm) the machine's transition: the next draw's full_hist reads the word
            }
            if ((u32)(p + 1) < F.lp_cap) {
                if (F.lp_raw) F.lp_raw[p + 1] = lraw;
                if (F.lp_drawn) F.lp_drawn[p + 1] = ldrawn;
            }
            chosen = tokc;
        }
    }
    if (F.ex.x_out) {
        __syncthreads();
        sample_embed(chosen, tid, F.ex);
    }
}
}  // namespace

// the checks and the six launches of gq_sample_full (ADJ = false) and of gq_sample_full_adj with something to adjust
namespace {
template <bool ADJ>
int full_launch(const void *logits, uint32_t vocab, int top_k, float top_p, float min_p, float temperature, uint32_t seed,
                int *counter, void *ws, size_t ws_bytes, int *tok_io, int *pos_io, int *next_tok, const int *ban, int *seq_out,
                uint32_t seq_cap, const void *embed_table, void *x_out, uint32_t dim, float *ssq_out, float repetition_penalty,
                uint32_t *seen, const uint32_t *suppress, float *lp_raw, float *lp_drawn, uint32_t lp_cap, const SampleAdj &adj, void *stream) {
    if (!logits || !counter || !ws || !next_tok) return gq_fail(GQ_EINVAL, "gq_sample_full: null pointer argument.");
    if (int rc = sample_vocab_ok(vocab)) return rc;
    if (ws_bytes < WS_BYTES || ((uintptr_t)ws & 15u)) return gq_fail(GQ_EINVAL, "gq_sample_full: the workspace is gq_sample_full_ws_bytes(vocab) bytes, 16-byte aligned.");
    if (top_k < 0) return gq_fail(GQ_EINVAL, "gq_sample_full: top_k must be >= 0 (0 = no top-k filter).");
    if (int rc = sample_top_p_ok(top_p, true)) return rc;
    if (!(min_p >= 0.f && min_p <= 1.f)) return gq_fail(GQ_EINVAL, "min_p must be in [0, 1] (0 = no min_p filter).");
    if (int rc = sample_penalty_ok(repetition_penalty, seen)) return rc;
    SampleEx ex{};
    if (int rc = sample_extras(ex, vocab, top_p, ban, seq_out, seq_cap, embed_table, x_out, dim, ssq_out)) return rc;  // (ex.vocab = vocab)
    hipStream_t s = (hipStream_t)stream;
    unsigned char *w8 = (unsigned char *)ws;
    const bool rep = repetition_penalty != 1.0f;
    ToksOf<ADJ> t{};
    static_cast<Toks &>(t) = Toks{(const uint16_t *)logits, vocab, ban, pos_io, repetition_penalty, seen, suppress};
    if constexpr (ADJ) t.adj = adj;
    u32 *hist = (u32 *)(w8 + WS_HIST), *ties = (u32 *)(w8 + WS_TIES);
    float *best_score = (float *)(w8 + WS_BEST), *lp_part = (float *)(w8 + WS_LP);
    int *best_tok = (int *)(w8 + WS_BEST + 4 * FB);
    u32 *maxkey = (u32 *)(w8 + WS_MAXKEY);
    hipLaunchKernelGGL(full_zero, dim3(FB), dim3(FT), 0, s, (uint4 *)hist, (rep ? 2u : 1u) * NBIN / 4u, maxkey);
    hipLaunchKernelGGL(full_hist<ADJ>, dim3(FB), dim3(FT), 0, s, t, hist, maxkey, lp_raw ? lp_part : nullptr);
    hipLaunchKernelGGL(full_scan, dim3(1), dim3(1024), 0, s, w8, ScanArgs{top_k, top_p, min_p, temperature, repetition_penalty, rep ? 1 : 0});
    hipLaunchKernelGGL(full_ties<ADJ>, dim3(FB), dim3(FT), 0, s, t, (const unsigned char *)w8, ties);
    hipLaunchKernelGGL(full_race<ADJ>, dim3(FB), dim3(FT), 0, s, t, (const unsigned char *)w8, (const u32 *)ties, temperature, seed, (const int *)counter, best_score, best_tok);
    const FinishArgs F{counter, tok_io, pos_io, next_tok, ex, seen, lp_raw, lp_drawn, lp_cap, temperature};
    hipLaunchKernelGGL(full_finish<ADJ>, dim3(1), dim3(1024), 0, s, t, (const unsigned char *)w8, (const float *)best_score, (const int *)best_tok,
                       (const float *)lp_part, F);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}
}  // namespace

extern "C" size_t gq_sample_full_ws_bytes(uint32_t vocab) { return vocab > GQ_SAMPLER_MAX_VOCAB ? 0 : WS_BYTES; }

extern "C" int gq_sample_full(const void *logits, uint32_t vocab, int top_k, float top_p, float min_p, float temperature, uint32_t seed,
                              int *counter, void *ws, size_t ws_bytes, int *tok_io, int *pos_io, int *next_tok, const int *ban, int *seq_out,
                              uint32_t seq_cap, const void *embed_table, void *x_out, uint32_t dim, float *ssq_out, float repetition_penalty,
                              uint32_t *seen, const uint32_t *suppress, float *lp_raw, float *lp_drawn, uint32_t lp_cap, void *stream) {
    return full_launch<false>(logits, vocab, top_k, top_p, min_p, temperature, seed, counter, ws, ws_bytes, tok_io, pos_io, next_tok, ban, seq_out, seq_cap,
                              embed_table, x_out, dim, ssq_out, repetition_penalty, seen, suppress, lp_raw, lp_drawn, lp_cap, SampleAdj{}, stream);
}

extern "C" int gq_sample_full_topn(const void *logits, uint32_t vocab, int top_k, float top_p, float min_p, float temperature, uint32_t seed,
                                   int *counter, void *ws, size_t ws_bytes, int *tok_io, int *pos_io, int *next_tok, const int *ban, int *seq_out,
                                   uint32_t seq_cap, const void *embed_table, void *x_out, uint32_t dim, float *ssq_out, float repetition_penalty,
                                   uint32_t *seen, const uint32_t *suppress, float *lp_raw, float *lp_drawn, uint32_t lp_cap, int top_n, int *top_ids,
                                   float *top_lps, void *topn_ws, void *stream) {
    if (int rc = gq_topn_check(vocab, top_n, top_ids, top_lps, topn_ws, lp_raw && ws ? ws : nullptr)) return rc;
    if (int rc = gq_sample_full(logits, vocab, top_k, top_p, min_p, temperature, seed, counter, ws, ws_bytes, tok_io, pos_io, next_tok, ban, seq_out, seq_cap,
                                embed_table, x_out, dim, ssq_out, repetition_penalty, seen, suppress, lp_raw, lp_drawn, lp_cap, stream))
        return rc;
    // (the partials full_hist left for full_finish: the same words, combined in the same order)
    return gq_topn_launch(logits, vocab, top_n, (const float *)((unsigned char *)ws + WS_LP), pos_io, top_ids, top_lps, lp_cap, topn_ws, stream);
}

// gq_sample_full_adj (fsm == NULL) and gq_sample_full_fsm: one body
static int sample_full_adj_fsm(const void *logits, uint32_t vocab, int top_k, float top_p, float min_p, float temperature, uint32_t seed,
                               int *counter, void *ws, size_t ws_bytes, int *tok_io, int *pos_io, int *next_tok, const int *ban, int *seq_out,
                               uint32_t seq_cap, const void *embed_table, void *x_out, uint32_t dim, float *ssq_out, float repetition_penalty,
                               uint32_t *seen, const uint32_t *suppress, float *lp_raw, float *lp_drawn, uint32_t lp_cap, int top_n, int *top_ids,
                               float *top_lps, void *topn_ws, const GqSampleAdjust *adj, const GqTokenFsm *fsm, void *stream) {
    if (int rc = sample_adjust_ok(adj)) return rc;
    if (int rc = sample_fsm_ok(fsm, vocab)) return rc;
    if (top_n)
        if (int rc = gq_topn_check(vocab, top_n, top_ids, top_lps, topn_ws, lp_raw && ws ? ws : nullptr)) return rc;
    if (!fsm && sample_adjust_neutral(adj)) {  // the entry without the suffix: its launches, its refusals
        if (int rc = gq_sample_full(logits, vocab, top_k, top_p, min_p, temperature, seed, counter, ws, ws_bytes, tok_io, pos_io, next_tok, ban, seq_out, seq_cap,
                                    embed_table, x_out, dim, ssq_out, repetition_penalty, seen, suppress, lp_raw, lp_drawn, lp_cap, stream))
            return rc;
    } else if (int rc = full_launch<true>(logits, vocab, top_k, top_p, min_p, temperature, seed, counter, ws, ws_bytes, tok_io, pos_io, next_tok, ban, seq_out,
                                          seq_cap, embed_table, x_out, dim, ssq_out, repetition_penalty, seen, suppress, lp_raw, lp_drawn, lp_cap,
                                          fsm ? sample_fsm_of(adj, fsm) : sample_adjust_of(adj), stream)) {
        return rc;
    }
    if (!top_n) return GQ_OK;
    return gq_topn_launch(logits, vocab, top_n, (const float *)((unsigned char *)ws + WS_LP), pos_io, top_ids, top_lps, lp_cap, topn_ws, stream);
}

extern "C" int gq_sample_full_adj(const void *logits, uint32_t vocab, int top_k, float top_p, float min_p, float temperature, uint32_t seed,
                                  int *counter, void *ws, size_t ws_bytes, int *tok_io, int *pos_io, int *next_tok, const int *ban, int *seq_out,
                                  uint32_t seq_cap, const void *embed_table, void *x_out, uint32_t dim, float *ssq_out, float repetition_penalty,
                                  uint32_t *seen, const uint32_t *suppress, float *lp_raw, float *lp_drawn, uint32_t lp_cap, int top_n, int *top_ids,
                                  float *top_lps, void *topn_ws, const GqSampleAdjust *adj, void *stream) {
    return sample_full_adj_fsm(logits, vocab, top_k, top_p, min_p, temperature, seed, counter, ws, ws_bytes, tok_io, pos_io, next_tok, ban, seq_out, seq_cap,
                               embed_table, x_out, dim, ssq_out, repetition_penalty, seen, suppress, lp_raw, lp_drawn, lp_cap, top_n, top_ids, top_lps, topn_ws, adj,
                               nullptr, stream);
}

extern "C" int gq_sample_full_fsm(const void *logits, uint32_t vocab, int top_k, float top_p, float min_p, float temperature, uint32_t seed,
                                  int *counter, void *ws, size_t ws_bytes, int *tok_io, int *pos_io, int *next_tok, const int *ban, int *seq_out,
                                  uint32_t seq_cap, const void *embed_table, void *x_out, uint32_t dim, float *ssq_out, float repetition_penalty,
                                  uint32_t *seen, const uint32_t *suppress, float *lp_raw, float *lp_drawn, uint32_t lp_cap, int top_n, int *top_ids,
                                  float *top_lps, void *topn_ws, const GqSampleAdjust *adj, const GqTokenFsm *fsm, void *stream) {
    return sample_full_adj_fsm(logits, vocab, top_k, top_p, min_p, temperature, seed, counter, ws, ws_bytes, tok_io, pos_io, next_tok, ban, seq_out, seq_cap,
                               embed_table, x_out, dim, ssq_out, repetition_penalty, seen, suppress, lp_raw, lp_drawn, lp_cap, top_n, top_ids, top_lps, topn_ws, adj,
                               fsm, stream);
}
