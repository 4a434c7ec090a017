// sampler.hip -- the fused sampler of the decode step, gfx950: top-k / nucleus filter / exponential-race draw over the lm_head's fp16
// logits, with the optional repetition penalty, token sets and per-token log-probabilities, and the token set builder.
// The entry points read the step counter / position from DEVICE memory so a captured hipGraph can be replayed for every token.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gq_internal.h"
#include "sampler_core.h"
#include "wave_util.h"

namespace {

using namespace gqs;  // the images, the race, the ban list, the log-sum-exp merge, publishing, the host checks: sampler_core.h
using gqw::h16;
using gqw::h2f;
using gqw::wave_reduce_bcast;

// Top-k sampling exactly as generate.py:53-73 defines the distribution: logits / max(T, 1e-5), keep the top k,
// softmax, then draw with the exponential race  argmax_i p_i / q_i, q ~ Exp(1)   (multinomial_sample_one_no_sync).
// Equivalent form used here: argmax_i (logit_i / T - log q_i) over the k candidates.  The random numbers come from a
// counter-based hash of (seed, step counter in device memory) -- torch's Philox stream is not reproduced (the
// reference's sampling is not reproducible across runs either: no fixed generator on the sampled path).
// Two launches: per-block candidates, then a single-block merge.  Writes the next token AND feeds it back into
// `tok_io` / increments `pos_io` so a captured graph advances by itself.
constexpr int SAMP_BLOCKS = 128, SAMP_K = 64;  // (the kernels are built for 32 and for 64 candidates per block)
constexpr u32 SAMP_MAX_VOCAB = GQ_SAMPLER_MAX_VOCAB;  // SAMP_BLOCKS slices of <= 2048 logits (the wide instance; <= 131072: slices of <= 1024)
static_assert(SAMP_MAX_VOCAB == 2048u * SAMP_BLOCKS, "the wide instance's slice");

// Selection of the K largest by binary search on a UNIQUE integer key (monotone image of the value in the high
// bits, inverted index in the low bits so that ties go to the lowest index): nbits rounds of "count keys >= candidate"
// (registers + one DPP wave reduction + one LDS combine per round) instead of K rounds of block-wide arg-max.
// The bits of a candidate value that the keys carry -- all 32 of a penalised value (REP), else the 16 of the fp16 logit it is -- their
// image, and the value an image stands for
template <bool REP>
__device__ __forceinline__ auto value_bits(float v) {
    if constexpr (REP) return __builtin_bit_cast(u32, v);
    else return __builtin_bit_cast(uint16_t, (h16)v);
}
__device__ __forceinline__ u32 key_image(uint16_t h) {
    return ordered_key16(h);
}
__device__ __forceinline__ u32 key_image(u32 b) {
    return ordered_key32(b);
}
template <bool REP>
__device__ __forceinline__ float key_value(u32 img) {
    if constexpr (REP) return __builtin_bit_cast(float, unordered_key32(img));
    else return h2f(unordered_key16(img));
}

// The K-th largest of the 64 * EPT keys of ONE wave by binary search on the key bits: the count of a round is EPT ballots +
// scalar population counts -- no LDS, no barrier (a block-wide search pays a 1024-thread barrier per bit: 13 us
// for 33 bits).  Two levels of it replace a block-wide search: every wave keeps its own top K (a global top-K key is in
// the top K of its wave), one wave then searches the survivors.
// The low LOWBITS bits of a key are the tie-breaking position: they are searched only when the value bits leave more than
// K keys at the threshold (rare), which halves the rounds.
// (The key widths are template parameters, not arguments: as arguments they would share one function between the instances -- the
// compiler then no longer sees them as constants of that function.)
template <int EPT, typename KeyT, int NBITS, int LOWBITS>
__device__ __forceinline__ KeyT wave_select_threshold(const KeyT (&key)[EPT], int K) {
    KeyT t = 0;
    int ct = 0x7FFFFFFF;  // count of keys >= t
    for (int bit = NBITS - 1; bit >= 0; bit--) {
        if (bit == LOWBITS - 1 && ct == K) break;  // exactly K keys carry a value >= the threshold value: no tie to break
        const KeyT cand = t | ((KeyT)1 << bit);
        int c = 0;
#pragma unroll
        for (int e = 0; e < EPT; e++) c += __popcll(__builtin_amdgcn_ballot_w64(key[e] >= cand));
        if (c >= K) {  // wave-uniform
            t = cand;
            ct = c;
        }
    }
    return t;
}
// writes the keys >= t (and != 0) of the wave to dst[0 .. count) in lane order; returns the count (<= K for a threshold
// from wave_select_threshold: keys are unique)
template <int EPT, typename KeyT>
__device__ __forceinline__ int wave_compact(const KeyT (&key)[EPT], KeyT t, KeyT *dst, int cap, u32 l) {
    int base = 0;
#pragma unroll
    for (int e = 0; e < EPT; e++) {
        const bool p = key[e] >= t && key[e] != 0;
        const u64 b = __builtin_amdgcn_ballot_w64(p);
        const int pos = base + __popcll(b & ((1ull << l) - 1ull));
        if (p && pos < cap) dst[pos] = key[e];
        base += __popcll(b);
    }
    return base;
}

// REP (gq_sample_topk_rep): a token of `suppress` is no candidate, a token of `seen` carries s = v < 0 ? v * rp : v / rp in fp32.  The
// candidate values are then fp32 numbers and the keys carry all 32 bits of them.
struct SampleRep {
    float rp;
    const u32 *seen, *suppress;
};
// LP (gq_sample_topk_lp): the drawn token's log-probabilities next to the draw.  The selection keys are integers and the race is the same
// sequence of fp32 operations, so the draw of an LP instance is that of the instance without it, bit for bit.
//   ws: 2 * SAMP_BLOCKS floats, (m_b) then (z_b = sum exp(v - m_b)) of block b's slice, over the RAW fp16 logits -- banned, suppressed
//       and penalised tokens count with the value the model gave them.  NULL: no raw log-probability is asked for.
struct SampleLp {
    float *ws, *raw, *drawn;
    u32 cap;
    const uint16_t *logits;  // stage 2 reads the drawn token's raw logit
};

// A kernel argument only the instances with ON take: an instance without it keeps the argument list (and the kernarg layout) it
// would have had alone, and reads T{} -- a constant the compiler folds every test of away.
template <bool ON, typename T>
struct Opt {
    Opt(const T &) {}
    __device__ __forceinline__ T get() const { return T{}; }
};
template <typename T>
struct Opt<true, T> {
    T v;
    Opt(const T &x) : v(x) {}
    __device__ __forceinline__ T get() const { return v; }
};

// The two kernels below are ONE text for every instance: <REP, LP> = <false, false> is what gq_sample_topk / _ex / _p launch (and what
// bench.py and a default generate() run), <true, false> serves gq_sample_topk_rep, <., true> gq_sample_topk_lp.  The instructions of the
// <false, false> instances are pinned (tools/cmp_kernels.py against the build before a change, profiles/sampler_unify_cmp_kernels.txt).
// <true, true> with ADJ serves gq_sample_topk_adj (frequency / presence penalty, logit bias: a member token's adjusted fp16 pattern h' --
// gqs::adjust16 -- stands in for its logit at the key site of stage 1, stage 2 counts the drawn token); ADJ = false leaves every other
// instance the instructions it had (profiles/sampler_adjust_cmp_kernels.txt).  The same ADJ instances serve gq_sample_topk_fsm (a token-level
// state machine: SampleAdj carries a SampleFsm; stage 1 takes the mask row of the machine's state for `suppress`, stage 2's publishing lane
// makes the transition -- gqs::fsm_suppress, gqs::sample_fsm_step).
// What moves an instance is not the sharing but the SHAPE of an expression: a conversion inside or outside the arm of a select turns a
// v_cndmask into a branch, or four narrow loads into one wide one.  Where an instance's sequence or its measured time needs another
// shape the text forks at compile time, on PLAIN or LP, under a comment `fork (site)` that names the instruction difference (DESIGN.md,
// "One sampler kernel pair", has the list and the measurements); nothing else is written twice.
template <bool REP> struct Key1 { typedef u64 T; };  // stage-1 key: 32 + LB bits (REP) or 16 + LB
template <> struct Key1<false> { typedef u32 T; };

// stage 1: each of the 128 blocks selects the top KM of its slice (<= 256 * EPT logits, EPT per thread in registers); KM = 32 or 64.
// Two instances of the widths: EPT = 4, LB = 10 (slices of <= 1024: vocab <= 131072) and EPT = 8, LB = 11 (slices of <= 2048: vocab <=
// 262144).  The grid is SAMP_BLOCKS either way -- the callers' work areas are 128 * KM words -- so a wider vocabulary is a longer slice.
// key = (order-preserving image of the value) << LB | (2^LB - 1 - position in the slice): the 16 bits of the fp16 logit, or (REP) the 32
// bits of the penalised one.  The words of the two token sets are read where the logits are: a thread's EPT <= 8 consecutive tokens lie
// in at most two of them (a slice starts at any token, not at a multiple of 32).
template <int KM, int EPT, int LB, bool REP, bool LP, bool ADJ>
__global__ void __launch_bounds__(256) sample_stage1(const uint16_t *logits, u32 V, float *cand_val, int *cand_idx, const int *ban, const int *pos_io,
                                                     Opt<REP || LP, SampleRep> rep_, Opt<LP, float *> lp_ws_, Opt<ADJ, SampleAdj> adj_) {
    typedef typename Key1<REP>::T KeyT;
    constexpr bool PLAIN = !REP && !LP;
    static_assert(!ADJ || (REP && LP), "the adjustment is built on the general form only");
    constexpr int VB = REP ? 32 : 16;  // value bits of a key
    static_assert(256 * EPT == 1 << LB && EPT <= 8 && VB + LB <= 8 * (int)sizeof(KeyT),
                  "a slice is one position per key of the block; a thread's tokens span two set words");
    constexpr u32 LMASK = (1u << LB) - 1u;
    __shared__ KeyT surv[4 * KM];
    __shared__ KeyT fin[KM];
    __shared__ float lpm[4], lpz[4];  // (LP) a wave's maximum and its sum of exp(v - maximum)
    const SampleRep rep = rep_.get();
    float *const lp_ws = lp_ws_.get();
    const SampleAdj adj = adj_.get();
    const u32 *suppress = rep.suppress;
    if constexpr (ADJ) suppress = fsm_suppress(adj.fsm, suppress);  // (_fsm) the forbidden set of the machine's state stands in for the set
    const u32 per = (V + SAMP_BLOCKS - 1) / SAMP_BLOCKS;  // <= 256 * EPT
    const u32 lo = blockIdx.x * per, hi = min(lo + per, V);
    const u32 tid = threadIdx.x, w = tid >> 6, l = tid & 63u;
    int bid[4] = {-1, -1, -1, -1};
    ban_ids(ban, pos_io, bid);
    u64 sbits = 0ull, pbits = 0ull;  // bit e: token lo + tid * EPT + e is seen / suppressed
    const u32 g0 = lo + tid * (u32)EPT;
    if (REP && g0 < hi) {  // (words of tokens < hi <= V only: a set is ceil(V / 32) words)
        const u32 w0 = g0 >> 5, w1 = min(g0 + (u32)EPT - 1u, hi - 1u) >> 5;
        if (rep.seen) sbits = ((u64)rep.seen[w0] | ((u64)(w1 != w0 ? rep.seen[w1] : 0u) << 32)) >> (g0 & 31u);
        if (suppress) pbits = ((u64)suppress[w0] | ((u64)(w1 != w0 ? suppress[w1] : 0u) << 32)) >> (g0 & 31u);
    }
    u64 bbits = 0ull, cbits = 0ull;  // (ADJ) bit e: the token has a listed bias / has been generated: the two ways of being a member
    if (ADJ && g0 < hi) {
        const u32 w0 = g0 >> 5, w1 = min(g0 + (u32)EPT - 1u, hi - 1u) >> 5;
        if (adj.bias_set) bbits = ((u64)adj.bias_set[w0] | ((u64)(w1 != w0 ? adj.bias_set[w1] : 0u) << 32)) >> (g0 & 31u);
        if (adj.out_set) cbits = ((u64)adj.out_set[w0] | ((u64)(w1 != w0 ? adj.out_set[w1] : 0u) << 32)) >> (g0 & 31u);
    }
    KeyT key[EPT];
    float raw[EPT];  // (LP) every logit of the slice, the banned and the suppressed ones too; -inf past the end
#pragma unroll
    for (int e = 0; e < EPT; e++) {
        const u32 li = tid * (u32)EPT + (u32)e, gi = lo + li;
        // put back (id test): gqs::is_banned(gi, bid), written out -- as a call it reorders the compares of every instance, the plain ones too
        const bool banned = (int)gi == bid[0] || (int)gi == bid[1] || (int)gi == bid[2] || (int)gi == bid[3];
        // fork (slice load): LP needs every logit of the slice for its statistics (-inf past the end); the others load their candidates
        // only -- one global_load_ushort under the candidate test
        uint16_t hb = 0;
        if constexpr (LP) raw[e] = h2f(hb = gi < hi ? logits[gi] : (uint16_t)0xFC00u);
        const bool cand = gi < hi && !banned && !((pbits >> e) & 1ull);
        if constexpr (!LP) hb = cand ? logits[gi] : (uint16_t)0x7E00u;  // (the NaN pattern: no candidate)
        // key = (order-preserving image of the value, position): unique, and both parts are recovered from it.  A NaN of either sign is no
        // candidate (key 0, like a banned id): its image would lie above +inf (0x7E00) or below -inf (0xFE00).
        KeyT k = 0;
        if constexpr (REP) {
            if (cand) {
                // (ADJ) a member's adjusted pattern h' stands in for its logit from here on; raw[e] above stays raw
                if constexpr (ADJ) hb = adjust_token(hb, gi, (bbits >> e) & 1ull, (cbits >> e) & 1ull, adj);
                const float v = h2f(hb), sv = ((sbits >> e) & 1ull) ? penalise(v, rep.rp) : v;
                if (sv == sv) k = ((u64)ordered_key32(__builtin_bit_cast(u32, sv)) << LB) | (u64)(LMASK - li);
            }
        } else if constexpr (LP) {
            // fork (key test): two tests and a branch per logit; the NaN pattern of the form without LP folds them into one select
            if (cand && !is_nan16(hb)) k = (ordered_key16(hb) << LB) | (LMASK - li);
        } else {
            k = is_nan16(hb) ? 0u : ((ordered_key16(hb) << LB) | (LMASK - li));
        }
        key[e] = k;
    }
    if (LP && lp_ws) {  // (m_w, sum exp(v - m_w)) of the wave: a finite v has a finite m_w >= v, a -inf one contributes 0
        float mt = raw[0];
#pragma unroll
        for (int e = 1; e < EPT; e++) mt = fmaxf(mt, raw[e]);
        const float mw = wave_reduce_bcast<true>(mt);
        float zt = 0.f;
#pragma unroll
        for (int e = 0; e < EPT; e++) zt += raw[e] == NINF ? 0.f : expf(raw[e] - mw);
        const float zw = wave_reduce_bcast<false>(zt);
        if (l == 0) {
            lpm[w] = mw;
            lpz[w] = zw;
        }
    }
    // fork (zeroing surv): two u32 keys per lane in one 64-bit LDS write; the other forms write one key per lane (a wave's LDS ops are in order)
    if constexpr (PLAIN) {
        if (l < KM / 2) reinterpret_cast<u64 *>(surv + w * KM)[l] = 0ull;
    } else {
        if (l < KM) surv[w * KM + l] = 0;
    }
    const KeyT t = wave_select_threshold<EPT, KeyT, VB + LB, LB>(key, KM);
    wave_compact<EPT, KeyT>(key, t, surv + w * KM, KM, l);
    __syncthreads();
    if (w == 0) {  // top KM of the 4 * KM survivors
        KeyT k2[KM / 16];
#pragma unroll
        for (int e = 0; e < KM / 16; e++) k2[e] = surv[(u32)e * 64u + l];
        const KeyT t2 = wave_select_threshold<KM / 16, KeyT, VB + LB, LB>(k2, KM);
        if (l < KM) fin[l] = 0;
        const int n = wave_compact<KM / 16, KeyT>(k2, t2, fin, KM, l);
        if (l < KM) {
            const KeyT k = fin[l];
            const bool ok = (int)l < n && k != 0;
            const u32 li = LMASK - ((u32)k & LMASK);
            // fork (candidate store): the conversion inside the arm is a branch, in front of the select a v_cndmask (a slice shorter than KM: padded)
            if constexpr (PLAIN) {
                cand_val[blockIdx.x * KM + l] = ok ? key_value<REP>((u32)(k >> LB)) : -3.0e38f;
            } else {
                const float val = key_value<REP>((u32)(k >> LB));
                cand_val[blockIdx.x * KM + l] = ok ? val : -3.0e38f;
            }
            cand_idx[blockIdx.x * KM + l] = ok ? (int)(lo + li) : -1;
        }
        if (LP && lp_ws && l == 0) {  // the four waves in a fixed order; a block wholly past the end leaves (-inf, 0)
            const float mb = fmaxf(fmaxf(lpm[0], lpm[1]), fmaxf(lpm[2], lpm[3]));
            float zb = 0.f;
#pragma unroll
            // (a partial is left out by its SUM being 0, not by its maximum being -inf: fmaxf drops a NaN, so a wave whose only logits
            // are NaN has m = -inf and z = NaN, and that NaN has to reach the log-probability.  z == 0 happens with m = -inf only.)
            for (int i = 0; i < 4; i++) zb += lpz[i] == 0.f ? 0.f : lpz[i] * expf(lpm[i] - mb);
            lp_ws[blockIdx.x] = mb;
            lp_ws[SAMP_BLOCKS + blockIdx.x] = zb;
        }
    }
}

// stage 2: one block, 128 * KM candidates (KM / 8 per thread), select the global top-k, then the exponential-race draw.
// key = (order-preserving image of the candidate value) << IB | (2^IB - 1 - token id): IB = 17 (vocab <= 131072) or 18 (<= 262144);
// everything behind the selection sees token ids only and is the same in both widths.  The publishing lane sets the drawn token's bit in
// `seen`.  (LP) Wave 1, idle while wave 0 selects, combines the 128 partials of stage 1 (two per lane, then the wave in a fixed butterfly:
// no atomics) and leaves (M, log Z) in LDS; wave 0 loads the raw logits of its candidates in front of the nucleus code (the latency
// hides behind it), normalises the kept candidates' a_c = s_c / T behind the race, and lane 0 stores the two numbers at the index
// seq_out uses.
template <int KM, int IB, bool REP, bool LP, bool ADJ>
__global__ void __launch_bounds__(1024) sample_stage2(const float *cand_val, const int *cand_idx, int top_k, float temperature,
                                                      u32 seed, int *counter, int *tok_io, int *pos_io, int *next_tok, SampleEx ex,
                                                      Opt<REP || LP, u32 *> seen_, Opt<REP || LP, u32> V_, Opt<LP, SampleLp> lp_, Opt<ADJ, SampleAdj> adj_) {
    static_assert(!ADJ || (REP && LP), "the adjustment is built on the general form only");
    static_assert(SAMP_BLOCKS == 128, "two partials per lane of wave 1");
    constexpr bool PLAIN = !REP && !LP;
    constexpr int EPT = KM / 8;  // candidates per thread
    constexpr int VB = REP ? 32 : 16;  // value bits of a key (REP = false: the candidates are fp16 values, exact)
    constexpr u32 IMASK = (1u << IB) - 1u;
    __shared__ float selv[KM];
    __shared__ int seli[KM];
    __shared__ u64 surv[16 * KM];
    __shared__ u64 fin[KM];
    __shared__ int slot, chosen;
    __shared__ float lpM, lpLogZ;  // (LP) max m_b and log sum z_b exp(m_b - M)
    u32 *const seen = seen_.get();
    const u32 V = V_.get();
    const SampleLp lp = lp_.get();
    const u32 tid = threadIdx.x, w = tid >> 6, l = tid & 63u;
    float pm0 = NINF, pm1 = NINF, pz0 = 0.f, pz1 = 0.f;  // (LP) loaded here, used behind the first barrier
    if (LP && lp.ws && w == 1) {
        pm0 = lp.ws[l];
        pm1 = lp.ws[64u + l];
        pz0 = lp.ws[SAMP_BLOCKS + l];
        pz1 = lp.ws[SAMP_BLOCKS + 64u + l];
    }
    u64 key[EPT];
#pragma unroll
    for (int e = 0; e < EPT; e++) {
        const u32 c = tid * (u32)EPT + (u32)e;
        const float v = cand_val[c];
        const int id = cand_idx[c];
        const auto bits = value_bits<REP>(v);
        if constexpr (PLAIN) {
            // fork (key build): the image formed inside the arm keeps one global_load_dword per candidate inside a branch; formed in front
            // of the select, the loads of a thread become one global_load_dwordx4
            key[e] = id >= 0 ? (((u64)key_image(bits) << IB) | (u64)(IMASK - (u32)id)) : 0ull;
        } else {
            const u32 img = key_image(bits);
            key[e] = id >= 0 ? (((u64)img << IB) | (u64)(IMASK - (u32)id)) : 0ull;
        }
    }
    const int K = top_k < 1 ? 1 : (top_k > KM ? KM : top_k);
    if (l < KM) surv[w * KM + l] = 0ull;
    const u64 t = wave_select_threshold<EPT, u64, VB + IB, IB>(key, K);
    wave_compact<EPT, u64>(key, t, surv + w * KM, KM, l);
    __syncthreads();
    if (w == 0) {
        u64 k8[KM / 4];
#pragma unroll
        for (int e = 0; e < KM / 4; e++) k8[e] = surv[(u32)e * 64u + l];
        const u64 t2 = wave_select_threshold<KM / 4, u64, VB + IB, IB>(k8, K);
        if (l < KM) fin[l] = 0ull;
        const int n2 = wave_compact<KM / 4, u64>(k8, t2, fin, KM, l);
        if (l == 0) slot = n2;
        if (l < KM) {
            const u64 k = fin[l];
            selv[l] = key_value<REP>((u32)(k >> IB));
            seli[l] = (int)(IMASK - ((u32)k & IMASK));
        }
    } else if (LP && w == 1 && lp.ws) {
        lse_merge128(pm0, pm1, pz0, pz1, l, lpM, lpLogZ);
    }
    __syncthreads();
    if (w == 0) {
        const int n = min(slot, K);
        const float T = fmaxf(temperature, 1e-5f);
        const u32 ctr = (u32)counter[0];
        float score = -3.0e38f;
        int tokc = 0x7FFFFFFF;
        // (LP) the raw logit of this lane's candidate (an id of the vocabulary), asked for here and used behind the race
        const float rawv = (LP && lp.raw && (int)l < n) ? h2f(lp.logits[seli[l]]) : 0.f;
        // nucleus filter on the top-k survivors -- transformers' TopPLogitsWarper behind TopKLogitsWarper behind the temperature
        // (generation/logits_process.py: probabilities of the scaled, top-k-filtered scores, cumulative sum in ASCENDING order, a token
        // goes when the sum up to and including it is <= 1 - top_p, the most probable one always stays).  n <= 64 candidates, one per
        // lane: the cumulative sum of a lane is a loop over the wave (ties ordered by token id, higher id first = the lower key).
        bool keep = (int)l < n;
        if (ex.top_p > 0.f && ex.top_p < 1.f) {
            const float v = (int)l < n ? selv[l] / T : -3.0e38f;
            float mx = v;
#pragma unroll
            for (int sh = 32; sh >= 1; sh >>= 1) mx = fmaxf(mx, __shfl_xor(mx, sh, 64));
            const float e = (int)l < n ? __expf(v - mx) : 0.f;
            float z = e;
#pragma unroll
            for (int sh = 32; sh >= 1; sh >>= 1) z += __shfl_xor(z, sh, 64);
            const float pr = e / z;
            const int myid = (int)l < n ? seli[l] : -1;
            float cum = 0.f;
            int greater = 0;
            for (int j = 0; j < n; j++) {
                const float vj = __shfl(v, j, 64), pj = __shfl(pr, j, 64);
                const int idj = __shfl(myid, j, 64);
                const bool below = vj < v || (vj == v && idj > myid);  // j sorts before this lane in ascending order
                cum += (below || j == (int)l) ? pj : 0.f;
                greater += (vj > v || (vj == v && idj < myid)) ? 1 : 0;
            }
            keep = keep && (greater == 0 || !(cum <= 1.0f - ex.top_p));
        }
        if (keep) {
            score = race_score(selv[l], T, race_u(seed, ctr, (u32)seli[l]));
            tokc = seli[l];
        }
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) {
            const float os = __shfl_xor(score, sh, 64);
            const int ot = __shfl_xor(tokc, sh, 64);
            if (os > score || (os == score && ot < tokc)) { score = os; tokc = ot; }
        }
        // fork (publish): the log-probability locals live in a scope of their own -- declared at this one, dead, they swap two registers in
        // the nucleus loop of the instances without LP
        if constexpr (LP) {  // every lane holds the drawn token now.  An empty candidate set (no id of the vocabulary): both numbers are NaN.
            float lraw = __builtin_nanf(""), ldrawn = __builtin_nanf("");
            if ((u32)tokc < V) {
                const int win = (int)__builtin_ctzll(__builtin_amdgcn_ballot_w64(keep && seli[l] == tokc));  // one lane: token ids are unique
                // v_tok - lse over the whole vocabulary, as (v_tok - M) - log Z: the difference's rounding is in units of the result
                if (lp.raw) lraw = (__shfl(rawv, win, 64) - lpM) - lpLogZ;
                if (lp.drawn) {  // a_tok - log sum_C exp(a_c) over the kept candidates, a_c as the race forms it
                    const float a = keep ? selv[l] / T : NINF;
                    float mx = a;
#pragma unroll
                    for (int sh = 32; sh >= 1; sh >>= 1) mx = fmaxf(mx, __shfl_xor(mx, sh, 64));
                    float z = (keep && a != NINF) ? expf(a - mx) : 0.f;
#pragma unroll
                    for (int sh = 32; sh >= 1; sh >>= 1) z += __shfl_xor(z, sh, 64);
                    ldrawn = (__shfl(a, win, 64) - mx) - logf(z);
                }
            }
            if (l == 0) {
                const int p = pos_io ? pos_io[0] : 0;  // (before sample_publish increments it)
                sample_publish(tokc, ctr, counter, tok_io, pos_io, next_tok, ex, seen, V);
                if constexpr (ADJ) {
                    sample_count(tokc, V, adj_.get());  // (the drawn token's count and its bit in out_set, next to `seen`)
                    sample_fsm_step(tokc, V, adj_.get().fsm);  // (_fsm) the machine's transition: the next draw's stage 1 reads the word
                }
                chosen = tokc;
                if ((u32)(p + 1) < lp.cap) {
                    if (lp.raw) lp.raw[p + 1] = lraw;
                    if (lp.drawn) lp.drawn[p + 1] = ldrawn;
                }
            }
        } else if (l == 0) {
            sample_publish(tokc, ctr, counter, tok_io, pos_io, next_tok, ex, seen, V);
            chosen = tokc;
        }
    }
    if (ex.x_out) {
        __syncthreads();
        sample_embed(chosen, tid, ex);
    }
}

// token set of gq_token_set_build: one block -- the words are cleared (clear != 0), the block meets, then every id in [0, V) sets its
// bit with a vector atomic (duplicates and ids of one word from several threads are then no race)
__global__ void __launch_bounds__(1024) token_set_build_kernel(const int *ids, u32 n, u32 V, u32 *set, int clear) {
    const u32 words = (V + 31u) / 32u;
    if (clear)
        for (u32 i = threadIdx.x; i < words; i += 1024u) set[i] = 0u;
    __syncthreads();
    for (u32 i = threadIdx.x; i < n; i += 1024u) {
        const u32 t = (u32)ids[i];
        if (t < V) atomicOr(set + (t >> 5), 1u << (t & 31u));
    }
}

// the bias table of gq_token_bias_build: one block -- bias_set is cleared, the block meets, then every id in [0, V) sets its bit (a vector
// atomic: ids of one word come from several threads) and stores its value; the ids are distinct, so no two threads store to one word
__global__ void __launch_bounds__(1024) token_bias_build(const int *ids, const float *values, u32 n, u32 V, u32 *bias_set, float *bias) {
    const u32 words = (V + 31u) / 32u;
    for (u32 i = threadIdx.x; i < words; i += 1024u) bias_set[i] = 0u;
    __syncthreads();
    for (u32 i = threadIdx.x; i < n; i += 1024u) {
        const u32 t = (u32)ids[i];
        if (t < V) {
            atomicOr(bias_set + (t >> 5), 1u << (t & 31u));
            bias[t] = values[i];
        }
    }
}

// the mask rows of gq_token_fsm_build: block s builds row s of `masks`, the FORBIDDEN set of state s -- the row is filled by the state's
// default (default_next[s] < 0: every token forbidden, else none), the block meets, every edge of the row then forbids (edge_next < 0) or
// allows its token, the block meets again, and the request's static set and the bits at and past V in the last word are OR-ed on top.  The
// second and third phase use vector atomics only (tokens of one word come from several threads; no thread reads back a word another one
// stored).  An edge token outside [0, V) is ignored.
__global__ void __launch_bounds__(256) token_fsm_build(const int *row_ptr, const int *edge_tok, const int *edge_next, const int *default_next, u32 V,
                                                        const u32 *base, u32 *masks) {
    const u32 words = (V + 31u) / 32u, s = blockIdx.x;
    u32 *row = masks + (size_t)s * words;
    const u32 fill = default_next[s] < 0 ? 0xFFFFFFFFu : 0u;
    for (u32 i = threadIdx.x; i < words; i += 256u) row[i] = fill;
    __syncthreads();
    const int lo = row_ptr[s], hi = row_ptr[s + 1];
    for (int e = lo + (int)threadIdx.x; e < hi; e += 256) {
        const u32 t = (u32)edge_tok[e];
        if (t >= V) continue;
        if (edge_next[e] < 0) atomicOr(row + (t >> 5), 1u << (t & 31u));
        else atomicAnd(row + (t >> 5), ~(1u << (t & 31u)));
    }
    __syncthreads();
    for (u32 i = threadIdx.x; i < words; i += 256u) {
        u32 m = base ? base[i] : 0u;
        if (i == words - 1u && (V & 31u)) m |= 0xFFFFFFFFu << (V & 31u);
        if (m) atomicOr(row + i, m);
    }
}

// (Measured and removed: a ONE-launch greedy draw -- one 1024-thread block keeps the largest key of its 16-byte units of the
// logits -- for temperature 0.  21 us with a load loop, no better than the two launches above with all 16 loads of a thread in flight
// (865.6 / 864.1 against 867.9 / 868.3 tokens/s): one CU takes the 250 KiB of logits slower than 128 blocks + one do.)

// the pair of one form and width (logits per thread, local-position bits, token-id bits): candidates per block by top_k
template <bool REP, bool LP, bool ADJ, int EPT, int LB, int IB, int KM>
void sample_launch_km(const void *logits, uint32_t vocab, int top_k, float temperature, uint32_t seed, int *counter, float *work_val, int *work_idx,
                      int *tok_io, int *pos_io, int *next_tok, const SampleEx &ex, const SampleRep &rep, u32 *seen, const SampleLp &lp, const SampleAdj &adj,
                      hipStream_t s) {
    hipLaunchKernelGGL((sample_stage1<KM, EPT, LB, REP, LP, ADJ>), dim3(SAMP_BLOCKS), dim3(256), 0, s, (const uint16_t *)logits, vocab, work_val, work_idx, ex.ban,
                       pos_io, Opt<REP || LP, SampleRep>(rep), Opt<LP, float *>(lp.ws), Opt<ADJ, SampleAdj>(adj));
    hipLaunchKernelGGL((sample_stage2<KM, IB, REP, LP, ADJ>), dim3(1), dim3(1024), 0, s, work_val, work_idx, top_k, temperature, seed, counter, tok_io, pos_io,
                       next_tok, ex, Opt<REP || LP, u32 *>(seen), Opt<REP || LP, u32>(vocab), Opt<LP, SampleLp>(lp), Opt<ADJ, SampleAdj>(adj));
}
template <bool REP, bool LP, bool ADJ = false>
void sample_launch_form(const void *logits, uint32_t vocab, int top_k, float temperature, uint32_t seed, int *counter, float *work_val, int *work_idx,
                        int *tok_io, int *pos_io, int *next_tok, const SampleEx &ex, const SampleRep &rep, u32 *seen, const SampleLp &lp, hipStream_t s,
                        const SampleAdj &adj = SampleAdj{}) {
    if (vocab <= 131072u) {  // slices of <= 1024 logits, 17-bit token ids
        if (top_k <= 32) sample_launch_km<REP, LP, ADJ, 4, 10, 17, 32>(logits, vocab, top_k, temperature, seed, counter, work_val, work_idx, tok_io, pos_io, next_tok, ex, rep, seen, lp, adj, s);
        else sample_launch_km<REP, LP, ADJ, 4, 10, 17, 64>(logits, vocab, top_k, temperature, seed, counter, work_val, work_idx, tok_io, pos_io, next_tok, ex, rep, seen, lp, adj, s);
    } else {  // slices of <= 2048 logits through the same 128 blocks, 18-bit token ids
        if (top_k <= 32) sample_launch_km<REP, LP, ADJ, 8, 11, 18, 32>(logits, vocab, top_k, temperature, seed, counter, work_val, work_idx, tok_io, pos_io, next_tok, ex, rep, seen, lp, adj, s);
        else sample_launch_km<REP, LP, ADJ, 8, 11, 18, 64>(logits, vocab, top_k, temperature, seed, counter, work_val, work_idx, tok_io, pos_io, next_tok, ex, rep, seen, lp, adj, s);
    }
}
// rep == NULL: the instances of gq_sample_topk / _ex / _p;  lp != NULL (with rep): those of gq_sample_topk_lp;  adj != NULL (with rep and lp, whose
// pointers may all be NULL): those of gq_sample_topk_adj
int sample_launch(const void *logits, uint32_t vocab, int top_k, float temperature, uint32_t seed, int *counter, float *work_val, int *work_idx,
                  int *tok_io, int *pos_io, int *next_tok, const SampleEx &ex, void *stream, const SampleRep *rep = nullptr, u32 *seen = nullptr,
                  const SampleLp *lp = nullptr, const SampleAdj *adj = nullptr) {
    if (!logits || !counter || !work_val || !work_idx || !next_tok) return gq_fail(GQ_EINVAL, "null pointer argument.");
    if (top_k > SAMP_K) return gq_fail(GQ_ENOTSUP, "top_k > 64 is not supported by the fused sampler.");
    if (int rc = sample_vocab_ok(vocab)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const SampleRep r = rep ? *rep : SampleRep{};
    const SampleLp q = lp ? *lp : SampleLp{};
    // (log-probabilities without a penalty and without sets: the fp16 keys -- the same draw, and a request for log-probabilities alone
    // does not pay for a penalty it does not use.  Measured on the 8B geometry: the fp32 keys cost 10.8 us per token, the
    // log-probabilities 0.9 us.)
    const bool plain = r.rp == 1.0f && !r.seen && !r.suppress && !seen;
    if (rep && lp && adj)
        sample_launch_form<true, true, true>(logits, vocab, top_k, temperature, seed, counter, work_val, work_idx, tok_io, pos_io, next_tok, ex, r, seen, q, s, *adj);
    else if (rep && lp && plain)
        sample_launch_form<false, true>(logits, vocab, top_k, temperature, seed, counter, work_val, work_idx, tok_io, pos_io, next_tok, ex, r, seen, q, s);
    else if (rep && lp)
        sample_launch_form<true, true>(logits, vocab, top_k, temperature, seed, counter, work_val, work_idx, tok_io, pos_io, next_tok, ex, r, seen, q, s);
    else if (rep)
        sample_launch_form<true, false>(logits, vocab, top_k, temperature, seed, counter, work_val, work_idx, tok_io, pos_io, next_tok, ex, r, seen, q, s);
    else
        sample_launch_form<false, false>(logits, vocab, top_k, temperature, seed, counter, work_val, work_idx, tok_io, pos_io, next_tok, ex, r, seen, q, s);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}
}  // namespace

extern "C" int gq_sample_topk(const void *logits, uint32_t vocab, int top_k, float temperature, uint32_t seed, int *counter,
                              float *work_val, int *work_idx, int *tok_io, int *pos_io, int *next_tok, void *stream) {
    if (top_k > 32) return gq_fail(GQ_ENOTSUP, "top_k > 32 is not supported by gq_sample_topk (work buffers of 128 * 32: gq_sample_topk_ex takes 64).");
    return sample_launch(logits, vocab, top_k, temperature, seed, counter, work_val, work_idx, tok_io, pos_io, next_tok, SampleEx{}, stream);
}

extern "C" int gq_sample_topk_ex(const void *logits, uint32_t vocab, int top_k, float temperature, uint32_t seed, int *counter,
                                 float *work_val, int *work_idx, int *tok_io, int *pos_io, int *next_tok, const int *ban, int *seq_out,
                                 uint32_t seq_cap, const void *embed_table, void *x_out, uint32_t dim, float *ssq_out, void *stream) {
    return gq_sample_topk_p(logits, vocab, top_k, 1.0f, temperature, seed, counter, work_val, work_idx, tok_io, pos_io, next_tok, ban, seq_out, seq_cap,
                            embed_table, x_out, dim, ssq_out, stream);
}

extern "C" int gq_sample_topk_p(const void *logits, uint32_t vocab, int top_k, float top_p, float temperature, uint32_t seed, int *counter,
                                float *work_val, int *work_idx, int *tok_io, int *pos_io, int *next_tok, const int *ban, int *seq_out,
                                uint32_t seq_cap, const void *embed_table, void *x_out, uint32_t dim, float *ssq_out, void *stream) {
    SampleEx ex{};
    if (int rc = sample_extras(ex, vocab, top_p, ban, seq_out, seq_cap, embed_table, x_out, dim, ssq_out)) return rc;
    return sample_launch(logits, vocab, top_k, temperature, seed, counter, work_val, work_idx, tok_io, pos_io, next_tok, ex, stream);
}

extern "C" int gq_sample_topk_rep(const void *logits, uint32_t vocab, int top_k, float top_p, float temperature, uint32_t seed, int *counter,
                                  float *work_val, int *work_idx, int *tok_io, int *pos_io, int *next_tok, const int *ban, int *seq_out,
                                  uint32_t seq_cap, const void *embed_table, void *x_out, uint32_t dim, float *ssq_out, float repetition_penalty,
                                  uint32_t *seen, const uint32_t *suppress, void *stream) {
    return gq_sample_topk_lp(logits, vocab, top_k, top_p, temperature, seed, counter, work_val, work_idx, tok_io, pos_io, next_tok, ban, seq_out, seq_cap,
                             embed_table, x_out, dim, ssq_out, repetition_penalty, seen, suppress, nullptr, nullptr, nullptr, 0u, stream);
}

extern "C" int gq_sample_topk_lp(const void *logits, uint32_t vocab, int top_k, float top_p, float temperature, uint32_t seed, int *counter,
                                 float *work_val, int *work_idx, int *tok_io, int *pos_io, int *next_tok, const int *ban, int *seq_out,
                                 uint32_t seq_cap, const void *embed_table, void *x_out, uint32_t dim, float *ssq_out, float repetition_penalty,
                                 uint32_t *seen, const uint32_t *suppress, float *lp_ws, float *lp_raw, float *lp_drawn, uint32_t lp_cap,
                                 void *stream) {
    if (int rc = sample_penalty_ok(repetition_penalty, seen)) return rc;
    if (lp_raw && !lp_ws) return gq_fail(GQ_EINVAL, "gq_sample_topk_lp: lp_raw needs the lp_ws workspace (2 * 128 floats).");
    SampleEx ex{};
    if (int rc = sample_extras(ex, vocab, top_p, ban, seq_out, seq_cap, embed_table, x_out, dim, ssq_out)) return rc;
    const SampleRep rep{repetition_penalty, seen, suppress};
    if (!lp_raw && !lp_drawn)  // only the draw: the instances of gq_sample_topk_rep
        return sample_launch(logits, vocab, top_k, temperature, seed, counter, work_val, work_idx, tok_io, pos_io, next_tok, ex, stream, &rep, seen);
    const SampleLp lp{lp_raw ? lp_ws : nullptr, lp_raw, lp_drawn, lp_cap, (const uint16_t *)logits};
    return sample_launch(logits, vocab, top_k, temperature, seed, counter, work_val, work_idx, tok_io, pos_io, next_tok, ex, stream, &rep, seen, &lp);
}

extern "C" int gq_token_set_build(const int *ids, uint32_t n, uint32_t vocab, uint32_t *set, int clear, void *stream) {
    if (!set || (n && !ids) || !vocab) return gq_fail(GQ_EINVAL, "gq_token_set_build: null pointer argument or vocab == 0.");
    if (!n && !clear) return GQ_OK;
    hipLaunchKernelGGL(token_set_build_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, ids, n, vocab, set, clear);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}

extern "C" int gq_token_bias_build(const int *ids, const float *values, uint32_t n, uint32_t vocab, uint32_t *bias_set, float *bias, void *stream) {
    if (!bias_set || !bias || (n && (!ids || !values)) || !vocab) return gq_fail(GQ_EINVAL, "gq_token_bias_build: null pointer argument or vocab == 0.");
    hipLaunchKernelGGL(token_bias_build, dim3(1), dim3(1024), 0, (hipStream_t)stream, ids, values, n, vocab, bias_set, bias);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}

extern "C" int gq_token_fsm_build(const int *row_ptr, const int *edge_tok, const int *edge_next, const int *default_next, uint32_t n_states,
                                  uint32_t vocab, const uint32_t *base_suppress, uint32_t *masks, void *stream) {
    if (!row_ptr || !edge_next || !default_next || !masks || !n_states || !vocab)
        return gq_fail(GQ_EINVAL, "gq_token_fsm_build: null pointer argument, n_states == 0 or vocab == 0.");
    hipLaunchKernelGGL(token_fsm_build, dim3(n_states), dim3(256), 0, (hipStream_t)stream, row_ptr, edge_tok, edge_next, default_next, vocab, base_suppress, masks);
    GQ_HIP_CHECK(hipGetLastError());
    return GQ_OK;
}

// gq_sample_topk_adj (fsm == NULL) and gq_sample_topk_fsm: one body
static int sample_topk_adj_fsm(const void *logits, uint32_t vocab, int top_k, float top_p, float temperature, uint32_t seed, int *counter,
                               float *work_val, int *work_idx, int *tok_io, int *pos_io, int *next_tok, const int *ban, int *seq_out,
                               uint32_t seq_cap, const void *embed_table, void *x_out, uint32_t dim, float *ssq_out, float repetition_penalty,
                               uint32_t *seen, const uint32_t *suppress, float *lp_ws, float *lp_raw, float *lp_drawn, uint32_t lp_cap, int top_n,
                               int *top_ids, float *top_lps, void *topn_ws, const GqSampleAdjust *adj, const GqTokenFsm *fsm, void *stream) {
    if (int rc = sample_adjust_ok(adj)) return rc;
    if (int rc = sample_fsm_ok(fsm, vocab)) return rc;
    if (!fsm && sample_adjust_neutral(adj)) {  // the entry without the suffix: its launches, its refusals
        if (top_n)
            return gq_sample_topk_lp_topn(logits, vocab, top_k, top_p, temperature, seed, counter, work_val, work_idx, tok_io, pos_io, next_tok, ban, seq_out,
                                          seq_cap, embed_table, x_out, dim, ssq_out, repetition_penalty, seen, suppress, lp_ws, lp_raw, lp_drawn, lp_cap, top_n,
                                          top_ids, top_lps, topn_ws, stream);
        return gq_sample_topk_lp(logits, vocab, top_k, top_p, temperature, seed, counter, work_val, work_idx, tok_io, pos_io, next_tok, ban, seq_out, seq_cap,
                                 embed_table, x_out, dim, ssq_out, repetition_penalty, seen, suppress, lp_ws, lp_raw, lp_drawn, lp_cap, stream);
    }
    if (top_n)
        if (int rc = gq_topn_check(vocab, top_n, top_ids, top_lps, topn_ws, lp_raw && lp_ws ? lp_ws : nullptr)) return rc;
    if (int rc = sample_penalty_ok(repetition_penalty, seen)) return rc;
    if (lp_raw && !lp_ws) return gq_fail(GQ_EINVAL, "gq_sample_topk_lp: lp_raw needs the lp_ws workspace (2 * 128 floats).");
    SampleEx ex{};
    if (int rc = sample_extras(ex, vocab, top_p, ban, seq_out, seq_cap, embed_table, x_out, dim, ssq_out)) return rc;
    const SampleRep rep{repetition_penalty, seen, suppress};
    const SampleLp lp{lp_raw ? lp_ws : nullptr, lp_raw, lp_drawn, lp_cap, (const uint16_t *)logits};
    const SampleAdj a = fsm ? sample_fsm_of(adj, fsm) : sample_adjust_of(adj);
    if (int rc = sample_launch(logits, vocab, top_k, temperature, seed, counter, work_val, work_idx, tok_io, pos_io, next_tok, ex, stream, &rep, seen, &lp, &a))
        return rc;
    if (!top_n) return GQ_OK;
    return gq_topn_launch(logits, vocab, top_n, lp_ws, pos_io, top_ids, top_lps, lp_cap, topn_ws, stream);
}

extern "C" int gq_sample_topk_adj(const void *logits, uint32_t vocab, int top_k, float top_p, float temperature, uint32_t seed, int *counter,
                                  float *work_val, int *work_idx, int *tok_io, int *pos_io, int *next_tok, const int *ban, int *seq_out,
                                  uint32_t seq_cap, const void *embed_table, void *x_out, uint32_t dim, float *ssq_out, float repetition_penalty,
                                  uint32_t *seen, const uint32_t *suppress, float *lp_ws, float *lp_raw, float *lp_drawn, uint32_t lp_cap, int top_n,
                                  int *top_ids, float *top_lps, void *topn_ws, const GqSampleAdjust *adj, void *stream) {
    return sample_topk_adj_fsm(logits, vocab, top_k, top_p, temperature, seed, counter, work_val, work_idx, tok_io, pos_io, next_tok, ban, seq_out, seq_cap,
                               embed_table, x_out, dim, ssq_out, repetition_penalty, seen, suppress, lp_ws, lp_raw, lp_drawn, lp_cap, top_n, top_ids, top_lps,
                               topn_ws, adj, nullptr, stream);
}

extern "C" int gq_sample_topk_fsm(const void *logits, uint32_t vocab, int top_k, float top_p, float temperature, uint32_t seed, int *counter,
                                  float *work_val, int *work_idx, int *tok_io, int *pos_io, int *next_tok, const int *ban, int *seq_out,
                                  uint32_t seq_cap, const void *embed_table, void *x_out, uint32_t dim, float *ssq_out, float repetition_penalty,
                                  uint32_t *seen, const uint32_t *suppress, float *lp_ws, float *lp_raw, float *lp_drawn, uint32_t lp_cap, int top_n,
                                  int *top_ids, float *top_lps, void *topn_ws, const GqSampleAdjust *adj, const GqTokenFsm *fsm, void *stream) {
    return sample_topk_adj_fsm(logits, vocab, top_k, top_p, temperature, seed, counter, work_val, work_idx, tok_io, pos_io, next_tok, ban, seq_out, seq_cap,
                               embed_table, x_out, dim, ssq_out, repetition_penalty, seen, suppress, lp_ws, lp_raw, lp_drawn, lp_cap, top_n, top_ids, top_lps,
                               topn_ws, adj, fsm, stream);
}
