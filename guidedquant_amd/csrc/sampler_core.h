// sampler_core.h -- the arithmetic the fused sampler's three kernel files share, once: sampler.hip (the two-stage top-k sampler), sampler_full.hip
// (the sampler over the whole vocabulary) and topn.hip (the top-n alternatives) compare their results bit for bit -- the same key order, the
// same race, the same penalised value, the same log Z -- so a rounding point or an order of operations lives here and nowhere else.  Device
// helpers first, the host checks the entry points share at the end.  DESIGN.md, "The sampler's shared arithmetic once", has the contracts as
// a table and the proof that the pinned instances of sampler.hip did not move (profiles/sampler_core_cmp_kernels.txt).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gq_internal.h"

namespace gqs {
typedef uint32_t u32;
typedef unsigned long long u64;

constexpr float NINF = -__builtin_inff();
constexpr int NO_TOKEN = 0x7FFFFFFF;  // the token of an empty candidate set: no id of any vocabulary
static_assert(GQ_SSQ_SLOTS == 1024, "sample_embed writes one hand-over slot per thread");

// the counter-based random word: integer mixing only
__device__ __forceinline__ u32 hash32(u32 x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// Order-preserving images: a > b as numbers <=> image(a) > image(b) as unsigned words (-0 below +0), and the way back.  No rounding.
__device__ __forceinline__ u32 ordered_key16(uint16_t h) { return (h & 0x8000u) ? (u32)(uint16_t)~h : ((u32)h | 0x8000u); }
__device__ __forceinline__ uint16_t unordered_key16(u32 o) { return (o & 0x8000u) ? (uint16_t)(o & 0x7FFFu) : (uint16_t)~o; }
// the same image of an fp32 bit pattern (a penalised logit is an fp32 number that in general is no fp16 value)
__device__ __forceinline__ u32 ordered_key32(u32 b) { return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ u32 unordered_key32(u32 o) { return (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o; }
// a NaN logit of either sign is no candidate in any selector: its image would lie above +inf (0x7E00) or below -inf (0xFE00)
__device__ __forceinline__ bool is_nan16(uint16_t h) { return (h & 0x7FFFu) > 0x7C00u; }

// the repetition penalty of a seen token's logit, fp32: one product or one division
// (-0 is not < 0; the division is IEEE's, correctly rounded: the library is built without fast-math)
__device__ __forceinline__ float penalise(float v, float rp) { return v < 0.f ? v * rp : v / rp; }

// The additive adjustment of a MEMBER token's logit (gq_sample_topk_adj / gq_sample_full_adj: a token with a listed bias, or one the
// request has generated c > 0 times), defined to give an fp16 logit again: v = the fp16 logit widened, p = c > 0 ? fl32(fl32(fp * c) + pp) : 0,
// s = fl32(fl32(v + b) - p), h' = fp16(s) -- every operation rounded on its own (no fused multiply-add), the conversion to nearest even with
// subnormals kept, overflow to +-inf, NaN staying NaN.  Everything behind it takes h' for the logit; a non-member is not passed through here
// (its pattern stays as it is, -0 and NaN included).
__device__ __forceinline__ uint16_t adjust16(uint16_t h, float b, u32 c, float fp, float pp) {
    const float v = (float)__builtin_bit_cast(_Float16, h);
    const float p = c > 0u ? __fadd_rn(__fmul_rn(fp, (float)c), pp) : 0.f;
    const float s = __fsub_rn(__fadd_rn(v, b), p);
    return __builtin_bit_cast(uint16_t, (_Float16)s);
}
// The token-level state machine of the entries with the suffix _fsm: GqTokenFsm (include/gq_hip.h) as the device sees it.  state == NULL:
// none.  Row s of `masks` (`stride` words) is the FORBIDDEN set of state s in the layout of `suppress`; row s of the CSR table (edge_tok
// ascending in [row_ptr[s], row_ptr[s + 1])) and default_next[s] give the state behind a drawn token, -1 = none.
struct SampleFsm {
    int *state;
    const u32 *masks;
    u32 stride, n_states;
    const int *row_ptr, *edge_tok, *edge_next, *default_next;
};
// the state word as the kernels take it: a word outside [0, n_states) (the caller's mistake) is read as the last state, so that no row
// outside the tables is addressed
__device__ __forceinline__ u32 fsm_state_of(const SampleFsm &f) { return min((u32)f.state[0], f.n_states - 1u); }
// the `suppress` bitmap of this draw: the mask row of the current state (a wave-uniform load at kernel entry: the previous draw's last
// kernel wrote the word, behind a kernel boundary), or without a machine the caller's set
__device__ __forceinline__ const u32 *fsm_suppress(const SampleFsm &f, const u32 *suppress) {
    return f.state ? f.masks + (size_t)fsm_state_of(f) * f.stride : suppress;
}
// the transition, ONE lane, next to sample_publish: a binary search of the drawn token in the state's row, a hit gives edge_next, a miss
// default_next; an ordinary vector store.  The token of an empty candidate set, or a result of -1, leaves the state as it is.
__device__ __forceinline__ void sample_fsm_step(int tokc, u32 V, const SampleFsm &f) {
    if (!f.state || (u32)tokc >= V) return;
    const u32 s = fsm_state_of(f);
    int lo = f.row_ptr[s], hi = f.row_ptr[s + 1], nx = f.default_next[s];
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1), t = f.edge_tok[mid];
        if (t == tokc) {
            nx = f.edge_next[mid];
            break;
        }
        if (t < tokc) lo = mid + 1;
        else hi = mid;
    }
    if (nx >= 0 && (u32)nx < f.n_states) f.state[0] = nx;
}
// what the entries with the suffix _adj hand to their kernels: GqSampleAdjust (include/gq_hip.h) as the device sees it, and (_fsm) the machine
struct SampleAdj {
    float fp, pp;
    const u32 *bias_set;
    const float *bias;
    u32 *out_set, *out_count;
    SampleFsm fsm;
};
// the adjusted pattern of token gi with raw pattern h: bias[] and out_count[] are read for members only (the words of a non-member are undefined)
__device__ __forceinline__ uint16_t adjust_token(uint16_t h, u32 gi, bool biased, bool counted, const SampleAdj &a) {
    if (!biased && !counted) return h;
    return adjust16(h, biased ? a.bias[gi] : 0.f, counted ? a.out_count[gi] : 0u, a.fp, a.pp);
}
// the state update of a draw, ONE lane, next to sample_publish: the drawn token's count and its bit in out_set (vector atomics; the next
// step's first kernel reads both behind a kernel boundary).  out_count[t] means something for the tokens of out_set only, so a token's
// first draw STORES 1 and a later one adds 1: clearing out_set alone starts a request.  The token of an empty candidate set counts nowhere.
__device__ __forceinline__ void sample_count(int tokc, u32 V, const SampleAdj &a) {
    if (a.out_set && (u32)tokc < V) {
        const u32 bit = 1u << ((u32)tokc & 31u);
        if (atomicOr(a.out_set + ((u32)tokc >> 5), bit) & bit) atomicAdd(a.out_count + (u32)tokc, 1u);
        else a.out_count[(u32)tokc] = 1u;
    }
}

// The exponential race: argmax_i (s_i / T - log q_i), q ~ Exp(1) = -log(u).  u in (0, 1] from 24 bits of a word tied to (seed, step
// counter, TOKEN id) -- not to a slot, so every selector that keeps a token gives it the same number: one exact product by 2^-24
__device__ __forceinline__ float race_u(u32 seed, u32 ctr, u32 id) {
    const u32 r = hash32(seed ^ hash32(ctr * 0x9E3779B9u + id + 1u));
    return ((float)(r >> 8) + 1.0f) * (1.0f / 16777216.0f);
}
// the score: an IEEE division, the two fast logarithms, one subtraction -- in this order
__device__ __forceinline__ float race_score(float s, float T, float u) { return s / T - __logf(-__logf(u)); }
// (score, tok) wins against (other_score, other_tok): the higher score, an equal one towards the lower id; NO_TOKEN never wins and always
// loses, whatever score stands next to it (a NaN score never replaces a token)
__device__ __forceinline__ bool better(float score, int tok, float other_score, int other_tok) {
    return tok != NO_TOKEN && (other_tok == NO_TOKEN || score > other_score || (score == other_score && tok < other_tok));
}

// The ban list (HF's MinNewTokensLengthLogitsProcessor): device words {n (<= 4), until_pos, id0..id3} -> four ids, -1 = none; nothing is
// banned without a list or once *pos_io >= until_pos (wave-uniform scalar loads).  bid comes in as {-1, -1, -1, -1}: without a list it
// is not touched (the initialisation stands at the caller: written in here it moves the plain instances of sample_stage1)
__device__ __forceinline__ void ban_ids(const int *ban, const int *pos_io, int (&bid)[4]) {
    if (ban) {
        int nban = ban[0];
        if (pos_io && pos_io[0] >= ban[1]) nban = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) bid[i] = i < nban ? ban[2 + i] : -1;
    }
}
__device__ __forceinline__ bool is_banned(u32 gi, const int (&bid)[4]) {
    return (int)gi == bid[0] || (int)gi == bid[1] || (int)gi == bid[2] || (int)gi == bid[3];
}

// The 128 per-slice log-sum-exp partials (m_b, z_b = sum exp(v - m_b)) -> M = max m_b and log Z, Z = sum z_b exp(m_b - M), by ONE wave:
// lane l brings b = l (m0, z0) and b = 64 + l (m1, z1); fmaxf butterfly (xor 32 .. 1), the lane's two terms added, sum butterfly, logf
// -- no atomics, a fixed order: every kernel that combines the same words gets the same two numbers.  A partial is left out by its SUM
// being 0 (a slice past the end), not by its maximum being -inf: fmaxf drops a NaN, so a slice whose only logits are NaN has m = -inf
// and z = NaN, and that NaN has to reach the log-probability.  Lane 0 leaves the two numbers in lds_M and lds_logZ.  The caller keeps
// its loads (sample_stage2 asks for the words in front of its first barrier), these two LDS words and the barrier behind them.
__device__ __forceinline__ void lse_merge128(float m0, float m1, float z0, float z1, u32 l, float &lds_M, float &lds_logZ) {
    float M = fmaxf(m0, m1);
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) M = fmaxf(M, __shfl_xor(M, sh, 64));
    float Z = (z0 == 0.f ? 0.f : z0 * expf(m0 - M)) + (z1 == 0.f ? 0.f : z1 * expf(m1 - M));
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) Z += __shfl_xor(Z, sh, 64);
    if (l == 0) {
        lds_M = M;
        lds_logZ = logf(Z);
    }
}

// Extras of the extended entry points; all optional:
//   ban: the ban list above (EOS is suppressed until min_new_tokens are out);
//   seq_out[*pos_io + 1] = the drawn token (the host reads whole chunks of the sequence instead of cloning one word per step);
//   emb_table / x_out / ssq_out: the embedding row of the drawn token -> the hidden-state buffer of the NEXT step (+ its statistics
//        hand-over, gq_embed_lookup_ho) -- the step's graph then starts at layer 0's first GEMV, one launch less per token.
struct SampleEx {
    const int *ban;
    int *seq_out;
    u32 seq_cap;
    const uint16_t *emb_table;
    uint16_t *x_out;
    u32 dim, vocab;
    float *ssq_out;
    float top_p;  // nucleus threshold (gq_sample_topk_p); >= 1 or <= 0: off
};

// what the last kernel does with the token, ONE lane: outputs, token / position feedback, the sequence store -- what the next graph replay reads
// (seen: a token set or NULL -- the drawn token's bit, by a vector atomic from this one lane; the next step's first kernel reads the word
// behind a kernel boundary.  The token of an empty candidate set is no id of the vocabulary and sets nothing.)
__device__ __forceinline__ void sample_publish(int tokc, u32 ctr, int *counter, int *tok_io, int *pos_io, int *next_tok, const SampleEx &ex,
                                               u32 *seen, u32 V) {
    if (seen && (u32)tokc < V) atomicOr(seen + ((u32)tokc >> 5), 1u << ((u32)tokc & 31u));
    next_tok[0] = tokc;
    counter[0] = (int)(ctr + 1u);
    if (tok_io) tok_io[0] = tokc;
    const int p = pos_io ? pos_io[0] : 0;
    if (ex.seq_out && (u32)(p + 1) < ex.seq_cap) ex.seq_out[p + 1] = tokc;
    if (pos_io) pos_io[0] = p + 1;
}
// the next step's hidden state: tok_embeddings[token] (+ the statistics hand-over for layer 0's RMSNorm: a thread's sum of squares in
// element order, fp32); 1024 threads
__device__ __forceinline__ void sample_embed(int chosen, u32 tid, const SampleEx &ex) {
    u32 tk = (u32)chosen;
    if (tk >= ex.vocab) tk = 0;
    float acc = 0.f;
    for (u32 i = tid; i < ex.dim / 8u; i += 1024u) {
        const uint4 v = reinterpret_cast<const uint4 *>(ex.emb_table + (size_t)tk * ex.dim)[i];
        gq_store_wt(reinterpret_cast<uint4 *>(ex.x_out) + i, v);
        const u32 wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float a = (float)__builtin_bit_cast(_Float16, (uint16_t)(wd[k] & 0xFFFFu)), b = (float)__builtin_bit_cast(_Float16, (uint16_t)(wd[k] >> 16));
            acc += a * a;
            acc += b * b;
        }
    }
    if (ex.ssq_out) gq_store_wt(ex.ssq_out + tid, acc);  // (1024 threads = GQ_SSQ_SLOTS)
}

// ---- host: the refusals the entry points share, one message per mistake ----
inline int sample_vocab_ok(uint32_t vocab) {
    if (vocab > GQ_SAMPLER_MAX_VOCAB) return gq_fail(GQ_ENOTSUP, "vocab too large for the fused sampler (<= 262144).");
    return GQ_OK;
}
// (the two-stage entries take any top_p > 0 -- >= 1: off; gq_sample_full, `strict`, nothing above 1)
inline int sample_top_p_ok(float top_p, bool strict) {
    if (!(top_p > 0.f) || (strict && !(top_p <= 1.f))) return gq_fail(GQ_EINVAL, "top_p must be in (0, 1] (1 = no nucleus filter).");
    return GQ_OK;
}
// the extras, checked
inline int sample_extras(SampleEx &ex, uint32_t vocab, float top_p, const int *ban, int *seq_out, uint32_t seq_cap, const void *embed_table, void *x_out,
                         uint32_t dim, float *ssq_out) {
    if (int rc = sample_top_p_ok(top_p, false)) return rc;
    ex.top_p = top_p;
    ex.ban = ban;
    ex.seq_out = seq_out;
    ex.seq_cap = seq_cap;
    if (x_out) {
        if (!embed_table || dim % 8u) return gq_fail(GQ_EINVAL, "x_out needs the embedding table and dim % 8 == 0.");
        ex.emb_table = (const uint16_t *)embed_table;
        ex.x_out = (uint16_t *)x_out;
        ex.dim = dim;
        ex.vocab = vocab;
        ex.ssq_out = ssq_out;
    } else if (ssq_out) {
        return gq_fail(GQ_EINVAL, "ssq_out without x_out.");
    }
    return GQ_OK;
}
inline int sample_penalty_ok(float repetition_penalty, const uint32_t *seen) {
    if (!(repetition_penalty > 0.f) || !(repetition_penalty < INFINITY))
        return gq_fail(GQ_EINVAL, "repetition_penalty must be finite and > 0 (1 = no penalty).");
    if (!seen && repetition_penalty != 1.0f) return gq_fail(GQ_EINVAL, "repetition_penalty != 1 needs the `seen` token set.");
    return GQ_OK;
}
// the refusals of a GqSampleAdjust (NULL: nothing is asked for), in front of every other check of the entries with the suffix _adj
inline int sample_adjust_ok(const GqSampleAdjust *a) {
    if (!a) return GQ_OK;
    if (!(fabsf(a->frequency_penalty) < INFINITY) || !(fabsf(a->presence_penalty) < INFINITY))
        return gq_fail(GQ_EINVAL, "frequency_penalty and presence_penalty must be finite (0 = no penalty).");
    if (!a->bias_set != !a->bias) return gq_fail(GQ_EINVAL, "adjust: bias_set and bias come together or not at all.");
    if (!a->out_set != !a->out_count) return gq_fail(GQ_EINVAL, "adjust: out_set and out_count come together or not at all.");
    if (!a->out_set && (a->frequency_penalty != 0.f || a->presence_penalty != 0.f))
        return gq_fail(GQ_EINVAL, "a frequency_penalty or presence_penalty != 0 needs out_set and out_count.");
    return GQ_OK;
}
// (behind sample_adjust_ok) nothing is biased and nothing is counted: the entry without the suffix serves the call
inline bool sample_adjust_neutral(const GqSampleAdjust *a) { return !a || (!a->bias_set && !a->out_set); }
inline SampleAdj sample_adjust_of(const GqSampleAdjust *a) {
    return SampleAdj{a->frequency_penalty, a->presence_penalty, a->bias_set, a->bias, a->out_set, a->out_count, SampleFsm{}};
}
// the refusals of a GqTokenFsm (NULL: no machine), in front of every other check of the entries with the suffix _fsm.  The tables live on
// the device: their CONTENT is the builder's business (guidedquant_amd/token_fsm.py validates it), here only the struct is checked.
inline int sample_fsm_ok(const GqTokenFsm *f, uint32_t vocab) {
    if (!f) return GQ_OK;
    if (!f->masks || !f->row_ptr || !f->edge_next || !f->default_next || !f->state)
        return gq_fail(GQ_EINVAL, "fsm: masks, row_ptr, edge_next, default_next and state must not be NULL.");
    if (!f->n_states) return gq_fail(GQ_EINVAL, "fsm: n_states must be >= 1.");
    if (f->words_per_state != (vocab + 31u) / 32u) return gq_fail(GQ_EINVAL, "fsm: words_per_state must be ceil(vocab / 32).");
    return GQ_OK;
}
// a machine next to an adjustment (NULL or neutral: nothing is biased and nothing is counted)
inline SampleAdj sample_fsm_of(const GqSampleAdjust *a, const GqTokenFsm *f) {
    SampleAdj s = sample_adjust_neutral(a) ? SampleAdj{} : sample_adjust_of(a);
    s.fsm = SampleFsm{f->state, f->masks, f->words_per_state, f->n_states, f->row_ptr, f->edge_tok, f->edge_next, f->default_next};
    return s;
}
}  // namespace gqs
