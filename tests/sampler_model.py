"""Host model of the fused sampler (csrc/sampler.hip: sample_stage1 / sample_stage2 behind gq_sample_topk, gq_sample_topk_ex and
gq_sample_topk_p), in numpy and float64.  It restates the CONTRACT -- include/gq_hip.h and the comments above the kernels -- not the
kernels' data flow: no slices, waves, keys or work buffers appear here.

One draw, in order
  ban       device words {n <= 4, until_pos, id[0..3]}: while pos < until_pos the first n ids cannot be drawn
  order     the remaining tokens by (fp16 value descending, index ascending); among equal values -0 sorts BELOW +0 (gq_hip.h)
  top_k     clamped to [1, KM], KM = 32 (top_k <= 32) or 64; fewer than top_k tokens left: all of them.  -inf logits are candidates
            like any other (probability 0: never drawn while a finite one is among the candidates)
  T         max(T, 1e-5) as fp32; a_i = v_i / T
  nucleus   (0 < top_p < 1) p = softmax(a) over the candidates; cumulative sum in ascending order of (a, higher id first among
            equals, +-0 equal); a token goes when the sum up to and including it is <= 1 - top_p (fp32 difference); the first token of
            (a descending, id ascending) always stays
  race      r = hash32(seed ^ hash32(ctr * 0x9E3779B9 + id + 1)) in u32 arithmetic, u = ((r >> 8) + 1) / 2^24 in (0, 1],
            score_i = a_i - log(-log u_i); the largest score wins, equal scores go to the lower id
  state     counter = ctr + 1 (mod 2^32), tok = next_tok = token, seq[pos + 1] = token if pos + 1 < seq_cap, pos = pos + 1

Which draws the device may decide differently: the error model
The device evaluates score_i = fl(fl(v_i / T) - logf(-logf(u_i))) in fp32 (the library is built without fast-math: the division
and the subtraction are correctly rounded, u_i is exact).  Against the float64 score its error is bounded by
      e_i = C0 + c_a * |a_i| + C2 / L_i,        L_i = -log u_i
  c_a * |a_i|  the division (1/2 ulp, granted 2 1/2 for a build with the reciprocal form) and the subtraction's rounding in units of
               |a_i| (1/2 ulp): 3 ulp = 3 * 2^-23 <= C1 = 2^-21.  Two candidates with the SAME fp16 value (and the one T of a draw)
               carry the identical fl(v / T): the division's error cancels between them and only the subtraction's 2^-24 |a_i| stays
               (C1_EQ).  Without that, greedy (T = 1e-5, |a| ~ 1e5: C1 |a| ~ 0.1) could not be decided among equal logits.
  C0           the outer logarithm and the subtraction's rounding in units of |g_i|, g = -log L: logf is 1 ulp of a result of at most
               17 in magnitude where its argument is away from 1, plus an absolute 2^-21 near 1 (below); the subtraction adds
               2^-24 * 17.  Sum < 2^-19.  (|g| > 5 needs L < 0.007, where C2 / L > 7e-5 covers it many times over.)
  C2 / L_i     the inner logarithm near u = 1, where the WINNER's u lies (the largest score has the smallest L): an ABSOLUTE error
               d of logf(u) moves log L by d / L.  C2 = 2^-21: the absolute error the CUDA programming guide gives for __logf on
               [0.5, 2] (2^-21.41), taken as the class of a hardware-logarithm implementation; HIP publishes no table for this
               device.  It is a grant, not a measurement: the GPU test measures the largest float64 margin at which the device and
               this model disagree and asserts it is at most 1/8 of the uncertainty granted for that pair (its docstring has the figure).
A candidate j is ADMISSIBLE next to the winner w when score_w - score_j <= e_w + e_j.  A draw with more than one admissible token
is UNDECIDED.  -inf scores and NaN never are admissible next to a finite winner.

NaN logits: a NaN of either sign is never a candidate -- it ranks with the banned ids, and the finite tokens are drawn exactly as if the
NaN entries were banned.  A step whose unbanned logits are all NaN has an empty candidate set: the token is EMPTY_TOKEN (no id of the
vocabulary), the state advances as for any draw.  NAN_CASES run the profiles nan_few / nan_block / nan_all; NAN_FAULTS are the two
readings a sampler that orders NaN by its bits would give (tests/test_sampler_model_cpu.py shows that the cases catch them).

`fault=` injects one deviation (FAULTS); it is used by tests/test_sampler_model_cpu.py only, to show that the cases below catch it.
"""
from collections import namedtuple

import numpy as np

C0, C1, C1_EQ, C2 = 2.0**-19, 2.0**-21, 2.0**-24, 2.0**-21
BLOCKS = 128
MAX_VOCAB = 262144
FAULTS = ("temp_x1.05", "rng_by_slot", "counter_stuck", "top_k_plus_1", "top_k_minus_1", "tie_to_higher_index", "nucleus_lt",
          "nucleus_descending", "top_unprotected", "ban_le")
NAN_FAULTS = ("nan_wins", "neg_nan_as_number")
EMPTY_TOKEN = 0x7FFFFFFF  # what an empty candidate set publishes (sampler.hip: sample_publish)
M32 = np.uint64(0xFFFFFFFF)


def hash32(x):
    """sampler.hip::hash32 on an array of u32 values held in uint64"""
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & M32
    x ^= x >> np.uint64(16)
    return x


def uniform(seed, ctr, ids):
    """u in (0, 1] of token `ids` at counter `ctr` (arrays broadcast), exact in float64"""
    ctr = np.asarray(ctr, dtype=np.uint64) & M32
    ids = np.asarray(ids, dtype=np.uint64) & M32
    inner = hash32((ctr * np.uint64(0x9E3779B9) + ids + np.uint64(1)) & M32)
    r = hash32((np.uint64(seed & 0xFFFFFFFF) ^ inner) & M32)
    return ((r >> np.uint64(8)) + np.uint64(1)).astype(np.float64) / 16777216.0


def order_key(bits):
    """monotone integer image of fp16 bit patterns: larger value, larger key; -0 (0x8000) directly below +0 (0x0000)"""
    b = np.asarray(bits, dtype=np.uint16).astype(np.int64)
    return np.where(b & 0x8000, 0xFFFF - b, b | 0x8000)


def candidates(logits, top_k, banned=(), fault=None):
    """token ids of the top-k, best first, and the number of candidates the clamp leaves"""
    bits = np.ascontiguousarray(logits, dtype=np.float16).view(np.uint16)
    km = 32 if top_k <= 32 else 64
    assert top_k <= 64, "GQ_ENOTSUP"
    k = min(max(top_k, 1), km)
    if fault == "top_k_plus_1":
        k += 1
    if fault == "top_k_minus_1":
        k = max(k - 1, 1)
    key = order_key(bits)
    idx = np.arange(bits.size, dtype=np.int64)
    nan = (bits & 0x7FFF) > 0x7C00
    if fault == "nan_wins":           # ordered by its bits: +NaN above +inf, -NaN below -inf, both candidates
        live = np.ones(bits.size, dtype=bool)
    elif fault == "neg_nan_as_number":   # told by `bits > 0x7C00` on the pattern: a -NaN stays, below -inf
        live = ~(nan & (bits < 0x8000))
    else:
        live = ~nan
    for b in banned:
        if 0 <= b < bits.size:
            live[b] = False
    idx, key = idx[live], key[live]
    tie = idx if fault != "tie_to_higher_index" else -idx
    sel = np.lexsort((tie, -key))[:k]
    return idx[sel]


def nucleus(a, ids, top_p, fault=None):
    """keep mask over candidates with scaled logits a (float64) and token ids; also the distance of the nearest cumulative sum to
    the threshold (the guard against inputs that the fp32 sums of the device could decide either way)"""
    n = a.size
    if not (0.0 < top_p < 1.0):
        return np.ones(n, dtype=bool), np.inf
    thr = float(np.float32(1.0) - np.float32(top_p))
    with np.errstate(invalid="ignore"):
        e = np.exp(a - a.max())
    p = e / e.sum()
    asc = np.lexsort((-ids, a))  # ascending a; among equals the higher id first
    if fault == "nucleus_descending":
        asc = asc[::-1]
    cum = np.empty(n)
    cum[asc] = np.cumsum(p[asc])
    gone = cum < thr if fault == "nucleus_lt" else np.minimum(cum, 1.0) <= thr
    top = np.lexsort((ids, -a))[0]
    dist = np.abs(np.delete(cum, top) - thr).min() if n > 1 else np.inf
    if fault != "top_unprotected":  # (without the protection a top_p below 2^-24 removes every token: `run` then reports token -1)
        gone[top] = False
    return ~gone, dist


Run = namedtuple("Run", "tokens admissible undecided margin_to counter pos tok seq boundary_dist n_candidates")


def run(logits, n, top_k, T, top_p=1.0, seed=0, counter=0, pos=0, ban=None, seq_cap=0, fault=None):
    """n consecutive draws from one logits vector.  ban = (n_ids, until_pos, ids).  Returns
      tokens       int64 [n]   the model's token per draw
      admissible   list of int64 arrays: every token the device may draw (the model's first); one element when decided
      undecided    bool [n]
      margin_to    function (draw, token) -> (score_winner - score_token, uncertainty granted for the pair); (inf, 0) when the token
                   is no candidate of that draw
      counter, pos, tok, seq   the state after the run (counter as int32, seq as a dict position -> token)"""
    logits = np.ascontiguousarray(logits, dtype=np.float16)
    Tq = float(max(np.float32(T), np.float32(1e-5)))
    if fault == "temp_x1.05":
        Tq *= 1.05
    ctr0 = counter & 0xFFFFFFFF
    steps = np.arange(n, dtype=np.uint64)
    ctrs = (np.uint64(ctr0) + (steps if fault != "counter_stuck" else np.uint64(0) * steps)) & M32
    poss = pos + np.arange(n)
    if ban is not None and ban[0] > 0:
        active = (poss <= ban[1]) if fault == "ban_le" else (poss < ban[1])
        ids_banned = tuple(ban[2][:ban[0]])
    else:
        active, ids_banned = np.zeros(n, dtype=bool), ()
    tokens = np.empty(n, dtype=np.int64)
    undecided = np.zeros(n, dtype=bool)
    admissible = [None] * n
    detail = [None] * n
    bdist, ncand = np.inf, []
    for state in (True, False):
        rows = np.nonzero(active == state)[0]
        if rows.size == 0:
            continue
        ids = candidates(logits, top_k, ids_banned if state else (), fault)
        ncand.append(ids.size)
        isnan = np.isnan(logits[ids].astype(np.float32))
        if ids.size == 0 or isnan.any():   # empty: no token; (faults only) a NaN candidate wins the draw: its score compares false
            t = EMPTY_TOKEN if ids.size == 0 else int(ids[isnan].min())
            for r in rows:
                tokens[r], admissible[r], detail[r] = t, np.array([t]), (ids[:0], np.zeros(0), np.zeros(0))
            continue
        v = logits[ids].astype(np.float64)
        with np.errstate(over="ignore"):
            a = v / Tq
        keep, dist = nucleus(a, ids, top_p, fault)
        bdist = min(bdist, dist)
        if not keep.any():
            for r in rows:
                tokens[r], admissible[r], detail[r] = -1, np.array([-1]), (ids[:0], a[:0], a[:0])
            continue
        slot = np.arange(ids.size)[keep]
        ids, v, a = ids[keep], v[keep], a[keep]
        u = uniform(seed, ctrs[rows][:, None], (slot if fault == "rng_by_slot" else ids)[None, :])
        with np.errstate(divide="ignore", invalid="ignore"):
            L = -np.log(u)
            score = a[None, :] - np.log(L)
            errg = C0 + C2 / L
        # the winner: largest score, lowest id among equals (ids are not sorted: pick by a lexicographic key)
        best = score.max(axis=1)
        isbest = score == best[:, None]
        w = np.where(isbest, ids[None, :], np.iinfo(np.int64).max).argmin(axis=1)
        same = v[None, :] == v[w][:, None]
        absa = np.abs(a)
        with np.errstate(invalid="ignore"):
            ca_j = np.where(same, C1_EQ, C1) * np.where(np.isfinite(absa), absa, 0.0)[None, :]
            ca_w = np.where(same, C1_EQ, C1) * np.where(np.isfinite(absa[w]), absa[w], 0.0)[:, None]
            grant = errg + ca_j + errg[np.arange(rows.size), w][:, None] + ca_w
            margin = best[:, None] - score
            adm = np.isfinite(score) & (margin <= grant)
        adm[np.arange(rows.size), w] = True
        for i, r in enumerate(rows):
            tokens[r] = ids[w[i]]
            others = [j for j in np.nonzero(adm[i])[0] if j != w[i]]
            admissible[r] = np.concatenate([[ids[w[i]]], ids[others]]).astype(np.int64)
            undecided[r] = len(others) > 0
            detail[r] = (ids, margin[i], grant[i])

    def margin_to(draw, token):
        ids_, m_, g_ = detail[draw]
        hit = np.nonzero(ids_ == token)[0]
        if hit.size == 0 or not np.isfinite(m_[hit[0]]):
            return np.inf, 0.0
        return float(m_[hit[0]]), float(g_[hit[0]])

    seq = {int(poss[i]) + 1: int(tokens[i]) for i in range(n) if int(poss[i]) + 1 < seq_cap}
    end = (ctr0 + (n if fault != "counter_stuck" else 0)) & 0xFFFFFFFF
    return Run(tokens, admissible, undecided, margin_to, end - (1 << 32) if end >= 1 << 31 else end, pos + n, int(tokens[-1]), seq,
               bdist, ncand)


# ------------------------------------------------------------------------------------------------ logit profiles (host only)
def _hash_u32(i, salt):
    return hash32((np.asarray(i, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(salt)) & M32)


def profile(name, V, salt=0):
    """fp16 logits of length V.  Integer formulas or numpy's PCG64: the same bits on every machine."""
    rng = np.random.default_rng(1000 + salt + V)
    per = (V + BLOCKS - 1) // BLOCKS
    wave = 256 if V <= 131072 else 512  # consecutive slice positions one wave of stage 1 holds
    if name == "gauss":
        return (rng.standard_normal(V) * 2).astype(np.float16)
    if name == "quant":  # steps of 1/4: ties straddle the k-th place
        return (np.round(rng.standard_normal(V) * 2 * 4) / 4).astype(np.float16)
    if name == "equal":
        return np.full(V, 1.5, dtype=np.float16)
    if name == "negsub":  # negative subnormals and the smallest negative normals
        return (np.uint16(0x8001) + (_hash_u32(np.arange(V), 7 + salt) % np.uint64(0x07FF)).astype(np.uint16)).view(np.float16)
    if name in ("zeros_plus", "zeros_minus"):
        # 20 ones, then zeros of both signs, the rest -1: top_k = 50 cuts inside the zeros.  zeros_plus: more than 30 are +0 (only +0
        # survive, lowest index first); zeros_minus: 10 are +0 (all taken) and the cut falls inside the -0
        x = np.full(V, -1.0, dtype=np.float16)
        place = rng.permutation(V)
        x[place[:20]] = 1.0
        z = place[20:140]
        nplus = 60 if name == "zeros_plus" else 10
        bits = x.view(np.uint16)
        bits[z[:nplus]] = 0x0000
        bits[z[nplus:]] = 0x8000
        return x
    if name in ("top64_one_wave", "top64_one_block", "top64_block_each"):
        x = (rng.standard_normal(V) * 2).astype(np.float16)
        vals = (20.0 + rng.permutation(64) / 16.0).astype(np.float16)
        if name == "top64_one_wave":  # wave 2 of block 5
            where = 5 * per + 2 * wave + 100 + np.arange(64)
            assert per >= 3 * wave
        elif name == "top64_one_block":  # block 5, 16 per wave
            where = 5 * per + (np.arange(64) % 4) * wave + 3 + 11 * (np.arange(64) // 4)
            assert per >= 4 * wave
        else:
            where = np.arange(64) * 2 * per + (np.arange(64) * 37) % per
        assert where.max() < V and np.unique(where).size == 64
        x[where] = vals
        return x
    if name == "ten_finite":
        x = np.full(V, -np.inf, dtype=np.float16)
        x[rng.permutation(V)[:10]] = (rng.standard_normal(10) * 2).astype(np.float16)
        return x
    if name in ("nan_few", "nan_block", "nan_all"):
        x = (rng.standard_normal(V) * 2).astype(np.float16)
        b = x.view(np.uint16)
        if name == "nan_few":      # 5 NaN of both signs and both payload kinds, one of them where the arg-max would be
            where = np.concatenate([[int(np.argmax(x.astype(np.float32)))], rng.permutation(V)[:6]])
            where = where[np.sort(np.unique(where, return_index=True)[1])][:5]
            b[where] = np.array([0x7E00, 0xFE00, 0x7C01, 0xFFFF, 0x7E00], dtype=np.uint16)[:where.size]
        elif name == "nan_block":  # the whole stage-1 slice that holds the arg-max, signs alternating
            blk = int(np.argmax(x.astype(np.float32))) // per
            n = min((blk + 1) * per, V) - blk * per
            b[blk * per:blk * per + n] = np.where(np.arange(n) % 2 == 0, 0x7E00, 0xFE00).astype(np.uint16)
        else:
            b[:] = np.where(np.arange(V) % 3 == 0, 0xFE00, 0x7E00).astype(np.uint16)
        return x
    if name == "planted_high_id":  # the arg-max sits at id V - 5 (>= 131072 on the wide instance)
        x = (rng.standard_normal(V) * 2).astype(np.float16)
        x[V - 5] = 12.0
        return x
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ the committed cases
# entry: "topk" = gq_sample_topk (128 x 32 work buffers, no extras), "ex" = gq_sample_topk_ex, "p" = gq_sample_topk_p.
# ban: (n, until_pos - pos0, ids) with ids possibly "argmax" / "top4" (resolved against the logits).  dim: embedding fold.
Case = namedtuple("Case", "name V prof top_k T top_p seed counter n entry ban pos0 seq_cap dim exact_boundary")


def _case(name, V, prof, top_k, T, top_p=1.0, seed=77, counter=0, n=None, entry=None, ban=None, pos0=0, seq_cap=None, dim=0, exact_boundary=False):
    if n is None:
        n = 8 if T == 0.0 else 1000
    if entry is None:
        entry = "p" if top_p < 1.0 else "ex"
    if seq_cap is None:
        seq_cap = pos0 + n + 2
    return Case(name, V, prof, top_k, T, top_p, seed, counter, n, entry, ban, pos0, seq_cap, dim, exact_boundary)


WRAP31, WRAP32 = 2**31 - 2, 2**32 - 2
CASES = [
    # vocabulary sizes: slices of 0 / 1 / 2 logits, blocks wholly past the end, both instances, a ragged last slice
    _case("v1", 1, "gauss", 50, 1.0, n=16),
    _case("v2", 2, "gauss", 50, 1.0, counter=WRAP31),
    _case("v2_topk", 2, "gauss", 2, 1.0, entry="topk"),
    _case("v127", 127, "gauss", 64, 1.0, seed=0),
    _case("v128", 128, "quant", 33, 0.3, top_p=0.95),
    _case("v129", 129, "gauss", 31, 2.5, entry="topk", counter=WRAP32),
    _case("v129_k_over_v", 129, "equal", 64, 1.0, ban=(4, 10**6, (0, 5, 64, 128)), n=2000),  # 125 live tokens, k = 64
    _case("v40_k_over_v", 40, "quant", 50, 1.0, seed=0xFFFFFFFF),  # top_k larger than V
    _case("v300", 300, "quant", 32, 1.0, entry="topk", seed=0),
    _case("v300_p", 300, "gauss", 50, 1.0, top_p=0.5, counter=4096),
    _case("v4096", 4096, "gauss", 50, 0.3, top_p=0.95, seed=0xFFFFFFFF),
    _case("v4096_k1", 4096, "quant", 1, 1.0, entry="topk", n=64),
    _case("v4096_k2", 4096, "quant", 2, 2.5, entry="topk"),
    _case("v32000", 32000, "gauss", 50, 1.0, n=2000, counter=WRAP31),
    _case("v32000_q33", 32000, "quant", 33, 1.0, seed=0),
    _case("v32000_q31", 32000, "quant", 31, 0.3, entry="topk", counter=WRAP32),
    _case("v32000_q32_p", 32000, "quant", 32, 2.5, top_p=0.5),
    _case("v32000_p005", 32000, "gauss", 64, 2.5, top_p=0.05, counter=4096),
    _case("v131072", 131072, "gauss", 64, 1.0, n=2000, seed=0xFFFFFFFF),
    _case("v131072_q", 131072, "quant", 50, 2.5, top_p=0.95, counter=WRAP32),
    _case("v131073", 131073, "gauss", 64, 1.0, seed=0, counter=WRAP31),
    _case("v131073_q32", 131073, "quant", 32, 1.0, entry="topk"),
    _case("v151936", 151936, "gauss", 50, 0.3, top_p=0.95, n=2000),
    _case("v151936_q", 151936, "quant", 64, 2.5, seed=0xFFFFFFFF, counter=WRAP32),
    _case("v151936_q33_p", 151936, "quant", 33, 1.0, top_p=0.5, seed=0),
    # greedy (T = 0 is a race at T = 1e-5): a unique maximum, ties among equal logits, the wide instance
    _case("greedy_gauss", 32000, "gauss", 50, 0.0),
    _case("greedy_quant", 32000, "quant", 64, 0.0, seed=0),
    _case("greedy_quant_topk", 4096, "quant", 32, 0.0, entry="topk", counter=WRAP31),
    _case("greedy_equal", 300, "equal", 50, 0.0, counter=4096),
    _case("greedy_wide", 151936, "quant", 50, 0.0, top_p=0.95, seed=0xFFFFFFFF),
    _case("greedy_k1", 131073, "gauss", 1, 0.0, entry="topk"),
    # value profiles
    _case("equal", 4096, "equal", 64, 1.0, n=2000),
    _case("equal_p", 32000, "equal", 50, 0.3, top_p=0.95, seed=0),
    _case("equal_k2_p_half", 300, "equal", 2, 1.0, top_p=0.5, n=200, exact_boundary=True),
    _case("negsub", 4096, "negsub", 50, 1.0, counter=WRAP31),
    _case("negsub_cold", 32000, "negsub", 33, 0.3, seed=0),
    _case("zeros_plus", 300, "zeros_plus", 50, 1.0),
    _case("zeros_minus", 4096, "zeros_minus", 50, 1.0, seed=0xFFFFFFFF),
    _case("zeros_minus_p", 4096, "zeros_minus", 50, 2.5, top_p=0.95),
    _case("top64_one_wave", 131072, "top64_one_wave", 64, 2.5),
    _case("top64_one_wave_wide", 262144, "top64_one_wave", 64, 2.5, seed=0),
    _case("top64_one_block", 131072, "top64_one_block", 64, 1.0, top_p=0.95),
    _case("top64_one_block_wide", 262144, "top64_one_block", 50, 2.5),
    _case("top64_block_each", 32000, "top64_block_each", 64, 2.5, counter=4096),
    _case("top64_block_each_wide", 151936, "top64_block_each", 64, 1.0, seed=0xFFFFFFFF),
    _case("ten_finite", 32000, "ten_finite", 50, 1.0),
    _case("ten_finite_p", 151936, "ten_finite", 50, 2.5, top_p=0.95, seed=0),
    _case("top_p_tiny", 32000, "gauss", 50, 1.0, top_p=1e-9, n=200),  # 1 - top_p rounds to 1: only the protected token stays
    # ban list
    _case("ban_argmax", 32000, "gauss", 50, 0.3, ban=(1, 10**6, "argmax")),
    _case("ban_argmax_greedy", 4096, "gauss", 32, 0.0, ban=(1, 10**6, "argmax")),
    _case("ban_top4", 4096, "gauss", 33, 1.0, top_p=0.95, ban=(4, 10**6, "top4"), seed=0),
    _case("ban_expires", 32000, "gauss", 50, 1.0, ban=(4, 500, "top4"), pos0=17, counter=WRAP32),
    _case("ban_zero_ids", 4096, "gauss", 50, 1.0, ban=(0, 10**6, "top4")),
    _case("ban_high_id", 151936, "planted_high_id", 50, 1.0, ban=(1, 400, "argmax")),
    _case("ban_expires_greedy", 4096, "gauss", 50, 0.0, ban=(1, 4, "argmax"), pos0=9),
    _case("seq_cap_short", 4096, "gauss", 50, 1.0, pos0=3, seq_cap=600),
    # embedding fold
    _case("embed_8", 131073, "gauss", 50, 1.0, dim=8, n=500),
    _case("embed_256", 4096, "quant", 64, 2.5, top_p=0.95, dim=256, n=500, seed=0),
    _case("embed_8200", 300, "gauss", 50, 1.0, dim=8200, n=300, counter=WRAP31),
]
# NaN logits (not in CASES: an empty candidate set publishes EMPTY_TOKEN, which the consumers of CASES index the vocabulary with).
# Every entry point, both vocabulary widths, T = 0 and 0.8, top_k 1 / 32 / 50.
NAN_CASES = [
    _case("nan_few_k1_greedy", 4096, "nan_few", 1, 0.0, entry="topk"),
    _case("nan_few_k32", 32000, "nan_few", 32, 0.8, entry="topk", n=300),
    _case("nan_few_k50", 32000, "nan_few", 50, 0.8, n=300),
    _case("nan_few_k50_greedy_wide", 151936, "nan_few", 50, 0.0),
    _case("nan_few_k50_p_wide", 151936, "nan_few", 50, 0.8, top_p=0.9, n=300),
    _case("nan_few_v5", 5, "nan_few", 50, 0.8, n=16),   # every logit NaN: 5 tokens, 5 NaN
    _case("nan_few_ban", 4096, "nan_few", 32, 0.8, ban=(1, 10**6, "argmax"), n=300),
    _case("nan_block_k32", 32000, "nan_block", 32, 0.8, entry="topk", n=300),
    _case("nan_block_k50_greedy", 4096, "nan_block", 50, 0.0),
    _case("nan_block_k50_p", 32000, "nan_block", 50, 0.8, top_p=0.9, n=300),
    _case("nan_block_k1_wide", 262144, "nan_block", 1, 0.8, n=16),
    _case("nan_block_v100", 100, "nan_block", 50, 0.8, n=300),   # slices of one logit: one NaN, 99 candidates
    _case("nan_all_k1", 4096, "nan_all", 1, 0.0, entry="topk"),
    _case("nan_all_k50", 32000, "nan_all", 50, 0.8, n=16),
    _case("nan_all_k32_p_wide", 151936, "nan_all", 32, 0.8, top_p=0.9, n=16),
]
CASE_BY_NAME = {c.name: c for c in CASES + NAN_CASES}
assert len(CASE_BY_NAME) == len(CASES) + len(NAN_CASES)


def case_inputs(c):
    """(logits fp16 [V], ban tuple with absolute until_pos and 4 ids, or None)"""
    x = profile(c.prof, c.V)
    ban = None
    if c.ban is not None:
        nb, until, ids = c.ban
        if ids == "argmax":
            ids = (int(candidates(x, 1)[0]), )
        elif ids == "top4":
            ids = tuple(int(t) for t in candidates(x, 4))
        ids = tuple(ids) + (0, ) * (4 - len(ids))
        ban = (nb, c.pos0 + until, ids)
    return x, ban


def case_run(c, fault=None):
    x, ban = case_inputs(c)
    return run(x, c.n, c.top_k, c.T, c.top_p, c.seed, c.counter, c.pos0, ban, c.seq_cap, fault)


def embed_table(c):
    """fp16 [V][dim]: rows tell tokens apart (first element = id % 2048, exact) and carry values of mixed size"""
    rng = np.random.default_rng(c.dim)
    t = (rng.standard_normal((c.V, c.dim)) * rng.uniform(0.1, 4.0, (c.V, 1))).astype(np.float16)
    t[:, 0] = (np.arange(c.V) % 2048).astype(np.float16)
    return t
