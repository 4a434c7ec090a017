"""Host model of gq_sample_full (csrc/sampler_full.hip), in numpy and float64.  Like tests/sampler_model.py, sampler_rep_model.py and
sampler_lp_model.py, whose pieces it is built from (hash32 / uniform, the penalty, the two log-probabilities' definitions), it restates the
CONTRACT of include/gq_hip.h, not the kernels' data flow: no histograms, images, slices or fixed-point sums appear here.

One draw, in order
  live      every token but a NaN logit of either sign, an id of the ban list while pos < until_pos, a token of `suppress`
  value     s = fp16 logit as fp32; a token of `seen` gets sampler_rep_model.penalised (np.float32 operations: correctly rounded)
  order     (s descending by its fp32 bit pattern image: -0 below +0; id ascending)
  top_k     0: all live tokens; >= 1: the first n_k = min(top_k, live).  No clamp
  scale     T = max(T, 1e-5) as fp32, a = fl32(s / T), m = a of the first token, w = exp(a - m) in float64 (1 for the first token)
  nucleus   (0 < top_p < 1) Z_k = sum of w over the n_k survivors; rank j goes when sum_{i >= j} w_i <= (1 - top_p) * Z_k (fp32 difference);
            rank 0 stays: n_p
  min_p     (0 < min_p <= 1) rank j goes when w_j < min_p; rank 0 stays: n_m
  n         min(n_p, n_m): the candidates are the first n tokens of the order
  race, state   sampler_rep_model's: score = a - log(-log u), u from (seed, counter, id); the drawn token joins `seen`
  lp        lp_raw = v_tok - log sum_t exp(v_t) over all tokens (sampler_lp_model.lse64); lp_drawn = a_tok - log sum_{c < n} exp(a_c)
As in sampler_rep_model a run is TEACHER-FORCED with the tokens a device run drew (`forced`); without them the model follows its own.

Error model
  race      the grants of sampler_model.py (C0, C1, C1_EQ, C2), unchanged.
  top_k     exact: the order is one of integers.
  masses    the device forms d = fl32(a - m) (|error| <= 2^-24 |d|), w' = expf(d) (OCML: 1 ulp, relative 2^-23) and adds floor(w' * 2^44)
            in 64-bit integers (exact sums; every token loses < 2^-44, at most 2^18 tokens: < 2^-26 of Z >= 1).  A token with d < -30.5
            has w < 2^-44 and counts 0: inside the 2^-26.  For the others the relative error of w' is <= 30.5 * 2^-24 + 2^-23 < 2^-18.8,
            so every partial sum of w is within 2^-18.8 + 2^-26 of itself.  The threshold (1 - top_p) * Z_k is one float64 product of the
            fp32 difference and the integer sum, floored: < 2^-44.  Comparing two such sums doubles it: G_MASS = 2^-16 (the contract's
            cap) covers 2 * 2^-18.8 = 2^-17.8.
  min_p     w' >= min_p is decided on expf(fl32(a - m)): the rounding of the difference moves the exponent by <= 2^-24 |a - m|, one ulp
            of expf by 2^-23: G_A(a, m) = 2^-20 * max(1, |a| + |m|) >= 2^-24 (|a| + |m|) + 2^-22, inside the contract's cap of 2^-18 * max(1, |a| + |m|).
            A token with a == m has the exact difference 0 and the exact w = 1 on the device too: it takes no grant.
  n_lo / n_hi: the number of candidates with the nucleus threshold moved by -+ G_MASS * Z_k and the min_p threshold by -+ G_A in a.  A draw
  is UNDECIDED when the race is undecided or when the winner over the first n_lo tokens is not the winner over the first n_hi.

`fault=` injects one deviation (FAULTS), for tests/test_sampler_full_model_cpu.py only.  A penalty applied BEHIND the temperature differs
from the contract by roundings only -- (v / rp) / T against (v / T) / rp -- but the order is one of fp32 bit patterns and the top_k cut
takes no grant: the case `pen_before_scale` plants a seen fp16 logit whose fl32(v / 1.05) IS the fp16 logit of an unseen token with the
lower id (an exact tie: the lower id is first), while fl32(fl32(v / 0.7) / 1.05) lies one ulp above fl32(v' / 0.7); top_k = 1 then draws
the other token.
"""
from collections import namedtuple

import numpy as np

import sampler_lp_model as lpm
import sampler_model as sm
import sampler_rep_model as rm
from sampler_model import C0, C1, C1_EQ, C2, M32, uniform  # noqa: F401

EMPTY_TOKEN = 0x7FFFFFFF
G_MASS = 2.0**-16
FAULTS = ("top_k_plus_1", "top_k_minus_1", "tie_to_higher_id", "nucleus_over_vocab", "min_p_before_nucleus", "min_p_le", "top_unprotected",
          "penalty_after_temperature", "suppressed_counts_to_top_k", "top_k_0_as_1")


def g_a(a, m):
    return 2.0**-20 * np.maximum(1.0, np.abs(a) + abs(m))


State = namedtuple("State", "ids s a w cum n_k n n_lo n_hi Z_k")


def _state(v32, live, pen, rp, top_k, Tq, top_p, min_p, fault, drop_after):
    """the order and the cuts for one (live set, seen set)"""
    ids = np.nonzero(live)[0]
    s = v32[ids].copy()
    p = pen[ids]
    if p.any():
        s[p] = rm.penalised(s[p], rp)
    a_late = None
    if fault == "penalty_after_temperature":  # (the scaled value is penalised: the order is then that of fl32(fl32(v / T) / rp), another rounding)
        with np.errstate(all="ignore"):
            a_late = (v32[ids] / np.float32(Tq)).astype(np.float32)
        if p.any():
            a_late[p] = rm.penalised(a_late[p], rp)
    tie = ids if fault != "tie_to_higher_id" else -ids
    o = np.lexsort((tie, -rm.image32(s if a_late is None else a_late)))
    ids, s = ids[o], s[o]
    if a_late is not None:
        s = a_late[o] * np.float32(Tq)  # (only told apart by equality further down)
        a_late = a_late[o]
    k = top_k
    if fault == "top_k_plus_1" and k:
        k += 1
    if fault == "top_k_minus_1" and k > 1:
        k -= 1
    if fault == "top_k_0_as_1" and k == 0:
        k = 1
    n_k = ids.size if k == 0 else min(k, ids.size)
    s_full = s
    ids, s = ids[:n_k], s[:n_k]
    if a_late is not None:
        a_late = a_late[:n_k]
    if drop_after is not None:  # (fault: the suppressed tokens were selected with the others and leave behind the top-k)
        keep = ~drop_after[ids]
        ids, s = ids[keep], s[keep]
        n_k = ids.size
    if n_k == 0:
        z = np.zeros(0)
        return State(ids, s, z, z, z, 0, 0, 0, 0, 0.0)
    with np.errstate(all="ignore"):
        a = (s / np.float32(Tq)).astype(np.float32).astype(np.float64) if a_late is None else a_late.astype(np.float64)
        m = a[0]
        w = np.where(a == m, 1.0, np.exp(a - m))
    w = np.nan_to_num(w, nan=0.0)
    cum = np.cumsum(w)
    Z_k = float(cum[-1])

    def n_nucleus(shift, over=None):
        if not (0.0 < top_p < 1.0):
            return n_k
        ww = w if over is None else w[:over]
        Z = Z_k if over is None else float(ww.sum())
        if fault == "nucleus_over_vocab":
            with np.errstate(all="ignore"):
                Z = float(np.nan_to_num(np.exp((s_full / np.float32(Tq)).astype(np.float32).astype(np.float64) - m)).sum())
        tail = np.cumsum(ww[::-1])[::-1]
        if fault != "nucleus_over_vocab":
            Z = float(tail[0])  # (the same summation order as the tails: a threshold of 1 * Z is then exactly the whole tail)
        thr = float(np.float32(1.0) - np.float32(top_p)) * Z + shift * Z
        gone = tail <= thr
        if fault != "top_unprotected":
            gone[0] = False
        return int(np.argmax(gone)) if gone.any() else ww.size

    def n_minp(sign):
        if not (0.0 < min_p <= 1.0):
            return n_k
        d = a - m
        lim = np.log(min_p) + sign * g_a(a, m)
        with np.errstate(invalid="ignore"):
            gone = (d <= lim) if fault == "min_p_le" else (d < lim)
        gone = np.where(np.isnan(d), a != m, gone)
        # (a == m: the device's difference is an exact 0 and its w an exact 1 as well -- no grant; it goes under the `<=` fault at min_p = 1 only)
        gone = np.where(a == m, fault == "min_p_le" and min_p >= 1.0, gone)
        gone[0] = False
        return int(np.argmax(gone)) if gone.any() else n_k

    if fault == "min_p_before_nucleus":
        nm = n_minp(0.0)
        n = n_lo = n_hi = min(nm, n_nucleus(0.0, over=nm))
    else:
        n = min(n_nucleus(0.0), n_minp(0.0))
        n_lo = min(n_nucleus(+G_MASS), n_minp(+1.0))
        n_hi = min(n_nucleus(-G_MASS), n_minp(-1.0))
    return State(ids, s, a, w, cum, n_k, n, min(n_lo, n), max(n_hi, n), Z_k)


Run = namedtuple("Run", "tokens admissible undecided margin_to counter pos tok seq seen n n_lo n_hi n_k Z_k Z_kept mass_at lp_raw lp_drawn cut_pinned")


def run(logits, n, top_k, T, top_p=1.0, min_p=0.0, seed=0, counter=0, pos=0, ban=None, seq_cap=0, rp=1.0, seen0=(), suppress=(), forced=None,
        fault=None, n_dev=None):
    """n consecutive draws.  forced: the tokens a device run drew; n_dev: the device's own candidate counts (for lp_drawn of its set).
    Returns sampler_model.Run's fields (tokens, admissible, undecided, margin_to, counter, pos, tok, seq), `seen` (the set after the run) and
    per draw n, n_lo, n_hi, n_k, Z_k, Z_kept (the model's own n), mass_at(draw, count) = the sum of w over the first `count` tokens, lp_raw /
    lp_drawn (dicts slot -> value, for the forced tokens), and cut_pinned (n_lo == n_hi on every draw)."""
    logits = np.ascontiguousarray(logits, dtype=np.float16)
    V = logits.size
    assert V <= sm.MAX_VOCAB and top_k >= 0, "refused"
    Tq = float(max(np.float32(T), np.float32(1e-5)))
    v32 = logits.astype(np.float32)
    dead = np.isnan(v32)
    sup = np.zeros(V, dtype=bool)
    sup[np.asarray([t for t in suppress if 0 <= t < V], dtype=np.int64)] = True
    drop_after = sup if fault == "suppressed_counts_to_top_k" else None
    if drop_after is None:
        dead = dead | sup
    track = np.float32(rp) != np.float32(1.0)
    seen = np.zeros(V, dtype=bool)
    seen_all = np.zeros(V, dtype=bool)
    for t in seen0:
        if 0 <= t < V:
            seen_all[t] = True
            if track:
                seen[t] = True
    nb, until, bids = (ban[0], ban[1], [b for b in ban[2][:ban[0]] if 0 <= b < V]) if ban is not None and ban[0] > 0 else (0, 0, [])
    ctr0 = counter & 0xFFFFFFFF
    full_lse = lpm.lse64(v32) if not np.isnan(v32).any() else float("nan")
    tokens = np.empty(n, dtype=np.int64)
    undecided = np.zeros(n, dtype=bool)
    admissible, detail, states = [None] * n, [None] * n, [None] * n
    out = {k: np.zeros(n, dtype=np.int64) for k in ("n", "n_lo", "n_hi", "n_k")}
    Zk, Zkept = np.zeros(n), np.zeros(n)
    seq, lp_raw, lp_drawn = {}, {}, {}
    memo_key, memo = None, None
    version = 0
    for i in range(n):
        banned = bool(nb and pos + i < until)
        key = (banned, version)
        if key != memo_key:
            live = ~dead
            if banned:
                live = live.copy()
                live[bids] = False
            memo_key, memo = key, _state(v32, live, seen, rp, top_k, Tq, top_p, min_p, fault, drop_after)
        st = memo
        states[i] = st
        out["n"][i], out["n_lo"][i], out["n_hi"][i], out["n_k"][i] = st.n, st.n_lo, st.n_hi, st.n_k
        Zk[i] = st.Z_k
        Zkept[i] = st.cum[st.n - 1] if st.n else 0.0
        ctr = (ctr0 + i) & 0xFFFFFFFF
        tok = EMPTY_TOKEN
        if st.n_hi == 0 or st.n == 0:
            admissible[i], detail[i] = np.array([EMPTY_TOKEN], dtype=np.int64), (st.ids[:0], np.zeros(0), np.zeros(0))
            if st.n_hi:
                undecided[i] = True
        else:
            ids, s, a = st.ids[:st.n_hi], st.s[:st.n_hi], st.a[:st.n_hi]
            u = uniform(seed, np.uint64(ctr), ids)
            with np.errstate(divide="ignore", invalid="ignore"):
                L = -np.log(u)
                score = a - np.log(L)
                errg = C0 + C2 / L
            absa = np.where(np.isfinite(a), np.abs(a), 0.0)

            def winner(cnt):
                sc = score[:cnt]
                best = sc.max()
                return int(np.where(sc == best, ids[:cnt], np.iinfo(np.int64).max).argmin())

            w = winner(st.n)
            w_lo, w_hi = winner(max(st.n_lo, 1)), winner(st.n_hi)
            # admissible: within the race grants of the best score of the smallest candidate count that holds the token
            run_best = np.maximum.accumulate(score)
            ref = np.where(np.arange(st.n_hi) < st.n_lo, run_best[max(st.n_lo, 1) - 1], run_best)
            # (the grant is taken against the model's winner: equal fp32 values carry the identical fl(s / T))
            same = s == s[w]
            with np.errstate(invalid="ignore"):
                grant = errg + np.where(same, C1_EQ, C1) * absa + errg[w] + np.where(same, C1_EQ, C1) * absa[w]
                margin = ref - score
                adm = np.isfinite(score) & (margin <= grant)
                margin_w = score[w] - score
            adm[w] = False
            tok = int(ids[w])
            admissible[i] = np.concatenate([[tok], ids[adm]]).astype(np.int64)
            undecided[i] = bool(adm.any()) or ids[w_lo] != ids[w_hi]
            detail[i] = (ids, margin_w, grant)
        tokens[i] = tok
        drawn = tok if forced is None else int(forced[i])
        slot = pos + i + 1
        if slot < seq_cap:
            seq[slot] = drawn
        # the two log-probabilities of the token that was drawn, over the device's own candidate set where it is given
        cnt = st.n if n_dev is None else int(n_dev[i])
        if drawn == EMPTY_TOKEN or cnt == 0:
            lp_raw[slot] = lp_drawn[slot] = float("nan")
        else:
            lp_raw[slot] = float(v32[drawn]) - full_lse if 0 <= drawn < V else float("nan")
            hit = np.nonzero(st.ids[:cnt] == drawn)[0]
            if hit.size:
                with np.errstate(invalid="ignore"):
                    lp_drawn[slot] = 0.0 if cnt == 1 else float(st.a[hit[0]] - st.a[0] - np.log(st.cum[cnt - 1]))
            else:
                lp_drawn[slot] = float("nan")
        if 0 <= drawn < V:
            seen_all[drawn] = True
            if track and not seen[drawn]:
                seen[drawn] = True
                version += 1

    def margin_to(draw, token):
        ids_, m_, g_ = detail[draw]
        hit = np.nonzero(ids_ == token)[0]
        if hit.size == 0 or not np.isfinite(m_[hit[0]]):
            return np.inf, 0.0
        return float(m_[hit[0]]), float(g_[hit[0]])

    def mass_at(draw, count):
        return float(states[draw].cum[count - 1]) if count else 0.0

    end = (ctr0 + n) & 0xFFFFFFFF
    last = int(tokens[-1]) if forced is None else int(forced[n - 1])
    return Run(tokens, admissible, undecided, margin_to, end - (1 << 32) if end >= 1 << 31 else end, pos + n, last, seq,
               rm.token_set(np.nonzero(seen_all)[0], V), out["n"], out["n_lo"], out["n_hi"], out["n_k"], Zk, Zkept, mass_at, lp_raw, lp_drawn,
               bool((out["n_lo"] == out["n_hi"]).all()))


# ------------------------------------------------------------------------------------------------ logit profiles
def profile(name, V, salt=0):
    """sampler_model's profiles, and `peaky`: a few well separated high logits over a far lower floor -- every cut falls in a wide gap of the
    masses, so n_lo == n_hi; `ninf_tail`: -inf logits from rank 40 on"""
    if name == "peaky":
        rng = np.random.default_rng(3000 + salt + V)
        x = np.full(V, -20.0, dtype=np.float16)
        top = rng.permutation(V)[:min(V, 12)]
        x[top] = (8.0 - 0.75 * np.arange(top.size)).astype(np.float16)
        return x
    if name == "ninf_tail":
        rng = np.random.default_rng(3100 + salt + V)
        x = np.full(V, -np.inf, dtype=np.float16)
        top = rng.permutation(V)[:min(V, 40)]
        x[top] = (rng.standard_normal(top.size) * 2).astype(np.float16)
        return x
    return sm.profile(name, V, salt)


# ------------------------------------------------------------------------------------------------ the committed cases
Case = namedtuple("Case", "name V prof top_k T top_p min_p seed counter n rp seen0 suppress ban pos0 seq_cap dim pinned plant")
WRAP31, WRAP32 = sm.WRAP31, sm.WRAP32


def _case(name, V, prof, top_k, T=1.0, top_p=1.0, min_p=0.0, rp=1.0, seen0=(), suppress=(), seed=77, counter=0, n=None, ban=None, pos0=0, seq_cap=None,
          dim=0, pinned=False, plant=()):
    if n is None:
        n = 8 if T == 0.0 else (40 if (top_k == 0 or top_k > 1000) and V > 32000 else 200)
    if seq_cap is None:
        seq_cap = pos0 + n + 2
    return Case(name, V, prof, top_k, T, top_p, min_p, seed, counter, n, rp, seen0, suppress, ban, pos0, seq_cap, dim, pinned, tuple(plant))


CASES = [
    # vocabularies: slices of 0 / 1 / 8 logits, both slice widths of the shipped sampler, a ragged last slice
    _case("v1", 1, "gauss", 0, n=16),
    _case("v5_k200", 5, "gauss", 200, top_p=0.9, n=64),
    _case("v100_full", 100, "gauss", 0, counter=WRAP31),
    _case("v100_nan_block", 100, "nan_block", 0, T=0.8, min_p=0.05),
    _case("v1000_k65", 1000, "quant", 65, top_p=0.9),
    _case("v1000_minp", 1000, "gauss", 0, min_p=0.05, seed=0),
    _case("v32000_k200", 32000, "gauss", 200),
    _case("v32000_k200_quant_p", 32000, "quant", 200, T=2.5, top_p=0.9, seed=0),
    _case("v32000_full_p", 32000, "gauss", 0, top_p=0.95, n=100),
    _case("v131072_k5000", 131072, "gauss", 5000, n=60, seed=0xFFFFFFFF),
    _case("v131072_quant_p_minp", 131072, "quant", 0, T=0.7, top_p=0.9, min_p=0.02),
    _case("v131073_k200_minp", 131073, "gauss", 200, min_p=0.05, counter=WRAP32),
    _case("v131073_full", 131073, "quant", 0, T=0.3),
    _case("v151936_k200", 151936, "gauss", 200, T=0.8, top_p=0.9, min_p=0.01),
    _case("v151936_full_p", 151936, "gauss", 0, T=0.6, top_p=0.9),
    _case("v151936_k_vocab", 151936, "quant", 151936, T=0.25, n=40),
    _case("v262144_k200_p", 262144, "quant", 200, top_p=0.9, seed=0),
    _case("v262144_full", 262144, "gauss", 0, T=0.3, n=40),
    _case("v262144_k_over", 262144, "gauss", 300000, min_p=0.1, n=20),
    # the cut pinned exactly: n_lo == n_hi on every draw
    _case("peaky_k65", 32000, "peaky", 65, pinned=True),
    _case("peaky_p", 32000, "peaky", 0, top_p=0.9, pinned=True),
    _case("peaky_minp", 151936, "peaky", 0, min_p=0.05, pinned=True),
    _case("peaky_k200_p", 1000, "peaky", 200, top_p=0.7, pinned=True),
    _case("peaky_k200_minp", 131073, "peaky", 200, min_p=0.2, pinned=True),
    _case("peaky_p_minp", 1000, "peaky", 0, top_p=0.95, min_p=0.02, pinned=True),
    _case("peaky_all", 32000, "peaky", 200, T=1.5, top_p=0.9, min_p=0.05, pinned=True),
    _case("equal_k70", 300, "equal", 70, pinned=True),           # ties across the top_k cut: the 70 lowest ids
    _case("equal_k70_p_half", 1000, "equal", 70, top_p=0.5),     # the nucleus cut inside one value: 35 of the 70 (the threshold itself)
    _case("top_p_tiny", 1000, "gauss", 0, top_p=1e-9, pinned=True),  # 1 - top_p rounds to 1: only the protected token stays
    _case("min_p_one", 1000, "quant", 0, min_p=1.0, pinned=True),    # the tokens that tie the maximum stay
    _case("min_p_one_equal", 300, "equal", 0, min_p=1.0, pinned=True),  # every token ties the maximum: w = 1 exactly, all stay
    # greedy-like
    _case("greedy_full", 32000, "quant", 0, T=0.0),
    _case("greedy_k200_minp", 151936, "gauss", 200, T=0.0, min_p=0.05),
    # ban, penalty, sets
    _case("ban_expires", 32000, "gauss", 200, top_p=0.9, ban=(4, 60, "top4"), pos0=17, counter=WRAP32),
    _case("rep_seeded", 4096, "gauss", 200, top_p=0.9, rp=1.3, seen0="half"),
    _case("rep_full_minp", 32000, "quant", 0, min_p=0.05, rp=1.05, seen0="top4", n=100),
    _case("rep_mixed_k65", 300, "mixed", 65, rp=2.0, seen0="half", seed=3),
    _case("rep_reward", 1000, "gauss", 100, top_p=0.8, rp=0.8, seen0="rank4to7"),
    _case("sup_all_but_one", 300, "gauss", 0, top_p=0.9, min_p=0.1, rp=1.3, suppress="all_but_137", n=16, pinned=True),
    _case("sup_everything", 300, "gauss", 200, suppress="all", n=8, pinned=True),
    _case("sup_top4_k65", 4096, "gauss", 65, suppress="top4", rp=1.05),
    # the penalty in front of the temperature: fl32(0x212B / 1.05) is the fp16 value 0x20EC exactly -- a tie, the lower (unseen) id first
    _case("pen_before_scale", 300, "flat", 1, T=0.7, rp=1.05, seen0=(200, ), plant=((200, 0x212B), (100, 0x20EC)), n=4, pinned=True),
    # NaN and -inf
    _case("nan_few_full", 32000, "nan_few", 0, T=0.8, top_p=0.9, n=100),
    _case("nan_all", 4096, "nan_all", 200, n=8, pinned=True),
    _case("ninf_at_cut_k65", 1000, "ninf_tail", 65, pinned=True),   # 40 finite logits, the cut among the -inf ones
    _case("ninf_full_p", 32000, "ninf_tail", 0, top_p=0.9),
    # embedding fold
    _case("embed_64", 4096, "gauss", 200, min_p=0.05, dim=64, n=60),
]
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


def case_inputs(c):
    """(logits fp16 [V], seen0 ids, suppress ids, ban tuple with absolute until_pos and 4 ids or None)"""
    if c.prof in ("mixed", "flat"):  # (sampler_rep_model's: every kind of logit / -5 everywhere)
        x = rm.case_logits(rm.Case(c.name, c.V, c.prof, (), 0, 0, 0, 0, 0, 0, 0, (), (), None, 0, 0, 0))
    else:
        x = profile(c.prof, c.V).copy()
    for t, val in c.plant:  # (id, fp16 bit pattern or float)
        x[t] = rm._f16(val)

    def resolve(spec):
        if spec == "all":
            return tuple(range(c.V))
        return rm._resolve(spec, x, c.V)
    ban = None
    if c.ban is not None:
        nb, until, ids = c.ban
        ids = resolve(ids)
        ban = (nb, c.pos0 + until, tuple(ids) + (0, ) * (4 - len(ids)))
    return x, resolve(c.seen0), resolve(c.suppress), ban


def case_run(c, forced=None, fault=None, n_dev=None):
    x, seen0, suppress, ban = case_inputs(c)
    return run(x, c.n, c.top_k, c.T, c.top_p, c.min_p, c.seed, c.counter, c.pos0, ban, c.seq_cap, c.rp, seen0, suppress, forced, fault, n_dev)
