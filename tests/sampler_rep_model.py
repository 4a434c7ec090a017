"""Host model of gq_sample_topk_rep (csrc/sampler.hip: the REP instances of sample_stage1 / sample_stage2) and of gq_token_set_build, in numpy.
Like tests/sampler_model.py it restates the CONTRACT of include/gq_hip.h, not the kernels: no slices, keys or work buffers.  hash32,
uniform, nucleus, the logit profiles and the error constants are sampler_model's own.

One draw, in order
  suppress  a token of the suppress set is no candidate; neither is a token of the ban list while pos < until_pos.  Nothing left: the token
            is EMPTY_TOKEN (INT_MAX), the state advances as always and the seen set stays (what the other entry points do with an empty set)
  penalty   v = fp16 logit as fp32, rp = fp32 penalty; a token of `seen` gets s = v < 0 ? v * rp : v / rp -- np.float32 operations, which
            are correctly rounded (a true division); -0 is not < 0; every other token has s = v
  order     candidates = the first top_k (clamped to [1, KM]) of (s descending by its fp32 bit pattern image: -0 below +0; id ascending)
  T, nucleus, race, counter, pos, seq   as sampler_model.run, with s in place of the fp16 value (s is exact here: no grant for it)
  state     the drawn token joins `seen`

Every draw changes the set, so a run is TEACHER-FORCED: `forced` holds the tokens a device run produced, and draw i is judged with the set
those tokens left behind (seen0 + forced[:i]).  Per draw the answer is the model's token, the admissible tokens and decided or not --
sampler_model's error model, the C1_EQ grant going to candidates of equal FP32 value s.  Without `forced` the model follows its own tokens.

`fault=` injects one deviation (FAULTS), for tests/test_sampler_rep_model_cpu.py only.  One deviation that suggests itself is NOT in the
list because no input can show it: comparing `v <= 0` instead of `v < 0` moves only +0 and -0 from the division to the product, and for
rp > 0 both give the same zero of the same sign.
"""
from collections import namedtuple

import numpy as np

import sampler_model as sm
from sampler_model import C0, C1, C1_EQ, C2, M32, hash32, nucleus, profile, uniform  # noqa: F401  (one definition of each)

EMPTY_TOKEN = 0x7FFFFFFF
FAULTS = ("mul_div_swapped", "penalty_per_occurrence", "s_rounded_to_fp16", "set_not_updated", "set_updated_before_draw", "suppress_ignored",
          "suppressed_counts_to_top_k")


def token_set(ids, V, base=None):
    """gq_token_set_build: uint32 [ceil(V / 32)], token t = bit t & 31 of word t >> 5; ids outside [0, V) are ignored; base = the set before
    (None: cleared)"""
    w = np.zeros((V + 31) // 32, dtype=np.uint32) if base is None else np.array(base, dtype=np.uint32)
    ids = np.asarray(list(ids), dtype=np.int64).reshape(-1)
    ids = ids[(ids >= 0) & (ids < V)]
    np.bitwise_or.at(w, ids >> 5, (np.uint32(1) << (ids & 31).astype(np.uint32)))
    return w


def image32(s):
    """monotone integer image of fp32 bit patterns: larger value, larger image; -0 directly below +0"""
    b = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32).astype(np.int64)
    return np.where(b & 0x80000000, 0xFFFFFFFF - b, b | 0x80000000)


def penalised(v32, rp, times=None, fault=None):
    """s of SEEN tokens with fp32 logits v32 (times: occurrences per token, for the per-occurrence fault)"""
    rp = np.float32(rp)
    s = np.array(v32, dtype=np.float32)
    reps = 1 if times is None else int(np.max(times, initial=1))
    with np.errstate(all="ignore"):
        for r in range(reps):
            neg = s < 0 if fault != "mul_div_swapped" else ~(s < 0)
            nxt = np.where(neg, s * rp, s / rp).astype(np.float32)
            s = nxt if times is None else np.where(np.asarray(times) > r, nxt, s)
        if fault == "s_rounded_to_fp16":
            s = s.astype(np.float16).astype(np.float32)
    return s


Run = namedtuple("Run", "tokens admissible undecided margin_to counter pos tok seq boundary_dist seen candidates0")


def run(logits, n, top_k, T, top_p=1.0, seed=0, counter=0, pos=0, ban=None, seq_cap=0, rp=1.0, seen0=(), suppress=(), forced=None, fault=None):
    """n consecutive draws.  seen0: the history so far (ids, duplicates allowed), suppress: ids, forced: the tokens a device run drew (None:
    the model's own).  Returns sampler_model.Run's fields plus `seen` (the set after the run, as gq_token_set_build lays it out) and
    `candidates0` (the candidate ids of the first draw, best first)."""
    logits = np.ascontiguousarray(logits, dtype=np.float16)
    V = logits.size
    assert top_k <= 64 and V <= sm.MAX_VOCAB, "GQ_ENOTSUP"
    assert np.isfinite(rp) and rp > 0, "GQ_EINVAL"
    k = min(max(top_k, 1), 32 if top_k <= 32 else 64)
    Tq = float(max(np.float32(T), np.float32(1e-5)))
    v32 = logits.astype(np.float32)
    dead = np.zeros(V, dtype=bool)  # suppressed
    sup = np.asarray([t for t in suppress if 0 <= t < V], dtype=np.int64)
    if fault != "suppress_ignored":
        dead[sup] = True
    dead[np.isnan(v32)] = True  # a NaN logit of either sign is never a candidate (sampler_model.py): it ranks with the suppressed ids
    drop_after = dead if fault == "suppressed_counts_to_top_k" else None  # (fault: selected with the others, removed behind the top-k)
    sel_dead = np.zeros(V, dtype=bool) if drop_after is not None else dead
    img0 = image32(v32)
    static = np.lexsort((np.arange(V), -img0))  # ids by (value descending, id ascending), nobody penalised
    static = static[~sel_dead[static]]
    count = np.zeros(V, dtype=np.int64)
    seen_ids = []
    for t in seen0:
        if 0 <= t < V:
            if not count[t]:
                seen_ids.append(int(t))
            count[t] += 1
    ctr0 = counter & 0xFFFFFFFF
    nb, until, bids = (ban[0], ban[1], [b for b in ban[2][:ban[0]] if 0 <= b < V]) if ban is not None and ban[0] > 0 else (0, 0, [])
    tokens = np.empty(n, dtype=np.int64)
    undecided = np.zeros(n, dtype=bool)
    admissible, detail = [None] * n, [None] * n
    bdist, cand0, seq = np.inf, None, {}
    for i in range(n):
        if fault == "set_updated_before_draw" and forced is not None and 0 <= forced[i] < V:
            if not count[forced[i]]:
                seen_ids.append(int(forced[i]))
            count[forced[i]] += 1
        banned = bids if (nb and pos + i < until) else []
        # candidates: the best k unseen tokens of the static order, merged with the seen tokens at their penalised values
        m = len(seen_ids)
        head = static[:k + m + len(banned)]
        head = head[count[head] == 0]
        sid = np.asarray(seen_ids, dtype=np.int64)
        sid = sid[~sel_dead[sid]] if m else sid
        ids = np.concatenate([head, sid])
        s = np.concatenate([v32[head], penalised(v32[sid], rp, count[sid] if fault == "penalty_per_occurrence" else None, fault)]).astype(np.float32)
        if banned:
            live = ~np.isin(ids, banned)
            ids, s = ids[live], s[live]
        sel = np.lexsort((ids, -image32(s)))[:k]
        ids, s = ids[sel], s[sel]
        if drop_after is not None:
            live = ~drop_after[ids]
            ids, s = ids[live], s[live]
        if i == 0:
            cand0 = ids.copy()
        ctr = (ctr0 + i) & 0xFFFFFFFF
        tok = EMPTY_TOKEN
        if ids.size:
            with np.errstate(over="ignore", invalid="ignore"):
                a = s.astype(np.float64) / Tq
            keep, dist = nucleus(a, ids, top_p)
            bdist = min(bdist, dist)
            ids_k, s_k, a_k = ids[keep], s[keep], a[keep]
            u = uniform(seed, np.uint64(ctr), ids_k)
            with np.errstate(divide="ignore", invalid="ignore"):
                L = -np.log(u)
                score = a_k - np.log(L)
                errg = C0 + C2 / L
                best = score.max()
                w = int(np.where(score == best, ids_k, np.iinfo(np.int64).max).argmin())
                same = s_k == s_k[w]  # equal fp32 values carry the identical fl(s / T)
                absa = np.where(np.isfinite(a_k), np.abs(a_k), 0.0)
                grant = errg + np.where(same, C1_EQ, C1) * absa + errg[w] + np.where(same, C1_EQ, C1) * absa[w]
                margin = best - score
                adm = np.isfinite(score) & (margin <= grant)
            adm[w] = False
            tok = int(ids_k[w])
            admissible[i] = np.concatenate([[tok], ids_k[adm]]).astype(np.int64)
            undecided[i] = bool(adm.any())
            detail[i] = (ids_k, margin, grant)
        else:
            admissible[i], detail[i] = np.array([EMPTY_TOKEN], dtype=np.int64), (ids, np.zeros(0), np.zeros(0))
        tokens[i] = tok
        drawn = tok if forced is None else int(forced[i])
        if pos + i + 1 < seq_cap:
            seq[pos + i + 1] = drawn
        if fault not in ("set_not_updated", "set_updated_before_draw") and 0 <= drawn < V:
            if not count[drawn]:
                seen_ids.append(drawn)
            count[drawn] += 1

    def margin_to(draw, token):
        ids_, m_, g_ = detail[draw]
        hit = np.nonzero(ids_ == token)[0]
        if hit.size == 0 or not np.isfinite(m_[hit[0]]):
            return np.inf, 0.0
        return float(m_[hit[0]]), float(g_[hit[0]])

    end = (ctr0 + n) & 0xFFFFFFFF
    last = int(tokens[-1]) if forced is None else int(forced[n - 1])
    return Run(tokens, admissible, undecided, margin_to, end - (1 << 32) if end >= 1 << 31 else end, pos + n, last, seq, bdist,
               token_set(seen_ids, V), cand0)


# ------------------------------------------------------------------------------------------------ the committed cases
# logits = sampler_model.profile(prof, V) (or "mixed" / "flat" below) with `plant` = ((id, fp16 bit pattern or float), ...) written over it.
# seen0 / suppress / ban ids: tuples of ids, or a string resolved against the logits by case_inputs.
Case = namedtuple("Case", "name V prof plant top_k T top_p seed counter n rp seen0 suppress ban pos0 seq_cap dim")
RPS = (1.05, 1.3, 2.0, 0.8)


def _case(name, V, prof, top_k, T, rp, seen0=(), suppress=(), plant=(), top_p=1.0, seed=77, counter=0, n=None, ban=None, pos0=0, seq_cap=None, dim=0):
    if n is None:
        n = 300 if V > 32000 else 600
    if seq_cap is None:
        seq_cap = pos0 + n + 2
    return Case(name, V, prof, tuple(plant), top_k, T, top_p, seed, counter, n, rp, seen0, suppress, ban, pos0, seq_cap, dim)


def layout_ids(V):
    """ids at which the bit layout of a set can go wrong: 0, 31, 32, V - 1, the first and last id of stage-1 slice 5 (and of the last
    slice), and an id >= 131072"""
    per = (V + sm.BLOCKS - 1) // sm.BLOCKS
    last_slice = (V - 1) // per
    ids = {0, 31, 32, V - 1, 5 * per, 6 * per - 1, last_slice * per, 131072, 131072 + 33}
    return tuple(sorted(t for t in ids if 0 <= t < V))


def _f16(x):
    return np.float16(x) if not isinstance(x, int) else np.array([x], dtype=np.uint16).view(np.float16)[0]


# values at which the penalty's formula can go wrong: positive, negative, both zeros, both infinities' finite side, subnormals
MIXED_BITS = (0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x3800, 0xB800, 0x3C00, 0xBC00, 0x4000, 0xC000, 0x4200, 0xFC00)


def case_logits(c):
    if c.prof == "mixed":
        rng = np.random.default_rng(2000 + c.V)
        x = np.asarray(MIXED_BITS, dtype=np.uint16)[rng.integers(0, len(MIXED_BITS), c.V)].view(np.float16).copy()
    elif c.prof == "flat":
        x = np.full(c.V, -5.0, dtype=np.float16)
    else:
        x = profile(c.prof, c.V).copy()
    for t, val in c.plant:
        x[t] = _f16(val)
    return x


def _resolve(spec, x, V):
    if not isinstance(spec, str):
        return tuple(int(t) for t in spec)
    rank = sm.candidates(x, 64)
    if spec == "layout":
        return layout_ids(V)
    if spec == "half":  # every second id and the layout ids
        return tuple(sorted(set(range(0, V, 2)) | set(layout_ids(V))))
    if spec == "argmax":
        return (int(rank[0]), )
    if spec == "top4":
        return tuple(int(t) for t in rank[:4])
    if spec == "rank4to7":
        return tuple(int(t) for t in rank[4:8])
    if spec == "all_but_137":
        return tuple(t for t in range(V) if t != 137)
    raise KeyError(spec)


def case_inputs(c):
    """(logits fp16 [V], seen0 ids, suppress ids, ban tuple with absolute until_pos and 4 ids or None)"""
    x = case_logits(c)
    ban = None
    if c.ban is not None:
        nb, until, ids = c.ban
        ids = _resolve(ids, x, c.V)
        ban = (nb, c.pos0 + until, tuple(ids) + (0, ) * (4 - len(ids)))
    return x, _resolve(c.seen0, x, c.V), _resolve(c.suppress, x, c.V), ban


def case_run(c, forced=None, fault=None):
    x, seen0, suppress, ban = case_inputs(c)
    return run(x, c.n, c.top_k, c.T, c.top_p, c.seed, c.counter, c.pos0, ban, c.seq_cap, c.rp, seen0, suppress, forced, fault)


def _neighbours_of_penalised_one():
    """the fp16 values directly below and above fl32(1.0 / 1.05), which is no fp16 value"""
    s = np.float32(1.0) / np.float32(1.05)
    h = np.float16(s)
    lo, hi = (h, np.nextafter(h, np.float16(2))) if np.float32(h) < s else (np.nextafter(h, np.float16(0)), h)
    assert np.float32(lo) < s < np.float32(hi)
    return float(lo), float(hi)


_LO, _HI = _neighbours_of_penalised_one()
CASES = []
# set layout: every vocabulary size, the layout ids planted high so that a wrong bit shows in the draws; as seen ids and as suppressed ids
for _i, _V in enumerate((1, 2, 33, 300, 4096, 131072, 131073, 151936, 262144)):
    _pl = tuple((t, 9.0 + (j % 4) / 4) for j, t in enumerate(layout_ids(_V)))
    CASES.append(_case("layout_seen_v%d" % _V, _V, "gauss", 50, 1.0, RPS[_i % 4] if RPS[_i % 4] > 1 else 2.0, seen0="layout", plant=_pl, counter=_i, n=16 if _V < 3 else None))
    CASES.append(_case("layout_sup_v%d" % _V, _V, "gauss", 33, 1.0, 1.05, suppress=layout_ids(_V)[:1] if _V < 3 else "layout", plant=_pl, seed=_i, n=16 if _V < 3 else None))
CASES += [
    # values: every kind of logit among the seen tokens, every penalty (0.8 rewards repetition: the products and quotients grow)
    *[_case("values_rp%g" % r, 300, "mixed", 64, 1.0, r, seen0="half", seed=j) for j, r in enumerate(RPS)],
    *[_case("values_wide_rp%g" % r, 131073, "mixed", 64, 2.5, r, seen0="half", seed=j, counter=sm.WRAP32) for j, r in enumerate(RPS[:2])],
    _case("values_plus_inf", 300, "gauss", 4, 1.0, 1.3, seen0=(7, ), plant=((7, 0x7C00), ), n=16),
    _case("values_quant", 4096, "quant", 50, 0.3, 1.3, seen0="half", top_p=0.95),
    # fp32 order 1: token 10 seen at 1.0 / 1.05, strictly between two adjacent fp16 values held by unseen tokens on either side of its id
    _case("between_fp16_k2", 300, "flat", 2, 1.0, 1.05, seen0=(10, ), plant=((10, 1.0), (20, _HI), (5, _LO)), n=300),
    _case("between_fp16_greedy", 300, "flat", 1, 0.0, 1.05, seen0=(10, ), plant=((10, 1.0), (20, _HI), (5, _LO)), n=8),
    _case("between_fp16_k2_wide", 131073, "flat", 2, 1.0, 1.05, seen0=(131072, ), plant=((131072, 1.0), (131073 - 40000, _LO), (40000, _HI)), n=300),
    # fp32 order 2: a seen 2.0 at rp = 2 ties an unseen 1.0; the lower id on either side
    _case("tie_seen_lower", 300, "flat", 1, 0.0, 2.0, seen0=(40, ), plant=((40, 2.0), (41, 1.0)), n=8),
    _case("tie_seen_higher", 300, "flat", 1, 0.0, 2.0, seen0=(41, ), plant=((41, 2.0), (40, 1.0)), n=8),
    _case("tie_k2_sampled", 4096, "flat", 2, 1.0, 2.0, seen0=(3000, ), plant=((3000, 2.0), (100, 1.0), (3500, 1.0)), n=300),
    # cut: the penalised arg-max leaves the top k and token number k + 1 enters
    *[_case("cut_k%d" % k, 4096, "gauss", k, 1.0, 2.0, seen0="argmax", seed=k, n=300) for k in (1, 32, 33, 64)],
    # state: every draw penalises itself -- 0, 1, 2, ... (top_k = 1: among equal logits the lowest unseen id is the one candidate)
    _case("state_v300", 300, "equal", 1, 0.0, 1.3, n=300),
    _case("state_v131073", 131073, "equal", 1, 0.0, 1.3, n=300),
    # suppress
    _case("sup_argmax", 4096, "gauss", 50, 0.3, 1.05, suppress="argmax"),
    _case("sup_argmax_greedy", 32000, "gauss", 1, 0.0, 1.3, suppress="argmax", n=64),
    _case("sup_and_seen", 4096, "gauss", 2, 1.0, 1.3, seen0="top4", suppress="top4", n=300),
    _case("sup_all_but_one", 300, "gauss", 50, 1.0, 1.3, suppress="all_but_137", n=16),
    _case("sup_ban_active", 4096, "gauss", 8, 1.0, 1.05, suppress="rank4to7", ban=(4, 10**6, "top4"), n=300),
    _case("sup_ban_expires", 4096, "gauss", 8, 1.0, 1.05, suppress="rank4to7", ban=(4, 150, "top4"), pos0=17, n=300),
    _case("sup_nucleus_embed", 4096, "quant", 64, 2.5, 1.05, suppress="top4", top_p=0.9, dim=64, n=300, seed=1),
    _case("sup_embed_wide", 151936, "gauss", 50, 1.0, 1.3, suppress="top4", seen0="rank4to7", dim=8, n=300),
]
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
