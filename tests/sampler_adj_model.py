"""Host model of the additive adjustment of gq_sample_topk_adj / gq_sample_full_adj (include/gq_hip.h: frequency_penalty, presence_penalty,
logit_bias), in numpy, and the case tables of the two differential GPU tests.

The adjustment is DEFINED to give an fp16 logit, so the model is one function over the logits and nothing else: a draw through the new
entries equals, bit for bit, a draw through the existing entries on `adjusted_logits(raw, ...)`.  For a MEMBER token -- listed in the bias
(a listed 0.0 still makes it one) or generated c > 0 times in this request --

    p  = c > 0 ? fl32(fl32(frequency_penalty * (float)c) + presence_penalty) : 0
    s  = fl32(fl32(v + b) - p)                 v = the fp16 logit widened to fp32, b = its bias (0 when not listed)
    h' = fp16(s)                               to nearest even, subnormals kept, overflow to +-inf, NaN stays NaN

and a non-member keeps its bit pattern (-0 and NaN included).  numpy's float32 operations are correctly rounded one by one and its
float32 -> float16 conversion rounds to nearest even with subnormals: tests/test_sampler_adj_model_cpu.py checks both against exact
rational arithmetic.  The counts are of the tokens generated in this request: `tally` leaves the prompt out.

`fault=` injects one deviation (FAULTS), for tests/test_sampler_adj_model_cpu.py only.
"""
from collections import namedtuple

import numpy as np

import sampler_model as sm
from sampler_rep_model import layout_ids

FAULTS = ("fused_multiply_add", "penalty_without_count", "prompt_counted", "left_in_fp32")


def tally(V, generated, prompt=(), fault=None):
    """int64 [V]: how often each token was GENERATED in this request (the prompt does not count)"""
    c = np.zeros(V, dtype=np.int64)
    ids = list(generated) + (list(prompt) if fault == "prompt_counted" else [])
    for t in ids:
        if 0 <= t < V:
            c[t] += 1
    return c


def adjusted_values(x16, bias, counts, fp, pp, fault=None):
    """fp32 [V]: the value every token carries into the draw (h' widened; a non-member's own logit widened), and the member mask"""
    x16 = np.ascontiguousarray(x16, dtype=np.float16)
    V = x16.size
    b = np.zeros(V, dtype=np.float32)
    listed = np.zeros(V, dtype=bool)
    for t, val in (bias or {}).items():
        b[int(t)] = np.float32(val)
        listed[int(t)] = True
    c = np.asarray(counts, dtype=np.int64).reshape(V)
    member = listed | (c > 0)
    v = x16.astype(np.float32)
    fp, pp = np.float32(fp), np.float32(pp)
    with np.errstate(all="ignore"):
        cf = c.astype(np.float32)
        if fault == "fused_multiply_add":  # fl32(fp * c + pp): one rounding (the product of two fp32 numbers is exact in float64)
            p = (fp.astype(np.float64) * cf.astype(np.float64) + np.float64(pp)).astype(np.float32)
        else:
            p = ((fp * cf).astype(np.float32) + pp).astype(np.float32)
        p = np.where((c > 0) | (fault == "penalty_without_count"), p, np.float32(0.0)).astype(np.float32)
        s = ((v + b).astype(np.float32) - p).astype(np.float32)
        if fault != "left_in_fp32":
            s = s.astype(np.float16).astype(np.float32)
    return np.where(member, s, v).astype(np.float32), member


def adjusted_logits(x16, bias, counts, fp, pp):
    """fp16 [V]: the logits the draw is made from -- x16: the raw fp16 logits; bias: {id: value} or None; counts: int [V], the tokens generated
    so far in this request; fp, pp: frequency and presence penalty"""
    x16 = np.ascontiguousarray(x16, dtype=np.float16)
    s, member = adjusted_values(x16, bias, counts, fp, pp)
    out = x16.copy()
    with np.errstate(all="ignore"):
        out[member] = s[member].astype(np.float16)  # (exact: s is an fp16 value)
    return out


# ------------------------------------------------------------------------------------------------ the formula's committed cases
# (fp16 bit pattern of the logit, bias or None = not listed, count, frequency_penalty, presence_penalty, expected fp16 bit pattern or None)
# -- every expectation is worked out by hand in the comment; tests/test_sampler_adj_model_cpu.py also checks each against exact rationals
FORMULA_CASES = [
    # membership: a listed 0.0 turns -0 into +0 (-0 + +0 = +0), an unlisted -0 with no count stays; so does an unlisted NaN
    ("listed_zero_bias_minus0", 0x8000, 0.0, 0, 0.5, 0.25, 0x0000),
    ("unlisted_minus0", 0x8000, None, 0, 0.5, 0.25, 0x8000),
    ("unlisted_nan", 0x7E7E, None, 0, 0.5, 0.25, 0x7E7E),
    ("counted_minus0_zero_penalties", 0x8000, None, 3, 0.0, 0.0, 0x0000),
    # a listed bias with c == 0: no penalty, whatever the two are
    ("listed_no_count", 0x3C00, 1.0, 0, 7.0, 9.0, 0x4000),
    # round to nearest EVEN: 1 + 2^-11 lies half way between 0x3C00 and 0x3C01 -> 0x3C00; 1 + 2^-10 + 2^-11 half way between 0x3C01 and 0x3C02 -> 0x3C02
    ("tie_to_even_down", 0x3C00, 2.0**-11, 0, 0.0, 0.0, 0x3C00),
    ("tie_to_even_up", 0x3C01, 2.0**-11, 0, 0.0, 0.0, 0x3C02),
    # a subnormal result: 2^-14 - 2^-15 = 2^-15 = 0x0200; and the smallest one, 2^-24
    ("subnormal", 0x0400, -2.0**-15, 0, 0.0, 0.0, 0x0200),
    ("subnormal_min", 0x0000, 2.0**-24, 0, 0.0, 0.0, 0x0001),
    ("subnormal_tie_to_zero", 0x0000, 2.0**-25, 0, 0.0, 0.0, 0x0000),
    # overflow: -60000 - 70000 -> -inf; 65504 + 16 = 65520 is the tie that rounds to +inf; 65504 + 15 stays
    ("overflow_minus_inf", 0xFB53, -70000.0, 0, 0.0, 0.0, 0xFC00),
    ("overflow_tie_plus_inf", 0x7BFF, 16.0, 0, 0.0, 0.0, 0x7C00),
    ("below_overflow", 0x7BFF, 15.0, 0, 0.0, 0.0, 0x7BFF),
    ("minus_inf_stays", 0xFC00, 100.0, 2, 1.0, 1.0, 0xFC00),
    # NaN stays NaN (the payload is not pinned)
    ("nan_listed", 0x7E7E, 1.0, 0, 0.0, 0.0, None),
    ("nan_counted", 0xFE01, None, 2, 0.5, 0.5, None),
    # frequency and presence: a token counted twice pays 2 * 0.5 + 0.25 = 1.25; counted once 0.75
    ("twice", 0x4000, None, 2, 0.5, 0.25, 0x3A00),
    ("once", 0x4000, None, 1, 0.5, 0.25, 0x3D00),
    # negative penalties reward: 1 - (3 * -0.5 + -0.25) = 2.75
    ("negative_penalties", 0x3C00, None, 3, -0.5, -0.25, 0x4180),
    # bias and both penalties: (1 + 0.5) - (2 * 0.25 + 0.125) = 0.875
    ("all_three", 0x3C00, 0.5, 2, 0.25, 0.125, 0x3B00),
    # every operation rounded on its own: fp = 0.1f * 2^20, c = 3: the product rounds UP to 0.3f * 2^20, and with pp = -0.3f * 2^20 the
    # sum is 0 -> h' = +0; one fused multiply-add keeps the product's low bits: p = -2^-7, h' = 2^-7 (0x2000)
    ("product_rounded_before_the_sum", 0x0000, None, 3, float(np.float32(0.1) * np.float32(2.0**20)), float(-np.float32(0.3) * np.float32(2.0**20)), 0x0000),
    # the result is an fp16 value: 1 + 0.001 in fp32 is none -> 0x3C01 (1 + 2^-10 = 1.00098 is the nearest)
    ("rounded_to_fp16", 0x3C00, 0.001, 0, 0.0, 0.0, 0x3C01),
]


def formula_case(row, fault=None):
    """(fp32 value the draw sees, member) of one FORMULA_CASES row"""
    _, bits, b, c, fp, pp, _ = row
    x = np.array([bits], dtype=np.uint16).view(np.float16)
    s, member = adjusted_values(x, {} if b is None else {0: b}, [c], fp, pp, fault)
    return s[0], bool(member[0])


# ------------------------------------------------------------------------------------------------ the cases of the two GPU tests
# logits = sampler_model.profile(prof, V) ("flat": all -5, "ones": all 1.0) with `plant` = ((id, value), ...) written over it; bias / pre:
# ((id, value), ...) / ((id, count), ...) or "layout" = sampler_rep_model.layout_ids(V) with values / counts that differ by id.
# seen0 / suppress: tuples of ids ("all": every id); ban = (n, until (relative to pos0), ids); lp_cut: lp_cap ends this many slots before
# the run does (0: behind it)
Case = namedtuple("Case", "name V prof plant top_k T top_p min_p seed n rp seen0 suppress ban pos0 bias pre fp pp dim lp_cut top_n")


def _case(name, V, prof, top_k, T, fp=0.0, pp=0.0, bias=(), pre=(), plant=(), top_p=1.0, min_p=0.0, seed=5, n=64, rp=1.0, seen0=(), suppress=(),
          ban=None, pos0=0, dim=0, lp_cut=0, top_n=0):
    return Case(name, V, prof, tuple(plant), top_k, T, top_p, min_p, seed, n, rp, seen0, suppress, ban, pos0, bias, pre, fp, pp, dim, lp_cut, top_n)


def case_logits(c):
    if c.prof == "flat":
        x = np.full(c.V, -5.0, dtype=np.float16)
    elif c.prof == "ones":
        x = np.full(c.V, 1.0, dtype=np.float16)
    else:
        x = sm.profile(c.prof, c.V).copy()
    for t, val in c.plant:
        x[t] = np.float16(val)
    return x


def case_inputs(c):
    """(raw logits fp16 [V], bias {id: value}, pre-counts int64 [V], seen0 ids, suppress ids, ban (n, absolute until_pos, 4 ids) or None)"""
    x = case_logits(c)
    lay = layout_ids(c.V)
    bias = {t: (-1.0, 0.5, 2.25, -0.001)[j % 4] for j, t in enumerate(lay)} if c.bias == "layout" else {int(t): float(v) for t, v in c.bias}
    pre = np.zeros(c.V, dtype=np.int64)
    for j, (t, n) in enumerate(((t, 1 + j % 3) for j, t in enumerate(lay)) if c.pre == "layout" else c.pre):
        pre[t] = n
    suppress = tuple(range(c.V)) if c.suppress == "all" else tuple(c.suppress)
    ban = None
    if c.ban is not None:
        nb, until, ids = c.ban
        ban = (nb, c.pos0 + until, tuple(ids) + (0, ) * (4 - len(ids)))
    return x, bias, pre, tuple(c.seen0), suppress, ban


_HALF = 2.0**-11  # half an fp16 ulp at 1.0
TOPK_CASES = []
# the layout of the two new sets and of the dense arrays: every vocabulary, the layout ids planted high so that a wrong bit shows in the
# draws, biased and pre-counted at once
for _i, _V in enumerate((1, 33, 300, 4096, 131073, 262144)):
    _pl = tuple((t, 6.0 + (j % 4) / 4) for j, t in enumerate(layout_ids(_V)))
    TOPK_CASES.append(_case("layout_v%d" % _V, _V, "gauss", (50, 2, 64, 1, 50, 64)[_i], 1.0, fp=0.75, pp=0.5, bias="layout", pre="layout", plant=_pl,
                            seed=_i, n=300 if _V <= 4096 else 64, top_n=(0, 3, 0, 20, 0, 5)[_i]))
TOPK_CASES += [
    # top_k 1 / 2 / 50 / 64 over one profile with both penalties
    *[_case("penalties_k%d" % k, 4096, "gauss", k, 0.7 if k > 1 else 0.0, fp=0.3, pp=0.6, n=128, seed=k) for k in (1, 2, 50, 64)],
    # equal logits, greedy, a frequency penalty: the draw walks 0, 1, 2, ... and then returns by count
    _case("equal_greedy_walk", 33, "ones", 1, 0.0, fp=0.5, n=100),
    _case("equal_greedy_walk_wide", 131073, "ones", 1, 0.0, fp=0.5, n=64),
    # bias only (no count arrays at all); and a listed 0.0 on a -0 logit next to an unlisted -0
    _case("bias_only", 4096, "gauss", 50, 1.0, bias="layout", n=128, top_n=2),
    _case("bias_zero_on_minus0", 300, "flat", 2, 1.0, bias=((10, 0.0), ), plant=((10, -0.0), (5, -0.0), (20, -0.0)), n=64),
    # a bias that creates fp16 ties with unlisted neighbours on both sides of the id: 1.0 + 0.5 against 1.5 at ids 5 and 20; and one that
    # only ties after the rounding (1 + 2^-11 -> 1.0)
    _case("bias_ties_both_sides", 300, "flat", 2, 1.0, bias=((10, 0.5), ), plant=((10, 1.0), (5, 1.5), (20, 1.5)), n=128),
    _case("bias_ties_greedy", 300, "flat", 1, 0.0, bias=((10, 0.5), ), plant=((10, 1.0), (20, 1.5)), n=64),
    _case("bias_ties_after_rounding", 300, "flat", 2, 1.0, bias=((10, _HALF), ), plant=((10, 1.0), (5, 1.0), (20, 1.0)), n=128),
    # a bias of -70000 on the arg-max: -inf; a candidate like any other, never drawn while one is finite
    _case("bias_to_minus_inf", 4096, "gauss", 50, 1.0, bias=((7, -70000.0), ), plant=((7, 30.0), ), n=64, top_n=1),
    # everything at once: repetition penalty (behind the additive terms), suppress, an expiring ban
    _case("mix_rp_suppress_ban", 4096, "gauss", 8, 1.0, fp=0.4, pp=0.2, bias="layout", pre="layout", rp=1.3, seen0=(0, 31, 32, 100, 101), suppress=(1, 2, 4095),
          ban=(2, 40, (3, 4)), pos0=17, n=128, top_n=4),
    _case("mix_negative_penalties", 4096, "quant", 64, 2.5, fp=-0.25, pp=-0.5, rp=0.8, seen0=(5, 6), n=128),
    _case("nucleus", 4096, "quant", 50, 1.0, fp=0.5, pp=0.25, bias="layout", top_p=0.9, n=128),
    # the embedding fold, two widths
    _case("embed_fold", 4096, "gauss", 50, 1.0, fp=0.5, pp=0.5, bias="layout", dim=64, n=64),
    _case("embed_fold_wide", 151936, "gauss", 50, 1.0, fp=0.5, pp=0.5, bias="layout", pre="layout", dim=8, n=64, top_n=2),
    # lp_cap shorter than the run
    _case("lp_cap_short", 300, "gauss", 50, 1.0, fp=0.5, pp=0.5, n=64, lp_cut=20, top_n=3),
    # an empty candidate set: nothing is counted
    _case("all_suppressed", 33, "gauss", 50, 1.0, fp=0.5, pp=0.5, pre=((3, 2), ), bias=((4, 1.0), ), suppress="all", n=64, pos0=2),
]
FULL_CASES = []
for _i, _V in enumerate((33, 4096, 151936, 262144)):
    _pl = tuple((t, 6.0 + (j % 4) / 4) for j, t in enumerate(layout_ids(_V)))
    FULL_CASES.append(_case("full_layout_v%d" % _V, _V, "gauss", (0, 200, 0, 200)[_i], 1.0, fp=0.75, pp=0.5, bias="layout", pre="layout", plant=_pl, seed=_i,
                            top_p=(1.0, 0.9, 0.9, 1.0)[_i], min_p=(0.05, 0.0, 0.0, 0.05)[_i], n=128 if _V <= 4096 else 64, top_n=(3, 0, 5, 0)[_i]))
FULL_CASES += [
    _case("full_no_filter", 4096, "gauss", 0, 1.0, fp=0.3, pp=0.6, n=128),
    _case("full_k200", 4096, "gauss", 200, 0.7, fp=0.3, pp=0.6, n=128),
    _case("full_top_p", 4096, "quant", 0, 1.0, fp=0.5, pp=0.25, bias="layout", top_p=0.9, n=128),
    _case("full_min_p", 4096, "quant", 0, 1.0, fp=0.5, pp=0.25, bias="layout", min_p=0.05, n=128, top_n=2),
    _case("full_equal_by_count", 33, "ones", 0, 0.0, fp=0.5, n=100),
    _case("full_bias_only", 4096, "gauss", 200, 1.0, bias="layout", n=128),
    _case("full_bias_ties_both_sides", 300, "flat", 200, 1.0, bias=((10, 0.5), ), plant=((10, 1.0), (5, 1.5), (20, 1.5)), top_p=0.9, n=128),
    _case("full_bias_ties_inside_cut", 300, "flat", 2, 1.0, bias=((10, 0.5), ), plant=((10, 1.0), (5, 1.5), (20, 1.5)), n=128),
    _case("full_bias_to_minus_inf", 4096, "gauss", 0, 1.0, bias=((7, -70000.0), ), plant=((7, 30.0), ), n=64),
    _case("full_mix_rp_suppress_ban", 4096, "gauss", 200, 1.0, fp=0.4, pp=0.2, bias="layout", pre="layout", rp=1.3, seen0=(0, 31, 32, 100, 101), suppress=(1, 2, 4095),
          ban=(2, 40, (3, 4)), pos0=17, top_p=0.9, min_p=0.05, n=128, top_n=4),
    _case("full_embed_fold", 4096, "gauss", 0, 1.0, fp=0.5, pp=0.5, bias="layout", dim=64, min_p=0.05, n=64),
    _case("full_lp_cap_short", 300, "gauss", 0, 1.0, fp=0.5, pp=0.5, n=64, lp_cut=20, top_n=3),
    _case("full_all_suppressed", 33, "gauss", 0, 1.0, fp=0.5, pp=0.5, pre=((3, 2), ), bias=((4, 1.0), ), suppress="all", n=64, pos0=2),
]
CASE_BY_NAME = {c.name: c for c in TOPK_CASES + FULL_CASES}
assert len(CASE_BY_NAME) == len(TOPK_CASES) + len(FULL_CASES)
