"""CPU: tests/sampler_adj_model.py, the host model of the additive adjustment (frequency_penalty, presence_penalty, logit_bias), against
exact rational arithmetic rounded step by step, and the model's own committed cases against injected faults."""
from fractions import Fraction

import numpy as np
import pytest

import sampler_adj_model as am


def rne(q, prec, emin, emax):
    """the number of the binary format (prec significand bits, exponents emin .. emax, subnormals) nearest to the rational q, ties to
    even; +-inf past the format's range (as a float: every format here fits a double)"""
    if q == 0:
        return 0.0
    sign, a = (-1.0 if q < 0 else 1.0), abs(q)
    e = max(a.numerator.bit_length() - a.denominator.bit_length(), emin)
    while e > emin and Fraction(2) ** e > a:
        e -= 1
    while Fraction(2) ** (e + 1) <= a:
        e += 1
    ulp = Fraction(2) ** (e - prec + 1)
    n, r = divmod(a, ulp)
    n = int(n)
    if r * 2 > ulp or (r * 2 == ulp and n % 2 == 1):
        n += 1
    out = n * ulp
    if out >= Fraction(2) ** (emax + 1):
        return sign * float("inf")
    return sign * float(out)


def fl32(q):
    return rne(q, 24, -126, 127)


def fl16(q):
    return rne(q, 11, -14, 15)


def exact_adjust(v, b, c, fp, pp):
    """the formula on finite inputs, every operation exact and then rounded once"""
    F = Fraction
    p = F(0)
    if c > 0:
        p = F(fl32(F(fl32(F(fp) * c)) + F(pp)))
    return fl16(F(fl32(F(fl32(F(v) + F(b))) - p)))


def test_the_rounding_helper_knows_the_formats():
    assert fl16(Fraction(65520)) == float("inf") and fl16(Fraction(65519)) == 65504.0
    assert fl16(Fraction(1, 2**25)) == 0.0 and fl16(Fraction(3, 2**26)) == 2.0**-24 and fl16(Fraction(1, 2**24)) == 2.0**-24
    assert fl16(1 + Fraction(1, 2**11)) == 1.0 and fl16(1 + Fraction(3, 2**11)) == 1.0 + 2.0**-9
    assert fl32(Fraction(1, 10)) == float(np.float32(0.1)) and fl32(Fraction(2)**128) == float("inf")
    assert fl32(Fraction(1, 2**150)) == 0.0 and fl32(Fraction(1, 2**149)) == 2.0**-149


@pytest.mark.parametrize("row", am.FORMULA_CASES, ids=lambda r: r[0])
def test_committed_case(row):
    name, bits, b, c, fp, pp, want = row
    s, member = am.formula_case(row)
    x = np.array([bits], dtype=np.uint16).view(np.float16)
    got = am.adjusted_logits(x, {} if b is None else {0: b}, [c], fp, pp).view(np.uint16)[0]
    assert member == (b is not None or c > 0)
    if want is None:
        assert np.isnan(s) and (got & 0x7FFF) > 0x7C00, (name, hex(got))
        return
    assert got == want, (name, hex(got), hex(want))
    if not member:
        assert got == bits
    v = float(x[0])
    if member and np.isfinite(v):  # against exact rationals (the sign of a zero is the table's own expectation)
        exact = exact_adjust(v, 0.0 if b is None else float(np.float32(b)), c, float(np.float32(fp)), float(np.float32(pp)))
        assert float(np.array([got], dtype=np.uint16).view(np.float16)[0]) == exact, (name, exact)


def test_random_members_against_exact_rationals():
    rng = np.random.default_rng(7)
    n = 3000
    bits = rng.integers(0, 0x7C00, n).astype(np.uint16) | (rng.integers(0, 2, n).astype(np.uint16) << 15)  # every finite fp16 value
    x = bits.view(np.float16)
    scale = 2.0 ** rng.integers(-26, 18, n)
    b = (rng.standard_normal(n) * scale).astype(np.float32)
    c = rng.integers(0, 6, n)
    c[::17] = rng.integers(2**20, 2**24, c[::17].size)  # (large counts: the product's rounding)
    fp = (rng.standard_normal(n) * 2.0 ** rng.integers(-12, 4, n)).astype(np.float32)
    pp = (rng.standard_normal(n) * 2.0 ** rng.integers(-12, 4, n)).astype(np.float32)
    bits[::13], b[::13], c[::13] = 0, (b[::13] * np.float32(2.0**-40)).astype(np.float32), 0  # (results below half the smallest subnormal)
    kinds = set()
    for i in range(n):
        got = am.adjusted_logits(x[i:i + 1], {0: float(b[i])}, [int(c[i])], float(fp[i]), float(pp[i]))
        exact = exact_adjust(float(x[i]), float(b[i]), int(c[i]), float(fp[i]), float(pp[i]))
        g = float(got[0])
        assert g == exact, (i, hex(int(bits[i])), float(b[i]), int(c[i]), float(fp[i]), float(pp[i]), g, exact)
        kinds.add("inf" if np.isinf(g) else "sub" if 0 < abs(g) < 2.0**-14 else "zero" if g == 0 else "normal")
    assert kinds == {"inf", "sub", "zero", "normal"}, kinds


def test_membership_over_a_vector():
    x = np.array([0x8000, 0x8000, 0x8000, 0x7E7E, 0x3C00, 0x3C00], dtype=np.uint16).view(np.float16)
    counts = [0, 0, 2, 0, 0, 1]
    got = am.adjusted_logits(x, {0: 0.0, 4: 0.25}, counts, 0.5, 0.25).view(np.uint16)
    # listed 0.0: -0 -> +0; unlisted -0: stays; counted -0: 0 - 1.25; unlisted NaN: stays; listed: 1.25; counted once: 1 - 0.75
    assert got.tolist() == [0x0000, 0x8000, 0xBD00, 0x7E7E, 0x3D00, 0x3400]
    assert am.adjusted_logits(x, None, np.zeros(6, dtype=np.int64), 0.5, 0.25).view(np.uint16).tolist() == x.view(np.uint16).tolist()


def test_frequency_and_presence_are_told_apart_by_a_token_counted_twice():
    x = np.full(3, 2.0, dtype=np.float16)
    counts = [0, 1, 2]
    freq = am.adjusted_logits(x, None, counts, 0.5, 0.0).astype(np.float32).tolist()
    pres = am.adjusted_logits(x, None, counts, 0.0, 0.5).astype(np.float32).tolist()
    assert freq == [2.0, 1.5, 1.0] and pres == [2.0, 1.5, 1.5]


def test_the_prompt_does_not_count():
    assert am.tally(8, [1, 1, 9, -1, 7], prompt=[1, 2, 3]).tolist() == [0, 2, 0, 0, 0, 0, 0, 1]
    assert am.tally(8, [1, 1, 7], prompt=[1, 2, 3], fault="prompt_counted").tolist() == [0, 3, 1, 1, 0, 0, 0, 1]


@pytest.mark.parametrize("fault", am.FAULTS)
def test_every_fault_is_caught_by_a_committed_case(fault):
    if fault == "prompt_counted":  # a fault of the tally: caught by a penalised draw of a prompt token
        x = np.full(8, 1.0, dtype=np.float16)
        good = am.adjusted_logits(x, None, am.tally(8, [1], prompt=[2]), 0.5, 0.5)
        bad = am.adjusted_logits(x, None, am.tally(8, [1], prompt=[2], fault=fault), 0.5, 0.5)
        assert good.tolist() == [1, 0, 1, 1, 1, 1, 1, 1] and bad[2] != good[2]
        return
    caught = []
    for row in am.FORMULA_CASES:
        want = row[-1]
        if want is None:
            continue
        s, _ = am.formula_case(row, fault)
        with np.errstate(over="ignore"):
            s16 = np.float32(s).astype(np.float16)
        if not (np.float32(s16) == s and s16.view(np.uint16) == want):
            caught.append(row[0])
    assert caught, fault
    print(fault, "caught by", caught)
    expect = {"fused_multiply_add": "product_rounded_before_the_sum", "penalty_without_count": "listed_no_count", "left_in_fp32": "rounded_to_fp16"}
    assert expect[fault] in caught


def test_the_case_tables_cover_what_the_gpu_tests_promise():
    names = [c.name for c in am.TOPK_CASES]
    assert sorted({c.V for c in am.TOPK_CASES if c.name.startswith("layout_")}) == [1, 33, 300, 4096, 131073, 262144]
    assert {c.top_k for c in am.TOPK_CASES} >= {1, 2, 50, 64} and all(64 <= c.n <= 300 for c in am.TOPK_CASES + am.FULL_CASES)
    for need in ("equal_greedy_walk", "bias_only", "bias_ties_both_sides", "bias_to_minus_inf", "mix_rp_suppress_ban", "nucleus", "embed_fold", "lp_cap_short"):
        assert need in names
    assert sorted({c.V for c in am.FULL_CASES if c.name.startswith("full_layout_")}) == [33, 4096, 151936, 262144]
    assert {c.top_k for c in am.FULL_CASES} == {0, 2, 200} and {c.top_p for c in am.FULL_CASES} == {1.0, 0.9} and {c.min_p for c in am.FULL_CASES} == {0.0, 0.05}
    for c in am.TOPK_CASES + am.FULL_CASES:
        x, bias, pre, seen0, suppress, ban = am.case_inputs(c)
        assert x.dtype == np.float16 and x.size == c.V and all(0 <= t < c.V for t in bias) and pre.shape == (c.V, )
        # the tie cases tie: token 10's adjusted logit equals its unlisted neighbours'
        if "bias_ties" in c.name:
            adj = am.adjusted_logits(x, bias, pre, c.fp, c.pp).view(np.uint16)
            assert adj[10] == adj[20]
