"""CPU: the host model of the full-domain sweeps (tests/halfsweep_model.py).

(a) the reference's own numbers over the 63 488 finite fp16 gates: how many the decode-path tests never reach (|g| > 12), how many have a
    subnormal SiLU, how many have two candidates in each window and how far apart those lie; the strictness caps of both windows -- all
    conditions on the reference alone;
(b) torch's own SiLU (fp32 and fp16 tensors) and numpy's fp32 expression are inside the DELTA_ROWS candidates of every finite gate, and
    torch's leaves fp16(q) at one gate only;
(c) `scramble` is a bijection in every row, rows disagree everywhere, `scramble_finite` is a bijection of the finite patterns;
(d) the fp8 write rule (kv8_model.quantize) over all 65 536 patterns at four reciprocal scales: every code occurs, +-Inf clamp, NaN stays
    NaN, the ties go to the even mantissa;
(e) the selector layers return what was planted through oracle.ap_gemv_f16, bit for bit with -0 as +0;
(f) every fault of halfsweep_model.FAULTS is rejected by the checkers the GPU tests use;
(g) the dry dispatch sends the selector shapes of tests/test_halfsweep_ap_gpu.py to the families that test names.
"""
import numpy as np
import pytest

import halfsweep_model as hs
import kv8_model as k8

G = hs.half(hs.FINITE)
ALL = hs.half(hs.PATTERNS)


def test_the_domain_the_existing_tests_leave_out():
    assert hs.FINITE.size == 63488
    s = hs.to_half(hs.silu64(G))
    assert int((np.abs(G) > 12).sum()) == 25598
    sub = (np.abs(s) < 2.0**-14) & (s != 0)
    assert int(sub.sum()) == 4855 and int((sub & (G < -12)).sum()) == 763
    assert float(G[sub].min()) == pytest.approx(-20.33, abs=0.01) and float(G[sub].max()) == pytest.approx(1.2e-4, rel=0.02)
    assert (hs.bits(s[G < -20.4]) == 0x8000).all()   # -0 from there on
    assert (s[G > 32] == G[G > 32]).all()


@pytest.mark.parametrize("delta,two,cap", [(hs.DELTA_ROWS, 56, 0.002), (hs.DELTA_DECODE, 1991, 0.05)], ids=["rows", "decode"])
def test_windows_and_strictness_caps(delta, two, cap):
    c = hs.bits(hs.silu_candidates(G, delta)).astype(np.int64)
    mag = c & 0x7FFF
    assert (c[0] >> 15 == c[2] >> 15).all()
    assert int(np.abs(mag[0] - mag[2]).max()) == 1                 # never more than one ulp apart ...
    assert ((c[1] == c[0]) | (c[1] == c[2])).all()                 # ... so the primary is one of the two
    n2 = int((c[0] != c[2]).sum())
    assert n2 == two and n2 / G.size < cap
    u = hs.half(hs.scramble(hs.FINITE, 1))
    p = hs.pair_candidates(G, u, delta)
    assert float((~hs.same(p[0], p[2])).mean()) < cap              # the products are no looser than the SiLU values


def test_windows_are_the_documented_ones():
    assert hs.DELTA_ROWS == 2.0**-21 and hs.DELTA_DECODE == 2.0**-16
    import test_ap_exact_fused_gpu as ef
    assert hs.DELTA_DECODE is ef.DELTA


def test_non_finite_gates_compare_by_class():
    g = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0], dtype=np.float16)
    c = hs.silu_candidates(g, hs.DELTA_DECODE)
    for row in c:
        assert row[0] == np.inf and np.isnan(row[1]) and np.isnan(row[2])
        assert hs.bits(row[3:]).tolist() == [0x0000, 0x8000]
    nan_other_payload = hs.half(np.array([0xFE01], dtype=np.uint16))
    assert hs.same(nan_other_payload, c[1][2:3]).all()
    assert not hs.same(np.float16(0.0), np.float16(-0.0)) and hs.same(np.float16(0.0), np.float16(-0.0), zero_signs=False)
    assert not hs.same(np.float16(np.inf), np.float16(-np.inf))
    # Inf * 0 and a NaN up are NaN outputs
    p = hs.pair_candidates(np.array([np.inf, 1.0], dtype=np.float16), np.array([0.0, np.nan], dtype=np.float16), hs.DELTA_ROWS)
    assert np.isnan(p).all()


def test_fp32_evaluations_of_the_host_libraries():
    import torch
    cand = hs.silu_candidates(G, hs.DELTA_ROWS)
    g32 = G.astype(np.float32)
    t32 = torch.nn.functional.silu(torch.from_numpy(g32.copy())).numpy().astype(np.float16)
    t16 = torch.nn.functional.silu(torch.from_numpy(G.copy())).numpy()
    with np.errstate(over="ignore"):
        n32 = (g32 / (np.float32(1.0) + np.exp(-g32))).astype(np.float16)
    for name, got in (("torch fp32", t32), ("torch fp16", t16), ("numpy fp32", n32)):
        ok, nonprimary = hs.in_candidates(got, cand)
        assert ok.all(), (name, G[~ok][:4])
        if name != "numpy fp32":   # (numpy's vectorised expf differs between builds; torch's lands off fp16(q) at the gate 2^-24 only)
            assert hs.FINITE[nonprimary].tolist() == [1], name


def test_scramble():
    rows = [hs.scramble(hs.PATTERNS, c) for c in range(4)]
    for r in rows:
        assert np.array_equal(np.sort(r), hs.PATTERNS)
    for a in range(4):
        for b in range(a):
            assert (rows[a] != rows[b]).all()
        assert (rows[a] != hs.PATTERNS).mean() > 0.999
    f = hs.scramble_finite(hs.FINITE, 0)
    assert np.array_equal(np.sort(f), hs.FINITE)
    assert (f != np.roll(f, 1)).all()


# ------------------------------------------------------------------------------------------------ the fp8 write rule
@pytest.mark.parametrize("inv", hs.INV_SCALES)
def test_fp8_write_rule_over_every_pattern(inv):
    codes = hs.fp8_codes(ALL, inv)
    assert np.unique(codes).size == 256
    assert codes[0x7C00] == k8.MAX_CODE and codes[0xFC00] == 0xFE
    nan = np.isnan(ALL)
    assert int(nan.sum()) == 2046 and ((codes[nan] & 0x7F) == k8.NAN_CODE).all()
    assert ((codes[~nan] & 0x7F) != k8.NAN_CODE).all()               # nothing else becomes a NaN
    assert hs.fp8_ok(codes, codes, ALL).all()
    tie, lower, upper = hs.fp8_ties(ALL, inv)
    assert (codes[tie] == np.where(lower & 1, upper, lower)[tie]).all()   # the neighbour with the even mantissa
    if inv == 1.0:
        assert int(tie.sum()) == 254                                  # 252 midpoints of two codes, and +-464 (448 | the 480 without a code)
        assert int((tie & (np.abs(ALL.astype(np.float32)) < 448)).sum()) == 252


# ------------------------------------------------------------------------------------------------ selector layers
@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    o.build()
    return o


def test_pair_selector_returns_the_planted_values(oracle):
    K, b = 256, 2
    planted = hs.half(hs.FINITE)
    for lo in range(0, planted.size, 3968):
        v = planted[lo:lo + 3968]
        q, lut, x = hs.pair_selector(v, K, b)
        y = oracle.ap_gemv_f16(x, q, lut, b)[0]
        assert hs.same(y, v, zero_signs=False).all()
        assert (hs.bits(y[v == 0]) == 0).all()                         # -0 arrives as +0


def test_prologue_selector_returns_the_products(oracle):
    K, b = 256, 2
    q, lut = hs.prologue_selector(K, b)
    g = hs.half(hs.FINITE[np.arange(K) * 248 + 5])
    u = hs.prologue_ups(g)
    h = hs.pair_candidates(g, u, 0.0)[1]
    y = oracle.ap_gemv_f16(h, q, lut, b)[0]
    assert hs.same(y, h, zero_signs=False).all()


def test_prologue_products_are_exact_small_dyadics():
    u = hs.prologue_ups(G)
    for delta in (hs.DELTA_ROWS, hs.DELTA_DECODE):
        c = hs.silu_candidates(G, delta).astype(np.float64)
        h = c * u.astype(np.float64)
        assert (h * 2048 == np.round(h * 2048)).all() and (np.abs(h) <= 2.0).all()   # 4096 of them: at most 2^24 units of 2^-11
        assert (h[1] * 1024 == np.round(h[1] * 1024)).all() and (np.abs(h[1]) < 2.0).all()
        assert (hs.pair_candidates(G, u, delta).astype(np.float64) == h).all()       # the fp16 product is exact


# ------------------------------------------------------------------------------------------------ injected faults
def _silu_rejects(got, u, delta):
    ok, _ = hs.in_candidates(got, hs.pair_candidates(ALL, u, delta))
    return int((~ok).sum())


@pytest.mark.parametrize("delta", [hs.DELTA_ROWS, hs.DELTA_DECODE], ids=["rows", "decode"])
@pytest.mark.parametrize("fault", hs.SILU_FAULTS)
def test_silu_faults_are_rejected(fault, delta):
    for row in range(2):
        u = hs.half(hs.scramble(hs.PATTERNS, row))
        assert _silu_rejects(hs.pair_candidates(ALL, u, delta)[1], u, delta) == 0    # the correct vector passes
        assert _silu_rejects(hs.faulty_silu(fault, ALL, u), u, delta) > 0, (fault, row)
    # the prologue's power-of-two ups: the value faults show there too (neighbours_up needs differing ups: rows above)
    if fault != "neighbours_up":
        u = hs.prologue_ups(G)
        ok, _ = hs.in_candidates(hs.faulty_silu(fault, G, u), hs.pair_candidates(G, u, delta), zero_signs=False)
        assert not ok.all() or fault == "no_fp16_silu"   # (one rounding or two: the same value when the up is a power of two)


@pytest.mark.parametrize("inv", hs.INV_SCALES)
@pytest.mark.parametrize("fault", hs.FP8_FAULTS)
def test_fp8_faults_are_rejected(fault, inv):
    want = hs.fp8_codes(ALL, inv)
    bad = ~hs.fp8_ok(hs.faulty_fp8(fault, ALL, inv), want, ALL)
    assert bad.any(), fault
    if fault == "ties_away" and inv == 1.0:
        assert int(bad.sum()) == 252


def test_the_fault_list_is_covered():
    assert set(hs.FAULTS) == set(hs.SILU_FAULTS) | set(hs.FP8_FAULTS) and len(hs.FAULTS) == 9


def test_the_sweeps_reach_their_families():
    """the dry dispatch, without a device: every family whose CASES rows list the form serves the selector shapes of
    tests/test_halfsweep_ap_gpu.py under the knobs that test sets"""
    import os

    import test_bounds_ap_gemv_gpu as t
    import test_halfsweep_ap_gpu as ap
    from guidedquant_amd import _lib
    saved = {k: v for k, v in os.environ.items() if k.startswith("GQ_")}
    try:
        assert set(ap.PAIR_FAMILIES) == set(ap.SILU_FAMILIES) == {"exact", "pair-table", "plane", "plane-local", "stream", "dq", "wide"}
        for fam, (b, K) in ap.PAIR_FAMILIES.items():
            t.set_env(fam)
            assert ap._pair_rows(fam, K, b) == (4096 if fam == "plane-local" else ap.PAIR_ROWS), fam
            assert b == (5 if fam == "wide" else 2)
        for fam, (b, K) in ap.SILU_FAMILIES.items():
            t.set_env(fam)
            for flags in (0, ap.GQ_PRO_SILU_MUL):
                assert _lib.ap_plan_route(K, K, b, 1, False, flags, 0)[:2] == (fam, 1), (fam, flags)
    finally:
        for k in [k for k in os.environ if k.startswith("GQ_")]:
            del os.environ[k]
        os.environ.update(saved)
        _lib.lib().gq_reset_env_cache()
        _lib.lib().gq_set_ap_mode(-1)
