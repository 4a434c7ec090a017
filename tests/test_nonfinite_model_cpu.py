"""CPU: the model of tests/nonfinite_model.py -- the oracle's fp16 scalar ops carry the classes as numpy float16 does, the classifier is
right on all 65 536 patterns, the references ALONE give the intended classes for every input the GPU tests commit to, the dry dispatch
sends every launch of tests/test_nonfinite_ap_gemv_gpu.py to its family, and the checker accepts the reference and rejects every injected
fault (nonfinite_model.FAULTS, "neg_nan_dropped"; the sampler's "nan_wins" and "neg_nan_as_number" are in test_sampler_model_cpu.py)."""
import os

import numpy as np
import pytest

import halfsweep_model as hs
import nonfinite_model as nf
import test_bounds_ap_gemv_gpu as t
from guidedquant_amd import _lib

N, R0 = nf.N_ROWS, 17
SHAPES = nf.family_shapes(t.CASES)
FORMS = {fam: set().union(*[set(c[4]) for c in t.CASES if c[0] == fam]) for fam in SHAPES}
# one pattern (or more) of every class and kind: zeros, subnormals, normals, the largest finite, the infinities, NaNs of either sign and payload
REPS = np.array([0x0000, 0x8000, 0x0001, 0x83FF, 0x3C00, 0xBC00, 0x3555, 0xC400, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x7C01, 0xFDFF], dtype=np.uint16)


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    o.build()
    return o


@pytest.fixture(autouse=True)
def _restore_env():
    saved = {k: v for k, v in os.environ.items() if k.startswith("GQ_")}
    yield
    for k in [k for k in os.environ if k.startswith("GQ_")]:
        del os.environ[k]
    os.environ.update(saved)
    _lib.lib().gq_reset_env_cache()
    _lib.lib().gq_set_ap_mode(-1)


def test_classify_on_every_pattern():
    h = hs.half(hs.PATTERNS)
    c = nf.classify(h)
    f = h.astype(np.float32)
    assert np.array_equal(c == nf.NAN, np.isnan(f)) and np.array_equal(c == nf.PINF, f == np.inf) and np.array_equal(c == nf.NINF, f == -np.inf)
    assert (c == nf.FINITE).sum() == hs.FINITE.size
    assert nf.classify64(np.array([65519.9, 65520.0, -65520.0, 1e300, np.nan])).tolist() == [nf.FINITE, nf.PINF, nf.NINF, nf.PINF, nf.NAN]
    assert all(nf.classify(nf.poison(p)) == (nf.NAN if "nan" in p else nf.PINF if p == "+inf" else nf.NINF) for p in nf.POISONS)


def test_oracle_scalar_ops_carry_the_classes(oracle):
    """h2d / d2h / h_fma (h_add = fma(a, 1, b), h_mul = fma(a, b, -0)) against numpy float16 over every pair of REPS: the same class, and
    the same bits where the result is no NaN"""
    L = oracle.lib()
    for a in REPS:
        ha = hs.half([a])[0]
        d = L.gq_oracle_h2d(int(a))
        assert nf.classify(ha) == nf.classify64(np.array(d)) and (np.isnan(d) or L.gq_oracle_d2h(d) == a)
        for b in REPS:
            hb = hs.half([b])[0]
            with np.errstate(all="ignore"):
                want = {"add": np.float16(np.float32(ha) + np.float32(hb)), "mul": np.float16(np.float32(ha) * np.float32(hb))}
            got = {"add": L.gq_oracle_hfma(int(a), 0x3C00, int(b)), "mul": L.gq_oracle_hfma(int(a), int(b), 0x8000)}
            for op in want:
                g = hs.half([got[op]])[0]
                assert nf.classify(g) == nf.classify(want[op]), (op, hex(a), hex(b))
                assert np.isnan(want[op]) or got[op] == hs.bits(want[op])[0], (op, hex(a), hex(b), hex(got[op]))
    big = L.gq_oracle_hfma(0x7BFF, 0x3C00, 0x7BFF)   # 65504 + 65504
    assert big == 0x7C00 and L.gq_oracle_hfma(0xFBFF, 0x4000, 0x0000) == 0xFC00 and L.gq_oracle_d2h(65519.99) == 0x7BFF


@pytest.mark.parametrize("fam", sorted(SHAPES))
def test_routes_of_the_gpu_cases(fam):
    bits, K = SHAPES[fam]
    t.set_env(fam)
    for form in sorted(FORMS[fam]):
        norm, flags = t.FORMS[form]
        assert _lib.ap_plan_route(N, K, bits, 1, norm, flags, 0)[0] == fam, form
    for M in (2, 3, 4):
        assert (_lib.ap_plan_route(N, K, bits, M, False, 0, 0)[0] == fam) == (fam in nf.BATCH_FAMILIES), M
    if fam in nf.tail_shapes(t.CASES):
        b2, k2 = nf.tail_shapes(t.CASES)[fam]
        assert k2 > 1024 and k2 // 1024 * 1024 <= nf.placements(k2)["tail"] < k2 and _lib.ap_plan_route(N, k2, b2, 1, False, 0, 0)[0] == fam


def _accept_and_reject(ref16, rc, exact, clean=None, input_fault_ref=None):
    """the checker passes the reference itself and rejects every fault that applies to these classes"""
    base = ref16 if clean is None else np.where(clean, ref16, np.float16(1.0))
    assert nf.check(ref16, rc, exact, clean, None if clean is None else base) == ([], 0)
    rejected = set()
    for fault in nf.FAULTS:
        if fault == "neg_nan_dropped" or (fault == "nan_leaks_to_neighbour_row" and (clean is None or not clean.any())):
            continue
        bad_out = nf.faulty(fault, ref16, rc, clean)
        if np.array_equal(hs.bits(bad_out), hs.bits(ref16)):
            continue   # (no element of the class the fault touches)
        assert nf.check(bad_out, rc, exact, clean, None if clean is None else base)[0], fault
        rejected.add(fault)
    return rejected


@pytest.mark.parametrize("fam", sorted(SHAPES))
def test_reference_classes_and_faults_of_the_gemv_inputs(oracle, fam):
    bits, K = SHAPES[fam]
    exact = fam in nf.EXACT_ORDER
    L = nf.layer(N, K, bits)
    q, lut, x = L["q"], L["lut"], L["x"]
    rejected = set()
    # activations: every row of every committed input is non-finite by the reference alone
    jobs = [("plain", tag, xp, None) for tag, xp in nf.poisoned_vectors(x, L["hot"][0])]
    if "norm" in FORMS[fam]:
        jobs += [("norm", tag, xp, L["nw"]) for tag, xp in nf.poisoned_vectors(x, L["hot"][0])]
        jobs += [("norm", "w " + tag, x, wp) for tag, wp in nf.poisoned_vectors(L["nw"])]
    if "silu" in FORMS[fam]:
        gate, up = L["gu"][:K], L["gu"][K:]
        jobs += [("silu", tag, np.concatenate([gp, up]), None) for tag, gp in nf.poisoned_vectors(gate)]
        for pname in ("+inf", "-inf"):
            g2, u2 = gate.copy(), up.copy()
            g2[0], u2[0] = 0, nf.poison(pname)
            jobs.append(("silu", "up " + pname, np.concatenate([g2, u2]), None))
    for form, tag, xp, nw in jobs:
        act = nf.activation(form, xp, nw)
        ref = nf.gemv_ref(oracle, act, q, lut, bits, exact)
        rc = nf.classify(ref)
        assert (rc != nf.FINITE).all(), (form, tag)
        if form == "norm" and "inf@" in tag and not tag.startswith("w "):   # ssq = Inf: scale 0, the Inf element NaN, the rest 0
            assert (nf.classify(act) == nf.NAN).sum() == 1 and (act[nf.classify(act) == nf.FINITE] == 0).all() and (rc == nf.NAN).all()
        rejected |= _accept_and_reject(ref, rc, exact)
        if "-nan" in tag and form == "plain":   # a negative NaN read as a number: the output is finite, and rejected
            dropped = nf.gemv_ref(oracle, nf.drop_negative_nan(xp), q, lut, bits, exact)
            assert (nf.classify(dropped) == nf.FINITE).all() and nf.check(dropped, rc, exact)[0]
            rejected.add("neg_nan_dropped")
    # one lut entry, one residual element: only row R0
    codes = oracle.ap_unpack(q, bits)
    others = np.arange(N) != R0
    clean_ref = nf.gemv_ref(oracle, x, q, lut, bits, exact)
    assert (nf.classify(clean_ref) == nf.FINITE).all()
    for pname in nf.POISONS:
        lp = lut.copy()
        lp[R0, codes[R0, 0]] = nf.poison(pname)
        ref = nf.gemv_ref(oracle, x, q, lp, bits, exact)
        rc = nf.classify(ref)
        assert rc[R0] != nf.FINITE and (rc[others] == nf.FINITE).all()
        rejected |= _accept_and_reject(ref, rc, exact, others)
        rp = L["res"].copy()
        rp[R0] = nf.poison(pname)
        rc = nf.classify(nf.epilogue_ref(clean_ref, rp))
        assert rc[R0] == nf.classify(nf.poison(pname)) and (rc[others] == nf.FINITE).all()
        for row in (R0 - 1, R0):
            lp = lut.copy()
            lp[row, codes[row, 0]] = nf.poison(pname)
            rc = nf.classify(nf.epilogue_ref(nf.gemv_ref(oracle, x, q, lp, bits, exact), pairs=True))
            assert rc[row // 2] != nf.FINITE and (np.delete(rc, row // 2) == nf.FINITE).all()
    assert rejected == set(nf.FAULTS), set(nf.FAULTS) - rejected


@pytest.mark.parametrize("fam", sorted(SHAPES))
def test_overflow_inputs_by_the_reference_alone(oracle, fam):
    bits, K = SHAPES[fam]
    q, lut, x, res, y64 = nf.overflow_layer(oracle, N, K, bits)
    big = np.abs(y64) > 1e5
    assert big.sum() >= N // 2 and (~big).sum() >= N // 2 - 1 and ((np.abs(y64[~big]) > 5.9e4) & (np.abs(y64[~big]) < 6.1e4)).all()
    want = np.where(y64 > 0, nf.PINF, nf.NINF)
    for exact in (True, False):   # the fp16-order reference and the rounded exact product agree on the classes
        ref = nf.gemv_ref(oracle, x, q, lut, bits, exact)
        rc = nf.classify(ref)
        assert np.array_equal(rc[big], want[big]) and (rc[~big] == nf.FINITE).all()
        assert nf.check_overflow(ref[big], y64[big]) == []
        assert nf.check_overflow(nf.faulty("inf_saturated", ref[big], rc[big]), y64[big])
        assert np.array_equal(nf.classify(nf.epilogue_ref(ref, res)), want)
    # every fp32 partial sum is finite: all terms of a row share its sign, so no partial exceeds the row's result
    W = oracle.ap_dequant(q, lut, bits).astype(np.float64)
    assert ((W >= 0).all(axis=1) | (W <= 0).all(axis=1)).all() and (x > 0).all() and np.abs(y64).max() < 1e6
