"""The host model of the QTIP transform side (tests/qtip_xf_model.py) can be trusted, and can fail: it reproduces the recorded device
digests of tests/golden/qtip_xf_bits.json bit for bit, stays inside the float64 rounding bound at every length and table the GPU test
(tests/test_qtip_xf_exact_gpu.py) uses, agrees with the reference's matmul_hadU / matmul_hadUt vectors, and every injected fault makes
a comparison of that test's shape list fail.  No GPU."""
import glob
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

import qtip_xf_cases as C
import qtip_xf_model as m

HERE = os.path.dirname(os.path.abspath(__file__))
XF_N, XF_KF = C.XF_N, C.XF_KF

# the recorded cases the model reproduces (the others depend on the trellis matvec or on __expf)
REPRODUCED = tuple(
    [f"linear_out M{M} resid{r} parts{p}" for r in (0, 1) for p in (1, 3) for M in (32, 128, 4096)]
    + [f"linear_out_seg Ms{ms} resid{r} parts{p}" for r in (0, 1) for p in (1, 2) for ms in ("128", "1024x256x256")]
    + [f"linear_out_in K{K} parts{p}" for K in (256, 1024) for p in (1, 2)]
    + [f"transform out resid transpose{t}" for t in (0, 1)]
    + [f"transform in {pro} transpose{t}" for pro in ("none", "rmsnorm") for t in (0, 1)])
REPRODUCED_MID = tuple(f"mlp_mid rows parts{p}" for p in (1, 2))  # gate_out and up_out only


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _model_outputs(name):
    """the outputs of one recorded case from the model; the inputs drawn exactly as tests/qtip_xf_cases.py draws them"""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    w = name.split()
    if w[0] in ("linear_out", "linear_out_seg"):
        Ms = [int(s) for s in w[1].lstrip("Ms").split("x")]
        res, parts = w[2] == "resid1", int(w[3][5:])
        ys = [C._sums(rng, parts * M) for M in Ms]
        svs = [C._signs(rng, M, 32.0) for M in Ms]
        rss = [C._f16(rng, M) if res else None for M in Ms]
        fn = m.linear_out if w[0] == "linear_out" else m.linear_out_seg
        return {f"out{i}": fn(ys[i], svs[i], rss[i], M) for i, M in enumerate(Ms)}
    if w[0] == "linear_out_in":
        K, parts = int(w[1][1:]), int(w[2][5:])
        y = C._sums(rng, parts * K)
        sv, resid, nw = C._signs(rng, K, 32.0), C._f16(rng, K), C._normw(rng, K)
        sus = [C._signs(rng, K) for _ in range(3)]
        h, xt = m.linear_out_in(y, sv, resid, nw, sus, K)
        return {"hidden": h, "xt0": xt[0], "xt1": xt[1], "xt2": xt[2]}
    hk, n = m.hadK(XF_KF), XF_N
    if w[0] == "transform" and w[1] == "in":
        x, _, nw, su = C._f16(rng, n), C._f16(rng, n), C._normw(rng, n), C._signs(rng, n)
        return {"out": m.factor_transform_in(x, su, hk, int(w[3][-1]), nw if w[2] == "rmsnorm" else None)}
    if w[0] == "transform":
        y, sv, resid = C._sums(rng, n), C._signs(rng, n, 32.0), C._f16(rng, n)
        return {"out": m.factor_transform_out(y, sv, resid, hk, int(w[3][-1]))}
    assert w[0] == "mlp_mid"
    parts = int(w[2][5:])
    yg, yu = (C._sums(rng, parts * n) for _ in range(2))
    svg, svu, sud = C._signs(rng, n, 32.0), C._signs(rng, n, 32.0), C._signs(rng, n)
    g, u, _, _ = m.mlp_mid(yg, yu, svg, svu, sud, hk)
    return {"gate_out": g, "up_out": u}


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(HERE, "golden", "qtip_xf_bits.json")) as f:
        return json.load(f)["cases"]


def test_the_list_of_reproduced_cases():
    assert len(REPRODUCED) == 30 and len(set(REPRODUCED)) == 30
    assert set(REPRODUCED + REPRODUCED_MID) <= set(C.CASES)


@pytest.mark.parametrize("name", REPRODUCED + REPRODUCED_MID)
def test_model_reproduces_the_recorded_device_digests(recorded, name):
    got = _model_outputs(name)
    if name in REPRODUCED:
        assert set(got) == set(recorded[name]), name
    for k, a in got.items():
        assert _sha(a) == recorded[name][k], (name, k)


# ------------------------------------------------------------------------------------------------ against float64
def _within(got32, want64, absum, d):
    err = np.abs(np.asarray(got32, dtype=np.float64) - want64)
    assert (err <= d * 2.0**-24 * absum).all(), (float(err.max()), float(np.min(d * 2.0**-24 * absum)))


@pytest.mark.parametrize("n", sorted(set(m.HADAMARD_N + m.LINEAR_OUT_M + m.PROLOGUE_K)))
def test_butterflies_against_float64(n):
    x = m.in_sums(m.case_rng("f64", n), 1, n)
    want = m.fwht64(x, n)
    if n > 1:
        _within(m.fwht32(x, n), want, np.abs(x.astype(np.float64)).sum(), m.depth(n))
    else:
        assert m.fwht32(x, n)[0] == x[0]
    if n <= 1024:
        S = m.sylvester(n)
        np.testing.assert_allclose(want, S @ x.astype(np.float64), rtol=0, atol=1e-12 * np.abs(x).sum())
    if n <= 2048:  # the identity through the model is the Sylvester matrix, exactly
        assert (m.hadamard(np.eye(n, dtype=np.float32), n, 1.0) == m.sylvester(n)).all()


@pytest.mark.parametrize("M", m.SEG_M)
def test_segmented_form_against_float64(M):
    x = m.in_sums(m.case_rng("f64 seg", M), 1, M)
    got = m.fwht32(m.seg_combine(x, M), 128)
    _within(got, m.fwht64(x, M), np.abs(x.astype(np.float64)).sum(), m.depth(128, seg=True))


@pytest.mark.parametrize("Kf,P", m.FACTOR_SHAPES)
@pytest.mark.parametrize("transpose", [0, 1])
def test_factor_widths_against_float64(Kf, P, transpose):
    n, hk = Kf * P, m.hadK(Kf)
    x = m.in_sums(m.case_rng("f64 factor", Kf, P), 1, n)
    got = m.factor_product(m.fwht32(x, P).reshape(Kf, P), hk, transpose).reshape(-1)
    _within(got, m.had64(x, hk, P, transpose), np.abs(x.astype(np.float64)).sum(), m.depth(P, Kf))


def test_factor_tables_are_hadamard_and_some_are_not_symmetric():
    nonsym = [Kf for Kf in m.HAD_FACTORS if not (m.hadK(Kf) == m.hadK(Kf).T).all()]
    for Kf in m.HAD_FACTORS:
        hk = m.hadK(Kf).astype(np.int64)
        assert (np.abs(hk) == 1).all() and (hk @ hk.T == Kf * np.eye(Kf, dtype=np.int64)).all()
    assert nonsym, "the transpose flag needs a table that is not symmetric"


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(HERE, "golden", "had_n*.npz"))))
def test_model_against_the_reference_goldens(path):
    g = np.load(path)
    n, Kf = int(g["n"]), int(g["K"])
    for X, Y, Yt in zip(g["X"], g["Y"], g["Yt"]):
        if Kf == 1:
            got = gott = m.hadamard(X, n, n ** -0.5)
        else:
            hk, rows = g["hadK"].astype(np.float32), m.fwht32(X, n // Kf).reshape(Kf, n // Kf)
            got = m.factor_product(rows, hk, 0).reshape(-1) * m.inv_sqrt(n)
            gott = m.factor_product(rows, hk, 1).reshape(-1) * m.inv_sqrt(n)
        np.testing.assert_allclose(got, Y, rtol=2e-5, atol=2e-5)
        np.testing.assert_allclose(gott, Yt, rtol=2e-5, atol=2e-5)


# ------------------------------------------------------------------------------------------------ SiLU * up: the bound's condition
@pytest.mark.parametrize("Kf,P", m.FACTOR_SHAPES)
def test_silumul_inputs_have_few_ambiguous_elements(Kf, P):
    g, u = m.in_gate_up(Kf * P)
    assert m.silumul_share(g, u) <= 1 / 16


@pytest.mark.parametrize("parts", [1, 2])
@pytest.mark.parametrize("Kf", m.HAD_FACTORS)
def test_mlp_mid_inputs_have_few_ambiguous_elements(Kf, parts):
    """gate_out / up_out of the model are what SiLU * up sees inside gq_qtip_mlp_mid (the device's are bit-identical to them)"""
    g, u, _, bound = m.mlp_mid(*m.in_mlp_mid(Kf, parts), m.hadK(Kf))
    assert m.silumul_share(g, u) <= 1 / 16
    assert set(m.MID_KF) <= set(m.HAD_FACTORS) and bound.shape == (64, )


# ------------------------------------------------------------------------------------------------ injected faults
def _bits_differ(a, b):
    return bool((np.ascontiguousarray(a).view(np.uint16) != np.ascontiguousarray(b).view(np.uint16)).any())


def _fault_cases(fault):
    """(label, outputs with the fault, outputs without) over the part of the GPU test's shape list the fault can touch"""
    if fault in ("stage_swapped", "last_of_two_skipped", "parts_descending"):
        for M in m.LINEAR_OUT_M:
            rng = m.case_rng("fault", M)
            y, sv, res = m.in_sums(rng, 4, M), m.in_signs(rng, M, 32.0), m.in_f16(rng, M)
            yield f"linear_out M{M}", m.linear_out(y, sv, res, M, fault), m.linear_out(y, sv, res, M)
    if fault == "no_half_rs":
        for K in m.OUT_IN_K:
            rng = m.case_rng("fault", K)
            y, sv, res, nw = m.in_sums(rng, 1, K), m.in_signs(rng, K, 32.0), m.in_f16(rng, K), m.in_normw(rng, K)
            su = [m.in_signs(rng, K)]
            yield f"linear_out_in K{K}", m.linear_out_in(y, sv, res, nw, su, K, fault=fault)[1][0], m.linear_out_in(y, sv, res, nw, su, K)[1][0]
    if fault in ("factor_transposed", "scale_before_product", "kq_running_sum", "no_half_rs", "stage_swapped"):
        for Kf, P in m.FACTOR_SHAPES[:16]:
            n, hk, rng = Kf * P, m.hadK(Kf), m.case_rng("fault", Kf, P)
            y, sv, res = m.in_sums(rng, 1, n), m.in_signs(rng, n, 32.0), m.in_f16(rng, n)
            x, su, nw = m.in_f16(rng, n), m.in_signs(rng, n), m.in_normw(rng, n)
            yield f"transform out {Kf}x{P}", m.factor_transform_out(y, sv, res, hk, 0, fault), m.factor_transform_out(y, sv, res, hk, 0)
            yield f"transform in rmsnorm {Kf}x{P}", m.factor_transform_in(x, su, hk, 1, nw, fault=fault), m.factor_transform_in(x, su, hk, 1, nw)


@pytest.mark.parametrize("fault", m.FAULTS)
def test_injected_faults_are_rejected(fault):
    hit = [label for label, bad, good in _fault_cases(fault) if _bits_differ(bad, good)]
    assert hit, fault
    if fault == "last_of_two_skipped":  # exactly the lengths whose last pass holds two stages
        assert hit == ["linear_out M32", "linear_out M2048", "linear_out M16384"]
    if fault == "factor_transposed":    # a symmetric table cannot tell
        assert not any(f" {Kf}x" in label for label in hit for Kf in m.HAD_FACTORS if (m.hadK(Kf) == m.hadK(Kf).T).all())


def test_the_fault_list_is_covered():
    assert set(m.FAULTS) == {"stage_swapped", "last_of_two_skipped", "factor_transposed", "scale_before_product", "parts_descending",
                             "no_half_rs", "kq_running_sum"}
