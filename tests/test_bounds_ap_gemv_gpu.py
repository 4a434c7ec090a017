"""GPU: every kernel family of the Any-Precision GEMV (guidedquant_amd/_lib.py::AP_ROUTES) at its smallest ragged shapes, with every
buffer guard-banded and poisoned (tests/guarded.py, ap_helpers.run_fused_guarded / run_gemv_guarded).

Each launch is checked twice: the guards around x, qweight, lut, norm_weight, residual, out, the workspace and the hand-over slots
must be untouched (exact equality), and the result must pass the checker the family already has -- bit identity with
oracle.ap_gemv_f16 behind the reference's element-wise ops for the exact-order families (test_ap_exact_fused_gpu.check_all_forms),
ap_helpers._check_fast for the fast ones.  No tolerance is introduced here.

CASES is data: the shapes were chosen with the dry dispatch (gq_debug_ap_plan_route) as the smallest each family serves --
  * an odd N with N % 16 != 0 and N % 4 != 0 -- one row behind the last full group of 16 -- and an even N with N % 32 != 0 for the
    pair epilogue.  The exact-order families are checked bit for bit, so 17 and 21 do; 114 (57 pairs) for the pair epilogue, so
    that the strictness clause of check_pairs -- fewer than a fifth of the elements may have two candidates -- is not left to
    chance.  The fast families take 113 (7 groups + 1 row) and 114: the normwise clause of _check_fast, ||got - ref|| <= 1.05 ||fp16(exact)
    - ref||, is a statement about many rows -- one output that legitimately rounds the other way than fp16(exact) adds about
    3 ulp^2 to a squared norm of about N ulp^2, which 1.05 covers from N = 30 on and 17 rows do not (seen on an MI355X at
    (N, K) = (17, 256), 4 bits); at 113 rows the clause holds up to three such outputs;
  * the smallest K the family serves (generic 32, exact / wide 128, plane 256, dq 1024, stream 2048, pair-table 4096, the two
    K > 16384 forms 16640 / 18432), and a K with a tail chunk (K % 1024 != 0: 1056, 1280, 4352, 16640) where the family takes one
    (dq serves K % 1024 == 0 and stream K % 2048 == 0 only: no tail chunk exists for them);
tests/test_bounds_ap_routes_cpu.py reproduces every (case, form) -> family entry without a device.

Found with these tests: the stream kernel's residual epilogue dropped residual[N - 1] for odd N (its 64-bit residual fetch is bounded
by N * 2 bytes and the last dword straddles the bound).  Such launches are now declined by the stream kernel's launch and served by
the plane kernels: test_stream_declines_the_residual_epilogue_at_odd_n; the stream cases with an odd N run no residual form.  stream-qkv-rope is not a route
of these entry points (tests/test_qkv_rope_gpu.py guards that launch).
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_ap_exact_fused_gpu as ef  # noqa: E402  (the exact-order checker: check_all_forms, check_pairs, _eq and their inputs)
from ap_helpers import _check_fast, check_nonhot_accuracy, half_add, rmsnorm_ref, run_fused_guarded, run_gemv_guarded, silu_mul_ref  # noqa: E402

EPS = 1e-5
FAST = dict(GQ_PL_MIN_MWEIGHTS=0, GQ_PL_MAX_BITS=4, GQ_DQ=0)   # what ap_helpers._fast() sets
# family -> (gq_set_ap_mode, environment): the knobs the suite already steers the dispatch with
ENV = {
    "exact": (1, {}),
    "pair-table": (1, dict(GQ_AP_PT=2)),
    "generic": (1, dict(GQ_AP_FORCE_GENERIC=1)),
    "wide": (0, {}),
    "plane": (0, dict(FAST, GQ_PL_LOCAL=0, GQ_ST=0)),
    "plane-local": (0, dict(FAST, GQ_PL_LOCAL=1, GQ_ST=0)),
    "plane-chain": (0, dict(FAST, GQ_PL_LOCAL=0, GQ_ST=0)),
    "stream": (0, dict(FAST, GQ_PL_LOCAL=1, GQ_ST=3)),
    "stream-ksplit": (0, dict(FAST, GQ_PL_LOCAL=1)),
    "dq": (0, dict(GQ_DQ=7, GQ_DQ_MIN_MWEIGHTS=0)),
}
# form -> (RMSNorm prologue, GQ_EPI_* / GQ_PRO_* flags) of gq_anyprec_gemv_fused
FORMS = {"plain": (False, 0), "norm": (True, 0), "silu": (False, 2), "resid": (False, 1), "norm+resid": (True, 1), "silu+resid": (False, 3),
         "pairs": (False, 4), "norm+pairs": (True, 4), "ho": (False, 1)}
ALL = ("plain", "norm", "silu", "resid", "norm+resid", "silu+resid", "pairs", "norm+pairs", "ho")   # (pairs: even N only)
NO_NORM = ("plain", "silu", "resid", "silu+resid", "pairs", "ho")
NO_RESID = ("plain", "norm", "silu")   # the stream kernel at an odd N: the residual forms go to the plane kernels
PLAIN = ("plain", "resid", "ho")
BATCH = (2, 3, 5, 8)   # M of gq_anyprec_gemv, where the family serves M > 1

# (family, bits, N, K, forms, batch rows M)
CASES = []
for _b in (2, 3, 4):
    CASES += [("exact", _b, 17, 128, ALL, BATCH), ("exact", _b, 21, 1280, ALL, ()), ("exact", _b, 114, 4352, ALL, BATCH),
              ("exact", _b, 50, 4096, ALL, ())]                      # (K = 4096: the in-register instance of the kernel)
    CASES += [("plane", _b, 113, 256, ALL, BATCH), ("plane", _b, 113, 1280, ALL, ()), ("plane", _b, 114, 4352, ALL, BATCH)]
    CASES += [("plane-local", _b, 113, 256, NO_NORM, ()), ("plane-local", _b, 113, 1280, NO_NORM, ()), ("plane-local", _b, 114, 4352, NO_NORM, ())]
    CASES += [("plane-chain", _b, 113, 16640, PLAIN, (2, )), ("plane-chain", _b, 114, 18432, PLAIN, ())]
    CASES += [("stream", _b, 113, 2048, NO_RESID, ()), ("stream", _b, 113, 4096, NO_RESID, ()), ("stream", _b, 114, 2048, ALL, ())]
    CASES += [("dq", _b, 113, 1024, ALL, ()), ("dq", _b, 113, 2048, ALL, ()), ("dq", _b, 114, 1024, ALL, ())]
CASES += [("pair-table", 2, 17, 4096, ALL, ()), ("pair-table", 2, 114, 16640, ALL, ())]
for _b in (2, 4, 8):
    CASES += [("generic", _b, 17, 32, PLAIN, BATCH), ("generic", _b, 21, 1056, PLAIN, BATCH), ("generic", _b, 18, 96, PLAIN, ())]
for _b in (5, 6, 7, 8):
    CASES += [("wide", _b, 17, 128, ALL, ()), ("wide", _b, 21, 1280, ALL, ()), ("wide", _b, 114, 4352, ALL, ())]
# stream-ksplit (2 bits, with a workspace): (N, K, GQ_ST_KSLICE).  K = 18432 is the smallest K > 16384 it serves (slices of 2048 under
# either setting: 4096 does not divide it); 20480 is the smallest with slices of 4096.  The dry dispatch accepts every N >= 1:
# N = 1 runs only the scalar tail of ap_ksplit_reduce_kernel (guards and finiteness; the envelope needs rows, see above), 113 its vector
# path and the tail.
KSPLIT_CASES = [(1, 18432, 0), (113, 18432, 0), (113, 18432, 2048), (114, 20480, 0), (113, 20480, 2048)]
EXACT_ORDER = ("exact", "pair-table", "generic", "wide")


def case_id(c):
    return f"{c[0]}-b{c[1]}-N{c[2]}-K{c[3]}"


def case_forms(c):
    """the (form, has_norm, flags) launches a case makes: pair forms need an even N"""
    return [(f, ) + FORMS[f] for f in c[4] if c[2] % 2 == 0 or "pairs" not in f]


def set_env(family, **extra):
    from guidedquant_amd import _lib
    mode, env = ENV[family]
    for k in [k for k in os.environ if k.startswith("GQ_")]:
        del os.environ[k]
    for k, v in dict(env, **extra).items():
        os.environ[k] = str(v)
    _lib.lib().gq_reset_env_cache()
    _lib.check(_lib.lib().gq_set_ap_mode(mode), "gq_set_ap_mode")


@pytest.fixture(autouse=True)
def _restore_env():
    from guidedquant_amd import _lib
    saved = {k: v for k, v in os.environ.items() if k.startswith("GQ_")}
    yield
    for k in [k for k in os.environ if k.startswith("GQ_")]:
        del os.environ[k]
    os.environ.update(saved)
    _lib.lib().gq_reset_env_cache()
    _lib.lib().gq_set_ap_mode(-1)


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    o.build()
    return o


def _layer(N, K, bits, seed):
    from guidedquant_amd import pack
    rng = np.random.default_rng(seed)
    return rng, pack.random_planes(N, K, bits, seed=seed), np.sort(rng.normal(0, 0.02, (N, 1 << bits)).astype(np.float16), axis=1)


def _check_ssq(out, ssq):
    """the hand-over slots: all written, their total the sum of squares of the stored fp16 values (tests/test_handover_gpu.py)"""
    want = (out.astype(np.float64)**2).sum()
    assert np.isfinite(ssq).all() and abs(ssq.astype(np.float64).sum() - want) <= 1e-5 * want


def _check_chain_residual(got, x, res, q, lut, bits, oracle):
    """the two-launch K split with a residual (tests/test_ap_fused_gpu.py::test_residual_epilogue_two_launch_k_split):
    out = fp16(fp16(resid + fp16(y1)) + fp16(y2)), four roundings, each <= 2^-11 of the value rounded"""
    K = x.size
    k1 = ((K // 2 + 1023) // 1024) * 1024
    y1 = oracle.ap_gemv_f64(x[:k1], np.ascontiguousarray(q[:, :, :k1 // 32]), lut, bits)[0]
    y2 = oracle.ap_gemv_f64(x[k1:], np.ascontiguousarray(q[:, :, k1 // 32:]), lut, bits)[0]
    r = res.astype(np.float64)
    scale = np.abs(oracle.ap_dequant(q, lut, bits).astype(np.float64)) @ np.abs(x.astype(np.float64))
    tol = 2.0**-11 * 1.002 * (np.abs(y1) + np.abs(y2) + np.abs(r + y1) + np.abs(r + y1 + y2)) + 1e-5 * scale + 1e-7
    assert (np.abs(got.astype(np.float64) - (r + y1 + y2)) <= tol).all()


def _exact_order_case(oracle, monkeypatch, fam, bits, N, K, forms, batch):
    seed = 1000 * bits + N + K
    run = lambda *a, **k: run_fused_guarded(*a, expect=fam, **k)  # noqa: E731
    if "norm" in forms:
        monkeypatch.setattr(ef, "run_fused", run)   # (check_all_forms launches through the module's run_fused)
        f = ef._forms(N, K, bits, seed)
        assert f["rows"].size == N
        ef.check_all_forms(N, K, bits, f, tag=f" [{fam}]")
        q, lut, x, res = f["q"], f["lut"], f["xn"], f["res"]
    else:
        rng, q, lut = _layer(N, K, bits, seed)
        x, res = rng.normal(0, 1, K).astype(np.float16), rng.normal(0, 1, N).astype(np.float16)
        want = oracle.ap_gemv_f16(x, q, lut, bits)[0]
        ef._eq(run(x, q, lut, bits), want, "plain")
        ef._eq(run(x, q, lut, bits, residual=res, flags=1), half_add(res, want), "residual epilogue")
    if "ho" in forms:
        want = half_add(res, oracle.ap_gemv_f16(x, q, lut, bits)[0])
        out, ssq = run(x, q, lut, bits, residual=res, flags=1, want_ssq=True)
        ef._eq(out, want, "residual epilogue with the hand-over statistics")
        _check_ssq(out, ssq)
    if batch:
        X = np.random.default_rng(seed + 1).normal(0, 1, (max(batch), K)).astype(np.float16)
        want = oracle.ap_gemv_f16(X, q, lut, bits)
        for M in batch:
            ef._eq(run_gemv_guarded(X[:M], q, lut, bits, expect=fam), want[:M], f"M = {M}")


def _fast_case(oracle, fam, bits, N, K, forms, batch, workspace=False, nround=None, envelope=True):
    rng, q, lut = _layer(N, K, bits, 1000 * bits + N + K)
    run = lambda *a, **k: run_fused_guarded(*a, expect=fam, workspace=workspace, **k)  # noqa: E731
    x = rng.normal(0, 1, K)
    hot = rng.choice(K, 4, replace=False)
    x[hot] *= 30.0
    x = x.astype(np.float16)
    res = rng.normal(0, 1, N).astype(np.float16)
    nw = (1 + 0.1 * rng.normal(0, 1, K)).astype(np.float16)
    gu = rng.normal(0, 1.5, 2 * K).astype(np.float16)
    got = run(x, q, lut, bits)
    assert np.isfinite(got.astype(np.float32)).all()
    if envelope:
        _check_fast(got, x, q, lut, bits, oracle, nround=nround)
    else:   # a single row: the accuracy criterion of the K-split tests (ap_helpers.check_nonhot_accuracy), which needs no population
        check_nonhot_accuracy(got, x, hot, q, lut, bits, oracle, nround=nround)
    idx = np.arange(N // 2)
    if "resid" in forms:
        got_r = run(x, q, lut, bits, residual=res, flags=1)
        if fam == "plane-chain":
            _check_chain_residual(got_r, x, res, q, lut, bits, oracle)
        else:   # one fp16 add behind the fp16-rounded sums (model.py:311-313): bit-identical to the two ops
            assert np.array_equal(got_r.view(np.uint16), half_add(res, got).view(np.uint16))
    if "ho" in forms:
        out, ssq = run(x, q, lut, bits, residual=res, flags=1, want_ssq=True)
        assert np.array_equal(out.view(np.uint16), got_r.view(np.uint16))   # the request for the statistics changes no output
        _check_ssq(out, ssq)
    if "norm" in forms:
        got_n = run(x, q, lut, bits, norm_weight=nw, eps=EPS)
        _check_fast(got_n, rmsnorm_ref(x, nw, EPS), q, lut, bits, oracle, nround=nround)
        if "norm+resid" in forms:
            both = run(x, q, lut, bits, norm_weight=nw, eps=EPS, residual=res, flags=1)
            assert np.array_equal(both.view(np.uint16), half_add(res, got_n).view(np.uint16))
        if "norm+pairs" in forms and N % 2 == 0:
            o = run(x, q, lut, bits, norm_weight=nw, eps=EPS, flags=4, out_elems=N // 2)
            ef.check_pairs(o, got_n, idx, "RMSNorm + pairs")
    if "silu" in forms:
        got_s = run(gu, q, lut, bits, flags=2)
        _check_fast(got_s, silu_mul_ref(gu[:K], gu[K:]), q, lut, bits, oracle, nround=nround)
        if "silu+resid" in forms:
            both = run(gu, q, lut, bits, residual=res, flags=3)
            assert np.array_equal(both.view(np.uint16), half_add(res, got_s).view(np.uint16))
    if "pairs" in forms and N % 2 == 0:
        o = run(x, q, lut, bits, flags=4, out_elems=N // 2)
        ef.check_pairs(o, got, idx, "pairs")
    if batch:
        X = rng.normal(0, 1, (max(batch), K)).astype(np.float16)
        for M in batch:
            out = run_gemv_guarded(X[:M], q, lut, bits, expect=fam)
            for m in range(M):
                _check_fast(out[m], X[m], q, lut, bits, oracle, nround=nround)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_guarded_family(oracle, monkeypatch, case):
    fam, bits, N, K, forms, batch = case
    set_env(fam)
    if fam in EXACT_ORDER:
        _exact_order_case(oracle, monkeypatch, fam, bits, N, K, forms, batch)
    else:
        _fast_case(oracle, fam, bits, N, K, forms, batch)


@pytest.mark.parametrize("N,K,kslice", KSPLIT_CASES)
def test_guarded_stream_ksplit(oracle, N, K, kslice):
    """K split over blocks: the workspace has exactly gq_anyprec_gemv_fused_ws_bytes bytes, poisoned, a guard directly behind it; the
    slices meet in fp32 and are rounded once (nround = 1).  No N here is a multiple of 4: each runs the scalar tail of
    ap_ksplit_reduce_kernel (N = 1 nothing else)."""
    from guidedquant_amd import _lib
    set_env("stream-ksplit", GQ_ST_KSLICE=kslice)
    slice_ = 4096 if (kslice == 0 and K % 4096 == 0) else 2048
    assert _lib.lib().gq_anyprec_gemv_fused_ws_bytes(N, K, 2, 1) == (K // slice_) * N * 4
    _fast_case(oracle, "stream-ksplit", 2, N, K, PLAIN, (), workspace=True, nround=1.0, envelope=N >= 30)


@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("N,K", [(113, 2048), (115, 4096)])
def test_stream_declines_the_residual_epilogue_at_odd_n(oracle, bits, N, K):
    """the finding of this file: with GQ_ST=3 every launch the stream kernel serves goes to it -- except a residual epilogue at an odd
    N, whose last residual element its 64-bit fetch would read as zero.  The plane kernel serves that launch, and every element gets
    its residual: one fp16 add behind that kernel's own plain result (GQ_ST=0), bit for bit."""
    from guidedquant_amd import _lib
    rng, q, lut = _layer(N, K, bits, 7 * bits + N + K)
    x, res = rng.normal(0, 1, K).astype(np.float16), rng.normal(0, 1, N).astype(np.float16)
    assert res[N - 1] != 0
    set_env("stream")
    _check_fast(run_fused_guarded(x, q, lut, bits, expect="stream"), x, q, lut, bits, oracle)
    fam = _lib.ap_plan_route(N, K, bits, 1, False, 1, 0)[0]
    assert fam in ("plane", "plane-local")
    got = run_fused_guarded(x, q, lut, bits, residual=res, flags=1, expect=fam)
    set_env("stream", GQ_ST=0)
    base = run_fused_guarded(x, q, lut, bits, expect=fam)
    _check_fast(base, x, q, lut, bits, oracle)
    assert np.array_equal(got.view(np.uint16), half_add(res, base).view(np.uint16))
