"""Exact mode (gq_set_ap_mode(1)) of the fused Any-Precision GEMV launches against the reference chain, bit for bit.

The decode step never runs the plain launch: it runs `gq_anyprec_gemv_fused` with the RMSNorm prologue (wqkv, w1w3), the SiLU * up
prologue, the residual epilogue (wo, w2) and the SiLU-pairs epilogue (w1w3), on `ap_gemv.hip::ap_gemv_quad_kernel` (its INREG instance
at rows of 4096 weights) and, at 2 bits with GQ_AP_PT, `ap_gemv_pt2_kernel`.  The default dispatch sends them every matrix below the
plane / dq thresholds as well.  Each form is compared with the reference's separate ops (tests/ap_helpers.py: `rmsnorm_ref`,
`silu_mul_ref`, `half_add`) followed by the order-faithful oracle GEMV (`oracle.ap_gemv_f16`).

Where the reference evaluates a transcendental or a reduction whose last bit the kernel may legitimately place differently (the
fp32 RMSNorm statistic, `__expf` in SiLU), the inputs are chosen so that every rounding point is unambiguous, and each test asserts
that property before comparing; the pairs epilogue, whose SiLU input is a GEMV output, is checked against a per-element candidate set.
"""
import ctypes
import os

import numpy as np
import pytest

from ap_helpers import half_add, rmsnorm_ref, run_fused, silu_mul_ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GQ_EPI_RESIDUAL, GQ_PRO_SILU_MUL, GQ_EPI_SILU_PAIRS = 1, 2, 4
PRO_NONE, PRO_RMSNORM, PRO_SILUMUL = 0, 1, 2
KNOBS = ("GQ_AP_D", "GQ_AP_T", "GQ_AP_BPC", "GQ_AP_INREG", "GQ_AP_PT")
# Relative error allowed to the fp32 SiLU quotient g / (1 + e^-g) on the device.  The kernels use __expf = v_exp_f32(g * log2 e):
# the product's rounding is a relative error of |g| 2^-24 in the power, v_exp_f32 adds about 1 ulp, the add and the division one
# rounding each -- below 2^-19 for |g| <= 32.  DELTA = 2^-16 leaves a factor of 8 to that bound.
DELTA = 2.0**-16
SILU_GATE_MAX = 12.0


@pytest.fixture(autouse=True)
def _exact_mode():
    from guidedquant_amd import _lib
    _lib.check(_lib.lib().gq_set_ap_mode(1), "gq_set_ap_mode")
    yield
    _lib.lib().gq_set_ap_mode(-1)
    for k in KNOBS:
        os.environ.pop(k, None)
    _lib.lib().gq_reset_env_cache()


def _set_env(**kv):
    """set (value) or clear (None) GQ_* knobs, then drop the library's env cache"""
    from guidedquant_amd import _lib
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    _lib.lib().gq_reset_env_cache()


def _plan(N, K, bits, pro, epilogue):
    """gq_debug_exact_plan_ex under the current env: [T, RS, SPB, D, grid, blocks per CU, kernel]"""
    from guidedquant_amd import _lib
    p = (ctypes.c_uint32 * 7)()
    rc = _lib.lib().gq_debug_exact_plan_ex(N, K, bits, pro, epilogue, p)
    assert rc == 0, (N, K, bits, pro, epilogue, rc)
    return tuple(int(v) for v in p)


def _layer(N, K, bits, seed):
    from guidedquant_amd import pack
    rng = np.random.default_rng(seed)
    q = pack.random_planes(N, K, bits, seed=seed)
    lut = np.sort(rng.normal(0, 0.02, (N, 1 << bits)).astype(np.float16), axis=1)
    return q, lut


def _rows(rng, N):
    """every row where N <= 4096; else the first and last row blocks (64 rows: several row steps of every plan) and random rows.
    Closed under (2i, 2i + 1), so that the pairs epilogue can be checked on the same sample."""
    if N <= 4096:
        return np.arange(N)
    r = np.concatenate([np.arange(64), np.arange(N - 64, N), rng.integers(0, N, 160)])
    r = np.concatenate([r & ~1, (r & ~1) + 1])
    return np.unique(r[r < N])


def _eq(got, want, what):
    g, w = np.asarray(got, np.float16).view(np.uint16), np.asarray(want, np.float16).view(np.uint16)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} elements differ, first at {bad[:4]}: {g[bad[:4]]} vs {w[bad[:4]]}"


# ------------------------------------------------------------------------------------------------ inputs with unambiguous rounding
def dyadic_rmsnorm_input(rng, K):
    """x = k / 8 with |k| <= 24 (a few channels at |k| = 24), random fp16 norm weights, and an eps drawn from a short list until the
    normalised values cannot depend on the last bits of the statistic.

    Every x^2 is a multiple of 2^-6 and sum k^2 <= 576 K <= 2^24 for K <= 28672, so every partial sum of squares is an exact fp32
    number: the kernel's fp32 sum equals the reference's in any order.  What is left is the fp32 scale r = rsqrt(mean + eps), which
    the kernel evaluates as 1 / sqrtf(..) and may place an ulp or two away; eps is kept only if fp16(fp32(k / 8 * r')) is the same
    for every |k| present and every fp32 r' within 8 ulp of the reference's r."""
    assert K <= 28672
    k = rng.integers(-24, 25, K)
    k[rng.choice(K, 6, replace=False)] = [24, -24, 24, -24, 23, -23]
    x = (k / 8.0).astype(np.float16)
    assert np.array_equal(x.astype(np.float64) * 8.0, k.astype(np.float64))
    ss = int(np.sum(k.astype(np.int64)**2))
    assert ss <= 2**24, ss                                     # exact fp32 sums (in units of 2^-6)
    nw = (1.0 + 0.25 * rng.normal(0, 1, K)).astype(np.float16)
    mags = (np.unique(np.abs(k)) / 8.0).astype(np.float32)
    for eps in [1e-5, 1e-6, 2e-5, 3e-6, 5e-5, 1e-4, 7e-6, 4e-5]:
        r = np.float32(1.0 / np.sqrt(np.mean(x.astype(np.float32).astype(np.float64)**2) + np.float64(eps)))   # rmsnorm_ref's scale
        rr = (np.array([r], np.float32).view(np.int32) + np.arange(-8, 9, dtype=np.int32)).view(np.float32)
        n16 = (mags[:, None] * rr[None, :]).astype(np.float16)    # fp32 products, one fp16 rounding
        if (n16 == n16[:, :1]).all():
            return x, nw, eps
    raise AssertionError("no eps in the list gives unambiguous normalised values")


def silu_gates(rng, K):
    """random fp16 gates whose SiLU rounds to one fp16 value under a relative perturbation DELTA of the fp32 quotient (redrawn
    otherwise; at most 20 % of draws), and random fp16 up values"""
    g = np.clip(rng.normal(0, 2.5, K), -SILU_GATE_MAX, SILU_GATE_MAX).astype(np.float16)
    redrawn = 0
    for _ in range(50):
        bad = ~_silu_unambiguous(g)
        if not bad.any():
            break
        redrawn += int(bad.sum())
        g[bad] = np.clip(rng.normal(0, 2.5, int(bad.sum())), -SILU_GATE_MAX, SILU_GATE_MAX).astype(np.float16)
    assert _silu_unambiguous(g).all()
    assert redrawn <= 0.2 * K, redrawn
    # the reference's own fp32 evaluation lands on the same fp16 value
    g32 = g.astype(np.float32)
    s_ref = (g32 / (np.float32(1.0) + np.exp(-g32))).astype(np.float16)
    assert np.array_equal(s_ref.view(np.uint16), _silu64(g).astype(np.float16).view(np.uint16))
    up = rng.normal(0, 1, K).astype(np.float16)
    return g, up


def _silu64(g16):
    g = np.asarray(g16, np.float16).astype(np.float64)
    return g / (1.0 + np.exp(-g))


def _silu_unambiguous(g16):
    q = _silu64(g16)
    lo, hi = (q * (1 - DELTA)).astype(np.float16), (q * (1 + DELTA)).astype(np.float16)
    return lo.view(np.uint16) == hi.view(np.uint16)


def check_pairs(out, y, idx, what):
    """out[i] (i in idx) of the SiLU-pairs epilogue against y = the chain's rows: out[i] must be one of fp16(fp16(q') * y[2i + 1]),
    q' = g / (1 + e^-g) perturbed by at most DELTA (relative), g = y[2i].  (y[2i], y[2i + 1] are fp16 values; their product is exact
    in float64, so each candidate is one rounding.)"""
    g, u = y[2 * idx], y[2 * idx + 1].astype(np.float64)
    q = _silu64(g)
    cand = np.stack([((q * f).astype(np.float16).astype(np.float64) * u).astype(np.float16).view(np.uint16) for f in (1 - DELTA, 1.0, 1 + DELTA)])
    o = np.asarray(out[idx], np.float16).view(np.uint16)
    ok = (cand == o[None, :]).any(axis=0)
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} pair outputs outside their candidate sets, first at {idx[~ok][:4]}"
    assert (cand[0] != cand[2]).mean() < 0.2     # (the check is strict: most elements have one candidate)


# ------------------------------------------------------------------------------------------------ 1. every fused form, bit for bit
LLAMA = [(6144, 4096), (28672, 4096), (4096, 14336), (10240, 8192), (3072, 2048), (4096, 11008)]
WIDTHS = [(1000, 2304), (4098, 3584), (4098, 4608), (1000, 5120), (4098, 12288), (1000, 18944)]
RAGGED = [(1000, 4096), (4098, 4096), (4097, 4096), (4097, 4608)]
TINY = [(1000, 128), (4098, 256)]


def _forms(N, K, bits, seed):
    """run every fused form of one layer; return the outputs and the oracle chain of the sampled rows"""
    rng = np.random.default_rng(seed)
    q, lut = _layer(N, K, bits, seed)
    rows = _rows(rng, N)
    qs, ls = np.ascontiguousarray(q[:, rows, :]), lut[rows]
    x, nw, eps = dyadic_rmsnorm_input(rng, K)
    g, up = silu_gates(rng, K)
    res = rng.normal(0, 1, N).astype(np.float16)
    xn = rmsnorm_ref(x, nw, eps)
    xs = silu_mul_ref(g, up)
    gu = np.concatenate([g, up])
    y_n = oracle_gemv(xn, qs, ls, bits)
    y_s = oracle_gemv(xs, qs, ls, bits)
    return dict(q=q, lut=lut, rows=rows, x=x, nw=nw, eps=eps, gu=gu, res=res, xn=xn, y_n=y_n, y_s=y_s)


def oracle_gemv(x, qs, ls, bits):
    from oracle import oracle
    return oracle.ap_gemv_f16(x, qs, ls, bits)[0]


def check_all_forms(N, K, bits, f, tag=""):
    q, lut, rows, res = f["q"], f["lut"], f["rows"], f["res"]
    x, nw, eps, xn, gu = f["x"], f["nw"], f["eps"], f["xn"], f["gu"]
    y_n, y_s = f["y_n"], f["y_s"]
    _eq(run_fused(xn, q, lut, bits)[rows], y_n, f"plain{tag}")
    _eq(run_fused(x, q, lut, bits, norm_weight=nw, eps=eps)[rows], y_n, f"RMSNorm prologue{tag}")
    _eq(run_fused(gu, q, lut, bits, flags=GQ_PRO_SILU_MUL)[rows], y_s, f"SiLU * up prologue{tag}")
    _eq(run_fused(xn, q, lut, bits, residual=res, flags=GQ_EPI_RESIDUAL)[rows], half_add(res[rows], y_n), f"residual epilogue{tag}")
    _eq(run_fused(x, q, lut, bits, norm_weight=nw, eps=eps, residual=res, flags=GQ_EPI_RESIDUAL)[rows], half_add(res[rows], y_n),
        f"RMSNorm + residual{tag}")
    _eq(run_fused(gu, q, lut, bits, residual=res, flags=GQ_PRO_SILU_MUL | GQ_EPI_RESIDUAL)[rows], half_add(res[rows], y_s),
        f"SiLU * up + residual{tag}")
    if N % 2 == 0:
        idx = np.unique(rows // 2)
        assert np.isin(2 * idx + 1, rows).all()
        y_full = np.zeros(N, np.float16)  # (y of the sampled rows, indexed by row)
        y_full[rows] = y_n
        o = run_fused(xn, q, lut, bits, flags=GQ_EPI_SILU_PAIRS, out_elems=N // 2)
        check_pairs(o, y_full, idx, f"pairs{tag}")
        o = run_fused(x, q, lut, bits, norm_weight=nw, eps=eps, flags=GQ_EPI_SILU_PAIRS, out_elems=N // 2)
        check_pairs(o, y_full, idx, f"RMSNorm + pairs{tag}")


@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("N,K", LLAMA + WIDTHS + RAGGED + TINY)
def test_fused_forms_match_the_reference_chain(N, K, bits):
    """RMSNorm prologue, SiLU * up prologue, residual epilogue (alone and after either prologue), SiLU-pairs epilogue (with and
    without RMSNorm): the Llama 8B / 70B / 1B / 7B shapes (6144 x 4096 runs the INREG instance), widths outside Llama's (partial
    last chunks, odd row steps), ragged N, tiny K"""
    f = _forms(N, K, bits, seed=N * 7 + K + bits)
    check_all_forms(N, K, bits, f)


@pytest.mark.parametrize("bits", [2, 3, 4])
def test_rmsnorm_prologue_rereads_items_on_long_rows(bits):
    """520 x 28672 with RMSNorm: K = 28672 is more than 16 x the stager threads' 32-activation items, so items beyond a thread's
    first are read again behind the statistic (ap_exact.h::stage_items); the residual epilogue behind it"""
    N, K = 520, 28672
    rng = np.random.default_rng(bits)
    q, lut = _layer(N, K, bits, seed=bits + 11)
    T = _plan(N, K, bits, PRO_RMSNORM, 0)[0]
    assert 4 * (K // 128) > T // 2, "the launch would not re-read items"  # (half the block's waves stage x)
    x, nw, eps = dyadic_rmsnorm_input(rng, K)
    res = rng.normal(0, 1, N).astype(np.float16)
    y = oracle_gemv(rmsnorm_ref(x, nw, eps), q, lut, bits)
    _eq(run_fused(x, q, lut, bits, norm_weight=nw, eps=eps), y, "RMSNorm")
    _eq(run_fused(x, q, lut, bits, norm_weight=nw, eps=eps, residual=res, flags=GQ_EPI_RESIDUAL), half_add(res, y), "RMSNorm + residual")
    idx = np.arange(N // 2)
    check_pairs(run_fused(x, q, lut, bits, norm_weight=nw, eps=eps, flags=GQ_EPI_SILU_PAIRS, out_elems=N // 2), y, idx, "RMSNorm + pairs")


# ------------------------------------------------------------------------------------------------ 2. every launch configuration
# (N, K, bits, the prologue / epilogue, the knobs swept: those whose every value gives this shape a plan of its own)
SWEEP_CASES = [(28672, 4096, 2, "rmsnorm_pairs", KNOBS), (6144, 4096, 4, "pairs", ("GQ_AP_T", "GQ_AP_INREG")),
               (28672, 4096, 3, "pairs", ("GQ_AP_D", "GQ_AP_T", "GQ_AP_BPC", "GQ_AP_INREG")), (4098, 4608, 3, "rmsnorm_pairs", ("GQ_AP_T", )),
               (22016, 4608, 4, "pairs", ("GQ_AP_D", "GQ_AP_T", "GQ_AP_BPC")), (8192, 11008, 2, "silu_residual", ("GQ_AP_D", "GQ_AP_T", "GQ_AP_BPC", "GQ_AP_PT")),
               (4096, 14336, 4, "rmsnorm_residual", ("GQ_AP_D", "GQ_AP_T"))]


def _sweep_values(knob, K, bits):
    if knob == "GQ_AP_D":
        return [1, 2, 3] if bits == 4 else [1, 2, 3, 4]      # (4 bits: pick_quad_cfg caps the ring at 3)
    if knob == "GQ_AP_T":
        return [t for t in range(64, 513, 64) if t >= K // 128]
    if knob == "GQ_AP_BPC":
        return [1, 2, 3, 8]
    if knob == "GQ_AP_INREG":
        assert K == 4096
        return [0, 1]
    if knob == "GQ_AP_PT":
        assert bits == 2
        return [0, 2]
    raise AssertionError(knob)


_SWEEP_PARAMS = [pytest.param(c[:4], knob, id=f"{c[0]}x{c[1]}-{c[2]}b-{c[3]}-{knob}") for c in SWEEP_CASES for knob in c[4]]


def _form_flags(form):
    pro = PRO_RMSNORM if "rmsnorm" in form else (PRO_SILUMUL if "silu_" in form else PRO_NONE)
    epi = (GQ_EPI_SILU_PAIRS if "pairs" in form else 0) | (GQ_EPI_RESIDUAL if "residual" in form else 0) | (GQ_PRO_SILU_MUL if pro == PRO_SILUMUL else 0)
    return pro, epi


@pytest.mark.parametrize("case,knob", _SWEEP_PARAMS)
def test_every_launch_configuration_gives_the_same_bits(case, knob):
    """one knob at a time over every value the planner accepts: each setting must change the plan the dispatcher makes
    (gq_debug_exact_plan_ex) and leave the output bit-identical to the reference chain"""
    N, K, bits, form = case
    pro, epi = _form_flags(form)
    rng = np.random.default_rng(N + K + bits)
    q, lut = _layer(N, K, bits, seed=N + bits)
    rows = _rows(rng, N)
    qs, ls = np.ascontiguousarray(q[:, rows, :]), lut[rows]
    x, nw, eps = dyadic_rmsnorm_input(rng, K)
    g, up = silu_gates(rng, K)
    res = rng.normal(0, 1, N).astype(np.float16)
    if pro == PRO_RMSNORM:
        xin, y = x, oracle_gemv(rmsnorm_ref(x, nw, eps), qs, ls, bits)
    elif pro == PRO_SILUMUL:
        xin, y = np.concatenate([g, up]), oracle_gemv(silu_mul_ref(g, up), qs, ls, bits)
    else:
        xin, y = x, oracle_gemv(x, qs, ls, bits)
    pairs = bool(epi & GQ_EPI_SILU_PAIRS)
    if pairs:
        y_full = np.zeros(N, np.float16)
        y_full[rows] = y
        idx = np.unique(rows // 2)
    base = {"GQ_AP_D": 1} if knob == "GQ_AP_INREG" else {}
    plans = {}
    for v in _sweep_values(knob, K, bits):
        _set_env(**base, **{knob: v})
        p = _plan(N, K, bits, pro, epi)
        plans[v] = p
        if knob == "GQ_AP_D":
            assert p[3] == v, p
        elif knob == "GQ_AP_T":
            assert p[0] == v, p
        elif knob == "GQ_AP_INREG":
            assert p[6] == v, p
        elif knob == "GQ_AP_PT":
            assert (p[6] == 2) == (v == 2), p
        if pairs:
            assert (p[1] * p[2]) % 2 == 0, p
        out = run_fused(xin, q, lut, bits, norm_weight=nw if pro == PRO_RMSNORM else None, eps=eps, residual=res if epi & GQ_EPI_RESIDUAL else None,
                        flags=epi, out_elems=N // 2 if pairs else None)
        if pairs:
            check_pairs(out, y_full, idx, f"{knob}={v} plan {p}")
        elif epi & GQ_EPI_RESIDUAL:
            _eq(out[rows], half_add(res[rows], y), f"{knob}={v} plan {p}")
        else:
            _eq(out[rows], y, f"{knob}={v} plan {p}")
    assert len(set(plans.values())) == len(plans), plans       # no value left the plan as another value had it


@pytest.mark.parametrize("bits,D", [(2, 1), (2, 2), (2, 3), (2, 4), (4, 1), (4, 2), (4, 3)])
def test_multi_batch_plain_launch_across_ring_depths(oracle, bits, D):
    """M = 2 .. 8 batch rows (grid.y) of the plain launch at every ring depth"""
    from guidedquant_amd import ap_gemv
    N, K = 28672, 4096
    _set_env(GQ_AP_D=D)
    assert _plan(N, K, bits, PRO_NONE, 0)[3] == D
    rng = np.random.default_rng(bits * 10 + D)
    q, lut = _layer(N, K, bits, seed=bits + 5)
    rows = _rows(rng, N)
    qs, ls = np.ascontiguousarray(q[:, rows, :]), lut[rows]
    d = torch.device("cuda:0")
    qt, lt = torch.from_numpy(q).to(d), torch.from_numpy(lut).to(d)
    for M in (2, 5, 8):
        X = rng.normal(0, 1, (M, K)).astype(np.float16)
        out = torch.full((M, 1, N), float("nan"), dtype=torch.float16, device=d)
        ap_gemv.anyprec_gemv(torch.from_numpy(X).to(d).reshape(M, 1, K), out, qt, lt, bits)
        torch.cuda.synchronize()
        got = out.cpu().numpy().reshape(M, N)
        want = oracle.ap_gemv_f16(X, qs, ls, bits)
        _eq(got[:, rows], want, f"M={M} D={D}")


# ------------------------------------------------------------------------------------------------ 3. the default dispatch
@pytest.mark.parametrize("N,K,bits", [(3072, 2048, 2), (3072, 2048, 3), (3072, 2048, 4), (2048, 4096, 4), (2048, 2048, 3), (4096, 2048, 3)])
def test_default_dispatch_small_matrices_are_reference_exact(N, K, bits):
    """matrices below the plane and dq thresholds (ap_dispatch.hip, ap_serve) run the exact kernel in the default mode
    too: Llama-3.2-1B's wqkv, a 4-bit 2048 x 4096, 3-bit matrices under 16 M weights -- every fused form bit-identical to exact mode,
    which is the reference chain"""
    from guidedquant_amd import _lib
    f = _forms(N, K, bits, seed=N + K + bits + 3)
    check_all_forms(N, K, bits, f, " (exact mode)")
    q, lut, res, x, nw, eps, xn, gu = (f[k] for k in ("q", "lut", "res", "x", "nw", "eps", "xn", "gu"))
    launches = [dict(x=xn), dict(x=x, norm_weight=nw), dict(x=gu, flags=GQ_PRO_SILU_MUL), dict(x=xn, residual=res, flags=GQ_EPI_RESIDUAL),
                dict(x=x, norm_weight=nw, residual=res, flags=GQ_EPI_RESIDUAL), dict(x=gu, residual=res, flags=GQ_PRO_SILU_MUL | GQ_EPI_RESIDUAL),
                dict(x=xn, flags=GQ_EPI_SILU_PAIRS, out_elems=N // 2), dict(x=x, norm_weight=nw, flags=GQ_EPI_SILU_PAIRS, out_elems=N // 2)]
    outs = {}
    for mode in (1, -1):
        _lib.check(_lib.lib().gq_set_ap_mode(mode), "gq_set_ap_mode")
        outs[mode] = [run_fused(kw.pop("x"), q, lut, bits, eps=eps, **kw) for kw in (dict(d) for d in launches)]
    for i, (a, b) in enumerate(zip(outs[1], outs[-1])):
        _eq(b, a, f"default vs exact mode, form {i}")


# ------------------------------------------------------------------------------------------------ 4. pairs at odd row steps
@pytest.mark.parametrize("N,K,bits,rms", [(73728, 4608, 4, False), (22016, 4608, 2, False), (22016, 4608, 3, True), (22016, 4608, 4, False),
                                          (4098, 4608, 2, True), (28672, 11008, 2, False), (28672, 11008, 3, True), (28672, 11008, 4, False),
                                          (520, 18944, 3, True), (1000, 11008, 4, True)])
def test_pairs_epilogue_at_odd_row_steps(N, K, bits, rms):
    """rows of 4608 / 11008 / 18944 weights have an odd number of row slots per step (256 threads / 36 quads = 7, 512 / 86 = 5,
    512 / 148 = 3): the planner keeps every block on an even number of rows, so the gate / up pairs never straddle a block, and the
    launch is served (it used to be refused with GQ_ENOTSUP).  Gemma-2-27B's w1w3 (73728 x 4608), 7B-like w1w3 rows."""
    pro = PRO_RMSNORM if rms else PRO_NONE
    p = _plan(N, K, bits, pro, GQ_EPI_SILU_PAIRS)
    assert p[1] % 2 == 1 and p[2] % 2 == 0, p
    rng = np.random.default_rng(N + K + bits)
    q, lut = _layer(N, K, bits, seed=N + K + bits)
    rows = _rows(rng, N)
    qs, ls = np.ascontiguousarray(q[:, rows, :]), lut[rows]
    x, nw, eps = dyadic_rmsnorm_input(rng, K)
    xin = rmsnorm_ref(x, nw, eps) if rms else x
    y = oracle_gemv(xin, qs, ls, bits)
    y_full = np.zeros(N, np.float16)
    y_full[rows] = y
    plain = run_fused(xin, q, lut, bits)
    _eq(plain[rows], y, "plain")
    o = run_fused(x, q, lut, bits, norm_weight=nw if rms else None, eps=eps, flags=GQ_EPI_SILU_PAIRS, out_elems=N // 2)
    check_pairs(o, y_full, np.unique(rows // 2), "pairs")
