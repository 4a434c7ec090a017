"""Host model of NaN / Inf propagation (tests/test_nonfinite_*_gpu.py): what a kernel must return when an operand is not finite, and when
a finite result lies beyond fp16.  numpy and the CPU oracle only: no GPU.  Like tests/halfsweep_model.py it restates the CONTRACT.

The reference of an operation is its existing float64 / oracle reference evaluated with IEEE semantics: NaN op x = NaN, Inf - Inf = NaN,
0 * Inf = NaN, a finite sum beyond 65 520 rounds to Inf with its sign.  oracle/gq_oracle.c h2d / d2h / h_add / h_mul / h_fma carry the
classes (tests/test_nonfinite_model_cpu.py compares them with numpy float16 over every pair of classes).  Every output has a class,
FINITE, PINF, NINF or NAN (`classify`), and `check` holds a kernel's output against the reference's classes:

  R1  no hiding     reference not finite -> output not finite.  No exception, no share left out.
  R2  no spreading  an output whose inputs, by the operation's definition, hold no non-finite value (`clean`) is bit-identical to the
                    same launch with the non-finite values replaced by finite ones (`baseline`).
  R3  class         exact = True (the kernels that follow the reference's fp16 order: exact, pair-table, generic, wide, dense GEMV,
                    LUT-GEMM, rows kernels): the class equals the reference's everywhere, NaN by class and not by payload.
                    exact = False (fp32-accumulating and matrix-core kernels): where the reference says +-Inf the output is that Inf or
                    NaN (`nan_for_inf` counts those); the opposite sign or a finite value is not accepted.  Where it says NaN, R1 holds.
  overflow          `check_overflow`: finite operands, 1e5 <= |y64| <= 1e6: the output is Inf with the sign of y64, never +-65504.

What the references give for the forms of the fused GEMV (ap_helpers restates the element-wise ops; they are IEEE as they stand):
  RMSNorm   a NaN in x: ssq is NaN, every element NaN.  An Inf in x: ssq = Inf, the scale 1 / sqrt(Inf) = 0, the Inf element 0 * Inf = NaN and
            every other element 0; behind the GEMV every row is NaN.  A non-finite norm weight poisons its own element.
  SiLU * up g / (1 + e^-g) as halfsweep_model.silu64: NaN -> NaN, +Inf -> +Inf, -Inf -> -Inf / Inf = NaN; an Inf up over a zero gate is NaN.
  residual  fp16(res + y): only the element's own row.
  pairs     out[i] = silu(y[2 i]) * y[2 i + 1]: only the pair of a poisoned row.

`FAULTS` are deviations `faulty` injects into a correct output, for tests/test_nonfinite_model_cpu.py only.  One fault of the list this
model was written to is NOT here: "a NaN logit that wins the draw" is no deviation of an output array but of a draw, so it lives in
tests/sampler_model.py (NAN_FAULTS: `nan_wins`, modelled as "the lowest NaN id among the candidates is published", and
`neg_nan_as_number`) and is shown to be caught by tests/test_sampler_model_cpu.py, not by `check`.
"""
import numpy as np

import halfsweep_model as hs
from ap_helpers import half_add, rmsnorm_ref, silu_mul_ref

FINITE, PINF, NINF, NAN = 0, 1, 2, 3
CLASS_NAMES = ("FINITE", "+INF", "-INF", "NAN")
# 0x7C01: a NaN whose payload lies in the low byte only -- the bf8 split h & 0xFF00 turns it into +Inf
POISONS = {"+nan": 0x7E00, "-nan": 0xFE00, "nan_lo": 0x7C01, "+inf": 0x7C00, "-inf": 0xFC00}
SENTINEL = 0x3C00   # what out and the workspaces hold before a launch: finite, so that a skipped store is no propagated NaN
EPS = 1e-5
EXACT_ORDER = ("exact", "pair-table", "generic", "wide")   # reference: the order-faithful fp16 oracle
CLASS_EXACT = EXACT_ORDER + ("dq", )   # checked with exact = True; dq (fp32 sums of fp16 weights) against the rounded float64 product
BATCH_FAMILIES = ("exact", "generic", "pair-table", "plane", "plane-chain")   # the families that serve M > 1 at N_ROWS rows (dry dispatch)
N_ROWS = 34        # two groups of 16 rows and two more: even (pairs), no multiple of 4 * 8 or 16
FAULTS = ("nan_as_0", "nan_as_-65504", "nan_as_-448", "inf_saturated", "nan_leaks_to_neighbour_row", "neg_nan_dropped")


def poison(name):
    return hs.half(np.array([POISONS[name]], dtype=np.uint16))[0]


def classify(h16):
    """class of every fp16 element"""
    b = hs.bits(h16).reshape(np.shape(h16))
    exp_all, man = (b & 0x7C00) == 0x7C00, (b & 0x03FF) != 0
    out = np.zeros(b.shape, dtype=np.uint8)
    out[exp_all & ~man & (b < 0x8000)] = PINF
    out[exp_all & ~man & (b >= 0x8000)] = NINF
    out[exp_all & man] = NAN
    return out


def classify64(y64):
    """class of fp16(y64), one rounding to nearest even"""
    return classify(hs.to_half(y64))


def check(got16, ref_class, exact, clean=None, baseline=None):
    """-> (violations: list of str, nan_for_inf: int).  got16 and ref_class have one shape; clean (bool) and baseline (fp16) belong together."""
    got16 = np.asarray(got16, dtype=np.float16)
    ref_class = np.asarray(ref_class, dtype=np.uint8)
    assert got16.shape == ref_class.shape
    gc = classify(got16)
    bad = []

    def report(rule, mask):
        idx = np.argwhere(mask)
        if idx.size:
            first = tuple(int(v) for v in idx[0])
            bad.append("%s: %d element(s), first %s: reference %s, got %s" % (rule, len(idx), first, CLASS_NAMES[ref_class[first]],
                                                                                hex(int(hs.bits(got16).reshape(got16.shape)[first]))))
    report("R1 hidden", (ref_class != FINITE) & (gc == FINITE))
    if clean is not None:
        clean = np.asarray(clean, dtype=bool)
        base = np.asarray(baseline, dtype=np.float16)
        assert clean.shape == got16.shape == base.shape and (ref_class[clean] == FINITE).all()
        report("R2 spread", clean & (hs.bits(got16).reshape(got16.shape) != hs.bits(base).reshape(base.shape)))
    inf = (ref_class == PINF) | (ref_class == NINF)
    sub = inf & (gc == NAN)
    if exact:
        report("R3 class", (gc != ref_class) & ~((ref_class != FINITE) & (gc == FINITE)))
    else:
        report("R3 class", inf & (gc != ref_class) & (gc != NAN) & (gc != FINITE))
    return bad, int(sub.sum())


def check_overflow(got16, y64):
    """finite operands whose exact result is far beyond fp16: Inf with the sign of y64 -> list of violations"""
    y64 = np.asarray(y64, dtype=np.float64)
    assert ((np.abs(y64) >= 1e5) & (np.abs(y64) <= 1e6)).all()
    want = np.where(y64 > 0, PINF, NINF).astype(np.uint8)
    gc = classify(got16)
    idx = np.flatnonzero(gc != want)
    if not idx.size:
        return []
    return ["overflow: %d element(s), first %d: y64 = %r, got %s" % (idx.size, idx[0], float(y64[idx[0]]), hex(int(hs.bits(got16)[idx[0]])))]


# ------------------------------------------------------------------------------------------------ where the poison goes
def placements(K, hot=None):
    """name -> index: element 0, element K - 1, one element of the tail chunk (K % 1024 != 0), and the neighbour of a hot channel in its
    group of 128 (the MFMA group of the plane and stream kernels)"""
    out = {"first": 0, "last": K - 1}
    if K % 1024:
        lo = K // 1024 * 1024
        out["tail"] = lo + (K - lo) // 2
    if hot is not None and K > 1:
        g = int(hot) // 128 * 128
        out["hot_group"] = g + (int(hot) - g + 1) % min(128, K - g)
    return out


def poisoned_vectors(x16, hot=None):
    """(tag, vector) for every poison at every placement, a +Inf and a -Inf together, and the whole vector NaN"""
    x16 = np.asarray(x16, dtype=np.float16)
    K = x16.size
    for pname in POISONS:
        for where, i in placements(K, hot).items():
            v = x16.copy()
            v[i] = poison(pname)
            yield f"{pname}@{where}", v
    v = x16.copy()
    v[0], v[K - 1] = poison("+inf"), poison("-inf")
    yield "+inf&-inf", v
    yield "all_nan", np.full(K, poison("+nan"), dtype=np.float16)


# ------------------------------------------------------------------------------------------------ the fused GEMV's references
def activation(form, x16, norm_weight=None):
    """the vector the GEMV consumes behind the prologue of `form` ("plain", "norm", "silu": x = [gate | up])"""
    x16 = np.asarray(x16, dtype=np.float16)
    with np.errstate(all="ignore"):
        if form == "norm":
            return rmsnorm_ref(x16, norm_weight, EPS)
        if form == "silu":
            K = x16.size // 2
            return silu_mul_ref(x16[:K], x16[K:])
    return x16


def gemv_ref(oracle, act16, q, lut, bits, exact):
    """fp16 [N]: the reference GEMV -- the order-faithful fp16 one for the exact-order families, fp16(float64 product) for the others"""
    with np.errstate(all="ignore"):
        if exact:
            return oracle.ap_gemv_f16(act16, q, lut, bits)[0]
        return hs.to_half(oracle.ap_gemv_f64(act16, q, lut, bits)[0])


def epilogue_ref(y16, residual=None, pairs=False):
    with np.errstate(all="ignore"):
        if pairs:
            return hs.pair_candidates(y16[0::2], y16[1::2], 0.0)[1]
        return y16 if residual is None else half_add(residual, y16)


# ------------------------------------------------------------------------------------------------ the committed inputs
def family_shapes(cases, form="plain"):
    """family -> (bits, K): the lowest bit width and the smallest K among the rows of test_bounds_ap_gemv_gpu.CASES that list `form`"""
    out = {}
    for fam, bits, _, K, forms, _ in cases:
        if form in forms:
            b0, k0 = out.get(fam, (bits, K))
            out[fam] = (min(b0, bits), min(k0, K))
    return out


def tail_shapes(cases):
    """family -> (bits, K): the smallest K > 1024 with K % 1024 != 0 among the family's rows (a tail chunk behind full chunks of 1024), at
    the lowest bit width; families without such a row (stream, dq: whole chunks only) are left out"""
    out = {}
    for fam, bits, _, K, _, _ in cases:
        if K > 1024 and K % 1024:
            b0, k0 = out.get(fam, (bits, K))
            out[fam] = (min(b0, bits), min(k0, K))
    return out


def layer(N, K, bits, seed=0):
    """(rng, qweight, lut, x, hot, residual, norm weight, [gate | up]): a finite layer with two hot channels (30 x) that the plane and
    stream kernels extract; no lut entry is zero"""
    from guidedquant_amd import pack
    rng = np.random.default_rng(9000 + 100 * bits + N + K + seed)
    q = pack.random_planes(N, K, bits, seed=seed + K)
    lut = np.sort(rng.normal(0, 0.02, (N, 1 << bits)).astype(np.float16), axis=1)
    lut[lut == 0] = np.float16(0.01)
    x = rng.normal(0, 1, K)
    hot = rng.choice(K, 2, replace=False)
    x[hot] *= 30.0
    x = x.astype(np.float16)
    x[x == 0] = np.float16(0.5)
    res = rng.normal(0, 1, N).astype(np.float16)
    nw = (1 + 0.1 * rng.normal(0, 1, K)).astype(np.float16)
    gu = rng.normal(0, 1.5, 2 * K).astype(np.float16)
    return dict(rng=rng, q=q, lut=lut, x=x, hot=hot, res=res, nw=nw, gu=gu)


BIG, NEAR, PUSH = 3.0e5, 6.0e4, 8192.0


def overflow_layer(oracle, N, K, bits, seed=0):
    """finite operands with results beyond fp16.  Every weight of a row has the row's sign and x > 0, so that every partial sum, in any
    order and any precision, lies between 0 and the row's result: no fp32 partial overflows.  Row r: r % 4 == 0 -> +BIG, 1 -> -BIG (the
    exact result, to 2^-10), 2 -> +NEAR, 3 -> -NEAR: below 65 504 alone, and beyond 65 520 with the residual +-PUSH of the same sign.
    -> (qweight, lut, x, residual, y64)"""
    from guidedquant_amd import pack
    rng = np.random.default_rng(77 + bits + K)
    q = pack.random_planes(N, K, bits, seed=seed + K + 1)
    x = rng.uniform(0.5, 1.5, K).astype(np.float16)
    lut = rng.uniform(1.0, 2.0, (N, 1 << bits)).astype(np.float16)
    r = np.arange(N)
    sign = np.where(r % 2 == 0, 1.0, -1.0)
    target = np.where(r % 4 < 2, BIG, NEAR) * sign
    for _ in range(2):   # (the second pass takes out the rounding of the first scaling)
        y = oracle.ap_gemv_f64(x, q, lut, bits)[0]
        lut = (lut.astype(np.float64) * (target / y)[:, None]).astype(np.float16)
    y64 = oracle.ap_gemv_f64(x, q, lut, bits)[0]
    assert np.isfinite(lut.astype(np.float32)).all() and (np.abs(y64 / target - 1) < 2.0**-9).all()
    res = (sign * PUSH).astype(np.float16)
    return q, lut, x, res, y64


# ------------------------------------------------------------------------------------------------ injected faults
def faulty(fault, got16, ref_class, clean=None):
    """a correct output (one that passes `check`) with one deviation"""
    out = np.array(got16, dtype=np.float16, copy=True)
    b = out.view(np.uint16)
    if fault == "nan_as_0":
        b[ref_class == NAN] = 0
    elif fault == "nan_as_-65504":   # what v_med3(x, -max, max) returns for a NaN x
        b[ref_class == NAN] = 0xFBFF
    elif fault == "nan_as_-448":     # the same clamp at the fp8 range (-448 = 0xDF00 as fp16)
        b[ref_class == NAN] = 0xDF00
    elif fault == "inf_saturated":
        b[ref_class == PINF] = 0x7BFF
        b[ref_class == NINF] = 0xFBFF
    elif fault == "nan_leaks_to_neighbour_row":
        rows = np.flatnonzero(clean)
        assert rows.size
        b[rows[0]] = 0x7E00
    else:
        raise AssertionError(fault)
    return out


def drop_negative_nan(x16):
    """the input fault "neg_nan_dropped": a kernel that tells NaN by `bits > 0x7C00` on the SIGNED pattern reads -NaN as a number (here 0)"""
    out = np.array(x16, dtype=np.float16, copy=True)
    b = out.view(np.uint16)
    b[(b & 0x8000 != 0) & (classify(out) == NAN)] = 0
    return out


# ------------------------------------------------------------------------------------------------ the scoring head, the dense GEMV, the rows RMSNorm
def classify32(a):
    """class of every fp32 / float64 element (no rounding)"""
    a = np.asarray(a, dtype=np.float64)
    out = np.zeros(a.shape, dtype=np.uint8)
    out[a == np.inf], out[a == -np.inf], out[np.isnan(a)] = PINF, NINF, NAN
    return out


def head_ref(logits64, target):
    """(lse, logprob) of head_nll_model.model with IEEE semantics: a NaN logit makes the row's lse NaN, a +Inf logit makes it +Inf, a -Inf
    logit adds exp(-Inf) = 0; logprob = logit[target] - lse, so Inf - Inf = NaN and a -Inf target logit under a finite lse is -Inf"""
    x = np.asarray(logits64, dtype=np.float64)
    with np.errstate(all="ignore"):
        m = np.where(np.isfinite(x), x, -np.inf).max(axis=1)
        m = np.where(np.isfinite(m), m, 0.0)
        lse = m + np.log(np.exp(x - m[:, None]).sum(axis=1))   # (exp(+Inf) = Inf, exp(NaN) = NaN, exp(-Inf) = 0: numpy's sum carries them)
        t = np.asarray(target).astype(np.int64)
        lp = np.where(t >= 0, x[np.arange(x.shape[0]), np.maximum(t, 0)] - lse, 0.0)
    return lse, lp


def check32(got, ref, clean=None, baseline=None):
    """`check` for fp32 outputs of fp32-accumulating kernels (exact = False) -> (violations, nan_for_inf)"""
    got, rc = np.asarray(got, dtype=np.float32), classify32(ref)
    gc = classify32(got)
    bad = []
    hidden = (rc != FINITE) & (gc == FINITE)
    if hidden.any():
        i = int(np.flatnonzero(hidden)[0])
        bad.append("R1 hidden: %d element(s), first %d: reference %s, got %r" % (hidden.sum(), i, CLASS_NAMES[rc.reshape(-1)[i]], float(got.reshape(-1)[i])))
    if clean is not None:
        spread = np.asarray(clean, dtype=bool) & (got.view(np.uint32) != np.asarray(baseline, dtype=np.float32).view(np.uint32))
        if spread.any():
            bad.append("R2 spread: %d element(s), first %d" % (spread.sum(), int(np.flatnonzero(spread)[0])))
    inf = (rc == PINF) | (rc == NINF)
    wrong = inf & (gc != rc) & (gc != NAN) & (gc != FINITE)
    if wrong.any():
        bad.append("R3 class: %d element(s) with the opposite infinity" % wrong.sum())
    return bad, int((inf & (gc == NAN)).sum())


def rmsnorm_rows_ref(x16, delta16, w16):
    """(x + delta written back, out) of gq_rmsnorm_rows, row by row with ap_helpers' roundings"""
    with np.errstate(all="ignore"):
        xs = x16 if delta16 is None else half_add(x16, delta16)
        return xs, np.stack([rmsnorm_ref(r, w16, EPS) for r in xs])
