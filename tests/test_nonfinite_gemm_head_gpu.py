"""GPU: NaN and Inf through the prompt GEMMs (ap_gemm_kernel, ap_gemm_pipe_kernel, ap_gemm_wide_kernel, the split-K gemm_reduce_kernel;
the GEMV's ap_ksplit_reduce_kernel is in tests/test_nonfinite_ap_gemv_gpu.py), the scoring head (head_nll_kernel + head_nll_merge_kernel), the dense lm_head GEMV (dense_gemv_kernel, with and
without the RMSNorm prologue) and the rows RMSNorm (rmsnorm_rows_kernel), against tests/nonfinite_model.py (R1 no hiding, R2 no spreading,
R3 class).  S covers one row, one full group of 16 and one more, and two and one more: S in {1, 17, 33}.  Outputs start from finite
values (fp16 1.0; the 8.4e37 the guarded fp32 buffers of the head are poisoned with), never from NaN.

head        V = 300 (two tiles and a ragged third), D = 64, the launch's own split and splits = 2.
            one token row poisoned (every poison, first and last column): its lse / logprob are not finite, every other row's logprob,
            lse and top1 are bit-identical to the clean launch;
            one lm_head row poisoned: a NaN makes EVERY lse and logprob NaN; a +-Inf entry makes column v0 +Inf or -Inf row by row --
            +Inf: lse = +Inf and a clean target's logprob -Inf (NaN accepted for either: Inf - Inf inside an online softmax); -Inf: the
            column adds 0, lse and a clean target's logprob are the model's without it (2 ulp16 of the largest logit, the bound of
            test_head_nll_gpu.py's round-off family), and the target v0 itself scores -Inf.
            FOUND here: a target whose logit is -Inf scored -1e30 (the finite stand-in NEG was the neutral element of the target's
            fmaxf fold); it is -Inf now, finite results unchanged.
dense GEMV  (N, K) = (33, 512): x poisoned (nonfinite_model.poisoned_vectors), plain and behind the RMSNorm prologue, then a norm weight: every row
            is R1, and the class is the float64 product's (a single Inf times a weight is that Inf in any summation order); one weight
            entry poisoned: its row only, the others R2.
prompt GEMM (the library keeps no route record for the prompt GEMMs as it does for the GEMV, so no launch can assert its kernel; the
            kernels are chosen through what csrc/ap_gemm.hip's dispatch reads -- K = 64 / 1088: ap_gemm_kernel, K = 2304: ap_gemm_pipe_kernel,
            GQ_GEMM_SHAPE 14 / 18: 4 / 8 waves, 5 to 8 bits: ap_gemm_wide_kernel -- and the split is asserted by its workspace size > 0)
            N = 36, K = 64 / 1088 (first kernel) and 2304 (pipelined), the dispatcher's tile and the forced ones, 5- and 8-bit (wide), and
            the planned K split through a workspace: one token row poisoned -> that row R1 (fp32-accumulating: NaN accepted for Inf),
            every other token row R2.
rows norm   D = 256: one element of x, of delta, of one row poisoned -- that row follows the model element by element (an Inf leaves NaN in
            its place and 0 elsewhere: ssq = Inf, scale 0), the x + delta written back as well, the other rows R2; one weight poisoned: its
            column in every row, the other columns R2.

Measured on an MI355X (NaN returned / outputs whose reference is +-Inf): head, token row 12 / 12 at every S; head, lm_head row 6 / 12,
160 / 204 and 322 / 396 at S = 1, 17, 33 (Inf - Inf inside the online softmax); dense GEMV and rows RMSNorm 0: class-exact.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import head_nll_model as hm  # noqa: E402
import halfsweep_model as hs  # noqa: E402
import nonfinite_model as nf  # noqa: E402
from test_head_nll_gpu import _run as head_run  # noqa: E402

SIZES = (1, 17, 33)


def _finish(bad, what, sub, n):
    print(f"{what}: NaN for Inf in {sub} of {n} outputs whose reference is +-Inf")
    assert not bad, "%d violation(s):\n%s" % (len(bad), "\n".join(bad[:12]))


# ------------------------------------------------------------------------------------------------ the scoring head
@pytest.mark.parametrize("S", SIZES)
def test_head_poisoned_token_row(S):
    V, D = 300, 64
    xn, W = hm.roundoff_case(S, V, D, seed=S)
    t = hm.targets(S, V, hm.split_ranges(V, 2), seed=1)
    r0 = S // 2
    bad, sub, n = [], 0, 0
    for splits in (0, 2):
        rc, blp, blse, btop = head_run(xn, W, t, splits)
        assert rc == 0 and np.isfinite(blp).all() and np.isfinite(blse).all()
        clean = np.arange(S) != r0
        for pname in nf.POISONS:
            for k in (0, D - 1):
                xp = xn.copy()
                xp[r0, k] = nf.poison(pname)
                rc, glp, glse, gtop = head_run(xp, W, t, splits)
                assert rc == 0
                lse, lp = nf.head_ref(hm.logits16(xp, W), t)
                assert not np.isfinite(lse[r0])
                for got, ref, base in ((glse, lse, blse), (glp, lp, blp)):
                    b, s_ = nf.check32(got, ref, clean, base)
                    bad += [f"splits {splits} {pname}@{k}: {v}" for v in b]
                    sub += s_
                    n += int(np.isinf(ref).sum())
                assert np.array_equal(gtop[clean], btop[clean]), "top1 of a clean row moved"
    _finish(bad, f"head, token row, S = {S}", sub, n)


@pytest.mark.parametrize("S", SIZES)
def test_head_poisoned_lm_head_row(S):
    V, D = 300, 64
    xn, W = hm.roundoff_case(S, V, D, seed=10 + S)
    bad, sub, n, seen_neg_target = [], 0, 0, 0
    for splits in (0, 2):
        for v0 in (0, 255, V - 1):   # first tile, last row of the second, the ragged tile's last
            t = hm.targets(S, V, hm.split_ranges(V, 2), seed=2)
            t[::3] = v0   # (some rows are scored on the poisoned column itself)
            for pname in nf.POISONS:
                Wp = W.copy()
                Wp[v0, 5] = nf.poison(pname)
                l64 = hm.logits16(xn, Wp)
                lse, lp = nf.head_ref(l64, t)
                rc, glp, glse, gtop = head_run(xn, Wp, t, splits)
                assert rc == 0
                if "nan" in pname:
                    assert np.isnan(lse).all() and np.isnan(lp[t >= 0]).all()
                for got, ref in ((glse, lse), (glp, lp)):
                    b, s_ = nf.check32(got, ref)
                    bad += [f"splits {splits} v0 {v0} {pname}: {v}" for v in b]
                    sub += s_
                    n += int(np.isinf(ref).sum())
                fin = np.isfinite(lse)   # the rows whose poisoned logit is -Inf: the column adds 0
                tol = 2.0 * hm.ulp16(np.abs(np.where(np.isfinite(l64), l64, 0.0)).max(axis=1))
                assert (np.abs(glse[fin].astype(np.float64) - lse[fin]) <= tol[fin]).all()
                ok = fin & np.isfinite(lp)
                assert (np.abs(glp[ok].astype(np.float64) - lp[ok]) <= tol[ok]).all()
                seen_neg_target += int((fin & (lp == -np.inf)).sum())
    assert S == 1 or seen_neg_target > 0, "no row was scored on a -Inf logit"
    _finish(bad, f"head, lm_head row, S = {S}", sub, n)


# ------------------------------------------------------------------------------------------------ the dense GEMV
def _dense(x, W, nw=None):
    from guidedquant_amd import _lib
    d = torch.device("cuda:0")
    N, K = W.shape
    tt = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float16)).to(d)  # noqa: E731
    xt, Wt, nt = tt(x), tt(W), tt(nw)
    out = torch.full((N, ), 1.0, dtype=torch.float16, device=d)
    _lib.check(_lib.lib().gq_dense_gemv_f16(xt.data_ptr(), Wt.data_ptr(), out.data_ptr(), N, K, nt.data_ptr() if nt is not None else None, nf.EPS,
                                            _lib.current_stream_ptr()), "gq_dense_gemv_f16")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _dense_ref(x, W, nw=None):
    act = nf.activation("norm", x, nw) if nw is not None else x
    with np.errstate(all="ignore"):
        return hs.to_half(W.astype(np.float64) @ act.astype(np.float64))


def test_dense_gemv():
    N, K = 33, 512   # (the kernel serves multiples of 512)
    rng = np.random.default_rng(3)
    W = rng.normal(0, 0.05, (N, K)).astype(np.float16)
    W[W == 0] = np.float16(0.01)
    x = rng.normal(0, 1, K).astype(np.float16)
    x[x == 0] = np.float16(0.5)
    nw = (1 + 0.1 * rng.normal(0, 1, K)).astype(np.float16)
    bad, sub, n = [], 0, 0

    def add(tag, got, ref, clean=None, base=None):
        nonlocal sub, n
        rc = nf.classify(ref)
        b, s_ = nf.check(got, rc, True, clean, base)
        bad.extend(f"{tag}: {v}" for v in b)
        sub += s_
        n += int(((rc == nf.PINF) | (rc == nf.NINF)).sum())
        return rc

    for with_norm in (False, True):
        w_ = nw if with_norm else None
        for tag, xp in nf.poisoned_vectors(x):
            rc = add(f"norm {with_norm} x {tag}", _dense(xp, W, w_), _dense_ref(xp, W, w_))
            assert (rc != nf.FINITE).all()
        base = _dense(x, W, w_)
        assert np.isfinite(base.astype(np.float32)).all()
        for pname in nf.POISONS:
            for r0, k in ((0, 0), (17, K - 1), (N - 1, 100)):
                Wp = W.copy()
                Wp[r0, k] = nf.poison(pname)
                add(f"norm {with_norm} W[{r0}, {k}] {pname}", _dense(x, Wp, w_), _dense_ref(x, Wp, w_), np.arange(N) != r0, base)
    for tag, wp in nf.poisoned_vectors(nw):
        rc = add(f"norm weight {tag}", _dense(x, W, wp), _dense_ref(x, W, wp))
        assert (rc != nf.FINITE).all()
    _finish(bad, "dense GEMV", sub, n)


# ------------------------------------------------------------------------------------------------ the rows RMSNorm
def _norm_rows(x, delta, w):
    from guidedquant_amd import _lib
    d = torch.device("cuda:0")
    S, D = x.shape
    tt = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float16)).to(d)  # noqa: E731
    xt, dt, wt = tt(x), tt(delta), tt(w)
    out = torch.full((S, D), 1.0, dtype=torch.float16, device=d)
    _lib.check(_lib.lib().gq_rmsnorm_rows(xt.data_ptr(), dt.data_ptr() if dt is not None else None, wt.data_ptr(), out.data_ptr(), S, D, nf.EPS,
                                          _lib.current_stream_ptr()), "gq_rmsnorm_rows")
    torch.cuda.synchronize()
    return xt.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize("S", SIZES)
def test_rmsnorm_rows(S):
    D = 256
    rng = np.random.default_rng(40 + S)
    x = rng.normal(0, 1, (S, D)).astype(np.float16)
    dl = rng.normal(0, 1, (S, D)).astype(np.float16)
    w = (1 + 0.1 * rng.normal(0, 1, D)).astype(np.float16)
    r0 = S // 2
    bad, sub, n = [], 0, 0

    def add(tag, got, ref, clean, base):
        nonlocal sub, n
        rc = nf.classify(ref)
        b, s_ = nf.check(got, rc, True, clean, base)
        bad.extend(f"{tag}: {v}" for v in b)
        sub += s_
        n += int(((rc == nf.PINF) | (rc == nf.NINF)).sum())

    for delta in (None, dl):
        bx, bo = _norm_rows(x, delta, w)
        assert np.isfinite(bo.astype(np.float32)).all()
        rows_clean = np.zeros((S, D), dtype=bool)
        rows_clean[np.arange(S) != r0] = True
        for pname in nf.POISONS:
            for k in (0, D - 1):
                for which in ("x", "delta") if delta is not None else ("x", ):
                    xp, dp = x.copy(), None if delta is None else delta.copy()
                    (xp if which == "x" else dp)[r0, k] = nf.poison(pname)
                    gx, go = _norm_rows(xp, dp, w)
                    rx, ro = nf.rmsnorm_rows_ref(xp, dp, w)
                    assert (nf.classify(ro[r0]) != nf.FINITE).any()
                    add(f"{which}[{r0}, {k}] {pname} out", go, ro, rows_clean, bo)
                    add(f"{which}[{r0}, {k}] {pname} x", gx, rx, rows_clean, bx)
                wp = w.copy()
                wp[k] = nf.poison(pname)
                gx, go = _norm_rows(x, delta, wp)
                _, ro = nf.rmsnorm_rows_ref(x, delta, wp)
                cols_clean = np.ones((S, D), dtype=bool)
                cols_clean[:, k] = False
                assert (nf.classify(ro[:, k]) != nf.FINITE).all()
                add(f"w[{k}] {pname}", go, ro, cols_clean, bo)
                assert np.array_equal(gx.view(np.uint16), bx.view(np.uint16))
    _finish(bad, f"rows RMSNorm, S = {S}", sub, n)


# ------------------------------------------------------------------------------------------------ the prompt GEMMs
GEMM_N = 36
# (bits, K, GQ_GEMM_SHAPE or None, workspace): ap_gemm_kernel (K = 64, 1088) and ap_gemm_pipe_kernel (K = 2304) under the dispatcher's
# choice and both forced tile shapes of test_bounds_ap_gemm_gpu (14, 18), ap_gemm_wide_kernel (5 and 8 bits), and the planned K split of
# the short grid at K = 2304 (two ranges through the workspace, gemm_reduce_kernel)
GEMM_CASES = [(2, 64, None, False), (4, 1088, 14, False), (3, 1088, 18, False), (2, 2304, None, False), (2, 2304, 14, False), (4, 2304, 18, False),
              (2, 2304, None, True), (3, 2304, None, True), (5, 64, None, False), (8, 1088, None, False), (5, 2304, None, False)]


def _gemm(X, q, lut, bits, ws):
    """gq_anyprec_gemm / gq_anyprec_gemm_ws on tests/guarded.py buffers; out and the workspace hold finite values (payloads), the guards as ever"""
    import guarded
    from guidedquant_amd import _lib
    L = _lib.lib()
    S, K = X.shape
    N = q.shape[1]
    g = guarded.Guards()
    xb, qb, lb = g.inp("x", np.ascontiguousarray(X)), g.inp("qweight", np.ascontiguousarray(q)), g.inp("lut", np.ascontiguousarray(lut))
    out = g.inp("out", np.full(S * N, nf.SENTINEL, dtype=np.uint16))
    nb = 0
    if ws:
        nb = int(L.gq_anyprec_gemm_ws_bytes(S, N, K, bits))
        wb = g.inp("workspace", np.ones(max(nb // 4, 1), dtype=np.float32))
        rc = L.gq_anyprec_gemm_ws(xb.ptr(), out.ptr(), qb.ptr(), lb.ptr(), S, N, K, bits, wb.ptr(), nb, _lib.current_stream_ptr())
    else:
        rc = L.gq_anyprec_gemm(xb.ptr(), out.ptr(), qb.ptr(), lb.ptr(), S, N, K, bits, _lib.current_stream_ptr())
    _lib.check(rc, "gq_anyprec_gemm")
    g.check()
    return out.numpy(np.float16, (S, N)), nb


@pytest.fixture
def gemm_env():
    import os
    from guidedquant_amd import _lib
    knobs = ("GQ_GEMM_SHAPE", "GQ_GEMM_KSPLIT", "GQ_GEMM_KSHAPE")
    saved = {k: os.environ.get(k) for k in knobs}

    def set_shape(shape):
        for k in knobs:
            os.environ.pop(k, None)
        if shape is not None:
            os.environ["GQ_GEMM_SHAPE"] = str(shape)
        _lib.lib().gq_reset_env_cache()
    yield set_shape
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v
    _lib.lib().gq_reset_env_cache()


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("bits,K,shape,ws", GEMM_CASES, ids=["b%d-K%d-shape%s-ws%d" % c for c in GEMM_CASES])
def test_prompt_gemm_poisoned_token_row(gemm_env, bits, K, shape, ws, S):
    """one token row poisoned (every poison; first column, last column, both infinities, the whole row NaN): that row of the output is
    not finite (the float64 product's class; NaN accepted for Inf), every other token row is bit-identical to the clean launch"""
    from oracle import oracle
    oracle.build()
    gemm_env(shape)
    Lr = nf.layer(GEMM_N, K, bits)
    q, lut = Lr["q"], Lr["lut"]
    X = np.random.default_rng(S + K).normal(0, 1, (S, K)).astype(np.float16)
    X[X == 0] = np.float16(0.5)
    r0 = S // 2
    base, nb = _gemm(X, q, lut, bits, ws)
    assert np.isfinite(base.astype(np.float32)).all() and (nb > 0) == ws, nb
    clean = np.zeros((S, GEMM_N), dtype=bool)
    clean[np.arange(S) != r0] = True
    bad, sub, n = [], 0, 0
    for tag, xp in nf.poisoned_vectors(X[r0]):
        Xp = X.copy()
        Xp[r0] = xp
        rc = np.zeros((S, GEMM_N), dtype=np.uint8)
        with np.errstate(all="ignore"):
            rc[r0] = nf.classify64(oracle.ap_gemv_f64(xp, q, lut, bits)[0])
        assert (rc[r0] != nf.FINITE).all()
        got, _ = _gemm(Xp, q, lut, bits, ws)
        b, s_ = nf.check(got, rc, False, clean, base)
        bad += [f"{tag}: {v}" for v in b]
        sub += s_
        n += int(((rc == nf.PINF) | (rc == nf.NINF)).sum())
    _finish(bad, f"prompt GEMM bits {bits} K {K} shape {shape} ws {ws} S {S}", sub, n)
