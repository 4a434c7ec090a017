"""GPU: NaN and Inf through gq_anyprec_gemv_fused and gq_anyprec_gemv, family by family, against tests/nonfinite_model.py (R1 no hiding,
R2 no spreading, R3 class, overflow).

The families and their knobs are those of tests/test_bounds_ap_gemv_gpu.py (CASES, set_env); every launch asserts its route.  A family runs
at the smallest K and the lowest bit width of its CASES rows, with N = 34 rows (two groups of 16 and two more; tests/test_nonfinite_model_cpu.py
shows that the dry dispatch sends every form here to its family).  out, and the batch launches' guarded out, are pre-filled with 1.0 and
not with NaN: an element a kernel skipped would otherwise pass for a propagated NaN.

  x            every poison (+NaN, -NaN, the low-byte NaN 0x7C01, +Inf, -Inf) at element 0, K - 1, in the tail chunk and next to an
               extracted hot channel in its group of 128; a +Inf and a -Inf together; the whole vector NaN.  Plain, behind the RMSNorm
               prologue (then a poisoned norm weight instead) and behind the SiLU * up prologue (gate poisoned; up +-Inf over a gate of 0).
               Every row's reference is non-finite: R1 and R3 on all of them.
  lut          one entry of row 17, the code of its column 0, poisoned: row 17 is R1 / R3, the 33 others are bit-identical to the clean
               launch (R2).  Plain, residual epilogue, and the pair epilogue (rows 16 and 17: gate and up of pair 8; the other 16 pairs R2).
  residual     one element poisoned: its row R1 / R3, the others R2.
  batch        M = 2, 3, 4 rows of gq_anyprec_gemv where the family serves a batch, row 1 poisoned: the other rows R2.
  overflow     nonfinite_model.overflow_layer: rows of +-3e5 must be +-Inf; rows of +-6e4 are finite alone and +-Inf behind a residual
               of +-8192.

  tail chunk   the same activations at the family's smallest K with a tail chunk behind full chunks of 1024 (1056, 1280, 16640)
  K split      stream-ksplit with its workspace (18432 columns: nine slices, ap_ksplit_reduce_kernel): x, a lut entry, a residual element
  qkv_rope     gq_anyprec_gemv_qkv_rope: x, and an entry of the position's cos / sin row; the rotated q and the cache rows by class

R3 is exact (the oracle's class, NaN vs +Inf vs -Inf) for the exact-order families exact, pair-table, generic and wide, and for dq (against the rounded
float64 product); for plane, plane-local, plane-chain, stream and stream-ksplit a NaN where the reference says +-Inf is accepted and counted (printed per test).

Measured on an MI355X (NaN returned / outputs whose reference is +-Inf); no R1, R2, R3 or overflow violation in any family:
  activations     exact 0 / 606, wide 0 / 608, pair-table 0 / 442, generic 0 / 283, dq 0 / 428 (class-exact, dq too);
                  plane 602 / 602, plane-local 386 / 386, plane-chain 287 / 287, stream 440 / 440: a non-finite activation stays in the
                  bf8 image (no threshold, nothing extracted) and every row comes back NaN, never an infinity
  lut / residual  0 / 2 in every family: the poisoned row carries the poison's own class, the other 33 rows are bit-identical
  batch rows      exact 0 / 450, generic 0 / 441, pair-table 0 / 456, plane 444 / 444, plane-chain 453 / 453
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import nonfinite_model as nf  # noqa: E402
import test_bounds_ap_gemv_gpu as t  # noqa: E402
from ap_helpers import assert_route, run_fused  # noqa: E402
from test_bounds_ap_gemv_gpu import _restore_env, oracle  # noqa: E402,F401  (autouse: the GQ_* environment and the mode are put back)

N = nf.N_ROWS
R0 = 17
SHAPES = nf.family_shapes(t.CASES)
FORMS = {fam: set().union(*[set(c[4]) for c in t.CASES if c[0] == fam]) for fam in SHAPES}
BATCH = nf.BATCH_FAMILIES
FILL = 1.0


def _run(fam, *a, **k):
    return run_fused(*a, expect=fam, fill=FILL, **k)


def _run_batch(fam, X, q, lut, bits):
    """gq_anyprec_gemv with guarded buffers; out holds the finite sentinel (an input payload of guarded.py: the guards are as it makes them)"""
    import guarded
    from guidedquant_amd import _lib
    X = np.ascontiguousarray(X, dtype=np.float16)
    M, K = X.shape
    g = guarded.Guards()
    xb, qb, lb = g.inp("x", X), g.inp("qweight", np.ascontiguousarray(q)), g.inp("lut", np.ascontiguousarray(lut, dtype=np.float16))
    out = g.inp("out", np.full(M * q.shape[1], nf.SENTINEL, dtype=np.uint16))
    _lib.check(_lib.lib().gq_anyprec_gemv(xb.ptr(), out.ptr(), qb.ptr(), lb.ptr(), M, q.shape[1], K, bits, 0, _lib.current_stream_ptr()), "gq_anyprec_gemv")
    assert_route(fam)
    g.check()
    return out.numpy(np.float16, (M, q.shape[1]))


class Tally:
    def __init__(self, fam):
        self.fam, self.bad, self.sub, self.n, self.launches = fam, [], 0, 0, 0

    def add(self, tag, got, ref_class, clean=None, baseline=None):
        bad, sub = nf.check(got, ref_class, self.fam in nf.CLASS_EXACT, clean, baseline)
        self.bad += [f"{tag}: {b}" for b in bad]
        self.sub += sub
        self.n += int(((ref_class == nf.PINF) | (ref_class == nf.NINF)).sum())
        self.launches += 1

    def done(self, what):
        print(f"{what} {self.fam}: {self.launches} launches, NaN for Inf in {self.sub} of {self.n} outputs whose reference is +-Inf")
        assert not self.bad, "%d violation(s):\n%s" % (len(self.bad), "\n".join(self.bad[:12]))


def _setup(fam):
    bits, K = SHAPES[fam]
    t.set_env(fam)
    return bits, K, nf.layer(N, K, bits), fam in nf.EXACT_ORDER


@pytest.mark.parametrize("fam", sorted(SHAPES))
def test_poisoned_activations(oracle, fam):
    bits, K, L, exact = _setup(fam)
    q, lut = L["q"], L["lut"]
    tally = Tally(fam)

    def one(tag, form, x, nw=None, flags=0):
        got = _run(fam, x, q, lut, bits, norm_weight=nw, eps=nf.EPS, flags=flags)
        ref = nf.gemv_ref(oracle, nf.activation(form, x, nw), q, lut, bits, exact)
        rc = nf.classify(ref)
        assert (rc != nf.FINITE).all(), f"{tag}: the reference itself is finite in {int((rc == nf.FINITE).sum())} rows"
        tally.add(f"{form} {tag}", got, rc)

    for tag, xp in nf.poisoned_vectors(L["x"], L["hot"][0]):
        one(tag, "plain", xp)
    if "norm" in FORMS[fam]:
        for tag, xp in nf.poisoned_vectors(L["x"], L["hot"][0]):
            one("x " + tag, "norm", xp, L["nw"])
        for tag, wp in nf.poisoned_vectors(L["nw"]):
            one("weight " + tag, "norm", L["x"], wp)
    if "silu" in FORMS[fam]:
        gate, up = L["gu"][:K], L["gu"][K:]
        for tag, gp in nf.poisoned_vectors(gate):
            one("gate " + tag, "silu", np.concatenate([gp, up]), flags=2)
        for pname in ("+inf", "-inf"):
            for where, i in nf.placements(K).items():
                g2, u2 = gate.copy(), up.copy()
                g2[i], u2[i] = 0, nf.poison(pname)
                one(f"up {pname}@{where} over a zero gate", "silu", np.concatenate([g2, u2]), flags=2)
    tally.done("activations")


TAIL_SHAPES = nf.tail_shapes(t.CASES)


@pytest.mark.parametrize("fam", sorted(TAIL_SHAPES))
def test_poisoned_activations_with_a_tail_chunk(oracle, fam):
    """the family's smallest K with a tail chunk behind full chunks of 1024 (1056, 1280, 16640): every placement, the tail's included"""
    bits, K = TAIL_SHAPES[fam]
    t.set_env(fam)
    L = nf.layer(N, K, bits)
    exact = fam in nf.EXACT_ORDER
    tally = Tally(fam)
    from guidedquant_amd import _lib
    assert _lib.ap_plan_route(N, K, bits, 1, False, 0, 0)[0] == fam
    assert K // 1024 * 1024 <= nf.placements(K)["tail"] < K
    for tag, xp in nf.poisoned_vectors(L["x"], L["hot"][0]):
        rc = nf.classify(nf.gemv_ref(oracle, xp, L["q"], L["lut"], bits, exact))
        assert (rc != nf.FINITE).all()
        tally.add(tag, _run(fam, xp, L["q"], L["lut"], bits), rc)
    tally.done(f"activations, K = {K}")


KSPLIT_N, KSPLIT_K = 34, 18432


def test_stream_ksplit_with_a_workspace(oracle):
    """the K split over blocks (stream-ksplit: fp32 slices in a workspace, ap_ksplit_reduce_kernel): x poisoned, then one lut entry and one
    residual element with R2 on the other rows.  The workspace starts at 1.0 like out."""
    from guidedquant_amd import _lib
    fam, bits = "stream-ksplit", 2
    t.set_env(fam)
    nb = _lib.lib().gq_anyprec_gemv_fused_ws_bytes(KSPLIT_N, KSPLIT_K, bits, 1)
    assert nb > 0 and _lib.ap_plan_route(KSPLIT_N, KSPLIT_K, bits, 1, False, 0, nb)[0] == fam
    L = nf.layer(KSPLIT_N, KSPLIT_K, bits)
    q, lut, x, res = L["q"], L["lut"], L["x"], L["res"]
    run = lambda *a, **k: _run(fam, *a, workspace=True, **k)  # noqa: E731
    tally = Tally(fam)
    for tag, xp in nf.poisoned_vectors(x, L["hot"][0]):
        rc = nf.classify(nf.gemv_ref(oracle, xp, q, lut, bits, False))
        assert (rc != nf.FINITE).all()
        tally.add(tag, run(xp, q, lut, bits), rc)
    codes = oracle.ap_unpack(q, bits)
    others = np.arange(KSPLIT_N) != R0
    base, base_r = run(x, q, lut, bits), run(x, q, lut, bits, residual=res, flags=1)
    assert np.isfinite(base.astype(np.float32)).all()
    for pname in nf.POISONS:
        lp = lut.copy()
        lp[R0, codes[R0, 0]] = nf.poison(pname)
        tally.add(f"lut {pname}", run(x, q, lp, bits), nf.classify(nf.gemv_ref(oracle, x, q, lp, bits, False)), others, base)
        rp = res.copy()
        rp[R0] = nf.poison(pname)
        ref = nf.epilogue_ref(nf.gemv_ref(oracle, x, q, lut, bits, False), rp)
        tally.add(f"residual {pname}", run(x, q, lut, bits, residual=rp, flags=1), nf.classify(ref), others, base_r)
    tally.done("K split with a workspace")


@pytest.mark.parametrize("fam", sorted(SHAPES))
def test_poisoned_lut_entry_and_residual(oracle, fam):
    bits, K, L, exact = _setup(fam)
    q, lut, x, res = L["q"], L["lut"], L["x"], L["res"]
    codes = oracle.ap_unpack(q, bits)
    tally = Tally(fam)
    others = np.arange(N) != R0
    base = _run(fam, x, q, lut, bits)
    assert np.isfinite(base.astype(np.float32)).all()
    base_r = _run(fam, x, q, lut, bits, residual=res, flags=1) if "resid" in FORMS[fam] else None
    base_p = _run(fam, x, q, lut, bits, flags=4, out_elems=N // 2) if "pairs" in FORMS[fam] else None
    for pname in nf.POISONS:
        lp = lut.copy()
        lp[R0, codes[R0, 0]] = nf.poison(pname)
        ref = nf.gemv_ref(oracle, x, q, lp, bits, exact)
        assert nf.classify(ref)[R0] != nf.FINITE and (nf.classify(ref)[others] == nf.FINITE).all()
        tally.add(f"lut {pname}", _run(fam, x, q, lp, bits), nf.classify(ref), others, base)
        if base_r is not None:
            got = _run(fam, x, q, lp, bits, residual=res, flags=1)
            tally.add(f"lut {pname} + residual", got, nf.classify(nf.epilogue_ref(ref, res)), others, base_r)
            rp = res.copy()
            rp[R0] = nf.poison(pname)
            got = _run(fam, x, q, lut, bits, residual=rp, flags=1)
            tally.add(f"residual {pname}", got, nf.classify(nf.epilogue_ref(nf.gemv_ref(oracle, x, q, lut, bits, exact), rp)), others, base_r)
        if base_p is not None:
            for row in (R0 - 1, R0):   # gate and up of one pair
                lp = lut.copy()
                lp[row, codes[row, 0]] = nf.poison(pname)
                rc = nf.classify(nf.epilogue_ref(nf.gemv_ref(oracle, x, q, lp, bits, exact), pairs=True))
                assert rc[row // 2] != nf.FINITE
                got = _run(fam, x, q, lp, bits, flags=4, out_elems=N // 2)
                tally.add(f"lut {pname} row {row} + pairs", got, rc, np.arange(N // 2) != row // 2, base_p)
    tally.done("lut / residual")


@pytest.mark.parametrize("fam", BATCH)
def test_poisoned_batch_row(oracle, fam):
    bits, K, L, exact = _setup(fam)
    q, lut = L["q"], L["lut"]
    X = np.random.default_rng(5).normal(0, 1, (4, K)).astype(np.float16)
    tally = Tally(fam)
    for M in (2, 3, 4):
        from guidedquant_amd import _lib
        assert _lib.ap_plan_route(N, K, bits, M, False, 0, 0)[0] == fam
        base = _run_batch(fam, X[:M], q, lut, bits)
        assert np.isfinite(base.astype(np.float32)).all()
        clean = np.ones((M, N), dtype=bool)
        clean[1] = False
        for tag, xp in nf.poisoned_vectors(X[1]):
            Xp = X[:M].copy()
            Xp[1] = xp
            rc = np.zeros((M, N), dtype=np.uint8)
            rc[1] = nf.classify(nf.gemv_ref(oracle, xp, q, lut, bits, exact))
            assert (rc[1] != nf.FINITE).all()
            tally.add(f"M = {M} {tag}", _run_batch(fam, Xp, q, lut, bits), rc, clean, base)
    tally.done("batch")


@pytest.mark.parametrize("fam", sorted(SHAPES))
def test_finite_results_beyond_fp16(oracle, fam):
    """a finite sum beyond 65 520 is +-Inf as round-to-nearest-even gives it, never +-65504"""
    bits, K = SHAPES[fam]
    t.set_env(fam)
    q, lut, x, res, y64 = nf.overflow_layer(oracle, N, K, bits)
    big = np.abs(y64) > 1e5
    got = _run(fam, x, q, lut, bits)
    bad = nf.check_overflow(got[big], y64[big])
    near = got[~big].astype(np.float64)
    assert np.isfinite(near).all() and (np.abs(near / y64[~big] - 1) < 0.03).all(), "the rows of +-6e4 are finite without the residual"
    if "resid" in FORMS[fam]:
        got_r = _run(fam, x, q, lut, bits, residual=res, flags=1)
        want = np.where(y64 > 0, nf.PINF, nf.NINF)
        idx = np.flatnonzero(nf.classify(got_r) != want)
        bad += ["residual pushes over: row %d (y64 %r, residual %r) is %s" % (i, float(y64[i]), float(res[i]), hex(int(got_r.view(np.uint16)[i]))) for i in idx[:6]]
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ gq_anyprec_gemv_qkv_rope
def test_qkv_rope_poisoned_activation_and_rope_tables():
    """the fused q / k / v GEMV with RoPE and the cache write in its epilogue (stream-qkv-rope), (H, Hkv, hd, K) = (8, 2, 128, 4096), 2 bits,
    position 7 of a cache of 40 rows that holds finite junk.
      x poisoned      behind the RMSNorm prologue every projection is NaN (nonfinite_model: ssq NaN, or ssq = Inf and 0 * Inf): the rotated
                      q, and row 7 of the k and the v cache, are non-finite in every element (R1);
      cos / sin       one entry of the position's row poisoned (elements j and j + hd / 2 hold the same angle: both, so that the case does
                      not depend on which of the two a kernel reads): elements j and j + hd / 2 of every rotated q head and of every
                      key head follow apply_rotary_pos_emb's fp16 expression on the unfused projection by class (a NaN entry: NaN; an
                      Inf entry: +-Inf, or NaN where the other term is the opposite infinity); every other element, and the whole v
                      row, is bit-identical to the clean launch (R2).
    In every case the 39 other rows of both caches keep their bits."""
    import os
    import torch as T
    from guidedquant_amd import _lib
    from guidedquant_amd.model import rope_tables
    import halfsweep_model as hs
    L = _lib.lib()
    H, Hkv, hd, K, max_seq, bits, p = 8, 2, 128, 4096, 40, 2, 7
    Nq = (H + 2 * Hkv) * hd
    L.gq_set_ap_mode(0)
    os.environ["GQ_PL_MIN_MWEIGHTS"], os.environ["GQ_ST"] = "0", "2"
    L.gq_reset_env_cache()
    if not L.gq_anyprec_qkv_rope_supported(Nq, K, bits, hd):
        pytest.skip("gq_anyprec_qkv_rope_supported(1536, 4096, 2, 128) == 0: shape not served by the fused launch in this build")
    d = T.device("cuda:0")
    g = T.Generator().manual_seed(11)
    qw = T.randint(-2**31, 2**31 - 1, (bits, Nq, K // 32), dtype=T.int32, generator=g).to(d)
    lut = (T.randn(Nq, 1 << bits, generator=g) * 0.03).half().to(d)
    nw = (1 + 0.1 * T.randn(K, generator=g)).half().to(d)
    x0 = T.randn(K, generator=g).half()
    junk = (T.randn(Hkv, max_seq, hd, generator=g) * 5).half()
    cos0, sin0 = (t.cpu() for t in rope_tables(hd, max_seq, 500000.0, d))
    st = _lib.current_stream_ptr()
    pos = T.tensor([p], dtype=T.int32, device=d)

    def fused(x, cos, sin):
        xd, cd, sd = x.to(d), cos.to(d).contiguous(), sin.to(d).contiguous()
        kc, vc = junk.clone().to(d), junk.clone().to(d)
        out = T.full((Nq, ), FILL, dtype=T.float16, device=d)
        _lib.check(L.gq_anyprec_gemv_qkv_rope(xd.data_ptr(), out.data_ptr(), qw.data_ptr(), lut.data_ptr(), Nq, K, bits, nw.data_ptr(), nf.EPS, pos.data_ptr(),
                                              cd.data_ptr(), sd.data_ptr(), kc.data_ptr(), vc.data_ptr(), H, Hkv, hd, max_seq, st), "gq_anyprec_gemv_qkv_rope")
        assert_route("stream-qkv-rope")
        T.cuda.synchronize()
        kc, vc = kc.cpu(), vc.cpu()
        rest = T.arange(max_seq) != p
        assert T.equal(kc[:, rest].view(T.int16), junk[:, rest].view(T.int16)) and T.equal(vc[:, rest].view(T.int16), junk[:, rest].view(T.int16))
        return out[:H * hd].cpu().numpy().reshape(H, hd), kc[:, p].numpy(), vc[:, p].numpy()

    bq, bk, bv = fused(x0, cos0, sin0)
    assert all(np.isfinite(a.astype(np.float32)).all() for a in (bq, bk, bv))
    # the unfused projection (the same kernel family: bit-identical, tests/test_qkv_rope_gpu.py), for the rotation's model
    proj = T.zeros(Nq, dtype=T.float16, device=d)
    _lib.check(L.gq_anyprec_gemv_fused(x0.to(d).data_ptr(), proj.data_ptr(), qw.data_ptr(), lut.data_ptr(), Nq, K, bits, nw.data_ptr(), nf.EPS, None, 0, st), "wqkv")
    T.cuda.synchronize()
    proj = proj.cpu()
    q_un, k_un = proj[:H * hd].view(H, hd), proj[H * hd:(H + Hkv) * hd].view(Hkv, hd)
    assert T.equal(proj[(H + Hkv) * hd:].view(T.int16), T.from_numpy(bv.copy()).reshape(-1).view(T.int16))

    def rope(v, c, s):
        rot = T.cat((-v[..., hd // 2:], v[..., :hd // 2]), dim=-1)
        return ((v * c) + (rot * s)).numpy()

    bad, launches = [], 0
    for tag, xp in nf.poisoned_vectors(x0.numpy()):
        gq_, gk, gv = fused(T.from_numpy(xp.copy()), cos0, sin0)
        for name, got in (("q", gq_), ("k", gk), ("v", gv)):
            b, _ = nf.check(got, np.full(got.shape, nf.NAN, dtype=np.uint8), False)
            bad += [f"x {tag} {name}: {v}" for v in b]
        launches += 1
    for table in ("cos", "sin"):
        for pname in nf.POISONS:
            for j in (0, hd // 2 - 1, 17):
                cos, sin = cos0.clone(), sin0.clone()
                tb = cos if table == "cos" else sin
                tb[p, j] = tb[p, j + hd // 2] = T.from_numpy(np.array([nf.poison(pname)]))[0]
                gq_, gk, gv = fused(x0, cos, sin)
                cols = np.zeros(hd, dtype=bool)
                cols[[j, j + hd // 2]] = True
                for name, got, un, base in (("q", gq_, q_un, bq), ("k", gk, k_un, bk)):
                    rc = nf.classify(rope(un, cos[p], sin[p]))
                    assert (rc[:, cols] != nf.FINITE).all() and (rc[:, ~cols] == nf.FINITE).all()
                    clean = np.broadcast_to(~cols, got.shape)
                    b, _ = nf.check(got, rc, True, clean, base)
                    bad += [f"{table}[{p}, {j}] {pname} {name}: {v}" for v in b]
                if not hs.same(gv, bv).all():
                    bad.append(f"{table}[{p}, {j}] {pname}: the v row changed")
                launches += 1
    print(f"qkv_rope: {launches} launches")
    assert not bad, "%d violation(s):\n%s" % (len(bad), "\n".join(bad[:12]))
