"""GPU: NaN and Inf through LUT-GEMM and the QTIP kernels that have a small stand-alone launch, against tests/nonfinite_model.py.  Outputs
start from finite values (1.0), never from NaN.

LUT-GEMM      gq_lutgemm_gemv and gq_lutgemm_gemv_ws (GQ_LUTGEMM_WS = 0 / 1), both block widths (GQ_LG_SMALL_BLOCKS = 0 and the default),
              (N, K, group) = (300, 1024, 32) and (64, 256, 128) at 2 bits, on a NON-ZERO initial out (the kernel adds to it): x
              poisoned (nonfinite_model.poisoned_vectors), one alpha, one q_bias and one initial out element poisoned.  The kernel walks
              the reference's fp16 operation sequence, so the class must equal oracle.lutgemm_f16's exactly (R3 exact), and where the
              oracle is finite the bits must equal its bits -- which is R2 and more.
QTIP matvec   decompress_matvec (M, K) = (256, 512), R = 2: x poisoned; the float64 product's class per row (fp32 accumulation: NaN
              accepted for Inf).
QTIP linear   gq_qtip_linear_in + gq_qtip_linear_out on (K, M) = (128, 256) and (32, 32): plain, RMSNorm and SiLU * up prologues.  The
              input passes a Hadamard transform, which mixes every element into every output: with one NaN (or one Inf: the transform
              of a vector with a single Inf is all +-Inf, and the trellis product of both infinities is NaN) EVERY output is non-finite,
              so R1 is observable on the SiLU * up site the half sweep could not reach.  One SV entry and one residual element
              poisoned: that row only, the others bit-identical to the clean launch.
QTIP GEMM     gq_qtip_gemm_ws (the prompt kernel), (M, K) = (256, 512), S in {1, 17, 33}: one token row poisoned -> that row by the float64
              product's class, every other token row bit-identical.
pretransformed  the fourth prologue of gq_qtip_linear_in (the fp16 vector the matvec consumes is handed in): one element k poisoned; the
              reference is built from the kernel's own finite launches by linearity -- the one-hot launch at k returns column k of the
              decoded weights -- so row r is the class of w[r, k] * poison (+ the finite rest): R1 and R3 per row.
partial sums  gq_qtip_linear_out and gq_qtip_linear_out_seg on M = 256 with parts = 2 and a residual: a NaN / Inf in ONE partial sum reaches
              every output through the Hadamard transform (float64 Sylvester reference: class per output); one SV entry, one residual
              element: that row, the others bit-identical.
factor width  gq_qtip_transform at 11008 = 172 * 64 with the golden hadK table (tests/golden/had_n11008.npz): the output side with one
              poisoned sum (every output non-finite) and one poisoned scale (that output only, the others bit-identical); the input
              side with one poisoned element (every output non-finite).
mlp_mid       gq_qtip_mlp_mid at 11008, parts = 2: a poisoned partial sum of gate (of up) makes every gate (up) output and every z32
              non-finite and leaves up (gate) bit-identical; a poisoned gate scale reaches its own gate output and, behind the
              172-point side of the input transform, column r0 % 64 of z32 [172][64] -- every other gate output, every up output and
              every other column of z32 bit-identical.
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import halfsweep_model as hs  # noqa: E402
import nonfinite_model as nf  # noqa: E402
from test_qtip_gpu import _rand_qlinear  # noqa: E402

D = "cuda:0"


@pytest.fixture
def env():
    from guidedquant_amd import _lib
    knobs = ("GQ_LUTGEMM_WS", "GQ_LG_SMALL_BLOCKS")
    saved = {k: os.environ.get(k) for k in knobs}

    def set_(**kv):
        for k in knobs:
            os.environ.pop(k, None)
        for k, v in kv.items():
            if v is not None:
                os.environ[k] = str(v)
        _lib.lib().gq_reset_env_cache()
    yield set_
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v
    _lib.lib().gq_reset_env_cache()


# ------------------------------------------------------------------------------------------------ LUT-GEMM
@pytest.mark.parametrize("small", (None, 0), ids=("blocks-default", "blocks-wide"))
@pytest.mark.parametrize("ws", ("0", "1"))
@pytest.mark.parametrize("N,K,g", [(300, 1024, 32), (64, 256, 128)])
def test_lutgemm_class_exact(env, N, K, g, ws, small):
    from guidedquant_amd.ap_gemv import lutgemm_gemv
    from oracle import oracle
    oracle.build()
    env(GQ_LUTGEMM_WS=ws, GQ_LG_SMALL_BLOCKS=small)
    bits = 2
    rng = np.random.default_rng(N + K)
    q = rng.integers(-2**31, 2**31, (K // 32, bits, N), dtype=np.int64).astype(np.int32)
    alpha = (rng.random((K // g, bits, N)) * 0.01 + 0.001).astype(np.float16)
    qb = rng.normal(0, 0.01, (K // g, N)).astype(np.float16)
    x = rng.normal(0, 1, K).astype(np.float16)
    out0 = rng.normal(0, 1, N).astype(np.float16)
    qd = torch.from_numpy(q).to(D)

    def run(x_, a_, b_, o_):
        o = torch.from_numpy(o_.copy()).reshape(1, 1, N).to(D)
        lutgemm_gemv(torch.from_numpy(x_.copy()).reshape(1, 1, K).to(D), o, qd, torch.from_numpy(a_.copy()).to(D), torch.from_numpy(b_.copy()).to(D), bits, g)
        torch.cuda.synchronize()
        return o.cpu().numpy().reshape(N)

    bad = []

    def one(tag, x_, a_, b_, o_, rows=None):
        with np.errstate(all="ignore"):
            want = oracle.lutgemm_f16(x_, q, a_, b_, bits, g, out=o_)
        got = run(x_, a_, b_, o_)
        rc = nf.classify(want)
        if rows is not None:
            assert (rc[rows] != nf.FINITE).all() and (np.delete(rc, rows) == nf.FINITE).all(), tag
        else:
            assert (rc != nf.FINITE).all(), tag
        b, _ = nf.check(got, rc, True, rc == nf.FINITE, want)
        bad.extend(f"{tag}: {v}" for v in b)

    one("clean", x, alpha, qb, out0, rows=[])
    for tag, xp in nf.poisoned_vectors(x):
        one("x " + tag, xp, alpha, qb, out0)
    for pname in nf.POISONS:
        for n0 in (0, N - 1, 33):
            ap_, bp, op = alpha.copy(), qb.copy(), out0.copy()
            ap_[-1, 0, n0] = nf.poison(pname)   # (plane 0: the reference reads a group's first alpha and doubles it plane by plane)
            one(f"alpha[-1, 0, {n0}] {pname}", x, ap_, qb, out0, rows=[n0])
            bp[0, n0] = nf.poison(pname)
            one(f"q_bias[0, {n0}] {pname}", x, alpha, bp, out0, rows=[n0])
            op[n0] = nf.poison(pname)
            one(f"out[{n0}] {pname}", x, alpha, qb, op, rows=[n0])
    assert not bad, "%d violation(s):\n%s" % (len(bad), "\n".join(bad[:12]))


# ------------------------------------------------------------------------------------------------ QTIP
def _recipe(R, M, K, seed=42):
    g = torch.Generator().manual_seed(seed)
    comp = torch.randint(-2**31, 2**31 - 1, (R * M * K // 32, ), dtype=torch.int32, generator=g)
    tlut = torch.clamp(torch.randn(512, 2, generator=g) / 16, -1, 1).half()
    x = torch.clamp(torch.randn(40, K, generator=g) / 16, -1, 1).half()
    return comp.numpy(), tlut.numpy(), x.numpy()


def test_qtip_matvec():
    from guidedquant_amd.qtip import qtip_kernels
    from oracle import oracle
    oracle.build()
    M, K, R = 256, 512, 2
    comp, tlut, X = _recipe(R, M, K)
    W = oracle.qtip_decode(comp, tlut, M, K, R).astype(np.float64)
    cd, td = torch.from_numpy(comp).to(D), torch.from_numpy(tlut.reshape(-1).copy()).to(D)
    bad, sub, n = [], 0, 0
    for tag, xp in nf.poisoned_vectors(X[0]):
        out = torch.full((M, 1), 1.0, dtype=torch.float32, device=D)
        getattr(qtip_kernels, f"decompress_matvec_16_9_{R}_1_{M}_1_{K}")(out, cd, torch.from_numpy(xp.copy()).reshape(K, 1).to(D), td)
        torch.cuda.synchronize()
        with np.errstate(all="ignore"):
            ref = W @ xp.astype(np.float64)
        assert not np.isfinite(ref).any()
        b, s_ = nf.check32(out.cpu().numpy()[:, 0], ref)
        bad += [f"{tag}: {v}" for v in b]
        sub += s_
        n += int(np.isinf(ref).sum())
    print(f"QTIP matvec: NaN for Inf in {sub} of {n} outputs whose reference is +-Inf")
    assert not bad, "%d violation(s):\n%s" % (len(bad), "\n".join(bad[:12]))


def _linear(lin, x16, pro=0, x2=None, normw=None, resid=None, sv=None):
    """gq_qtip_linear_in + gq_qtip_linear_out for one QuantizedLinear (tests/test_qtip_gpu._fused_linear with finite pre-fills)"""
    from guidedquant_amd import _lib
    L = _lib.lib()
    K, M = lin.in_features, lin.out_features
    su = lin.SU.float().contiguous()
    sv = (lin.SV.float() * 32.0).contiguous() if sv is None else sv
    y32 = torch.full((M, ), 1.0, dtype=torch.float32, device=D)
    out = torch.full((M, ), 1.0, dtype=torch.float16, device=D)
    ain = (_lib.GqQtipIn * 1)(_lib.GqQtipIn(lin.trellis.data_ptr(), su.data_ptr(), lin.tlut.data_ptr(), y32.data_ptr(), M))
    aout = (_lib.GqQtipOut * 1)(_lib.GqQtipOut(y32.data_ptr(), sv.data_ptr(), resid.data_ptr() if resid is not None else None, out.data_ptr(), M))
    st = _lib.current_stream_ptr()
    _lib.check(L.gq_qtip_linear_in(x16.data_ptr(), x2.data_ptr() if x2 is not None else None, normw.data_ptr() if normw is not None else None,
                                   nf.EPS, pro, K, lin.K, 1, ain, 0, None, 1, st), "gq_qtip_linear_in")
    _lib.check(L.gq_qtip_linear_out(1, aout, st), "gq_qtip_linear_out")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("K,M", [(128, 256), (32, 32)])
def test_qtip_linear_prologues_sv_and_residual(K, M):
    lin = _rand_qlinear(K, M, 2, seed=K + M)
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(K, generator=g) * 0.7).half().numpy()
    x2 = torch.randn(K, generator=g).half().numpy()
    nw = (1 + 0.2 * torch.randn(K, generator=g)).half().to(D)
    res = torch.randn(M, generator=g).half().numpy()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(D)  # noqa: E731
    hidden = []
    for pro, kw in ((0, {}), (1, dict(normw=nw)), (2, dict(x2=dev(x2)))):
        base = _linear(lin, dev(x), pro, **kw)
        assert np.isfinite(base.astype(np.float32)).all()
        for tag, xp in nf.poisoned_vectors(x):
            got = _linear(lin, dev(xp), pro, **kw)
            fin = np.isfinite(got.astype(np.float32))
            if fin.any():
                hidden.append(f"prologue {pro} x {tag}: {int(fin.sum())} of {M} outputs finite, first {int(np.flatnonzero(fin)[0])}")
        if pro == 2:   # up +-Inf over a gate of 0: 0 * Inf = NaN at the site
            for pname in ("+inf", "-inf"):
                gz, up = x.copy(), x2.copy()
                gz[3], up[3] = 0, nf.poison(pname)
                got = _linear(lin, dev(gz), pro, x2=dev(up))
                if np.isfinite(got.astype(np.float32)).any():
                    hidden.append(f"prologue 2 up {pname} over a zero gate: finite outputs")
    # one SV entry, one residual element: row r0 only
    r0 = M // 2 + 1
    others = np.arange(M) != r0
    base = _linear(lin, dev(x), resid=dev(res))
    for pname in nf.POISONS:
        rc = np.zeros(M, dtype=np.uint8)
        rc[r0] = nf.classify(nf.poison(pname))
        rp = res.copy()
        rp[r0] = nf.poison(pname)
        b, _ = nf.check(_linear(lin, dev(x), resid=dev(rp)), rc, True, others, base)   # fp16(res + y): the poison's own class
        hidden += [f"residual {pname}: {v}" for v in b]
        # SV scales the transformed sum t of its own row: out[r0] = fp16(t * SV[r0]) + res[r0], so an Inf scale takes t's sign
        sv0 = (lin.SV.float() * 32.0).contiguous()
        t = (float(base[r0]) - float(res[r0])) / float(sv0[r0])
        sv = sv0.clone()
        sv[r0] = float(nf.poison(pname))
        with np.errstate(all="ignore"):
            rc[r0] = nf.classify64(np.array([t * float(nf.poison(pname)) + float(res[r0])]))[0]
        assert t != 0 and rc[r0] != nf.FINITE
        b, _ = nf.check(_linear(lin, dev(x), resid=dev(res), sv=sv), rc, False, others, base)
        hidden += [f"SV {pname}: {v}" for v in b]
    assert not hidden, "%d violation(s):\n%s" % (len(hidden), "\n".join(hidden[:12]))


@pytest.mark.parametrize("S", (1, 17, 33))
def test_qtip_gemm_poisoned_token_row(S):
    from guidedquant_amd import _lib
    from oracle import oracle
    oracle.build()
    L = _lib.lib()
    M, K, R = 256, 512, 2
    comp, tlut, X = _recipe(R, M, K)
    X = X[:S].copy()
    W = oracle.qtip_decode(comp, tlut, M, K, R).astype(np.float64)
    cd, td = torch.from_numpy(comp).to(D), torch.from_numpy(tlut.copy()).to(D)

    def run(X_):
        xd = torch.from_numpy(X_.copy()).to(D)
        out = torch.full((S, M), 1.0, dtype=torch.float32, device=D)
        nb = L.gq_qtip_gemm_ws_bytes(S, M, K, R)
        w = torch.full((max(nb // 4, 4), ), 1.0, dtype=torch.float32, device=D)
        _lib.check(L.gq_qtip_gemm_ws(out.data_ptr(), cd.data_ptr(), xd.data_ptr(), td.data_ptr(), S, M, K, R, w.data_ptr() if nb else None, nb,
                                     _lib.current_stream_ptr()), "gq_qtip_gemm_ws")
        torch.cuda.synchronize()
        return out.cpu().numpy()

    base = run(X)
    assert np.isfinite(base).all()
    r0 = S // 2
    clean = np.zeros((S, M), dtype=bool)
    clean[np.arange(S) != r0] = True
    bad, sub, n = [], 0, 0
    for tag, xp in nf.poisoned_vectors(X[r0]):
        Xp = X.copy()
        Xp[r0] = xp
        with np.errstate(all="ignore"):
            ref = Xp.astype(np.float64) @ W.T
        assert not np.isfinite(ref[r0]).any() and np.isfinite(ref[clean]).all()
        b, s_ = nf.check32(run(Xp), ref, clean, base)
        bad += [f"{tag}: {v}" for v in b]
        sub += s_
        n += int(np.isinf(ref).sum())
    print(f"QTIP GEMM S = {S}: NaN for Inf in {sub} of {n} outputs whose reference is +-Inf")
    assert not bad, "%d violation(s):\n%s" % (len(bad), "\n".join(bad[:12]))


def test_qtip_pretransformed_prologue():
    from guidedquant_amd import _lib
    L = _lib.lib()
    K, M, R = 128, 256, 2
    lin = _rand_qlinear(K, M, R, seed=77)
    g = torch.Generator().manual_seed(9)
    xs = (torch.randn(K, generator=g) / 16).half().numpy()

    def run(v):
        vd = torch.from_numpy(np.ascontiguousarray(v)).to(D)
        y = torch.full((M, ), 1.0, dtype=torch.float32, device=D)
        ain = (_lib.GqQtipIn * 1)(_lib.GqQtipIn(lin.trellis.data_ptr(), None, lin.tlut.data_ptr(), y.data_ptr(), M))
        _lib.check(L.gq_qtip_linear_in(vd.data_ptr(), None, None, 0.0, 3, K, R, 1, ain, 0, None, 1, _lib.current_stream_ptr()), "pre-transformed")
        torch.cuda.synchronize()
        return y.cpu().numpy()

    base = run(xs)
    assert np.isfinite(base).all()
    bad, sub_, n = [], 0, 0
    for k in (0, K - 1, 37):
        hot = np.zeros(K, dtype=np.float16)
        hot[k] = 1
        w = run(hot).astype(np.float64)            # column k of the decoded weights, exact
        rest = xs.copy()
        rest[k] = 0
        r64 = run(rest).astype(np.float64)
        for pname in nf.POISONS:
            xp = xs.copy()
            xp[k] = nf.poison(pname)
            with np.errstate(all="ignore"):
                ref = w * float(nf.poison(pname)) + r64
            assert not np.isfinite(ref).any()
            b, s_ = nf.check32(run(xp), ref)
            bad += [f"xs[{k}] {pname}: {v}" for v in b]
            sub_ += s_
            n += int(np.isinf(ref).sum())
    print(f"QTIP pre-transformed prologue: NaN for Inf in {sub_} of {n} outputs whose reference is +-Inf")
    assert not bad, "%d violation(s):\n%s" % (len(bad), "\n".join(bad[:12]))


def _sylvester(n):
    H = np.array([[1.0]])
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])
    return H


@pytest.mark.parametrize("entry", ("gq_qtip_linear_out", "gq_qtip_linear_out_seg"))
def test_qtip_transform_out_partial_sum_sv_and_residual(entry):
    from guidedquant_amd import _lib
    L = _lib.lib()
    M, parts = 256, 2
    g = torch.Generator().manual_seed(3)
    ys = (torch.randn(parts, M, generator=g) * 3).numpy().astype(np.float32)
    sv = ((torch.randn(M, generator=g) * 0.3 + 1) * 32).numpy().astype(np.float32)
    res = torch.randn(M, generator=g).half().numpy()
    H = _sylvester(M)

    def run(y_, sv_, res_):
        yd, sd, rd = (torch.from_numpy(np.ascontiguousarray(a)).to(D) for a in (y_, sv_, res_))
        o = torch.full((M, ), 1.0, dtype=torch.float16, device=D)
        arr = (_lib.GqQtipOut * 1)(_lib.GqQtipOut(yd.data_ptr(), sd.data_ptr(), rd.data_ptr(), o.data_ptr(), M, parts))
        _lib.check(getattr(L, entry)(1, arr, _lib.current_stream_ptr()), entry)
        torch.cuda.synchronize()
        return o.cpu().numpy()

    def ref(y_, sv_, res_):
        """class of fp16((H y) M^-1/2 * SV) + res in float64: +-1 * Inf keeps Inf's sign times the entry's, any sum with a NaN is NaN"""
        with np.errstate(all="ignore"):
            t = (H * y_.astype(np.float64).sum(axis=0)[None, :]).sum(axis=1) / np.sqrt(M)
            return nf.classify64(t * sv_.astype(np.float64) + res_.astype(np.float64))

    base = run(ys, sv, res)
    assert np.isfinite(base.astype(np.float32)).all()
    bad, sub_, n = [], 0, 0
    r0 = 131
    others = np.arange(M) != r0
    for pname in nf.POISONS:
        pv = float(nf.poison(pname))
        for j in (0, M - 1, 77):
            yp = ys.copy()
            yp[1, j] = pv
            rc = ref(yp, sv, res)
            assert (rc != nf.FINITE).all()
            b, s_ = nf.check(run(yp, sv, res), rc, False)
            bad += [f"partial sum [1, {j}] {pname}: {v}" for v in b]
            sub_ += s_
            n += int(((rc == nf.PINF) | (rc == nf.NINF)).sum())
        rc = np.zeros(M, dtype=np.uint8)
        rp = res.copy()
        rp[r0] = nf.poison(pname)
        rc[r0] = nf.classify(nf.poison(pname))
        b, _ = nf.check(run(ys, sv, rp), rc, False, others, base)
        bad += [f"residual {pname}: {v}" for v in b]
        t = (float(base[r0]) - float(res[r0])) / float(sv[r0])
        sp = sv.copy()
        sp[r0] = pv
        with np.errstate(all="ignore"):
            rc[r0] = nf.classify64(np.array([t * pv + float(res[r0])]))[0]
        b, _ = nf.check(run(ys, sp, res), rc, False, others, base)
        bad += [f"SV {pname}: {v}" for v in b]
    print(f"{entry}: NaN for Inf in {sub_} of {n} outputs whose reference is +-Inf")
    assert not bad, "%d violation(s):\n%s" % (len(bad), "\n".join(bad[:12]))


def _golden_11008():
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "had_n11008.npz"))
    return g, int(g["n"]), int(g["K"]), torch.from_numpy(g["hadK"].astype(np.float32)).to(D).contiguous()


def test_qtip_transform_on_a_factor_width():
    from guidedquant_amd import _lib
    L = _lib.lib()
    g, n, Kf, hk = _golden_11008()
    ones = np.ones(n, dtype=np.float32)
    y0 = np.ascontiguousarray(g["X"][0]).astype(np.float32)

    def out_side(y_, vec_):
        yd, vd = torch.from_numpy(y_.copy()).to(D), torch.from_numpy(vec_.copy()).to(D)
        o = torch.full((n, ), 1.0, dtype=torch.float16, device=D)
        xf = (_lib.GqQtipXf * 1)(_lib.GqQtipXf(yd.data_ptr(), vd.data_ptr(), hk.data_ptr(), None, o.data_ptr()))
        _lib.check(L.gq_qtip_transform(0, None, None, None, 0.0, 0, 1, xf, n, Kf, 0, None), "out side")
        torch.cuda.synchronize()
        return o.cpu().numpy()

    def in_side(x16):
        xd, vd = torch.from_numpy(x16.copy()).to(D), torch.from_numpy(ones).to(D)
        o = torch.full((n, ), 1.0, dtype=torch.float16, device=D)
        xf = (_lib.GqQtipXf * 1)(_lib.GqQtipXf(None, vd.data_ptr(), hk.data_ptr(), None, o.data_ptr()))
        _lib.check(L.gq_qtip_transform(1, xd.data_ptr(), None, None, 0.0, 0, 1, xf, n, Kf, 1, None), "in side")
        torch.cuda.synchronize()
        return o.cpu().numpy()

    base_o, base_i = out_side(y0, ones), in_side(y0.astype(np.float16))
    assert np.isfinite(base_o.astype(np.float32)).all() and np.isfinite(base_i.astype(np.float32)).all() and (base_o != 0).mean() > 0.99
    bad = []
    r0 = 5000
    others = np.arange(n) != r0
    allbad = np.full(n, nf.NAN, dtype=np.uint8)   # (R1 only under exact = False: any non-finite class is accepted for NaN)
    for pname in nf.POISONS:
        pv = float(nf.poison(pname))
        for j in (0, n - 1, 6000):
            yp = y0.copy()
            yp[j] = pv
            bad += [f"out side y32[{j}] {pname}: {v}" for v in nf.check(out_side(yp, ones), allbad, False)[0]]
            xp = y0.astype(np.float16)
            xp[j] = nf.poison(pname)
            bad += [f"in side x[{j}] {pname}: {v}" for v in nf.check(in_side(xp), allbad, False)[0]]
        vp = ones.copy()
        vp[r0] = pv
        rc = np.zeros(n, dtype=np.uint8)
        with np.errstate(all="ignore"):
            rc[r0] = nf.classify64(np.array([float(base_o[r0]) * pv]))[0]
        bad += [f"out side scale[{r0}] {pname}: {v}" for v in nf.check(out_side(y0, vp), rc, False, others, base_o)[0]]
    assert not bad, "%d violation(s):\n%s" % (len(bad), "\n".join(bad[:12]))


def test_qtip_mlp_mid():
    import ctypes
    from guidedquant_amd import _lib
    L = _lib.lib()
    g, n, Kf, hk = _golden_11008()
    parts = 2
    hkT16, hk16 = hk.t().contiguous().half(), hk.half().contiguous()
    gen = torch.Generator().manual_seed(11)
    yg = (torch.randn(parts, n, generator=gen) * 3.0).numpy()
    yu = (torch.randn(parts, n, generator=gen) * 3.0).numpy()
    svg = ((torch.rand(n, generator=gen) + 0.5) * torch.sign(torch.randn(n, generator=gen)) * 32.0 * 0.02).numpy()
    svu = ((torch.rand(n, generator=gen) + 0.5) * torch.sign(torch.randn(n, generator=gen)) * 32.0 * 0.02).numpy()
    sud = torch.sign(torch.randn(n, generator=gen)).to(D)

    def run(yg_, yu_, svg_):
        a, b, c, d_ = (torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).to(D) for t in (yg_, yu_, svg_, svu))
        z = torch.full((n, ), 1.0, dtype=torch.float32, device=D)
        g16 = torch.full((n, ), 1.0, dtype=torch.float16, device=D)
        u16 = torch.full((n, ), 1.0, dtype=torch.float16, device=D)
        mid = _lib.GqQtipMid(a.data_ptr(), b.data_ptr(), c.data_ptr(), d_.data_ptr(), hkT16.data_ptr(), sud.data_ptr(), hk16.data_ptr(),
                             z.data_ptr(), g16.data_ptr(), u16.data_ptr())
        _lib.check(L.gq_qtip_mlp_mid(ctypes.pointer(mid), parts, n, Kf, None), "gq_qtip_mlp_mid")
        torch.cuda.synchronize()
        return z.cpu().numpy(), g16.cpu().numpy(), u16.cpu().numpy()

    bz, bg, bu = run(yg, yu, svg)
    assert np.isfinite(bz).all() and np.isfinite(bg.astype(np.float32)).all() and np.isfinite(bu.astype(np.float32)).all()
    bad = []

    def all_nonfinite(tag, a):
        fin = np.isfinite(np.asarray(a, dtype=np.float32))
        if fin.any():
            bad.append(f"{tag}: {int(fin.sum())} of {a.size} finite, first {int(np.flatnonzero(fin)[0])}")

    def same(tag, a, b):
        if not np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)):
            bad.append(f"{tag}: changed")

    r0 = 64 * 100 + 21
    for pname in nf.POISONS:
        pv = float(nf.poison(pname))
        yp = yg.copy()
        yp[1, 4321] = pv
        z, g16, u16 = run(yp, yu, svg)
        all_nonfinite(f"gate partial {pname}: gate", g16), all_nonfinite(f"gate partial {pname}: z32", z), same(f"gate partial {pname}: up", u16, bu)
        yp = yu.copy()
        yp[0, 17] = pv
        z, g16, u16 = run(yg, yp, svg)
        all_nonfinite(f"up partial {pname}: up", u16), all_nonfinite(f"up partial {pname}: z32", z), same(f"up partial {pname}: gate", g16, bg)
        sp = svg.copy()
        sp[r0] = pv
        z, g16, u16 = run(yg, yu, sp)
        same(f"gate scale {pname}: up", u16, bu)
        same(f"gate scale {pname}: the other gate outputs", np.delete(g16, r0), np.delete(bg, r0))
        all_nonfinite(f"gate scale {pname}: gate[{r0}]", g16[r0:r0 + 1])
        z2, b2 = z.reshape(Kf, 64), bz.reshape(Kf, 64)
        all_nonfinite(f"gate scale {pname}: z32[:, {r0 % 64}]", z2[:, r0 % 64])
        same(f"gate scale {pname}: the other columns of z32", np.delete(z2, r0 % 64, axis=1), np.delete(b2, r0 % 64, axis=1))
    assert not bad, "%d violation(s):\n%s" % (len(bad), "\n".join(bad[:12]))
