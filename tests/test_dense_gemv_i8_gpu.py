"""GPU: the int8 lm_head GEMV (csrc/head_q8.hip::dense_gemv_i8_kernel, gq_dense_gemv_i8) against float64, at the bound of
tests/test_dense_gemv_exact_gpu.py, and with probes whose result is exact.  The mirror of that file for the int8 entry.

    out[n] = fp16( scale[n] * sum_k xn[k] * q[n][k] ),   reference: float64 sum_k xn[k] * (scale[n] * q[n][k])
Bound (the project's own, unchanged: fp32 accumulation, one more fp32 rounding for the scale, one fp16 rounding):
    |got - ref| <= 2^-11 * 1.001 * |ref| + c * sum_k |xn_k| |scale_n q_nk| + 1e-7,      c = 1e-5, with the RMSNorm prologue 2e-5
A dropped or doubled k, a mis-signed byte or another row's scale breaks it by orders of magnitude.  With the prologue the reference
normalises with the kernel's rounding points, exactly as tests/test_dense_gemv_exact_gpu.py::_normalised does (its docstring has the
argument for the second 1e-5).

Shapes: every N of {1, 15, 16, 17, 33, 1000, 3001} against every K of {512, 1024, 3584, 4096, 4608, 8192} (a lane holds 16 weights, a
wave 1024 columns per step: 512 -- half a wave, once; 3584 and 4608 -- a last step of half a wave; 4608 and up: the prologue's loop
behind the two prefetched units) and (64, 81408), the largest K whose activations fit the LDS.  Each under the default plan and with
GQ_DENSE_I8_RPB=16 (many blocks, a ragged last one), with and without the prologue.  `out` lies between 16 NaN guard elements on each
side and is NaN-filled before the launch."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

NS = (1, 15, 16, 17, 33, 1000, 3001)
KS = (512, 1024, 3584, 4096, 4608, 8192)
GUARD = 16
EPS = 1e-5


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(params=["default", "rpb16"])
def plan(request):
    from guidedquant_amd import _lib
    if request.param == "rpb16":
        os.environ["GQ_DENSE_I8_RPB"] = "16"
    _lib.lib().gq_reset_env_cache()
    yield request.param
    os.environ.pop("GQ_DENSE_I8_RPB", None)
    _lib.lib().gq_reset_env_cache()


def _launch(x, q, scale, N, K, nw=None):
    """out fp16 [N] of a launch into a guarded, NaN-filled buffer; asserts the guards"""
    from guidedquant_amd import _lib
    assert q.dtype == torch.int8 and q.is_contiguous() and scale.dtype == torch.float32
    buf = torch.full((N + 2 * GUARD, ), float("nan"), dtype=torch.float16, device=x.device)
    _lib.check(_lib.lib().gq_dense_gemv_i8(x.data_ptr(), q.data_ptr(), scale.data_ptr(), buf.data_ptr() + 2 * GUARD, N, K,
                                           nw.data_ptr() if nw is not None else None, EPS, _lib.current_stream_ptr()), "gq_dense_gemv_i8")
    torch.cuda.synchronize()
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + N:]).all(), "written outside out[0 .. N)"
    return buf[GUARD:GUARD + N].clone()


def _inputs(K, rows):
    """q uniform over -127 .. 127 with both extremes in every row, scale log-uniform in [2^-12, 2^-6], x as in the fp16 test (2 % of
    the channels x 8)"""
    g = torch.Generator()
    g.manual_seed(K)
    q = torch.randint(-127, 128, (rows, K), generator=g, dtype=torch.int32)
    r = torch.arange(rows)
    lo = torch.randint(0, K, (rows, ), generator=g)
    hi = (lo + 1 + torch.randint(0, K - 1, (rows, ), generator=g)) % K   # (another column than lo)
    q[r, lo], q[r, hi] = -127, 127
    scale = torch.exp2(-12.0 + 6.0 * torch.rand(rows, generator=g)).float()
    x = (torch.randn(K, generator=g) * torch.where(torch.rand(K, generator=g) < 0.02, 8.0, 1.0)).half()
    nw = (1 + 0.1 * torch.randn(K, generator=g)).half()
    d = _dev()
    return q.to(torch.int8).to(d), scale.to(d), x.to(d), nw.to(d)


def _normalised(x, nw, K):
    """float64 with the kernel's rounding points"""
    s = (1.0 / torch.sqrt((x.double()**2).sum() / K + EPS)).float()
    return (x.float() * s).half() * nw


def _check(got, xr, q, scale, c):
    W64, x64 = q.double() * scale.double()[:, None], xr.double()
    ref = W64 @ x64
    mag = W64.abs() @ x64.abs()
    err = (got.double() - ref).abs()
    assert torch.isfinite(got.float()).all()
    bound = 2.0**-11 * 1.001 * ref.abs() + c * mag + 1e-7
    print("N %d K %d c %g: largest err / sum|x||w| %.3e, err / bound %.3f" % (q.shape[0], q.shape[1], c, float((err / mag).max()), float((err / bound).max())))
    assert (err <= bound).all(), (q.shape, float((err / (mag + 1e-30)).max()))


@pytest.mark.parametrize("K", KS)
def test_every_row_tail_against_float64(plan, K):
    qall, sall, x, nw = _inputs(K, max(NS))
    xn = _normalised(x, nw, K)
    for N in NS:
        q, s = qall[:N].contiguous(), sall[:N].contiguous()
        _check(_launch(x, q, s, N, K), x, q, s, 1e-5)
        _check(_launch(x, q, s, N, K, nw), xn, q, s, 2e-5)


def test_largest_k_that_fits(plan):
    N, K = 64, 81408
    q, s, x, nw = _inputs(K, N)
    _check(_launch(x, q, s, N, K), x, q, s, 1e-5)
    _check(_launch(x, q, s, N, K, nw), _normalised(x, nw, K), q, s, 2e-5)


def _refused(K, misalign=0):
    from guidedquant_amd import _lib
    d = _dev()
    qb = torch.ones(4 * K + 16, dtype=torch.int8, device=d)
    s = torch.ones(4, dtype=torch.float32, device=d)
    x = torch.ones(K, dtype=torch.float16, device=d)
    out = torch.full((4, ), float("nan"), dtype=torch.float16, device=d)
    rc = _lib.lib().gq_dense_gemv_i8(x.data_ptr(), qb.data_ptr() + misalign, s.data_ptr(), out.data_ptr(), 4, K, None, EPS, _lib.current_stream_ptr())
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused call launched"
    return rc


@pytest.mark.parametrize("K", (81920, 768))
def test_unserved_k_is_refused_without_a_launch(K):
    assert _refused(K) != 0


def test_misaligned_or_null_pointers_are_refused():
    from guidedquant_amd import _lib
    assert _refused(512, misalign=8) == _lib.GQ_EINVAL
    assert _refused(512, misalign=1) == _lib.GQ_EINVAL
    d = _dev()
    q = torch.ones(4, 512, dtype=torch.int8, device=d)
    sb = torch.ones(8, dtype=torch.float32, device=d)
    x = torch.ones(512 + 8, dtype=torch.float16, device=d)
    out = torch.full((4, ), float("nan"), dtype=torch.float16, device=d)
    L, sp = _lib.lib(), _lib.current_stream_ptr()
    assert L.gq_dense_gemv_i8(x.data_ptr(), q.data_ptr(), sb.data_ptr() + 2, out.data_ptr(), 4, 512, None, EPS, sp) == _lib.GQ_EINVAL
    assert L.gq_dense_gemv_i8(x.data_ptr() + 2, q.data_ptr(), sb.data_ptr(), out.data_ptr(), 4, 512, None, EPS, sp) == _lib.GQ_EINVAL
    assert L.gq_dense_gemv_i8(x.data_ptr(), q.data_ptr(), sb.data_ptr(), out.data_ptr(), 4, 512, x.data_ptr() + 2, EPS, sp) == _lib.GQ_EINVAL
    assert L.gq_dense_gemv_i8(x.data_ptr(), None, sb.data_ptr(), out.data_ptr(), 4, 512, None, EPS, sp) == _lib.GQ_EINVAL
    assert L.gq_dense_gemv_i8(x.data_ptr(), q.data_ptr(), None, out.data_ptr(), 4, 512, None, EPS, sp) == _lib.GQ_EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


def _probe_ks(K):
    ks = {0, 1, 7, 8, 9, 15, 16, K - 16, K - 9, K - 8, K - 1}
    for m in range(512, K + 1, 512):
        ks |= {m - 1, m, m + 1}
    return sorted(k for k in ks if 0 <= k < K)


@pytest.mark.parametrize("K", (512, 3584, 8192))
def test_one_hot_x_returns_the_scaled_code(plan, K):
    """x = e_k, no prologue: out[n] = fp16(fp32(scale[n]) * fp32(q[n][k])) bit for bit (one product by 1, sums with zeros, the fp32
    product with the scale rounded once, then the fp16 rounding)"""
    N = 33
    q, s, _, _ = _inputs(K, N)
    q = torch.where(q == 0, torch.full_like(q, 3), q)  # (a zero's sign is not the probe's business)
    for k in _probe_ks(K):
        x = torch.zeros(K, dtype=torch.float16, device=q.device)
        x[k] = 1.0
        got = _launch(x, q, s, N, K)
        want = (s * q[:, k].float()).half()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (K, k)


@pytest.mark.parametrize("N,K", [(17, 512), (3001, 512), (1000, 4096), (33, 3584)])
def test_row_addressing_with_a_diagonal_code(plan, N, K):
    """q[n][k] = 64 only for k == n mod K, scale 2^-7: out[n] = x[n mod K] / 2, exactly (x holds signed even integers below 2048)"""
    d = _dev()
    n = torch.arange(N, device=d)
    q = torch.zeros(N, K, dtype=torch.int8, device=d)
    q[n, n % K] = 64
    s = torch.full((N, ), 2.0**-7, dtype=torch.float32, device=d)
    x = (2 * (((torch.arange(K, device=d) * 7 + 3) % 1019) + 1)).half()
    x = torch.where(torch.arange(K, device=d) % 2 == 0, x, -x)
    assert float(x.abs().max()) < 2048
    got = _launch(x, q, s, N, K)
    assert torch.equal(got.view(torch.int16), (x[n % K] / 2).contiguous().view(torch.int16))


@pytest.mark.parametrize("K", (512, 3584))
def test_all_extreme_codes(plan, K):
    """q = +-127 everywhere, |x| = 8: finite and within the bound"""
    N = 33
    g = torch.Generator()
    g.manual_seed(K + 1)
    d = _dev()
    q = (torch.randint(0, 2, (N, K), generator=g) * 254 - 127).to(torch.int8).to(d)
    x = ((torch.randint(0, 2, (K, ), generator=g) * 2 - 1) * 8.0).half().to(d)
    s = torch.exp2(-12.0 + 6.0 * torch.rand(N, generator=g)).float().to(d)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).half().to(d)
    _check(_launch(x, q, s, N, K), x, q, s, 1e-5)
    _check(_launch(x, q, s, N, K, nw), _normalised(x, nw, K), q, s, 2e-5)


def test_nonfinite_activations():
    """tests/nonfinite_model.py's conventions (as tests/test_nonfinite_gemm_head_gpu.py::test_dense_gemv): a NaN in x gives NaN in every
    output, with and without the prologue; an Inf gives what the float64 model gives row by row -- +-Inf by the sign of the code at that
    column, NaN where the code is 0 or where two infinities of opposite sign meet; behind the prologue (scale 1 / sqrt(Inf) = 0,
    0 * Inf = NaN) every row is NaN.  Classes equal the reference's everywhere (R1, R3 exact)."""
    import halfsweep_model as hs
    import nonfinite_model as nf
    N, K = 33, 3584   # (a tail step of half a wave: nf.placements puts a poison in it)
    q, s, x, nw = _inputs(K, N)
    q[::3, 0], q[1::3, K - 1] = 0, 0       # (rows whose code at a poisoned column is zero: 0 * Inf = NaN)
    tail = nf.placements(K)["tail"]
    q[2::3, tail] = 0
    xh = x.cpu().numpy()
    xh[xh == 0] = np.float16(0.5)
    W64 = q.cpu().numpy().astype(np.float64) * s.cpu().numpy().astype(np.float64)[:, None]
    bad = []
    for with_norm in (False, True):
        w_ = nw if with_norm else None
        seen = set()
        for tag, xp in nf.poisoned_vectors(xh):
            act = nf.activation("norm", xp, nw.cpu().numpy()) if with_norm else xp
            with np.errstate(all="ignore"):
                ref = hs.to_half((W64 * act.astype(np.float64)[None, :]).sum(axis=1))
            rc = nf.classify(ref)
            assert (rc != nf.FINITE).all()
            if "nan" in tag or with_norm:
                assert (rc == nf.NAN).all(), tag
            seen |= set(int(v) for v in rc)
            got = _launch(torch.from_numpy(xp).to(q.device), q, s, N, K, w_).cpu().numpy()
            b, _ = nf.check(got, rc, True)
            bad += [f"norm {with_norm} x {tag}: {v}" for v in b]
        assert with_norm or seen == {nf.PINF, nf.NINF, nf.NAN}, "the cases do not reach every class"
    assert not bad, "%d violation(s):\n%s" % (len(bad), "\n".join(bad[:12]))
