"""GPU: the dense fp16 GEMV of the lm_head (csrc/decode.hip::dense_gemv_kernel, gq_dense_gemv_f16) against float64, at the bound of
the project's GEMM tests, and with probes whose result is exact.

Bound (tests/test_ap_gemm_gpu.py::_check: fp32 accumulation, one fp16 rounding):
    |got - ref| <= 2^-11 * 1.001 * |ref| + c * sum_k |x_k| |W_nk| + 1e-7,      c = 1e-5, with the RMSNorm prologue 2e-5
One dropped or doubled k costs about 1 / K of the sum (2e-4 at K = 5120): ten times the second term.  With the prologue the reference
normalises with the kernel's rounding points -- the statistic rounded to fp32, x * scale rounded to fp16, the fp16 product with the
weight; the device adds the squares in another order, so its fp32 scale may differ by an ulp and flip a normalised value by one or two
fp16 ulps where it sat on a rounding boundary (at most 0.1 % of them, tests/test_prefill_native_gpu.py::test_rmsnorm_rows): at most
1e-3 * 2^-10 ~ 1e-6 of the sum, which the second 1e-5 holds tenfold.

Shapes: every N of {1, 15, 16, 17, 33, 1000, 3001} (a block is 4 waves x 4 rows: tails of every kind; rows past N are read clamped
to N - 1 and never written) against every K of {512, 1024, 4096, 4608, 5120, 8192} (512: three quarters of the threads hold no unit
of x; 4608 and up: the prologue's loop over the units behind the two prefetched ones), and (64, 81408), the largest K whose
activations fit the LDS.  Each under the default plan and with GQ_DENSE_RPB=16 (many blocks, a ragged last one).  `out` lies between
16 NaN guard elements on each side."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NS = (1, 15, 16, 17, 33, 1000, 3001)
KS = (512, 1024, 4096, 4608, 5120, 8192)
GUARD = 16
EPS = 1e-5


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(params=["default", "rpb16"])
def plan(request):
    from guidedquant_amd import _lib
    if request.param == "rpb16":
        os.environ["GQ_DENSE_RPB"] = "16"
    _lib.lib().gq_reset_env_cache()
    yield request.param
    os.environ.pop("GQ_DENSE_RPB", None)
    _lib.lib().gq_reset_env_cache()


def _launch(x, W, N, K, nw=None):
    """out fp16 [N] of a launch into a guarded, NaN-filled buffer; asserts the guards"""
    from guidedquant_amd import _lib
    buf = torch.full((N + 2 * GUARD, ), float("nan"), dtype=torch.float16, device=x.device)
    _lib.check(_lib.lib().gq_dense_gemv_f16(x.data_ptr(), W.data_ptr(), buf.data_ptr() + 2 * GUARD, N, K, nw.data_ptr() if nw is not None else None,
                                            EPS, _lib.current_stream_ptr()), "gq_dense_gemv_f16")
    torch.cuda.synchronize()
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + N:]).all(), "written outside out[0 .. N)"
    return buf[GUARD:GUARD + N].clone()


def _inputs(K, rows):
    g = torch.Generator()
    g.manual_seed(K)
    W = (torch.randn(rows, K, generator=g) * 0.02).half()
    x = (torch.randn(K, generator=g) * torch.where(torch.rand(K, generator=g) < 0.02, 8.0, 1.0)).half()
    nw = (1 + 0.1 * torch.randn(K, generator=g)).half()
    d = _dev()
    return W.to(d), x.to(d), nw.to(d)


def _normalised(x, nw, K):
    """float64 with the kernel's rounding points"""
    scale = (1.0 / torch.sqrt((x.double()**2).sum() / K + EPS)).float()
    return (x.float() * scale).half() * nw


def _check(got, xr, W, c):
    W64, x64 = W.double(), xr.double()
    ref = W64 @ x64
    scale = W64.abs() @ x64.abs()
    err = (got.double() - ref).abs()
    assert torch.isfinite(got.float()).all()
    bound = 2.0**-11 * 1.001 * ref.abs() + c * scale + 1e-7
    print("N %d K %d c %g: largest err / sum|x||w| %.3e, err / bound %.3f" % (W.shape[0], W.shape[1], c, float((err / scale).max()), float((err / bound).max())))
    assert (err <= bound).all(), (W.shape, float((err / (scale + 1e-30)).max()))


@pytest.mark.parametrize("K", KS)
def test_every_row_tail_against_float64(plan, K):
    Wall, x, nw = _inputs(K, max(NS))
    xn = _normalised(x, nw, K)
    for N in NS:
        W = Wall[:N].contiguous()
        _check(_launch(x, W, N, K), x, W, 1e-5)
        _check(_launch(x, W, N, K, nw), xn, W, 2e-5)


def test_largest_k_that_fits(plan):
    N, K = 64, 81408
    W, x, nw = _inputs(K, N)
    _check(_launch(x, W, N, K), x, W, 1e-5)
    _check(_launch(x, W, N, K, nw), _normalised(x, nw, K), W, 2e-5)


@pytest.mark.parametrize("K", (81920, 768))
def test_unserved_k_is_refused_without_a_launch(K):
    from guidedquant_amd import _lib
    d = _dev()
    W = torch.ones(4, K, dtype=torch.float16, device=d)
    x = torch.ones(K, dtype=torch.float16, device=d)
    out = torch.full((4, ), float("nan"), dtype=torch.float16, device=d)
    rc = _lib.lib().gq_dense_gemv_f16(x.data_ptr(), W.data_ptr(), out.data_ptr(), 4, K, None, EPS, _lib.current_stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and torch.isnan(out).all()


def _probe_ks(K):
    ks = {0, 1, 7, 8, 9, 15, 16, K - 16, K - 9, K - 8, K - 1}
    for m in range(512, K + 1, 512):
        ks |= {m - 1, m, m + 1}
    return sorted(k for k in ks if 0 <= k < K)


@pytest.mark.parametrize("K", (512, 4608, 8192))
def test_one_hot_x_returns_the_weight_column(plan, K):
    """x = e_k: without the prologue out[n] is W[n][k] bit for bit (one product by 1, sums with zeros, no rounding); with it
    W[n][k] * nw[k] / sqrt(1 / K + eps) to 2^-9 (three fp16 roundings: the scale, its product with the weight, the output)"""
    N = 33
    W, _, nw = _inputs(K, N)
    W = torch.where(W == 0, torch.full_like(W, 0.02), W)  # (a zero's sign is not the probe's business)
    for k in _probe_ks(K):
        x = torch.zeros(K, dtype=torch.float16, device=W.device)
        x[k] = 1.0
        got = _launch(x, W, N, K)
        assert torch.equal(got.view(torch.int16), W[:, k].contiguous().view(torch.int16)), (K, k)
        got = _launch(x, W, N, K, nw).double()
        ref = W[:, k].double() * nw[k].double() / np.sqrt(1.0 / K + EPS)
        assert ((got - ref).abs() <= 2.0**-9 * ref.abs() + 1e-7).all(), (K, k)


@pytest.mark.parametrize("N,K", [(17, 512), (3001, 512), (1000, 4096), (33, 4608)])
def test_row_addressing_with_a_diagonal_weight(plan, N, K):
    """W[n][k] = 1 only for k == n mod K: out[n] = x[n mod K], exactly (x holds integers below 2048)"""
    d = _dev()
    n = torch.arange(N, device=d)
    W = torch.zeros(N, K, dtype=torch.float16, device=d)
    W[n, n % K] = 1.0
    x = (((torch.arange(K, device=d) * 7 + 3) % 2039) + 1).half()
    x = torch.where(torch.arange(K, device=d) % 2 == 0, x, -x)
    got = _launch(x, W, N, K)
    assert torch.equal(got.view(torch.int16), x[n % K].contiguous().view(torch.int16))
