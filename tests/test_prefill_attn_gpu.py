"""GPU: the prompt attention kernel (csrc/prefill_attn.hip) through the C ABI -- gq_attn_prefill on guard-banded, poisoned buffers
(tests/guarded.py), against the host models of tests/prefill_attn_model.py.

  count     every attended cache row exactly once for every query row, at every S x window pair of the grid
            S in {1, BQ - 1, BQ, BQ + 1, 2 BQ + 3} x window in {0, 1, 2, BK - 1, BK, BK + 1, T + 7}, start in {0, 1, BK - 1, BK, BK + 5},
            max_seq in {T, T + 3}, head_dim in {64, 128} (prefill_attn_model.covering_cases: 35 cases, two launches each)
            and at a far start: S = BQ + 1, start in {2^17 - BK + 5, 2^17} x window in {0, BK + 1, 4099, T + 7}, max_seq in {T, T + 3},
            head_dim in {64, 128} (prefill_attn_model.long_count_cases: 8 cases, two launches each) -- a first key tile kt0 = klo / BK
            of about 2000, the tile skipping and the size_t row arithmetic there; window 0 walks 2049 tiles per block through the
            register prefetch.  The sums are integers below 2^24 (times the power of two P is rounded at): exact.
  profiles  the online softmax's rescale paths and random data against float64, elementwise
                |got - want| <= (4 * 2^-11 + (T / 32 + T / 64) * 2^-24) * max|V|        (prefill_attn_model.error_bound)
            P rounded to fp16 costs 2^-11 relative in the numerator and at most as much in the normaliser, the output's own fp16
            rounding 2^-11 -- together under 4 * 2^-11; the second term is the worst-case chain of fp32 roundings of the MFMA
            accumulator (one per 32 keys) and of a lane's normaliser share (one per key tile), 5.6e-7 at the 200 keys of the short
            cases.  Short: 200 keys, three head geometries, windows 0 and BK + 1.  Long: S = BQ + 3, start = T - S, every profile plus
            sink_first / sink_last (one key at score 0, T - 1 keys at a weight of 0.9 * 2^-25, V = -2 / +2) at
            (H, Hkv, hd, T) = (2, 1, 128, 2^17 + 69) with window 0 and (2, 1, 64, 2^18 + 69) with windows 0 and 4099; the float64
            reference runs on the device.  torch SDPA's error on the same inputs is printed next to the kernel's (recorded, not
            asserted).
            sink_first is the case the kernel failed while it rounded P to fp16 at scale 1 (every tail weight flushed to 0 in the
            numerator, kept in the fp32 normaliser).  Measured on an MI355X, |got - want| / max|V| (max|V| = 2), worst of the long cases:
                                        T = 2^17 + 69 (hd 128)    T = 2^18 + 69 (hd 64), W 0 / W 4099     bound
              sink_first, scale 1       3.59e-3  (fails)          6.60e-3 (fails) / 7.5e-14               2.32e-3 / 2.69e-3
              sink_first, scale 2^15    3.21e-4                   1.22e-3 / 7.5e-14                         (torch SDPA: 3.59e-3, 7.09e-3)
              sink_last                 1.70e-4                   2.40e-4 / 2.19e-4
              ramp_up / ramp_down       1.52e-5 / 1.16e-5         8.8e-6 / 9.2e-6, 9.5e-6 / 1.26e-5
              hi300 / lo300             2.4e-6 / 2.4e-6           1.3e-6 / 9.1e-6 both
              stairs_first / _last      1.9e-6 / 1.9e-6           1.9e-6 / 1.51e-5 both
              cur_above / cur_below     2.3e-6 / 2.3e-6           1.4e-6 / 1.12e-5 both
            (the CPU emulation, prefill_attn_model.emulate_row, gives 3.41e-3 for sink_first at scale 1 and 2^17 + 69 keys; sink_last measured the same at both
            scales; apart from sink_first the figures equal SDPA's to two digits.)  Wall time on an MI355X: every long
            case under 0.3 s (count probe, two launches of up to 67 MB caches: 0.27 s; profile at 2^18 + 69 keys: 0.21 s).
  unsupported shapes return GQ_ENOTSUP and write nothing.
Cache rows >= T hold NaN / +-Inf / 65504 (attn_probes.POISON_BITS); rows of [0, T) no query attends hold 65504 in the count probe."""
import math

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import attn_probes  # noqa: E402
import prefill_attn_model as pam  # noqa: E402
from guarded import Guards  # noqa: E402


def _L():
    from guidedquant_amd import _lib
    return _lib


BQ, BK = 64, 64  # (asserted against the library's published tile sizes below)


def test_published_tile_sizes():
    L = _L()
    assert (L.PREFILL_ATTN_BQ, L.PREFILL_ATTN_BK) == (BQ, BK)
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "gq_hip.h")).read()
    assert int(re.search(r"#define GQ_PREFILL_ATTN_BQ (\d+)", hdr).group(1)) == BQ and int(re.search(r"#define GQ_PREFILL_ATTN_BK (\d+)", hdr).group(1)) == BK


def _launch(q, K, V, S, start, H, Hkv, hd, scale, window):
    L = _L()
    g = Guards()
    bq, bk, bv = g.inp("q", q), g.inp("k_cache", K), g.inp("v_cache", V)
    bo = g.out("out", S * H * hd * 2)
    rc = L.lib().gq_attn_prefill(bq.ptr(), bk.ptr(), bv.ptr(), bo.ptr(), S, start, H, Hkv, hd, K.shape[1], scale, window, None)
    g.check()
    return rc, bo.view(torch.float16, (S, H * hd)).clone()


CASES = pam.covering_cases(BQ, BK)


@pytest.mark.parametrize("S,start,window,slack,hd", CASES, ids=["S%d-start%d-W%d-slack%d-hd%d" % c for c in CASES])
def test_count_probe_every_attended_row_once(S, start, window, slack, hd):
    H, Hkv = 4, 2
    T = start + S
    for coarse in (False, True):
        q, K, V, expect = pam.count_probe(H, Hkv, hd, S, start, window, T + slack, coarse)
        rc, out = _launch(q, K, V, S, start, H, Hkv, hd, attn_probes.default_scale(hd), window)
        assert rc == 0, _L().lib().gq_last_error()
        assert torch.isfinite(out.float()).all(), "not finite"
        d = attn_probes.ulp_distance(out.cpu(), expect)
        worst = int(d.max())
        if worst > 1:
            i, e = divmod(int(d.argmax()), H * hd)
            raise AssertionError("count probe (coarse %s): query row %d, element %d is %r, expected %r (%d fp16 steps)" %
                                 (coarse, i, e, float(out[i, e]), float(expect[i, e]), worst))


_HEADS = [(4, 4, 64), (8, 2, 128), (7, 1, 128)]
_ERRS = []


@pytest.mark.parametrize("window", [0, BK + 1])
@pytest.mark.parametrize("H,Hkv,hd", _HEADS, ids=["H%d-Hkv%d-hd%d" % h for h in _HEADS])
@pytest.mark.parametrize("name", attn_probes.PROFILES + ("random",))
def test_profiles_against_float64(name, H, Hkv, hd, window):
    import torch.nn.functional as F
    S, start = 2 * BQ + 3, BK + 5  # 200 keys: four key tiles, three query tiles, an offset off the tile grid
    T = start + S
    scale = attn_probes.default_scale(hd)
    q, K, V = pam.profile_probe(name, H, Hkv, hd, S, start, T + 3, scale, BK)
    want = pam.reference(q, K, V, start, scale, window)
    rc, out = _launch(q, K, V, S, start, H, Hkv, hd, scale, window)
    assert rc == 0, _L().lib().gq_last_error()
    got = out.cpu().double()
    assert torch.isfinite(got).all()
    vmax = float(V[:, :T].float().abs().max())
    err = float((got - want).abs().max())
    # torch SDPA on the same fp16 inputs, explicit mask: recorded next to the kernel's figure
    G = H // Hkv
    d = torch.device("cuda:0")
    m = pam.attend_mask(S, start, T, window).to(d)[None, None]
    kd, vd = K[:, :T].to(d).repeat_interleave(G, dim=0)[None], V[:, :T].to(d).repeat_interleave(G, dim=0)[None]
    y = F.scaled_dot_product_attention(q.to(d)[None], kd, vd, attn_mask=m, dropout_p=0.0, scale=scale)
    sdpa_err = float((y[0].transpose(0, 1).reshape(S, H * hd).cpu().double() - want).abs().max())
    bound = pam.error_bound(T, vmax)
    print("%s H%d/%d hd%d W%d: max|V| %.3f  kernel %.3e  SDPA %.3e  bound %.3e" % (name, H, Hkv, hd, window, vmax, err, sdpa_err, bound))
    assert err <= bound, (name, err, bound)


LONG_COUNT = pam.long_count_cases(BQ, BK)


@pytest.mark.parametrize("S,start,window,slack,hd", LONG_COUNT, ids=["S%d-start%d-W%d-slack%d-hd%d" % c for c in LONG_COUNT])
def test_count_probe_at_a_far_start(S, start, window, slack, hd):
    H, Hkv = 4, 2
    T = start + S
    for coarse in (False, True):
        q, K, V, expect = pam.count_probe(H, Hkv, hd, S, start, window, T + slack, coarse)
        rc, out = _launch(q, K, V, S, start, H, Hkv, hd, attn_probes.default_scale(hd), window)
        assert rc == 0, _L().lib().gq_last_error()
        assert torch.isfinite(out.float()).all(), "not finite"
        d = attn_probes.ulp_distance(out.cpu(), expect)
        worst = int(d.max())
        if worst > 1:
            i, e = divmod(int(d.argmax()), H * hd)
            raise AssertionError("count probe (coarse %s): query row %d, element %d is %r, expected %r (%d fp16 steps)" %
                                 (coarse, i, e, float(out[i, e]), float(expect[i, e]), worst))


_LONG = [(H, Hkv, hd, T, w) for H, Hkv, hd, T, wins in pam.LONG_PROFILE_CASES for w in wins]


@pytest.mark.parametrize("H,Hkv,hd,T,window", _LONG, ids=["H%d-Hkv%d-hd%d-T%d-W%d" % c for c in _LONG])
@pytest.mark.parametrize("name", attn_probes.PROFILES + pam.SINK_PROFILES)
def test_profiles_against_float64_at_long_T(name, H, Hkv, hd, T, window):
    import torch.nn.functional as F
    S = BQ + 3
    start = T - S
    scale = attn_probes.default_scale(hd)
    q, K, V = pam.profile_probe(name, H, Hkv, hd, S, start, T + 3, scale, BK)
    d = torch.device("cuda:0")
    qd, Kd, Vd = q.to(d), K[:, :T].to(d), V[:, :T].to(d)
    want = pam.reference(qd, Kd, Vd, start, scale, window).cpu()  # (float64 on the device)
    rc, out = _launch(q, K, V, S, start, H, Hkv, hd, scale, window)
    assert rc == 0, _L().lib().gq_last_error()
    got = out.cpu().double()
    assert torch.isfinite(got).all()
    vmax = float(V[:, :T].float().abs().max())
    err = float((got - want).abs().max())
    G = H // Hkv
    m = pam.attend_mask(S, start, T, window).to(d)[None, None]
    y = F.scaled_dot_product_attention(qd[None], Kd.repeat_interleave(G, dim=0)[None], Vd.repeat_interleave(G, dim=0)[None], attn_mask=m, dropout_p=0.0,
                                       scale=scale)
    sdpa_err = float((y[0].transpose(0, 1).reshape(S, H * hd).cpu().double() - want).abs().max())
    bound = pam.error_bound(T, vmax)
    print("%s H%d/%d hd%d T%d W%d: max|V| %.3f  kernel %.3e  SDPA %.3e  bound %.3e" % (name, H, Hkv, hd, T, window, vmax, err, sdpa_err, bound))
    assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("H,Hkv,hd", [(4, 2, 96), (6, 4, 64), (4, 2, 32)])
def test_unsupported_shape_is_declined_and_writes_nothing(H, Hkv, hd):
    L = _L()
    assert L.lib().gq_attn_prefill_supported(H, Hkv, hd) == 0
    S, start = 5, 2
    T = start + S
    g = torch.Generator().manual_seed(0)
    q = torch.randn(H, S, hd, generator=g).half()
    K = torch.randn(Hkv, T, hd, generator=g).half()
    V = torch.randn(Hkv, T, hd, generator=g).half()
    rc, out = _launch(q, K, V, S, start, H, Hkv, hd, 1.0 / math.sqrt(hd), 0)
    assert rc == L.GQ_ENOTSUP
    assert bool((out.view(torch.int16) == 0x7E7E).all())  # the poison pattern, untouched


def test_supported_shapes_and_argument_checks():
    L = _L()
    for H, Hkv, hd in ((4, 4, 64), (8, 2, 128), (7, 1, 128), (28, 4, 128)):
        assert L.lib().gq_attn_prefill_supported(H, Hkv, hd) == 1
    # start + S beyond the cache: a bad argument, nothing launched
    q = torch.zeros(2, 4, 64, dtype=torch.float16)
    K = torch.zeros(1, 5, 64, dtype=torch.float16)
    rc, out = _launch(q, K, K.clone(), 4, 2, 2, 1, 64, 0.125, 0)
    assert rc == L.GQ_EINVAL and bool((out.view(torch.int16) == 0x7E7E).all())
