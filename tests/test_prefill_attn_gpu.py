"""GPU: the prompt attention kernel (csrc/prefill_attn.hip) through the C ABI -- gq_attn_prefill on guard-banded, poisoned buffers
(tests/guarded.py), against the host models of tests/prefill_attn_model.py.

  count     every attended cache row exactly once for every query row, at every S x window pair of the grid
            S in {1, BQ - 1, BQ, BQ + 1, 2 BQ + 3} x window in {0, 1, 2, BK - 1, BK, BK + 1, T + 7}, start in {0, 1, BK - 1, BK, BK + 5},
            max_seq in {T, T + 3}, head_dim in {64, 128} (prefill_attn_model.covering_cases: 35 cases, two launches each)
  profiles  the online softmax's rescale paths and random data against float64, elementwise |got - want| <= 2^-9 max|V|:
            P rounded to fp16 costs 2^-11 relative in the numerator and at most as much in the normaliser, the output's own fp16
            rounding 2^-11 -- together under 4 * 2^-11 -- and fp32 accumulation over at most 400 keys adds under 3e-5.  torch SDPA's
            error on the same inputs is printed next to the kernel's (recorded, not asserted).
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
    print("%s H%d/%d hd%d W%d: max|V| %.3f  kernel %.3e  SDPA %.3e  bound %.3e" % (name, H, Hkv, hd, window, vmax, err, sdpa_err, 2.0**-9 * vmax))
    assert err <= 2.0**-9 * vmax, (name, err, 2.0**-9 * vmax)


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
