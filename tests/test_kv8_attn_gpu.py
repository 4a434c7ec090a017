"""GPU: the attention launches over an fp8 (e4m3) KV cache -- gq_attn_decode_roped_kv8 (csrc/decode.hip, attn_roped_kernel<.., KV8>) and
gq_attn_prefill_kv8 (csrc/prefill_attn.hip) -- through the C ABI on guard-banded buffers (tests/guarded.py).

  bit identity   every e4m3 value is an fp16 value, and a power of two moves through the arithmetic exactly: with scales 1.0 and with
                 power-of-two scales (2^-3 | 1 for K, 2^2 | 2^-1 for V, mixed per head) the launch equals gq_attn_decode_roped / _window
                 (gq_attn_prefill) on an fp16 cache that holds code * scale, BIT FOR BIT -- the launches tests/test_attn_probes_gpu.py,
                 test_attn_window_gpu.py and test_prefill_attn_gpu.py already pin.
  count          K = 0, V one-hot (both are codes): every attended row exactly once.  A wrong byte stride shows here.
  free scales    against float64 over the dequantised values, with the bounds the fp16 launches are held to (dequantisation is exact,
                 the error budget is the same): attn_probes.PROFILE_C on (err - 2^-10 |ref|) / A for the decode launch
                 (test_attn_probes_gpu.py), prefill_attn_model.error_bound(T, max|V scale|) for the prompt kernel (test_prefill_attn_gpu.py).
Cache contents: random bytes without 0x7f / 0xff; rows no query may read hold 0x7f (NaN) and 0x7e (448) alternating.
Positions of the decode launches: attn_probes.geometry(hd, pos, n_split).boundary for pos in {0, 31, 32, PASS, 2 PASS, 2 PASS + 1,
4 PASS + 5}, n_split in {1, 4, 8}, window in {0, 1, PASS + 3, >= max_seq}."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import attn_probes as ap  # noqa: E402
import kv8_model as k8  # noqa: E402
import prefill_attn_model as pam  # noqa: E402
from guarded import Guards  # noqa: E402

HEADS_IDS = ["H%d-Hkv%d-hd%d" % h for h in k8.HEADS]
SPLITS = (1, 4, 8)
# (S, start, window); the last one at a far start: S = BQ + 3 behind 2^17 cached rows, a window over 65 key tiles
PREFILL_CASES = [(1, 0, 0), (65, 0, 0), (70, 59, 0), (64, 64, 24), (17, 130, 70), (67, 2**17, 4099)]


def _L():
    from guidedquant_amd import _lib
    return _lib


def _dev():
    return torch.device("cuda:0")


def _pass(hd):
    return ap.geometry(hd, 0, 1).PASS


def _max_seq(hd):
    return 4 * _pass(hd) + 5 + 11


def _windows(hd):
    return (0, 1, _pass(hd) + 3, _max_seq(hd) + 7)


def _positions(hd, n_split):
    P = _pass(hd)
    out = set()
    for pos in (0, 31, 32, P, 2 * P, 2 * P + 1, 4 * P + 5):
        out |= set(ap.geometry(hd, pos, n_split).boundary)
    return sorted(out)


def _lo(pos, window):
    return pos + 1 - window if window and pos + 1 > window else 0


_pools = {}


def _codes(Hkv, hd, which, max_code):
    """the random caches of a head geometry (CPU, uint8 [Hkv, max_seq, hd]), generated once"""
    key = (Hkv, hd, which, max_code)
    if key not in _pools:
        g = torch.Generator().manual_seed(7 + hd + 13 * Hkv + (0 if which == "k" else 1))
        _pools[key] = k8.random_codes((Hkv, _max_seq(hd), hd), g, max_code)
    return _pools[key]


def _q(H, hd):
    key = ("q", H, hd)
    if key not in _pools:
        _pools[key] = (torch.randn(H, hd, generator=torch.Generator().manual_seed(3 + H)) * 0.05).half()
    return _pools[key]


def _with_stale(codes, lo, pos):
    c = codes.clone()
    n, hd = c.shape[1], c.shape[2]
    if lo > 0:
        c[:, :lo] = k8.stale_rows(lo, hd)
    if n > pos + 1:
        c[:, pos + 1:] = k8.stale_rows(n - pos - 1, hd)
    return c


def _decode8(L, _lib, q, Kc, Vc, ks, vs, pos, H, Hkv, hd, ns, window, max_seq=None):
    """one gq_attn_decode_roped_kv8 launch on guarded buffers: (rc, out fp16 [H, hd] (poison where unwritten), guards)"""
    max_seq = Kc.shape[1] if max_seq is None else max_seq
    g = Guards()
    bq, bp, bk, bv = g.inp("q", q), g.inp("pos", torch.tensor([pos], dtype=torch.int32)), g.inp("k_cache", Kc), g.inp("v_cache", Vc)
    bks, bvs = g.inp("k_scale", ks), g.inp("v_scale", vs)
    out = g.out("out", H * hd * 2)
    ws = g.out("ws", H * ns * (hd + 2) * 4) if ns > 1 else None
    rc = L.gq_attn_decode_roped_kv8(bq.ptr(), bp.ptr(), bk.ptr(), bv.ptr(), bks.ptr(), bvs.ptr(), out.ptr(), H, Hkv, hd, max_seq, ap.default_scale(hd), ns,
                                    ws.ptr() if ws is not None else None, window, _lib.current_stream_ptr())
    g.check()
    return rc, out.view(torch.float16, (H, hd)).clone(), g


def _decode16(L, _lib, q, K16, V16, pos, H, Hkv, hd, ns, window):
    d = _dev()
    out = torch.full((H, hd), float("nan"), dtype=torch.float16, device=d)
    ws = torch.full((H * ns * (hd + 2),), float("nan"), dtype=torch.float32, device=d)
    posd = torch.tensor([pos], dtype=torch.int32, device=d)
    args = (q.data_ptr(), posd.data_ptr(), K16.data_ptr(), V16.data_ptr(), out.data_ptr(), H, Hkv, hd, K16.shape[1], ap.default_scale(hd), ns,
            ws.data_ptr() if ns > 1 else None)
    if window:
        rc = L.gq_attn_decode_roped_window(*args, window, _lib.current_stream_ptr())
    else:
        rc = L.gq_attn_decode_roped(*args, _lib.current_stream_ptr())
    _lib.check(rc, "fp16 launch")
    torch.cuda.synchronize()
    return out


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("scales", ["ones", "pow2"])
@pytest.mark.parametrize("H,Hkv,hd", k8.HEADS, ids=HEADS_IDS)
def test_decode_launch_equals_the_fp16_launch_bit_for_bit(H, Hkv, hd, scales):
    _lib = _L()
    L = _lib.lib()
    ks, vs = k8.scale_sets(Hkv)[scales]
    q = _q(H, hd)
    qd = q.to(_dev())
    n = 0
    for window in _windows(hd):
        for ns in SPLITS:
            for pos in _positions(hd, ns):
                lo = _lo(pos, window)
                Kc, Vc = _with_stale(_codes(Hkv, hd, "k", 0x7E), lo, pos), _with_stale(_codes(Hkv, hd, "v", 0x7E), lo, pos)
                K16, V16 = k8.dequant(Kc, ks).half().to(_dev()), k8.dequant(Vc, vs).half().to(_dev())  # (code * 2^k: exact in fp16)
                rc, got, _ = _decode8(L, _lib, q, Kc, Vc, ks, vs, pos, H, Hkv, hd, ns, window)
                _lib.check(rc, "gq_attn_decode_roped_kv8")
                want = _decode16(L, _lib, qd, K16, V16, pos, H, Hkv, hd, ns, window)
                assert torch.isfinite(want.float()).all(), (window, ns, pos)
                assert torch.equal(_bits(got), _bits(want)), "window %d n_split %d pos %d: %d element(s) differ, worst %d fp16 steps" % (
                    window, ns, pos, int((_bits(got) != _bits(want)).sum()), int(ap.ulp_distance(got, want).max()))
                n += 1
    print("H%d/%d hd%d %s: %d launches bit-identical" % (H, Hkv, hd, scales, n))


@pytest.mark.parametrize("H,Hkv,hd", k8.HEADS, ids=HEADS_IDS)
def test_decode_count_probe_every_attended_row_once(H, Hkv, hd):
    _lib = _L()
    L = _lib.lib()
    one = torch.ones(Hkv)
    max_seq = _max_seq(hd)
    for window in (0, _pass(hd) + 3):
        for ns in SPLITS:
            for pos in _positions(hd, ns):
                lo = _lo(pos, window)
                p = ap.count_probe(H, Hkv, hd, pos, max_seq)
                Vc = _with_stale(torch.where(p.V == 1.0, k8.ONE_CODE, 0).to(torch.uint8), lo, pos)
                Kc = _with_stale(torch.zeros_like(Vc), lo, pos)
                rc, got, _ = _decode8(L, _lib, p.q, Kc, Vc, one, one, pos, H, Hkv, hd, ns, window)
                _lib.check(rc, "gq_attn_decode_roped_kv8")
                cnt = p.V[:, lo:pos + 1].double().sum(1) / (pos + 1 - lo)
                expect = cnt.repeat_interleave(H // Hkv, dim=0).half()
                ap.check_exact(got.cpu(), p._replace(expect=expect))


@pytest.mark.parametrize("H,Hkv,hd", k8.HEADS, ids=HEADS_IDS)
def test_decode_launch_with_free_scales_against_float64(H, Hkv, hd):
    _lib = _L()
    L = _lib.lib()
    ks, vs = k8.scale_sets(Hkv)["free"]
    q = _q(H, hd)
    P = _pass(hd)
    worst = -1.0
    for window in (0, P + 3):
        for ns in SPLITS:
            for pos in (0, 31, 32, P, 2 * P, 2 * P + 1, 4 * P + 5):
                lo = _lo(pos, window)
                Kc, Vc = _with_stale(_codes(Hkv, hd, "k", 0x7E), lo, pos), _with_stale(_codes(Hkv, hd, "v", 0x7E), lo, pos)
                rc, got, _ = _decode8(L, _lib, q, Kc, Vc, ks, vs, pos, H, Hkv, hd, ns, window)
                _lib.check(rc, "gq_attn_decode_roped_kv8")
                # float64 over the dequantised rows [lo, pos] (the read rule: code * fp32 scale), the criterion of attn_probes.profile_ratio
                Kd, Vd = k8.dequant(Kc, ks, torch.float64)[:, lo:], k8.dequant(Vc, vs, torch.float64)[:, lo:]
                ref, _, A = ap.reference(q, Kd, Vd, pos - lo, ap.default_scale(hd))
                o = got.cpu().double()
                assert torch.isfinite(o).all(), (window, ns, pos)
                # (err - 2^-10 |ref|) / A <= c, multiplied out: an element whose attended V values are all zero has A = 0 and must be exact
                excess = (o - ref).abs() - 2.0**-10 * ref.abs()
                assert bool((excess <= ap.PROFILE_C * A).all()), (window, ns, pos, float((excess - ap.PROFILE_C * A).max()))  # tests/test_attn_probes_gpu.py:193
                worst = max(worst, float((excess / A)[A > 0].max()))
    print("H%d/%d hd%d: worst profile ratio %.3e (c = %.3e)" % (H, Hkv, hd, worst, ap.PROFILE_C))


@pytest.mark.parametrize("H,Hkv,hd", k8.HEADS, ids=HEADS_IDS)
def test_decode_past_the_cache_gives_nan_and_leaves_the_caches(H, Hkv, hd):
    _lib = _L()
    L = _lib.lib()
    one = torch.ones(Hkv)
    Kc, Vc = _codes(Hkv, hd, "k", 0x7E)[:, :40].contiguous(), _codes(Hkv, hd, "v", 0x7E)[:, :40].contiguous()
    for ns in (1, 4):
        for pos in (40, 41, 2**31 - 1):
            rc, got, g = _decode8(L, _lib, _q(H, hd), Kc, Vc, one, one, pos, H, Hkv, hd, ns, 0)
            _lib.check(rc, "gq_attn_decode_roped_kv8")
            assert bool(torch.isnan(got.float()).all()) and bool((_bits(got) == 0x7E00).all())
            assert torch.equal(g["k_cache"].view(torch.uint8).cpu(), Kc.reshape(-1)) and torch.equal(g["v_cache"].view(torch.uint8).cpu(), Vc.reshape(-1))


@pytest.mark.parametrize("hd", [32, 96])
def test_unsupported_head_dim_is_declined_and_writes_nothing(hd):
    _lib = _L()
    L = _lib.lib()
    H, Hkv = 4, 2
    one = torch.ones(Hkv)
    c = torch.zeros(Hkv, 16, hd, dtype=torch.uint8)
    rc, got, _ = _decode8(L, _lib, torch.zeros(H, hd, dtype=torch.float16), c, c, one, one, 3, H, Hkv, hd, 1, 0)
    assert rc == _lib.GQ_ENOTSUP and bool((_bits(got) == 0x7E7E).all())
    rc, out = _prefill8(L, torch.zeros(H, 2, hd, dtype=torch.float16), c, c, one, one, 2, 1, H, Hkv, hd, 0)
    assert rc == _lib.GQ_ENOTSUP and bool((_bits(out) == 0x7E7E).all())


# ------------------------------------------------------------------------------------------------------------------ the prompt kernel
def _prefill8(L, q, Kc, Vc, ks, vs, S, start, H, Hkv, hd, window):
    g = Guards()
    bq, bk, bv, bks, bvs = g.inp("q", q), g.inp("k_cache", Kc), g.inp("v_cache", Vc), g.inp("k_scale", ks), g.inp("v_scale", vs)
    bo = g.out("out", S * H * hd * 2)
    rc = L.gq_attn_prefill_kv8(bq.ptr(), bk.ptr(), bv.ptr(), bks.ptr(), bvs.ptr(), bo.ptr(), S, start, H, Hkv, hd, Kc.shape[1], ap.default_scale(hd), window, None)
    g.check()
    return rc, bo.view(torch.float16, (S, H * hd)).clone()


def _prefill16(L, _lib, q, K16, V16, S, start, H, Hkv, hd, window):
    g = Guards()
    bq, bk, bv = g.inp("q", q), g.inp("k_cache", K16), g.inp("v_cache", V16)
    bo = g.out("out", S * H * hd * 2)
    _lib.check(L.gq_attn_prefill(bq.ptr(), bk.ptr(), bv.ptr(), bo.ptr(), S, start, H, Hkv, hd, K16.shape[1], ap.default_scale(hd), window, None), "gq_attn_prefill")
    g.check()
    return bo.view(torch.float16, (S, H * hd)).clone()


def _prefill_caches(Hkv, hd, S, start, window):
    """random codes in the rows some query attends; 448 in the rows of [0, T) below every window (a visited tile holds them: masked, and
    0 x 448 = 0 inside the product, as the fp16 tests' 65504); NaN / 448 at and behind T (never read); max_seq = T + 3"""
    T = start + S
    used = pam.attend_mask(S, start, T, window).any(dim=0)
    out = []
    for which in ("k", "v"):
        pool = _codes(Hkv, hd, which, 0x7E)
        c = pool[:, torch.arange(T + 3) % pool.shape[1]]  # (a cache longer than the pool repeats it)
        c[:, :T][:, ~used] = k8.MAX_CODE
        c[:, T:] = k8.stale_rows(3, hd)
        out.append(c.contiguous())
    return out


@pytest.mark.parametrize("scales", ["ones", "pow2"])
@pytest.mark.parametrize("S,start,window", PREFILL_CASES, ids=["S%d-start%d-W%d" % c for c in PREFILL_CASES])
@pytest.mark.parametrize("H,Hkv,hd", k8.HEADS, ids=HEADS_IDS)
def test_prefill_launch_equals_the_fp16_launch_bit_for_bit(H, Hkv, hd, S, start, window, scales):
    _lib = _L()
    L = _lib.lib()
    ks, vs = k8.scale_sets(Hkv)[scales]
    q = (torch.randn(H, S, hd, generator=torch.Generator().manual_seed(S + start)) * 0.05).half()
    Kc, Vc = _prefill_caches(Hkv, hd, S, start, window)
    rc, got = _prefill8(L, q, Kc, Vc, ks, vs, S, start, H, Hkv, hd, window)
    _lib.check(rc, "gq_attn_prefill_kv8")
    want = _prefill16(L, _lib, q, k8.dequant(Kc, ks).half(), k8.dequant(Vc, vs).half(), S, start, H, Hkv, hd, window)
    assert torch.isfinite(want.float()).all()
    assert torch.equal(_bits(got), _bits(want)), "%d element(s) differ, worst %d fp16 steps" % (int((_bits(got) != _bits(want)).sum()), int(ap.ulp_distance(got, want).max()))


@pytest.mark.parametrize("S,start,window", PREFILL_CASES, ids=["S%d-start%d-W%d" % c for c in PREFILL_CASES])
@pytest.mark.parametrize("hd", [64, 128])
def test_prefill_count_probe_every_attended_row_once(hd, S, start, window):
    _lib = _L()
    L = _lib.lib()
    H, Hkv = 4, 2
    one = torch.ones(Hkv)
    for coarse in (False, True):
        q, K, V, expect = pam.count_probe(H, Hkv, hd, S, start, window, start + S + 3, coarse)
        # (the probe's 65504 / NaN / Inf rows -- rows no query attends -- become 448 and NaN codes)
        Vc = torch.where(V == 1.0, k8.ONE_CODE, torch.where(V == 0.0, 0, torch.where(torch.isfinite(V), k8.MAX_CODE, k8.NAN_CODE))).to(torch.uint8)
        Kc = torch.where(K == 0.0, 0, torch.where(torch.isfinite(K), k8.MAX_CODE, k8.NAN_CODE)).to(torch.uint8)
        rc, out = _prefill8(L, q, Kc, Vc, one, one, S, start, H, Hkv, hd, window)
        _lib.check(rc, "gq_attn_prefill_kv8")
        assert torch.isfinite(out.float()).all(), "not finite"
        d = ap.ulp_distance(out.cpu(), expect)
        assert int(d.max()) <= 1, (coarse, int(d.argmax()), int(d.max()))


@pytest.mark.parametrize("S,start,window", PREFILL_CASES, ids=["S%d-start%d-W%d" % c for c in PREFILL_CASES])
@pytest.mark.parametrize("H,Hkv,hd", k8.HEADS, ids=HEADS_IDS)
def test_prefill_launch_with_free_scales_against_float64(H, Hkv, hd, S, start, window):
    _lib = _L()
    L = _lib.lib()
    ks, vs = k8.scale_sets(Hkv)["free"]
    q = (torch.randn(H, S, hd, generator=torch.Generator().manual_seed(S + start)) * 0.05).half()
    Kc, Vc = _prefill_caches(Hkv, hd, S, start, window)
    rc, got = _prefill8(L, q, Kc, Vc, ks, vs, S, start, H, Hkv, hd, window)
    _lib.check(rc, "gq_attn_prefill_kv8")
    T = start + S
    lo = max(0, start + 1 - window) if window else 0  # (rows below every query's window are left out: the mask rule knows differences only)
    used = pam.attend_mask(S, start, T, window).any(dim=0)[None, lo:, None]
    zero = torch.zeros((), dtype=torch.float64)
    Kd = torch.where(used, k8.dequant(Kc[:, lo:T], ks, torch.float64), zero)  # (rows no query attends: masked in the model too; NaN x 0 is not 0)
    Vd = torch.where(used, k8.dequant(Vc[:, lo:T], vs, torch.float64), zero)
    want = pam.reference(q, Kd, Vd, start - lo, ap.default_scale(hd), window)
    o = got.cpu().double()
    assert torch.isfinite(o).all()
    vmax = float(Vd.abs().max())
    err = float((o - want).abs().max())
    bound = pam.error_bound(T, vmax)  # (the bound of tests/test_prefill_attn_gpu.py)
    print("H%d/%d hd%d S%d start%d W%d: max|V scale| %.3f  err %.3e  bound %.3e" % (H, Hkv, hd, S, start, window, vmax, err, bound))
    assert err <= bound, (err, bound)
