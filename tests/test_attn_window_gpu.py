"""GPU, kernel level: the sliding-window forms of the decode attention launches (csrc/decode.hip, WIN; gq_attn_decode_split_window,
_split_qknorm_window, _split_bias_window, gq_attn_decode_roped_window) through the C ABI.

The query at `pos` of a layer with window W attends the cached rows [lo, pos], lo = max(0, pos + 1 - W), n = pos + 1 - lo, and the launch
is the launch without a window at position n - 1 shifted by lo.  So:

  shift identity   out (and, for the entries that rotate, the cache row they write) equal BIT FOR BIT what the old entry gives at
                   pos' = n - 1 on a second cache that holds rows [lo, pos] as rows [0, n - 1] -- with the rows < lo and > pos of the first
                   cache poisoned (NaN / +-Inf / 65504, attn_probes.POISON_BITS): whatever reads one of them shows.  No tolerance.
  float64          the score profiles of attn_probes on the shifted rows against attn_probes.reference, with the bound
                   tests/test_attn_probes_gpu.py:193 applies to its profile probes (`assert r <= ap.PROFILE_C`, c = 2^-14 on
                   (|out - ref| - 2^-10 |ref|) / A): the window forms do not rest on the project's own kernel without a window alone.
  count            K = 0, V one-hot by class: out[d] = #rows of class d in [lo, pos] / n exactly; the class planted only below lo gives 0.
  window >= max_seq  bit-equal to the old entry on the same cache.
  window == 0      GQ_EINVAL, nothing launched.
"""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import attn_probes as ap  # noqa: E402

ENTRIES = ("split", "qknorm", "bias", "roped")
NAMES = dict(split="gq_attn_decode_split", qknorm="gq_attn_decode_split_qknorm", bias="gq_attn_decode_split_bias", roped="gq_attn_decode_roped")
HEADS = ((8, 2), (4, 4))  # 8 / 2: the four-heads-per-block form of the roped entry is reachable at n_split >= 4
SPLITS = (1, 4, 8, 32)
GQ_EINVAL = -22
_tables, _noise = {}, {}


def _dev():
    return torch.device("cuda:0")


def window_geometry(hd, pos, n_split, W):
    """(lo, n, splits): the row ranges [p0, p1) the blocks of a window launch take -- those of attn_probes.geometry at position n - 1,
    shifted by lo"""
    lo = pos + 1 - W if pos + 1 > W else 0
    n = pos + 1 - lo
    geo = ap.geometry(hd, n - 1, n_split)
    return lo, n, [(lo + a, lo + b) for a, b in geo.splits]


def window_cases(hd):
    """(W, max_seq, [pos ..]) of the shift-identity test: every window length at which the launch takes another path (one row; less than
    a batch of a wave; one row more than the rows requested ahead of the position; the solo rule's last and first-beyond length; splits
    that end inside a pass; 32 passes), each at the positions around pos = W - 1 (where lo leaves 0), a pass later, and at the last row of
    the cache.  max_seq - W is odd: lo is odd at pos = W (lo = 1) and at pos = max_seq - 1."""
    g = ap.geometry(hd, 0, 1)
    P, out = g.PASS, []
    for W in (1, g.PPW * ap.U - 1, ap.SPEC + 1, 2 * P, 2 * P + 1, 3 * P + 5, 32 * P):
        max_seq = W + P + 41
        poss = sorted({p for p in (W - 2, W - 1, W, W + 1, W + P - 1, max_seq - 1) if 0 <= p < max_seq})
        out.append((W, max_seq, poss))
    return out


def _rope_tables(hd):
    if hd not in _tables:
        inv = 1.0 / (500000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32, device=_dev()) / hd))
        fr = torch.outer(torch.arange(ap.NMAX, dtype=torch.float32, device=_dev()), inv)
        emb = torch.cat((fr, fr), dim=-1)
        _tables[hd] = (emb.cos().half().contiguous(), emb.sin().half().contiguous())
    return _tables[hd]


def _pool(name, shape, lo, hi, seed):
    key = (name, tuple(shape))
    if key not in _noise:
        g = torch.Generator()
        g.manual_seed(seed)
        _noise[key] = (lo + (hi - lo) * torch.rand(shape, generator=g)).half().to(_dev())
    return _noise[key]


def _poison_rows(n):
    bits = torch.tensor(ap.POISON_BITS, dtype=torch.int32, device=_dev())[torch.arange(n, device=_dev()) % 4].to(torch.int16)
    return bits.view(torch.float16)[None, :, None]


def _poison_outside(K, V, lo, pos):
    """whole rows of NaN / +Inf / -Inf / 65504 in every row < lo and > pos"""
    for T in (K, V):
        if lo > 0:
            T[:, :lo] = _poison_rows(lo)
        if T.shape[1] > pos + 1:
            T[:, pos + 1:] = _poison_rows(T.shape[1] - pos - 1)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _extra(entry, H, Hkv, hd):
    """what an entry takes behind the workspace: the q / k norm weights and eps, or the bias"""
    if entry == "qknorm":
        return (_pool("qw", (hd,), 0.5, 1.5, 3).data_ptr(), _pool("kw", (hd,), 0.5, 1.5, 4).data_ptr(), 1e-6)
    if entry == "bias":
        return (_pool("bias", ((H + 2 * Hkv) * hd,), -0.5, 0.5, 5).data_ptr(),)
    return ()


def _launch(L, _lib, entry, window, src, pos, kc, vc, H, Hkv, hd, max_seq, ns, row_off=0, extra=None):
    """one launch; window None: the old entry.  row_off: the cos / sin tables start at that row.  Returns out [H, hd] (NaN before)."""
    d = _dev()
    posd = torch.tensor([pos], dtype=torch.int32, device=d)
    out = torch.full((H, hd), float("nan"), dtype=torch.float16, device=d)
    ws = torch.full((H * ns * (hd + 2),), float("nan"), dtype=torch.float32, device=d)
    wsp = ws.data_ptr() if ns > 1 else None
    st = _lib.current_stream_ptr()
    extra = _extra(entry, H, Hkv, hd) if extra is None else extra
    wargs = () if window is None else (window,)
    name = NAMES[entry] + ("" if window is None else "_window")
    if entry == "roped":
        rc = getattr(L, name)(src.data_ptr(), posd.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), H, Hkv, hd, max_seq, ap.default_scale(hd),
                              ns, wsp, *wargs, st)
    else:
        cos, sin = _rope_tables(hd)
        rc = getattr(L, name)(src.data_ptr(), posd.data_ptr(), cos.data_ptr() + row_off * hd * 2, sin.data_ptr() + row_off * hd * 2, kc.data_ptr(),
                              vc.data_ptr(), out.data_ptr(), H, Hkv, hd, max_seq, ap.default_scale(hd), ns, wsp, *extra, *wargs, st)
    _lib.check(rc, name)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("H,Hkv", HEADS, ids=["%dx%d" % h for h in HEADS])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("entry", ENTRIES)
def test_a_window_launch_is_the_old_launch_shifted_by_lo(entry, hd, H, Hkv):
    from guidedquant_amd import _lib
    L = _lib.lib()
    rot = entry != "roped"
    Kn = _pool("k", (4, ap.NMAX, hd), -1.0, 1.0, 1)[:Hkv]
    Vn = _pool("v", (4, ap.NMAX, hd), -2.0, 2.0, 2)[:Hkv]
    src = _pool("qkv", ((8 + 2 * 4) * 128,), -1.0, 1.0, 6)[:(H + 2 * Hkv) * hd].contiguous()  # q | k | v (roped: the rotated q in front)
    ran, odd = 0, 0
    for W, max_seq, poss in window_cases(hd):
        for pos in poss:
            lo, n, _ = window_geometry(hd, pos, 1, W)
            odd += lo % 2
            k1, v1 = Kn[:, :max_seq].clone(), Vn[:, :max_seq].clone()
            _poison_outside(k1, v1, lo, pos)
            if rot:  # (the current row comes from the launch, not from the cache)
                k1[:, pos] = float("nan")
                v1[:, pos] = float("nan")
            k0, v0 = k1.clone(), v1.clone()
            # the twin: rows [lo, pos] as rows [0, n - 1] of a cache of max_seq - lo rows, stale rows behind them
            m2 = max_seq - lo
            k2, v2 = torch.empty(Hkv, m2, hd, dtype=torch.float16, device=_dev()), torch.empty(Hkv, m2, hd, dtype=torch.float16, device=_dev())
            _poison_outside(k2, v2, 0, -1)
            k2[:, :n], v2[:, :n] = k1[:, lo:pos + 1], v1[:, lo:pos + 1]
            for ns in SPLITS:
                ka, va, kb, vb = k1.clone(), v1.clone(), k2.clone(), v2.clone()
                got = _launch(L, _lib, entry, W, src, pos, ka, va, H, Hkv, hd, max_seq, ns)
                want = _launch(L, _lib, entry, None, src, n - 1, kb, vb, H, Hkv, hd, m2, ns, row_off=lo)
                what = (entry, hd, H, Hkv, "W", W, "pos", pos, "lo", lo, "n_split", ns)
                assert torch.isfinite(want.float()).all(), what  # (the twin itself read no stale row)
                assert torch.equal(_bits(got), _bits(want)), what + ("out", int((_bits(got) != _bits(want)).sum()))
                if rot:  # the row the launch wrote, and nothing else
                    assert torch.equal(_bits(ka[:, pos]), _bits(kb[:, n - 1])) and torch.equal(_bits(va[:, pos]), _bits(vb[:, n - 1])), what
                    assert torch.isfinite(ka[:, pos].float()).all() and torch.isfinite(va[:, pos].float()).all(), what
                    ka[:, pos], va[:, pos] = k0[:, pos], v0[:, pos]
                assert torch.equal(_bits(ka[:, :lo]), _bits(k0[:, :lo])) and torch.equal(_bits(va[:, :lo]), _bits(v0[:, :lo])), what + ("rows < lo",)
                assert torch.equal(_bits(ka), _bits(k0)) and torch.equal(_bits(va), _bits(v0)), what + ("cache",)
                ran += 1
    assert odd >= 2 and ran >= 4 * 7 * 4


PROFILE_FORMS = ("split", "bias", "roped")


def _rots(entry, hd, pos):
    """what the launch does to the q and the k it is handed: the rotation at the TRUE position (the bias of these tests is zero; the QK-norm
    entry runs the count probe only, whose k is zero and whose q does not matter)"""
    if entry == "roped":
        return ap._ident, ap._ident
    cos, sin = _rope_tables(hd)
    c, s = cos[pos], sin[pos]

    def rope(x):
        return (x * c) + (torch.cat((-x[..., hd // 2:], x[..., :hd // 2]), dim=-1) * s)
    return rope, rope


def _embed(p, lo, class0=False):
    """the probe's caches behind `lo` rows that are out of the window: poison, or (class0) zero K and the V class of element 0"""
    Hkv, m, hd = p.K.shape
    K, V = torch.empty(Hkv, lo + m, hd, dtype=torch.float16, device=_dev()), torch.empty(Hkv, lo + m, hd, dtype=torch.float16, device=_dev())
    _poison_outside(K, V, lo, -1)
    if class0:
        K[:, :lo], V[:, :lo] = 0, 0
        V[:, :lo, 0] = 1
    K[:, lo:], V[:, lo:] = p.K, p.V
    return K, V


def _src(entry, p):
    return p.q.contiguous() if entry == "roped" else torch.cat((p.q_in.reshape(-1), p.k_in.reshape(-1), p.v_in.reshape(-1))).contiguous()


def _window_launch_on(L, _lib, entry, p, lo, H, Hkv, hd, ns, K, V):
    """the probe at position p.pos of its own rows, as a window launch at lo + p.pos with W = p.pos + 1 on the embedding caches"""
    pos, W = lo + p.pos, p.pos + 1
    if entry != "roped":
        K[:, pos], V[:, pos] = float("nan"), float("nan")
    zero = _pool("zero_bias", ((H + 2 * Hkv) * hd,), 0.0, 0.0, 0)  # (kept alive in the pool: the launch gets its address)
    assert float(zero.abs().max()) == 0.0
    extra = (zero.data_ptr(),) if entry == "bias" else None
    keep = (K.clone(), V.clone())
    out = _launch(L, _lib, entry, W, _src(entry, p), pos, K, V, H, Hkv, hd, K.shape[1], ns, extra=extra)
    if entry != "roped":  # (row pos: the rotated k / the v of the probe's current token)
        # (by value: a zero element may come out of the launch's fp16 operations with the other sign than out of torch's)
        assert torch.equal(K[:, pos], p.K[:, p.pos]) and torch.equal(V[:, pos], p.V[:, p.pos]), (entry, p.kind, "row pos")
        K[:, pos], V[:, pos] = keep[0][:, pos], keep[1][:, pos]
    assert torch.equal(_bits(K), _bits(keep[0])) and torch.equal(_bits(V), _bits(keep[1])), (entry, p.kind, "cache")
    return out


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("entry", PROFILE_FORMS)
def test_window_launch_against_float64_on_the_score_profiles(entry, hd):
    from guidedquant_amd import _lib
    L = _lib.lib()
    H, Hkv, scale, lo = 8, 2, ap.default_scale(hd), 37
    P = ap.geometry(hd, 0, 1).PASS
    worst, ran = 0.0, 0
    for pp, ns in ((33, 4), (8 * P - 1, 8), (8 * P, 8), (8 * P + 1, 8)):
        names = ap.profile_names(hd, pp, ns)
        assert names
        rot_q, rot_k = _rots(entry, hd, lo + pp)
        for name in names:
            p = ap.profile_probe(name, H, Hkv, hd, pp, ns, pp + 40, scale, rot_q=rot_q, rot_k=rot_k, device=_dev())
            K, V = _embed(p, lo)
            out = _window_launch_on(L, _lib, entry, p, lo, H, Hkv, hd, ns, K, V)
            r = ap.profile_ratio(out, p, scale)  # (the reference: float64 over rows 0..pp of the probe = rows [lo, pos] of the launch)
            print("%s hd %d lo %d n %d n_split %d %s: (err - 2^-10 |ref|) / A = %.3e" % (entry, hd, lo, pp + 1, ns, name, r))
            worst = max(worst, r)
            assert r <= ap.PROFILE_C, (entry, name, pp, ns, r)  # tests/test_attn_probes_gpu.py:193
            ran += 1
    print("%s hd %d: worst profile ratio %.3e (c = %.3e)" % (entry, hd, worst, ap.PROFILE_C))
    assert ran == 4 + 3 * len(ap.PROFILES)


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("entry", ENTRIES)
def test_count_probe_inside_a_window(entry, hd):
    """every row of [lo, pos] exactly once and none below: the rows below lo are real rows (K = 0 like every other: weight 1 if they were
    read) of class 0, which no row of the window has"""
    from guidedquant_amd import _lib
    L = _lib.lib()
    H, Hkv = 8, 2
    P = ap.geometry(hd, 0, 1).PASS
    for n, lo, ns in ((16, 35, 1), (20, 31, 4), (2 * P, 77, 4), (1024, P + 3, 4), (1024, P + 3, 32), (3 * P + 5, 2 * P + 1, 8)):
        pp = n - 1
        rot_q, rot_k = _rots(entry, hd, lo + pp)
        p = ap.count_probe(H, Hkv, hd, pp, pp + 40, rot_q=rot_q, rot_k=rot_k, device=_dev())
        t = torch.arange(n, device=_dev())
        V = torch.zeros(Hkv, n, hd, dtype=torch.float16, device=_dev())
        V[:, t, 1 + t % (hd - 1)] = 1  # classes 1 .. hd - 1 inside the window
        p.V[:, :n] = V
        p.v_in.copy_(V[:, pp])
        Kc, Vc = _embed(p, lo, class0=True)
        out = _window_launch_on(L, _lib, entry, p, lo, H, Hkv, hd, ns, Kc, Vc)  # (the bias is zero; q / k norm weights as in _extra)
        want = (V.float().sum(1) / torch.tensor(float(n), device=_dev())).half().repeat_interleave(H // Hkv, dim=0)  # fp32 quotient, one fp16 rounding
        assert torch.equal(_bits(out), _bits(want)), (entry, hd, n, lo, ns, out[0, :4], want[0, :4])
        assert float(out[:, 0].abs().max()) == 0.0, (entry, hd, n, lo, ns, "a row below lo was counted")


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("entry", ENTRIES)
def test_a_window_the_cache_never_outgrows_is_the_old_entry(entry, hd):
    from guidedquant_amd import _lib
    L = _lib.lib()
    H, Hkv = 8, 2
    P = ap.geometry(hd, 0, 1).PASS
    src = _pool("qkv", ((8 + 2 * 4) * 128,), -1.0, 1.0, 6)[:(H + 2 * Hkv) * hd].contiguous()
    for pos, ns in ((5, 1), (5, 4), (2 * P + 1, 4), (5 * P + 3, 8), (5 * P + 3, 1)):
        max_seq = pos + 40
        k1, v1 = _pool("k", (4, ap.NMAX, hd), -1.0, 1.0, 1)[:Hkv, :max_seq].clone(), _pool("v", (4, ap.NMAX, hd), -2.0, 2.0, 2)[:Hkv, :max_seq].clone()
        _poison_outside(k1, v1, 0, pos)
        for W in (max_seq, max_seq + 1, 2**32 - 1):
            ka, va, kb, vb = k1.clone(), v1.clone(), k1.clone(), v1.clone()
            got = _launch(L, _lib, entry, W, src, pos, ka, va, H, Hkv, hd, max_seq, ns)
            want = _launch(L, _lib, entry, None, src, pos, kb, vb, H, Hkv, hd, max_seq, ns)
            assert torch.isfinite(want.float()).all()
            assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(ka), _bits(kb)) and torch.equal(_bits(va), _bits(vb)), (entry, hd, pos, ns, W)


@pytest.mark.parametrize("entry", ENTRIES)
def test_window_zero_is_declined_without_a_launch(entry):
    from guidedquant_amd import _lib
    L = _lib.lib()
    H, Hkv, hd, max_seq, pos = 8, 2, 64, 64, 9
    d = _dev()
    src = _pool("qkv", ((8 + 2 * 4) * 128,), -1.0, 1.0, 6)[:(H + 2 * Hkv) * hd].contiguous()
    kc, vc = torch.ones(Hkv, max_seq, hd, dtype=torch.float16, device=d), torch.ones(Hkv, max_seq, hd, dtype=torch.float16, device=d)
    posd = torch.tensor([pos], dtype=torch.int32, device=d)
    out = torch.full((H, hd), float("nan"), dtype=torch.float16, device=d)
    st = _lib.current_stream_ptr()
    name = NAMES[entry] + "_window"
    if entry == "roped":
        rc = getattr(L, name)(src.data_ptr(), posd.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), H, Hkv, hd, max_seq, 0.125, 1, None, 0, st)
    else:
        cos, sin = _rope_tables(hd)
        rc = getattr(L, name)(src.data_ptr(), posd.data_ptr(), cos.data_ptr(), sin.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), H, Hkv,
                              hd, max_seq, 0.125, 1, None, *_extra(entry, H, Hkv, hd), 0, st)
    torch.cuda.synchronize()
    assert rc == GQ_EINVAL == _lib.GQ_EINVAL, rc
    assert b"window" in L.gq_last_error()
    assert torch.isnan(out).all() and bool((kc == 1).all()) and bool((vc == 1).all())
