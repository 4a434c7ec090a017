"""GPU: the decode attention launches on the probes of tests/attn_probes.py -- every cached row exactly once, with its own V row, at
every pass / split / speculation boundary, through the combine's second loop (33 and 64 splits), with NaN / Inf rows behind the
position, and the online softmax through its rescale paths against float64.

Forms: gq_attn_decode_split, gq_attn_decode_split_qknorm, gq_attn_decode_roped (one head per block, and the default with the four heads
of a KV group in one block -- both settings bit-identical), gq_attn_decode_qtip.  n_split, max_seq (= pos + 40) and the workspace
(NaN-filled: every partial result that is combined was written by this launch) are always explicit.

Assertions: count / needle / twin within 1 fp16 step of the exact expectation; score profiles |out - ref| <= 2^-10 |ref| + c A with
c = 2^-14 (ref, A from float64; 2^-10 is the final fp16 rounding doubled, the base-2 argument of the fast exponential carries about
2^-24 |x| log2(e) with |x| <= 120: a weight error under 2^-17, at most 512 sequential fp32 additions per stream add 2^-15 at worst);
the caches bit for bit what they were, row pos of the split forms = the rotated k / the v of the current token.

Measured worst (err - 2^-10 |ref|) / A per form on an MI355X, over all profiles and contexts (the bound stays at c = 2^-14 = 6.10e-5):
  gq_attn_decode_split                      4.61e-6  (hd 128, pos 33, +-300: the scores of a rotated q are not exact in fp32)
  gq_attn_decode_roped, one head per block  3.48e-6  (hd 128, pos 33, +-300: the fp32 rounding of score * 2^-3.5; hd 64: 4.0e-9)
  gq_attn_decode_roped, default             3.48e-6  (bit-identical to one head per block on every probe)
The float32 host emulator gives 3.48e-6 on the same inputs (test_attn_probes_cpu.py).  The QK-norm and QTIP forms run the exact probes
only.  No probe failed: csrc/decode.hip is as it was.
"""
import math
import os

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import attn_probes as ap  # noqa: E402

# worst (err - 2^-10 |ref|) / A over the score profiles, per form (MI355X); the bound is c = ap.PROFILE_C = 2^-14
MEASURED = {"split": 4.61e-6, "roped_gqa0": 3.48e-6, "roped": 3.48e-6}

CASES = [(f, H, Hkv, hd) for f, geos in (("split", ((2, 2), (4, 2))), ("qknorm", ((4, 2),)), ("roped_gqa0", ((4, 1), (4, 2))),
                                         ("roped", ((4, 1), (8, 1), (8, 2)))) for H, Hkv in geos for hd in (64, 128)] + [("qtip", 8, 2, 128)]
GROUPS = ("short", "solo", "jump", "wide")
_tables, _sylv = {}, {}


def _dev():
    return torch.device("cuda:0")


def _rope_tables(hd):
    if hd not in _tables:
        inv = 1.0 / (500000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32, device=_dev()) / hd))
        fr = torch.outer(torch.arange(ap.NMAX, dtype=torch.float32, device=_dev()), inv)
        emb = torch.cat((fr, fr), dim=-1)
        _tables[hd] = (emb.cos().half().contiguous(), emb.sin().half().contiguous())
    return _tables[hd]


def _rotate_half(x):
    return torch.cat((-x[..., x.shape[-1] // 2:], x[..., :x.shape[-1] // 2]), dim=-1)


def _rots(form, hd, pos):
    """what the launch does to the q and the k it is handed (torch restatement, the rounding points of apply_rotary_pos_emb and of
    Qwen3RMSNorm as in test_qknorm_attn_gpu.py); the norm weights are 1 for q and 8 for k: a planted current row is 8 q"""
    if form.startswith("roped"):
        return ap._ident, ap._ident, None
    cos, sin = _rope_tables(hd)
    c, s = cos[pos], sin[pos]

    def rope(x):
        return (x * c) + (_rotate_half(x) * s)
    if form != "qknorm":
        return rope, rope, None
    qw = torch.ones(hd, dtype=torch.float16, device=_dev())
    kw = 8 * qw
    eps = 1e-6

    def norm(x, w):
        xf = x.float()
        return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)).to(x.dtype) * w
    return (lambda x: rope(norm(x, qw))), (lambda x: rope(norm(x, kw))), (qw, kw, eps)


def _sylvester(M):
    if M not in _sylv:
        i = torch.arange(M, device=_dev())
        b = i[:, None] & i[None, :]
        par = torch.zeros_like(b)
        for k in range(14):
            par ^= (b >> k) & 1
        _sylv[M] = (1 - 2 * par).double()
    return _sylv[M]


def _qtip_sums(x):
    """fp32 sums y with  fp16((H_M y) M^-1/2 * 1) = x  (H H = M I; exact for the probes' values: M^-1/2 is a power of two)"""
    M = x.numel()
    return (_sylvester(M) @ x.double().reshape(-1) / math.sqrt(M)).float().contiguous()


def _launch(L, _lib, form, p, H, Hkv, hd, ns, scale, norm):
    """one launch on fresh copies of the probe's caches; returns out [H, hd]; asserts the cache integrity"""
    d, pos, max_seq = _dev(), p.pos, p.max_seq
    kc, vc = p.K.clone(), p.V.clone()
    posd = torch.tensor([pos], dtype=torch.int32, device=d)
    out = torch.full((H, hd), float("nan"), dtype=torch.float16, device=d)
    ws = torch.full((H * ns * (hd + 2),), float("nan"), dtype=torch.float32, device=d)
    wsp = ws.data_ptr() if ns > 1 else None
    st = _lib.current_stream_ptr()
    if form.startswith("roped"):
        q = p.q.contiguous()
        _lib.check(L.gq_attn_decode_roped(q.data_ptr(), posd.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), H, Hkv, hd, max_seq, scale, ns,
                                          wsp, st), form)
    else:
        kc[:, pos] = float("nan")  # (the current row comes from the launch, not from the cache)
        vc[:, pos] = float("nan")
        cos, sin = _rope_tables(hd)
        qkv = torch.cat((p.q_in.reshape(-1), p.k_in.reshape(-1), p.v_in.reshape(-1))).contiguous()
        args = (posd.data_ptr(), cos.data_ptr(), sin.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), H, Hkv, hd, max_seq, scale, ns, wsp)
        if form == "split":
            _lib.check(L.gq_attn_decode_split(qkv.data_ptr(), *args, st), form)
        elif form == "qknorm":
            _lib.check(L.gq_attn_decode_split_qknorm(qkv.data_ptr(), *args, norm[0].data_ptr(), norm[1].data_ptr(), norm[2], st), form)
        else:
            ys = [_qtip_sums(x) for x in (p.q_in, p.k_in, p.v_in)]
            ones = [torch.ones(y.numel(), dtype=torch.float32, device=d) for y in ys]
            arr = (_lib.GqQtipOut * 3)(*[_lib.GqQtipOut(y.data_ptr(), o.data_ptr(), None, None, y.numel(), 1) for y, o in zip(ys, ones)])
            _lib.check(L.gq_attn_decode_qtip(arr, *args, st), form)
    torch.cuda.synchronize()
    # the poisoned rows behind pos, the rows before it, and row pos itself (split forms: the rotated k and the v of the current token)
    assert torch.equal(kc.view(torch.int16), p.K.view(torch.int16)), (form, p.kind, pos, ns, "k cache")
    assert torch.equal(vc.view(torch.int16), p.V.view(torch.int16)), (form, p.kind, pos, ns, "v cache")
    return out


def _run(L, _lib, form, p, H, Hkv, hd, ns, scale, norm):
    if form != "roped":
        return _launch(L, _lib, form, p, H, Hkv, hd, ns, scale, norm)
    out = _launch(L, _lib, form, p, H, Hkv, hd, ns, scale, norm)
    if ns >= 4 and (H // Hkv) % 4 == 0:  # both settings exist: one head per block gives the same bits
        os.environ["GQ_ATTN_GQA"] = "0"
        L.gq_reset_env_cache()
        try:
            one = _launch(L, _lib, form, p, H, Hkv, hd, ns, scale, norm)
        finally:
            os.environ.pop("GQ_ATTN_GQA", None)
            L.gq_reset_env_cache()
        assert torch.equal(one.view(torch.int16), out.view(torch.int16)), (p.kind, p.pos, ns, "GQ_ATTN_GQA=0 differs")
    return out


def _quantise_current_v(p):
    """qtip: the v of the current token comes out of a transform of fp32 sums -- kept on a 2^-11 grid, where those sums are exact"""
    v = (p.V[:, p.pos].float() * 2048).round() / 2048
    p.V[:, p.pos] = v.half()
    p.v_in.copy_(p.V[:, p.pos])


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("form,H,Hkv,hd", CASES, ids=["%s-%dx%d-hd%d" % c for c in CASES])
def test_attention_launch_on_the_probes(form, H, Hkv, hd, group):
    from guidedquant_amd import _lib
    L = _lib.lib()
    os.environ.pop("GQ_ATTN_GQA", None)
    if form == "roped_gqa0":
        os.environ["GQ_ATTN_GQA"] = "0"
    L.gq_reset_env_cache()
    d, scale = _dev(), ap.default_scale(hd)
    exact_only = form in ("qknorm", "qtip")
    ctxs = ap.contexts(hd)[group]
    if form == "qtip":  # one context per group
        ctxs = ctxs[-2:-1]
    worst = 0.0
    try:
        for pos, ns in ctxs:
            geo = ap.geometry(hd, pos, ns)
            max_seq = pos + 40
            rot_q, rot_k, norm = _rots(form, hd, pos)
            kw = dict(rot_q=rot_q, rot_k=rot_k, device=d)
            probes = [ap.count_probe(H, Hkv, hd, pos, max_seq, **kw)]
            kw2 = dict(kw, zero_cur=exact_only)
            probes += [ap.twin_probe(r, H, Hkv, hd, pos, max_seq, scale, **kw2) for r in ap.plan_rows(ap.twin_pairs(geo), 2, H, Hkv, pos)] if pos else []
            needles = ap.plan_rows(geo.boundary, 1, H, Hkv, pos)
            assert {r for rows in needles for r in rows if r is not None} == set(geo.boundary)
            probes += [ap.needle_probe(r, H, Hkv, hd, pos, max_seq, scale, **kw2) for r in needles]
            for p in probes:
                if form == "qtip":
                    _quantise_current_v(p)
                ap.check_exact(_run(L, _lib, form, p, H, Hkv, hd, ns, scale, norm), p)
            if exact_only:
                continue
            for name in ap.profile_names(hd, pos, ns):
                p = ap.profile_probe(name, H, Hkv, hd, pos, ns, max_seq, scale, **kw)
                out = _run(L, _lib, form, p, H, Hkv, hd, ns, scale, norm)
                r = ap.profile_ratio(out, p, scale)
                print("%s %dx%d hd %d pos %d n_split %d %s: (err - 2^-10 |ref|) / A = %.3e" % (form, H, Hkv, hd, pos, ns, name, r))
                worst = max(worst, r)
                assert r <= ap.PROFILE_C, (name, pos, ns, r)
        print("%s %dx%d hd %d %s: worst profile ratio %.3e (c = %.3e)" % (form, H, Hkv, hd, group, worst, ap.PROFILE_C))
    finally:
        os.environ.pop("GQ_ATTN_GQA", None)
        L.gq_reset_env_cache()
