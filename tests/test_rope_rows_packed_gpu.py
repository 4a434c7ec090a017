"""GPU: the row write of the packed pass (csrc/prefill.hip, gq_rope_cache_rows_packed: the cache row apart from the RoPE position) through
the C ABI on guard-banded, poisoned buffers, against the entries it restates -- gq_rope_cache_rows (no norm weights) and
gq_qknorm_rope_cache_rows (both norm weights).  head_dim {64, 128}, S {1, 5, 70}; every comparison is of bytes.

  row == pos            q_out and both caches are those of the existing entry.
  row a permutation     (apart from pos, one entry >= max_seq) q_out is still the existing entry's; cache row row[s] holds what the
                        existing entry writes at pos[s] in a cache of its own; every other byte keeps the poison pattern; the entry at
                        or beyond max_seq writes nothing; the guard bands hold."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from guarded import Guards  # noqa: E402

MAX_SEQ = 96
EPS = 1e-6
H, HKV = 4, 2


def _L():
    from guidedquant_amd import _lib
    return _lib


def _tables(hd):
    fr = torch.outer(torch.arange(MAX_SEQ).float(), 1.0 / (10000.0 ** (torch.arange(0, hd, 2).float() / hd)))
    emb = torch.cat((fr, fr), dim=-1)
    return emb.cos().half().contiguous(), emb.sin().half().contiguous()


def _launch(form, packed, qkv, pos, row, cos, sin, qw, kw, S, hd):
    """(q_out, k_cache, v_cache) as int16 bits on the host, caches [HKV, MAX_SEQ, hd]"""
    _lib = _L()
    L = _lib.lib()
    g = Guards()
    b = dict(qkv=g.inp("qkv", qkv), pos=g.inp("pos", pos), row=g.inp("row", row), cos=g.inp("cos", cos), sin=g.inp("sin", sin), qw=g.inp("qw", qw), kw=g.inp("kw", kw))
    q, kc, vc = g.out("q", H * S * hd * 2), g.out("kc", HKV * MAX_SEQ * hd * 2), g.out("vc", HKV * MAX_SEQ * hd * 2)
    shape = (S, H, HKV, hd, MAX_SEQ)
    if packed:
        norm = (b["qw"].ptr(), b["kw"].ptr(), EPS) if form == "qknorm" else (None, None, 0.0)
        rc = L.gq_rope_cache_rows_packed(b["qkv"].ptr(), b["pos"].ptr(), b["row"].ptr(), b["cos"].ptr(), b["sin"].ptr(), q.ptr(), kc.ptr(), vc.ptr(), *shape, *norm, None)
    elif form == "qknorm":
        rc = L.gq_qknorm_rope_cache_rows(b["qkv"].ptr(), b["pos"].ptr(), b["cos"].ptr(), b["sin"].ptr(), q.ptr(), kc.ptr(), vc.ptr(), *shape, b["qw"].ptr(), b["kw"].ptr(), EPS, None)
    else:
        rc = L.gq_rope_cache_rows(b["qkv"].ptr(), b["pos"].ptr(), b["cos"].ptr(), b["sin"].ptr(), q.ptr(), kc.ptr(), vc.ptr(), *shape, None)
    _lib.check(rc, "row write")
    g.check()
    return q.view(torch.int16).cpu(), kc.view(torch.int16, (HKV, MAX_SEQ, hd)).cpu(), vc.view(torch.int16, (HKV, MAX_SEQ, hd)).cpu()


@pytest.mark.parametrize("S", [1, 5, 70])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("form", ["plain", "qknorm"])
def test_rows_against_the_existing_entries(form, hd, S):
    g = torch.Generator().manual_seed(1000 * S + hd + (form == "qknorm"))
    qkv = torch.randn(S, (H + 2 * HKV) * hd, generator=g).half()
    qw = kw = None
    if form == "qknorm":
        qw, kw = (0.5 + torch.rand(hd, generator=g)).half(), (0.5 + torch.rand(hd, generator=g)).half()
    cos, sin = _tables(hd)
    # positions as a pack has them: sequences of 3, 1, .. rows end to end, each counting from 0
    pos = torch.tensor([(s % 4) if s < 8 else s - 8 for s in range(S)], dtype=torch.int32)
    ident = torch.arange(S, dtype=torch.int32)
    POISON = 0x7E7E
    # ---- row == pos (distinct positions: the identity) against the existing entry
    q0, k0, v0 = _launch(form, False, qkv, ident, None, cos, sin, qw, kw, S, hd)
    q1, k1, v1 = _launch(form, True, qkv, ident, ident, cos, sin, qw, kw, S, hd)
    assert torch.equal(q1, q0) and torch.equal(k1, k0) and torch.equal(v1, v0)
    # ---- row a permutation apart from pos; its last entry at or beyond max_seq
    row = ((torch.arange(S) * 37 + 11) % MAX_SEQ).to(torch.int32)  # (37 and 96 are co-prime: distinct rows)
    row[-1] = MAX_SEQ + (S % 3)
    assert len(set(row.tolist())) == S and (S == 1 or not torch.equal(row[:-1], pos[:-1]))
    qp, kp, vp = _launch(form, True, qkv, pos, row, cos, sin, qw, kw, S, hd)
    # what the existing entry makes of row s at position pos[s]: one launch per distinct position set (positions repeat across sequences)
    qe = torch.empty(H, S, hd, dtype=torch.int16)
    want_k, want_v = torch.full((HKV, MAX_SEQ, hd), POISON, dtype=torch.int16), torch.full((HKV, MAX_SEQ, hd), POISON, dtype=torch.int16)
    for s in range(S):
        qs, ks, vs = _launch(form, False, qkv[s:s + 1].contiguous(), pos[s:s + 1].contiguous(), None, cos, sin, qw, kw, 1, hd)
        qe[:, s] = qs.view(H, 1, hd)[:, 0]
        if int(row[s]) < MAX_SEQ:
            want_k[:, int(row[s])], want_v[:, int(row[s])] = ks[:, int(pos[s])], vs[:, int(pos[s])]
    assert torch.equal(qp.view(H, S, hd), qe), "q_out differs from the existing entry's"
    assert torch.equal(kp, want_k) and torch.equal(vp, want_v)  # (the written rows, and the poison pattern everywhere else)
    assert int((kp[0, :, 0] != POISON).sum()) == S - 1


def test_argument_checks_write_nothing():
    _lib = _L()
    L = _lib.lib()
    S = 2
    for hd, qw, kw, row, want in ((64, True, False, True, _lib.GQ_EINVAL), (64, False, False, False, _lib.GQ_EINVAL), (32, True, True, True, _lib.GQ_ENOTSUP),
                                  (40, False, False, True, _lib.GQ_ENOTSUP)):
        g = Guards()
        W = (H + 2 * HKV) * hd
        one = torch.ones(MAX_SEQ, hd, dtype=torch.float16)
        b = dict(qkv=g.inp("qkv", torch.ones(S, W, dtype=torch.float16)), pos=g.inp("pos", torch.tensor([0, 1], dtype=torch.int32)), cos=g.inp("cos", one),
                 w=g.inp("w", torch.ones(hd, dtype=torch.float16)))
        q, kc, vc = g.out("q", H * S * hd * 2), g.out("kc", HKV * MAX_SEQ * hd * 2), g.out("vc", HKV * MAX_SEQ * hd * 2)
        rc = L.gq_rope_cache_rows_packed(b["qkv"].ptr(), b["pos"].ptr(), b["pos"].ptr() if row else None, b["cos"].ptr(), b["cos"].ptr(), q.ptr(), kc.ptr(), vc.ptr(),
                                         S, H, HKV, hd, MAX_SEQ, b["w"].ptr() if qw else None, b["w"].ptr() if kw else None, EPS, None)
        g.check()
        assert rc == want, (hd, rc)
        for o in (q, kc, vc):
            assert bool((o.view(torch.uint8) == 0x7E).all())
