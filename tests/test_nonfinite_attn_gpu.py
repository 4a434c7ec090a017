"""GPU: NaN and Inf through the decode attention (gq_attn_decode_roped: attn_roped_kernel with the four heads of a KV group in one block and
with one head per block, GQ_ATTN_GQA on and off, and attn_combine_kernel behind 3 splits) on an fp16 cache, against the float64 reference of
tests/attn_probes.py evaluated with IEEE semantics (torch: softmax of a row with a +Inf or NaN score is NaN, exp(-Inf) = 0, 0 * Inf = NaN).

H = 8 heads over Hkv = 2 groups, head_dim 128 (PASS = 128 rows); contexts (pos, n_split) = (33, 1) and (513, 4): the splits are
[0, 256), [256, 512), [512, 514), so rows 127 / 255 / 511 end a pass / a split and the last split holds two rows.  out and the split
workspace start at 1.0.  Rows behind pos hold NaN / Inf / 65504 as in the other attention tests: they must not matter.

Poisoned in turn (every poison of nonfinite_model.POISONS):
  one element of one q head           that head is NaN in the reference (NaN score, or scores of both infinities); the 7 others R2
  one element of an attended K row    at row 0, the last row of a pass, of a split, and the current position: per head of the group the
                                      score is NaN or +Inf (head NaN) or -Inf (weight 0: the head stays finite, within 2^-10 |ref| +
                                      2^-14 A of the reference -- attn_probes.check_profile's bound); the other group's heads R2
  one element of an attended V row    column c of the group's four heads is the poison's class (NaN accepted for Inf); every other
                                      column of those heads and every other head R2
  a -Inf score over an Inf V          K and V of one row: 0 * Inf = NaN in that column of the heads whose score is -Inf
R2 is bit identity with the clean launch of the same context and setting.

FOUND here: softmax_update (csrc/attn_core.h) gave a row the weight 0 unless `score > -2e38`; a NaN score compares false, so a NaN in an
attended K row left the head finite (all 15 K-NaN cases of every context and setting).  The test is `!(score <= -2e38)` now.
Measured on an MI355X after the fix: no violation; NaN for Inf in 0 of 24 (pos 33) and 0 of 40 (pos 513) outputs whose reference is
+-Inf, with GQ_ATTN_GQA on and off alike -- an Inf in V comes out as that Inf.
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import attn_probes as ap  # noqa: E402
import halfsweep_model as hs  # noqa: E402
import nonfinite_model as nf  # noqa: E402

H, HKV, HD = 8, 2, 128
G = H // HKV
CONTEXTS = ((33, 1), (513, 4))


def _t16(bits):
    return torch.tensor([bits], dtype=torch.int16).view(torch.float16)[0] if bits < 0x8000 else torch.tensor([bits - 0x10000], dtype=torch.int16).view(torch.float16)[0]


def _inputs(pos, seed):
    g = torch.Generator().manual_seed(seed)
    max_seq = pos + 40
    q = torch.randn(H, HD, generator=g).half()
    K = (torch.randn(HKV, max_seq, HD, generator=g) * 0.5).half()
    V = torch.randn(HKV, max_seq, HD, generator=g).half()
    for i, b in enumerate(ap.POISON_BITS):   # stale rows behind the position
        K[:, pos + 1 + i::4] = _t16(b)
        V[:, pos + 1 + (i + 1) % 4::4] = _t16(b)
    return q, K, V, max_seq


def _launch(q, K, V, pos, max_seq, ns, scale, form="roped", k_scale=None):
    """one launch on tests/guarded.py buffers; out and the split workspace are payloads of 1.0 (finite), the guards as guarded.py makes them.
    form "roped": gq_attn_decode_roped on the cache as given; "split": gq_attn_decode_split, which takes the current token's q, k, v in
    one vector, rotates q and k (the tables here are cos = 1, sin = 0: the identity) and writes row pos of both caches itself -- the
    cache it is handed holds NaN there; "kv8": gq_attn_decode_roped_kv8 on uint8 caches of e4m3 codes with the scales k_scale (K and V)."""
    import guarded
    from guidedquant_amd import _lib
    L = _lib.lib()
    g = guarded.Guards()
    Kin, Vin = K, V
    if form == "split":
        Kin, Vin = K.clone(), V.clone()
        Kin[:, pos], Vin[:, pos] = float("nan"), float("nan")
    kc, vc = g.inp("k_cache", Kin.contiguous()), g.inp("v_cache", Vin.contiguous())
    posd = g.inp("pos", np.array([pos], dtype=np.int32))
    out = g.inp("out", np.full(H * HD, nf.SENTINEL, dtype=np.uint16))
    ws = g.inp("workspace", np.ones(H * ns * (HD + 2), dtype=np.float32))
    wsp, st = (ws.ptr() if ns > 1 else None), _lib.current_stream_ptr()
    if form == "roped":
        qd = g.inp("q", q.contiguous())
        rc = L.gq_attn_decode_roped(qd.ptr(), posd.ptr(), kc.ptr(), vc.ptr(), out.ptr(), H, HKV, HD, max_seq, scale, ns, wsp, st)
    elif form == "kv8":
        qd, ks = g.inp("q", q.contiguous()), g.inp("scales", k_scale.contiguous())
        rc = L.gq_attn_decode_roped_kv8(qd.ptr(), posd.ptr(), kc.ptr(), vc.ptr(), ks.ptr(), ks.ptr(), out.ptr(), H, HKV, HD, max_seq, scale, ns, wsp, 0, st)
    else:
        qkv = g.inp("qkv", torch.cat((q.reshape(-1), K[:, pos].reshape(-1), V[:, pos].reshape(-1))).contiguous())
        cos = g.inp("cos", torch.ones(max_seq, HD, dtype=torch.float16))
        sin = g.inp("sin", torch.zeros(max_seq, HD, dtype=torch.float16))
        rc = L.gq_attn_decode_split(qkv.ptr(), posd.ptr(), cos.ptr(), sin.ptr(), kc.ptr(), vc.ptr(), out.ptr(), H, HKV, HD, max_seq, scale, ns, wsp, st)
    _lib.check(rc, form)
    g.check()
    if form != "kv8":   # the caches afterwards: untouched, but for row pos, where the split form writes the rotated k and v -- by class
        for buf, want in ((kc, _as_attended(form, q, K, pos)[1]), (vc, V)):
            have = buf.view(torch.float16, tuple(want.shape)).cpu().numpy()
            assert hs.same(have, want.numpy()).all(), (form, "a cache row is not what the launch must leave")
    return out.numpy(np.float16, (H, HD))


def _identity_rope(x):
    """x * cos + rotate_half(x) * sin with cos = 1, sin = 0, in fp16 as apply_rotary_pos_emb rounds: the identity on finite values -- and
    IEEE on the others: an Inf at element e leaves 0 * Inf = NaN at its partner e +- head_dim / 2, a NaN poisons both"""
    half = x.shape[-1] // 2
    rot = torch.cat((-x[..., half:], x[..., :half]), dim=-1)
    return (x * torch.ones((), dtype=torch.float16)) + (rot * torch.zeros((), dtype=torch.float16))


def _as_attended(form, q, K, pos):
    """what the softmax sees: the split form rotates q and the current token's k itself"""
    if form != "split":
        return q, K
    K2 = K.clone()
    K2[:, pos] = _identity_rope(K[:, pos])
    return _identity_rope(q), K2


def _check(tag, got, base, q, K, V, pos, scale, clean, bad, tally, form="roped"):
    """R1 / R3 on every element, R2 on `clean`, and the finite bound on what stays finite outside `clean`"""
    q, K = _as_attended(form, q, K, pos)
    with np.errstate(all="ignore"):
        ref, _, A = ap.reference(q, K, V, pos, scale)
    ref, A = ref.numpy(), A.numpy()
    rc = nf.classify32(ref)
    assert (rc[clean] == nf.FINITE).all(), tag
    b, sub = nf.check(got, rc, False, clean, base)
    bad += [f"{tag}: {v}" for v in b]
    tally[0] += sub
    tally[1] += int(((rc == nf.PINF) | (rc == nf.NINF)).sum())
    fin = (rc == nf.FINITE) & ~clean & np.isfinite(A)
    g64 = got.astype(np.float64)
    with np.errstate(invalid="ignore"):
        over = fin & ~(np.abs(g64 - ref) <= 2.0**-10 * np.abs(ref) + ap.PROFILE_C * A + 2.0**-24)
    if over.any():
        i = tuple(int(v) for v in np.argwhere(over)[0])
        bad.append(f"{tag}: {int(over.sum())} finite element(s) off the reference, first {i}: got {g64[i]!r}, reference {ref[i]!r}")
    return rc


@pytest.fixture(autouse=True)
def _restore_env():
    from guidedquant_amd import _lib
    saved = os.environ.get("GQ_ATTN_GQA")
    yield
    os.environ.pop("GQ_ATTN_GQA", None)
    if saved is not None:
        os.environ["GQ_ATTN_GQA"] = saved
    _lib.lib().gq_reset_env_cache()


FORMS = (("roped", 1), ("roped", 0), ("split", 1))


@pytest.mark.parametrize("form,gqa", FORMS, ids=("roped-gqa", "roped-one_head_per_block", "split"))
@pytest.mark.parametrize("pos,ns", CONTEXTS)
def test_decode_fp16(pos, ns, form, gqa):
    from guidedquant_amd import _lib
    os.environ["GQ_ATTN_GQA"] = str(gqa)
    _lib.lib().gq_reset_env_cache()
    scale = ap.default_scale(HD)
    q, K, V, max_seq = _inputs(pos, 100 + pos)
    run = lambda q_, K_, V_: _launch(q_, K_, V_, pos, max_seq, ns, scale, form)  # noqa: E731
    base = run(q, K, V)
    assert np.isfinite(base.astype(np.float32)).all()
    bad, tally = [], [0, 0]
    head_of = np.arange(H)[:, None] * np.ones((1, HD), dtype=np.int64)
    col_of = np.ones((H, 1), dtype=np.int64) * np.arange(HD)[None, :]
    rows = sorted({0, min(127, pos - 1), min(255, pos - 1), min(511, pos - 1), pos})
    finite_heads = 0
    for pname in nf.POISONS:
        pv = _t16(nf.POISONS[pname])
        for h0, e in ((0, 0), (5, HD - 1)):
            qp = q.clone()
            qp[h0, e] = pv
            rc = _check(f"q[{h0}, {e}] {pname}", run(qp, K, V), base, qp, K, V, pos, scale, head_of != h0, bad, tally, form)
            assert (rc[h0] == nf.NAN).all()
        for t in rows:
            g0, e, c = t % HKV, 5, 77
            mine = (head_of // G) == g0
            Kp = K.clone()
            Kp[g0, t, e] = pv
            rc = _check(f"K[{g0}, {t}, {e}] {pname}", run(q, Kp, V), base, q, Kp, V, pos, scale, ~mine, bad, tally, form)
            finite_heads += int((rc[mine.any(axis=1)] == nf.FINITE).all(axis=1).sum())
            Vp = V.clone()
            Vp[g0, t, c] = pv
            rc = _check(f"V[{g0}, {t}, {c}] {pname}", run(q, K, Vp), base, q, K, Vp, pos, scale, ~(mine & (col_of == c)), bad, tally, form)
            assert (rc[mine & (col_of == c)] != nf.FINITE).all()
            if "inf" in pname:   # a -Inf (or +Inf) score over an Inf V
                Vp = V.clone()
                Vp[g0, t, c] = _t16(0x7C00)
                rc = _check(f"K and V [{g0}, {t}] {pname}", run(q, Kp, Vp), base, q, Kp, Vp, pos, scale, ~mine, bad, tally, form)
                assert (rc[mine & (col_of == c)] == nf.NAN).all()
    assert finite_heads > 0, "no head met a -Inf score"
    print(f"decode {form} pos {pos} n_split {ns} GQ_ATTN_GQA={gqa}: NaN for Inf in {tally[0]} of {tally[1]} outputs whose reference is +-Inf")
    assert not bad, "%d violation(s):\n%s" % (len(bad), "\n".join(bad[:12]))


# ------------------------------------------------------------------------------------------------ the fp8 cache
@pytest.mark.parametrize("gqa", (1, 0), ids=("gqa", "one_head_per_block"))
@pytest.mark.parametrize("pos,ns", CONTEXTS)
def test_decode_fp8_nan_code_reads_back_as_nan(pos, ns, gqa):
    """gq_attn_decode_roped_kv8 with GQ_ATTN_GQA on and off (the fp8 cache has no split-form entry: the current token's row is written by
    gq_rope_cache_rows_kv8 and attended from the cache).  e4m3 has no infinity, its NaN codes are 0x7F and 0xFF.  One code of an attended K row: the group's heads are
    NaN; of an attended V row: that column of the group's heads is NaN; everything else is bit-identical to the clean launch.  Rows behind
    pos hold NaN codes and 448 (kv8_model.stale_rows): they must not matter."""
    import kv8_model as k8
    from guidedquant_amd import _lib
    os.environ["GQ_ATTN_GQA"] = str(gqa)
    _lib.lib().gq_reset_env_cache()
    g = torch.Generator().manual_seed(7 + pos)
    max_seq = pos + 40
    q = torch.randn(H, HD, generator=g).half()
    Kc = k8.random_codes((HKV, max_seq, HD), g, max_exp_code=0x3F)   # |value| < 2: moderate scores
    Vc = k8.random_codes((HKV, max_seq, HD), g, max_exp_code=0x47)
    Kc[:, pos + 1:] = k8.stale_rows(max_seq - pos - 1, HD)
    Vc[:, pos + 1:] = k8.stale_rows(max_seq - pos - 1, HD)
    scales = torch.tensor([0.5, 2.0], dtype=torch.float32)
    scale = ap.default_scale(HD)
    deq = lambda c: k8.dequant(c, scales, torch.float32).half()  # noqa: E731  (code * a power of two: exact in fp16)
    run = lambda K_, V_: _launch(q, K_, V_, pos, max_seq, ns, scale, "kv8", scales)  # noqa: E731
    base = run(Kc, Vc)
    assert np.isfinite(base.astype(np.float32)).all()
    head_of = np.arange(H)[:, None] * np.ones((1, HD), dtype=np.int64)
    col_of = np.ones((H, 1), dtype=np.int64) * np.arange(HD)[None, :]
    bad, tally = [], [0, 0]
    for code in (0x7F, 0xFF):
        for t in sorted({0, min(127, pos - 1), min(255, pos - 1), min(511, pos - 1), pos}):
            g0, e, c = t % HKV, 5, 77
            mine = (head_of // G) == g0
            Kp = Kc.clone()
            Kp[g0, t, e] = code
            rc = _check(f"K code {code:#x} [{g0}, {t}]", run(Kp, Vc), base, q, deq(Kp), deq(Vc), pos, scale, ~mine, bad, tally)
            assert (rc[mine] == nf.NAN).all()
            Vp = Vc.clone()
            Vp[g0, t, c] = code
            rc = _check(f"V code {code:#x} [{g0}, {t}]", run(Kc, Vp), base, q, deq(Kc), deq(Vp), pos, scale, ~(mine & (col_of == c)), bad, tally)
            assert (rc[mine & (col_of == c)] == nf.NAN).all()
    assert not bad, "%d violation(s):\n%s" % (len(bad), "\n".join(bad[:12]))


# ------------------------------------------------------------------------------------------------ the prompt attention
PH, PHKV, PHD = 4, 2, 64
BK = 64


def _prefill(q, K, V, S, start, scale, window, scales=None):
    """gq_attn_prefill / gq_attn_prefill_kv8 on guarded buffers, out a payload of 1.0; returns fp16 [S, PH * PHD]"""
    import guarded
    from guidedquant_amd import _lib
    L = _lib.lib()
    g = guarded.Guards()
    bq, bk, bv = g.inp("q", q.contiguous()), g.inp("k_cache", K.contiguous()), g.inp("v_cache", V.contiguous())
    bo = g.inp("out", np.full(S * PH * PHD, nf.SENTINEL, dtype=np.uint16))
    if scales is None:
        rc = L.gq_attn_prefill(bq.ptr(), bk.ptr(), bv.ptr(), bo.ptr(), S, start, PH, PHKV, PHD, K.shape[1], scale, window, None)
    else:
        bs = g.inp("scales", scales.contiguous())
        rc = L.gq_attn_prefill_kv8(bq.ptr(), bk.ptr(), bv.ptr(), bs.ptr(), bs.ptr(), bo.ptr(), S, start, PH, PHKV, PHD, K.shape[1], scale, window, None)
    _lib.check(rc, "gq_attn_prefill")
    g.check()
    return bo.numpy(np.float16, (S, PH, PHD))


def _prefill_ref(q, K, V, S, start, scale, window):
    """float64, IEEE, with the DEFINITION's treatment of a key a query does not attend: it is no operand (not 0 x V) -> (out [S, PH, PHD], mask)"""
    import prefill_attn_model as pam
    T = start + S
    m = pam.attend_mask(S, start, T, window)
    Kd = K[:, :T].double().repeat_interleave(PH // PHKV, dim=0)
    Vd = V[:, :T].double().repeat_interleave(PH // PHKV, dim=0)
    s = torch.einsum("hsd,htd->hst", q.double(), Kd) * float(torch.tensor(scale, dtype=torch.float32))
    s = torch.where(m[None], s, torch.full((), -float("inf"), dtype=torch.float64))
    w = torch.softmax(s, dim=-1)
    out = torch.zeros(S, PH, PHD, dtype=torch.float64)
    for i in range(S):
        att = m[i]
        out[i] = torch.einsum("ht,htd->hd", w[:, i, att], Vd[:, att])
    return out.numpy(), m.numpy()


@pytest.mark.parametrize("kv8", (False, True), ids=("fp16", "fp8"))
@pytest.mark.parametrize("S,start,window", [(70, 0, 0), (70, 5, 0), (70, 5, 17), (1, 69, 0)])
def test_prefill_poisoned_key_and_value_rows(S, start, window, kv8):
    """prefill_attn_kernel, fp16 and fp8 caches, with and without a window, a chunk at an offset, one query row.  K or V of one cached
    token t poisoned (t in the first key tile, and in the second, which the first block of 64 queries skips):
      one q element           that query's head is NaN, every other query and head bit-identical (R2);
      queries that attend t   R1 by the reference (a NaN or +Inf score: the head is NaN; -Inf: weight 0; V: that column);
      queries that do not     what the CODE guarantees, established by reading csrc/prefill_attn.hip: a masked SCORE is replaced by a select,
                              so a poisoned K row never reaches a query that does not attend it -- bit-identical to the clean launch;
                              a masked P is exactly 0 but the key's V row is still an operand of the P V matrix product wherever its
                              tile of 64 keys is not skipped as a whole, and 0 x NaN / 0 x Inf is NaN there: column c of such a query MAY
                              be NaN (counted and printed, not demanded -- SDPA's math path spreads the same way); every other column,
                              every other group's head, and every query whose block skips the tile (wholly above its diagonal or
                              below its window) is bit-identical to the clean launch."""
    import kv8_model as k8
    import prefill_attn_model as pam
    g = torch.Generator().manual_seed(S + start + window)
    T = start + S
    max_seq = T + 3
    scale = 1.0 / np.sqrt(PHD)
    q = torch.randn(PH, S, PHD, generator=g).half()
    scales = torch.tensor([0.5, 2.0], dtype=torch.float32) if kv8 else None
    if kv8:
        K = k8.random_codes((PHKV, max_seq, PHD), g, max_exp_code=0x3F)
        V = k8.random_codes((PHKV, max_seq, PHD), g, max_exp_code=0x47)
        K[:, T:], V[:, T:] = k8.stale_rows(max_seq - T, PHD), k8.stale_rows(max_seq - T, PHD)
        deq = lambda c: k8.dequant(c, scales, torch.float32).half()  # noqa: E731
        poisons = {"nan 0x7f": 0x7F, "nan 0xff": 0xFF}
    else:
        K = (torch.randn(PHKV, max_seq, PHD, generator=g) * 0.5).half()
        V = torch.randn(PHKV, max_seq, PHD, generator=g).half()
        K[:, T:], V[:, T:] = float("nan"), float("inf")
        deq = lambda c: c  # noqa: E731
        poisons = {p: _t16(b) for p, b in nf.POISONS.items()}
    run = lambda K_, V_: _prefill(q, K_, V_, S, start, scale, window, scales)  # noqa: E731
    base = run(K, V)
    assert np.isfinite(base.astype(np.float32)).all()
    vmax = float(deq(V)[:, :T].float().abs().max())
    bound = pam.error_bound(T, vmax)
    bad, spread, seen = [], 0, 0
    grp = (np.arange(PH) // (PH // PHKV))
    # one element of one q head of one query row: that query's head is NaN (a NaN score, or scores of both infinities), every other
    # query and head keeps its bits
    for (h0, i0, e) in ((1, S // 2, 0), (PH - 1, S - 1, PHD - 1)):
        for pname, bits_ in nf.POISONS.items():
            qp = q.clone()
            qp[h0, i0, e] = _t16(bits_)
            got = _prefill(qp, K, V, S, start, scale, window, scales)
            ref, _ = _prefill_ref(qp, deq(K), deq(V), S, start, scale, window)
            rc = nf.classify32(ref)
            clean = np.ones((S, PH, PHD), dtype=bool)
            clean[i0, h0] = False
            one_key = int(pam.attend_mask(S, start, T, window)[i0].sum()) == 1   # (a single attended key: softmax of one +-Inf score is NaN as well)
            assert (rc[i0, h0] == nf.NAN).all() and (rc[clean] == nf.FINITE).all(), (pname, one_key)
            b, _ = nf.check(got, rc, False, clean, base)
            bad += [f"q[{h0}, {i0}, {e}] {pname}: {v}" for v in b]
    for t in sorted({min(20, T - 1), min(68, T - 1), T - 1}):
        g0, e, c = t % PHKV, 3, 41
        tile_lo = t // BK * BK
        for pname, pv in poisons.items():
            for which in ("K", "V"):
                Kp, Vp = K.clone(), V.clone()
                (Kp if which == "K" else Vp)[g0, t, e if which == "K" else c] = pv
                got = run(Kp, Vp)
                ref, m = _prefill_ref(q, deq(Kp), deq(Vp), S, start, scale, window)
                rc = nf.classify32(ref)
                attends = m[:, t]                                  # [S]
                touched = np.zeros((S, PH, PHD), dtype=bool)       # where the definition lets the poison act
                touched[np.ix_(attends, grp == g0, np.arange(PHD) if which == "K" else np.array([c]))] = True
                assert (rc[~touched] == nf.FINITE).all() and (which == "K" or (rc[touched] != nf.FINITE).all())
                clean = ~touched
                if which == "V":   # recorded, not demanded: column c of the group's heads in queries whose block loads t's tile
                    pos_q = start + np.arange(S)
                    blk_hi = start + np.minimum((np.arange(S) // 64 + 1) * 64, S) - 1   # last position of the query's block of 64
                    loads = (blk_hi >= tile_lo) & ~attends
                    if window:
                        blk_lo = start + np.arange(S) // 64 * 64
                        loads &= (tile_lo + BK - 1) > (blk_lo - window)
                    may = np.zeros((S, PH, PHD), dtype=bool)
                    may[np.ix_(loads, grp == g0, np.array([c]))] = True
                    spread += int((~np.isfinite(got.astype(np.float32)) & may).sum())
                    seen += int(may.sum())
                    clean = clean & ~may
                b, _ = nf.check(got, rc, False, clean, base)
                bad += [f"{which}[{g0}, {t}] {pname}: {v}" for v in b]
                fin = (rc == nf.FINITE) & touched
                with np.errstate(invalid="ignore"):
                    over = fin & ~(np.abs(got.astype(np.float64) - ref) <= bound)
                if over.any():
                    bad.append(f"{which}[{g0}, {t}] {pname}: {int(over.sum())} finite element(s) of attending queries off the reference")
    print(f"prefill S {S} start {start} window {window} fp8 {kv8}: masked 0 x V made {spread} of {seen} outputs of non-attending queries non-finite")
    assert not bad, "%d violation(s):\n%s" % (len(bad), "\n".join(bad[:12]))
