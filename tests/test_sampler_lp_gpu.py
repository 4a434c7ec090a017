"""GPU: gq_sample_topk_lp through the C ABI against tests/sampler_lp_model.py, on tests/guarded.py buffers.

Cases: every `ex` / `p` case of sampler_model.CASES (penalty 1, no sets) and every case of sampler_rep_model.CASES.  Each case runs three
times from the same state: through gq_sample_topk_rep, and twice through gq_sample_topk_lp.  Outputs and the workspace start poisoned
(guarded.POISON: 0x7E7E7E7E, 8.4e37 as a float); the guards of everything the entry may write are checked after EVERY call of the first
gq_sample_topk_lp run, and all guards at the end of every run.

Per case
  draw unchanged   next_tok, seq_out, counter, pos_io, tok_io, x_out, ssq_out and the seen set of the new entry equal the old entry's, byte
                   for byte
  lp_raw           every draw: |got - model| <= 4 * max(ref_err(logits), ulp32(|lse|)), ref_err = the error of torch's CPU fp32
                   log_softmax against float64 ON THE CASE'S OWN LOGITS (sampler_lp_model.ref_err), lse the float64 log-sum.  The factor is
                   the one of tests/test_head_nll_gpu.py: one exp rounding of the rescale per partial and per combine level on top of a
                   one-pass fp32 softmax
  lp_drawn         T >= 0.3: the same bound with ref_err and lse taken on the kept candidates' a_c, on every draw whose kept set the
                   model decides -- all of them with top_p == 1 (the set is the key-exact top-k); with top_p < 1 the draws whose
                   nucleus cut is at least 1e-5 from every cumulative sum.  LEFT OUT by that rule: every draw of `equal_k2_p_half`
                   (built on the threshold) and of no other case.  T == 0: finite, <= 0, and == 0.0 when the model's kept set has one
                   member.  top_k == 1: exactly 0.0
  slots            every slot outside [pos0 + 1, pos0 + n], and every slot at or past lp_cap, keeps the poison; `seq_cap_short` runs with
                   an lp_cap shorter than the run
  determinism      the two gq_sample_topk_lp runs leave identical bits in both arrays
`values_plus_inf` holds a +inf logit: the contract leaves its two numbers unspecified, so only draw, slots and determinism are checked.

The worst ratio to the bound is printed per case.  The first MI355X run of this file: 95 cases compared, the worst lp_raw at 0.367 of its
bound (state_v131073), the worst lp_drawn at 0.334 (values_rp1.3).
"""
import functools

import numpy as np
import pytest

import guarded
import sampler_lp_model as lp
import sampler_model as sm
import sampler_rep_model as rm

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

BLOCKS = sm.BLOCKS
POISON32 = np.uint32(0x7E7E7E7E)
EXTRA = 8  # slots of the two arrays behind lp_cap
FACTOR = 4.0


def _i32(v):
    return np.array(v, dtype=np.int32).reshape(-1)


def _run(c, entry, lp_cap=None, raw=True, drawn=True, ws=True, check_each=False, top_k=None, V=None, expect=0, x=None):
    """one case through `entry` ("rep" or "lp") from its initial state; the state afterwards as numpy arrays"""
    from guidedquant_amd import _lib
    L = _lib.lib()
    x0, kw = lp.case_args(c)
    x = x0 if x is None else x  # (x: logits in place of the case's own)
    ban, seen0, suppress, rp = kw["ban"], kw.get("seen0"), kw.get("suppress"), float(kw.get("rp", 1.0))
    lp_len = c.pos0 + c.n + 2 + EXTRA
    gi, go = guarded.Guards(), guarded.Guards()
    logits = gi.inp("logits", x.view(np.int16))
    banw = gi.inp("ban", _i32([ban[0], ban[1], *ban[2]]) if ban is not None else None)
    table = gi.inp("table", sm.embed_table(c).view(np.int16) if c.dim else None)
    wv, wi = go.out("work_val", 4 * BLOCKS * 64), go.out("work_idx", 4 * BLOCKS * 64)
    ctr = go.inp("counter", _i32([c.counter - (1 << 32) if c.counter >= 1 << 31 else c.counter]))
    pos, tok = go.inp("pos", _i32([c.pos0])), go.inp("tok", _i32([-5]))
    nt, seq = go.out("next_tok", 4 * (c.n + 1)), go.out("seq", 4 * c.seq_cap)
    xo = go.out("x_out", 2 * c.n * c.dim) if c.dim else None
    ssq = go.out("ssq_out", 4 * c.n * 1024) if c.dim else None
    seen = sup = None
    s = _lib.current_stream_ptr()
    if seen0 is not None:  # (a case of sampler_rep_model: both sets through gq_token_set_build)
        nw = (c.V + 31) // 32
        seen = go.out("seen", 4 * nw)
        ids = torch.tensor(list(seen0), dtype=torch.int32, device="cuda:0") if len(seen0) else None
        _lib.check(L.gq_token_set_build(ids.data_ptr() if ids is not None else None, len(seen0), c.V, seen.ptr(), 1, s), "gq_token_set_build")
        if suppress:
            sup = gi.out("suppress", 4 * nw)
            ids = torch.tensor(list(suppress), dtype=torch.int32, device="cuda:0")
            _lib.check(L.gq_token_set_build(ids.data_ptr(), len(suppress), c.V, sup.ptr(), 1, s), "gq_token_set_build")
    lws = go.out("lp_ws", 4 * 2 * BLOCKS)
    lraw, ldrawn = go.out("lp_raw", 4 * lp_len), go.out("lp_drawn", 4 * lp_len)
    cap = c.pos0 + c.n + 2 if lp_cap is None else lp_cap
    for i in range(c.n):
        a = (logits.ptr(), c.V if V is None else V, c.top_k if top_k is None else top_k, c.top_p, c.T, c.seed, ctr.ptr(), wv.ptr(), wi.ptr(), tok.ptr(), pos.ptr(),
             nt.ptr() + 4 * i, guarded.ptr(banw), seq.ptr(), c.seq_cap, guarded.ptr(table), xo.ptr() + 2 * c.dim * i if c.dim else None, c.dim,
             ssq.ptr() + 4096 * i if c.dim else None, rp, guarded.ptr(seen), guarded.ptr(sup))
        if entry == "rep":
            rc = L.gq_sample_topk_rep(*a, s)
        else:
            rc = L.gq_sample_topk_lp(*a, lws.ptr() if ws else None, lraw.ptr() if raw else None, ldrawn.ptr() if drawn else None, cap, s)
        assert rc == expect, (c.name, entry, rc, L.gq_last_error())
        if check_each:
            go.check()
    go.check()
    gi.check()
    out = dict(nt=nt.numpy(np.int32), seq=seq.numpy(np.int32), ctr=ctr.numpy(np.int32), pos=pos.numpy(np.int32), tok=tok.numpy(np.int32),
               raw=lraw.numpy(np.float32), drawn=ldrawn.numpy(np.float32), ws=lws.numpy(np.uint32), wv=wv.numpy(np.uint32))
    if seen is not None:
        out["seen"] = seen.numpy(np.uint32)
    if c.dim:
        out.update(x=xo.numpy(np.uint16), ssq=ssq.numpy(np.uint32))
    return out


STATE = ("nt", "seq", "ctr", "pos", "tok", "seen", "x", "ssq")


def _same_state(a, b):
    return [k for k in STATE if k in a and not np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8))]


def _lp_cap(c):
    return c.pos0 + c.n // 2 if c.name == "seq_cap_short" else c.pos0 + c.n + 2


@functools.lru_cache(maxsize=None)
def _case(name):
    """the three device runs of a case and the model teacher-forced with the tokens of the first gq_sample_topk_lp run"""
    assert torch.cuda.is_available()
    c = lp.CASE_BY_NAME[name]
    old = _run(c, "rep")
    new = _run(c, "lp", lp_cap=_lp_cap(c), check_each=True)
    again = _run(c, "lp", lp_cap=_lp_cap(c))
    x, kw = lp.case_args(c)
    model = lp.run(x, new["nt"][:c.n].astype(np.int64), lp_cap=_lp_cap(c), **kw)
    return c, x, old, new, again, model


@functools.lru_cache(maxsize=4096)
def _ref_err_of(values):
    return lp.ref_err(np.frombuffer(values, dtype=np.float32))


def _bound(values32, lse):
    """4 * max(ref_err(values), ulp32(|lse|))"""
    v = np.ascontiguousarray(values32, dtype=np.float32)
    return FACTOR * max(_ref_err_of(v.tobytes()), lp.ulp32(lse))


@pytest.mark.parametrize("name", [c.name for c in lp.ALL_CASES])
def test_case(name):
    c, x, old, new, again, model = _case(name)
    # the draw is gq_sample_topk_rep's
    assert _same_state(old, new) == [], name
    assert new["nt"][c.n] == np.int32(0x7E7E7E7E)
    # slots: poison everywhere but in [pos0 + 1, pos0 + n] below lp_cap
    cap = _lp_cap(c)
    written = np.zeros(new["raw"].size, dtype=bool)
    written[c.pos0 + 1:min(c.pos0 + c.n + 1, cap)] = True
    for arr in ("raw", "drawn"):
        bits = new[arr].view(np.uint32)
        assert (bits[~written] == POISON32).all(), (name, arr, "a slot outside the run or past lp_cap was written", np.nonzero(bits[~written] != POISON32)[0][:8])
        assert (bits[written] != POISON32).all(), (name, arr, "a slot of the run was not written")
        assert np.array_equal(bits, again[arr].view(np.uint32)), (name, arr, "two runs from the same state differ")
    assert sorted(model.raw) == np.nonzero(written)[0].tolist()
    if not lp.specified(x):
        print("%s: logits outside the contract (+inf / NaN / all -inf): the two numbers are not compared" % name)
        return
    b_raw = _bound(x.astype(np.float32), model.draws[0].lse_raw) if np.isfinite(model.draws[0].lse_raw) else 0.0
    worst_raw = worst_drawn = 0.0
    compared = 0
    for d in model.draws:
        if d.slot is None:
            continue
        g_raw, g_drawn = float(new["raw"][d.slot]), float(new["drawn"][d.slot])
        if np.isnan(d.raw):  # an empty candidate set
            assert d.member and np.isnan(g_raw) and np.isnan(g_drawn), (name, d.slot, g_raw, g_drawn)
            continue
        err = abs(g_raw - d.raw)
        worst_raw = max(worst_raw, err / b_raw)
        assert err <= b_raw, (name, "lp_raw", d.slot, g_raw, d.raw, err, b_raw)
        if c.top_k == 1:
            assert g_drawn == 0.0, (name, d.slot, g_drawn)
        if c.T == 0.0:
            assert np.isfinite(g_drawn) and g_drawn <= 0.0, (name, d.slot, g_drawn)
            if d.ids.size == 1:
                assert g_drawn == 0.0, (name, d.slot, g_drawn)
        elif c.T >= 0.3 and (c.top_p >= 1.0 or d.decided):
            assert d.member, (name, d.slot, "the drawn token is no kept candidate of the model")
            b = _bound(d.a, d.lse_drawn)
            err = abs(g_drawn - d.drawn)
            worst_drawn = max(worst_drawn, err / b)
            assert err <= b, (name, "lp_drawn", d.slot, g_drawn, d.drawn, err, b)
            compared += 1
    print("%s: worst |lp_raw - model| / bound %.3f (bound %.3e), worst |lp_drawn - model| / bound %.3f on %d of %d draws"
          % (name, worst_raw, b_raw, worst_drawn, compared, c.n))
    if c.T >= 0.3 and name != "equal_k2_p_half":
        assert compared == sum(d.slot is not None and not np.isnan(d.raw) for d in model.draws), (name, "draws left out of the lp_drawn comparison")


def test_one_logit_far_above_the_rest_in_the_last_slice():
    V = 262144
    big = V - 7
    c = rm._case("one_high", V, "flat", 50, 1.0, 1.0, n=8)
    x = np.full(V, -60000.0, dtype=np.float16)
    x[big] = np.float16(60000.0)
    new = _run(c, "lp", check_each=True, x=x)
    assert new["nt"][:c.n].tolist() == [big] * c.n
    assert (new["raw"][1:c.n + 1] == 0.0).all(), new["raw"][1:c.n + 1]
    assert (new["drawn"][1:c.n + 1] <= 0.0).all() and np.isfinite(new["drawn"][1:c.n + 1]).all()


def test_a_banned_argmax_still_counts_in_the_sum():
    c = sm.CASE_BY_NAME["ban_argmax"]
    _, x, old, new, again, model = _case(c.name)
    top = int(sm.candidates(x, 1)[0])
    v = x.astype(np.float64)
    without = lp.lse64(np.delete(v, top))
    assert top not in new["nt"][:c.n].tolist()
    for d in model.draws:
        tokv = float(v[int(new["nt"][d.slot - 1 - c.pos0])])
        assert float(new["raw"][d.slot]) < tokv - without - 1e-3, d.slot  # (the arg-max of 32000 gaussians carries far more than 1e-3 of the mass)


def test_everything_suppressed_gives_nan_and_the_state_of_rep():
    c = rm._case("all_suppressed", 300, "gauss", 50, 1.0, 1.3, suppress=tuple(range(300)), seen0=(3, 4), n=6, pos0=2)
    old, new = _run(c, "rep"), _run(c, "lp", check_each=True)
    assert _same_state(old, new) == []
    assert new["nt"][:c.n].tolist() == [rm.EMPTY_TOKEN] * c.n
    assert np.isnan(new["raw"][3:9]).all() and np.isnan(new["drawn"][3:9]).all()
    assert (new["raw"].view(np.uint32)[:3] == POISON32).all() and (new["raw"].view(np.uint32)[9:] == POISON32).all()


def test_argument_forms():
    from guidedquant_amd import _lib
    c = rm.CASE_BY_NAME["sup_nucleus_embed"]
    both = _case(c.name)[3]
    only_raw = _run(c, "lp", drawn=False, check_each=True)
    only_drawn = _run(c, "lp", raw=False, ws=False, check_each=True)
    assert np.array_equal(only_raw["raw"].view(np.uint32), both["raw"].view(np.uint32)) and (only_raw["drawn"].view(np.uint32) == POISON32).all()
    assert np.array_equal(only_drawn["drawn"].view(np.uint32), both["drawn"].view(np.uint32)) and (only_drawn["raw"].view(np.uint32) == POISON32).all()
    assert (only_drawn["ws"] == POISON32).all(), "the workspace was written although lp_raw is NULL"
    assert _same_state(both, only_raw) == [] and _same_state(both, only_drawn) == []
    neither = _run(c, "lp", raw=False, drawn=False, check_each=True)
    assert _same_state(_case(c.name)[2], neither) == []
    assert (neither["raw"].view(np.uint32) == POISON32).all() and (neither["drawn"].view(np.uint32) == POISON32).all() and (neither["ws"] == POISON32).all()
    # refused calls write nothing at all
    one = c._replace(n=1)
    for kw, rc in ((dict(ws=False), _lib.GQ_EINVAL), (dict(top_k=65), _lib.GQ_ENOTSUP), (dict(V=262145), _lib.GQ_ENOTSUP)):
        out = _run(one, "lp", expect=rc, **kw)
        assert out["ctr"][0] == one.counter and out["pos"][0] == one.pos0 and out["tok"][0] == -5, kw
        for k in ("nt", "seq", "raw", "drawn", "ws", "wv", "x", "ssq"):
            assert (out[k].view(np.uint8) == guarded.POISON).all(), (kw, k)


def _nan_seen_case():
    """the penalised NaN: the NaN ids of nan_few are in the history (s = NaN * rp or NaN / rp is NaN: the fp32 keys)"""
    ids = tuple(int(t) for t in np.flatnonzero(np.isnan(sm.profile("nan_few", 4096).astype(np.float32))))
    return rm._case("nan_few_seen_rp1.3", 4096, "nan_few", 50, 0.8, 1.3, seen0=ids + (17, 18), n=300)


NAN_LP_CASES = [c for c in sm.NAN_CASES if c.entry in ("ex", "p")] + [_nan_seen_case()]


@pytest.mark.parametrize("c", NAN_LP_CASES, ids=lambda c: c.name)
def test_nan_logits_through_rep_and_lp(c):
    """NaN logits through gq_sample_topk_rep and gq_sample_topk_lp: no NaN token is drawn and the decided draws are the model's; lp_raw,
    whose sum runs over ALL logits, is NaN for every draw (no hiding); lp_drawn is taken over the kept candidates and keeps the bound of
    test_case; all logits NaN: the empty set's token and NaN in both"""
    x, kw = lp.case_args(c)
    old, new = _run(c, "rep"), _run(c, "lp", check_each=True)
    assert _same_state(old, new) == [], c.name
    got = new["nt"][:c.n].astype(np.int64)
    nan = np.isnan(x.astype(np.float32))
    if hasattr(c, "rp"):
        m = rm.case_run(c)
    else:
        m = sm.case_run(c)
    dec = ~m.undecided
    assert np.array_equal(got[dec], m.tokens[dec]), ("decided draws differ", c.name, [(i, int(got[i]), int(m.tokens[i])) for i in np.nonzero(dec & (got != m.tokens))[0][:8]])
    live = got != rm.EMPTY_TOKEN
    assert not nan[got[live]].any() and live.all() != nan.all()
    sl = slice(c.pos0 + 1, c.pos0 + c.n + 1)
    assert np.isnan(new["raw"][sl]).all(), (c.name, "lp_raw hides a NaN logit", new["raw"][sl][:8])
    if nan.all():
        assert np.isnan(new["drawn"][sl]).all()
        return
    model = lp.run(x, got, lp_cap=c.pos0 + c.n + 2, **kw)
    compared = 0
    for d in model.draws:
        g = float(new["drawn"][d.slot])
        assert np.isnan(d.raw) and d.member
        if c.top_k == 1:
            assert g == 0.0
        if c.T == 0.0:
            assert np.isfinite(g) and g <= 0.0
        elif c.top_p >= 1.0 or d.decided:
            assert abs(g - d.drawn) <= _bound(d.a, d.lse_drawn), (c.name, d.slot, g, d.drawn)
            compared += 1
    assert c.T == 0.0 or compared >= c.n // 2
