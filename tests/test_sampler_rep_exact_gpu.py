"""GPU: every draw of gq_sample_topk_rep against its host model (tests/sampler_rep_model.py), through the C ABI, and gq_token_set_build
against a numpy bitmap.

Each case of sampler_rep_model.CASES builds its two token sets with gq_token_set_build, draws its n tokens in one go (every draw writes
its token to a word of its own) and is read back after one synchronise.  The model is then TEACHER-FORCED with the tokens the device
drew (every draw changes the seen set).  Asserted per case: a decided draw equals the model's token, an undecided one is admissible;
counter, position, tok_io and the sequence store after the run; the seen set equal to the model's word for word, the suppress set
unchanged; x_out bit-equal to the table row of the drawn token; the words behind the work buffers and behind both sets untouched.

Identity: with repetition_penalty = 1 and no sets the entry leaves tokens, counter, position, tok_io, sequence store and embedding
output bit-equal to gq_sample_topk_p's, for every `ex` / `p` case of sampler_model.CASES, on the same device in the same test.

Over all cases: where device and model disagree, the model's float64 margin is at most 1/8 of the uncertainty it granted that pair,
and the undecided share keeps the caps of the CPU test.

The last test prints the figures (draws, undecided, disagreements, the largest margin and its share of the grant).  The first MI355X
run of this file printed:
    draws 14584, undecided 0, device != model 0, largest margin 0.000e+00, largest margin / granted 0.0000
"""
import numpy as np
import pytest

import sampler_model as sm  # (tests/ is on the path: rootdir conftest)
import sampler_rep_model as rm

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 64
NAN16 = 0x7E00
SET_GUARD = 0x5A5A5A5A
BLOCKS = sm.BLOCKS


def _p(t):
    return t.data_ptr() if t is not None else None


def _build_set(L, ids, V, d, clear=1, words=None):
    """a set of ceil(V / 32) words with GUARD words behind it, through gq_token_set_build"""
    from guidedquant_amd import _lib
    nw = (V + 31) // 32
    if words is None:
        words = torch.full((nw + GUARD, ), SET_GUARD, dtype=torch.int32, device=d)
        words[:nw] = 0x0F0F0F0F if clear else 0  # (clear = 1 must wipe what is there)
    idt = torch.tensor(list(ids), dtype=torch.int32, device=d) if len(ids) else None
    _lib.check(L.gq_token_set_build(_p(idt), len(ids), V, _p(words), clear, _lib.current_stream_ptr()), "gq_token_set_build")
    return words


def _words(t, V):
    nw = (V + 31) // 32
    a = t.cpu().numpy().view(np.uint32)
    return a[:nw], a[nw:]


def _device_run(c):
    from guidedquant_amd import _lib
    L = _lib.lib()
    d = torch.device("cuda:0")
    x, seen0, suppress, ban = rm.case_inputs(c)
    logits = torch.from_numpy(x.view(np.int16).copy()).to(d)
    wv = torch.full((BLOCKS * 64 + GUARD, ), -7.0, dtype=torch.float32, device=d)
    wi = torch.full((BLOCKS * 64 + GUARD, ), -7, dtype=torch.int32, device=d)
    ctr = torch.tensor([c.counter - (1 << 32) if c.counter >= 1 << 31 else c.counter], dtype=torch.int32, device=d)
    pos = torch.tensor([c.pos0], dtype=torch.int32, device=d)
    tok = torch.full((1, ), -5, dtype=torch.int32, device=d)
    nt = torch.full((c.n + 1, ), -1, dtype=torch.int32, device=d)
    seq = torch.full((c.seq_cap + GUARD, ), -1, dtype=torch.int32, device=d)
    banw = torch.tensor([ban[0], ban[1], *ban[2]], dtype=torch.int32, device=d) if ban is not None else None
    seen = _build_set(L, seen0, c.V, d)
    sup = _build_set(L, suppress, c.V, d) if suppress else None
    table = xo = ssq = None
    if c.dim:
        table = torch.from_numpy(sm.embed_table(c).view(np.int16)).to(d)
        xo = torch.full((c.n, c.dim), NAN16, dtype=torch.int16, device=d)
        ssq = torch.full((c.n, 1024), float("nan"), dtype=torch.float32, device=d)
    s = _lib.current_stream_ptr()
    for i in range(c.n):
        rc = L.gq_sample_topk_rep(_p(logits), c.V, c.top_k, c.top_p, c.T, c.seed, _p(ctr), _p(wv), _p(wi), _p(tok), _p(pos), nt.data_ptr() + 4 * i,
                                  _p(banw), _p(seq), c.seq_cap, _p(table), xo[i].data_ptr() if c.dim else None, c.dim,
                                  ssq[i].data_ptr() if c.dim else None, c.rp, _p(seen), _p(sup), s)
        _lib.check(rc, "gq_sample_topk_rep")
    torch.cuda.synchronize()
    out = dict(nt=nt.cpu().numpy(), seq=seq.cpu().numpy(), ctr=int(ctr.item()), pos=int(pos.item()), tok=int(tok.item()),
               guards=(wv[BLOCKS * 64:].cpu().numpy(), wi[BLOCKS * 64:].cpu().numpy()), seen=_words(seen, c.V),
               sup=_words(sup, c.V) if sup is not None else None)
    if c.dim:
        out.update(x=xo.cpu().numpy(), ssq=ssq.cpu().numpy())
    return out


@pytest.fixture(scope="module")
def runs():
    """every case on the device, once, and the model teacher-forced with the tokens the device drew"""
    assert torch.cuda.is_available()
    out = {}
    for c in rm.CASES:
        out[c.name] = dev = _device_run(c)
        dev["model"] = rm.case_run(c, forced=dev["nt"][:c.n].astype(np.int64))
    return out


def _disagreements(c, dev):
    """[(draw, margin, granted)] of the draws whose device token is not the model's"""
    m = dev["model"]
    got = dev["nt"][:c.n].astype(np.int64)
    return [(int(i), ) + m.margin_to(int(i), int(got[i])) for i in np.nonzero(got != m.tokens)[0]]


@pytest.mark.parametrize("name", [c.name for c in rm.CASES])
def test_every_draw_equals_the_model(runs, name):
    c, dev = rm.CASE_BY_NAME[name], runs[name]
    bad, m = _disagreements(c, dev), dev["model"]
    x, seen0, suppress, ban = rm.case_inputs(c)
    got = dev["nt"][:c.n].astype(np.int64)
    assert dev["nt"][c.n] == -1
    bad = [(i, int(got[i]), int(m.tokens[i]), mg, gr) for i, mg, gr in bad]
    dec = ~m.undecided
    assert np.array_equal(got[dec], m.tokens[dec]), ("decided draws differ", name, [(i, int(got[i]), int(m.tokens[i])) for i in np.nonzero(dec & (got != m.tokens))[0][:8]])
    assert all(int(got[i]) in m.admissible[i].tolist() for i in np.nonzero(~dec)[0]), ("an undecided draw is not admissible", name, bad[:8])
    assert not set(got.tolist()) & set(suppress), "a suppressed token was drawn"
    # the state after the run
    assert (dev["ctr"], dev["pos"], dev["tok"]) == (m.counter, m.pos, int(got[-1])), (name, dev["ctr"], dev["pos"], dev["tok"])
    want = np.full(c.seq_cap + GUARD, -1, dtype=np.int64)
    for i in range(c.n):
        if c.pos0 + i + 1 < c.seq_cap:
            want[c.pos0 + i + 1] = got[i]
    assert np.array_equal(dev["seq"].astype(np.int64), want), name
    assert m.seq == {k: int(dev["seq"][k]) for k in m.seq}
    # the sets: seen = what the model's set is after the same tokens, word for word; suppress untouched; nothing behind either
    assert np.array_equal(dev["seen"][0], m.seen), (name, np.nonzero(dev["seen"][0] != m.seen)[0][:8])
    assert np.array_equal(m.seen, rm.token_set(list(seen0) + [t for t in got.tolist() if t < c.V], c.V))
    assert (dev["seen"][1] == SET_GUARD).all(), "the seen set was written past its end"
    if dev["sup"] is not None:
        assert np.array_equal(dev["sup"][0], rm.token_set(suppress, c.V)) and (dev["sup"][1] == SET_GUARD).all()
    assert (dev["guards"][0] == -7.0).all() and (dev["guards"][1] == -7).all(), "a work buffer was written past its end"
    if c.dim:
        table = sm.embed_table(c)
        assert np.array_equal(dev["x"].view(np.uint16), table[got].view(np.uint16)), name
        ref = (table[got].astype(np.float64)**2).sum(axis=1)
        tot = dev["ssq"].astype(np.float64).sum(axis=1)
        assert np.isfinite(dev["ssq"]).all() and (np.abs(tot - ref) <= 1e-6 * ref).all(), (name, float((np.abs(tot - ref) / ref).max()))


def test_the_draws_the_cases_are_named_for(runs):
    """what must hold on the device whatever the race decides"""
    for name in ("state_v300", "state_v131073"):  # every draw penalises itself
        assert runs[name]["nt"][:300].tolist() == list(range(300)), name
    assert runs["between_fp16_greedy"]["nt"][:2].tolist() == [20, 10]  # (fp16 neighbour above, then the penalised token: never id 5 first)
    assert set(runs["between_fp16_k2"]["nt"][:1].tolist()) <= {20, 10}
    assert runs["tie_seen_lower"]["nt"][0] == 40 and runs["tie_seen_higher"]["nt"][0] == 40
    assert set(runs["sup_all_but_one"]["nt"][:16].tolist()) == {137}
    assert set(runs["layout_sup_v1"]["nt"][:16].tolist()) == {rm.EMPTY_TOKEN}  # (an empty candidate set: INT_MAX, as the old entry points)
    for k in (1, 32, 33, 64):
        c = rm.CASE_BY_NAME["cut_k%d" % k]
        top = np.lexsort((np.arange(c.V), -sm.order_key(rm.case_logits(c).view(np.uint16))))[:k + 1]
        assert int(runs[c.name]["nt"][0]) in top[1:].tolist()


def _old_and_new(c):
    """the case through gq_sample_topk_p / _ex and through gq_sample_topk_rep(rp = 1, no sets): two states, same inputs"""
    from guidedquant_amd import _lib
    L = _lib.lib()
    d = torch.device("cuda:0")
    x, ban = sm.case_inputs(c)
    logits = torch.from_numpy(x.view(np.int16).copy()).to(d)
    banw = torch.tensor([ban[0], ban[1], *ban[2]], dtype=torch.int32, device=d) if ban is not None else None
    table = torch.from_numpy(sm.embed_table(c).view(np.int16)).to(d) if c.dim else None
    s = _lib.current_stream_ptr()
    outs = []
    for new in (False, True):
        wv = torch.full((BLOCKS * 64 + GUARD, ), -7.0, dtype=torch.float32, device=d)
        wi = torch.full((BLOCKS * 64 + GUARD, ), -7, dtype=torch.int32, device=d)
        ctr = torch.tensor([c.counter - (1 << 32) if c.counter >= 1 << 31 else c.counter], dtype=torch.int32, device=d)
        pos = torch.tensor([c.pos0], dtype=torch.int32, device=d)
        tok = torch.full((1, ), -5, dtype=torch.int32, device=d)
        nt = torch.full((c.n + 1, ), -1, dtype=torch.int32, device=d)
        seq = torch.full((c.seq_cap + GUARD, ), -1, dtype=torch.int32, device=d)
        xo = torch.full((c.n, max(c.dim, 1)), NAN16, dtype=torch.int16, device=d)
        ssq = torch.full((c.n, 1024), float("nan"), dtype=torch.float32, device=d)
        for i in range(c.n):
            a = (_p(logits), c.V, c.top_k, c.top_p, c.T, c.seed, _p(ctr), _p(wv), _p(wi), _p(tok), _p(pos), nt.data_ptr() + 4 * i, _p(banw), _p(seq), c.seq_cap,
                 _p(table), xo[i].data_ptr() if c.dim else None, c.dim, ssq[i].data_ptr() if c.dim else None)
            rc = L.gq_sample_topk_rep(*a, 1.0, None, None, s) if new else L.gq_sample_topk_p(*a, s)
            _lib.check(rc, "fused sampler")
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy() for t in (nt, seq, ctr, pos, tok, xo, ssq, wv[BLOCKS * 64:], wi[BLOCKS * 64:])])
    return outs


@pytest.mark.parametrize("name", [c.name for c in sm.CASES if c.entry in ("ex", "p")])
def test_without_penalty_and_sets_the_entry_is_the_old_one(name):
    old, new = _old_and_new(sm.CASE_BY_NAME[name])
    for a, b, what in zip(old, new, ("next_tok", "seq_out", "counter", "pos_io", "tok_io", "x_out", "ssq_out", "guard", "guard")):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (name, what)


def test_token_set_build_against_a_numpy_bitmap():
    from guidedquant_amd import _lib
    L = _lib.lib()
    d = torch.device("cuda:0")
    rng = np.random.default_rng(5)
    for V in (1, 2, 33, 300, 4096, 131073, 151936, 262144):
        nw = (V + 31) // 32
        ids = rng.integers(0, V, 500).tolist() + [0, 0, V - 1, V - 1, 31 % V, 32 % V, V, V + 31, -1, -2**31, 2**31 - 1]  # duplicates, out of range
        w = _build_set(L, ids, V, d, clear=1)
        got, guard = _words(w, V)
        assert np.array_equal(got, rm.token_set(ids, V)) and (guard == SET_GUARD).all(), V
        # clear = 0 adds to what is there; n = 0 with clear = 0 changes nothing; n = 0 with clear = 1 clears
        more = rng.integers(0, V, 40).tolist()
        _build_set(L, more, V, d, clear=0, words=w)
        got, guard = _words(w, V)
        assert np.array_equal(got, rm.token_set(ids + more, V)) and (guard == SET_GUARD).all(), V
        _build_set(L, [], V, d, clear=0, words=w)
        assert np.array_equal(_words(w, V)[0], rm.token_set(ids + more, V))
        _build_set(L, [], V, d, clear=1, words=w)
        got, guard = _words(w, V)
        assert not got.any() and (guard == SET_GUARD).all() and got.size == nw, V
    # a long history: more ids than the block has threads
    V = 151936
    ids = rng.integers(0, V, 20000).tolist()
    assert np.array_equal(_words(_build_set(L, ids, V, d), V)[0], rm.token_set(ids, V))


def test_disagreement_margins_and_undecided_share(runs):
    worst_margin, worst_ratio, n_dis, tot, und = 0.0, 0.0, 0, 0, 0
    for c in rm.CASES:
        dis, m = _disagreements(c, runs[c.name]), runs[c.name]["model"]
        share = float(m.undecided.mean())
        assert share <= 0.05, (c.name, share)
        assert m.boundary_dist >= 1e-5, (c.name, m.boundary_dist)
        tot += c.n
        und += int(m.undecided.sum())
        for i, mg, gr in dis:
            n_dis += 1
            print("disagreement: case %s draw %d margin %.3e granted %.3e" % (c.name, i, mg, gr))
            if np.isfinite(mg) and gr > 0:
                worst_margin, worst_ratio = max(worst_margin, mg), max(worst_ratio, mg / gr)
            else:
                worst_ratio = np.inf
    print("draws %d, undecided %d, device != model %d, largest margin %.3e, largest margin / granted %.4f" % (tot, und, n_dis, worst_margin, worst_ratio))
    assert und <= 0.02 * tot
    assert worst_ratio <= 1.0 / 8.0, (worst_margin, worst_ratio)
