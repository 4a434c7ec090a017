"""GPU: every draw of gq_sample_full against its host model (tests/sampler_full_model.py), through the C ABI, with every buffer allocated
through tests/guarded.py (guard bands and poison around the workspace, the sequence store, the log-probabilities, x_out and the sets).

Each case of sampler_full_model.CASES draws its n tokens in one go (every draw writes its token to a word of its own and its 24-byte report
is copied aside on the stream) and is read back after one synchronise.  The model is then TEACHER-FORCED with the tokens and the candidate
counts of the device.  Per case: a decided draw equals the model's token, an undecided one is admissible; n_lo <= n <= n_hi and the
reported n_k is exact; Z_k and Z_kept are within G_MASS (relative) of the model's float64 sums for the device's own n; counter, position,
tok_io, the sequence store, the seen set, x_out / ssq_out and the two log-probabilities (sampler_lp_model's bound: 4 * max(ref_err, ulp));
no guard touched; a second run on equal state is bit-identical in every output, the report included.

Over all cases: where device and model disagree with the same candidate count, the float64 margin is at most 1/8 of the grant; the largest
relative error of the two masses is at most 1/8 of G_MASS; the undecided share keeps the caps of the CPU test.

Cross-check: for top_k <= 64, top_p = 1, min_p = 0 on equal state, gq_sample_full draws gq_sample_topk_rep's token on every decided draw
(sampler_rep_model.CASES), and gq_sample_topk_p's where there is no penalty (sampler_model.CASES, entries ex / p).

The last test prints the figures.  The first MI355X run of this file printed:
    draws 6212, undecided 10, device != model 0, largest margin 0.000e+00, largest margin / granted 0.0000, device n != model n on 0 draws,
    largest mass error 1.726e-08 (G_MASS / 8 = 1.907e-06)
"""
import numpy as np
import pytest

import sampler_full_model as fm  # (tests/ is on the path: rootdir conftest)
import sampler_lp_model as lp
import sampler_model as sm
import sampler_rep_model as rm
from guarded import Guards, ptr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _i32(x):
    return x - (1 << 32) if x >= 1 << 31 else x


def _device_run(c, inputs=None, entry="full"):
    """the case's n draws through gq_sample_full (or, entry = "rep" / "p", gq_sample_topk_rep / gq_sample_topk_p with work buffers); everything
    read back"""
    from guidedquant_amd import _lib
    L = _lib.lib()
    d = "cuda:0"
    x, seen0, suppress, ban = inputs if inputs is not None else fm.case_inputs(c)
    V, n = c.V, c.n
    rp = getattr(c, "rp", 1.0)
    g = Guards(d)
    logits = g.inp("logits", x.view(np.int16))
    seen = g.inp("seen", rm.token_set(seen0, V).view(np.int32))
    sup = g.inp("suppress", rm.token_set(suppress, V).view(np.int32)) if len(suppress) else None
    ws_bytes = int(L.gq_sample_full_ws_bytes(V))
    ws = g.out("ws", ws_bytes if entry == "full" else 128 * 64 * 8)
    ctr = g.inp("counter", np.array([_i32(c.counter)], dtype=np.int32))
    pos = g.inp("pos", np.array([c.pos0], dtype=np.int32))
    tok = g.inp("tok", np.array([-5], dtype=np.int32))
    nt = g.inp("next_tok", np.full(n, -1, dtype=np.int32))
    seq = g.inp("seq", np.full(c.seq_cap, -1, dtype=np.int32))
    banw = g.inp("ban", np.array([ban[0], ban[1], *ban[2]], dtype=np.int32)) if ban is not None else None
    lpr, lpd = g.out("lp_raw", 4 * c.seq_cap), g.out("lp_drawn", 4 * c.seq_cap)
    reports = torch.zeros((n, 24), dtype=torch.uint8, device=d)
    table = xo = ssq = None
    if c.dim:
        table = g.inp("table", sm.embed_table(c).view(np.int16))
        xo, ssq = g.out("x_out", n * c.dim * 2), g.out("ssq", n * 1024 * 4)
    s = _lib.current_stream_ptr()
    wsv = ws.view(torch.uint8)
    for i in range(n):
        xi = xo.ptr() + i * c.dim * 2 if c.dim else None
        si = ssq.ptr() + i * 4096 if c.dim else None
        if entry == "full":
            rc = L.gq_sample_full(logits.ptr(), V, c.top_k, c.top_p, getattr(c, "min_p", 0.0), c.T, c.seed, ctr.ptr(), ws.ptr(), ws_bytes, tok.ptr(), pos.ptr(),
                                  nt.ptr() + 4 * i, ptr(banw), seq.ptr(), c.seq_cap, ptr(table), xi, c.dim, si, rp, seen.ptr(), ptr(sup), lpr.ptr(), lpd.ptr(),
                                  c.seq_cap, s)
            reports[i].copy_(wsv[:24])
        elif entry == "rep":
            rc = L.gq_sample_topk_rep(logits.ptr(), V, c.top_k, c.top_p, c.T, c.seed, ctr.ptr(), ws.ptr(), ws.ptr() + 128 * 64 * 4, tok.ptr(), pos.ptr(),
                                      nt.ptr() + 4 * i, ptr(banw), seq.ptr(), c.seq_cap, ptr(table), xi, c.dim, si, rp, seen.ptr(), ptr(sup), s)
        else:  # "p": the fp16-key instances, what bench.py and a default generate() launch (no penalty, no sets: `seen` stays as it is)
            assert rp == 1.0 and sup is None
            rc = L.gq_sample_topk_p(logits.ptr(), V, c.top_k, c.top_p, c.T, c.seed, ctr.ptr(), ws.ptr(), ws.ptr() + 128 * 64 * 4, tok.ptr(), pos.ptr(),
                                    nt.ptr() + 4 * i, ptr(banw), seq.ptr(), c.seq_cap, ptr(table), xi, c.dim, si, s)
        _lib.check(rc, "fused sampler")
    g.check()
    rep = reports.cpu().numpy()
    out = dict(nt=nt.numpy(np.int32), seq=seq.numpy(np.int32), ctr=int(ctr.numpy(np.int32)[0]), pos=int(pos.numpy(np.int32)[0]), tok=int(tok.numpy(np.int32)[0]),
               seen=seen.numpy(np.uint32), sup=sup.numpy(np.uint32) if sup is not None else None, lp_raw=lpr.numpy(np.float32), lp_drawn=lpd.numpy(np.float32),
               n=rep[:, 0:4].copy().view(np.uint32)[:, 0], n_k=rep[:, 4:8].copy().view(np.uint32)[:, 0], Z_k=rep[:, 8:16].copy().view(np.float64)[:, 0],
               Z_kept=rep[:, 16:24].copy().view(np.float64)[:, 0], logits=logits.numpy(np.uint16))
    if c.dim:
        out.update(x=xo.numpy(np.uint16, (n, c.dim)), ssq=ssq.numpy(np.float32, (n, 1024)))
    return out


@pytest.fixture(scope="module")
def runs():
    assert torch.cuda.is_available()
    out = {}
    for c in fm.CASES:
        out[c.name] = dev = _device_run(c)
        dev["model"] = fm.case_run(c, forced=dev["nt"].astype(np.int64), n_dev=dev["n"])
    return out


def _disagreements(c, dev):
    m = dev["model"]
    got = dev["nt"].astype(np.int64)
    return [(int(i), ) + m.margin_to(int(i), int(got[i])) for i in np.nonzero((got != m.tokens) & (dev["n"] == m.n))[0]]


def _mass_errors(c, dev):
    """relative errors of the reported Z_k and Z_kept against the model's sums over n_k and over the device's own n"""
    m = dev["model"]
    errs = []
    for i in range(c.n):
        for got, want in ((dev["Z_k"][i], m.Z_k[i]), (dev["Z_kept"][i], m.mass_at(i, int(dev["n"][i])))):
            errs.append(abs(got - want) / want if want > 0 else abs(got))
    return errs


@pytest.mark.parametrize("name", [c.name for c in fm.CASES])
def test_every_draw_equals_the_model(runs, name):
    c, dev = fm.CASE_BY_NAME[name], runs[name]
    m = dev["model"]
    x, seen0, suppress, ban = fm.case_inputs(c)
    got = dev["nt"].astype(np.int64)
    dec = ~m.undecided
    print("%s: n %d..%d (model %d..%d), n_k %d, undecided %d of %d" % (name, dev["n"].min(), dev["n"].max(), m.n.min(), m.n.max(), dev["n_k"][0], int((~dec).sum()), c.n))
    assert np.array_equal(dev["n_k"].astype(np.int64), m.n_k), (name, dev["n_k"][:4], m.n_k[:4])
    assert ((m.n_lo <= dev["n"]) & (dev["n"] <= m.n_hi)).all(), (name, dev["n"][:4], m.n_lo[:4], m.n_hi[:4])
    if c.pinned:
        assert m.cut_pinned and np.array_equal(dev["n"].astype(np.int64), m.n), name
    assert np.array_equal(got[dec], m.tokens[dec]), ("decided draws differ", name, [(i, int(got[i]), int(m.tokens[i])) for i in np.nonzero(dec & (got != m.tokens))[0][:8]])
    assert all(int(got[i]) in m.admissible[i].tolist() for i in np.nonzero(~dec)[0]), ("an undecided draw is not admissible", name)
    assert not set(got.tolist()) & set(suppress), "a suppressed token was drawn"
    errs = _mass_errors(c, dev)
    assert max(errs) <= fm.G_MASS, (name, max(errs))
    # the state after the run
    assert (dev["ctr"], dev["pos"], dev["tok"]) == (m.counter, m.pos, int(got[-1])), (name, dev["ctr"], dev["pos"], dev["tok"])
    want = np.full(c.seq_cap, -1, dtype=np.int64)
    for i in range(c.n):
        if c.pos0 + i + 1 < c.seq_cap:
            want[c.pos0 + i + 1] = got[i]
    assert np.array_equal(dev["seq"].astype(np.int64), want), name
    assert np.array_equal(dev["seen"], m.seen), (name, np.nonzero(dev["seen"] != m.seen)[0][:8])
    if dev["sup"] is not None:
        assert np.array_equal(dev["sup"], rm.token_set(suppress, c.V))
    if c.dim:
        table = sm.embed_table(c)
        assert np.array_equal(dev["x"], table[got].view(np.uint16)), name
        ref = (table[got].astype(np.float64)**2).sum(axis=1)
        tot = dev["ssq"].astype(np.float64).sum(axis=1)
        assert np.isfinite(dev["ssq"]).all() and (np.abs(tot - ref) <= 1e-6 * ref).all(), name
    # the log-probabilities: written at pos + 1 of every draw and nowhere else
    slots = [c.pos0 + i + 1 for i in range(c.n) if c.pos0 + i + 1 < c.seq_cap]
    untouched = np.ones(c.seq_cap, dtype=bool)
    untouched[slots] = False
    for arr in (dev["lp_raw"], dev["lp_drawn"]):
        assert (arr.view(np.uint32)[untouched] == 0x7E7E7E7E).all(), name
    empty = got == fm.EMPTY_TOKEN
    for i in np.nonzero(empty)[0]:
        assert np.isnan(dev["lp_raw"][c.pos0 + i + 1]) and np.isnan(dev["lp_drawn"][c.pos0 + i + 1])
    if lp.specified(x) and c.T >= 0.3:
        v32 = x.astype(np.float32)
        b_raw = 4 * max(lp.ref_err(v32), lp.ulp32(lp.lse64(v32)))
        for i in range(c.n):
            slot = c.pos0 + i + 1
            if empty[i]:
                continue
            assert abs(float(dev["lp_raw"][slot]) - m.lp_raw[slot]) <= b_raw, (name, i, dev["lp_raw"][slot], m.lp_raw[slot])
            wantd = m.lp_drawn[slot]
            assert np.isfinite(wantd), (name, i, "the drawn token is none of the device's own candidates")
            if dev["n"][i] == 1:
                assert dev["lp_drawn"][slot] == 0.0
            else:
                # (the candidates' mass is within G_MASS of itself: so is its logarithm; the difference and the result round in fp32)
                assert abs(float(dev["lp_drawn"][slot]) - wantd) <= fm.G_MASS + 4 * lp.ulp32(max(abs(wantd), 1.0)), (name, i, dev["lp_drawn"][slot], wantd)


def test_a_second_run_on_equal_state_is_bit_identical(runs):
    for name in ("v151936_k200", "rep_seeded", "v131072_quant_p_minp", "equal_k70_p_half", "embed_64", "v262144_full"):
        c = fm.CASE_BY_NAME[name]
        again = _device_run(c)
        for k, v in again.items():
            a = runs[name][k]
            same = a == v if not isinstance(v, np.ndarray) else np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(v).view(np.uint8))
            assert same, (name, k)


def test_the_draws_the_cases_are_named_for(runs):
    assert set(runs["sup_all_but_one"]["nt"].tolist()) == {137}
    assert set(runs["sup_everything"]["nt"].tolist()) == {fm.EMPTY_TOKEN} and set(runs["nan_all"]["nt"].tolist()) == {fm.EMPTY_TOKEN}
    assert runs["sup_everything"]["n"].tolist() == [0] * 8 and not runs["sup_everything"]["seen"].any()
    assert set(runs["equal_k70"]["nt"].tolist()) <= set(range(70)) and len(set(runs["equal_k70"]["nt"].tolist())) > 35
    assert runs["equal_k70"]["n"].tolist() == [70] * 200 and set(runs["equal_k70_p_half"]["n"].tolist()) <= {35, 36}
    assert runs["top_p_tiny"]["n"].tolist() == [1] * 200 and runs["v262144_k_over"]["n_k"].tolist() == [262144] * 20
    assert runs["ninf_at_cut_k65"]["n"].tolist() == [65] * 200
    assert runs["pen_before_scale"]["nt"].tolist() == [100, 200, 200, 200]  # (the penalty in front of the temperature: an exact tie, the lower id)
    x = fm.case_inputs(fm.CASE_BY_NAME["ninf_at_cut_k65"])[0]
    assert np.isfinite(x[runs["ninf_at_cut_k65"]["nt"]].astype(np.float32)).all()  # (a -inf candidate is never drawn next to a finite one)


def _same_state(c, inputs, entry):
    full = _device_run(c, inputs, "full")
    old = _device_run(c, inputs, entry)
    return full, old


@pytest.mark.parametrize("name", [c.name for c in rm.CASES if c.top_p == 1.0 and (c.V <= 4096 or c.name.startswith("layout_seen"))] +
                         ["p:" + c.name for c in sm.CASES if c.entry in ("ex", "p") and c.n <= 1000 and c.V != 32000 and c.top_p == 1.0])
def test_up_to_64_candidates_the_draw_is_the_shipped_kernels(name):
    """top_k <= 64 (>= 1), no min_p: gq_sample_full against gq_sample_topk_rep (sampler_rep_model's cases) and against gq_sample_topk_p (the
    "p:" cases of sampler_model, no penalty: the fp16-key instances) from equal state, draw for draw.  Every draw changes the state, so
    the comparison is of the whole run and stops at the first undecided draw of the model (behind it the two states may differ).  top_p = 1
    only: the nucleus of the shipped kernels compares VALUES (+0 == -0, ties by id), this one follows the order (-0 below +0)."""
    if name.startswith("p:"):
        c0 = sm.CASE_BY_NAME[name[2:]]
        x, ban = sm.case_inputs(c0)
        c = fm._case(name, c0.V, c0.prof, max(c0.top_k, 1), T=c0.T, top_p=c0.top_p, seed=c0.seed, counter=c0.counter, n=min(c0.n, 100), pos0=c0.pos0, dim=c0.dim)
        inputs = (x, (), (), ban)
        m = sm.run(x, c.n, c0.top_k, c0.T, c0.top_p, c0.seed, c0.counter, c0.pos0, ban, c.seq_cap)
    else:
        c0 = rm.CASE_BY_NAME[name]
        c = fm._case(name, c0.V, c0.prof, max(c0.top_k, 1), T=c0.T, top_p=c0.top_p, rp=c0.rp, seed=c0.seed, counter=c0.counter, n=min(c0.n, 100), pos0=c0.pos0,
                     dim=c0.dim)
        inputs = rm.case_inputs(c0)
        m = None
    full, old = _same_state(c, inputs, "p" if name.startswith("p:") else "rep")
    if m is None:
        m = rm.run(inputs[0], c.n, c0.top_k, c0.T, c0.top_p, c0.seed, c0.counter, c0.pos0, inputs[3], c.seq_cap, c0.rp, inputs[1], inputs[2],
                   forced=old["nt"].astype(np.int64))
    und = np.nonzero(m.undecided)[0]
    stop = int(und[0]) if und.size else c.n
    assert np.array_equal(full["nt"][:stop], old["nt"][:stop]), (name, stop, np.nonzero(full["nt"][:stop] != old["nt"][:stop])[0][:8])
    if stop == c.n:
        assert (full["ctr"], full["pos"], full["tok"]) == (old["ctr"], old["pos"], old["tok"])
        assert np.array_equal(full["seq"], old["seq"])
        if not name.startswith("p:"):  # (gq_sample_topk_p has no seen set)
            assert np.array_equal(full["seen"], old["seen"])
        if c.dim:
            assert np.array_equal(full["x"], old["x"]) and np.array_equal(full["ssq"].view(np.uint32), old["ssq"].view(np.uint32))


def test_refusals_write_nothing():
    from guidedquant_amd import _lib
    L = _lib.lib()
    g = Guards("cuda:0")
    V = 300
    nbytes = int(L.gq_sample_full_ws_bytes(V))
    assert nbytes > 0 and L.gq_sample_full_ws_bytes(262144) > 0 and L.gq_sample_full_ws_bytes(262145) == 0
    logits = g.inp("logits", np.zeros(V, dtype=np.float16).view(np.int16))
    ws, w = g.out("ws", nbytes), g.out("words", 64)

    def call(V=V, top_k=0, top_p=1.0, min_p=0.0, rp=1.0, seen=None, ws_bytes=nbytes, nt=w.ptr() + 8, ssq=None):
        return L.gq_sample_full(logits.ptr(), V, top_k, top_p, min_p, 1.0, 7, w.ptr(), ws.ptr(), ws_bytes, None, None, nt, None, None, 0, None, None, 0, ssq, rp,
                                seen, None, None, None, 0, _lib.current_stream_ptr())
    assert call(V=262145) == _lib.GQ_ENOTSUP
    for kw in (dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5), dict(min_p=-0.1), dict(min_p=1.5), dict(min_p=float("nan")), dict(rp=1.05), dict(rp=0.0),
               dict(ws_bytes=nbytes - 1), dict(nt=None), dict(ssq=w.ptr())):
        assert call(**kw) == _lib.GQ_EINVAL, kw
    g.check()
    assert (ws.numpy(np.uint8) == 0x7E).all() and (w.numpy(np.uint8) == 0x7E).all()


def test_disagreement_margins_masses_and_undecided_share(runs):
    worst_margin, worst_ratio, n_dis, tot, und, worst_mass, cut_moved = 0.0, 0.0, 0, 0, 0, 0.0, 0
    for c in fm.CASES:
        dev = runs[c.name]
        m = dev["model"]
        share = float(m.undecided.mean())
        assert share <= 0.05, (c.name, share)
        tot += c.n
        und += int(m.undecided.sum())
        cut_moved += int((dev["n"] != m.n).sum())
        worst_mass = max(worst_mass, max(_mass_errors(c, dev)))
        for i, mg, gr in _disagreements(c, dev):
            n_dis += 1
            print("disagreement: case %s draw %d margin %.3e granted %.3e" % (c.name, i, mg, gr))
            if np.isfinite(mg) and gr > 0:
                worst_margin, worst_ratio = max(worst_margin, mg), max(worst_ratio, mg / gr)
            else:
                worst_ratio = np.inf
    print("draws %d, undecided %d, device != model %d, largest margin %.3e, largest margin / granted %.4f, device n != model n on %d draws, "
          "largest mass error %.3e (G_MASS / 8 = %.3e)" % (tot, und, n_dis, worst_margin, worst_ratio, cut_moved, worst_mass, fm.G_MASS / 8))
    assert und <= 0.02 * tot
    assert worst_ratio <= 1.0 / 8.0, (worst_margin, worst_ratio)
    assert worst_mass <= fm.G_MASS / 8
