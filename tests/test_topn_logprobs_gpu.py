"""GPU: the top-n alternatives of gq_sample_topk_lp_topn and gq_sample_full_topn through the C ABI against tests/topn_model.py, on
tests/guarded.py buffers (outputs and workspaces start poisoned; every guard is checked after every call).

What is compared, per call
  ids, bits     top_ids and the BIT PATTERNS of top_lps equal the model's, teacher-forced with the (M, L) the device left in the first two
                floats of topn_ws (the documented test hook): the model then says which ids and which fp32 bits follow
  (M, L)        M + L against the float64 log-sum-exp of the logits within lp_raw's grant (topn_model.grant), where lp_raw is specified
  consistency   a drawn token found in the list has top_lps == lp_raw on the bit patterns; on both samplers
  draw          everything the entry without the suffix writes is byte-identical with and without the request (_same_state, lp_raw / lp_drawn)
  rows          every row but the step's keeps the poison
Sizes: vocab 1, 5, 1000, 131072, 131073 (the first size of the wide-slice instances), 151936, 262144 x n = 1, 5, 20; placements that break
a merge at a narrow and a wide ragged vocabulary; the index rule at the cap and with pos_io NULL; the refusals.
"""
import functools

import numpy as np
import pytest

import guarded
import sampler_lp_model as lp
import sampler_model as sm
import topn_model as tm

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

BLOCKS = 128
POISON32 = np.uint32(0x7E7E7E7E)
INT_MAX = 0x7FFFFFFF
STATE = ("nt", "seq", "ctr", "pos", "tok", "seen", "x", "ssq", "raw", "drawn")
NARROW, WIDE = 32001, 150001  # ragged last slices: 128 x 251 - 127, 128 x 1172 - 15


def _i32(v):
    return np.array(v, dtype=np.int32).reshape(-1)


def _run(x, n, sampler="lp", topn=True, steps=1, pos0=0, cap=None, top_k=50, T=1.0, top_p=1.0, min_p=0.0, ban=None, suppress=(), seen0=None, rp=1.0,
         dim=0, seed=77, counter=5, expect=0, V=None, null=()):
    """`steps` draws through gq_sample_topk_lp[_topn] ("lp") or gq_sample_full[_topn] ("full") from one initial state; the state afterwards.
    pos0 None: pos_io NULL.  null: names of pointers passed as NULL (top_ids, top_lps, topn_ws, lp_raw, lp_ws)."""
    from guidedquant_amd import _lib
    L = _lib.lib()
    x = np.ascontiguousarray(x, dtype=np.float16)
    Vx = x.size
    V = Vx if V is None else V
    p0 = 0 if pos0 is None else pos0
    cap = p0 + steps + 2 if cap is None else cap
    rows = cap + 3
    seq_cap = p0 + steps + 2
    gi, go = guarded.Guards(), guarded.Guards()
    logits = gi.inp("logits", x.view(np.int16))
    banw = gi.inp("ban", _i32([ban[0], ban[1], *ban[2]]) if ban is not None else None)
    table = gi.inp("table", ((np.arange(Vx * dim) % 251).astype(np.float16) / 16).view(np.int16) if dim else None)
    ctr = go.inp("counter", _i32([counter]))
    pos, tok = go.inp("pos", _i32([p0])), go.inp("tok", _i32([-5]))
    nt, seq = go.out("next_tok", 4 * (steps + 1)), go.out("seq", 4 * seq_cap)
    xo = go.out("x_out", 2 * steps * dim) if dim else None
    ssq = go.out("ssq_out", 4 * steps * 1024) if dim else None
    s = _lib.current_stream_ptr()
    seen = sup = None
    nw = (Vx + 31) // 32
    if seen0 is not None:
        seen = go.out("seen", 4 * nw)
        ids = torch.tensor(list(seen0), dtype=torch.int32, device="cuda:0") if len(seen0) else None
        _lib.check(L.gq_token_set_build(ids.data_ptr() if ids is not None else None, len(seen0), Vx, seen.ptr(), 1, s), "gq_token_set_build")
    if len(suppress):
        sup = gi.out("suppress", 4 * nw)
        ids = torch.tensor(list(suppress), dtype=torch.int32, device="cuda:0")
        _lib.check(L.gq_token_set_build(ids.data_ptr(), len(suppress), Vx, sup.ptr(), 1, s), "gq_token_set_build")
    lraw, ldrawn = go.out("lp_raw", 4 * rows), go.out("lp_drawn", 4 * rows)
    nn = max(n, 1)
    tids, tlps, tws = go.out("top_ids", 4 * rows * nn), go.out("top_lps", 4 * rows * nn), go.out("topn_ws", _lib.TOPN_WS_BYTES)
    if sampler == "lp":
        wv, wi, lws = go.out("work_val", 4 * BLOCKS * 64), go.out("work_idx", 4 * BLOCKS * 64), go.out("lp_ws", 4 * 2 * BLOCKS)
    else:
        ws = go.out("ws", L.gq_sample_full_ws_bytes(Vx))

    def P(name, b):
        return None if name in null else b.ptr()
    hooks = []
    for i in range(steps):
        tail = (guarded.ptr(banw), seq.ptr(), seq_cap, guarded.ptr(table), xo.ptr() + 2 * dim * i if dim else None, dim, ssq.ptr() + 4096 * i if dim else None,
                rp, guarded.ptr(seen), guarded.ptr(sup))
        io = (tok.ptr(), None if pos0 is None else pos.ptr(), nt.ptr() + 4 * i)
        if sampler == "lp":
            a = (logits.ptr(), V, top_k, top_p, T, seed, ctr.ptr(), wv.ptr(), wi.ptr()) + io + tail + (P("lp_ws", lws), P("lp_raw", lraw), ldrawn.ptr(), cap)
            fn = L.gq_sample_topk_lp_topn if topn else L.gq_sample_topk_lp
        else:
            a = (logits.ptr(), V, top_k, top_p, min_p, T, seed, ctr.ptr(), ws.ptr(), ws.nbytes) + io + tail + (P("lp_raw", lraw), ldrawn.ptr(), cap)
            fn = L.gq_sample_full_topn if topn else L.gq_sample_full
        if topn:
            a = a + (n, P("top_ids", tids), P("top_lps", tlps), P("topn_ws", tws))
        rc = fn(*a, s)
        assert rc == expect, (sampler, topn, rc, L.gq_last_error())
        go.check()
        if topn and rc == 0:
            hooks.append(tws.numpy(np.float32)[:2].copy())
    gi.check()
    out = dict(nt=nt.numpy(np.int32), seq=seq.numpy(np.int32), ctr=ctr.numpy(np.int32), pos=pos.numpy(np.int32), tok=tok.numpy(np.int32),
               raw=lraw.numpy(np.float32), drawn=ldrawn.numpy(np.float32), ids=tids.numpy(np.int32, (rows, nn)), lps=tlps.numpy(np.float32, (rows, nn)),
               tws=tws.numpy(np.uint32), hooks=hooks)
    if seen is not None:
        out["seen"] = seen.numpy(np.uint32)
    if dim:
        out.update(x=xo.numpy(np.uint16), ssq=ssq.numpy(np.uint32))
    if sampler == "lp":
        out.update(wv=wv.numpy(np.uint32), lws=lws.numpy(np.uint32))
    else:
        out["ws"] = ws.numpy(np.uint32)
    return out


def _same_state(a, b):
    return [k for k in STATE if k in a and not np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8))]


def _check_rows(x, n, out, written, raw_rows=None, what=""):
    """rows `written` (in call order, None = the call wrote no row) hold the model's ids and bits; every other row the poison; a drawn token
    that is listed carries lp_raw's bits.  Returns the number of draws found in their list."""
    assert torch.cuda.is_available()
    ids, lps = out["ids"], out["lps"].view(np.uint32)
    touched = np.zeros(ids.shape[0], dtype=bool)
    hits = 0
    raw_rows = written if raw_rows is None else raw_rows
    for step, (r, rr) in enumerate(zip(written, raw_rows)):
        if r is None:
            continue
        touched[r] = True
        M, L = out["hooks"][step]
        want_ids, want_lps = tm.top_n(x, n, M, L)
        assert ids[r].tolist() == want_ids.tolist(), (what, "ids of row", r, ids[r].tolist(), want_ids.tolist())
        nan = np.isnan(want_lps)  # (a NaN logit in the sum: L is NaN and so is every entry; which NaN is not pinned)
        assert np.array_equal(np.isnan(out["lps"][r]), nan) and np.array_equal(lps[r][~nan], want_lps.view(np.uint32)[~nan]), (what, "bits of row", r, out["lps"][r], want_lps)
        tokn = int(out["nt"][step])
        where = np.nonzero(ids[r] == tokn)[0]
        if where.size and rr is not None:
            hits += 1
            assert lps[r][where[0]] == out["raw"].view(np.uint32)[rr], (what, "the drawn token's entry is not lp_raw", r, out["lps"][r][where[0]], out["raw"][rr])
    assert (ids[~touched] == np.int32(0x7E7E7E7E)).all() and (lps[~touched] == POISON32).all(), (what, "a row outside the run was written")
    return hits


def _check_pair(x, out, what=""):
    """M + L of every call against the float64 log-sum-exp, within lp_raw's grant"""
    if not lp.specified(x):
        return
    want, g = lp.lse64(np.asarray(x, dtype=np.float16).astype(np.float32)), tm.grant(x)
    for M, L in out["hooks"]:
        assert abs(float(M) + float(L) - want) <= g, (what, float(M), float(L), want, g)


@functools.lru_cache(maxsize=None)
def _logits(V):
    """steps of 1/4 (ties at every place of a list) with a few -inf; short vocabularies: gaussians"""
    x = sm.profile("quant" if V >= 1000 else "gauss", V).copy()
    if V >= 1000:
        x[np.random.default_rng(V).permutation(V)[:7]] = -np.inf
    return x


@pytest.mark.parametrize("n", [1, 5, 20])
@pytest.mark.parametrize("V", [1, 5, 1000, 131072, 131073, 151936, 262144])
def test_sizes(V, n):
    x = _logits(V)
    out = _run(x, n, pos0=3, cap=8)
    hits = _check_rows(x, n, out, [4], what=(V, n))
    _check_pair(x, out, (V, n))
    if V <= n:  # the short vocabulary: filled
        assert out["ids"][4][V:].tolist() == [-1] * (n - V) and (out["lps"][4][V:] == -np.inf).all()
        assert hits == 1
    if V >= 1000:
        full = _run(x, n, sampler="full", pos0=3, cap=8, top_k=0, min_p=0.02)
        _check_rows(x, n, full, [4], what=(V, n, "full"))
        _check_pair(x, full, (V, n, "full"))
        assert np.array_equal(full["ids"][4], out["ids"][4])


def _placements(V):
    per = (V + BLOCKS - 1) // BLOCKS
    base = (sm.profile("gauss", V).astype(np.float32) * 0.5).astype(np.float16)
    vals = (20.0 + np.random.default_rng(V).permutation(20) / 8.0).astype(np.float16)
    out = {}

    def put(name, where, v):
        x = base.copy()
        x[np.asarray(where)] = v
        out[name] = x
    put("one_block", 5 * per + 3 + 7 * np.arange(20), vals)
    put("one_wave", 5 * per + 70 + np.arange(20), vals)
    put("one_per_block", np.arange(20) * 6 * per + (np.arange(20) * 37) % per, vals)
    put("equal_across_a_boundary", np.arange(40 * per - 3, 40 * per + 4), np.float16(21.0))
    put("equal_over_many_blocks", np.arange(25) * 5 * per + per - 1, np.float16(21.0))
    put("equal_in_the_last_slice", [V - 1, V - 2, V - 9, 127 * per, 11, 127 * per + 40], np.float16(21.0))
    put("winner_at_0", [0], np.float16(30.0))
    put("winner_at_the_end", [V - 1], np.float16(30.0))
    z = np.full(V, -3.0, dtype=np.float16)  # -0 +0 | -0 +0 around the boundary of slices 8 and 9, everything else below them
    z[9 * per - 2:9 * per + 2] = np.array([0x8000, 0x0000, 0x8000, 0x0000], dtype=np.uint16).view(np.float16)
    out["zeros_across_a_boundary"] = z
    out["all_equal"] = np.full(V, 1.5, dtype=np.float16)
    return out


@pytest.mark.parametrize("V", [NARROW, WIDE])
def test_placements_that_break_a_merge(V):
    assert V % BLOCKS and (V + BLOCKS - 1) // BLOCKS * (BLOCKS - 1) < V  # (a ragged, non-empty last slice)
    for name, x in _placements(V).items():
        for n in (5, 20):
            out = _run(x, n, pos0=0, cap=2, top_k=1, T=0.0)
            _check_rows(x, n, out, [1], what=(V, name, n))
            _check_pair(x, out, (V, name, n))
            got = out["ids"][1].tolist()
            if name == "winner_at_0":
                assert got[0] == 0
            if name == "winner_at_the_end":
                assert got[0] == V - 1
            if name == "zeros_across_a_boundary":
                per = (V + BLOCKS - 1) // BLOCKS
                assert got[:5] == [9 * per - 1, 9 * per + 1, 9 * per - 2, 9 * per, 0]
            if name.startswith("equal") or name == "all_equal":
                k = min(n, 7 if name == "equal_across_a_boundary" else 6 if name == "equal_in_the_last_slice" else n)
                assert got[:k] == sorted(got[:k]), (name, got)
            # greedy: the drawn token heads the list and carries lp_raw
            assert got[0] == int(out["nt"][0]) and out["lps"].view(np.uint32)[1][0] == out["raw"].view(np.uint32)[1]


@pytest.mark.parametrize("sampler", ["lp", "full"])
def test_the_list_is_that_of_the_bare_logits(sampler):
    V = NARROW
    x = sm.profile("gauss", V).copy()
    order = tm.raw_order(x)
    first, second, third = (int(t) for t in order[:3])
    # the largest logit is suppressed, the second banned, the third in the history under a penalty of 1.3; top_k = 1 and a temperature
    kw = dict(sampler=sampler, steps=3, pos0=2, top_k=1, T=0.7, ban=(1, 100, [second, 0, 0, 0]), suppress=(first, ), seen0=(third, 17), rp=1.3)
    out = _run(x, 20, **kw)
    hits = _check_rows(x, 20, out, [3, 4, 5], what=sampler)
    assert out["ids"][3].tolist() == order[:20].tolist() and out["ids"][3][0] == first
    assert first not in out["nt"][:3].tolist() and second not in out["nt"][:3].tolist()
    assert hits == 3  # (the tokens drawn from the processed top-1 are the 4th, 5th, .. of the raw order)
    assert _same_state(_run(x, 20, topn=False, **kw), out) == []


def _peaked(V):
    x = sm.profile("gauss", V).copy()
    x[np.random.default_rng(7).permutation(V)[:12]] = (14.0 + np.arange(12) / 4.0).astype(np.float16)
    return x


@pytest.mark.parametrize("V", [NARROW, WIDE])
@pytest.mark.parametrize("sampler,kw", [("lp", dict(top_k=50)), ("full", dict(top_k=0, min_p=0.01))], ids=["top_k_50", "whole_vocabulary_min_p"])
def test_the_draw_is_unchanged_and_a_listed_draw_carries_lp_raw(sampler, kw, V):
    x = _peaked(V)
    kw = dict(kw, sampler=sampler, steps=12, pos0=4, T=1.0, top_p=0.95, seen0=(1, 2, 3), rp=1.1, dim=64)
    old = _run(x, 20, topn=False, **kw)
    new = _run(x, 20, **kw)
    again = _run(x, 20, **kw)
    assert _same_state(old, new) == []
    rows = list(range(5, 17))
    hits = _check_rows(x, 20, new, rows, what=(sampler, V))
    _check_pair(x, new, (sampler, V))
    assert hits >= 6, hits  # (the twelve planted logits, all listed, carry nearly all of the mass)
    assert np.array_equal(new["ids"], again["ids"]) and np.array_equal(new["lps"].view(np.uint32), again["lps"].view(np.uint32)), "two runs from the same state differ"
    assert (old["ids"] == np.int32(0x7E7E7E7E)).all() and (old["tws"] == POISON32).all()


@pytest.mark.parametrize("sampler", ["lp", "full"])
def test_an_empty_candidate_set_still_lists_the_raw_order(sampler):
    V = 300
    x = sm.profile("gauss", V)
    kw = dict(sampler=sampler, steps=2, pos0=1, suppress=tuple(range(V)), seen0=(3, ), rp=1.3, top_k=50 if sampler == "lp" else 0)
    old, new = _run(x, 5, topn=False, **kw), _run(x, 5, **kw)
    assert _same_state(old, new) == [] and new["nt"][:2].tolist() == [INT_MAX] * 2 and np.isnan(new["raw"][2:4]).all()
    _check_rows(x, 5, new, [2, 3], what=sampler)
    assert new["ids"][2].tolist() == tm.raw_order(x)[:5].tolist()


@pytest.mark.parametrize("sampler", ["lp", "full"])
def test_nan_logits_are_not_listed(sampler):
    x = sm.profile("nan_few", 4096)
    out = _run(x, 20, sampler=sampler, top_k=50 if sampler == "lp" else 0)
    _check_rows(x, 20, out, [1], what=sampler)
    assert not np.isnan(x[out["ids"][1]].astype(np.float32)).any()
    allnan = sm.profile("nan_all", 300)
    out = _run(allnan, 5, sampler=sampler, top_k=50 if sampler == "lp" else 0)
    assert out["ids"][1].tolist() == [-1] * 5 and (out["lps"][1] == -np.inf).all()


@pytest.mark.parametrize("sampler", ["lp", "full"])
def test_the_row_index(sampler):
    x = _logits(1000)
    k = dict(sampler=sampler, top_k=50 if sampler == "lp" else 0)
    cap = 6
    # *pos_io = cap - 2 writes row cap - 1, *pos_io = cap - 1 writes nothing; the second step of a run that starts at cap - 2 is past the cap
    out = _run(x, 5, pos0=cap - 2, cap=cap, **k)
    _check_rows(x, 5, out, [cap - 1], what="cap - 2")
    out = _run(x, 5, pos0=cap - 1, cap=cap, **k)
    _check_rows(x, 5, out, [None], what="cap - 1")
    out = _run(x, 5, pos0=cap - 2, cap=cap, steps=2, **k)
    _check_rows(x, 5, out, [cap - 1, None], what="two steps")
    assert [tm.row(p, cap) for p in (cap - 2, cap - 1, None)] == [cap - 1, None, 0]
    # pos_io NULL: row 0 (lp_raw keeps its index 1)
    out = _run(x, 5, pos0=None, cap=cap, **k)
    _check_rows(x, 5, out, [0], raw_rows=[1], what="pos_io NULL")
    assert out["raw"].view(np.uint32)[1] != POISON32 and out["raw"].view(np.uint32)[0] == POISON32


@pytest.mark.parametrize("sampler", ["lp", "full"])
def test_refusals_write_nothing(sampler):
    from guidedquant_amd import _lib
    x = _logits(1000)
    k = dict(sampler=sampler, top_k=50 if sampler == "lp" else 0)
    cases = [(dict(V=262145), _lib.GQ_ENOTSUP), (dict(n=0), _lib.GQ_EINVAL), (dict(n=21), _lib.GQ_EINVAL), (dict(n=-1), _lib.GQ_EINVAL),
             (dict(null=("top_ids", )), _lib.GQ_EINVAL), (dict(null=("top_lps", )), _lib.GQ_EINVAL), (dict(null=("topn_ws", )), _lib.GQ_EINVAL),
             (dict(null=("lp_raw", )), _lib.GQ_EINVAL)]
    if sampler == "lp":
        cases += [(dict(null=("lp_ws", )), _lib.GQ_EINVAL), (dict(top_k=65), _lib.GQ_ENOTSUP)]
    else:
        cases += [(dict(top_k=-1), _lib.GQ_EINVAL)]
    for kw, rc in cases:
        kw = dict(k, **kw)
        out = _run(x, kw.pop("n", 5), pos0=2, counter=9, expect=rc, **kw)
        assert out["ctr"][0] == 9 and out["pos"][0] == 2 and out["tok"][0] == -5, kw
        for name in ("nt", "seq", "raw", "drawn", "ids", "lps", "tws", "wv", "lws", "ws"):
            if name in out:
                assert (out[name].view(np.uint8) == guarded.POISON).all(), (kw, name)
