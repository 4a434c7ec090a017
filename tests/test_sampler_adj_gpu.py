"""GPU: gq_sample_topk_adj and gq_token_bias_build through the C ABI -- a differential against the existing entries on logits the host
adjusted (tests/sampler_adj_model.py: the adjustment is defined to give an fp16 logit, so the two draws are equal bit for bit).

Per case of sampler_adj_model.TOPK_CASES (tests/sampler_adj_device.py has the run), in lockstep over the case's 64 to 300 draws:
  A  gq_sample_topk_adj on the raw logits;
  B  for each draw, gq_sample_topk_lp on adjusted_logits(raw, bias, counts so far) from the same state.
After every draw next_tok, tok_io, pos_io, counter, seq_out, seen, x_out, ssq_out and lp_drawn are equal byte for byte, out_set / out_count
equal the host's tally with every other word as it was (an empty candidate set leaves them alone), and the guards of A's buffers hold.
lp_raw of A is fl32(fl32(v_raw[tok] - M) - L) with (M, L) read from topn_ws of ONE gq_sample_topk_lp_topn call on the raw logits, the
top-n rows of A are that call's row, and a second run of A leaves identical bits everywhere.  Outputs, workspaces and the four new arrays
start poisoned."""
import numpy as np
import pytest

import guarded
import sampler_adj_device as dev
import sampler_adj_model as am

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

POISON32 = dev.POISON32
_TOKENS = {}


@pytest.mark.parametrize("name", [c.name for c in am.TOPK_CASES])
def test_case(name):
    assert torch.cuda.is_available()
    c = am.CASE_BY_NAME[name]
    _TOKENS[name] = tokens = dev.check_case(c, full=False)
    if name == "equal_greedy_walk":  # 0, 1, 2, ... and then back to the lowest id of the lowest count
        assert tokens == [i % c.V for i in range(c.n)]
    if name == "equal_greedy_walk_wide":
        assert tokens == list(range(c.n))
    if name == "bias_to_minus_inf":
        assert 7 not in tokens
    if name == "bias_ties_greedy":  # 1.0 + 0.5 ties the unlisted 1.5 at id 20: the lower id wins every greedy draw
        assert tokens == [10] * c.n
    if name == "all_suppressed":
        assert tokens == [dev.EMPTY_TOKEN] * c.n
    if name.startswith("penalties_k") and c.top_k > 1:
        assert len(set(tokens)) > 4


def test_the_penalties_change_the_draw():
    """the differential has something to show: without the adjustment the same seeds draw other tokens"""
    c = am.CASE_BY_NAME["penalties_k2"]
    with_adj = _TOKENS.get(c.name) or dev.check_case(c, full=False)
    plain = dev.Run(c, False, False)
    for i in range(c.n):
        plain.draw(i)
    torch.cuda.synchronize()
    assert plain.nt.numpy(np.int32)[:c.n].tolist() != with_adj


def test_neutral_forms_draw_what_the_entry_without_the_suffix_draws():
    from guidedquant_amd import _lib
    c = am.CASE_BY_NAME["mix_rp_suppress_ban"]
    old = dev.Run(c, False, False, 4)
    for i in range(c.n):
        old.draw(i, entry="gq_sample_topk_lp_topn")
    want = old.state()
    for adj in (None, _lib.GqSampleAdjust(0.0, 0.0, None, None, None, None)):
        new = dev.Run(c, False, False, 4)
        for i in range(c.n):
            new.draw(i, entry="gq_sample_topk_adj", adj=adj)
        new.go.check()
        got = new.state()
        for k in want:
            assert np.array_equal(want[k], got[k]), (k, adj is None)
    # top_n == 0: no list pointer is needed and topn.hip's pair is not launched (its workspace keeps the poison)
    lp = dev.Run(c, False, False)
    new = dev.Run(c, False, False)
    for i in range(c.n):
        lp.draw(i)
        new.draw(i, entry="gq_sample_topk_adj", adj=None)
    a, b = lp.state(), new.state()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_the_bias_table_builder():
    from guidedquant_amd import _lib
    L, s = _lib.lib(), _lib.current_stream_ptr()
    V = 300
    g = guarded.Guards()
    ids = np.array([0, 31, 32, 299, 300, -1, 100000, 64], dtype=np.int32)  # (300, -1 and 100000 are outside [0, V): ignored)
    vals = np.arange(1, 9, dtype=np.float32) / 4
    gi, gv = g.inp("ids", ids), g.inp("values", vals)
    bs, bv = g.out("bias_set", 4 * ((V + 31) // 32)), g.out("bias", 4 * V)
    assert L.gq_token_bias_build(gi.ptr(), gv.ptr(), ids.size, V, bs.ptr(), bv.ptr(), s) == 0
    g.check()
    want = np.full(V, POISON32, dtype=np.uint32)
    for t, v in zip(ids, vals):
        if 0 <= t < V:
            want[t] = np.float32(v).view(np.uint32)
    assert np.array_equal(bv.numpy(np.uint32), want), "a word of bias outside the listed ids was written"
    assert np.array_equal(bs.numpy(np.uint32), dev.token_set([0, 31, 32, 299, 64], V))
    # n == 0 just clears the set; a NULL pointer or vocab == 0 is refused and writes nothing
    assert L.gq_token_bias_build(None, None, 0, V, bs.ptr(), bv.ptr(), s) == 0
    g.check()
    assert not bs.numpy(np.uint32).any() and np.array_equal(bv.numpy(np.uint32), want)
    for a in ((gi.ptr(), gv.ptr(), 2, V, None, bv.ptr()), (gi.ptr(), gv.ptr(), 2, V, bs.ptr(), None), (None, gv.ptr(), 2, V, bs.ptr(), bv.ptr()),
              (gi.ptr(), None, 2, V, bs.ptr(), bv.ptr()), (gi.ptr(), gv.ptr(), 2, 0, bs.ptr(), bv.ptr())):
        assert L.gq_token_bias_build(*a, s) == _lib.GQ_EINVAL
    g.check()
    assert not bs.numpy(np.uint32).any() and np.array_equal(bv.numpy(np.uint32), want)


def test_refusals_write_nothing():
    from guidedquant_amd import _lib
    c = am.CASE_BY_NAME["mix_rp_suppress_ban"]._replace(n=1)
    inf, nan = float("inf"), float("nan")

    def refused(rc, top_n=4, **over):
        r = dev.Run(c, False, True, 4)
        before = r.state()
        a = r.adj
        fields = dict(frequency_penalty=a.frequency_penalty, presence_penalty=a.presence_penalty, bias_set=a.bias_set, bias=a.bias, out_set=a.out_set,
                      out_count=a.out_count)
        draw_over = {k: over.pop(k) for k in list(over) if k in ("top_k", "V", "lws", "lraw")}
        fields.update(over)
        r.draw(0, expect=rc, top_n=top_n, adj=_lib.GqSampleAdjust(*fields.values()), **draw_over)
        r.go.check()
        r.gi.check()
        after = r.state()
        for k in before:
            assert np.array_equal(before[k], after[k]), (over, draw_over, k)
        assert (r.wv.numpy(np.uint8) == guarded.POISON).all() and (r.lws.numpy(np.uint8) == guarded.POISON).all() and (r.topn_ws.numpy(np.uint8) == guarded.POISON).all()

    for over in (dict(frequency_penalty=inf), dict(frequency_penalty=nan), dict(presence_penalty=-inf), dict(presence_penalty=nan),  # a penalty that is not finite
                 dict(bias_set=None), dict(bias=None), dict(out_set=None), dict(out_count=None),                                       # a half-given pair
                 dict(out_set=None, out_count=None)):                                                                                   # a penalty without out_set
        refused(_lib.GQ_EINVAL, **over)
    # then the refusals of the entry without the suffix, with its codes
    refused(_lib.GQ_EINVAL, top_n=21)
    refused(_lib.GQ_EINVAL, top_n=-1)
    refused(_lib.GQ_EINVAL, lraw=None)            # a list without lp_raw
    refused(_lib.GQ_EINVAL, top_n=0, lws=None)    # lp_raw without its workspace
    refused(_lib.GQ_ENOTSUP, top_k=65)
    refused(_lib.GQ_ENOTSUP, V=262145)
