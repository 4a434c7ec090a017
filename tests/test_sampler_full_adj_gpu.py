"""GPU: gq_sample_full_adj through the C ABI -- the differential of tests/test_sampler_adj_gpu.py against gq_sample_full / gq_sample_full_topn
(tests/sampler_adj_device.py has the run, tests/sampler_adj_model.py the adjustment and the cases).

Per case of sampler_adj_model.FULL_CASES, in lockstep over its draws: A = gq_sample_full_adj on the raw logits, B = gq_sample_full on
adjusted_logits(raw, bias, counts so far) from the same state.  After every draw everything a draw writes, lp_drawn included, and the
workspace report {n, n_k, Z_k, Z_kept} are equal bit for bit; out_set / out_count equal the host's tally; lp_raw and the top-n rows of A
are the raw logits' (one gq_sample_full_topn call); two runs of A leave identical bits.  top_k 0 and 200 (and 2: a cut inside a tie the
bias made), top_p 0.9, min_p 0.05; vocabularies 33, 4096, 151936, 262144."""
import numpy as np
import pytest

import guarded
import sampler_adj_device as dev
import sampler_adj_model as am

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [c.name for c in am.FULL_CASES])
def test_case(name):
    assert torch.cuda.is_available()
    c = am.CASE_BY_NAME[name]
    tokens = dev.check_case(c, full=True)
    if name == "full_equal_by_count":
        # (no top-k filter: at T = 1e-5 the race is among the tokens of the lowest count, 0.5 / 1e-5 above the rest -- every round of V
        # draws is a permutation of the vocabulary)
        assert sorted(tokens[:c.V]) == sorted(tokens[c.V:2 * c.V]) == list(range(c.V)) and tokens[:c.V] != list(range(c.V))
    if name == "full_bias_to_minus_inf":
        assert 7 not in tokens
    if name == "full_all_suppressed":
        assert tokens == [dev.EMPTY_TOKEN] * c.n
    if name == "full_no_filter":
        assert len(set(tokens)) > 4


def test_neutral_forms_draw_what_the_entry_without_the_suffix_draws():
    from guidedquant_amd import _lib
    c = am.CASE_BY_NAME["full_mix_rp_suppress_ban"]
    old = dev.Run(c, True, False, 4)
    for i in range(c.n):
        old.draw(i, entry="gq_sample_full_topn")
    want = old.state()
    for adj in (None, _lib.GqSampleAdjust(0.0, 0.0, None, None, None, None)):
        new = dev.Run(c, True, False, 4)
        for i in range(c.n):
            new.draw(i, entry="gq_sample_full_adj", adj=adj)
        new.go.check()
        got = new.state()
        for k in want:
            assert np.array_equal(want[k], got[k]), (k, adj is None)
    plain, new = dev.Run(c, True, False), dev.Run(c, True, False)
    for i in range(c.n):
        plain.draw(i)
        new.draw(i, entry="gq_sample_full_adj", adj=None)  # (top_n == 0: no list pointer)
    a, b = plain.state(), new.state()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_refusals_write_nothing():
    from guidedquant_amd import _lib
    c = am.CASE_BY_NAME["full_mix_rp_suppress_ban"]._replace(n=1)
    inf, nan = float("inf"), float("nan")

    def refused(rc, top_n=4, **over):
        r = dev.Run(c, True, True, 4)
        before = r.state()
        a = r.adj
        fields = dict(frequency_penalty=a.frequency_penalty, presence_penalty=a.presence_penalty, bias_set=a.bias_set, bias=a.bias, out_set=a.out_set,
                      out_count=a.out_count)
        draw_over = {k: over.pop(k) for k in list(over) if k in ("top_k", "V", "lraw")}
        fields.update(over)
        r.draw(0, expect=rc, top_n=top_n, adj=_lib.GqSampleAdjust(*fields.values()), **draw_over)
        r.go.check()
        r.gi.check()
        after = r.state()
        for k in before:
            assert np.array_equal(before[k], after[k]), (over, draw_over, k)
        assert (r.ws.numpy(np.uint8) == guarded.POISON).all() and (r.topn_ws.numpy(np.uint8) == guarded.POISON).all()

    for over in (dict(frequency_penalty=inf), dict(presence_penalty=nan), dict(bias_set=None), dict(bias=None), dict(out_set=None), dict(out_count=None),
                 dict(out_set=None, out_count=None)):
        refused(_lib.GQ_EINVAL, **over)
    refused(_lib.GQ_EINVAL, top_n=21)
    refused(_lib.GQ_EINVAL, lraw=None)
    refused(_lib.GQ_EINVAL, top_n=0, top_k=-1)
    refused(_lib.GQ_ENOTSUP, V=262145)
