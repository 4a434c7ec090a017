"""GPU: the wide instance of the fused sampler (csrc/sampler.hip: 131072 < vocab <= 262144 -- the published Qwen3 vocabulary is 151936)
through the C ABI: gq_sample_topk_p with the 128 x 64 work buffers every caller allocates, gq_sample_topk with 128 x 32 for one case.

The reference is computed with torch on the host.  The candidates are the first k of the order (fp16 value descending, index
ascending) -- a stable sort, since fp16 ties are common among 150,000 logits -- and the greedy token is the first of that order.
Logits come from a CPU generator, so the planted cases and the tie checks below hold on every machine.  On a library without the
wide instance every launch here answers GQ_ENOTSUP."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

VOCABS = [131073, 151936, 200001, 262144]  # the first wide one, Qwen3's, a ragged last slice (no multiple of 128), the limit
BLOCKS = 128                                 # the sampler's grid: a block's slice is ceil(V / 128) logits


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _random_logits(V, seed=3):
    """randn * 2 in fp16 on the host (shared between the tests: clone before planting anything)"""
    g = torch.Generator()
    g.manual_seed(seed + V)
    return (torch.randn(V, generator=g) * 2).half()


def _order(x):
    """token ids by (fp16 value descending, index ascending)"""
    return torch.sort(x.float(), descending=True, stable=True).indices


class _Sampler:
    """the device words of one sampler state; `run` draws n tokens without a host round trip and returns them from the sequence store"""

    def __init__(self, km=64, cap=8192, counter=0):
        d = _dev()
        z = lambda n, dt: torch.zeros(n, dtype=dt, device=d)  # noqa: E731
        self.km = km
        self.wv, self.wi = z(BLOCKS * km, torch.float32), z(BLOCKS * km, torch.int32)
        self.ctr, self.tok, self.pos, self.nt = (z(1, torch.int32) for _ in range(4))
        self.ctr.fill_(counter)
        self.seq = torch.full((cap, ), -1, dtype=torch.int32, device=d)

    def launch(self, logits, k, T, top_p=1.0, seed=77, ban=None, table=None, x=None, ssq=None):
        from guidedquant_amd import _lib
        L = _lib.lib()
        V = logits.numel()
        if self.km == 32:
            return L.gq_sample_topk(logits.data_ptr(), V, k, T, seed, self.ctr.data_ptr(), self.wv.data_ptr(), self.wi.data_ptr(), self.tok.data_ptr(),
                                    self.pos.data_ptr(), self.nt.data_ptr(), _lib.current_stream_ptr())
        return L.gq_sample_topk_p(logits.data_ptr(), V, k, top_p, T, seed, self.ctr.data_ptr(), self.wv.data_ptr(), self.wi.data_ptr(), self.tok.data_ptr(),
                                  self.pos.data_ptr(), self.nt.data_ptr(), ban.data_ptr() if ban is not None else None, self.seq.data_ptr(), self.seq.numel(),
                                  table.data_ptr() if table is not None else None, x.data_ptr() if x is not None else None,
                                  x.numel() if x is not None else 0, ssq.data_ptr() if ssq is not None else None, _lib.current_stream_ptr())

    def run(self, logits, n, k, T, **kw):
        from guidedquant_amd import _lib
        p0 = int(self.pos.item())
        out = []
        for _ in range(n):
            _lib.check(self.launch(logits, k, T, **kw), "fused sampler")
            if self.km == 32:  # (gq_sample_topk has no sequence store)
                out.append(int(self.nt.item()))
        torch.cuda.synchronize()
        return out if self.km == 32 else self.seq[p0 + 1:p0 + 1 + n].tolist()

    def greedy(self, logits, k=1):
        return self.run(logits, 1, k, 0.0)[0]


@pytest.mark.parametrize("V", VOCABS)
def test_greedy_and_candidate_set_on_random_logits(V):
    x = _random_logits(V)
    ref = _order(x)
    assert float(x[ref[0]]) > float(x[ref[1]])  # (T = 0 is a race at T = 1e-5: a tied maximum would be drawn from both)
    lg = x.to(_dev())
    s = _Sampler()
    assert s.greedy(lg, 50) == int(ref[0])
    assert int(s.tok.item()) == int(s.nt.item()) == int(ref[0]) and int(s.pos.item()) == 1 and int(s.ctr.item()) == 1
    draws = s.run(lg, 300, 50, 1.0)
    assert set(draws) <= set(ref[:50].tolist()) and len(set(draws)) > 5
    # token / position feedback, the counter and the sequence store advance as at narrow widths
    assert int(s.pos.item()) == 301 and int(s.ctr.item()) == 301
    assert int(s.tok.item()) == int(s.nt.item()) == draws[-1] and int(s.seq[301]) == draws[-1] and int(s.seq[302]) == -1


@pytest.mark.parametrize("V", VOCABS)
def test_planted_winner_is_found_at_every_kind_of_position(V):
    per = (V + BLOCKS - 1) // BLOCKS
    assert 1024 < per <= 2048
    # first / last token, either side of 2^17, and two positions whose index inside the block's slice needs the 11th bit
    places = sorted({0, 131071, 131072, V - 1, 77 * per + 1024, 78 * per - 1})
    assert all(0 <= i < V for i in places) and (77 * per + 1024) // per == 77
    x0 = _random_logits(V)
    s = _Sampler()
    for i in places:
        x = x0.clone()
        x[i] = 30.0
        assert int(_order(x)[0]) == i
        for k in (1, 64):
            assert s.greedy(x.to(_dev()), k) == i, (V, i, k)


@pytest.mark.parametrize("V", VOCABS)
def test_top_64_inside_one_slice_across_local_position_1024(V):
    per = (V + BLOCKS - 1) // BLOCKS
    hi = min(per, 1056)  # 64 neighbouring positions of block 5's slice: below and above local position 1024
    where = torch.arange(5 * per + hi - 64, 5 * per + hi)
    assert int(where[0]) - 5 * per < 1024 <= int(where[-1]) - 5 * per
    g = torch.Generator()
    g.manual_seed(V)
    vals = (20.0 + torch.randperm(64, generator=g).float() / 16).half()  # 64 distinct fp16 values (spacing 1/64 below 32)
    x = _random_logits(V).clone()
    x[where] = vals
    ref = _order(x)
    assert set(ref[:64].tolist()) == set(where.tolist()) and float(x[ref[0]]) == 20.0 + 63 / 16
    lg = x.to(_dev())
    s = _Sampler()
    assert s.greedy(lg, 64) == int(ref[0])
    draws = s.run(lg, 2000, 64, 1.0)
    assert set(draws) <= set(where.tolist()) and int(ref[0]) in draws and len(set(draws)) > 32


@pytest.mark.parametrize("V", VOCABS)
def test_equal_maxima_go_to_the_lower_index(V):
    per = (V + BLOCKS - 1) // BLOCKS
    s = _Sampler()
    # the last logit of one slice and the first of the next; either side of 2^17; two blocks far apart, upper one first in no order
    for a, b in ((40 * per - 1, 40 * per), (131071, 131072), (3 * per + 1030, 100 * per + 7)):
        assert a < b < V
        x = _random_logits(V).clone()
        x[a] = x[b] = 30.0
        ref = _order(x)
        assert ref[:2].tolist() == [a, b] and float(x[ref[2]]) < 30.0  # (the reference order is unambiguous)
        lg = x.to(_dev())
        # (greedy = top_k 1, as generate() asks for it: with more candidates T = 0 is a race at T = 1e-5, which equal values share)
        assert s.greedy(lg, 1) == a, (V, a, b)
        # with k = 2 at T = 1 both are drawn and nothing else is
        assert set(s.run(lg, 64, 2, 1.0)) == {a, b}


def test_ban_list_holds_ids_beyond_131072():
    """Qwen3's EOS ids (151643 / 151645) at the published vocabulary: the arg-max is banned while *pos_io < until"""
    V, eos, eos2 = 151936, 151645, 151643
    x = _random_logits(V).clone()
    x[eos], x[eos2] = 30.0, 29.0
    ref = _order(x)
    assert ref[:2].tolist() == [eos, eos2] and float(x[ref[2]]) < 29.0
    third = int(ref[2])
    lg = x.to(_dev())
    ban = torch.tensor([1, 3, eos, 0, 0, 0], dtype=torch.int32, device=_dev())
    s = _Sampler()
    assert s.run(lg, 5, 1, 0.0, ban=ban) == [eos2, eos2, eos2, eos, eos]  # positions 0..2 are below `until` = 3
    ban.copy_(torch.tensor([2, 8, eos2, eos, 0, 0], dtype=torch.int32))
    assert s.run(lg, 4, 50, 0.0, ban=ban) == [third, third, third, eos]    # positions 5..7, then 8
    # sampled draws under the ban never give a banned id
    s2 = _Sampler()
    ban.copy_(torch.tensor([2, 1 << 30, eos, eos2, 0, 0], dtype=torch.int32))
    draws = s2.run(lg, 200, 50, 1.0, ban=ban)
    assert set(draws) <= set(ref[2:52].tolist())


def test_embedding_of_a_drawn_token_beyond_131072_is_folded_in():
    from guidedquant_amd import _lib
    V, D, t = 151936, 64, 140001
    d = _dev()
    x = _random_logits(V).clone()
    x[t] = 30.0
    g = torch.Generator()
    g.manual_seed(11)
    table = torch.randn(V, D, generator=g).half().to(d)
    xo = torch.zeros(D, dtype=torch.float16, device=d)
    ssq = torch.zeros(_lib.SSQ_SLOTS, dtype=torch.float32, device=d)
    s = _Sampler()
    assert s.run(x.to(d), 1, 50, 0.0, table=table, x=xo, ssq=ssq) == [t]
    assert torch.equal(xo, table[t])
    # (the bound of the hand-over check in test_hf_routes_gpu.py::test_sampler_with_64_candidates_ban_and_sequence_store)
    assert abs(float(ssq.double().sum()) - float((table[t].double()**2).sum())) < 1e-3


def test_nucleus_filter_at_the_published_qwen3_vocabulary_matches_transformers_warper_chain():
    """k = 50, top_p = 0.9 at 151936 logits against TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper (on the host), in the
    manner of test_hf_routes_gpu.py::test_nucleus_filter_of_the_fused_sampler_matches_transformers_warper_chain"""
    pytest.importorskip("transformers")
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    V, k, p, T = 151936, 50, 0.9, 1.0
    x = _random_logits(V)
    srt = torch.sort(x.float(), descending=True, stable=True).values
    assert float(srt[k - 1]) > float(srt[k])  # (no tie across the top-k boundary: the warper's `<` would keep more than k)
    sc = x.float().view(1, -1)
    for wp in (TemperatureLogitsWarper(T), TopKLogitsWarper(k), TopPLogitsWarper(p)):
        sc = wp(torch.zeros(1, 1, dtype=torch.long), sc)
    want = torch.softmax(sc, dim=-1).view(-1).numpy()
    support = set(np.nonzero(want > 0)[0].tolist())
    assert 1 < len(support) < k
    s = _Sampler()
    draws = np.asarray(s.run(x.to(_dev()), 6000, k, T, top_p=p, seed=99))
    cnt = np.bincount(draws, minlength=V).astype(np.float64) / len(draws)
    assert set(np.nonzero(cnt)[0].tolist()) <= support, sorted(set(np.nonzero(cnt)[0].tolist()) - support)
    assert np.abs(cnt - want).max() < 0.03, np.abs(cnt - want).max()


def test_the_narrow_and_the_wide_instance_draw_the_same_tokens():
    """131072 logits through the narrow pair; the same with one lowest-possible logit appended (131073) through the wide pair: the
    slices differ (1024 / 1025 logits per block), the top 50 do not, and the random number is tied to the token id -- so with one
    seed and one starting counter the two sequences are equal"""
    x = _random_logits(131072)
    y = torch.cat([x, torch.tensor([float("-inf")], dtype=torch.float16)])
    assert y.numel() == 131073
    seqs = []
    for lg in (x, y):
        s = _Sampler(counter=1234)
        seqs.append(s.run(lg.to(_dev()), 200, 50, 1.0, seed=5))
    assert seqs[0] == seqs[1] and len(set(seqs[0])) > 5


def test_distribution_at_the_published_qwen3_vocabulary():
    """gq_sample_topk (work buffers of 128 * 32): 3000 draws at T = 1 follow softmax(top-32) within the bound of
    test_decode_gpu.py::test_fused_sampler_matches_reference_distribution"""
    V = 151936
    x = _random_logits(V)
    ref = _order(x)[:32]
    s = _Sampler(km=32)
    draws = s.run(x.to(_dev()), 3000, 32, 1.0)
    assert set(draws) <= set(ref.tolist())
    p = torch.softmax(x[ref].float(), dim=0).numpy()
    cnt = np.array([draws.count(int(i)) for i in ref.tolist()], dtype=np.float64) / len(draws)
    assert np.abs(cnt - p).max() < 0.04, (cnt, p)
    assert int(s.pos.item()) == 3000 and int(s.ctr.item()) == 3000


def test_vocabularies_beyond_262144_and_more_than_64_candidates_are_refused():
    from guidedquant_amd import _lib
    x = torch.zeros(262145, dtype=torch.float16, device=_dev())
    s = _Sampler()
    assert s.launch(x, 50, 1.0) == _lib.GQ_ENOTSUP
    assert b"262144" in _lib.lib().gq_last_error()
    assert s.launch(x[:262144], 65, 1.0) == _lib.GQ_ENOTSUP
    assert s.launch(x[:262144], 50, 1.0) == 0
    assert _Sampler(km=32).launch(x[:151936], 33, 1.0) == _lib.GQ_ENOTSUP  # (gq_sample_topk: 32 candidates)
    torch.cuda.synchronize()
