"""CPU: the host model of gq_sample_full (tests/sampler_full_model.py) against transformers' warper chain and against the models of the
shipped sampler, and the evidence that its committed cases catch every deviation of FAULTS and keep the undecided share small."""
import functools

import numpy as np
import pytest

import sampler_full_model as fm
import sampler_rep_model as rm


@functools.lru_cache(maxsize=None)
def _run(name):
    return fm.case_run(fm.CASE_BY_NAME[name])


CHAIN = [  # (V, profile, T, top_k, top_p, min_p): small vocabularies without ties at a cut (transformers' top-k keeps EVERY token that ties the k-th),
    # every filter alone and together
    (100, "gauss", 1.0, 0, 1.0, 0.0), (100, "gauss", 0.7, 0, 0.9, 0.0), (100, "gauss", 1.0, 0, 1.0, 0.1), (300, "gauss", 1.3, 80, 1.0, 0.0),
    (300, "gauss", 0.8, 80, 0.9, 0.05), (200, "gauss", 1.0, 70, 0.8, 0.0), (250, "gauss", 1.5, 0, 0.95, 0.02), (100, "peaky", 1.0, 70, 0.9, 0.2),
]


@pytest.mark.parametrize("V,prof,T,top_k,top_p,min_p", CHAIN)
def test_frequencies_follow_transformers_warper_chain(V, prof, T, top_k, top_p, min_p):
    torch = pytest.importorskip("torch")
    lpz = pytest.importorskip("transformers.generation.logits_process")
    x = fm.profile(prof, V)
    scores = torch.from_numpy(x.astype(np.float32))[None, :]
    ids = torch.zeros((1, 1), dtype=torch.long)
    chain = [lpz.TemperatureLogitsWarper(T)] + ([lpz.TopKLogitsWarper(top_k)] if top_k else []) + ([lpz.TopPLogitsWarper(top_p)] if top_p < 1 else []) \
        + ([lpz.MinPLogitsWarper(min_p)] if min_p > 0 else [])
    for w in chain:
        scores = w(ids, scores)
    probs = torch.softmax(scores, dim=-1)[0].numpy().astype(np.float64)
    n = 3000
    r = fm.run(x, n, top_k, T, top_p, min_p, seed=5, counter=100)
    # the support first: the float32 chain and the model keep the same tokens (the vocabularies are chosen so that no cut is a near-tie)
    assert r.cut_pinned
    st_ids = sorted(np.nonzero(probs > 0)[0].tolist())
    order = np.lexsort((np.arange(V), -rm.image32(x.astype(np.float32))))
    assert sorted(order[:int(r.n[0])].tolist()) == st_ids, (int(r.n[0]), len(st_ids))
    assert set(r.tokens.tolist()) <= set(st_ids)
    freq = np.bincount(r.tokens, minlength=V) / n
    # every probability within 5 standard deviations of its binomial (plus one count): 8 vectors x <= 300 tokens, fixed seeds
    tol = 5.0 * np.sqrt(probs * (1 - probs) / n) + 1.0 / n
    assert (np.abs(freq - probs) <= tol).all(), float((np.abs(freq - probs) - tol).max())


@pytest.mark.parametrize("fault", fm.FAULTS)
def test_every_fault_changes_a_decided_draw(fault):
    hit = []
    for c in fm.CASES:
        if c.V > 32000:
            continue
        good = _run(c.name)
        bad = fm.case_run(c, forced=good.tokens, fault=fault)
        dec = ~good.undecided
        if (bad.tokens[dec] != good.tokens[dec]).any():
            hit.append(c.name)
            break
    assert hit, fault


def test_undecided_share():
    tot = und = 0
    for c in fm.CASES:
        r = _run(c.name)
        assert c.n <= 300
        assert float(r.undecided.mean()) <= 0.05, (c.name, float(r.undecided.mean()))
        assert ((r.n_lo <= r.n) & (r.n <= r.n_hi) & (r.n_hi <= r.n_k)).all(), c.name
        if c.pinned:
            assert r.cut_pinned, c.name
        tot += c.n
        und += int(r.undecided.sum())
    assert und <= 0.02 * tot, (und, tot)
    # every filter alone has a case whose cut is pinned exactly
    pinned = [c for c in fm.CASES if c.pinned]
    assert any(c.top_k and c.top_p == 1 and not c.min_p for c in pinned) and any(not c.top_k and c.top_p < 1 and not c.min_p for c in pinned)
    assert any(not c.top_k and c.top_p == 1 and c.min_p for c in pinned)


def test_the_grants_keep_the_contracts_caps():
    assert fm.G_MASS <= 2.0**-16
    for a, m in ((0.0, 0.0), (3.0, 5.0), (-1e5, 1e5), (0.3, -0.2)):
        assert fm.g_a(a, m) <= 2.0**-18 * max(1.0, abs(a) + abs(m))
        assert fm.g_a(a, m) >= 2.0**-24 * (abs(a) + abs(m)) + 2.0**-22


@pytest.mark.parametrize("name", [c.name for c in rm.CASES if c.V <= 4096 and c.top_p == 1.0])
def test_up_to_64_candidates_the_draws_are_sampler_rep_models(name):
    """top_k <= 64, top_p = 1, min_p = 0: the same tokens, admissible sets, state and seen set as sampler_rep_model, draw for draw"""
    c = rm.CASE_BY_NAME[name]
    x, seen0, suppress, ban = rm.case_inputs(c)
    n = min(c.n, 120)
    old = rm.run(x, n, c.top_k, c.T, c.top_p, c.seed, c.counter, c.pos0, ban, c.seq_cap, c.rp, seen0, suppress)
    new = fm.run(x, n, max(c.top_k, 1), c.T, 1.0, 0.0, c.seed, c.counter, c.pos0, ban, c.seq_cap, c.rp, seen0, suppress)
    assert np.array_equal(old.tokens, new.tokens) and np.array_equal(old.undecided, new.undecided)
    assert all(sorted(a.tolist()) == sorted(b.tolist()) for a, b in zip(old.admissible, new.admissible))
    assert (old.counter, old.pos, old.tok) == (new.counter, new.pos, new.tok) and {k: v for k, v in old.seq.items()} == new.seq
    assert np.array_equal(old.seen, new.seen)
    assert (new.n == np.minimum(new.n_k, max(c.top_k, 1))).all()
