"""CPU: the host side of the long-prompt pass (guidedquant_amd/model.py) -- the mask rows built from positions, the chunk planner, a
cache beyond MASK_TABLE_MAX rows without [n, n] tables -- and the test models of tests/prefill_attn_model.py against each other."""
import pytest

torch = pytest.importorskip("torch")

import prefill_attn_model as pam  # noqa: E402


@pytest.mark.parametrize("W", [None, 1, 3, 16])
def test_mask_rows_from_positions_equal_the_table_rows(W):
    from guidedquant_amd.model import mask_rows, window_mask
    n = 16
    table = window_mask(n, W)
    for pos in (torch.arange(n), torch.tensor([0]), torch.tensor([15, 3, 7]), torch.arange(5, 12, dtype=torch.int32)):
        got = mask_rows(pos, n, W)
        assert got.dtype == torch.bool and torch.equal(got, table[pos.long()])
        assert torch.equal(mask_rows(pos, 9, W), table[pos.long(), :9])  # (the prompt pass reads the first T columns only)
    # and the tests' own statement of the rule
    assert torch.equal(pam.attend_mask(7, 5, 12, W or 0), table[5:12, :12])


@pytest.mark.parametrize("S,chunk", [(1, 4), (4, 4), (5, 4), (8, 4), (9, 4), (70, 16), (17, 16), (16390, 4096), (3, 1)])
def test_chunk_planner_covers_the_prompt_once_in_order(S, chunk):
    from guidedquant_amd.model import prefill_chunks
    for start in (0, 7):
        pieces = prefill_chunks(S, chunk, start)
        at = start
        for a, n in pieces:
            assert a == at and 1 <= n <= chunk
            at += n
        assert at == start + S
        assert all(n == chunk for _, n in pieces[:-1]) and len(pieces) == -(-S // chunk)
    assert prefill_chunks(5, 4) == [(0, 4), (4, 1)]  # (S = chunk + 1: a one-token tail)


def _pair(monkeypatch, windows):
    import guidedquant_amd.model as M
    torch.manual_seed(0)
    kw = dict(block_size=32, vocab_size=64, n_layer=2, n_head=4, n_local_heads=2, dim=64, intermediate_size=128, model_name="llama-tiny",
              layer_windows=windows)
    tabled = M.Transformer(torch.float32, M.ModelArgs(**kw)).eval()
    bare = M.Transformer(torch.float32, M.ModelArgs(**kw)).eval()
    bare.load_state_dict(tabled.state_dict())
    tabled.setup_caches(1, 16)
    monkeypatch.setattr(M, "MASK_TABLE_MAX", 8)
    bare.setup_caches(1, 16)
    return tabled, bare


@pytest.mark.parametrize("windows", [None, (None, 3), (5, 3)])
def test_a_cache_beyond_the_table_limit_keeps_no_tables_and_computes_the_same(monkeypatch, windows):
    import guidedquant_amd.model as M
    assert M.MASK_TABLE_MAX == 16384
    tabled, bare = _pair(monkeypatch, windows)
    assert tabled.causal_mask.shape == (16, 16) and set(tabled.window_masks) == {w for w in (windows or ()) if w is not None}
    assert getattr(bare, "causal_mask", None) is None and not getattr(bare, "window_masks", None)
    big = [n for n, t in list(bare.named_buffers()) + list(vars(bare).items()) if isinstance(t, torch.Tensor) and t.dtype == torch.bool]
    assert not big, big
    idx = torch.randint(0, 64, (1, 10))
    with torch.no_grad():
        want, got = tabled(idx, torch.arange(10)), bare(idx, torch.arange(10))
        assert torch.equal(got, want)  # bit for bit: the same mask bits
        # a decode step at a later position, int32 positions as generate() passes them
        tok, pos = torch.randint(0, 64, (1, 1)), torch.tensor([10], dtype=torch.int32)
        assert torch.equal(bare(tok, pos), tabled(tok, pos))


def test_reference_and_count_probe_agree():
    """the float64 reference on the count probe's tensors gives the probe's own expectation: the mask rule is stated once in each"""
    BQ, BK = 64, 64
    for S, start, window, slack, hd in pam.covering_cases(BQ, BK)[::4]:
        T = start + S
        for coarse in (False, True):
            q, K, V, expect = pam.count_probe(2, 1, hd, S, start, window, T + slack, coarse)
            assert torch.isfinite(K[:, :T].float()).all() and K.shape[1] == T + slack
            ref = pam.reference(q, K, V, start, hd**-0.5, window)
            assert float((ref - expect.double()).abs().max()) <= 2.0**-11, (S, start, window)


def test_covering_cases_hold_every_value_and_every_pair():
    BQ, BK = 64, 64
    cases = pam.covering_cases(BQ, BK)
    assert len(cases) <= 80
    wins = {(S, "T+7" if w == st + S + 7 else w) for S, st, w, _, _ in cases}
    assert len(wins) == 35
    for S in (1, BQ - 1, BQ, BQ + 1, 2 * BQ + 3):
        assert {w for s, w in wins if s == S} == {0, 1, 2, BK - 1, BK, BK + 1, "T+7"}
