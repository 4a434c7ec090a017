"""CPU: the host side of the long-prompt pass (guidedquant_amd/native_prompt.py, guidedquant_amd/model.py) -- the mask rows built from positions, the chunk planner, a
cache beyond MASK_TABLE_MAX rows without [n, n] tables -- and the test models of tests/prefill_attn_model.py against each other:
the long grids, the sink profiles, and the float32 emulation of the kernel's online softmax (pam.emulate_row), which states on the
CPU what rounding P to fp16 at scale 1 loses behind a large first key at 2^17 keys, and that the scale 2^15 keeps it."""
import math

import pytest

torch = pytest.importorskip("torch")

import attn_probes  # noqa: E402
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


def test_the_jitter_pool_serves_any_length_and_keeps_its_first_4096_values():
    g = torch.Generator().manual_seed(5)
    old = (2.0 * torch.rand(4096, generator=g) - 1.0).double()  # (what profile_scores drew when its pool ended here)
    for T in (1, 200, 4096):
        assert torch.equal(pam.profile_scores("hi300", T, 64, T - 1), 300.0 + old[:T])
    T = 2**17 + 69
    s = pam.profile_scores("cur_above", T, 64, T - 1)
    assert s.shape == (T,) and torch.equal(s[:4096], old) and float(s[T - 1]) == 100.0
    tail = s[4096:T - 1]
    assert float(tail.abs().max()) <= 1.0 and abs(float(tail.mean())) < 0.02 and tail.unique().numel() > 2**16  # (fresh draws, not a repeat)


def test_long_count_cases_hold_every_pair_and_their_expectation_is_exact():
    """the grid, and count / n of the probe against integer arithmetic: the kernel's sums are integers below 2^24 (times 2^15), exact in
    fp32, so one rounding of 1 / n and one of the product are all that separates it from the expectation (<= 1 fp16 step)"""
    BQ, BK = 64, 64
    cases = pam.long_count_cases(BQ, BK)
    assert len(cases) == 8 and {c[0] for c in cases} == {BQ + 1}
    pairs = {(st, "T+7" if w == st + S + 7 else w) for S, st, w, _, _ in cases}
    assert pairs == {(st, w) for st in (2**17 - BK + 5, 2**17) for w in (0, BK + 1, 4099, "T+7")}
    for axis in (1, 2):  # every start and every window class meets both slacks and both head_dims
        for v in {c[axis] if axis == 1 else min(c[2], 2**17) for c in cases}:
            sub = [c for c in cases if (c[axis] if axis == 1 else min(c[2], 2**17)) == v]
            assert {c[3] for c in sub} == {0, 3} and {c[4] for c in sub} == {64, 128}, (axis, v)
    for S, start, window, slack, hd in cases:
        T = start + S
        assert T < 2**24
        for coarse in (False, True):
            q, K, V, expect = pam.count_probe(2, 1, hd, S, start, window, T + slack, coarse)
            assert K.shape[1] == T + slack and torch.isfinite(K[:, :T].float()).all()
            t = torch.arange(T)
            cls = ((t // hd) % hd) if coarse else (t % hd)
            pre = torch.zeros(T + 1, hd, dtype=torch.int64)
            pre[1:] = torch.cumsum((cls[:, None] == torch.arange(hd)[None, :]).to(torch.int64), dim=0)
            for i in (0, 1, BQ - 1, BQ):
                p = start + i
                lo = p + 1 - window if window and p + 1 > window else 0
                cnt = pre[p + 1] - pre[lo]  # int64 [hd]
                assert int(cnt.sum()) == p + 1 - lo
                want = (cnt.double() / float(p + 1 - lo)).half()
                assert torch.equal(expect[i, :hd], want) and torch.equal(expect[i, hd:], want), (S, start, window, coarse, i)
            lo_all = start + 1 - window if window and start + 1 > window else 0
            assert bool((V[0, :lo_all] == 65504.0).all()) and bool((K[0, :lo_all] == 65504.0).all())  # rows below every window
            assert bool((K[0, lo_all:T] == 0).all())


def _sink_row(name, hd, T, BK):
    """the last query row of a sink profile at T keys: exp2-domain fp32 scores as the kernel forms them, V's first column, the float64
    result and the realised softmax weights relative to the large key"""
    S = 3
    scale = hd**-0.5
    q, K, V = pam.profile_probe(name, 2, 1, hd, S, T - S, T + 3, scale, BK)
    c = torch.tensor(scale, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    x = (K[0, :T].float() @ q[0, S - 1].float()) * c  # (products of +-1 with fp16 multiples of one value: the dot is exact in fp32)
    sd = (K[0, :T].double() @ q[0, S - 1].double()) * float(torch.tensor(scale, dtype=torch.float32))
    want = pam.reference(q, K, V, T - S, scale, 0)[S - 1, :1]
    return x, V[0, :T, :1], want, torch.exp(sd - sd.max()), V


@pytest.mark.parametrize("name", pam.SINK_PROFILES)
def test_sink_profiles_and_the_emulated_softmax_at_long_T(name):
    """sink_first, P rounded at scale 1: every tail weight is 0 in the numerator and the result leaves float64 by the tail's share of the
    softmax times its V, (T - 1) * 0.9 * 2^-25 * max|V| = 3.5e-3 max|V| -- outside error_bound.  At scale 2^15, and for sink_last at either scale, inside."""
    BK, hd, T = 64, 128, 2**17 + 69
    assert pam.SINK_TAIL == math.log(0.9 * 2.0**-25)
    x, v, want, w, V = _sink_row(name, hd, T, BK)
    big = 0 if name == "sink_first" else T - 1
    assert float(w[big]) == 1.0 and float(V[0, big].float().abs().min()) == 2.0 and bool((V[0, big] == -2.0).all())
    tail = torch.cat([w[:big], w[big + 1:]])
    assert 0.89 * 2.0**-25 < float(tail.min()) and float(tail.max()) < 0.91 * 2.0**-25 < 2.0**-25  # K's fp16 rounding moves it by < 1 %
    assert bool((torch.cat([V[0, :big], V[0, big + 1:T]]) == 2.0).all()) and float(V[:, :T].float().abs().max()) == 2.0
    vmax, bound = 2.0, pam.error_bound(T, 2.0)
    err = {k: float((pam.emulate_row(x, v, BK, k) - want).abs().max()) for k in (0, pam.P_SCALE_LOG2)}
    print("%s T %d: unscaled %.3e  scaled %.3e  bound %.3e (x max|V| = %g)" % (name, T, err[0], err[pam.P_SCALE_LOG2], bound, vmax))
    assert err[pam.P_SCALE_LOG2] <= bound
    if name == "sink_first":
        assert err[0] > bound, (err[0], bound)
        lost = (T - 1) * 0.9 * 2.0**-25
        assert abs(err[0] - 2.0 * lost / (1.0 + lost)) < 0.05 * err[0]  # all of the tail's numerator (+2 each), the normaliser's fp32 roundings aside
    else:
        assert err[0] <= bound


def test_the_emulated_softmax_follows_float64_on_the_old_profiles():
    """the emulator itself, where nothing is flushed: every profile at 200 keys and an offset off the tile grid, inside the bound at both
    scales (and a first tile that begins in front of the first attended key)"""
    BK, hd, S, start = 64, 64, 3, 197
    T = start + S
    scale = hd**-0.5
    c = torch.tensor(scale, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    for name in attn_probes.PROFILES + pam.SINK_PROFILES:
        q, K, V = pam.profile_probe(name, 2, 1, hd, S, start, T + 3, scale, BK)
        for window in (0, 70):
            want = pam.reference(q, K, V, start, scale, window)[S - 1, :hd]
            lo = T - window if window else 0
            x = (K[0, lo:T].float() @ q[0, S - 1].float()) * c
            for k in (0, pam.P_SCALE_LOG2):
                got = pam.emulate_row(x, V[0, lo:T], BK, k, first=lo)
                vmax = float(V[0, :T].float().abs().max())
                assert float((got - want).abs().max()) <= pam.error_bound(T, vmax), (name, window, k)


def test_error_bound_reproduces_the_old_bound_at_short_lengths():
    for T in (1, 200, 400):
        assert 2.0**-9 <= pam.error_bound(T, 1.0) <= 2.0**-9 + 3e-5
    assert pam.error_bound(2**17 + 69, 2.0) == (4 * 2.0**-11 + ((2**17 + 69) / 32 + (2**17 + 69) / 64) * 2.0**-24) * 2.0
