"""GPU: packed scoring -- `Transformer.score_packed_native` (guidedquant_amd/native_prompt.py: several sequences as one piece through
gq_rope_cache_rows_packed and gq_attn_prefill_packed) on the tiny models of test_prefill_chunked_gpu.py (Llama, a window model, Qwen2 with
its q/k/v bias, Qwen3 with QK-norm), and `AnyPrecisionForCausalLM.score_many` / `loglikelihood_many` on the tiny Llama of
test_score_native_gpu.py.

  1. one sequence: score_packed_native([a]) is score_native(a) under GQ_PREFILL_ATTN=1, bit for bit (the same shapes, GEMMs, tile grid, head).
  2. content isolation: [a, b, c] and [a', b, c'] (other tokens, the same lengths) give b the same bits; caches full of NaN rows in
     front of the pass leave no NaN in any result.
  3. the kernel route against the SDPA route with the block-diagonal mask (GQ_PREFILL_ATTN=0): test_kv8_model_gpu._close's form on the
     log-probabilities, with that file's fp16 bounds (element-wise 1e-2 of the largest |logprob|, norm-wise 3e-3).
  4. against the one-sequence pass (the public API; Llama, Mistral with a window on every layer, Qwen2 with its bias, Qwen3 with QK-norm):
     not bit-equal, the GEMMs see other row counts.  The yardstick is the distance between the two routes that exist without packing,
     computed here per model: worst |score(native=True) - score(native=False)| over the same sequences; score_many's log-probabilities
     must lie within 2 x the yardstick of score(native=True)'s -- all three are roundings of one model.  (On the `Transformer` itself the
     yardstick is void: its HIP pass and its module forward keep the same rounding points and agree exactly on these models.)
     Measured on an MI355X (worst |dlogprob|: score_many vs score(native=True) / yardstick):
         llama 9.20e-3 / 7.83e-3 (1.17 x)   mistral 1.70e-2 / 1.92e-2 (0.88 x)   qwen2 1.08e-2 / 1.01e-2 (1.07 x)   qwen3 1.75e-2 / 1.44e-2 (1.22 x)
     (3: hip-packed vs sdpa-packed at most 2.6e-4 element-wise and 9.1e-5 norm-wise on the four models.)
  5. loglikelihood_many is the sum over the continuation rows of (4)'s results; with `rows`, head_rows is the continuation token count.
  6. a sequence longer than a pack goes through score() (the one-sequence plan: no "packed" entry).
  7. an fp8 cache, the tensor-parallel and the pipelined decoder raise NotImplementedError.
  8. native=True on a request the fused route does not serve raises."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KINDS = ["llama-2bit", "window8", "qwen2", "qwen3"]
LENS = (23, 40, 17)  # a pack of 80 rows: two query tiles, the second sequence astride row 64
E_BOUND, R_BOUND = 1e-2, 3e-3  # test_kv8_model_gpu.py's fp16 bounds


def _dev():
    return torch.device("cuda:0")


_models = {}


def _model(kind):
    if kind not in _models:
        import test_prefill_chunked_gpu as tpc
        m = tpc._BUILD[kind]()
        m.setup_caches(1, 128)
        assert m.native_ready()
        _models[kind] = m
    m = _models[kind]
    if m.kv_cache_dtype != "fp16":
        m.setup_caches(1, 128, kv_cache_dtype="fp16")
    return m


def _seqs(m, seed, lens=LENS):
    g = torch.Generator(device=_dev()).manual_seed(seed)
    return [torch.randint(0, m.config.vocab_size, (n, ), dtype=torch.int32, device=_dev(), generator=g) for n in lens]


def _split(lp, hit, lens):
    """the per-sequence results of a pass whose head ran on every row"""
    out, b = [], 0
    for n in lens:
        out.append((lp[b:b + n - 1].clone(), hit[b:b + n - 1].clone()))
        b += n
    return out


def _row_tol(dec, s):
    """2 ulp16(max |logit| of the row), the rule between two heads over the same rows (tests/test_head_nll_gpu.py): [n - 1], float64"""
    import head_nll_model as hm
    n = s.numel()
    with torch.no_grad():
        logits = dec.prefill_native(s.view(1, -1).to(torch.int32), torch.arange(n, dtype=torch.int32, device=s.device), start=0, last_only=False)[0, :n - 1]
    return torch.from_numpy(2.0 * hm.ulp16(logits.double().abs().max(dim=1).values.cpu().numpy()))


def _packed(m, seqs, rows=None):
    with torch.no_grad():
        lp, hit = m.score_packed_native(seqs, rows)
    torch.cuda.synchronize()
    return lp, hit


@pytest.mark.parametrize("kind", KINDS)
def test_one_sequence_is_score_native_bit_for_bit(kind, monkeypatch):
    monkeypatch.setenv("GQ_PREFILL_ATTN", "1")
    m = _model(kind)
    a = _seqs(m, 5, (70, ))[0]
    with torch.no_grad():
        want_lp, want_g = m.score_native(a)
    head = m.last_prefill_plan["head"]
    assert m.last_prefill_plan["attn"] == ["hip"] * len(m.layers)
    lp, hit = _packed(m, [a])
    assert m.last_prefill_plan == dict(chunks=[(0, 70)], attn=["hip-packed"] * len(m.layers), head=head, packed=dict(sequences=1, rows=70, head_rows=70))
    assert lp.shape == (70, ) and float(lp[-1]) == 0.0 and not bool(hit[-1])
    assert torch.equal(lp[:-1].view(torch.int32), want_lp.view(torch.int32)) and torch.equal(hit[:-1], want_g)


@pytest.mark.parametrize("attn", ["auto", "0"])
@pytest.mark.parametrize("kind", KINDS)
def test_content_isolation_and_nan_caches(kind, attn, monkeypatch):
    monkeypatch.setenv("GQ_PREFILL_ATTN", attn)
    m = _model(kind)
    a, b, c = _seqs(m, 6)
    a2, _, c2 = _seqs(m, 7)
    for blk in m.layers:
        blk.attention.kv_cache.k_cache.fill_(float("nan"))
        blk.attention.kv_cache.v_cache.fill_(float("nan"))
    lp1, hit1 = _packed(m, [a, b, c])
    assert m.last_prefill_plan["attn"] == ["sdpa-packed" if attn == "0" else "hip-packed"] * len(m.layers)
    assert m.last_prefill_plan["packed"] == dict(sequences=3, rows=sum(LENS), head_rows=sum(LENS))
    lp2, hit2 = _packed(m, [a2, b, c2])
    assert bool(torch.isfinite(lp1).all()) and bool(torch.isfinite(lp2).all())
    r1, r2 = _split(lp1, hit1, LENS), _split(lp2, hit2, LENS)
    assert torch.equal(r1[1][0].view(torch.int32), r2[1][0].view(torch.int32)) and torch.equal(r1[1][1], r2[1][1])
    assert not torch.equal(r1[0][0], r2[0][0])  # (the other sequences did change)


def _close(got, want, what):
    scale = want.abs().max().item()
    e, r = (got - want).abs().max().item() / scale, ((got - want).norm() / want.norm()).item()
    print("%s: max|logprob| %.3f  element-wise %.3e  norm-wise %.3e   (bounds %.3e / %.3e)" % (what, scale, e, r, E_BOUND, R_BOUND))
    assert torch.isfinite(got).all()
    assert e <= E_BOUND, (what, e)
    assert r <= R_BOUND, (what, r)


@pytest.mark.parametrize("kind", KINDS)
def test_kernel_route_against_the_sdpa_packed_route(kind, monkeypatch):
    m = _model(kind)
    seqs = _seqs(m, 8)
    monkeypatch.setenv("GQ_PREFILL_ATTN", "0")
    want, _ = _packed(m, seqs)
    assert set(m.last_prefill_plan["attn"]) == {"sdpa-packed"}
    monkeypatch.setenv("GQ_PREFILL_ATTN", "auto")
    got, _ = _packed(m, seqs)
    assert set(m.last_prefill_plan["attn"]) == {"hip-packed"}
    _close(got.double(), want.double(), kind + " hip-packed vs sdpa-packed")


def test_rows_reach_the_head_alone(monkeypatch):
    monkeypatch.delenv("GQ_PREFILL_ATTN", raising=False)
    m = _model("llama-2bit")
    seqs = _seqs(m, 10)
    full, fhit = _packed(m, seqs)
    rows = torch.zeros(sum(LENS), dtype=torch.bool)
    rows[20:22] = True   # the last two predictions of the first sequence
    rows[23 + 36:23 + 39] = True
    lp, hit = _packed(m, seqs, rows.to(_dev()))
    assert m.last_prefill_plan["packed"] == dict(sequences=3, rows=sum(LENS), head_rows=5) and lp.shape == (5, )
    sel = rows.to(_dev())
    # (the same pass up to the head's row count: the rule between two heads, 2 ulp16 of the row's largest logit)
    tol = torch.cat([_row_tol(m, seqs[0])[20:22], _row_tol(m, seqs[1])[36:39]])
    assert bool(((lp - full[sel]).abs().double().cpu() <= tol).all()) and hit.dtype == torch.bool and hit.shape == (5, )


def test_fp8_tp_and_pipeline_raise():
    from guidedquant_amd.pipeline import PipelinedDecoder
    from guidedquant_amd.tp import TensorParallelDecoder
    for cls in (TensorParallelDecoder, PipelinedDecoder):
        with pytest.raises(NotImplementedError, match="packed scoring"):
            cls.score_packed_native(object())
    m = _model("llama-2bit")
    m.setup_caches(1, 128, kv_cache_dtype="fp8")
    try:
        with pytest.raises(NotImplementedError, match="packed scoring: fp8 KV cache"):
            m.score_packed_native(_seqs(m, 1))
    finally:
        m.setup_caches(1, 128, kv_cache_dtype="fp16")


# ------------------------------------------------------------------------------------------------ the public API
_api = {}
API_KINDS = ["llama", "mistral", "qwen2", "qwen3"]


def _hf(kind="llama"):
    """the tiny Llama of test_score_native_gpu.py; the sliding-window Mistral (every layer), Qwen2 (q/k/v bias, mixed layers) and Qwen3
    (QK-norm, head_dim 128, mixed layers) of test_sliding_window_fused_gpu.py"""
    if kind not in _api:
        if kind == "llama":
            import test_score_native_gpu as tsn
            _api[kind] = tsn._hf_tiny()
        else:
            import test_sliding_window_fused_gpu as tsw
            _api[kind] = tsw._hf_model(tsw._config(kind, 128 if kind == "qwen3" else 64)[0])
    return _api[kind]


def _api_seqs(lens, seed=21):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 500, (n, ), generator=g) for n in lens]


API_LENS = (30, 75, 41, 64, 2, 119)


@pytest.mark.parametrize("kind", API_KINDS)
def test_score_many_against_score_and_its_yardstick(kind, monkeypatch):
    monkeypatch.delenv("GQ_PREFILL_ATTN", raising=False)
    monkeypatch.delenv("GQ_PREFILL_CHUNK", raising=False)
    m = _hf(kind)
    seqs = _api_seqs(API_LENS)
    fused = [m.score(s, native=True) for s in seqs]
    assert "packed" not in m._native_cache[("decoder", 2)].last_prefill_plan
    tree = [m.score(s, native=False) for s in seqs]
    yard = max(float((f["logprobs"] - t["logprobs"]).abs().max()) for f, t in zip(fused, tree))
    many = m.score_many(seqs, pack_tokens=160)
    dec = m._native_cache[("decoder", 2)]  # (asked for here: the module tree's pass in between may have rebuilt the decoder)
    # (first fit at 160 rows: [30, 75, 41, 2] -- 2 goes back into the first pack -- | [64] | [119]: the last pass is the third pack's)
    assert dec.last_prefill_plan["packed"] == dict(sequences=1, rows=119, head_rows=119) and set(dec.last_prefill_plan["attn"]) == {"hip-packed"}
    assert len(many) == len(seqs)
    worst = 0.0
    for r, f, n in zip(many, fused, API_LENS):
        assert r["logprobs"].shape == (n - 1, ) and r["greedy"].shape == (n - 1, ) and r["logprobs"].dtype == torch.float32
        assert r["nll"] == pytest.approx(float(-r["logprobs"].double().mean()))
        worst = max(worst, float((r["logprobs"] - f["logprobs"]).abs().max()))
    print("%s: score_many vs score(native=True) %.3e   yardstick |score(native=True) - score(native=False)| %.3e   ratio %.2f" % (
        kind, worst, yard, worst / max(yard, 1e-30)))
    assert worst <= 2.0 * yard, (worst, yard)


def test_score_many_off_the_fused_route_is_a_loop_over_score():
    m = _hf()
    seqs = _api_seqs(API_LENS)[:2]
    tree = [m.score(s, native=False) for s in seqs]
    loop = m.score_many(seqs, native=False)
    assert all(torch.equal(a["logprobs"], b["logprobs"]) and torch.equal(a["greedy"], b["greedy"]) and a["nll"] == b["nll"] for a, b in zip(loop, tree))
    assert m.score_many([]) == [] and m.loglikelihood_many([]) == []


def test_loglikelihood_many_sums_the_continuation_rows(monkeypatch):
    monkeypatch.delenv("GQ_PREFILL_ATTN", raising=False)
    m = _hf()
    lens, conts = (30, 75, 41, 12), (5, 1, 40, 11)
    seqs = _api_seqs(lens, seed=22)
    pairs = [(s[:n - k], s[n - k:]) for s, n, k in zip(seqs, lens, conts)]
    many = m.score_many(seqs, pack_tokens=256)
    got = m.loglikelihood_many(pairs, pack_tokens=256)
    dec = m._native_cache[("decoder", 2)]
    assert dec.last_prefill_plan["packed"] == dict(sequences=4, rows=sum(lens), head_rows=sum(conts))
    for (ll, greedy), r, k, s in zip(got, many, conts, seqs):
        # (the same pass up to the head's row count: per token the rule between two heads, 2 ulp16 of the row's largest logit)
        tol = float(_row_tol(dec, s.to(m.device))[-k:].sum())
        assert abs(ll - float(r["logprobs"][-k:].double().sum())) <= tol, (ll, tol)
        assert isinstance(ll, float) and isinstance(greedy, bool)
    one = [m.loglikelihood(c, t) for c, t in pairs]
    print("loglikelihood_many vs loglikelihood: %r" % [(round(a[0], 4), round(b[0], 4)) for a, b in zip(got, one)])
    with pytest.raises(ValueError, match="at least one token each"):
        m.loglikelihood_many([(seqs[0], seqs[0][:0])])


def test_an_over_long_sequence_goes_through_score(monkeypatch):
    monkeypatch.delenv("GQ_PREFILL_ATTN", raising=False)
    m = _hf()
    seqs = _api_seqs((20, 90, 25), seed=23)
    calls = []
    real = type(m).score
    monkeypatch.setattr(type(m), "score", lambda self, ids, **kw: (calls.append(int(torch.as_tensor(ids).numel())), real(self, ids, **kw))[1])
    many = m.score_many(seqs, pack_tokens=64)
    assert calls == [90]  # the pack [20, 25] is one packed pass, the over-long sequence the one-sequence pass
    one = real(m, seqs[1])
    assert torch.equal(many[1]["logprobs"], one["logprobs"]) and many[1]["nll"] == one["nll"]
    assert [r["logprobs"].shape[0] for r in many] == [19, 89, 24]


def test_native_true_raises_on_an_unserved_request(monkeypatch):
    m = _hf()
    seqs = _api_seqs((20, 25), seed=24)
    dec = m.native_decoder(2)
    monkeypatch.setattr(type(dec), "prefill_ready", lambda self, idx: False)
    with pytest.raises(ValueError, match="native=True: the fused model's prompt pass"):
        m.score_many(seqs, native=True)
    with pytest.raises(ValueError, match="native=True"):
        m.loglikelihood_many([(seqs[0][:5], seqs[0][5:])], native=True)
    assert len(m.score_many(seqs)) == 2  # (the automatic route falls back to the module tree)
    monkeypatch.undo()
    with pytest.raises(ValueError, match="token ids must lie in"):
        m.score_many([torch.tensor([1, 500, 2])])
    with pytest.raises(ValueError, match="at least two tokens"):
        m.score_many([torch.tensor([1])])
    with pytest.raises(ValueError, match="pack_tokens"):
        m.score_many(seqs, pack_tokens=1)
