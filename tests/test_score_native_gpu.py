"""GPU: `Transformer.score_native` (the HIP prompt pass with the scoring head gq_head_nll) and `AnyPrecisionForCausalLM.score` on the
fused route, on tiny random-init models built like those of test_kv8_model_gpu.py: Llama (dim 512, 2 layers, V = 1000) and Qwen3
(QK-norm, dim 256, 1 layer, V = 777) -- vocabularies that are no multiple of the kernel's 128-row tile, S = 131 rows (two row tiles).

The rule of every comparison (tests/test_head_nll_gpu.py, round-off family): two heads over the same rows may round a logit to
neighbouring fp16 values, so |dlogprob| <= 2 ulp16(max |logit| of the row) -- one step for the target's logit, one for the largest
term of the sum -- and the greedy flags are compared on the rows whose top-two gap is at least 2 ulp16.
  * score_native (kernel) against prefill_native(last_only=False) -> fp32 log_softmax -> gather;
  * chunk = 48 at S = 131 (pieces of 48, 48, 35 rows over the same caches) against one piece, both passes with GQ_PREFILL_ATTN=1 so that
    they differ in the chunking alone (measured: identical).  Under GQ_PREFILL_ATTN=auto the one-piece pass attends through torch SDPA
    and the chunked one through gq_attn_prefill; those two PASSES then differ by up to 2.4e-3 = 1.23 x the bound on the Llama model
    (0.38 x on Qwen3) while the two heads on the same rows agree to 1e-6 -- a difference of the attention implementations;
  * GQ_SCORE_HEAD=0 (the torch head in row blocks) against 1;
  * an fp8 KV cache runs, and the plan records the head;
  * a generate() after a score() -- one that grows the caches and so evicts the captured graph -- returns the tokens it returned before.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import head_nll_model as hm  # noqa: E402

S = 131
CACHE = 256


def _dev():
    return torch.device("cuda:0")


def _tiny(name, vocab, dim, n_head, n_layer, **extra):
    from guidedquant_amd.APLinear import APLinear
    from guidedquant_amd.generate import random_init_
    from guidedquant_amd.model import ModelArgs, Transformer
    d = _dev()
    cfg = ModelArgs(block_size=CACHE, vocab_size=vocab, n_layer=n_layer, n_head=n_head, dim=dim, intermediate_size=2 * dim, n_local_heads=2,
                    rope_base=500000, model_name=name, **extra)
    m = Transformer(torch.float16, cfg, linear_class=APLinear, linear_kwargs=dict(bitwidth=2, device=d)).to(device=d, dtype=torch.float16)
    random_init_(m, seed=2, lut_std=0.05)
    g = torch.Generator(device=d)
    g.manual_seed(1)
    for b in m.layers:
        b.input_layernorm.weight.data.copy_((1 + 0.1 * torch.randn(cfg.dim, device=d, generator=g)).half())
        b.post_attention_layernorm.weight.data.copy_((1 + 0.1 * torch.randn(cfg.dim, device=d, generator=g)).half())
        if cfg.qk_norm:
            b.attention.q_norm.weight.data.copy_((1 + 0.1 * torch.randn(cfg.head_dim, device=d, generator=g)).half())
            b.attention.k_norm.weight.data.copy_((1 + 0.1 * torch.randn(cfg.head_dim, device=d, generator=g)).half())
    m.norm.weight.data.copy_((1 + 0.1 * torch.randn(cfg.dim, device=d, generator=g)).half())
    return m.eval()


_BUILD = {
    "llama": lambda: _tiny("llama-test", 1000, 512, 8, 2),
    "qwen3": lambda: _tiny("qwen3-test", 777, 256, 4, 1, qk_norm=True, head_dim=64),
}
_cache = {}


def _model(kind):
    """the model, its S token ids, and the reference of the whole-piece pass: (logprob, row tolerance, rows with a clear top1, greedy)
    from prefill_native's logits -- computed once"""
    if kind not in _cache:
        m = _BUILD[kind]()
        m.setup_caches(1, CACHE)
        d = _dev()
        idx = torch.randint(0, m.config.vocab_size, (S, ), dtype=torch.int32, device=d, generator=torch.Generator(device=d).manual_seed(7))
        with torch.no_grad():
            logits = m.prefill_native(idx.view(1, -1), torch.arange(S, dtype=torch.int32, device=d), start=0, last_only=False)[0, :S - 1]
            assert m.last_prefill_plan.get("head") is None
            ls = torch.log_softmax(logits.float(), dim=-1)
            want = ls.gather(1, idx[1:].long()[:, None])[:, 0].double().cpu().numpy()
        l64 = logits.double().cpu().numpy()
        srt = np.sort(l64, axis=1)
        clear = (srt[:, -1] - srt[:, -2]) >= 2.0 * hm.ulp16(srt[:, -1])
        tol = 2.0 * hm.ulp16(np.abs(l64).max(axis=1))
        greedy = l64.argmax(axis=1) == idx[1:].cpu().numpy()
        _cache[kind] = (m, idx, want, tol, clear, greedy)
    return _cache[kind]


def _score(m, idx, head, monkeypatch, chunk=None):
    monkeypatch.setenv("GQ_SCORE_HEAD", head)
    with torch.no_grad():
        lp, greedy = m.score_native(idx, chunk=chunk)
    assert lp.shape == (S - 1, ) and lp.dtype == torch.float32 and greedy.shape == (S - 1, ) and greedy.dtype == torch.bool
    assert m.last_prefill_plan["head"] == ("hip-nll" if head == "1" else "torch")
    assert bool(torch.isfinite(lp).all()) and bool((lp <= 0).all())
    return lp.double().cpu().numpy(), greedy.cpu().numpy()


def _close(got, want, tol, what):
    d = np.abs(got - want)
    print("%s: worst |dlogprob| %.3e, worst |dlogprob| / (2 ulp16) %.3f" % (what, d.max(), (d / tol).max()))
    assert (d <= tol).all(), (what, (d / tol).max())


@pytest.mark.parametrize("kind", list(_BUILD))
def test_kernel_head_matches_the_logits_of_prefill_native(kind, monkeypatch):
    m, idx, want, tol, clear, greedy = _model(kind)
    assert clear.mean() >= 0.9
    got, g = _score(m, idx, "1", monkeypatch)
    _close(got, want, tol, kind + " kernel head vs prefill_native logits")
    assert np.array_equal(g[clear], greedy[clear])
    assert len(m.last_prefill_plan["chunks"]) == 1


@pytest.mark.parametrize("kind", list(_BUILD))
def test_chunked_pass_matches_one_piece(kind, monkeypatch):
    m, idx, want, tol, clear, greedy = _model(kind)
    # (the attention kernel in both passes, so that they differ in the chunking alone: under GQ_PREFILL_ATTN=auto a one-piece pass
    # attends through torch SDPA and a chunked one through gq_attn_prefill -- two attention implementations, whose difference
    # test_prefill_chunked_gpu.py bounds on the logits and which is no property of the scoring head)
    monkeypatch.setenv("GQ_PREFILL_ATTN", "1")
    one, g1 = _score(m, idx, "1", monkeypatch)
    got, g = _score(m, idx, "1", monkeypatch, chunk=48)
    assert set(m.last_prefill_plan["attn"]) == {"hip"}
    assert m.last_prefill_plan["chunks"] == [(0, 48), (48, 48), (96, 35)]
    _close(got, one, tol, kind + " chunk 48 vs one piece")
    assert np.array_equal(g[clear], g1[clear])


@pytest.mark.parametrize("kind", list(_BUILD))
def test_torch_head_matches_the_kernel_head(kind, monkeypatch):
    m, idx, want, tol, clear, greedy = _model(kind)
    monkeypatch.setattr(type(m), "SCORE_HEAD_ROWS", 50)  # (three row blocks at S = 131)
    ref, g0 = _score(m, idx, "0", monkeypatch)
    got, g1 = _score(m, idx, "1", monkeypatch)
    _close(got, ref, tol, kind + " kernel head vs torch head")
    _close(ref, want, tol, kind + " torch head vs prefill_native logits")
    assert np.array_equal(g0[clear], g1[clear])
    monkeypatch.setenv("GQ_SCORE_HEAD", "auto")
    with torch.no_grad():
        m.score_native(idx)
    assert m.last_prefill_plan["head"] == ("hip-nll" if type(m).SCORE_HEAD_AUTO == "1" else "torch")
    monkeypatch.setenv("GQ_SCORE_HEAD", "yes")
    with pytest.raises(ValueError, match="GQ_SCORE_HEAD"):
        m.score_native(idx)


def test_fp8_cache_runs_and_the_plan_records_the_head(monkeypatch):
    m, idx, want, tol, clear, greedy = _model("llama")
    m.setup_caches(1, CACHE, kv_cache_dtype="fp8")
    try:
        got, g = _score(m, idx, "1", monkeypatch)
        assert m.last_prefill_plan["attn"] == ["hip-kv8"] * len(m.layers) and m.last_prefill_plan["head"] == "hip-nll"
        ref, g0 = _score(m, idx, "0", monkeypatch)
        assert m.last_prefill_plan["attn"] == ["hip-kv8"] * len(m.layers) and m.last_prefill_plan["head"] == "torch"
        _close(got, ref, tol, "fp8 cache: kernel head vs torch head")
        assert np.abs(got - want).max() > 0.0  # (three mantissa bits in the cache: close to the fp16-cache pass, and not it)
    finally:
        m.setup_caches(1, CACHE, kv_cache_dtype="fp16")


def _hf_tiny():
    transformers = pytest.importorskip("transformers")
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    hf = transformers.LlamaConfig(hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=2,
                                  vocab_size=500, max_position_embeddings=512, rms_norm_eps=1e-5, tie_word_embeddings=False)
    names = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]
    hf.anyprec = dict(seed_precision=2, parent_precision=2, group_count=1, arch_config=dict(module_names=names, model_name="model", layers_name="layers"))
    m = AnyPrecisionForCausalLM.from_config_random(hf, device=_dev(), seed=5)
    with torch.no_grad():
        m.model.model.embed_tokens.weight.mul_(25.0)
        m.model.lm_head.weight.mul_(10.0)
    return m


def test_generate_after_score_returns_the_same_tokens(monkeypatch):
    monkeypatch.delenv("GQ_PREFILL_ATTN", raising=False)
    monkeypatch.setenv("GQ_SCORE_HEAD", "1")
    m = _hf_tiny()
    d = m.device
    ids = torch.randint(0, 500, (1, 20), device=d, generator=torch.Generator(device=d).manual_seed(3))
    plain = m.generate(ids, max_new_tokens=12, do_sample=False, pad_token_id=0)
    dec = m._native_cache[("decoder", 2)]
    assert dec.max_seq_length == 256 and sum(1 for k in m._native_cache if k[0] == "graph") == 1
    # a score within the caches: nothing is re-allocated, the graph stays
    r = m.score(ids)
    assert r["logprobs"].shape == (19, ) and r["greedy"].shape == (19, ) and dec.last_prefill_plan["head"] == "hip-nll"
    assert r["nll"] == pytest.approx(float(-r["logprobs"].double().mean()))
    assert dec.max_seq_length == 256 and sum(1 for k in m._native_cache if k[0] == "graph") == 1
    assert torch.equal(m.generate(ids, max_new_tokens=12, do_sample=False, pad_token_id=0), plain)
    # a score beyond them: the caches grow, the graph captured over the old ones is evicted
    long_ids = torch.randint(0, 500, (300, ), device=d, generator=torch.Generator(device=d).manual_seed(4))
    r = m.score(long_ids)
    assert r["logprobs"].shape == (299, ) and dec.max_seq_length == 512
    assert sum(1 for k in m._native_cache if k[0] == "graph") == 0
    again = m.generate(ids, max_new_tokens=12, do_sample=False, pad_token_id=0)
    assert torch.equal(again, plain)
    # the module tree gives the same answer up to the rounding of two different passes
    tree, fused = m.score(ids, native=False), m.score(ids)
    print("fused vs module tree nll: %.6f %.6f" % (fused["nll"], tree["nll"]))
    assert fused["nll"] == pytest.approx(tree["nll"], rel=1e-2)
    ll, _ = m.loglikelihood(ids[0, :15], ids[0, 15:])
    assert ll == pytest.approx(float(m.score(ids)["logprobs"][-5:].double().sum()), abs=1e-9)
    with pytest.raises(ValueError, match="token ids must lie in"):
        m.score(torch.tensor([1, 500, 2], device=d))


def test_score_leaves_the_decoder_usable_outside_inference_mode(monkeypatch):
    """score() on a fresh decoder grows its caches from 8 rows: they are allocated outside inference mode (as generate allocates them), so
    the in-place torch updates of other public calls -- the module forward's cache write under no_grad, set_kv_scales -- still work;
    and a decoder whose prompt pass does not serve the request is a routing decision: the module tree scores, the caches stay"""
    monkeypatch.delenv("GQ_PREFILL_ATTN", raising=False)
    monkeypatch.setenv("GQ_SCORE_HEAD", "1")
    m = _hf_tiny()
    d = m.device
    long_ids = torch.randint(0, 500, (300, ), device=d, generator=torch.Generator(device=d).manual_seed(4))
    r = m.score(long_ids)  # (the first call of the model: builds the decoder, caches 8 -> 512 rows)
    dec = m._native_cache[("decoder", 2)]
    assert dec.max_seq_length == 512 and dec.last_prefill_plan["head"] == "hip-nll" and r["logprobs"].shape == (299, )
    kc = dec.layers[0].attention.kv_cache
    assert not kc.k_cache.is_inference() and not dec.rope_cos.is_inference()
    ids32 = long_ids[:6].to(torch.int32)
    with torch.no_grad():
        out = dec(ids32[:5].view(1, -1), torch.arange(5, device=d, dtype=torch.int32))  # (KVCache.update writes the rows in place)
        step = dec.decode_native(ids32[5:6], torch.tensor([5], dtype=torch.int32, device=d))
    assert out.shape == (1, 5, 500) and bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(step.float()).all())
    r8 = m.score(long_ids, kv_cache_dtype="fp8")
    assert dec.kv_cache_dtype == "fp8" and dec.last_prefill_plan["attn"] == ["hip-kv8"] * len(dec.layers)
    kc = dec.layers[0].attention.kv_cache
    assert not kc.k_scale.is_inference() and not kc.k_cache.is_inference()
    two = torch.full((len(dec.layers), dec.config.n_local_heads), 2.0)
    dec.set_kv_scales(two, 0.5 * two)  # (in-place writes of the scale buffers)
    assert kc.k_scale.tolist() == [2.0, 2.0] and kc.v_inv.tolist() == [1.0, 1.0]
    assert bool(torch.isfinite(r8["logprobs"]).all()) and r8["logprobs"].shape == (299, )
    # a decoder whose prompt pass does not serve the request: the module tree scores, nothing of the decoder is touched
    fused = m.score(long_ids[:20])
    gen, rows, kv = dec._alloc_gen, dec.max_seq_length, dec.kv_cache_dtype
    monkeypatch.setattr(type(dec), "prefill_ready", lambda self, idx: False)
    dec.last_prefill_plan = None
    tree = m.score(long_ids[:20])
    assert dec.last_prefill_plan is None and (dec._alloc_gen, dec.max_seq_length, dec.kv_cache_dtype) == (gen, rows, kv)
    assert tree["nll"] == pytest.approx(fused["nll"], rel=1e-2)
    with pytest.raises(ValueError, match="kv_cache_dtype='fp8': the fused model's prompt pass"):
        m.score(long_ids[:20], kv_cache_dtype="fp8")
