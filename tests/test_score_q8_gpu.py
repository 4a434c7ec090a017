"""GPU: scoring through the int8 lm_head -- `Transformer.score_native(lm_head_dtype="int8")` (gq_head_nll_i8 / gq_head_nll_i8_topn, or the
torch form native_prompt.logits_q8) and `AnyPrecisionForCausalLM.score(..., lm_head_dtype="int8")` -- on tiny random-init fused models
(Llama geometry, dim 512, 2 layers; V = 1000 and 500: no multiple of the kernel's 128-row tile; S = 131 rows: two row tiles).

The reference is a float64 head on the fp16 rows norm(x) of the same pass (taken at the model's final norm during prefill_native):
logit = fp16(sum_k xn[k] q[v][k] scale[v]), then tests/head_nll_model.py.  The rule of every comparison is the round-off family's
(tests/test_head_nll_gpu.py): |dlogprob| <= 2 ulp16(max |logit| of the row), greedy flags on the rows whose top-two gap is at least that.
Every pass runs under GQ_PREFILL_ATTN=1, so that a chunked pass and a one-piece pass differ in the chunking alone.
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


def _reference(m, idx):
    """(logprob f64 [n - 1], row tolerance, rows with a clear top1, greedy) of the int8 head on the rows norm(x) of a one-piece pass"""
    n, rows = idx.numel(), []
    hook = m.norm.register_forward_hook(lambda mod, args, out: rows.append(out.detach()))
    try:
        with torch.no_grad():
            m.prefill_native(idx.view(1, -1), torch.arange(n, dtype=torch.int32, device=idx.device), start=0, last_only=False)
    finally:
        hook.remove()
    xn = rows[-1].reshape(n, -1)[:n - 1].cpu().numpy()
    q, scale = m.head_q8()
    l64 = hm.logits16(xn, q.cpu().numpy().astype(np.float64) * scale.cpu().numpy().astype(np.float64)[:, None])
    t = idx[1:].cpu().numpy()
    _, lp, top1 = hm.model(l64, t)
    srt = np.sort(l64, axis=1)
    return lp, 2.0 * hm.ulp16(np.abs(l64).max(axis=1)), (srt[:, -1] - srt[:, -2]) >= 2.0 * hm.ulp16(srt[:, -1]), top1 == t


_cache = {}


def _model():
    if not _cache:
        from guidedquant_amd.APLinear import APLinear
        from guidedquant_amd.generate import random_init_
        from guidedquant_amd.model import ModelArgs, Transformer
        d = _dev()
        cfg = ModelArgs(block_size=CACHE, vocab_size=1000, n_layer=2, n_head=8, dim=512, intermediate_size=1024, n_local_heads=2, rope_base=500000,
                        model_name="llama-test")
        m = Transformer(torch.float16, cfg, linear_class=APLinear, linear_kwargs=dict(bitwidth=2, device=d)).to(device=d, dtype=torch.float16).eval()
        random_init_(m, seed=2, lut_std=0.05)
        m.setup_caches(1, CACHE)
        idx = torch.randint(0, cfg.vocab_size, (S, ), dtype=torch.int32, device=d, generator=torch.Generator(device=d).manual_seed(7))
        _cache["m"] = (m, idx)
    return _cache["m"]


@pytest.mark.parametrize("top", [None, 5])
@pytest.mark.parametrize("chunk", [None, 48])
def test_kernel_head_and_torch_head_against_the_float64_head(chunk, top, monkeypatch):
    monkeypatch.setenv("GQ_PREFILL_ATTN", "1")
    monkeypatch.setenv("GQ_SCORE_HEAD", "1")
    m, idx = _model()
    with pytest.raises(ValueError, match="^lm_head_dtype='int8': "):
        m.score_native(idx, lm_head_dtype="int8")  # (the model is still at fp16)
    with torch.no_grad():
        fp16 = m.score_native(idx, chunk=chunk)[0].double().cpu().numpy()
    m.set_lm_head_dtype("int8")
    try:
        if "ref" not in _cache:
            _cache["ref"] = _reference(m, idx)
        want, tol, clear, greedy = _cache["ref"]
        assert clear.mean() >= 0.9
        for head, name in (("1", "hip-nll-i8-topn" if top else "hip-nll-i8"), ("0", "torch-i8")):
            monkeypatch.setenv("GQ_SCORE_HEAD", head)
            with torch.no_grad():
                lp, g, *lists = m.score_native(idx, chunk=chunk, top_logprobs=top, lm_head_dtype="int8")
                assert m.last_prefill_plan["head"] == name and len(m.last_prefill_plan["chunks"]) == (1 if chunk is None else 3)
                again = m.score_native(idx, chunk=chunk)[0].double().cpu().numpy()  # (no keyword: the fp16 head, on an int8 model too)
            got = lp.double().cpu().numpy()
            d = np.abs(got - want)
            print("head %s chunk %s top %s: worst |dlogprob| / (2 ulp16) %.3f" % (name, chunk, top, (d / tol).max()))
            assert (d <= tol).all(), (name, (d / tol).max())
            assert np.array_equal(g.cpu().numpy()[clear], greedy[clear])
            assert (got != fp16).any() and (head == "0" or np.array_equal(again, fp16))
            if top:
                ids, lps = lists
                assert ids.shape == (S - 1, top) and lps.shape == (S - 1, top) and bool((lps[:, :-1] >= lps[:, 1:]).all())
                hit = (ids == idx[1:, None].long()).cpu().numpy()  # (where the target is listed, its entry is its logprob)
                assert hit.any() and (np.abs(lps.double().cpu().numpy()[hit] - want[hit.any(axis=1)]) <= tol[hit.any(axis=1)]).all()
    finally:
        m.set_lm_head_dtype("fp16")


def test_score_api_requests_the_head(monkeypatch):
    transformers = pytest.importorskip("transformers")
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    monkeypatch.setenv("GQ_PREFILL_ATTN", "1")
    monkeypatch.setenv("GQ_SCORE_HEAD", "1")
    hf = transformers.LlamaConfig(hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=2,
                                  vocab_size=500, max_position_embeddings=512, rms_norm_eps=1e-5, tie_word_embeddings=False)
    names = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]
    hf.anyprec = dict(seed_precision=2, parent_precision=2, group_count=1, arch_config=dict(module_names=names, model_name="model", layers_name="layers"))
    m = AnyPrecisionForCausalLM.from_config_random(hf, device=_dev(), seed=5)
    with torch.no_grad():
        m.model.model.embed_tokens.weight.mul_(25.0)
        m.model.lm_head.weight.mul_(10.0)
    d = m.device
    ids = torch.randint(0, 500, (40, ), device=d, generator=torch.Generator(device=d).manual_seed(3))
    before = m.score(ids)
    dec = m._native_cache[("decoder", 2)]
    assert dec.last_prefill_plan["head"] == "hip-nll" and dec.lm_head_dtype == "fp16"
    r = m.score(ids, lm_head_dtype="int8", top_logprobs=5)
    assert dec.last_prefill_plan["head"] == "hip-nll-i8-topn" and dec.lm_head_dtype == "int8" and r["top_logprobs"].shape == (39, 5)
    want, tol, _, _ = _reference(dec, ids.to(torch.int32))
    got = r["logprobs"].double().cpu().numpy()
    assert (np.abs(got - want) <= tol).all() and (got != before["logprobs"].double().cpu().numpy()).any()
    k = 7
    ll, _ = m.loglikelihood(ids[:-k], ids[-k:], lm_head_dtype="int8")
    (ll_many, _), = m.loglikelihood_many([(ids[:-k], ids[-k:])], lm_head_dtype="int8")
    assert dec.last_prefill_plan["head"] == "hip-nll-i8"
    assert abs(ll - want[-k:].sum()) <= tol[-k:].sum() and abs(ll_many - want[-k:].sum()) <= tol[-k:].sum(), (ll, ll_many, want[-k:].sum())
    after = m.score(ids)  # (no keyword: the fp16 head again, whatever the request before left on the decoder)
    assert dec.last_prefill_plan["head"] == "hip-nll" and dec.lm_head_dtype == "fp16"
    assert torch.equal(after["logprobs"], before["logprobs"]) and torch.equal(after["greedy"], before["greedy"])
    with pytest.raises(ValueError, match="^lm_head_dtype='int8': "):
        m.score(ids, lm_head_dtype="int8", native=False)
