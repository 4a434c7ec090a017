"""GPU: the fused route (`prefill_native`, `decode_native`, `score`, `generate`) over an mxfp4 cache against the module forward over the SAME
kind of cache (`KVCache(mxfp4=True)`: stores by `mxfp4_quantize`, hands back `mxfp4_dequant`), on the tiny Llama and Qwen3-style models and
with the criterion and the bounds of test_kv8r_model_gpu.py: both sides dequantise exactly, so the format adds no error between them.
Layer 0's cache bytes behind the prompt pass equal `mxfp4_quantize` of the rows the fused route leaves in an fp16 cache.
Measured on MI355X: 4.8e-3 / 5.2e-3 at the most (bounds 1e-2 / 9.48e-3).  The SDPA prompt route (GQ_PREFILL_ATTN=0) runs as ONE piece: in
chunks of 32 torch's SDPA itself differs from the whole-sequence call of the module forward enough to move layer 1's rows across rounding
boundaries (13 + 17 of its cache bytes differ, against 1 + 1 in one piece; an fp8_row cache: 187 + 173 against 2 + 6), the two sides no
longer see the same cache values, and one e2m1 step is a quarter to a half of the element: 4.35e-2 / 1.24e-2 there, 4.3e-3 / 1.3e-3 in one
piece.  Layer 0's bytes are equal in every mode."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_kv8_model_gpu as t8  # noqa: E402
from test_kv8r_model_gpu import E_BOUND, R_BOUND  # noqa: E402

KINDS = ["llama-2bit", "qwen3", "window24"]
_models = {}


def _model(kind):
    """the model with an mxfp4 cache, and layer 0's fp16 cache rows behind the fused fp16 prompt pass over the S = 70 inputs"""
    if kind not in _models:
        m = t8._BUILD[kind]()
        m.setup_caches(1, t8.CACHE)
        idx, pos = t8._inputs(m, 70)
        with torch.no_grad():
            m.prefill_native(idx[:, :70], pos[:70], start=0, last_only=False, chunk=t8.CHUNK)
        kc = m.layers[0].attention.kv_cache
        rows16 = kc.k_cache[:, :, :70].clone(), kc.v_cache[:, :, :70].clone()
        m.setup_caches(1, t8.CACHE, kv_cache_dtype="mxfp4")
        kc, hd = m.layers[0].attention.kv_cache, m.config.head_dim
        assert m.kv_cache_dtype == "mxfp4" and m.native_ready() and m.kv8_unserved() is None
        assert kc.k_cache.dtype == torch.uint8 and kc.k_cache.shape == (1, 2, t8.CACHE, hd // 2) and kc.v_exp.shape == (1, 2, t8.CACHE, hd // 32)
        _models[kind] = (m, rows16)
    return _models[kind]


def _clear(m):
    for b in m.layers:
        kc = b.attention.kv_cache
        kc.k_cache.zero_(), kc.v_cache.zero_(), kc.k_exp.fill_(127), kc.v_exp.fill_(127)


def _close(got, want, what):
    e, r = t8._dev_of(got, want)
    print("%s: element-wise %.3e  norm-wise %.3e   (bounds %.3e / %.3e)" % (what, e, r, E_BOUND, R_BOUND))
    assert torch.isfinite(got).all()
    assert e <= E_BOUND and r <= R_BOUND, (what, e, r)


def _run(m, kind, S, plan, chunk=t8.CHUNK):
    """prompt pass against the module forward, then 8 decode steps step by step over the same history; rows >= S + 8 untouched"""
    idx, pos = t8._inputs(m, S)
    _clear(m)
    with torch.no_grad():
        want = m(idx[:, :S], pos[:S]).float().clone()
    _clear(m)
    with torch.no_grad():
        got = m.prefill_native(idx[:, :S], pos[:S], start=0, last_only=False, chunk=chunk).float().clone()
    assert m.last_prefill_plan["attn"] == [plan] * len(m.layers)
    _close(got, want, "%s %s prompt S=%d" % (kind, plan, S))
    for t in range(S, S + 8):  # the module forward first, then the fused step over the same rows < t (each writes row t itself)
        with torch.no_grad():
            want = m(idx[:, t:t + 1], pos[t:t + 1]).float().clone()
            got = m.decode_native(idx[0, t:t + 1], pos[t:t + 1]).float().clone()
        _close(got.view(-1), want.view(-1), "%s step %d" % (kind, t))
    for b in m.layers:
        kc = b.attention.kv_cache
        assert bool((kc.k_cache[:, :, S + 8:] == 0).all()) and bool((kc.v_exp[:, :, S + 8:] == 127).all()), "rows behind the steps were written"
        assert bool((kc.k_exp[:, :, :S + 8] != 127).any())


@pytest.mark.parametrize("kind", KINDS)
def test_fused_route_matches_the_module_forward_over_an_mxfp4_cache(kind, monkeypatch):
    from guidedquant_amd.model import mxfp4_quantize
    monkeypatch.delenv("GQ_PREFILL_ATTN", raising=False)
    m, rows16 = _model(kind)
    _run(m, kind, 70, "hip-mx4")
    idx, pos = t8._inputs(m, 70)
    _clear(m)
    with torch.no_grad():
        m.prefill_native(idx[:, :70], pos[:70], start=0, last_only=False, chunk=t8.CHUNK)
    kc = m.layers[0].attention.kv_cache
    for name, cache, exp, r16 in (("k", kc.k_cache, kc.k_exp, rows16[0]), ("v", kc.v_cache, kc.v_exp, rows16[1])):
        codes, byte = mxfp4_quantize(r16)
        assert torch.equal(cache[:, :, :70], codes) and torch.equal(exp[:, :, :70], byte), name + ": layer 0's cache bytes are not the host rule's"
    _run(m, kind, 17, "hip-mx4")
    if kind == "window24":  # the prompt attention as SDPA on the dequantised rows, one piece (the docstring says why)
        monkeypatch.setenv("GQ_PREFILL_ATTN", "0")
        _run(m, kind, 70, "sdpa-mx4", chunk=t8.CACHE)


def test_generate_and_score_with_an_mxfp4_cache_and_the_refusals(monkeypatch):
    monkeypatch.delenv("GQ_PREFILL_ATTN", raising=False)
    m = t8._hf_tiny()
    d = m.device
    ids = torch.randint(0, 512, (1, 20), device=d, generator=torch.Generator(device=d).manual_seed(3))
    plain = m.generate(ids, max_new_tokens=12, do_sample=False, pad_token_id=0)
    dec = m._native_cache[("decoder", 2)]
    out = m.generate(ids, max_new_tokens=12, do_sample=False, pad_token_id=0, kv_cache_dtype="mxfp4")
    assert out.shape == (1, 32) and torch.equal(out[:, :20], ids)
    assert dec.kv_cache_dtype == "mxfp4" and dec.last_prefill_plan["attn"] == ["hip-mx4"] * len(dec.layers)
    ids32 = ids.view(-1).to(torch.int32)
    # score(): the log-probabilities of the fused prompt pass against the module forward's over the same kind of cache
    got = m.score(ids.view(-1), kv_cache_dtype="mxfp4")
    assert dec.kv_cache_dtype == "mxfp4" and dec.last_prefill_plan["attn"] == ["hip-mx4"] * len(dec.layers)
    _clear(dec)
    with torch.no_grad():
        logits = dec(ids32[:20].view(1, -1), torch.arange(20, device=d, dtype=torch.int32)).float()[0]
    want = torch.log_softmax(logits[:-1], -1).gather(1, ids.view(-1, 1)[1:]).view(-1)
    _close(got["logprobs"].to(d).float(), want, "score")
    # the refusals: packed scoring, an adapter; then a plain generate: an fp16 cache again, and the tokens it gave before
    with pytest.raises(NotImplementedError, match="packed scoring: mxfp4 KV cache"):
        dec.score_packed_native([ids32[:5], ids32[5:9]])
    m._adapter = object()  # (any adapter: the refusal comes before it is looked at)
    with pytest.raises(ValueError, match="lora: the adapter is served by the fused decode model with an fp16 cache only"):
        m.score(ids.view(-1), kv_cache_dtype="mxfp4")
    m._adapter = None
    again = m.generate(ids, max_new_tokens=12, do_sample=False, pad_token_id=0)
    assert dec.kv_cache_dtype == "fp16" and dec.layers[0].attention.kv_cache.k_cache.dtype == torch.float16 and torch.equal(again, plain)
