"""GPU: the fused route (`prefill_native`, `decode_native`, `generate`) over an fp8_row cache against the module forward over the SAME cache, on
the six tiny models and with the criterion of test_kv8_model_gpu.py.  Both sides dequantise exactly: the bounds are that file's for scales
1.0, max(1e-2, 2 x 4.74e-3) / max(3e-3, 2 x 4.74e-3); measured on MI355X 6.77e-3 / 6.79e-3 at the most."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_kv8_model_gpu as t8  # noqa: E402

E_BOUND, R_BOUND = max(1e-2, 2 * 4.74e-3), max(3e-3, 2 * 4.74e-3)
_models = {}
_worst = [0.0, 0.0]


def _model(kind):
    """the model with an fp8_row cache, and the fp16-cache module forward's logits on the S = 70 inputs (taken before the switch)"""
    if kind not in _models:
        m = t8._BUILD[kind]()
        m.setup_caches(1, t8.CACHE)
        idx, pos = t8._inputs(m, 70)
        with torch.no_grad():
            ref16 = m(idx[:, :70], pos[:70]).float().clone()
        m.setup_caches(1, t8.CACHE, kv_cache_dtype="fp8_row")
        kc = m.layers[0].attention.kv_cache
        assert m.kv_cache_dtype == "fp8_row" and m.native_ready() and kc.k_cache.dtype == torch.float8_e4m3fn and kc.k_exp.shape == (1, 2, t8.CACHE)
        _models[kind] = (m, ref16)
    return _models[kind]


def _clear(m):
    for b in m.layers:
        kc = b.attention.kv_cache
        kc.k_cache.view(torch.uint8).zero_(), kc.v_cache.view(torch.uint8).zero_(), kc.k_exp.fill_(127), kc.v_exp.fill_(127)


def _close(got, want, what):
    e, r = t8._dev_of(got, want)
    _worst[0], _worst[1] = max(_worst[0], e), max(_worst[1], r)
    print("%s: element-wise %.3e  norm-wise %.3e   (bounds %.3e / %.3e; worst so far %.3e / %.3e)" % (what, e, r, E_BOUND, R_BOUND, _worst[0], _worst[1]))
    assert torch.isfinite(got).all()
    assert e <= E_BOUND and r <= R_BOUND, (what, e, r)


def _run(m, kind, S, plan):
    """prompt pass against the module forward, rows >= S untouched, then 8 decode steps step by step over the same history"""
    idx, pos = t8._inputs(m, S)
    _clear(m)
    with torch.no_grad():
        want = m(idx[:, :S], pos[:S]).float().clone()
    _clear(m)
    with torch.no_grad():
        got = m.prefill_native(idx[:, :S], pos[:S], start=0, last_only=False, chunk=t8.CHUNK).float().clone()
    assert m.last_prefill_plan["attn"] == [plan] * len(m.layers)
    _close(got, want, "%s %s prompt S=%d" % (kind, plan, S))
    for t in range(S, S + 8):  # the module forward first, then the fused step over the same rows < t (each writes row t itself)
        with torch.no_grad():
            want = m(idx[:, t:t + 1], pos[t:t + 1]).float().clone()
            got = m.decode_native(idx[0, t:t + 1], pos[t:t + 1]).float().clone()
        _close(got.view(-1), want.view(-1), "%s step %d" % (kind, t))
    for b in m.layers:
        kc = b.attention.kv_cache
        assert bool((kc.k_cache.view(torch.uint8)[:, :, S + 8:] == 0).all()) and bool((kc.v_exp[:, :, S + 8:] == 127).all()), "rows behind the steps were written"
        assert bool((kc.k_exp[:, :, :S + 8] != 127).any())


@pytest.mark.parametrize("kind", list(t8._BUILD))
def test_fused_route_matches_the_module_forward_over_an_fp8_row_cache(kind, monkeypatch):
    monkeypatch.delenv("GQ_PREFILL_ATTN", raising=False)
    m, ref16 = _model(kind)
    idx, pos = t8._inputs(m, 70)
    _clear(m)
    with torch.no_grad():
        ref8 = m(idx[:, :70], pos[:70]).float()
    e16, r16 = t8._dev_of(ref8, ref16)
    print("%s: fp8_row-cache vs fp16-cache module forward: element-wise %.3e  norm-wise %.3e" % (kind, e16, r16))
    assert E_BOUND < 0.5 * e16 and R_BOUND < 0.5 * r16, (e16, r16)
    _run(m, kind, 70, "hip-kv8r")
    _run(m, kind, 17, "hip-kv8r")
    if kind == "window24":  # the prompt attention as SDPA on the dequantised rows
        monkeypatch.setenv("GQ_PREFILL_ATTN", "0")
        _run(m, kind, 70, "sdpa-kv8r")


def test_generate_with_an_fp8_row_cache_and_back(monkeypatch):
    monkeypatch.delenv("GQ_PREFILL_ATTN", raising=False)
    m = t8._hf_tiny()
    d = m.device
    ids = torch.randint(0, 512, (1, 20), device=d, generator=torch.Generator(device=d).manual_seed(3))
    plain = m.generate(ids, max_new_tokens=12, do_sample=False, pad_token_id=0)
    dec = m._native_cache[("decoder", 2)]
    out = m.generate(ids, max_new_tokens=12, do_sample=False, pad_token_id=0, kv_cache_dtype="fp8_row")
    assert out.shape == (1, 32) and torch.equal(out[:, :20], ids)
    assert dec.kv_cache_dtype == "fp8_row" and dec.layers[0].attention.kv_cache.k_exp.dtype == torch.uint8
    assert dec.last_prefill_plan["attn"] == ["hip-kv8r"] * len(dec.layers)
    # the same 12 tokens by hand: the prompt but for its last token through the prompt pass, then greedy decode_native steps
    ids32 = ids.view(-1).to(torch.int32)
    _clear(dec)
    with torch.no_grad():
        dec.prefill_native(ids32[:19], torch.arange(19, device=d, dtype=torch.int32), start=0)
        tok, hand = ids32[19:20], []
        for t in range(19, 31):
            logits = dec.decode_native(tok, torch.tensor([t], dtype=torch.int32, device=d))
            tok = logits.view(-1).float().argmax().to(torch.int32).view(1)
            hand.append(int(tok))
    assert out[0, 20:].tolist() == hand
    # a plain generate afterwards: an fp16 cache again, and the tokens it gave before
    again = m.generate(ids, max_new_tokens=12, do_sample=False, pad_token_id=0)
    assert dec.kv_cache_dtype == "fp16" and dec.layers[0].attention.kv_cache.k_cache.dtype == torch.float16 and torch.equal(again, plain)
