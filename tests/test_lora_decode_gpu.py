"""GPU: a LoRA adapter on the fused decode step and the prompt pass (Transformer.set_adapter), on the tiny random-init models of
tests/test_kv8_model_gpu.py.  (a) a zero-B adapter: logits and cache bytes BIT-EQUAL to the model without one -- every pointer the step
rewires.  (b) adapters on q, v and on q, k, v, o, down: decode logits against the module forward with W_dense + s B A in fp32 on the
dequantised weights, at test_decode_gpu.TOL (exact mode); the reference itself must move by more than twice that against no adapter.
(c) prompt pass, then decode: the greedy tokens of token-by-token decode from position 0.  (d) the refusals.  (e) the HF wrapper: load_adapter
from a state dict and from a directory, generate() on route 1 against the decoder's own token-by-token decode, and its refusals."""
import json
import os
import sys

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from guidedquant_amd.lora import LoraAdapter  # noqa: E402
from lora_decode_timing import random_peft  # noqa: E402
from test_decode_gpu import TOL, _exact_mode  # noqa: E402,F401  (autouse: the exact GEMV mode the tolerance was set under)
from test_kv8_model_gpu import _BUILD, _dev  # noqa: E402
from test_lm_head_q8_model_gpu import PROMPT, _hf  # noqa: E402

ALL = ("q_proj", "k_proj", "v_proj", "o_proj", "down_proj")
TOKS = [5, 17, 900, 3, 3, 512, 44, 1023]


def _model(kind, targets=None, **kw):
    m = _BUILD[kind]()
    m.setup_caches(1, 32)
    if targets:
        m.set_adapter(LoraAdapter.from_peft(*random_peft(m.config, targets, seed=3, **kw)))
    return m


def _step(m, t, p):
    return m.decode_native(torch.tensor([t], dtype=torch.int32, device=_dev()), torch.tensor([p], dtype=torch.int32, device=_dev()))


def _decode(m, toks):
    """token by token from position 0 on zeroed caches: (logits per step, the K and V caches afterwards)"""
    caches = [t for b in m.layers for t in (b.attention.kv_cache.k_cache, b.attention.kv_cache.v_cache)]
    for t in caches:
        t.zero_()
    out = [_step(m, t, p).clone() for p, t in enumerate(toks)]
    return out, [t.clone() for t in caches]


def _merged_forward(m, modules, toks):
    """the module forward with W_dense + s B A in fp32 on the dequantised weights of the targeted linears (LoraAdapter.modules): logits per step"""
    from guidedquant_amd.plugin import anyprec_dequant
    c, d = m.config, _dev()
    nq, nkv = c.n_head * c.head_dim, c.n_local_heads * c.head_dim
    rows = dict(q_proj=("wqkv", 0, nq), k_proj=("wqkv", nq, nq + nkv), v_proj=("wqkv", nq + nkv, nq + 2 * nkv), o_proj=("wo", 0, c.dim), down_proj=("w2", 0, c.dim))
    W = {}
    for (layer, name), (A, B, s) in modules.items():
        attr, r0, r1 = rows[name]
        mod = getattr(m.layers[layer].feed_forward if attr == "w2" else m.layers[layer].attention, attr)
        if mod not in W:
            W[mod] = anyprec_dequant(mod.qweight, mod.lut, mod.bitwidth).float()
        W[mod][r0:r1] += s * (B @ A).to(d)
    for mod, w in W.items():
        mod.forward = lambda x, w=w, mod=mod: (x.float() @ w.T).half() + (mod.bias if mod.bias is not None else 0)
    try:
        with torch.no_grad():
            return [m(torch.tensor([[t]], dtype=torch.int32, device=d), torch.tensor([p], dtype=torch.int32, device=d)).float().view(-1).clone()
                    for p, t in enumerate(toks)]
    finally:
        for mod in W:
            del mod.forward


def _greedy(m, lg, start, n=12):
    toks = []
    for p in range(start, start + n):
        toks.append(int(lg.view(-1).argmax()))
        lg = _step(m, toks[-1], p)
    return toks


@pytest.mark.parametrize("kind", ["llama-2bit", "qwen2", "window24"])
def test_zero_b_adapter_is_bit_transparent(kind):
    m = _model(kind)
    want, want_kv = _decode(m, TOKS[:4])
    m.set_adapter(LoraAdapter.from_peft(*random_peft(m.config, ALL, b_std=0.0)))
    got, got_kv = _decode(m, TOKS[:4])
    assert m._native_state().adapter is not None
    assert all(torch.equal(a, b) for a, b in zip(got + got_kv, want + want_kv))


@pytest.mark.parametrize("targets", [("q_proj", "v_proj"), ALL])
@pytest.mark.parametrize("kind", ["llama-2bit", "qwen2"])
def test_adapter_decode_matches_the_merged_module_forward(kind, targets):
    m = _model(kind)
    ad = LoraAdapter.from_peft(*random_peft(m.config, targets, seed=3, b_std=0.1))
    ref, plain = _merged_forward(m, ad.modules, TOKS), _merged_forward(m, {}, TOKS)
    m.set_adapter(ad)
    for p, (a, r, b) in enumerate(zip(_decode(m, TOKS)[0], ref, plain)):
        scale = r.abs().max().item()
        err, moved = (a.float().view(-1) - r).abs().max().item(), (b - r).abs().max().item()
        assert torch.isfinite(a).all() and err <= TOL * scale, (p, err, scale)
        assert moved > 2 * TOL * scale, (p, moved, scale)  # (a route that ignored the adapter would fail the line above)


def test_prompt_pass_then_decode_gives_the_tokens_of_token_by_token_decode():
    m, d = _model("llama-2bit", ALL, b_std=0.1), _dev()
    by_prompt = _greedy(m, m.prefill_native(torch.tensor([TOKS], dtype=torch.int32, device=d), torch.arange(len(TOKS), dtype=torch.int32, device=d)), len(TOKS))
    assert by_prompt == _greedy(m, _decode(m, TOKS)[0][-1], len(TOKS))


def test_hf_wrapper_serves_the_adapter_on_route_1_and_refuses_the_other_routes(tmp_path):
    w, kw = _hf(), dict(max_new_tokens=12, do_sample=False, pad_token_id=0)
    ids = torch.tensor([PROMPT], device=w.device)
    gen = lambda **k: w.generate(ids, **kw, **k)[0, len(PROMPT):].tolist()  # noqa: E731
    plain = gen(native=True)
    sd, cfg = random_peft(w.native_decoder().config, ALL, seed=3, b_std=0.1)
    ad = w.load_adapter(sd, cfg)
    dec = w.native_decoder()
    assert dec.adapter is ad and w.native_decoder(adapter=None).adapter is None and w.native_decoder().adapter is ad
    got = gen(native=True)
    dec.setup_caches(1, 64)
    want = _greedy(dec, _decode(dec, PROMPT)[0][-1], len(PROMPT))  # (Transformer.set_adapter's result, token by token)
    assert got == want[:len(got)] and got != plain and gen() == got
    for refused in (dict(native=False), dict(capture=True), dict(num_beams=2)):
        with pytest.raises(ValueError, match="lora: "):
            gen(**refused)
    with pytest.raises(ValueError, match="lora: "):
        w.score(ids[0], native=False)
    assert w.score(ids[0])["nll"] != _hf().score(ids[0])["nll"]
    w.set_adapter(None)
    assert gen(native=True) == plain and gen(native=False) == plain
    with open(tmp_path / "adapter_config.json", "w") as f:
        json.dump(cfg, f)
    torch.save(sd, tmp_path / "adapter_model.bin")
    w.load_adapter(str(tmp_path))
    assert gen() == got


def test_refusals(monkeypatch):
    from guidedquant_amd.pipeline import PipelinedDecoder
    from guidedquant_amd.tp import TensorParallelDecoder
    m = _model("qwen3", ("q_proj", ))
    with pytest.raises(ValueError, match="lora: q / k / v targets on a QK-norm model"):
        m._native_state()
    m.set_adapter(LoraAdapter.from_peft(*random_peft(m.config, ("o_proj", "down_proj"))))
    assert m._native_state().adapter is not None  # (o / down targets are served on Qwen3)
    with pytest.raises(NotImplementedError, match="lora: packed scoring"):
        m.score_packed_native([torch.tensor([1, 2, 3], device=_dev())])
    with pytest.raises(NotImplementedError, match="lora: tensor-parallel"):
        TensorParallelDecoder(m, None, 0, 1, 8)
    with pytest.raises(NotImplementedError, match="lora: layer-pipelined"):
        PipelinedDecoder(m, 0, 1, range(2))
    m.setup_caches(1, 32, kv_cache_dtype="fp8")
    with pytest.raises(NotImplementedError, match="lora: the fp8 KV cache"):
        m._native_state()
    monkeypatch.setenv("GQ_NATIVE_PAIRS", "0")
    with pytest.raises(ValueError, match="lora: a down_proj target needs the paired gate / up rows"):
        _model("llama-2bit", ("down_proj", ))._native_state()
