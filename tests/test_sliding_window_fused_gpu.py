"""GPU, model level: Any-Precision checkpoints with sliding-window layers (Mistral as published: every layer; Qwen2 with use_sliding_window:
the layers from max_window_layers on, the q / k / v bias form; Qwen3 through layer_types, the QK-norm form) on the fused HIP route -- the
plain `generate()` lands there, agrees with transformers' own module tree, the prompt pass masks a prompt longer than the window, the
window shows in the logits, a captured DecodeGraph replays the eager step across pos = W, and what has no window form (tensor-parallel and
layer-pipelined decode) declines.  The sibling of tests/test_qwen2_fused_gpu.py / test_qwen3_fused_gpu.py, with their bounds.

Seed and prompt: chosen on fp32 module trees of the same geometry on the CPU (weights N(0, 0.02), embeddings x 25, lm_head x 10, seed 5, the
prompt below), where removing the window moves the last prompt position's logits norm-wise by 1.5e-1 (Mistral, 64 and 128), 4.7e-2 (Qwen2)
and 1.6e-1 (Qwen3) -- well beyond the 2 x 5e-3 the test below asks for."""
import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
pytestmark = pytest.mark.gpu

TOL = 2e-2  # of max|logit|: tests/test_decode_default_gpu.py:16
W = 16
_NAMES = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]
PROMPT = [61, 360, 442, 138, 452, 242, 45, 291, 207, 359, 237, 441, 13, 290, 35, 72, 292, 105, 86, 384, 461, 117, 150, 311, 17, 33, 40, 313, 505, 56,
          314, 393, 126, 16, 255, 110, 430, 59, 395, 117]  # 40 tokens: longer than W, the prompt pass needs the mask
_COMMON = dict(hidden_size=512, intermediate_size=1024, num_hidden_layers=3, num_key_value_heads=2, vocab_size=512, max_position_embeddings=256,
               rms_norm_eps=1e-6, tie_word_embeddings=False)
CASES = [("mistral", 64), ("mistral", 128), ("qwen2", 64), ("qwen3", 128)]


def _mode(m):
    from guidedquant_amd import _lib
    _lib.check(_lib.lib().gq_set_ap_mode(m), "gq_set_ap_mode")


@pytest.fixture(autouse=True)
def _restore():
    yield
    _mode(-1)


def _config(kind, hd, window=True):
    """the configuration, and its twin without the window (same tensors: nothing of the window is a weight)"""
    heads = 512 // hd
    if kind == "mistral":  # every layer
        return transformers.MistralConfig(sliding_window=W if window else None, head_dim=hd, num_attention_heads=heads, **_COMMON), (W, W, W)
    if kind == "qwen2":  # mixed layers, the bias form
        return transformers.Qwen2Config(use_sliding_window=window, sliding_window=W, max_window_layers=1, num_attention_heads=heads, **_COMMON), (None, W, W)
    lt = ["full_attention", "sliding_attention", "sliding_attention"] if window else ["full_attention"] * 3
    return transformers.Qwen3Config(layer_types=lt, sliding_window=W if window else None, use_sliding_window=window, head_dim=hd,
                                    num_attention_heads=heads, **_COMMON), (None, W, W)


def _hf_model(cfg, seed=5):
    """`test_qwen2_fused_gpu._hf_model`: 2-bit planes only, embeddings x 25 and lm_head x 10 for margins, seeded q / k / v biases of std 1
    where the tree has them"""
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    cfg.anyprec = dict(seed_precision=2, parent_precision=2, group_count=1, arch_config=dict(module_names=_NAMES, model_name="model", layers_name="layers"))
    m = AnyPrecisionForCausalLM.from_config_random(cfg, device=torch.device("cuda:0"), seed=seed)
    g = torch.Generator(device=m.device)
    g.manual_seed(seed + 1)
    with torch.no_grad():
        m.model.model.embed_tokens.weight.mul_(25.0)
        m.model.lm_head.weight.mul_(10.0)
        for layer in m.get_model_layers():
            for n in ("q_proj", "k_proj", "v_proj"):
                b = getattr(layer.self_attn, n).bias
                if b is not None:
                    b.copy_(torch.randn(b.shape, device=m.device, generator=g).half())
    return m


@pytest.mark.parametrize("kind,hd", CASES, ids=["%s-hd%d" % c for c in CASES])
def test_plain_generate_of_a_sliding_window_checkpoint_takes_the_fused_route(kind, hd):
    cfg, windows = _config(kind, hd)
    m = _hf_model(cfg)
    d = m.device
    ids = torch.tensor([PROMPT], device=d)
    T = ids.shape[1]
    assert T > W
    eager = m.generate(ids, max_new_tokens=24, do_sample=False, native=False, pad_token_id=0)
    fused = m.generate(ids, max_new_tokens=24, do_sample=False, pad_token_id=0)
    assert ("decoder", 2) in m._native_cache and fused.shape == eager.shape == (1, T + 24) and fused.dtype == ids.dtype
    dec = m._native_cache[("decoder", 2)]
    assert dec.config.layer_windows == windows and dec.config.head_dim == hd and dec.native_ready()
    assert dec.config.attn_bias == (kind == "qwen2") and dec.config.qk_norm == (kind == "qwen3")
    st = dec._native_state()
    assert st.layer_window == list(windows) and dec.max_seq_length > W
    agree = float((fused[0, T:] == eager[0, T:]).float().mean())
    print("%s head_dim %d: agreement %.3f" % (kind, hd, agree))
    assert torch.equal(fused[0, :T + 1], eager[0, :T + 1]) and agree >= 0.8, (agree, fused, eager)  # the Llama criterion, test_hf_routes_gpu.py:114-115
    # logits of the last prompt position: the HIP prompt pass (T > W: the explicit mask) and a decode step behind it (the window launch),
    # against transformers' module tree
    with torch.no_grad():
        want = m.model(ids).logits[0, -1].float()
        ids32 = ids.view(-1).to(torch.int32)
        assert dec.prefill_ready(ids32)
        got_p = dec.prefill_native(ids32, torch.arange(T, device=d, dtype=torch.int32), start=0).float().view(-1).clone()
        dec.prefill_native(ids32[:T - 1], torch.arange(T - 1, device=d, dtype=torch.int32), start=0)
        got_d = dec.decode_native(ids32[T - 1:], torch.tensor([T - 1], device=d, dtype=torch.int32)).float().view(-1).clone()
    torch.cuda.synchronize()
    scale = want.abs().max().item()
    for name, got in (("prefill_native", got_p), ("decode_native", got_d)):
        err, rel = (got - want).abs().max().item(), ((got - want).norm() / want.norm()).item()
        print("%s head_dim %d %s: max|logit| %.3f  element-wise %.3e  norm-wise %.3e" % (kind, hd, name, scale, err, rel))
        assert torch.isfinite(got).all()
        assert err <= TOL * scale, (name, err, scale)
        assert rel <= 5e-3, (name, rel)
    # and the window is in it: the module tree of the same weights without the window leaves the fused logits by more than twice what the
    # windowed tree is allowed
    del dec, st
    m._drop_native()
    twin = _hf_model(_config(kind, hd, window=False)[0])
    a, b = m.get_model_layers()[1].self_attn.q_proj, twin.get_model_layers()[1].self_attn.q_proj
    assert torch.equal(a.qweight, b.qweight) and torch.equal(m.model.lm_head.weight, twin.model.lm_head.weight)
    with torch.no_grad():
        full = twin.model(ids).logits[0, -1].float()
    for name, got in (("prefill_native", got_p), ("decode_native", got_d)):
        moved = ((got - full).norm() / full.norm()).item()
        print("%s head_dim %d %s: against the tree without the window norm-wise %.3e" % (kind, hd, name, moved))
        assert moved > 2 * 5e-3, (name, moved)


def test_decode_graph_replay_equals_the_eager_step_across_the_window():
    """positions 0 .. 23 with W = 16: the window starts to bite inside the captured steps"""
    from guidedquant_amd.generate import DecodeGraph
    m = _hf_model(_config("mistral", 128)[0], seed=7)
    d = m.device
    dec = m.native_decoder(2)
    dec.setup_caches(1, 64)
    assert dec.native_ready() and dec.config.layer_windows == (W, W, W) and dec._native_state().layer_window == [W, W, W]
    n = 24
    eager, t = [], 3
    with torch.no_grad():
        for p in range(n):
            lg = dec.decode_native(torch.tensor([t], dtype=torch.int32, device=d), torch.tensor([p], dtype=torch.int32, device=d))
            t = int(lg.float().view(-1).argmax().item())
            eager.append(t)
    for b in dec.layers:
        b.attention.kv_cache.k_cache.zero_()
        b.attention.kv_cache.v_cache.zero_()
    g = DecodeGraph(dec, d, native_sampling=True, temperature=0.0, top_k=32, seq_capacity=65, steps_per_replay=1)
    g.set_token(3, 0)
    for _ in range(n):
        g.step()
    torch.cuda.synchronize()
    assert g.seq[1:n + 1].tolist() == eager and int(g.pos.item()) == n
    assert len(set(eager)) > 4  # not a fixed point
    g.close() if hasattr(g, "close") else None


def test_a_windowed_layer_launches_the_window_entry_and_the_others_what_they_did(monkeypatch):
    """Qwen2, layers (None, W, W): layer 0 launches gq_attn_decode_split_bias with the arguments it always had, layers 1 and 2 the _window
    entry with W in front of the stream"""
    from guidedquant_amd import _lib
    m = _hf_model(_config("qwen2", 64)[0])
    d = m.device
    dec = m.native_decoder(2)
    dec.setup_caches(1, 64)
    L = _lib.lib()
    calls = []
    for name in ("gq_attn_decode_split_bias", "gq_attn_decode_split_bias_window", "gq_attn_decode_split", "gq_attn_decode_split_window",
                 "gq_attn_decode_roped", "gq_attn_decode_roped_window"):
        real = getattr(L, name)
        monkeypatch.setattr(L, name, lambda *a, _n=name, _r=real: (calls.append((_n, a)), _r(*a))[1])
    with torch.no_grad():
        dec.decode_native(torch.tensor([3], dtype=torch.int32, device=d), torch.tensor([0], dtype=torch.int32, device=d))
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert [c[0] for c in calls] == ["gq_attn_decode_split_bias", "gq_attn_decode_split_bias_window", "gq_attn_decode_split_bias_window"]
    assert len(calls[0][1]) == 16 and len(calls[1][1]) == 17 and calls[1][1][-2] == W and calls[2][1][-2] == W
    assert calls[1][1][7:14] == calls[0][1][7:14]  # heads, head_dim, max_seq, scale, n_split, workspace


def test_what_has_no_window_form_is_declined():
    from guidedquant_amd.pipeline import PipelinedDecoder
    from guidedquant_amd.tp import TensorParallelDecoder
    m = _hf_model(_config("mistral", 64)[0])
    dec = m.native_decoder(2)
    assert dec.config.layer_windows == (W, W, W)
    with pytest.raises(NotImplementedError, match="sliding-window"):
        TensorParallelDecoder(dec, None, 0, 2, 8)
    with pytest.raises(NotImplementedError, match="sliding-window"):
        PipelinedDecoder(dec, 0, 1, range(3))
