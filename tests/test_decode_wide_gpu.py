"""GPU: the fused decode model at 5 to 8 bits.  A two-layer Transformer of APLinear modules at those widths is native_ready(); its fused
step (every GEMV on ap_wide.hip's kernel) matches the torch forward, and a captured DecodeGraph gives the eager step's greedy tokens.
An Any-Precision checkpoint with an 8-bit parent serves generate(precision=5..8, native=True) on the fused route, with the tokens of
the module tree; its planes are released only at the parent's own precision, and they come back whole."""
import pytest

import test_decode_gpu as dg

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=[1, -1], ids=["exact", "default"])
def _mode(request):
    from guidedquant_amd import _lib
    _lib.check(_lib.lib().gq_set_ap_mode(request.param), "gq_set_ap_mode")
    yield
    _lib.lib().gq_set_ap_mode(-1)


def _clear_caches(m):
    for b in m.layers:
        b.attention.kv_cache.k_cache.zero_()
        b.attention.kv_cache.v_cache.zero_()


@pytest.mark.parametrize("bits", [5, 6, 7, 8])
def test_decode_native_matches_torch_forward_and_the_graph(bits):
    from guidedquant_amd.generate import DecodeGraph
    d = torch.device("cuda:0")
    m = dg._tiny_model(bits, 64)
    m.setup_caches(1, 32)
    assert m.native_ready()
    toks = [5, 17, 900, 3, 3, 512, 44, 1023]
    pos = lambda p: torch.tensor([p], dtype=torch.int32, device=d)  # noqa: E731
    with torch.no_grad():
        ref = [m(torch.tensor([[t]], dtype=torch.int32, device=d), pos(p)).float().view(-1) for p, t in enumerate(toks)]
        _clear_caches(m)
        for p, t in enumerate(toks):
            a = m.decode_native(torch.tensor([t], dtype=torch.int32, device=d), pos(p)).float().view(-1)
            torch.cuda.synchronize()
            scale = ref[p].abs().max().item()
            assert torch.isfinite(a).all()
            assert (a - ref[p]).abs().max().item() <= dg.TOL * scale, (p, (a - ref[p]).abs().max().item(), scale)
        # greedy tokens of the eager fused step from token 1 at position 0 ..
        _clear_caches(m)
        eager, t = [], 1
        for p in range(12):
            t = int(m.decode_native(torch.tensor([t], dtype=torch.int32, device=d), pos(p)).float().view(-1).argmax().item())
            eager.append(t)
    # .. are the captured graph's
    _clear_caches(m)
    g = DecodeGraph(m, d, native_sampling=True, temperature=0.0, top_k=32, seq_capacity=33)
    g.set_token(1, 0)
    got = []
    for _ in range(12):
        g.step()
        got.append(int(g.next_tok.item()))
    g.close()
    assert got == eager


def _parent8_model(seed=3, D=512, I=1024, H=8, KV=2, V=512, Lr=3):
    """a random Any-Precision checkpoint with a 3-bit seed and an 8-bit parent (the reference's default), with logit margins as
    tests/test_hf_routes_gpu.py::_single_precision_model gives them"""
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    hf = transformers.LlamaConfig(hidden_size=D, intermediate_size=I, num_hidden_layers=Lr, num_attention_heads=H, num_key_value_heads=KV,
                                  vocab_size=V, max_position_embeddings=256, rms_norm_eps=1e-5, tie_word_embeddings=False)
    names = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]
    hf.anyprec = dict(seed_precision=3, parent_precision=8, group_count=1, arch_config=dict(module_names=names, model_name="model", layers_name="layers"))
    m = AnyPrecisionForCausalLM.from_config_random(hf, device=torch.device("cuda:0"), seed=seed)
    with torch.no_grad():
        m.model.model.embed_tokens.weight.mul_(25.0)
        m.model.lm_head.weight.mul_(10.0)
    return m


def test_parent8_generate_at_5_to_8_bits_on_the_fused_route():
    m = _parent8_model()
    ids = torch.tensor([[3, 17, 5, 60, 2, 9]], device=m.device)
    l0 = m.get_model_layers()[0]
    planes = {k: v.clone() for k, v in m.model.state_dict().items() if k.endswith("qweight")}
    assert planes["model.layers.0.mlp.gate_proj.qweight"].shape[0] == 8
    for b in (5, 6, 7, 8):
        tree = m.generate(ids, max_new_tokens=16, do_sample=False, native=False, pad_token_id=0, precision=b)
        fused = m.generate(ids, max_new_tokens=16, do_sample=False, native=True, pad_token_id=0, precision=b)
        assert ("decoder", b) in m._native_cache and m.precision == 8
        wo = m._native_cache[("decoder", b)].layers[0].attention.wo
        assert wo.bitwidth == b and wo.qweight.shape[0] == b
        assert fused.shape == tree.shape == (1, 22)
        assert torch.equal(fused, tree), (b, fused, tree)
        # native=True releases the module tree's q / k / v / gate / up planes only where the parent IS the served precision: below 8
        # bits the tree keeps all 8 planes (it still serves the other precisions), at 8 the fused tensors take them over ..
        if b < 8:
            assert l0.self_attn.q_proj.qweight.shape[0] == 8 and m._released is None
        else:
            assert l0.self_attn.q_proj.qweight.numel() == 0 and m._released is not None
    # .. and the module tree takes every plane back
    again = m.generate(ids, max_new_tokens=4, do_sample=False, native=False, pad_token_id=0, precision=6)
    assert again.shape == (1, 10) and l0.self_attn.q_proj.qweight.numel() > 0
    after = m.model.state_dict()
    assert all(torch.equal(after[k], v) for k, v in planes.items())
