"""GPU: the opt-in int8 lm_head through the model, the captured step and the HF surface (Transformer.set_lm_head_dtype,
native_step.StepState.head, generate.DecodeGraph, AnyPrecisionForCausalLM.generate(lm_head_dtype=)).

The arithmetic bound is the one of tests/test_dense_gemv_i8_gpu.py, evaluated on the step's own normalised vector xn (the state's hidden
vector before the head, normalised with the kernel's rounding points):
    bound_n = 2^-11 * 1.001 * |ref_n| + 2e-5 * sum_k |xn_k| |scale_n q_nk| + 1e-7,    ref_n = float64 sum_k xn_k (scale_n q_nk)
  * a head that int8 holds exactly (output.weight = 2^-e * q): the int8 and the fp16 launch each lie within bound of the same float64
    sum, so |logit_i8 - logit_f16| <= 2 * bound;
  * a general head: |logit_i8 - float64(W_fp16 @ xn)| <= bound + sum_k |xn_k| * scale_n / 2 -- the arithmetic bound plus the bound of
    the quantisation error (|scale q - W| <= scale / 2 per weight).  Nothing is measured."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOKS = [5, 17, 900, 3, 3, 512, 44, 1023]
_NAMES = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]
PROMPT = [3, 17, 5, 60, 2, 9]


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _tiny_model(bits=2, hd=64):
    """tests/test_decode_gpu.py::_tiny_model: dim 512, vocab 1024, 2 layers"""
    from guidedquant_amd.APLinear import APLinear
    from guidedquant_amd.generate import random_init_
    from guidedquant_amd.model import ModelArgs, Transformer
    d = _dev()
    n_head = 8
    cfg = ModelArgs(block_size=256, vocab_size=1024, n_layer=2, n_head=n_head, dim=n_head * hd, intermediate_size=1024,
                    n_local_heads=2, rope_base=500000, model_name="llama-test")
    m = Transformer(torch.float16, cfg, linear_class=APLinear, linear_kwargs=dict(bitwidth=bits, device=d))
    m = m.to(device=d, dtype=torch.float16)
    random_init_(m, seed=bits, lut_std=0.05)
    g = torch.Generator(device=d)
    g.manual_seed(1)
    for b in m.layers:
        b.input_layernorm.weight.data.copy_((1 + 0.1 * torch.randn(cfg.dim, device=d, generator=g)).half())
        b.post_attention_layernorm.weight.data.copy_((1 + 0.1 * torch.randn(cfg.dim, device=d, generator=g)).half())
    m.norm.weight.data.copy_((1 + 0.1 * torch.randn(cfg.dim, device=d, generator=g)).half())
    m.setup_caches(1, 32)
    assert m.native_ready()
    return m.eval()


def _force(m, toks=TOKS):
    """teacher-forced decode steps: [(logits fp16 [V], xn float64 [D])], xn from the state's hidden vector before the head"""
    d, out = _dev(), []
    K, eps = m.config.dim, m.config.norm_eps
    with torch.no_grad():
        for p, t in enumerate(toks):
            lg = m.decode_native(torch.tensor([t], dtype=torch.int32, device=d), torch.tensor([p], dtype=torch.int32, device=d))
            torch.cuda.synchronize()
            x = m._native_state()["x"]
            s = (1.0 / torch.sqrt((x.double()**2).sum() / K + eps)).float()
            xn = ((x.float() * s).half() * m.norm.weight).double()
            out.append((lg.view(-1).clone(), xn))
    return out


def _bound(xn, q, scale):
    W64 = q.double() * scale.double()[:, None]
    ref = W64 @ xn
    return 2.0**-11 * 1.001 * ref.abs() + 2e-5 * (W64.abs() @ xn.abs()) + 1e-7


def test_a_head_that_int8_holds_exactly():
    m = _tiny_model()
    V, D = m.config.vocab_size, m.config.dim
    g = torch.Generator().manual_seed(3)
    q0 = torch.randint(-127, 128, (V, D), generator=g)
    q0[:, 5], q0[:, 300] = 127, -127
    s0 = torch.exp2(-torch.randint(6, 11, (V, ), generator=g).float())
    m.set_lm_head_dtype("int8")
    first = m.head_q8()[0]
    with torch.no_grad():  # (an in-place write behind the switch: the int8 copy is made again on the next use)
        m.output.weight.copy_((q0.float() * s0[:, None]).half())
    q, s = m.head_q8()
    assert q is not first and torch.equal(q.cpu().to(torch.int64), q0) and torch.equal(s.cpu(), s0)
    assert m.head_q8()[0] is q, "the copy is made once"
    m.setup_caches(1, 64)  # (a cache that grows does not make it again)
    assert m.head_q8()[0] is q
    assert not any(t is q or t is s for t in m.state_dict().values()) and len(m.state_dict()) == len(_tiny_model().state_dict())
    i8 = _force(m)
    m.set_lm_head_dtype("fp16")
    f16 = _force(m)
    worst = 0.0
    for (a, xn), (b, xn2) in zip(i8, f16):
        assert torch.equal(xn, xn2), "the layers in front of the head do not depend on it"
        assert torch.isfinite(a.float()).all()
        bound = _bound(xn, q, s)
        err = (a.double() - b.double()).abs()
        worst = max(worst, float((err / bound).max()))
        assert (err <= 2 * bound).all()
    print("lossless head: worst |i8 - f16| / bound %.3f (allowed 2)" % worst)


def _general(m, toks):
    m.set_lm_head_dtype("int8")
    q, s = m.head_q8()
    W64 = m.output.weight.detach().double()
    worst = 0.0
    for lg, xn in _force(m, toks):
        allowed = _bound(xn, q, s) + xn.abs().sum() * s.double() / 2
        err = (lg.double() - W64 @ xn).abs()
        worst = max(worst, float((err / allowed).max()))
        assert torch.isfinite(lg.float()).all() and (err <= allowed).all()
    print("general head: worst err / (bound + quantisation bound) %.3f" % worst)


def test_a_general_head_against_the_fp16_weights():
    _general(_tiny_model(), TOKS)


def test_a_general_head_on_a_qtip_model():
    from guidedquant_amd import model as gm
    from guidedquant_amd.generate import load_model
    gm.transformer_configs["qtip-q8-test"] = dict(model_name="llama-qtip-q8-test", block_size=128, vocab_size=512, n_layer=2,
                                                  n_head=8, dim=1024, intermediate_size=2048, n_local_heads=4)
    try:
        m = load_model("qtip-q8-test", "cuda:0", "qtip", 2, random_init=True)
    finally:
        del gm.transformer_configs["qtip-q8-test"]
    with torch.device("cuda:0"):
        m.setup_caches(max_batch_size=1, max_seq_length=64)
    assert m.native_ready() and m._native_kind() == "qtip"
    _general(m, [1, 17, 200, 5])


def _argmax_lowest(lg):
    """the sampler's order: the largest fp16 value, the lowest id among equals"""
    v = lg.view(-1).float()
    return int(torch.nonzero(v == v.max())[0])


def _eager(m, tok, steps):
    d, out = _dev(), []
    with torch.no_grad():
        for p in range(steps):
            lg = m.decode_native(torch.tensor([tok], dtype=torch.int32, device=d), torch.tensor([p], dtype=torch.int32, device=d))
            tok = _argmax_lowest(lg)
            out.append(tok)
    return out


@pytest.mark.parametrize("kw", [dict(), dict(fold_embed=True, steps_per_replay=4)], ids=["plain", "fold_embed-4_steps"])
def test_decode_graph_over_the_int8_head(kw):
    from guidedquant_amd.generate import DecodeGraph
    m, steps = _tiny_model(), 16
    with torch.no_grad():  # (margins between the logits: a greedy sequence that moves through the vocabulary)
        m.output.weight.mul_(8.0)
    m.set_lm_head_dtype("int8")
    want = _eager(m, 7, steps)
    g = DecodeGraph(m, _dev(), native_sampling=True, top_k=1, temperature=0.0, seq_capacity=64, **kw)
    try:
        assert g.native_sampling
        g.seq.zero_()
        g.ban.zero_()
        g.set_token(7, 0)
        g.set_history([7])
        for _ in range(steps // g.steps_per_replay):
            g.step()
        torch.cuda.synchronize()
        assert g.seq[1:steps + 1].tolist() == want
        # the other head under this graph: refused by the existing re-validation, in both directions
        m.set_lm_head_dtype("fp16")
        with pytest.raises(RuntimeError, match="bound to .* re-allocated"):
            g.step()
    finally:
        g.close()
    g = DecodeGraph(m, _dev(), native_sampling=True, top_k=1, temperature=0.0, seq_capacity=64, **kw)
    try:
        g.set_token(7, 0)
        g.step()
        m.set_lm_head_dtype("int8")
        with pytest.raises(RuntimeError, match="bound to .* re-allocated"):
            g.step()
    finally:
        g.close()


def test_the_default_is_untouched():
    a, b = _tiny_model(), _tiny_model()
    want = [lg for lg, _ in _force(a)]
    assert b.lm_head_dtype == "fp16" and b._head_q8 is None
    b.set_lm_head_dtype("int8")
    assert b.lm_head_dtype == "int8" and b._head_q8 is not None
    q, s = b.head_q8()
    V, D = b.config.vocab_size, b.config.dim
    assert q.dtype == torch.int8 and q.shape == (V, D) and s.dtype == torch.float32 and s.shape == (V, ) and q.is_cuda
    i8 = [lg for lg, _ in _force(b)]
    assert any(not torch.equal(x, y) for x, y in zip(i8, want)), "the int8 head never ran"
    del q, s
    b.set_lm_head_dtype("fp16")
    assert b.lm_head_dtype == "fp16" and b._head_q8 is None, "int8 tensors are still held"
    got = [lg for lg, _ in _force(b)]
    for x, y in zip(got, want):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16))
    # the module forward reads the fp16 head under either setting
    b.set_lm_head_dtype("int8")
    d = _dev()
    with torch.no_grad():
        l0 = a(torch.tensor([[5]], dtype=torch.int32, device=d), torch.tensor([0], dtype=torch.int32, device=d))
        l1 = b(torch.tensor([[5]], dtype=torch.int32, device=d), torch.tensor([0], dtype=torch.int32, device=d))
    assert torch.equal(l0, l1)


def test_quantiser_cpu_and_gpu_give_identical_tensors():
    from guidedquant_amd.head_q8 import quantize_rows_int8
    g = torch.Generator().manual_seed(2)
    W = (torch.randn(257, 512, generator=g) * torch.exp2(torch.randint(-9, 3, (257, 1), generator=g).float())).half()
    W[11] = 0
    q, s = quantize_rows_int8(W)
    qg, sg = quantize_rows_int8(W.to(_dev()))
    assert qg.is_cuda and torch.equal(qg.cpu(), q) and torch.equal(sg.cpu(), s)


def test_a_non_fp16_head_and_the_multi_device_decoders_decline():
    from guidedquant_amd.model import ModelArgs, Transformer
    from guidedquant_amd.pipeline import PipelinedDecoder
    from guidedquant_amd.tp import TensorParallelDecoder
    cfg = ModelArgs(block_size=64, vocab_size=64, n_layer=1, n_head=4, dim=256, intermediate_size=512, n_local_heads=2, model_name="llama-test")
    f32 = Transformer(torch.float32, cfg).to(_dev())
    with pytest.raises(ValueError, match="lm_head_dtype='int8': .*not fp16"):
        f32.set_lm_head_dtype("int8")
    assert f32.lm_head_dtype == "fp16" and f32._head_q8 is None
    m = _tiny_model()
    m.set_lm_head_dtype("int8")
    with pytest.raises(NotImplementedError, match="int8 lm_head"):  # (the constructors only: no second process)
        TensorParallelDecoder(m, None, 0, 2, 4)
    with pytest.raises(NotImplementedError, match="int8 lm_head"):
        PipelinedDecoder(m, 0, 1, range(0, 2), n_seq=1, max_new_tokens=4)
    assert m.lm_head_dtype == "int8"
    m.cpu()  # (the int8 copy follows output.weight: dropped with the move, and not to be had on the CPU)
    assert m._head_q8 is None
    with pytest.raises(ValueError, match="lm_head_dtype='int8'"):
        m.head_q8()


# ------------------------------------------------------------------------------------------------ the HF surface
def _hf(seed=5):
    """tests/test_repetition_penalty_routes_gpu.py::_model: hidden size 512 (the dense GEMV takes K % 512 == 0)"""
    transformers = pytest.importorskip("transformers")
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    cfg = transformers.LlamaConfig(hidden_size=512, intermediate_size=1024, num_hidden_layers=3, num_attention_heads=8, num_key_value_heads=2,
                                   vocab_size=512, max_position_embeddings=256, rms_norm_eps=1e-5, tie_word_embeddings=False)
    cfg.anyprec = dict(seed_precision=2, parent_precision=2, group_count=1, arch_config=dict(module_names=_NAMES, model_name="model", layers_name="layers"))
    m = AnyPrecisionForCausalLM.from_config_random(cfg, device=torch.device("cuda:0"), seed=seed)
    with torch.no_grad():  # (from_config_random draws N(0, 0.02) embeddings: scaled up so that the logits have margins)
        m.model.model.embed_tokens.weight.mul_(25.0)
        m.model.lm_head.weight.mul_(10.0)
    return m


def test_generate_with_the_int8_head():
    m, new = _hf(), 12
    ids = torch.tensor([PROMPT], device=m.device)
    T = ids.shape[1]
    fresh = _hf().generate(ids, max_new_tokens=new, do_sample=False, pad_token_id=0, native=True)
    out = m.generate(ids, max_new_tokens=new, do_sample=False, pad_token_id=0, native=True, lm_head_dtype="int8")
    assert any(k[0] == "graph" and ("lm_head", "int8") in k for k in m._native_cache)
    dec = m.native_decoder()
    assert dec.lm_head_dtype == "int8" and dec._head_q8 is not None
    assert out.shape[0] == 1 and T < out.shape[1] <= T + new and torch.equal(out[:, :T], ids)
    # the eager int8 loop on the decoder: the prompt as generate feeds it, then decode_native + the sampler's argmax
    ids32 = ids.view(-1).to(torch.int32)
    want, tok = [], int(ids32[T - 1])
    with torch.inference_mode():
        pre, pos = ids32[:T - 1], torch.arange(0, T - 1, device=m.device, dtype=torch.int32)
        assert dec.prefill_ready(pre)
        dec.prefill_native(pre, pos, start=0)
        for p in range(T - 1, T - 1 + new):
            lg = dec.decode_native(torch.tensor([tok], dtype=torch.int32, device=m.device), torch.tensor([p], dtype=torch.int32, device=m.device))
            tok = _argmax_lowest(lg)
            want.append(tok)
    n = out.shape[1] - T   # (shorter than `new` only where the sequence reached EOS)
    assert out[0, T:].tolist() == want[:n]
    # log-probabilities and the top-n lists come from the same step
    r = m.generate(ids, max_new_tokens=new, do_sample=False, pad_token_id=0, native=True, lm_head_dtype="int8", output_logprobs=True, top_logprobs=3)
    assert torch.equal(r.sequences, out)
    assert r.logprobs.shape == (1, n) and bool(torch.isfinite(r.logprobs).all()) and bool(torch.isfinite(r.top_logprobs).all())
    assert r.top_logprobs_ids.shape == (1, n, 3)
    for j in range(n):
        hit = (r.top_logprobs_ids[0, j] == r.sequences[0, T + j]).nonzero()
        assert hit.numel() == 1, "a greedy token is the most probable one: it is listed"
        assert r.top_logprobs[0, j, int(hit[0])].view(torch.int32) == r.logprobs[0, j].view(torch.int32)
    # declined by name, never a fall-back; the precision stays
    before = m.precision
    with pytest.raises(ValueError, match="lm_head_dtype='int8': served by the fused decode model only"):
        m.generate(ids, max_new_tokens=new, do_sample=False, pad_token_id=0, capture=True, lm_head_dtype="int8")
    with pytest.raises(ValueError, match="lm_head_dtype='int8': served by the fused decode model only"):
        m.generate(ids, max_new_tokens=new, do_sample=False, pad_token_id=0, native=False, lm_head_dtype="int8")
    with pytest.raises(ValueError, match="lm_head_dtype='int8': "):
        m.generate(ids, max_new_tokens=new, num_beams=2, do_sample=False, pad_token_id=0, lm_head_dtype="int8")
    assert m.precision == before
    # a call without the keyword is the call a fresh model makes
    again = m.generate(ids, max_new_tokens=new, do_sample=False, pad_token_id=0, native=True)
    assert torch.equal(again, fresh)
    assert dec.lm_head_dtype == "fp16" and dec._head_q8 is None
    assert not any(("lm_head", "int8") in k for k in m._native_cache if k[0] == "graph")
    assert torch.equal(m.generate(ids, max_new_tokens=new, do_sample=False, pad_token_id=0, native=True, lm_head_dtype="fp16"), fresh)
    assert m.native_decoder(lm_head_dtype="int8").lm_head_dtype == "int8" and m.native_decoder().lm_head_dtype == "int8"
    assert torch.equal(m.generate(ids, max_new_tokens=new, do_sample=False, pad_token_id=0, native=True), fresh)
    assert m.native_decoder().lm_head_dtype == "fp16"
