"""No GPU: the host side of the opt-in int8 lm_head -- `head_q8.quantize_rows_int8` against its stated rule, `lm_head_dtype_name`, and
the named errors of the surfaces that do not serve the option (a CPU model, `native=False`, `capture=True`)."""
import pytest

torch = pytest.importorskip("torch")


def _rows(N=37, K=96, seed=0):
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-9, 3, (N, 1), generator=g).float())).half()
    assert bool(torch.isfinite(W).all()) and bool((W.abs().amax(dim=1) > 0).all())
    return W


def test_quantised_rows_keep_the_stated_rule():
    from guidedquant_amd.head_q8 import quantize_rows_int8
    W = _rows()
    q, s = quantize_rows_int8(W)
    assert q.dtype == torch.int8 and q.shape == W.shape and q.is_contiguous()
    assert s.dtype == torch.float32 and s.shape == (W.shape[0], ) and s.is_contiguous()
    assert int(q.to(torch.int32).abs().max()) <= 127
    assert bool((q.to(torch.int32).abs().amax(dim=1) == 127).all()), "every row reaches +-127"
    assert torch.equal(s, W.float().abs().amax(dim=1) / 127.0)  # (an fp32 division of the fp32 maximum)
    # |scale * q - W| <= scale / 2, up to the rounding of the fp32 quotient the code was rounded from
    err = (s.double()[:, None] * q.double() - W.double()).abs()
    assert bool((err <= s.double()[:, None] / 2 * (1 + 2.0**-20)).all()), float((err / s.double()[:, None]).max())
    # the stated formula, element by element
    want = torch.round(W.float() / s[:, None]).clamp(-127, 127).to(torch.int8)
    assert torch.equal(q, want)


def test_ties_round_to_even():
    from guidedquant_amd.head_q8 import quantize_rows_int8
    # scale = 2^-7 exactly (the maximum is 127 * 2^-7); W / scale = 0.5, 1.5, 2.5, -0.5, -1.5, -2.5 -> 0, 2, 2, -0, -2, -2
    W = torch.tensor([[127.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, -127.0]]).mul(2.0**-7).half()
    q, s = quantize_rows_int8(W)
    assert float(s[0]) == 2.0**-7
    assert q[0].tolist() == [127, 0, 2, 2, 0, -2, -2, -127]


def test_exactly_representable_rows_come_back_unchanged():
    """rows scale * q that fp16 holds exactly, scale a power of two, +-127 in every row: absmax / 127 is that scale again, and the codes"""
    from guidedquant_amd.head_q8 import quantize_rows_int8
    g = torch.Generator().manual_seed(1)
    N, K = 29, 64
    q0 = torch.randint(-127, 128, (N, K), generator=g)
    q0[:, 3], q0[::2, 9], q0[1::2, 9] = 127, -127, 0
    s0 = torch.exp2(torch.randint(-14, -3, (N, ), generator=g).float())
    W = (q0.float() * s0[:, None]).half()
    assert torch.equal(W.float(), q0.float() * s0[:, None])  # (fp16-exact: |q| < 2^7, scale * q >= 2^-14 or zero)
    q, s = quantize_rows_int8(W)
    assert torch.equal(s, s0) and torch.equal(q.to(torch.int64), q0)
    q2, s2 = quantize_rows_int8((q.float() * s[:, None]).half())
    assert torch.equal(q2, q) and torch.equal(s2, s)


def test_a_row_of_zeros_and_non_finite_weights():
    from guidedquant_amd.head_q8 import quantize_rows_int8
    W = _rows(5, 32)
    W[2] = 0
    q, s = quantize_rows_int8(W)
    assert float(s[2]) == 1.0 and bool((q[2] == 0).all())
    assert bool((q[[0, 1, 3, 4]].to(torch.int32).abs().amax(dim=1) == 127).all())
    for bad in (float("nan"), float("inf"), float("-inf")):
        Wb = W.clone()
        Wb[3, 7] = bad
        with pytest.raises(ValueError, match="NaN or an Inf"):
            quantize_rows_int8(Wb)
    with pytest.raises(ValueError):
        quantize_rows_int8(W.float())
    with pytest.raises(ValueError):
        quantize_rows_int8(W[0])


def test_row_blocks_do_not_change_the_result(monkeypatch):
    from guidedquant_amd import head_q8
    W = _rows(41, 32, seed=4)
    q, s = head_q8.quantize_rows_int8(W)
    monkeypatch.setattr(head_q8, "ROWS", 16)  # (blocks of 16 rows with a ragged last one)
    q2, s2 = head_q8.quantize_rows_int8(W)
    assert torch.equal(q, q2) and torch.equal(s, s2)


def test_cpu_and_gpu_give_identical_tensors():
    from guidedquant_amd.head_q8 import quantize_rows_int8
    if not torch.cuda.is_available():
        pytest.skip("no GPU: the CPU half of the comparison is every other test of this file")
    W = _rows(257, 512, seed=2)
    q, s = quantize_rows_int8(W)
    qg, sg = quantize_rows_int8(W.cuda())
    assert qg.is_cuda and torch.equal(qg.cpu(), q) and torch.equal(sg.cpu(), s)


def test_lm_head_dtype_name():
    from guidedquant_amd.head_q8 import lm_head_dtype_name
    assert lm_head_dtype_name(None) == "fp16" and lm_head_dtype_name("fp16") == "fp16" and lm_head_dtype_name("int8") == "int8"
    for bad in ("fp8", "int4", "INT8", "", 8, torch.int8):
        with pytest.raises(ValueError, match="lm_head_dtype"):
            lm_head_dtype_name(bad)


def _tiny(dtype=torch.float32):
    from guidedquant_amd.model import ModelArgs, Transformer
    return Transformer(dtype, ModelArgs(dim=256, n_head=4, n_local_heads=2, n_layer=1, vocab_size=64, intermediate_size=512, block_size=64,
                                        model_name="llama-tiny")).eval()


def test_a_cpu_transformer_refuses_the_int8_head():
    from guidedquant_amd.pipeline import PipelinedDecoder
    from guidedquant_amd.tp import TensorParallelDecoder
    m = _tiny()
    assert m.lm_head_dtype == "fp16" and m._head_q8 is None
    for mm in (m, _tiny().half()):
        with pytest.raises(ValueError, match="lm_head_dtype='int8': .*CPU"):
            mm.set_lm_head_dtype("int8")
        assert mm.lm_head_dtype == "fp16" and mm._head_q8 is None
    with pytest.raises(ValueError, match="lm_head_dtype"):
        m.set_lm_head_dtype("int4")
    m.set_lm_head_dtype(None)
    m.set_lm_head_dtype("fp16")
    assert m.lm_head_dtype == "fp16"
    assert not any("q8" in k for k in m.state_dict())
    # the decoders that launch the head themselves decline an int8-head model by name (the attribute alone decides: no GPU needed)
    m.lm_head_dtype = "int8"
    with pytest.raises(NotImplementedError, match="int8 lm_head"):
        TensorParallelDecoder(m, None, 0, 2, 4)
    with pytest.raises(NotImplementedError, match="int8 lm_head"):
        PipelinedDecoder(m, 0, 1, range(0, 1), n_seq=1, max_new_tokens=4)


def test_generate_with_the_int8_head_on_surfaces_that_do_not_serve_it():
    transformers = pytest.importorskip("transformers")
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    hf = transformers.LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2,
                                  vocab_size=128, max_position_embeddings=64, rms_norm_eps=1e-5, tie_word_embeddings=False)
    names = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]
    hf.anyprec = dict(seed_precision=2, parent_precision=3, group_count=1, arch_config=dict(module_names=names, model_name="model", layers_name="layers"))
    m = AnyPrecisionForCausalLM.from_config_random(hf, device="cpu")
    ids = torch.tensor([[3, 17, 5]])
    before = m.precision
    other = [p for p in m.precisions if p != before][0]
    with pytest.raises(ValueError, match="lm_head_dtype='int8': the fused routes need the GPU"):
        m.generate(ids, max_new_tokens=2, do_sample=False, lm_head_dtype="int8", precision=other)
    assert m.precision == before
    with pytest.raises(ValueError, match="lm_head_dtype='int8': served by the fused decode model only"):
        m.generate(ids, max_new_tokens=2, do_sample=False, lm_head_dtype="int8", native=False, precision=other)
    assert m.precision == before
    with pytest.raises(ValueError, match="lm_head_dtype='int8': served by the fused decode model only"):
        m.generate(ids, max_new_tokens=2, do_sample=False, lm_head_dtype="int8", capture=True)
    with pytest.raises(ValueError, match="lm_head_dtype"):
        m.generate(ids, max_new_tokens=2, do_sample=False, lm_head_dtype="int4", precision=other)
    assert m.precision == before
    out = m.generate(ids, max_new_tokens=2, do_sample=False, lm_head_dtype="fp16")  # the default by name: popped, never reaches transformers
    assert out.shape == (1, 5)
    assert torch.equal(out, m.generate(ids, max_new_tokens=2, do_sample=False))
