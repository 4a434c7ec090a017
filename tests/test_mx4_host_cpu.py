"""No GPU: `model.mxfp4_quantize` / `mxfp4_dequant` (kv_cache_dtype="mxfp4") against the numpy model tests/mx4_model.py on the edge inputs of
the write rule, byte for byte, the stated error bound, and the keyword's refusals.  A case is one block of 32 values; case c sits in block
c % (head_dim / 32) of its row, beside random blocks of other magnitudes, and holds its special values at even and at odd positions."""
import numpy as np
import pytest

import mx4_model as mx

torch = pytest.importorskip("torch")

TIES = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])


def _bits(v, step=0):
    return (np.array([v], dtype=np.float16).view(np.uint16) + step).view(np.float16)[0]


def _blocks():
    """name -> 32 fp16 values"""
    rng = np.random.default_rng(4)
    out = {"zeros": np.zeros(32), "signed-zeros": np.where(np.arange(32) % 3 == 0, -0.0, 0.0),
           "subnormals": (np.arange(32, dtype=np.uint16) * 31 + 1).view(np.float16), "49152": rng.uniform(-3e4, 3e4, 32), "65504": rng.uniform(-6e4, 6e4, 32),
           "nan": rng.normal(0, 1, 32), "inf": rng.normal(0, 100, 32)}
    out["49152"][5], out["65504"][8], out["65504"][11] = 49152.0, -65504.0, 65504.0
    out["nan"][7], out["inf"][2], out["inf"][9] = np.nan, np.inf, -np.inf
    for k in (-15, -4, 0, 13):
        b = np.zeros(32)
        b[0], b[1:8], b[8:15], b[15:22], b[22] = 6.0, TIES, -TIES, TIES[::-1], -6.0  # every tie at both nibble positions, both signs
        out["ties*2^%d" % k] = b * 2.0**k
        for name, step in (("at", 0), ("above", 1)):  # amax exactly 6 * 2^k and one fp16 step above it
            b = rng.uniform(-3, 3, 32) * 2.0**k
            b[17] = -float(_bits(6.0 * 2.0**k, step))
            out["%s-6*2^%d" % (name, k)] = b
    return {n: np.asarray(b, dtype=np.float64).astype(np.float16) for n, b in out.items()}


BLOCKS = _blocks()


def rows(hd):
    """fp16 [len(BLOCKS), hd]: case c in block c % (hd / 32), random blocks at 2^(c % 9 - 4) around it"""
    rng = np.random.default_rng(hd)
    x = np.stack([rng.normal(0, 2.0 ** (c % 9 - 4), hd) for c in range(len(BLOCKS))]).astype(np.float16)
    for c, b in enumerate(BLOCKS.values()):
        x[c, 32 * (c % (hd // 32)):][:32] = b
    return x


@pytest.mark.parametrize("hd", [64, 128])
def test_quantize_equals_the_numpy_model_and_meets_the_bound(hd):
    from guidedquant_amd.model import mxfp4_dequant, mxfp4_quantize
    x = rows(hd)
    codes, exps = mxfp4_quantize(torch.from_numpy(x))
    want_c, want_e = mx.quantize(x)
    assert np.array_equal(exps.numpy(), want_e), np.argwhere(exps.numpy() != want_e)[:4]
    assert np.array_equal(codes.numpy(), want_c), np.argwhere(codes.numpy() != want_c)[:4]
    deq = mxfp4_dequant(codes, exps)
    assert deq.dtype == torch.float16 and np.array_equal(deq.double().numpy(), mx.dequant(want_c, want_e), equal_nan=True)  # (exact in fp16)
    x64, d64, names = x.astype(np.float64), deq.double().numpy(), list(BLOCKS)
    bad = np.repeat(want_e == 0xFF, 32, -1)
    assert np.isnan(d64[bad]).all() and np.isfinite(d64[~bad]).all()
    assert set(np.argwhere(want_e == 0xFF)[:, 0]) == {names.index("nan"), names.index("inf")}
    top = 6.0 * np.repeat(np.exp2(want_e.astype(np.float64) - 127), 32, -1)
    over = ~bad & (np.abs(x64) > top)  # (only behind the clamp at e = 13: they read 49152)
    assert set(np.argwhere(over)[:, 0]) == {names.index("65504"), names.index("above-6*2^13")} and (np.abs(d64[over]) == 49152.0).all()
    ok = ~bad & ~over
    assert (np.abs(x64 - d64)[ok] <= mx.error_bound(x64, want_e)[ok]).all()
    assert np.array_equal(np.signbit(d64[ok]), np.signbit(x64[ok]))  # (a signed zero keeps its sign)
    z = names.index("zeros")
    assert want_e[z, z % (hd // 32)] == 127 - 15 and (d64[x64 == 49152.0] == 49152.0).all()  # (an all-zero block: e = -15; 6 * 2^13 is kept)


def test_keyword_and_refusals():
    from guidedquant_amd.model import ModelArgs, Transformer
    m = Transformer(torch.float32, ModelArgs(dim=256, n_head=4, n_local_heads=2, n_layer=2, vocab_size=64, intermediate_size=512, block_size=64,
                                             model_name="llama-tiny")).eval()
    for bad in ("fp4", "int4"):
        with pytest.raises(ValueError, match="kv_cache_dtype"):
            m.setup_caches(1, 8, kv_cache_dtype=bad)
    m.setup_caches(1, 8, kv_cache_dtype="mxfp4")
    kc = m.layers[0].attention.kv_cache
    assert m.kv_cache_dtype == "mxfp4" and kc.k_cache.shape == (1, 2, 8, 32) and kc.k_cache.dtype == torch.uint8 and kc.v_exp.shape == (1, 2, 8, 2)
    with pytest.raises(ValueError, match="set_kv_scales: an mxfp4 cache has no per-head scales"):
        m.set_kv_scales(torch.ones(2, 2), torch.ones(2, 2))
    # the module forward over such a cache: the rows it stores are the write rule's
    idx, pos = torch.tensor([[3, 9, 1]]), torch.arange(3)
    with torch.no_grad():
        assert torch.isfinite(m(idx, pos)).all()
    assert bool((kc.k_exp[:, :, :3] != 127).any()) and bool((kc.k_exp[:, :, 3:] == 127).all())

    from guidedquant_amd import model as gm
    from guidedquant_amd.generate import load_model
    from guidedquant_amd.pipeline import PipelinedDecoder
    from guidedquant_amd.tp import TensorParallelDecoder
    with pytest.raises(NotImplementedError, match="mxfp4 KV cache: tensor-parallel"):
        TensorParallelDecoder(m, None, 0, 2, 4)
    with pytest.raises(NotImplementedError, match="mxfp4 KV cache: layer-pipelined"):
        PipelinedDecoder(m, 0, 1, range(0, 2), n_seq=1, max_new_tokens=4)
    gm.transformer_configs["qtip-test"] = dict(model_name="llama-qtip-test", block_size=64, vocab_size=128, n_layer=1, n_head=4, dim=256, intermediate_size=512,
                                               n_local_heads=2)
    try:
        q = load_model("qtip-test", "cpu", "qtip", 2, random_init=True)
    finally:
        del gm.transformer_configs["qtip-test"]
    with pytest.raises(NotImplementedError, match="mxfp4 KV cache: QTIP"):
        q.setup_caches(1, 8, kv_cache_dtype="mxfp4")

    transformers = pytest.importorskip("transformers")
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    hf = transformers.LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2,
                                  vocab_size=128, max_position_embeddings=64, rms_norm_eps=1e-5, tie_word_embeddings=False)
    names = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]
    hf.anyprec = dict(seed_precision=2, parent_precision=2, group_count=1, arch_config=dict(module_names=names, model_name="model", layers_name="layers"))
    ap = AnyPrecisionForCausalLM.from_config_random(hf, device="cpu")
    with pytest.raises(ValueError, match="kv_cache_dtype='mxfp4': the fused routes need the GPU"):
        ap.generate(torch.tensor([[3, 17, 5]]), max_new_tokens=2, do_sample=False, kv_cache_dtype="mxfp4")
