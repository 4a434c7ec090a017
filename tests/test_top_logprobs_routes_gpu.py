"""GPU, model level: top-n alternatives from the fused decode route -- `DecodeGraph(logprobs=True, top_logprobs=n)` and
`AnyPrecisionForCausalLM.generate(output_logprobs=True, top_logprobs=n)` -- on the tiny Llama of tests/test_decode_logprobs_gpu.py (D = 512,
3 layers, V = 512; the helper is restated here).  The kernels are pinned by tests/test_topn_logprobs_gpu.py; here: the rows land where
the tokens do, a multi-step replay leaves the bits of single steps, generate's two fields, the EOS cut and the refusals."""
import numpy as np
import pytest

import topn_model as tm

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
pytestmark = pytest.mark.gpu

_NAMES = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]
PROMPT = [3, 17, 5, 60, 2, 9]
SAMPLED = dict(do_sample=True, top_k=50, top_p=0.9, temperature=0.7, repetition_penalty=1.3)


@pytest.fixture(scope="module")
def llama():
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    cfg = transformers.LlamaConfig(hidden_size=512, intermediate_size=1024, num_hidden_layers=3, num_attention_heads=8, num_key_value_heads=2,
                                   vocab_size=512, max_position_embeddings=256, rms_norm_eps=1e-5, tie_word_embeddings=False)
    cfg.anyprec = dict(seed_precision=2, parent_precision=2, group_count=1, arch_config=dict(module_names=_NAMES, model_name="model", layers_name="layers"))
    m = AnyPrecisionForCausalLM.from_config_random(cfg, device=torch.device("cuda:0"), seed=5)
    with torch.no_grad():  # (from_config_random draws N(0, 0.02) embeddings: scaled up so that the logits have margins)
        m.model.model.embed_tokens.weight.mul_(25.0)
        m.model.lm_head.weight.mul_(10.0)
    return m


def _start(g, counter=5):
    g.seq.zero_()
    g.ban.zero_()
    g.rng_counter.fill_(counter)
    g.lp_raw.fill_(float("nan"))
    g.top_ids.fill_(-7)
    g.top_lps.fill_(float("nan"))
    g.set_token(7, 0)
    g.set_history([7])


@pytest.mark.parametrize("kw", [dict(temperature=0.7, top_k=50, top_p=0.9, repetition_penalty=1.3), dict(temperature=0.9, top_k=0, min_p=0.02)],
                         ids=["top_k_50", "whole_vocabulary"])
def test_decode_graph_one_and_four_steps_per_replay_leave_the_same_arrays(llama, kw):
    from guidedquant_amd.generate import DecodeGraph
    m, steps, n = llama, 16, 5
    dec = m.native_decoder(2)
    m._evict("graph")
    dec.setup_caches(1, 256)
    got = {}
    for spr, fold in ((1, True), (4, True), (1, False)):
        g = DecodeGraph(dec, m.device, native_sampling=True, fold_embed=fold, seq_capacity=257, steps_per_replay=spr, logprobs=True, top_logprobs=n, **kw)
        try:
            assert g.top_logprobs == n and g.top_ids.shape == g.top_lps.shape == (257, n) and g.top_ids.dtype == torch.int32 and g.top_lps.dtype == torch.float32
            _start(g)
            hits = 0
            for p in range(steps // spr):
                g.step()
                if spr == 1:  # the step's own logits: the row is the model's for them, and a listed draw carries lp_raw
                    torch.cuda.synchronize()
                    logits = dec._native_state()["logits"].view(-1).cpu().numpy().view(np.float16)[:512].copy()
                    row = g.top_ids[p + 1].cpu().numpy()
                    assert row.tolist() == tm.raw_order(logits)[:n].tolist(), p
                    tok = int(g.seq[p + 1])
                    if tok in row.tolist():
                        hits += 1
                        j = row.tolist().index(tok)
                        assert torch.equal(g.top_lps[p + 1, j].view(torch.int32), g.lp_raw[p + 1].view(torch.int32)), p
            torch.cuda.synchronize()
            assert spr != 1 or hits >= 1, hits
            assert bool((g.top_ids[0] == -7).all()) and bool((g.top_ids[steps + 1:] == -7).all()), "a row outside the run was written"
            assert bool(torch.isnan(g.top_lps[0]).all()) and bool(torch.isnan(g.top_lps[steps + 1:]).all())
            lps = g.top_lps[1:steps + 1]
            assert bool(torch.isfinite(lps).all()) and bool((lps <= 0).all()) and bool((lps[:, :-1] >= lps[:, 1:]).all())
            got[(spr, fold)] = (g.seq[:steps + 1].clone(), g.lp_raw[1:steps + 1].clone(), g.top_ids[1:steps + 1].clone(), g.top_lps[1:steps + 1].clone())
        finally:
            g.close()
    for a, b in zip(got[(1, True)], got[(4, True)]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "a four-step replay leaves other arrays than single steps"


def test_decode_graph_refusals_and_the_default(llama):
    from guidedquant_amd.generate import DecodeGraph
    m = llama
    dec = m.native_decoder(2)
    m._evict("graph")
    dec.setup_caches(1, 256)
    ok = dict(native_sampling=True, fold_embed=True, seq_capacity=16, temperature=0.0, top_k=1, logprobs=True, top_logprobs=5)
    for bad in (dict(logprobs=False), dict(seq_capacity=0), dict(native_sampling=False), dict(top_logprobs=21), dict(top_logprobs=-1), dict(top_logprobs=2.5)):
        with pytest.raises(ValueError, match="top_logprobs|logprobs"):
            DecodeGraph(dec, m.device, **dict(ok, **bad))
    g = DecodeGraph(dec, m.device, **dict(ok, top_logprobs=0))  # (the default allocates nothing)
    try:
        assert g.top_logprobs == 0 and g.top_ids is None and g.top_lps is None and g.sampler.topn_ws is None
    finally:
        g.close()


def test_generate_greedy_heads_every_list_with_the_drawn_token(llama):
    m, new, n = llama, 24, 5
    ids = torch.tensor([PROMPT], device=m.device)
    T = ids.shape[1]
    kw = dict(max_new_tokens=new, pad_token_id=0, do_sample=False)
    plain = m.generate(ids, output_logprobs=True, **kw)
    out = m.generate(ids, output_logprobs=True, top_logprobs=n, **kw)
    assert list(out.keys()) == ["sequences", "logprobs", "sampled_logprobs", "top_logprobs_ids", "top_logprobs"]
    assert list(plain.keys()) == ["sequences", "logprobs", "sampled_logprobs"]
    assert torch.equal(out.sequences, plain.sequences) and torch.equal(out.logprobs.view(torch.int32), plain.logprobs.view(torch.int32))
    assert out.top_logprobs_ids.shape == out.top_logprobs.shape == (1, new, n) and out.top_logprobs_ids.dtype == torch.int64 and out.top_logprobs.dtype == torch.float32
    assert torch.equal(out.top_logprobs_ids[0, :, 0], out.sequences[0, T:].long())
    assert torch.equal(out.top_logprobs[0, :, 0].view(torch.int32), out.logprobs[0].view(torch.int32))
    assert any(("top_logprobs", n) in k for k in m._native_cache if k[0] == "graph")
    # n = 20 on the same request: its first five are the list of n = 5
    out20 = m.generate(ids, output_logprobs=True, top_logprobs=20, **kw)
    assert torch.equal(out20.top_logprobs_ids[:, :, :n], out.top_logprobs_ids) and torch.equal(out20.top_logprobs[:, :, :n].view(torch.int32), out.top_logprobs.view(torch.int32))


def test_generate_sampled_with_an_early_eos_is_cut_where_the_sequence_is(llama):
    m, new, n = llama, 24, 5
    ids = torch.tensor([PROMPT], device=m.device)
    T = ids.shape[1]
    kw = dict(max_new_tokens=new, pad_token_id=0, **SAMPLED)
    torch.manual_seed(3)
    out = m.generate(ids, output_logprobs=True, top_logprobs=n, **kw)
    assert out.sequences.shape == (1, T + new) and out.top_logprobs.shape == (1, new, n)
    listed = (out.top_logprobs_ids[0] == out.sequences[0, T:, None]).any(dim=1)
    assert int(listed.sum()) >= 1
    for j in torch.nonzero(listed).view(-1).tolist():  # a listed draw carries `logprobs`
        k = int(torch.nonzero(out.top_logprobs_ids[0, j] == out.sequences[0, T + j])[0])
        assert torch.equal(out.top_logprobs[0, j, k].view(torch.int32), out.logprobs[0, j].view(torch.int32)), j
    eos = int(out.sequences[0, T + 6])
    torch.manual_seed(3)
    cut = m.generate(ids, eos_token_id=eos, output_logprobs=True, top_logprobs=n, **kw)
    k = cut.sequences.shape[1] - T
    assert 1 <= k <= 7 and int(cut.sequences[0, -1]) == eos and torch.equal(cut.sequences, out.sequences[:, :T + k])
    assert cut.top_logprobs_ids.shape == cut.top_logprobs.shape == (1, k, n) and cut.logprobs.shape == (1, k)
    assert torch.equal(cut.top_logprobs_ids, out.top_logprobs_ids[:, :k]) and torch.equal(cut.top_logprobs.view(torch.int32), out.top_logprobs[:, :k].view(torch.int32))


def test_generate_refusals_never_fall_back(llama, monkeypatch):
    m = llama
    ids = torch.tensor([PROMPT], device=m.device)
    called = []
    monkeypatch.setattr(m.model, "generate", lambda *a, **k: called.append(k) or ids)
    base = dict(max_new_tokens=4, do_sample=False, pad_token_id=0)
    for kw in (dict(top_logprobs=5), dict(top_logprobs=5, output_logprobs=False), dict(top_logprobs=0, output_logprobs=True),
               dict(top_logprobs=21, output_logprobs=True), dict(top_logprobs=-3, output_logprobs=True), dict(top_logprobs=5, output_logprobs=True, native=False),
               dict(top_logprobs=5, output_logprobs=True, capture=True), dict(top_logprobs=5, output_logprobs=True, num_beams=2)):
        with pytest.raises(ValueError):
            m.generate(ids, **dict(base, **kw))
    assert called == []
    # top_logprobs=None is the call without the keyword
    out = m.generate(ids, output_logprobs=True, top_logprobs=None, **base)
    assert list(out.keys()) == ["sequences", "logprobs", "sampled_logprobs"] and called == []
