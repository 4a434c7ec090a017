"""What the fused route costs for a Qwen3 layer, measured with bench.py's headline protocol (random-init model, captured DecodeGraph
with ten token steps per replay, the same setup replays, 5 warm-up steps, a 20-step window; `bench.decode_tok_s` is imported, not
restated), three things on one box in one run:

  (a) the Qwen3-8B geometry at 2 bits on the fused route -- wqkv GEMV, then ONE attention launch that normalises q / k per head,
      rotates, writes the cache row and attends (gq_attn_decode_split_qknorm); no RoPE epilogue in the wqkv launch;
  (b) the Llama-3.1-8B geometry through the same function: the yardstick for what the lost epilogue and four more layers cost;
  (c) the module-tree route on model (a): AnyPrecisionForCausalLM.generate(native=False) over transformers' Qwen3 modules.

The Qwen3-8B figures (36 layers, hidden 4096, MLP 12288, 32 / 8 heads of 128, vocab 151936, rope_theta 1e6, eps 1e-6) restate the public
config from memory; they could not be checked offline and matter here only as a shape set (guidedquant_amd.model.transformer_configs).
The captured step ends in the fused sampler, which serves up to 262144 logits: all three legs run the Qwen3 geometry at its published
vocabulary, 151936 (`vocab_size_timed` in the record: the vocabulary the timed model has; a table entry beyond the sampler's limit
would be cut to it).

Prints one JSON record and merges it into profiles/qwen3_fused_route.json under "timing_published_vocab" (other keys of that file are
kept: "timing" is the record taken while the sampler stopped at 131072 logits, with Qwen3's vocabulary cut to that).
    python tools/qwen3_decode_timing.py [--steps 20] [--warmup 5] [--repeats 3] [--no-module-tree]

`--arch qwen2`: the same protocol for the Qwen2.5-7B geometry (28 layers, hidden 3584, MLP 18944, 28 / 4 heads of 128, vocab 152064, a bias
on q / k / v; restated from memory like the Qwen3 figures) -- the fused route (plain wqkv GEMV, then gq_attn_decode_split_bias) against
the module-tree route (`generate(native=False)` over transformers' Qwen2 modules) in the same run.  Written to
profiles/qwen2_fused_route.json under "timing".
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QWEN3 = "Qwen/Qwen3-8B"
QWEN2 = "Qwen/Qwen2.5-7B"
LLAMA = "meta-llama/Meta-Llama-3.1-8B-Instruct"
OUT = os.path.join(ROOT, "profiles", "qwen3_fused_route.json")
OUT_QWEN2 = os.path.join(ROOT, "profiles", "qwen2_fused_route.json")


def timed_config(name):
    """the table entry; a vocabulary beyond what the fused sampler at the end of the captured step serves (262144) would be cut to that --
    Qwen3's 151936 and Llama's 128256 are timed as published"""
    from guidedquant_amd._lib import SAMPLER_MAX_VOCAB
    from guidedquant_amd.model import transformer_configs
    c = dict(transformer_configs[name])
    c["vocab_size"] = min(c["vocab_size"], SAMPLER_MAX_VOCAB)
    return c


def fused_tok_s(name, dev, steps, warmup, repeats):
    import torch
    import bench
    from guidedquant_amd.APLinear import APLinear
    from guidedquant_amd.generate import random_init_
    from guidedquant_amd.model import ModelArgs, Transformer
    torch.manual_seed(1234)
    # (generate.load_model with the vocabulary of timed_config)
    model = Transformer(torch.float16, ModelArgs(**timed_config(name)), linear_class=APLinear, linear_kwargs=dict(bitwidth=2, device=dev))
    model = random_init_(model.to(device=dev, dtype=torch.float16)).eval()
    model.setup_caches(1, bench.SEQ_NEW_TOKENS + 1)
    assert model.native_ready(), "the fused HIP decode step does not serve this model"
    graph, run_steps = bench.decode_tok_s(model, dev, steps, warmup)
    vals = []
    for _ in range(repeats):
        run_steps(warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_steps(steps)
        torch.cuda.synchronize()
        vals.append(steps / (time.perf_counter() - t0))
    graph.close() if hasattr(graph, "close") else None
    n = model.config.n_layer
    best = max(vals)
    rec = dict(model=model.config.model_name, n_layer=n, vocab_size_timed=model.config.vocab_size, tok_s=[round(v, 2) for v in vals], us_per_step=round(1e6 / best, 2),
               us_per_layer=round(1e6 / best / n, 3))
    del graph, model
    torch.cuda.empty_cache()
    return rec


def module_tree_tok_s(dev, new_tokens=100, name=QWEN3):
    """route 3 of AnyPrecisionForCausalLM.generate on the Qwen3-8B (or Qwen2.5-7B) geometry (random 2-bit planes), and the plain call
    (route 1) beside it"""
    import torch
    import transformers
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    c = timed_config(name)
    kw = dict(hidden_size=c["dim"], intermediate_size=c["intermediate_size"], num_hidden_layers=c["n_layer"], num_attention_heads=c["n_head"],
              num_key_value_heads=c["n_local_heads"], vocab_size=c["vocab_size"], max_position_embeddings=c["block_size"], rms_norm_eps=c["norm_eps"],
              tie_word_embeddings=False)
    if name == QWEN2:  # (head_dim = hidden_size / num_attention_heads; the q / k / v biases are part of the module tree)
        assert c["dim"] // c["n_head"] == c["head_dim"]
        cfg = transformers.Qwen2Config(**kw)
    else:
        cfg = transformers.Qwen3Config(head_dim=c["head_dim"], **kw)
    names = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]
    cfg.anyprec = dict(seed_precision=2, parent_precision=2, group_count=1, arch_config=dict(module_names=names, model_name="model", layers_name="layers"))
    m = AnyPrecisionForCausalLM.from_config_random(cfg, device=dev, seed=0)
    ids = torch.tensor([[1]], device=dev)

    def timed(**kw):
        m.generate(ids, max_new_tokens=8, min_new_tokens=8, do_sample=False, pad_token_id=0, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = m.generate(ids, max_new_tokens=new_tokens, min_new_tokens=new_tokens, do_sample=False, pad_token_id=0, **kw)
        torch.cuda.synchronize()
        return round((out.shape[1] - 1) / (time.perf_counter() - t0), 2)

    rec = dict(module_tree_tok_s=timed(native=False), generate_plain_tok_s=timed())
    rec["plain_call_on_fused_route"] = ("decoder", 2) in m._native_cache
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-module-tree", action="store_true")
    ap.add_argument("--arch", choices=["qwen3", "qwen2"], default="qwen3")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU (the HIP path has no fallback)"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.arch == "qwen2":
        return main_qwen2(args, dev)
    rec = dict(protocol="bench.py headline: random init, 2-bit, DecodeGraph with 10 steps per replay, %d warm-up steps, %d-step window, %d windows"
               % (args.warmup, args.steps, args.repeats),
               qwen3_fused=fused_tok_s(QWEN3, dev, args.steps, args.warmup, args.repeats),
               llama_fused=fused_tok_s(LLAMA, dev, args.steps, args.warmup, args.repeats))
    if not args.no_module_tree:
        rec["qwen3_hf_generate"] = module_tree_tok_s(dev)
    a, b = rec["qwen3_fused"], rec["llama_fused"]
    rec["us_per_layer_qwen3_minus_llama"] = round(a["us_per_layer"] - b["us_per_layer"], 3)
    whole = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            whole = json.load(f)
    whole["timing_published_vocab"] = rec
    with open(OUT, "w") as f:
        json.dump(whole, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


def main_qwen2(args, dev):
    rec = dict(protocol="bench.py headline: random init, 2-bit, DecodeGraph with 10 steps per replay, %d warm-up steps, %d-step window, %d windows; "
               "module tree: generate(native=False), 100 new tokens after an 8-token warm-up call" % (args.warmup, args.steps, args.repeats),
               qwen2_fused=fused_tok_s(QWEN2, dev, args.steps, args.warmup, args.repeats))
    if not args.no_module_tree:
        rec["qwen2_hf_generate"] = module_tree_tok_s(dev, name=QWEN2)
        rec["fused_over_module_tree"] = round(max(rec["qwen2_fused"]["tok_s"]) / rec["qwen2_hf_generate"]["module_tree_tok_s"], 2)
        assert rec["qwen2_hf_generate"]["plain_call_on_fused_route"]
    whole = {}
    if os.path.exists(OUT_QWEN2):
        with open(OUT_QWEN2) as f:
            whole = json.load(f)
    whole["timing"] = rec
    with open(OUT_QWEN2, "w") as f:
        json.dump(whole, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
