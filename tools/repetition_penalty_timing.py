"""What the repetition penalty costs per token inside the captured decode step, and what serving it on the fused route is worth.

Random-init Qwen2.5-7B geometry at 2 bits with 151936 logits (the published Qwen vocabulary; the table's own 152064 padded rows are cut
to it), bench.py's headline protocol restated for a DecodeGraph that takes a penalty: ten token steps per replay, embedding folded into
the sampler, greedy, sequences of 100 new tokens from a BOS prompt (`set_history` with it before every sequence, as generate() does).

  in-graph   TWO graphs over ONE model in ONE process -- repetition_penalty = 1.0 (gq_sample_topk_p: the fp16-key kernels) and 1.05
             (gq_sample_topk_rep: fp32 values, u64 keys in stage 1, the two token sets) -- timed in alternating windows, each window a
             host clock around `steps` token steps that ends in a device synchronise; per leg the windows' tokens/s, the best and the
             median, and the difference of the medians in us per token and in per cent
  module     AnyPrecisionForCausalLM.generate on the same geometry with repetition_penalty = 1.05: the module tree (native=False, what
             a plain generate() of a Qwen2.5-Instruct checkpoint took before the fused sampler served the penalty) against the plain call

Writes profiles/repetition_penalty_decode.json and prints the record.
    python tools/repetition_penalty_timing.py [--steps 200] [--warmup 20] [--repeats 5] [--no-module-tree]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QWEN2 = "Qwen/Qwen2.5-7B"
VOCAB = 151936
OUT = os.path.join(ROOT, "profiles", "repetition_penalty_decode.json")
SEQ_NEW_TOKENS, SPR = 100, 10


def timed_config():
    from guidedquant_amd.model import transformer_configs
    c = dict(transformer_configs[QWEN2])
    c["vocab_size"] = VOCAB
    return c


def make_runner(model, dev, rp):
    """bench.decode_tok_s for a graph with a penalty: (graph, run_steps)"""
    import torch
    from guidedquant_amd.generate import DecodeGraph
    graph = DecodeGraph(model, dev, native_sampling=True, temperature=0.0, top_k=32, fold_embed=True, steps_per_replay=SPR, repetition_penalty=rp)
    assert graph.native_sampling and (graph.seen is not None) == (rp != 1.0)
    bos = torch.tensor([[128000]], dtype=torch.int32, device=dev)
    zero = torch.zeros((1, ), dtype=torch.int32, device=dev)

    def run_steps(n):
        done = 0
        while done < n:
            graph.set_token(bos, zero)
            graph.set_history(bos.view(-1))  # (one small launch per 100 tokens on the penalty leg; nothing on the other)
            k = min(SEQ_NEW_TOKENS, n - done)
            for _ in range(k // SPR):
                graph.step()
            for _ in range(k % SPR):
                graph.step_one()
            done += k

    run_steps(2 * SEQ_NEW_TOKENS)  # (both captured graphs replayed, clocks up: set-up, outside every timed window)
    graph.step_one()
    torch.cuda.synchronize()
    return graph, run_steps


def in_graph(dev, steps, warmup, repeats):
    import torch
    from guidedquant_amd.APLinear import APLinear
    from guidedquant_amd.generate import random_init_
    from guidedquant_amd.model import ModelArgs, Transformer
    torch.manual_seed(1234)
    model = Transformer(torch.float16, ModelArgs(**timed_config()), linear_class=APLinear, linear_kwargs=dict(bitwidth=2, device=dev))
    model = random_init_(model.to(device=dev, dtype=torch.float16)).eval()
    model.setup_caches(1, SEQ_NEW_TOKENS + 1)
    assert model.native_ready(), "the fused HIP decode step does not serve this model"
    legs = {rp: make_runner(model, dev, rp) for rp in (1.0, 1.05)}
    vals = {rp: [] for rp in legs}
    for _ in range(repeats):
        for rp, (graph, run_steps) in legs.items():  # alternating: a drift of the box falls on both legs
            run_steps(warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_steps(steps)
            torch.cuda.synchronize()
            vals[rp].append(steps / (time.perf_counter() - t0))
    for g, _ in legs.values():
        g.close()
    rec = dict(model=model.config.model_name, n_layer=model.config.n_layer, vocab_size_timed=model.config.vocab_size)
    for rp, v in vals.items():
        rec["rp_%g" % rp] = dict(tok_s=[round(x, 2) for x in v], best=round(max(v), 2), median=round(statistics.median(v), 2),
                                 us_per_token_median=round(1e6 / statistics.median(v), 2))
    a, b = rec["rp_1"]["us_per_token_median"], rec["rp_1.05"]["us_per_token_median"]
    rec["penalty_us_per_token"] = round(b - a, 2)
    rec["penalty_per_cent"] = round(100.0 * (b - a) / a, 2)
    del legs, model
    torch.cuda.empty_cache()
    return rec


def module_tree(dev, new_tokens=100):
    import torch
    import transformers
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    c = timed_config()
    cfg = transformers.Qwen2Config(hidden_size=c["dim"], intermediate_size=c["intermediate_size"], num_hidden_layers=c["n_layer"],
                                   num_attention_heads=c["n_head"], num_key_value_heads=c["n_local_heads"], vocab_size=c["vocab_size"],
                                   max_position_embeddings=c["block_size"], rms_norm_eps=c["norm_eps"], tie_word_embeddings=False)
    names = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]
    cfg.anyprec = dict(seed_precision=2, parent_precision=2, group_count=1, arch_config=dict(module_names=names, model_name="model", layers_name="layers"))
    m = AnyPrecisionForCausalLM.from_config_random(cfg, device=dev, seed=0)
    m.model.generation_config.repetition_penalty = 1.05  # (as the published Qwen2.5-Instruct generation_config.json)
    ids = torch.tensor([[1]], device=dev)

    def timed(**kw):
        m.generate(ids, max_new_tokens=8, min_new_tokens=8, do_sample=False, pad_token_id=0, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = m.generate(ids, max_new_tokens=new_tokens, min_new_tokens=new_tokens, do_sample=False, pad_token_id=0, **kw)
        torch.cuda.synchronize()
        return round((out.shape[1] - 1) / (time.perf_counter() - t0), 2)

    rec = dict(repetition_penalty=1.05, module_tree_tok_s=timed(native=False), generate_plain_tok_s=timed())
    rec["plain_call_on_fused_route"] = ("decoder", 2) in m._native_cache
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-module-tree", action="store_true")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU (the HIP path has no fallback)"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rec = dict(protocol="random init, 2-bit, DecodeGraph with %d steps per replay, embedding folded, greedy top_k 32, sequences of %d new tokens; "
               "%d alternating windows of %d token steps per leg behind %d warm-up steps, host clock ending in a synchronise; module tree: "
               "generate(), 100 new tokens after an 8-token warm-up call" % (SPR, SEQ_NEW_TOKENS, args.repeats, args.steps, args.warmup),
               in_graph=in_graph(dev, args.steps, args.warmup, args.repeats))
    if not args.no_module_tree:
        rec["hf_generate"] = module_tree(dev)
        assert rec["hf_generate"]["plain_call_on_fused_route"]
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
