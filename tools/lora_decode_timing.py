"""What a LoRA adapter beside the quantized base costs on the fused decode route: the Llama-3.1-8B geometry, random init, 2 bits, three legs
alternating in one process (`--rounds` rounds of each):

  none     no adapter: the 5 launches per layer
  qv       r = 16 on q_proj, v_proj (peft's default targets): 2 side launches per layer (gq_lora_down, gq_lora_up) and the bias form of the
           attention launch instead of the forms that rotate inside the wqkv launch
  all      r = 16 on q, k, v, o, down: 6 side launches per layer

tok_s: in-graph decode (captured DecodeGraph, ten token steps per replay, fused sampler) from 50 cached positions, `--steps` token steps,
`--repeats` windows per leg and round.  The summary gives each leg's median tokens/s, the microseconds per token it adds to the
adapter-free leg, and the spread of its windows (max - min over median).  No threshold is asserted and no speed is promised: the record says
what came out.  Writes profiles/lora_decode.json.
    python tools/lora_decode_timing.py [--rounds 3] [--steps 200] [--warmup 50] [--repeats 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "lora_decode.json")
MAX_SEQ, POS, RANK, ALPHA = 1024, 50, 16, 32
LEGS = dict(none=(), qv=("q_proj", "v_proj"), all=("q_proj", "k_proj", "v_proj", "o_proj", "down_proj"))


def random_peft(c, targets, r=16, lora_alpha=32, seed=0, b_std=0.01):
    """(state dict in peft's key layout, adapter config) of a random adapter for the geometry `c` (ModelArgs): this tool's legs and the tests';
    b_std = 0 is a fresh adapter (B all zero)"""
    nq, nkv = c.n_head * c.head_dim, c.n_local_heads * c.head_dim
    shapes = dict(q_proj=(nq, c.dim), k_proj=(nkv, c.dim), v_proj=(nkv, c.dim), o_proj=(c.dim, nq), down_proj=(c.dim, c.intermediate_size))
    import torch
    g, sd = torch.Generator().manual_seed(seed), {}
    for layer in range(c.n_layer):
        for name in targets:
            n_out, n_in = shapes[name]
            base = f"base_model.model.model.layers.{layer}.{'mlp' if name == 'down_proj' else 'self_attn'}.{name}"
            sd[base + ".lora_A.weight"] = (torch.randn(r, n_in, generator=g) * n_in**-0.5).half().float()
            sd[base + ".lora_B.weight"] = (torch.randn(n_out, r, generator=g) * b_std).half().float()
    return sd, dict(r=r, lora_alpha=lora_alpha, target_modules=list(targets))


def adapter(cfg, targets, dev):
    from guidedquant_amd.lora import LoraAdapter
    return LoraAdapter.from_peft(*random_peft(cfg, targets, RANK, ALPHA, seed=7), cfg, dev)


def tok_s(model, dev, steps, warmup, repeats):
    import torch
    from guidedquant_amd.generate import DecodeGraph
    spr = 10
    assert steps % spr == 0 and warmup % spr == 0 and POS + warmup + steps < model.max_seq_length
    graph = DecodeGraph(model, dev, native_sampling=True, temperature=0.0, top_k=32, fold_embed=True, steps_per_replay=spr)
    vals = []
    for _ in range(repeats):
        graph.set_token(1, POS)
        for _ in range(warmup // spr):
            graph.step()
        graph.set_token(1, POS)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps // spr):
            graph.step()
        torch.cuda.synchronize()
        vals.append(round(steps / (time.perf_counter() - t0), 2))
    graph.close()
    return vals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU (the HIP path has no fallback)"
    from guidedquant_amd.APLinear import APLinear
    from guidedquant_amd.generate import random_init_
    from guidedquant_amd.model import ModelArgs, Transformer, transformer_configs
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(1234)
    cfg = ModelArgs(**dict(transformer_configs["meta-llama/Meta-Llama-3.1-8B"], block_size=MAX_SEQ))
    model = Transformer(torch.float16, cfg, linear_class=APLinear, linear_kwargs=dict(bitwidth=2, device=dev))
    model = random_init_(model.to(device=dev, dtype=torch.float16)).eval()
    model.setup_caches(1, MAX_SEQ)
    adapters = {name: adapter(cfg, t, dev) if t else None for name, t in LEGS.items()}
    rec = dict(protocol="random init, 2-bit, Llama-3.1-8B geometry, cache of %d rows, rank %d, from %d cached positions; legs alternating, %d rounds; "
               "DecodeGraph with 10 steps per replay, %d warm-up steps, %d-step window, %d windows per leg and round"
               % (MAX_SEQ, RANK, POS, args.rounds, args.warmup, args.steps, args.repeats),
               not_measured="every other geometry (70B, Qwen2 / Qwen3, window layers), 3- to 8-bit bases, ranks other than 16, long contexts",
               rounds=[])
    for r in range(args.rounds):
        for name in LEGS:
            model.set_adapter(adapters[name])
            assert model.native_ready()
            leg = dict(round=r, leg=name, targets=list(LEGS[name]), tok_s=tok_s(model, dev, args.steps, args.warmup, args.repeats))
            rec["rounds"].append(leg)
            print(json.dumps(leg), flush=True)
    windows = {name: [v for leg in rec["rounds"] if leg["leg"] == name for v in leg["tok_s"]] for name in LEGS}
    med = {name: statistics.median(v) for name, v in windows.items()}
    rec["summary"] = {name: dict(tok_s_median=med[name], us_per_token_over_none=round(1e6 / med[name] - 1e6 / med["none"], 1),
                                 window_spread=round((max(v) - min(v)) / med[name], 4)) for name, v in windows.items()}
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["summary"]))


if __name__ == "__main__":
    main()
