"""What packing buys lm-eval's request shape: `AnyPrecisionForCausalLM.loglikelihood` in a loop (one prompt pass per pair) against
`loglikelihood_many` (first-fit packs, one pass per pack) on the Llama-3.1-8B geometry, random init, 2 bits -- 256 (context,
continuation) pairs, total lengths drawn once from 32..256 and continuation lengths from 1..16 with a fixed seed.  The two variants
alternate in one process for `--rounds` rounds behind a warm-up of both (the first `--warm` pairs); a round is the whole set, timed by
the host clock around calls that end in host values, with a device synchronise in front and behind.

Per variant: sequences/s and tokens/s (median round; tokens = every token of every pair), the rounds' seconds (the spread), and the peak
of torch.cuda.max_memory_allocated over a round above what was allocated in front of the first round (the model and its caches).
The worst |difference| of the two variants' log-likelihoods is recorded next to the times.  No threshold is asserted: the record says
what came out.
    python tools/score_packed_timing.py [--rounds 3] [--pairs 256] [--pack-tokens N] [--layers N] [--out profiles/score_packed.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--warm", type=int, default=24)
    ap.add_argument("--pack-tokens", type=int, default=None, help="rows per pack (default: the library's, min(GQ_PREFILL_CHUNK, context))")
    ap.add_argument("--layers", type=int, default=32, help="fewer layers than the geometry's 32 (a quick look; the record says so)")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "score_packed.json"))
    args = ap.parse_args()
    import torch
    import transformers
    assert torch.cuda.is_available(), "needs a GPU (the HIP path has no fallback)"
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    hf = transformers.LlamaConfig(hidden_size=4096, intermediate_size=14336, num_hidden_layers=args.layers, num_attention_heads=32, num_key_value_heads=8,
                                  vocab_size=128256, max_position_embeddings=8192, rms_norm_eps=1e-5, rope_theta=500000.0, tie_word_embeddings=False)
    names = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]
    hf.anyprec = dict(seed_precision=2, parent_precision=2, group_count=1, arch_config=dict(module_names=names, model_name="model", layers_name="layers"))
    m = AnyPrecisionForCausalLM.from_config_random(hf, device=dev, seed=1234)

    g = torch.Generator().manual_seed(20)
    lens = torch.randint(32, 257, (args.pairs, ), generator=g).tolist()
    conts = torch.randint(1, 17, (args.pairs, ), generator=g).tolist()
    pairs = []
    for n, k in zip(lens, conts):
        ids = torch.randint(0, hf.vocab_size, (n, ), generator=g)
        pairs.append((ids[:n - k], ids[n - k:]))
    tokens = sum(lens)

    def loop(ps):
        return [m.loglikelihood(c, t, native=True) for c, t in ps]

    def many(ps):
        return m.loglikelihood_many(ps, pack_tokens=args.pack_tokens, native=True)

    variants = (("loglikelihood loop", loop), ("loglikelihood_many", many))
    for _, fn in variants:  # warm-up: code objects, the decoder, caches of both variants' sizes
        fn(pairs[:args.warm])
    many(pairs)  # (the packs' own shapes: the GEMM routes of a full pack)
    torch.cuda.synchronize()
    dec = m._native_cache[("decoder", 2)]
    base = torch.cuda.memory_allocated()
    rec = dict(protocol="random init, 2-bit, Llama-3.1-8B geometry (%d layers); %d pairs, total lengths 32..256 (sum %d tokens), continuations 1..16, "
               "seed 20; loglikelihood in a loop and loglikelihood_many alternating, %d rounds behind a warm-up of both; host clock around the whole "
               "set between device synchronises; peak_bytes: max_memory_allocated over a round above the allocation in front of the first round"
               % (args.layers, args.pairs, tokens, args.rounds), pairs=args.pairs, tokens=tokens, pack_tokens=args.pack_tokens, variants={})
    secs, peaks, results = {n: [] for n, _ in variants}, {n: 0 for n, _ in variants}, {}
    for r in range(args.rounds):
        for name, fn in variants:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            results[name] = fn(pairs)
            torch.cuda.synchronize()
            secs[name].append(round(time.perf_counter() - t0, 4))
            peaks[name] = max(peaks[name], int(torch.cuda.max_memory_allocated() - base))
            print(json.dumps(dict(round=r, variant=name, seconds=secs[name][-1])), flush=True)
    for name, _ in variants:
        med = statistics.median(secs[name])
        rec["variants"][name] = dict(seconds=secs[name], sequences_per_s=round(args.pairs / med, 1), tokens_per_s=round(tokens / med, 1),
                                     spread=round((max(secs[name]) - min(secs[name])) / med, 4), peak_bytes=peaks[name])
    rec["last_packed_plan"] = dict(dec.last_prefill_plan, chunks=[list(c) for c in dec.last_prefill_plan["chunks"]])
    a, b = results["loglikelihood loop"], results["loglikelihood_many"]
    rec["worst_abs_difference_of_loglikelihoods"] = max(abs(x[0] - y[0]) for x, y in zip(a, b))
    rec["greedy_flags_that_differ"] = sum(1 for x, y in zip(a, b) if x[1] != y[1])
    rec["speedup_median"] = round(statistics.median(secs["loglikelihood loop"]) / statistics.median(secs["loglikelihood_many"]), 3)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
