"""What the top-n alternatives cost inside the captured decode step (DecodeGraph(logprobs=True, top_logprobs=n): gq_sample_topk_lp_topn in
place of gq_sample_topk_lp -- the same two launches of the draw, and the two launches of csrc/topn.hip behind them).

Random-init Llama-3.1-8B geometry at 2 bits (128256 logits), the protocol of tools/decode_logprobs_timing.py: ten token steps per replay,
embedding folded into the sampler, greedy top_k 32, sequences of 100 new tokens from a BOS prompt.

THREE graphs over ONE model in ONE process, timed in alternating windows, each window a host clock around `steps` token steps that ends
in a device synchronise, behind `warmup` untimed steps; per leg the windows' tokens/s, the best, the median and the spread:
  logprobs  logprobs=True (gq_sample_topk_lp) -- the yardstick: the graph a caller of log-probabilities replays today
  top5      the same with top_logprobs=5
  top20     the same with top_logprobs=20
and the difference of each top leg's median from the yardstick's in us per token and in per cent.  Before the windows every graph decodes
one sequence from the same state: the tokens and lp_raw must be equal bit for bit (the draw is the same), every greedy token must head its
list with lp_raw's bits, and the first five of the list of 20 must be the list of 5.

Writes profiles/top_logprobs.json (--out: elsewhere) and prints the record.
    python tools/top_logprobs_timing.py [--steps 400] [--warmup 40] [--repeats 7] [--out PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LLAMA = "meta-llama/Meta-Llama-3.1-8B"
OUT = os.path.join(ROOT, "profiles", "top_logprobs.json")
SEQ_NEW_TOKENS, SPR = 100, 10
LEGS = {"logprobs": 0, "top5": 5, "top20": 20}


def make_runner(model, dev, n):
    """(graph, run_steps) of the leg with top_logprobs = n"""
    import torch
    from guidedquant_amd.generate import DecodeGraph
    graph = DecodeGraph(model, dev, native_sampling=True, temperature=0.0, top_k=32, fold_embed=True, steps_per_replay=SPR,
                        seq_capacity=SEQ_NEW_TOKENS + 2, logprobs=True, top_logprobs=n)
    assert graph.native_sampling and graph.lp_raw is not None and (graph.top_ids is not None) == (n > 0)
    bos = torch.tensor([[128000]], dtype=torch.int32, device=dev)
    zero = torch.zeros((1, ), dtype=torch.int32, device=dev)

    def run_steps(k_total):
        done = 0
        while done < k_total:
            graph.set_token(bos, zero)
            k = min(SEQ_NEW_TOKENS, k_total - done)
            for _ in range(k // SPR):
                graph.step()
            for _ in range(k % SPR):
                graph.step_one()
            done += k

    run_steps(2 * SEQ_NEW_TOKENS)  # (both captured graphs of the leg replayed, clocks up: set-up, outside every timed window)
    graph.step_one()
    torch.cuda.synchronize()
    return graph, run_steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU (the HIP path has no fallback)"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from guidedquant_amd.APLinear import APLinear
    from guidedquant_amd.generate import random_init_
    from guidedquant_amd.model import ModelArgs, Transformer, transformer_configs
    torch.manual_seed(1234)
    model = Transformer(torch.float16, ModelArgs(**transformer_configs[LLAMA]), linear_class=APLinear, linear_kwargs=dict(bitwidth=2, device=dev))
    model = random_init_(model.to(device=dev, dtype=torch.float16)).eval()
    model.setup_caches(1, SEQ_NEW_TOKENS + 1)
    assert model.native_ready(), "the fused HIP decode step does not serve this model"
    legs = {leg: make_runner(model, dev, n) for leg, n in LEGS.items()}
    # the same sequence from every graph: equal tokens and lp_raw; the lists agree with the draw and with each other
    seqs, raws = {}, {}
    sl = slice(1, SEQ_NEW_TOKENS + 1)
    for leg, (graph, run_steps) in legs.items():
        graph.rng_counter.zero_()
        run_steps(SEQ_NEW_TOKENS)
        torch.cuda.synchronize()
        seqs[leg], raws[leg] = graph.seq[sl].clone(), graph.lp_raw[sl].clone()
        assert torch.equal(seqs[leg], seqs["logprobs"]) and torch.equal(raws[leg].view(torch.int32), raws["logprobs"].view(torch.int32)), "the graphs differ in the draw"
        if graph.top_ids is not None:
            assert torch.equal(graph.top_ids[sl, 0], graph.seq[sl]), "a greedy token does not head its list"
            assert torch.equal(graph.top_lps[sl, 0].view(torch.int32), graph.lp_raw[sl].view(torch.int32)), "the drawn token's entry is not lp_raw"
    g5, g20 = legs["top5"][0], legs["top20"][0]
    assert torch.equal(g20.top_ids[sl, :5], g5.top_ids[sl]) and torch.equal(g20.top_lps[sl, :5].view(torch.int32), g5.top_lps[sl].view(torch.int32))
    mass20 = float(g20.top_lps[sl].double().exp().sum(dim=1).mean())
    vals = {leg: [] for leg in legs}
    for _ in range(args.repeats):
        for leg, (graph, run_steps) in legs.items():  # alternating: a drift of the box falls on every leg
            run_steps(args.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_steps(args.steps)
            torch.cuda.synchronize()
            vals[leg].append(args.steps / (time.perf_counter() - t0))
    for graph, _ in legs.values():
        graph.close()
    rec = dict(protocol="random init, 2-bit, DecodeGraph with %d steps per replay, embedding folded, greedy top_k 32, logprobs=True, seq_capacity %d, sequences "
               "of %d new tokens; %d alternating windows of %d token steps per leg behind %d warm-up steps, host clock ending in a synchronise"
               % (SPR, SEQ_NEW_TOKENS + 2, SEQ_NEW_TOKENS, args.repeats, args.steps, args.warmup),
               model=model.config.model_name, n_layer=model.config.n_layer, vocab_size=model.config.vocab_size, same_tokens_and_lp_raw=True,
               mean_mass_of_the_top_20=round(mass20, 4))
    for leg, v in vals.items():
        rec[leg] = dict(tok_s=[round(x, 2) for x in v], best=round(max(v), 2), median=round(statistics.median(v), 2),
                        spread_per_cent=round(100.0 * (max(v) - min(v)) / statistics.median(v), 3), us_per_token_median=round(1e6 / statistics.median(v), 2))
    a = rec["logprobs"]["us_per_token_median"]
    for leg in ("top5", "top20"):
        b = rec[leg]["us_per_token_median"]
        rec[leg + "_us_per_token"] = round(b - a, 2)
        rec[leg + "_per_cent"] = round(100.0 * (b - a) / a, 2)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
