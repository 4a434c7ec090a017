"""What per-token log-probabilities cost inside the captured decode step (DecodeGraph(logprobs=True): gq_sample_topk_lp in place of
gq_sample_topk_p -- the same two launches, a log-sum-exp over the vocabulary added to them).

Random-init Llama-3.1-8B geometry at 2 bits (128256 logits), bench.py's headline protocol restated for a DecodeGraph that keeps the
sequence: ten token steps per replay, embedding folded into the sampler, greedy top_k 32, sequences of 100 new tokens from a BOS prompt.

THREE graphs over ONE model in ONE process, timed in alternating windows, each window a host clock around `steps` token steps that ends
in a device synchronise, behind `warmup` untimed steps; per leg the windows' tokens/s, the best and the median:
  logprobs_off  the plain graph (gq_sample_topk_p: fp16 selection keys)
  logprobs_on   logprobs=True (gq_sample_topk_lp without a penalty or a token set: the fp16 keys of the plain draw, and the two numbers)
  rep_draw      no logprobs, suppress_tokens=[0] (gq_sample_topk_rep: fp32 values, u64 keys -- the form of the draw gq_sample_topk_lp
                takes with a penalty or a set; its distance from the plain graph is what such a request pays for the draw alone)
and the difference of the medians of the first two in us per token and in per cent.  Before the windows the first two graphs decode one
sequence from the same state: the tokens must be equal (the draw is the same), and the log-probabilities of the second graph finite.

Writes profiles/decode_logprobs.json and prints the record.
    python tools/decode_logprobs_timing.py [--steps 400] [--warmup 40] [--repeats 7]
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
OUT = os.path.join(ROOT, "profiles", "decode_logprobs.json")
SEQ_NEW_TOKENS, SPR = 100, 10


def make_runner(model, dev, leg):
    """bench.decode_tok_s for a graph that keeps the sequence (and, on one leg, its log-probabilities): (graph, run_steps)"""
    import torch
    from guidedquant_amd.generate import DecodeGraph
    graph = DecodeGraph(model, dev, native_sampling=True, temperature=0.0, top_k=32, fold_embed=True, steps_per_replay=SPR,
                        seq_capacity=SEQ_NEW_TOKENS + 2, **{"logprobs_on": {"logprobs": True}, "rep_draw": {"suppress_tokens": [0]}}.get(leg, {}))
    assert graph.native_sampling and (graph.lp_raw is not None) == (leg == "logprobs_on") and (graph.seen is not None) == (leg == "rep_draw")
    bos = torch.tensor([[128000]], dtype=torch.int32, device=dev)
    zero = torch.zeros((1, ), dtype=torch.int32, device=dev)

    def run_steps(n):
        done = 0
        while done < n:
            graph.set_token(bos, zero)
            graph.set_history(bos.view(-1))  # (one small launch per 100 tokens on the rep_draw leg; nothing on the others)
            k = min(SEQ_NEW_TOKENS, n - done)
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
    legs = {leg: make_runner(model, dev, leg) for leg in ("logprobs_off", "logprobs_on", "rep_draw")}
    # the same sequence from both graphs: equal tokens, finite log-probabilities
    seqs = {}
    for leg in ("logprobs_off", "logprobs_on"):
        graph, run_steps = legs[leg]
        graph.rng_counter.zero_()
        run_steps(SEQ_NEW_TOKENS)
        torch.cuda.synchronize()
        seqs[leg] = graph.seq[1:SEQ_NEW_TOKENS + 1].clone()
    assert torch.equal(seqs["logprobs_off"], seqs["logprobs_on"]), "the two graphs drew different tokens"
    g = legs["logprobs_on"][0]
    raw, drawn = g.lp_raw[1:SEQ_NEW_TOKENS + 1], g.lp_drawn[1:SEQ_NEW_TOKENS + 1]
    assert bool(torch.isfinite(raw).all()) and bool((raw <= 0).all()) and bool(torch.isfinite(drawn).all()) and bool((drawn <= 0).all())
    vals = {leg: [] for leg in legs}
    for _ in range(args.repeats):
        for lp, (graph, run_steps) in legs.items():  # alternating: a drift of the box falls on every leg
            run_steps(args.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_steps(args.steps)
            torch.cuda.synchronize()
            vals[lp].append(args.steps / (time.perf_counter() - t0))
    for graph, _ in legs.values():
        graph.close()
    rec = dict(protocol="random init, 2-bit, DecodeGraph with %d steps per replay, embedding folded, greedy top_k 32, seq_capacity %d, sequences of %d "
               "new tokens; %d alternating windows of %d token steps per leg behind %d warm-up steps, host clock ending in a synchronise"
               % (SPR, SEQ_NEW_TOKENS + 2, SEQ_NEW_TOKENS, args.repeats, args.steps, args.warmup),
               model=model.config.model_name, n_layer=model.config.n_layer, vocab_size=model.config.vocab_size, same_tokens=True,
               mean_logprob_of_the_sequence=round(float(raw.mean()), 4))
    for lp, v in vals.items():
        rec[lp] = dict(tok_s=[round(x, 2) for x in v], best=round(max(v), 2), median=round(statistics.median(v), 2),
                       us_per_token_median=round(1e6 / statistics.median(v), 2))
    a, b = rec["logprobs_off"]["us_per_token_median"], rec["logprobs_on"]["us_per_token_median"]
    rec["logprobs_us_per_token"] = round(b - a, 2)
    rec["logprobs_per_cent"] = round(100.0 * (b - a) / a, 2)
    rec["rep_draw_us_per_token"] = round(rec["rep_draw"]["us_per_token_median"] - a, 2)
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
