"""What the top-n list of the scoring head costs: gq_head_nll (no list) against gq_head_nll_topn at n = 5 and n = 20 and against what a
caller had to write without it -- the logits head on all S rows, float, log_softmax, gather and topk(20) in torch -- on the Llama-3.1-8B
geometry, random init, 2 bits, at S = 2048 and 4096 rows.  tools/score_timing.py's protocol for the head alone: the legs alternate in
one process, `--rounds` windows per leg and size, each window `--launches` calls between two events behind 5 warm-up calls.
  head_ms     per call, one figure per window; the record adds the median and the spread (min, max) over the windows of a leg;
  peak_bytes  torch.cuda.max_memory_allocated over one call above what was allocated in front of it (the model, the rows).
The head reads the final norm and output.weight only, so the model is built with `--layers` layers (default 1).  No threshold is
asserted: the record says what came out.
    python tools/score_topn_timing.py [--rounds 5] [--launches 20] [--out profiles/score_head_topn.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (2048, 4096)
LEGS = ("hip-nll", "hip-nll-top5", "hip-nll-top20", "torch-topk20")


def call(model, x, targets, leg):
    import torch
    if leg == "torch-topk20":
        ls = torch.log_softmax(model.output(model.norm(x)).float(), dim=-1)
        return ls.gather(1, targets.long().clamp(min=0)[:, None]), ls.topk(20, dim=-1)
    return model._score_head(x, targets, True, {"hip-nll": 0, "hip-nll-top5": 5, "hip-nll-top20": 20}[leg])


def window(model, x, targets, leg, launches):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        for i in range(launches + 5):
            if i == 5:
                e0.record()
            call(model, x, targets, leg)
        e1.record()
        torch.cuda.synchronize()
        ms = round(e0.elapsed_time(e1) / launches, 3)
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        call(model, x, targets, leg)
        torch.cuda.synchronize()
    return ms, int(torch.cuda.max_memory_allocated() - base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--layers", type=int, default=1)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "score_head_topn.json"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU (the HIP path has no fallback)"
    from guidedquant_amd.APLinear import APLinear
    from guidedquant_amd.generate import random_init_
    from guidedquant_amd.model import ModelArgs, Transformer, transformer_configs
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(1234)
    cfg = ModelArgs(**dict(transformer_configs["meta-llama/Meta-Llama-3.1-8B"], block_size=max(SIZES), n_layer=args.layers))
    model = Transformer(torch.float16, cfg, linear_class=APLinear, linear_kwargs=dict(bitwidth=2, device=dev))
    model = random_init_(model.to(device=dev, dtype=torch.float16)).eval()
    rec = dict(protocol="random init, 2-bit, Llama-3.1-8B geometry (dim %d, vocabulary %d; %d layer(s): the head reads the final norm and output.weight only); "
               "legs alternating in one process, %d windows per leg and size, each %d calls between two events behind 5 warm-up calls; peak_bytes: "
               "max_memory_allocated of one call above the allocation in front of it" % (cfg.dim, cfg.vocab_size, cfg.n_layer, args.rounds, args.launches),
               sizes=list(SIZES), legs={leg: {"S_%d" % S: dict(head_ms=[], peak_bytes=0) for S in SIZES} for leg in LEGS})
    g = torch.Generator(device=dev).manual_seed(5)
    rows = {}
    for S in SIZES:
        idx = torch.randint(0, cfg.vocab_size, (S, ), dtype=torch.int32, device=dev, generator=g)
        rows[S] = (torch.randn(S, cfg.dim, device=dev, generator=g).half(), torch.cat([idx[1:], torch.full((1, ), -1, dtype=torch.int32, device=dev)]))
    for r in range(args.rounds):
        for leg in LEGS:
            for S in SIZES:
                ms, peak = window(model, *rows[S], leg, args.launches)
                cell = rec["legs"][leg]["S_%d" % S]
                cell["head_ms"].append(ms)
                cell.update(peak_bytes=peak, median_ms=statistics.median(cell["head_ms"]), spread_ms=[min(cell["head_ms"]), max(cell["head_ms"])])
            print(json.dumps({"round": r, "leg": leg, **{k: v["head_ms"][-1] for k, v in rec["legs"][leg].items()}}), flush=True)
        with open(args.out, "w") as f:  # (written round by round: a run cut short leaves what it measured)
            json.dump(rec, f, indent=1)
            f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
