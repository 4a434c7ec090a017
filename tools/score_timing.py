"""What the scoring head costs: the kernel gq_head_nll (csrc/head_nll.hip) against the torch head (lm_head GEMM -> float -> log_softmax ->
gather / argmax in blocks of 512 rows) on the Llama-3.1-8B geometry, random init, 2 bits, at S = 2048 and 4096 rows -- the two heads
alternating in one process (`--rounds` rounds of torch, kernel):

  head_ms     `Transformer._score_head` alone on S residual rows, `--launches` calls between two events behind a warm-up;
  score_ms    the whole `Transformer.score_native` pass (32 layers + head) under GQ_SCORE_HEAD=0 / 1, `--runs` timed runs behind a warm-up;
  peak_bytes  torch.cuda.max_memory_allocated over one pass, above what was allocated before it (the pass's own intermediates).
No threshold is asserted: the record says what came out.  The default of GQ_SCORE_HEAD=auto (Transformer.SCORE_HEAD_AUTO) follows it by
the house rule: the kernel only if its head_ms is no larger than the torch head's at both sizes.
    python tools/score_timing.py [--rounds 4] [--launches 50] [--runs 5] [--out profiles/score_head.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (2048, 4096)


def head_ms(model, x, targets, kernel, launches):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        for i in range(launches + 5):
            if i == 5:
                e0.record()
            model._score_head(x, targets, kernel)
        e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / launches, 3)


def score_ms(model, idx, runs):
    import torch
    vals = []
    with torch.no_grad():
        for i in range(runs + 1):  # (the first run warms up)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            model.score_native(idx)
            e1.record()
            torch.cuda.synchronize()
            if i:
                vals.append(round(e0.elapsed_time(e1), 2))
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        model.score_native(idx)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
    return vals, int(peak), model.last_prefill_plan["head"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--layers", type=int, default=None, help="fewer layers than the geometry's 32 (a quick look; the record says so)")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "score_head.json"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU (the HIP path has no fallback)"
    from guidedquant_amd.APLinear import APLinear
    from guidedquant_amd.generate import random_init_
    from guidedquant_amd.model import ModelArgs, Transformer, transformer_configs
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(1234)
    geo = dict(transformer_configs["meta-llama/Meta-Llama-3.1-8B"], block_size=max(SIZES))
    if args.layers:
        geo["n_layer"] = args.layers
    cfg = ModelArgs(**geo)
    model = Transformer(torch.float16, cfg, linear_class=APLinear, linear_kwargs=dict(bitwidth=2, device=dev))
    model = random_init_(model.to(device=dev, dtype=torch.float16)).eval()
    model.setup_caches(1, max(SIZES))
    assert model.native_ready()
    rec = dict(protocol="random init, 2-bit, Llama-3.1-8B geometry (%d layers, dim %d, vocabulary %d); torch head and kernel head alternating, %d rounds; "
               "head_ms: Transformer._score_head on S rows, %d calls between two events behind 5 warm-up calls; score_ms: score_native, %d timed "
               "runs behind a warm-up; peak_bytes: max_memory_allocated of one pass above the allocation in front of it"
               % (cfg.n_layer, cfg.dim, cfg.vocab_size, args.rounds, args.launches, args.runs), sizes=list(SIZES), rounds=[])
    g = torch.Generator(device=dev).manual_seed(5)
    for r in range(args.rounds):
        for head in ("0", "1"):
            os.environ["GQ_SCORE_HEAD"] = head
            leg = dict(round=r, head="hip-nll" if head == "1" else "torch")
            for S in SIZES:
                idx = torch.randint(0, cfg.vocab_size, (S, ), dtype=torch.int32, device=dev, generator=g)
                x = torch.randn(S, cfg.dim, device=dev, generator=g).half()
                targets = torch.cat([idx[1:], torch.full((1, ), -1, dtype=torch.int32, device=dev)])
                h = head_ms(model, x, targets, head == "1", args.launches)
                s, peak, took = score_ms(model, idx, args.runs)
                assert took == leg["head"]
                leg["S_%d" % S] = dict(head_ms=h, score_ms=s, peak_bytes=peak)
            rec["rounds"].append(leg)
            print(json.dumps(leg), flush=True)
            with open(args.out, "w") as f:  # (written leg by leg: a run cut short leaves what it measured)
                json.dump(rec, f, indent=1)
                f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
