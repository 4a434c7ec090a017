"""What scoring through the int8 lm_head costs and how far it moves the numbers: gq_head_nll against gq_head_nll_i8, both _topn forms at
n = 5 and n = 20, and the whole `Transformer.score_native` pass with either head, on the Llama-3.1-8B geometry, random init, 2 bits, at
S = 2048 and 4096 rows.  tools/score_timing.py's protocol: the legs alternate in one process, `--rounds` windows per leg and size, a
head window is `--launches` calls between two events behind 5 warm-up calls, a pass window `--runs` timed runs behind one warm-up run.
  head_ms / score_ms   per call, one figure per window; the record adds the median and the spread (min, max) over a leg's windows;
  delta                on the random-init head, per size: rms and max of |logprob(int8) - logprob(fp16)| over the rows of one pass, and
                       the share of rows on which the two heads agree about the greedy flag.
No threshold is asserted: the record says what came out.
    python tools/score_head_q8_timing.py [--rounds 5] [--launches 20] [--runs 3] [--layers 32] [--out profiles/score_head_q8.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (2048, 4096)
HEAD_LEGS = {"%s%s" % (h, "-top%d" % n if n else ""): (h == "int8", n) for n in (0, 5, 20) for h in ("fp16", "int8")}


def head_ms(model, x, targets, q8, top_n, launches):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        for i in range(launches + 5):
            if i == 5:
                e0.record()
            model._score_head(x, targets, True, top_n, q8)
        e1.record()
        torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / launches, 3)


def score_ms(model, idx, head, runs):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        for i in range(runs + 1):  # (the first run warms up)
            if i == 1:
                e0.record()
            out = model.score_native(idx, lm_head_dtype=head)
        e1.record()
        torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / runs, 3), out


def add(cell, key, ms):
    cell[key].append(ms)
    cell.update(median_ms=statistics.median(cell[key]), spread_ms=[min(cell[key]), max(cell[key])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "score_head_q8.json"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU (the HIP path has no fallback)"
    from guidedquant_amd.APLinear import APLinear
    from guidedquant_amd.generate import random_init_
    from guidedquant_amd.model import ModelArgs, Transformer, transformer_configs
    os.environ["GQ_SCORE_HEAD"] = "1"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(1234)
    cfg = ModelArgs(**dict(transformer_configs["meta-llama/Meta-Llama-3.1-8B"], block_size=max(SIZES), n_layer=args.layers))
    model = Transformer(torch.float16, cfg, linear_class=APLinear, linear_kwargs=dict(bitwidth=2, device=dev))
    model = random_init_(model.to(device=dev, dtype=torch.float16)).eval()
    model.setup_caches(1, max(SIZES))
    model.set_lm_head_dtype("int8")  # (the fp16 legs read output.weight as on any model)
    rec = dict(protocol="random init, 2-bit, Llama-3.1-8B geometry (%d layers, dim %d, vocabulary %d); legs alternating in one process, %d windows per "
               "leg and size; head_ms: Transformer._score_head on S rows, %d calls between two events behind 5 warm-up calls; score_ms: score_native, "
               "%d timed runs behind a warm-up run" % (cfg.n_layer, cfg.dim, cfg.vocab_size, args.rounds, args.launches, args.runs), sizes=list(SIZES),
               head={leg: {"S_%d" % S: dict(head_ms=[]) for S in SIZES} for leg in HEAD_LEGS},
               score={h: {"S_%d" % S: dict(score_ms=[]) for S in SIZES} for h in ("fp16", "int8")}, delta={})
    g = torch.Generator(device=dev).manual_seed(5)
    rows, ids = {}, {}
    for S in SIZES:
        ids[S] = torch.randint(0, cfg.vocab_size, (S, ), dtype=torch.int32, device=dev, generator=g)
        rows[S] = (torch.randn(S, cfg.dim, device=dev, generator=g).half(), torch.cat([ids[S][1:], torch.full((1, ), -1, dtype=torch.int32, device=dev)]))
    for r in range(args.rounds):
        for leg, (q8, top_n) in HEAD_LEGS.items():
            for S in SIZES:
                add(rec["head"][leg]["S_%d" % S], "head_ms", head_ms(model, *rows[S], q8, top_n, args.launches))
            print(json.dumps({"round": r, "head": leg, **{k: v["head_ms"][-1] for k, v in rec["head"][leg].items()}}), flush=True)
        for S in SIZES:
            out = {}
            for h in ("fp16", "int8"):
                ms, out[h] = score_ms(model, ids[S], h, args.runs)
                add(rec["score"][h]["S_%d" % S], "score_ms", ms)
            d = (out["int8"][0].double() - out["fp16"][0].double()).abs()
            rec["delta"]["S_%d" % S] = dict(rms=float(d.pow(2).mean().sqrt()), max=float(d.max()), greedy_agreement=float((out["int8"][1] == out["fp16"][1]).double().mean()),
                                            nll_fp16=float(-out["fp16"][0].double().mean()), nll_int8=float(-out["int8"][0].double().mean()))
            print(json.dumps({"round": r, "S": S, **{h: rec["score"][h]["S_%d" % S]["score_ms"][-1] for h in ("fp16", "int8")}, **rec["delta"]["S_%d" % S]}), flush=True)
        with open(args.out, "w") as f:  # (written round by round: a run cut short leaves what it measured)
            json.dump(rec, f, indent=1)
            f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
