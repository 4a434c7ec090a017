"""What the whole-vocabulary sampler (gq_sample_full, csrc/sampler_full.hip) costs: per draw, next to the two-stage sampler it stands beside,
and per token inside the captured decode step, next to the torch sampling the same request ran through before.

ONE process; the legs of each comparison alternate behind a warm-up.
  draws   us per draw at 128256 and at 151936 logits (N(0, 2) fp16 logits, one stream, `--draws` calls between two events, `--repeats`
          alternating windows, the median): gq_sample_topk_p(top_k=50) and gq_sample_full for
            full                no filter                      top_p09      top_p 0.9
            min_p005            min_p 0.05                     top_k200     top_k 200
            top_k50_min_p       top_k 50 + min_p 0.05          k200_p_pen   top_k 200 + top_p 0.9 + penalty 1.05 (64 seen tokens)
  decode  tokens/s of DecodeGraph on the random-init Llama-3.1-8B geometry at 2 bits for top_k = 200, temperature 0.8:
            native          native_sampling=True with what only native sampling allows -- fold_embed, ten steps per replay: the step ends
                            in gq_sample_full
            native_single   native_sampling=True, no embedding fold, one step per replay: the torch leg's graph shape, so that this leg
                            against `torch` is the sampler alone
            torch           native_sampling=False: torch's top-k / softmax / multinomial ops captured in the graph, one step per replay --
                            what the request ran before
          `--windows` alternating windows of `--steps` token steps behind `--warmup`, host clock ending in a synchronise; per leg the
          windows, the median and the spread (max - min); `native_not_slower` = native median >= torch median - torch spread.

Writes profiles/sampler_full.json and prints the record.
    python tools/sampler_full_timing.py [--draws 200] [--repeats 7] [--steps 300] [--warmup 40] [--windows 5]
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
OUT = os.path.join(ROOT, "profiles", "sampler_full.json")
SETTINGS = {  # name -> (top_k, top_p, min_p, penalty)
    "full": (0, 1.0, 0.0, 1.0), "top_p09": (0, 0.9, 0.0, 1.0), "min_p005": (0, 1.0, 0.05, 1.0), "top_k200": (200, 1.0, 0.0, 1.0),
    "top_k50_min_p": (50, 1.0, 0.05, 1.0), "k200_p_pen": (200, 0.9, 0.0, 1.05),
}


def draw_legs(V, dev):
    """name -> a function that makes one draw on the current stream"""
    import torch
    from guidedquant_amd import _lib
    from guidedquant_amd.fused_sampler import FusedSampler
    g = torch.Generator(device="cpu").manual_seed(V)
    logits = (torch.randn(V, generator=g) * 2).to(torch.float16).to(dev)
    io = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(3)]
    legs = {}
    s0 = FusedSampler(V, dev, 50, top_p=1.0, temperature=0.8)
    legs["topk_p_k50"] = (s0, lambda s=s0: s.launch(logits, *io))
    for name, (k, p, mp, rp) in SETTINGS.items():
        s = FusedSampler(V, dev, k, top_p=p, temperature=0.8, min_p=mp, repetition_penalty=rp)
        assert s.full
        if rp != 1.0:
            s.set_history(torch.randint(0, V, (64, ), generator=g, dtype=torch.int32))
        legs[name] = (s, lambda s=s: s.launch(logits, *io))
    assert _lib.lib().gq_sample_full_ws_bytes(V) > 0
    return legs


def time_draws(V, dev, draws, repeats):
    import torch
    legs = draw_legs(V, dev)
    for _, fn in legs.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    vals = {n: [] for n in legs}
    for _ in range(repeats):
        for n, (_, fn) in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(draws):
                fn()
            b.record()
            b.synchronize()
            vals[n].append(1e3 * a.elapsed_time(b) / draws)
    return {n: dict(us_per_draw=[round(x, 2) for x in v], median=round(statistics.median(v), 2)) for n, v in vals.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU (the HIP path has no fallback)"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rec = dict(protocol="draws: %d calls between two events, %d alternating windows, temperature 0.8, N(0, 2) logits; decode: random init, 2-bit, top_k 200, "
               "temperature 0.8, %d alternating windows of %d token steps behind %d warm-up steps, host clock ending in a synchronise"
               % (args.draws, args.repeats, args.windows, args.steps, args.warmup), draws={})
    for V in (128256, 151936):
        rec["draws"][str(V)] = time_draws(V, dev, args.draws, args.repeats)
    from guidedquant_amd.APLinear import APLinear
    from guidedquant_amd.generate import DecodeGraph, random_init_
    from guidedquant_amd.model import ModelArgs, Transformer, transformer_configs
    torch.manual_seed(1234)
    model = Transformer(torch.float16, ModelArgs(**transformer_configs[LLAMA]), linear_class=APLinear, linear_kwargs=dict(bitwidth=2, device=dev))
    model = random_init_(model.to(device=dev, dtype=torch.float16)).eval()
    new = 100
    model.setup_caches(1, new + 1)
    assert model.native_ready(), "the fused HIP decode step does not serve this model"
    graphs = dict(native=DecodeGraph(model, dev, native_sampling=True, fold_embed=True, steps_per_replay=10, seq_capacity=new + 2, temperature=0.8, top_k=200),
                  native_single=DecodeGraph(model, dev, native_sampling=True, seq_capacity=new + 2, temperature=0.8, top_k=200),
                  torch=DecodeGraph(model, dev, native_sampling=False, temperature=0.8, top_k=200))
    assert all(graphs[n].native_sampling and graphs[n].sampler.full for n in ("native", "native_single")) and not graphs["torch"].native_sampling
    assert graphs["native_single"].steps_per_replay == 1 and not graphs["native_single"].fold_embed
    bos = torch.tensor([[128000]], dtype=torch.int32, device=dev)
    zero = torch.zeros((1, ), dtype=torch.int32, device=dev)

    def run_steps(graph, n):
        done = 0
        while done < n:
            graph.set_token(bos, zero)
            k = min(new, n - done)
            for _ in range(k // graph.steps_per_replay):
                graph.step()  # (the torch-sampling graph feeds token and position back behind the replay: `advance`)
            for _ in range(k % graph.steps_per_replay):
                graph.step_one()
            done += k

    vals = {n: [] for n in graphs}
    for _ in range(args.windows):
        for n, graph in graphs.items():
            run_steps(graph, args.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_steps(graph, args.steps)
            torch.cuda.synchronize()
            vals[n].append(args.steps / (time.perf_counter() - t0))
    for graph in graphs.values():
        graph.close()
    rec["decode"] = {n: dict(tok_s=[round(x, 2) for x in v], median=round(statistics.median(v), 2), spread=round(max(v) - min(v), 2)) for n, v in vals.items()}
    rec["decode"]["native_not_slower"] = rec["decode"]["native"]["median"] >= rec["decode"]["torch"]["median"] - rec["decode"]["torch"]["spread"]
    rec["model"], rec["vocab_size"] = model.config.model_name, model.config.vocab_size
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
