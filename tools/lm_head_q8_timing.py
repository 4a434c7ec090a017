"""The opt-in int8 lm_head against the fp16 head, measured in ONE process with alternating legs (needs the GPU):
    python tools/lm_head_q8_timing.py [--out profiles/lm_head_q8.json] [--bits 2 4] [--windows 6]

  1. head_alone   gq_dense_gemv_f16 against gq_dense_gemv_i8 with the RMSNorm prologue at 128256 x 4096, 151936 x 4096 and
                  128256 x 2048.  Every launch of a window reads another of three distinct weight buffers (1.6 GB of int8 or more
                  at the two 4096 shapes: the 256 MiB Infinity Cache holds none of a buffer when its turn comes again); 30 launches
                  per captured graph, HIP events around a replay.  us per launch and algorithmic bytes / s.
  2. decode       random-init Llama-3.1-8B geometry, DecodeGraph(native_sampling=True, fold_embed=True, steps_per_replay=10, top_k=50)
                  under both heads, tokens / s over windows of 500 tokens (wall clock around replays that end in a synchronise).  A
                  switch of the head re-allocates the step's buffers, so every leg captures its own graph and warms it up.
  3. accuracy     SYNTHETIC: the random-init 8B head over 256 hidden vectors taken from greedy decode steps -- rms and max |dlogit|,
                  top-1 agreement, the largest |d log-probability| of the fp16 head's top-1 token.  Random weights say nothing about
                  the perplexity of a published checkpoint.
Legs alternate (fp16, int8, fp16, ..), a warm-up behind every switch, `--windows` windows per leg; every figure comes with its median,
minimum, maximum and spread (max - min).  `verdict` holds the two conditions the option ships under."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from guidedquant_amd import _lib  # noqa: E402
from guidedquant_amd._graphs import capture, release  # noqa: E402

MODEL = "meta-llama/Meta-Llama-3.1-8B-Instruct"
SHAPES = ((128256, 4096), (151936, 4096), (128256, 2048))
NBUF, LAUNCHES = 3, 30
SEQ = 100  # tokens per sequence of the decode legs (bench.py's)


def stats(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3), spread=round(max(v) - min(v), 3),
                windows=[round(t, 3) for t in v])


def head_alone(V, D, windows, dev):
    L = _lib.lib()
    g = torch.Generator(device=dev)
    g.manual_seed(V + D)
    W16 = [(torch.randn(V, D, device=dev, generator=g) * 0.02).half() for _ in range(NBUF)]
    W8 = [torch.randint(-127, 128, (V, D), device=dev, generator=g, dtype=torch.int8) for _ in range(NBUF)]
    sc = [torch.rand(V, device=dev, generator=g) * 2.0**-9 + 2.0**-12 for _ in range(NBUF)]
    x = torch.randn(D, device=dev, generator=g).half()
    nw = (1 + 0.1 * torch.randn(D, device=dev, generator=g)).half()
    out = torch.zeros(V, dtype=torch.float16, device=dev)

    def f16(i):
        assert L.gq_dense_gemv_f16(x.data_ptr(), W16[i].data_ptr(), out.data_ptr(), V, D, nw.data_ptr(), 1e-5, _lib.current_stream_ptr()) == 0, L.gq_last_error()

    def i8(i):
        assert L.gq_dense_gemv_i8(x.data_ptr(), W8[i].data_ptr(), sc[i].data_ptr(), out.data_ptr(), V, D, nw.data_ptr(), 1e-5,
                                  _lib.current_stream_ptr()) == 0, L.gq_last_error()

    s = torch.cuda.Stream()
    graphs, us = {}, {"fp16": [], "int8": []}
    with torch.cuda.stream(s):
        for name, fn in (("fp16", f16), ("int8", i8)):
            for i in range(NBUF):
                fn(i)
            s.synchronize()
            gr = torch.cuda.CUDAGraph()
            with capture(gr, stream=s):
                for i in range(LAUNCHES):
                    fn(i % NBUF)
            graphs[name] = gr
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(windows):
            for name in ("fp16", "int8"):
                graphs[name].replay()  # (the warm-up behind the switch)
                s.synchronize()
                e0.record(s)
                graphs[name].replay()
                e1.record(s)
                s.synchronize()
                us[name].append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
        release(*graphs.values())
    nbytes = {"fp16": 2 * V * D + 4 * D + 2 * V, "int8": V * D + 4 * V + 4 * D + 2 * V}  # (weights [+ scales], x and norm weight, logits)
    rec = {"N": V, "K": D, "launches_per_window": LAUNCHES, "distinct_weight_buffers": NBUF}
    for name in us:
        rec[name] = dict(us=stats(us[name]), bytes=nbytes[name], GBps=round(nbytes[name] / statistics.median(us[name]) / 1e3, 1))
    rec["int8_faster_by_us"] = round(rec["fp16"]["us"]["median"] - rec["int8"]["us"]["median"], 3)
    rec["combined_spread_us"] = round(rec["fp16"]["us"]["spread"] + rec["int8"]["us"]["spread"], 3)
    return rec


def decode_legs(model, dev, windows, tokens):
    from guidedquant_amd.generate import DecodeGraph
    bos = torch.tensor([[128000]], dtype=torch.int32, device=dev)
    zero = torch.zeros((1, ), dtype=torch.int32, device=dev)
    tps = {"fp16": [], "int8": []}

    def run(graph, n):
        done = 0
        while done < n:
            graph.set_token(bos, zero)
            for _ in range(SEQ // graph.steps_per_replay):
                graph.step()
            done += SEQ

    for _ in range(windows):
        for name in ("fp16", "int8"):
            model.set_lm_head_dtype(name)
            graph = DecodeGraph(model, dev, native_sampling=True, fold_embed=True, steps_per_replay=10, top_k=50, temperature=0.8)
            try:
                run(graph, 200)  # (the warm-up behind the switch)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(graph, tokens)
                torch.cuda.synchronize()
                tps[name].append(tokens / (time.perf_counter() - t0))
            finally:
                graph.close()
    model.set_lm_head_dtype("fp16")
    return {name: stats(v) for name, v in tps.items()}


def accuracy(model, dev, n=256):
    """SYNTHETIC: random-init weights.  Hidden vectors of n greedy decode steps under the fp16 head, both heads over each of them."""
    model.set_lm_head_dtype("fp16")
    xs, l16 = [], []
    tok = torch.tensor([128000], dtype=torch.int32, device=dev)
    with torch.no_grad():
        for p in range(n):
            lg = model.decode_native(tok, torch.tensor([p], dtype=torch.int32, device=dev))
            xs.append(model._native_state()["x"].clone())
            l16.append(lg.view(-1).float().clone())
            tok = lg.view(-1).argmax().to(torch.int32).view(1)
        model.set_lm_head_dtype("int8")
        st = model._native_state()
        l8 = [st.head(x).view(-1).float().clone() for x in xs]
    model.set_lm_head_dtype("fp16")
    a, b = torch.stack(l16), torch.stack(l8)
    d = (a - b).abs()
    top = a.argmax(dim=1)
    lp16 = torch.log_softmax(a, dim=1).gather(1, top[:, None])
    lp8 = torch.log_softmax(b, dim=1).gather(1, top[:, None])
    return dict(label="synthetic: random-init weights, no statement about a published checkpoint", vectors=n,
                logit_rms=round(float(a.pow(2).mean().sqrt()), 5), dlogit_rms=round(float(d.pow(2).mean().sqrt()), 6),
                dlogit_max=round(float(d.max()), 6), top1_agreement=round(float((b.argmax(dim=1) == top).float().mean()), 5),
                dlogprob_top1_max=round(float((lp16 - lp8).abs().max()), 6))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lm_head_q8.json"))
    ap.add_argument("--bits", type=int, nargs="+", default=[2])
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--tokens", type=int, default=500)
    ap.add_argument("--skip_head_alone", action="store_true")
    a = ap.parse_args()
    assert a.windows >= 5, "at least five windows per leg"
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    from guidedquant_amd.generate import load_model
    dev = torch.device("cuda:0")
    rec = {"device": torch.cuda.get_device_name(0), "method": "one process, legs alternating fp16 / int8, a warm-up behind each switch, "
           "%d windows per leg; spread = max - min over the windows" % a.windows, "head_alone": [], "decode": {}, "not_measured": []}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")

    if not a.skip_head_alone:
        for V, D in SHAPES:
            r = head_alone(V, D, a.windows, dev)
            print("head alone %d x %d: fp16 %.1f us (%.0f GB/s, spread %.1f)  int8 %.1f us (%.0f GB/s, spread %.1f)" % (
                V, D, r["fp16"]["us"]["median"], r["fp16"]["GBps"], r["fp16"]["us"]["spread"], r["int8"]["us"]["median"], r["int8"]["GBps"],
                r["int8"]["us"]["spread"]), flush=True)
            rec["head_alone"].append(r)
            torch.cuda.empty_cache()
            save()
    for bits in a.bits:
        model = load_model(MODEL, dev, "ap", bits, random_init=True)
        model.setup_caches(1, 264)
        assert model.native_ready()
        r = decode_legs(model, dev, a.windows, a.tokens)
        print("decode %d-bit: fp16 head %.1f tokens/s (spread %.1f)  int8 head %.1f tokens/s (spread %.1f)" % (
            bits, r["fp16"]["median"], r["fp16"]["spread"], r["int8"]["median"], r["int8"]["spread"]), flush=True)
        rec["decode"]["%d_bit" % bits] = dict(model=MODEL + " geometry, random init", graph="native_sampling, fold_embed, steps_per_replay=10, top_k=50",
                                              tokens_per_window=a.tokens, tokens_per_s=r)
        save()
        if bits == a.bits[0]:
            rec["accuracy_synthetic"] = accuracy(model, dev)
            print("accuracy (synthetic):", rec["accuracy_synthetic"], flush=True)
            save()
        del model
        torch.cuda.empty_cache()
    rec["not_measured"] = [s for s in ("4-bit decode" if 4 not in a.bits else None, "Qwen3 geometry in the captured step",
                                       "perplexity on a published checkpoint (no checkpoint on the build machine)") if s]
    h = next((r for r in rec["head_alone"] if (r["N"], r["K"]) == (128256, 4096)), None)
    d0 = rec["decode"].get("%d_bit" % a.bits[0])
    rec["verdict"] = dict(
        head_alone_128256x4096_int8_faster_than_combined_spread=bool(h and h["int8_faster_by_us"] > h["combined_spread_us"]),
        decode_int8_not_slower=bool(d0 and d0["tokens_per_s"]["int8"]["median"] >= d0["tokens_per_s"]["fp16"]["median"]))
    save()
    print(json.dumps(rec["verdict"]))


if __name__ == "__main__":
    main()
