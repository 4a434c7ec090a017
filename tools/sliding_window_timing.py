"""What a sliding window costs and saves on the fused decode route: the Mistral-7B geometry (32 layers, hidden 4096, MLP 14336, 32 / 8
heads of 128, vocab 32000; restated from the public config), random init, 2 bits, every layer with W = 4096 -- against the same model
with the window taken off (ModelArgs.layer_windows = None: the launches it always had), at 4095 / 8000 / 16000 cached positions:

  tok_s          in-graph decode (captured DecodeGraph, ten token steps per replay, fused sampler): `--steps` token steps from the position,
                 `--repeats` windows, each started at the position again;
  attn_us        the attention launch of layer 0 alone (the entry and split count the step uses, + its combine launch) at the position:
                 `--launches` launches between two events, `--repeats` runs.

The expectation the record is read against: windowed attention at 16000 positions reads the rows full attention reads at 4095, so
`attn_us` of the two should agree within the spread of the runs, plus what the rows requested ahead of the position no longer save
(with lo > 0 they are dropped, csrc/decode.hip).  No threshold is asserted.  Writes profiles/sliding_window_decode.json.
    python tools/sliding_window_timing.py [--steps 20] [--warmup 10] [--repeats 3] [--launches 200]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "sliding_window_decode.json")
W, MAX_SEQ, POSITIONS = 4096, 16384, (4095, 8000, 16000)
MISTRAL_7B = dict(model_name="Mistral-7B-v0.1", block_size=32768, n_layer=32, n_head=32, n_local_heads=8, dim=4096, head_dim=128,
                  intermediate_size=14336, vocab_size=32000, rope_base=10000, norm_eps=1e-5)


def attention_entry(model):
    """the entry ApStep.layers takes for a layer without QK-norm or bias (native_step.py)"""
    from guidedquant_amd import _lib
    at, c = model.layers[0].attention, model.config
    roped = _lib.lib().gq_anyprec_qkv_rope_supported(at.wqkv.out_features, c.dim, at.wqkv.bitwidth, c.head_dim)
    return "gq_attn_decode_roped" if roped else "gq_attn_decode_split"


def attn_us(model, pos, launches, repeats):
    import torch
    from guidedquant_amd import _lib
    st = model._native_state()
    posd = torch.tensor([pos], dtype=torch.int32, device=st.x.device)
    entry, kv = attention_entry(model), st.kv(model.layers[0].attention, 0)
    vals = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for i in range(launches + 20):
            if i == 20:
                e0.record()
            st.attend(entry, st.qkv.data_ptr(), posd, kv, _lib.current_stream_ptr(), layer=0)
        e1.record()
        torch.cuda.synchronize()
        vals.append(round(e0.elapsed_time(e1) * 1e3 / launches, 3))
    return vals


def tok_s(model, dev, pos, steps, warmup, repeats):
    import torch
    from guidedquant_amd.generate import DecodeGraph
    spr = 10
    assert steps % spr == 0 and warmup % spr == 0 and pos + warmup + steps < model.max_seq_length
    graph = DecodeGraph(model, dev, native_sampling=True, temperature=0.0, top_k=32, fold_embed=True, steps_per_replay=spr)
    vals = []
    for _ in range(repeats):
        graph.set_token(1, pos)
        for _ in range(warmup // spr):
            graph.step()
        graph.set_token(1, pos)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps // spr):
            graph.step()
        torch.cuda.synchronize()
        vals.append(round(steps / (time.perf_counter() - t0), 2))
    graph.close() if hasattr(graph, "close") else None
    return vals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU (the HIP path has no fallback)"
    from guidedquant_amd.APLinear import APLinear
    from guidedquant_amd.generate import random_init_
    from guidedquant_amd.model import ModelArgs, Transformer
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(1234)
    cfg = ModelArgs(layer_windows=(W,) * MISTRAL_7B["n_layer"], **MISTRAL_7B)
    model = Transformer(torch.float16, cfg, linear_class=APLinear, linear_kwargs=dict(bitwidth=2, device=dev))
    model = random_init_(model.to(device=dev, dtype=torch.float16)).eval()
    model.setup_caches(1, MAX_SEQ)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    for b in model.layers:  # (a cache an earlier sequence filled: finite rows everywhere)
        for t in (b.attention.kv_cache.k_cache, b.attention.kv_cache.v_cache):
            t.copy_((torch.rand(t.shape, device=dev, generator=g) - 0.5).half())
    rec = dict(protocol="random init, 2-bit, Mistral-7B geometry, cache of %d rows; tok_s: DecodeGraph with 10 steps per replay, %d warm-up steps, "
               "%d-step window, %d windows per position; attn_us: layer 0's attention launch (+ combine), %d launches between two events, %d runs"
               % (MAX_SEQ, args.warmup, args.steps, args.repeats, args.launches, args.repeats), window=W, positions=list(POSITIONS))
    for name, lw in (("windowed", cfg.layer_windows), ("full", None)):
        model.config.layer_windows = lw
        model._reset_native()  # (the step's per-layer plan is rebuilt; the decode step takes no mask)
        assert model.native_ready()
        st = model._native_state()
        leg = dict(entry=attention_entry(model) + ("_window" if lw else ""), n_split=st.layer_split[0])
        for pos in POSITIONS:
            leg["pos_%d" % pos] = dict(rows_read=min(pos + 1, W) if lw else pos + 1, attn_us=attn_us(model, pos, args.launches, args.repeats),
                                       tok_s=tok_s(model, dev, pos, args.steps, args.warmup, args.repeats))
        rec[name] = leg
    a, b = rec["windowed"]["pos_16000"]["attn_us"], rec["full"]["pos_4095"]["attn_us"]
    rec["attn_us_windowed_16000_vs_full_4095"] = dict(windowed_16000=a, full_4095=b, spread_full_4095=round(max(b) - min(b), 3),
                                                      difference_of_medians=round(sorted(a)[len(a) // 2] - sorted(b)[len(b) // 2], 3))
    assert all(math.isfinite(v) for v in a + b)
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
