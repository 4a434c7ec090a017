"""What an fp8 (e4m3) KV cache costs and saves on the fused decode route: the Llama-3.1-8B geometry, random init, 2 bits, a cache of 32768
rows -- `kv_cache_dtype="fp8"` against the default fp16 cache, the two alternating in one process (`--rounds` rounds of fp16, fp8):

  tok_s          in-graph decode (captured DecodeGraph, ten token steps per replay, fused sampler) from 50 (the short-context step: the price
                 of the fp8 route's extra launch per layer) / 4095 / 16000 / 32000 cached positions: `--steps` token steps, `--repeats` windows;
  attn_us        layer 0's attention launch (+ its combine launch) alone at the position, `--launches` launches between two events;
                 fp8 also `row_write_us`: the gq_rope_cache_rows_kv8 launch (S = 1) the fp16 route has no counterpart of;
  prefill_ms     the prompt pass of 8192 tokens (chunks of 4096, the HIP prompt attention of the cache's dtype).
No threshold is asserted and no speed is promised: the record says what came out, losses included.  Writes profiles/kv8_decode.json.
    python tools/kv8_decode_timing.py [--rounds 2] [--steps 20] [--warmup 10] [--repeats 3] [--launches 200]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "kv8_decode.json")
MAX_SEQ, POSITIONS, PROMPT = 32768, (50, 4095, 16000, 32000), 8192


def _timed(fn, launches, repeats):
    import torch
    vals = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for i in range(launches + 20):
            if i == 20:
                e0.record()
            fn()
        e1.record()
        torch.cuda.synchronize()
        vals.append(round(e0.elapsed_time(e1) * 1e3 / launches, 3))
    return vals


def attn_us(model, pos, launches, repeats):
    """(attention + combine, row write or None) of layer 0 at the position, microseconds per launch"""
    import torch
    from guidedquant_amd import _lib
    st, at, c, L = model._native_state(), model.layers[0].attention, model.config, _lib.lib()
    posd = torch.tensor([pos], dtype=torch.int32, device=st.x.device)
    kv, sp = st.kv(at, 0), _lib.current_stream_ptr()
    if not st.kv8:
        roped = L.gq_anyprec_qkv_rope_supported(at.wqkv.out_features, c.dim, at.wqkv.bitwidth, c.head_dim)
        entry = "gq_attn_decode_roped" if roped else "gq_attn_decode_split"
        return _timed(lambda: st.attend(entry, st.qkv.data_ptr(), posd, kv, sp, layer=0), launches, repeats), None
    kvc, ws = at.kv_cache, st.attn_ws.data_ptr() if st.attn_ws is not None else None

    def attend():
        _lib.check(L.gq_attn_decode_roped_kv8(st.q8.data_ptr(), posd.data_ptr(), *kv, kvc.k_scale.data_ptr(), kvc.v_scale.data_ptr(), st.y.data_ptr(), c.n_head,
                                              c.n_local_heads, c.head_dim, model.max_seq_length, 1.0 / math.sqrt(c.head_dim), st.layer_split[0], ws, 0, sp), "attn")

    def write():
        _lib.check(L.gq_rope_cache_rows_kv8(st.qkv.data_ptr(), posd.data_ptr(), model.rope_cos.data_ptr(), model.rope_sin.data_ptr(), st.q8.data_ptr(), *kv,
                                            kvc.k_inv.data_ptr(), kvc.v_inv.data_ptr(), 1, c.n_head, c.n_local_heads, c.head_dim, model.max_seq_length,
                                            None, None, 0.0, None, sp), "rows")
    return _timed(attend, launches, repeats), _timed(write, launches, repeats)


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
    graph.close()
    return vals


def prefill_ms(model, dev, runs=2):
    import torch
    idx = torch.randint(0, model.config.vocab_size, (PROMPT,), dtype=torch.int32, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    pos = torch.arange(PROMPT, dtype=torch.int32, device=dev)
    vals = []
    with torch.no_grad():
        for i in range(runs + 1):  # (the first run warms up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.prefill_native(idx, pos, start=0)
            torch.cuda.synchronize()
            if i:
                vals.append(round((time.perf_counter() - t0) * 1e3, 2))
    return vals, sorted(set(model.last_prefill_plan["attn"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
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
    rec = dict(protocol="random init, 2-bit, Llama-3.1-8B geometry, cache of %d rows, scales 1.0; fp16 and fp8 caches alternating, %d rounds; tok_s: "
               "DecodeGraph with 10 steps per replay, %d warm-up steps, %d-step window, %d windows; attn_us / row_write_us: layer 0's launches, %d "
               "launches between two events, %d runs; prefill_ms: %d tokens, two timed runs behind a warm-up"
               % (MAX_SEQ, args.rounds, args.warmup, args.steps, args.repeats, args.launches, args.repeats, PROMPT),
               positions=list(POSITIONS), rounds=[])
    g = torch.Generator(device=dev)
    for r in range(args.rounds):
        for kv in ("fp16", "fp8"):
            model.setup_caches(1, MAX_SEQ, kv_cache_dtype=kv)
            assert model.native_ready() and model.kv_cache_dtype == kv
            g.manual_seed(1)
            for b in model.layers:  # (a cache an earlier sequence filled: finite rows everywhere, the same numbers up to the format)
                for t in (b.attention.kv_cache.k_cache, b.attention.kv_cache.v_cache):
                    t.copy_((torch.rand(t.shape[1:], device=dev, generator=g) - 0.5).half().to(t.dtype)[None])
            st = model._native_state()
            leg = dict(round=r, kv_cache_dtype=kv, n_split=st.layer_split[0],
                       cache_bytes=sum(t.numel() * t.element_size() for b in model.layers for t in (b.attention.kv_cache.k_cache, b.attention.kv_cache.v_cache)))
            for pos in POSITIONS:
                a, w = attn_us(model, pos, args.launches, args.repeats)
                leg["pos_%d" % pos] = dict(attn_us=a, **(dict(row_write_us=w) if w is not None else {}),
                                           tok_s=tok_s(model, dev, pos, args.steps, args.warmup, args.repeats))
            leg["prefill_ms"], leg["prefill_attn"] = prefill_ms(model, dev)
            rec["rounds"].append(leg)
            print(json.dumps(leg), flush=True)
            with open(OUT, "w") as f:  # (written leg by leg: a run cut short leaves what it measured)
                json.dump(rec, f, indent=1)
                f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
