"""What the MXFP4 KV cache (`kv_cache_dtype="mxfp4"`) costs on the fused decode route next to the fp16 and the per-row scaled fp8 cache: the
Llama-3.1-8B geometry, random init, 2 bits, a cache of 32768 rows, the three legs alternating in one process (`--rounds` rounds of fp16,
fp8_row, mxfp4), with the protocol and the timers of tools/kv8_decode_timing.py:

  tok_s          in-graph decode (captured DecodeGraph, ten token steps per replay, fused sampler) from 50 / 4095 / 16000 / 32000 cached
                 positions: `--steps` token steps, `--repeats` windows;
  attn_us        layer 0's attention launch (+ its combine launch) alone at the position, `--launches` launches between two events;
  row_write_us   fp8_row and mxfp4: the row-write launch (S = 1) in front of it;
  cache_bytes    codes and exponent bytes of all layers.
No threshold is asserted and no speed is promised: the record says what came out, losses included.  Writes profiles/kv_mxfp4_decode.json.
    python tools/kv_mx4_decode_timing.py [--rounds 2] [--steps 20] [--warmup 10] [--repeats 3] [--launches 200] [--out FILE]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kv8_decode_timing as k8t  # noqa: E402  (the timers, the positions and the cache size)
import kv8r_decode_timing as k8rt  # noqa: E402  (the fp8_row leg's launches)

OUT = os.path.join(ROOT, "profiles", "kv_mxfp4_decode.json")


def attn_us_mx4(model, pos, launches, repeats):
    """(attention + combine, row write) of layer 0 over the mxfp4 cache at the position, microseconds per launch"""
    import torch
    from guidedquant_amd import _lib
    st, at, c, L = model._native_state(), model.layers[0].attention, model.config, _lib.lib()
    posd = torch.tensor([pos], dtype=torch.int32, device=st.x.device)
    kv, sp, kvc = st.kv(at, 0), _lib.current_stream_ptr(), at.kv_cache
    ex = kvc.k_exp.data_ptr(), kvc.v_exp.data_ptr()
    ws = st.attn_ws.data_ptr() if st.attn_ws is not None else None

    def attend():
        _lib.check(L.gq_attn_decode_roped_mx4(st.q8.data_ptr(), posd.data_ptr(), *kv, *ex, st.y.data_ptr(), c.n_head, c.n_local_heads, c.head_dim,
                                              model.max_seq_length, 1.0 / math.sqrt(c.head_dim), st.layer_split[0], ws, 0, sp), "attn")

    def write():
        _lib.check(L.gq_rope_cache_rows_mx4(st.qkv.data_ptr(), posd.data_ptr(), model.rope_cos.data_ptr(), model.rope_sin.data_ptr(), st.q8.data_ptr(), *kv, *ex,
                                            1, c.n_head, c.n_local_heads, c.head_dim, model.max_seq_length, None, None, 0.0, None, sp), "rows")
    return k8t._timed(attend, launches, repeats), k8t._timed(write, launches, repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU (the HIP path has no fallback)"
    from guidedquant_amd.APLinear import APLinear
    from guidedquant_amd.generate import random_init_
    from guidedquant_amd.model import ModelArgs, Transformer, transformer_configs
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(1234)
    cfg = ModelArgs(**dict(transformer_configs["meta-llama/Meta-Llama-3.1-8B"], block_size=k8t.MAX_SEQ))
    model = Transformer(torch.float16, cfg, linear_class=APLinear, linear_kwargs=dict(bitwidth=2, device=dev))
    model = random_init_(model.to(device=dev, dtype=torch.float16)).eval()
    rec = dict(protocol="random init, 2-bit, Llama-3.1-8B geometry, cache of %d rows (fp8_row: exponent bytes 127; mxfp4: random codes, exponent bytes 127); fp16, "
               "fp8_row and mxfp4 alternating, %d rounds; tok_s: DecodeGraph with 10 steps per replay, %d warm-up steps, %d-step window, %d windows; attn_us / "
               "row_write_us: layer 0's launches, %d launches between two events, %d runs" % (k8t.MAX_SEQ, args.rounds, args.warmup, args.steps, args.repeats,
                                                                                              args.launches, args.repeats), positions=list(k8t.POSITIONS), rounds=[])
    g = torch.Generator(device=dev)
    timers = {"fp16": k8t.attn_us, "fp8_row": k8rt.attn_us_row, "mxfp4": attn_us_mx4}
    for r in range(args.rounds):
        for kv in ("fp16", "fp8_row", "mxfp4"):
            model.setup_caches(1, k8t.MAX_SEQ, kv_cache_dtype=kv)
            assert model.native_ready() and model.kv_cache_dtype == kv
            g.manual_seed(1)
            caches = [b.attention.kv_cache for b in model.layers]
            for kc in caches:  # (a cache an earlier sequence filled: finite rows everywhere)
                for t in (kc.k_cache, kc.v_cache):
                    if kv == "mxfp4":
                        t.copy_(torch.randint(0, 256, t.shape[1:], device=dev, generator=g, dtype=torch.uint8)[None])
                    else:
                        t.copy_((torch.rand(t.shape[1:], device=dev, generator=g) - 0.5).half().to(t.dtype)[None])
            tensors = [t for kc in caches for t in ((kc.k_cache, kc.v_cache) + ((kc.k_exp, kc.v_exp) if kv != "fp16" else ()))]
            st = model._native_state()
            leg = dict(round=r, leg=kv, n_split=st.layer_split[0], cache_bytes=sum(t.numel() * t.element_size() for t in tensors))
            for pos in k8t.POSITIONS:
                a, w = timers[kv](model, pos, args.launches, args.repeats)
                leg["pos_%d" % pos] = dict(attn_us=a, **(dict(row_write_us=w) if w is not None else {}),
                                           tok_s=k8t.tok_s(model, dev, pos, args.steps, args.warmup, args.repeats))
            rec["rounds"].append(leg)
            print(json.dumps(leg), flush=True)
            with open(args.out, "w") as f:  # (written leg by leg: a run cut short leaves what it measured)
                json.dump(rec, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
