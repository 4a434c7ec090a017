"""The prompt attention kernel (gq_attn_prefill, csrc/prefill_attn.hip) against torch SDPA as the prompt pass calls it, and the chunked
prompt pass of the 8B model, on one GPU.

  attention  q [32][S][128] against caches of 8 KV heads (the Llama-3-8B and the Mistral-7B geometry: the two differ in the window), random
             normal data, for (S, start, W) in CASES: the kernel and SDPA (`native_prompt._sdpa_gqa`: is_causal at start = 0 without a window,
             else the explicit [S, T] mask built from the positions) ALTERNATING, `--launches` launches between two events per run,
             `--repeats` runs each, after a warm-up of both at the shape.  Recorded per case: the microseconds of every run, the
             attended (query, key) pairs, the kernel's rate in TFLOP/s over them (4 * head_dim flops per pair and head), and
             max |kernel - SDPA| on the same inputs.  `auto_keeps` names what GQ_PREFILL_ATTN=auto should serve the case with: the
             kernel only where its median beats SDPA's.
  pass       the 32-layer 8B model (random init, 2 bits), prompts of 8192 and 32768 tokens at the default chunk (4096), last-token
             logits only: wall time around a device synchronise, one warm-up pass, `--passes` timed ones, with GQ_PREFILL_ATTN=1
             and =0 alternating; the peak of torch's allocator above the model and its caches.
Numbers from one box; no threshold is asserted.  Writes profiles/prefill_attention.json (or --out).
    python tools/prefill_attn_timing.py [--launches 20] [--repeats 3] [--passes 2] [--skip-pass]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "prefill_attention.json")
H, HKV, HD = 32, 8, 128
CASES = [(512, 0, 0), (2048, 0, 0), (4096, 0, 0), (4096, 4096, 0), (4096, 28672, 0), (4096, 12288, 4096)]
PROMPTS = (8192, 32768)


def attended_pairs(S, start, W):
    return sum(min(start + i + 1, W) if W else start + i + 1 for i in range(S))


def median(v):
    return sorted(v)[len(v) // 2]


def time_attention(S, start, W, launches, repeats, dev):
    import torch
    from guidedquant_amd import _lib
    from guidedquant_amd.model import _sdpa_gqa, mask_rows
    L = _lib.lib()
    T = start + S
    g = torch.Generator(device=dev)
    g.manual_seed(S + start + W)
    q = torch.randn(H, S, HD, device=dev, generator=g).half()
    kc = torch.randn(1, HKV, T, HD, device=dev, generator=g).half()
    vc = torch.randn(1, HKV, T, HD, device=dev, generator=g).half()
    out = torch.empty(S, H * HD, dtype=torch.float16, device=dev)
    pos = torch.arange(start, T, dtype=torch.int32, device=dev)
    mask = None if (start == 0 and not W) else mask_rows(pos, T, W or None)[None, None]
    scale = 1.0 / math.sqrt(HD)
    st = _lib.current_stream_ptr()

    def hip():
        _lib.check(L.gq_attn_prefill(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), S, start, H, HKV, HD, T, scale, W, st), "gq_attn_prefill")

    def sdpa():
        return _sdpa_gqa(q.unsqueeze(0), kc, vc, mask, H // HKV).transpose(1, 2).reshape(S, H * HD)

    hip()
    y = sdpa()
    torch.cuda.synchronize()
    diff = float((out.float() - y.float()).abs().max())
    rec = dict(S=S, start=start, window=W, pairs=attended_pairs(S, start, W), max_abs_diff_vs_sdpa=diff, hip_us=[], sdpa_us=[])
    for _ in range(repeats):
        for name, fn in (("hip_us", hip), ("sdpa_us", sdpa)):
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            rec[name].append(round(e0.elapsed_time(e1) * 1e3 / launches, 2))
    rec["hip_tflops"] = round(rec["pairs"] * 4.0 * HD * H / (median(rec["hip_us"]) * 1e-6) / 1e12, 1)
    rec["auto_keeps"] = "hip" if median(rec["hip_us"]) < median(rec["sdpa_us"]) else "sdpa"
    return rec


def time_pass(passes, dev):
    import torch
    from guidedquant_amd.APLinear import APLinear
    from guidedquant_amd.generate import random_init_
    from guidedquant_amd.model import ModelArgs, Transformer
    cfg = ModelArgs.from_name("meta-llama/Meta-Llama-3.1-8B")
    cfg.block_size = max(PROMPTS)
    model = Transformer(torch.float16, cfg, linear_class=APLinear, linear_kwargs=dict(bitwidth=2, device=dev))
    model = random_init_(model.to(device=dev, dtype=torch.float16)).eval()
    model.setup_caches(1, max(PROMPTS))
    assert model.native_ready() and model.causal_mask is None
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    recs = []
    for S in PROMPTS:
        idx = torch.randint(0, cfg.vocab_size, (S, ), dtype=torch.int32, device=dev, generator=g)
        pos = torch.arange(S, dtype=torch.int32, device=dev)
        rec = dict(tokens=S, chunk=4096)
        logits = {}
        for i in range(passes + 1):  # (pass 0 warms both routes up)
            for mode in ("1", "0"):
                os.environ["GQ_PREFILL_ATTN"] = mode
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                t0 = time.perf_counter()
                with torch.no_grad():
                    out = model.prefill_native(idx, pos, start=0)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                logits[mode] = out.float().view(-1).clone()
                if i:
                    rec.setdefault("attn_%s_ms" % mode, []).append(round(dt * 1e3, 1))
                    rec["attn_%s_peak_mb" % mode] = round((torch.cuda.max_memory_allocated() - base) / 1e6, 1)
                    rec["attn_%s_plan" % mode] = sorted(set(model.last_prefill_plan["attn"]))
        os.environ.pop("GQ_PREFILL_ATTN", None)
        rec["chunks"] = len(model.last_prefill_plan["chunks"])
        rec["logit_max_abs_diff_hip_vs_sdpa"] = float((logits["1"] - logits["0"]).abs().max())
        rec["logit_max_abs"] = float(logits["0"].abs().max())
        recs.append(rec)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--skip-pass", action="store_true")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU (the HIP path has no fallback)"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rec = dict(protocol="one MI355X, one box; attention: %d heads / %d KV heads of %d, random normal fp16, kernel and SDPA alternating, %d launches "
               "between two events, %d runs each after a warm-up; pass: Llama-3.1-8B geometry, 32 layers, random init, 2 bits, chunk 4096, wall time "
               "around a synchronise, %d timed passes per switch after one warm-up" % (H, HKV, HD, args.launches, args.repeats, args.passes),
               attention=[], prompt_pass=[])

    def flush():
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    for S, start, W in CASES:
        rec["attention"].append(time_attention(S, start, W, args.launches, args.repeats, dev))
        print(json.dumps(rec["attention"][-1]), flush=True)
        flush()
    if not args.skip_pass:
        rec["prompt_pass"] = time_pass(args.passes, dev)
        flush()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
