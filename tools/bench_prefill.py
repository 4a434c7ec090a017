"""Prefill micro-benchmark (GPU box): the fused-dequant MFMA GEMM (gq_anyprec_gemm; 2..4 bits csrc/ap_gemm.hip, 5..8 bits
csrc/ap_gemm_wide.hip) against the reference's two steps (anyprec_dequant -> torch.matmul = hipBLASLt) on the Llama-3-8B layer
shapes; us per call, TFLOP/s (2 S N K) and the fraction of the dense fp16 MFMA peak (2500 TFLOP/s).

    python tools/bench_prefill.py [BITS[,BITS..]] [--rows 128,512,2048] [--prompt-pass | --prompt-pass-only] [--json PATH]

Every call is timed on its own with HIP events and the MEDIAN is reported, with the spread (p10 / p90) of the same calls beside it.
Successive calls walk a rotating set of distinct weight tensors of at least 600 MB in all (more than the 256 MB Infinity Cache),
so neither side finds its planes cached from the call before.  --prompt-pass adds the whole 8B-shaped model's prompt pass
(`Transformer.prefill_native`) under the default dispatch, under GQ_PREFILL_FUSED=1 (every linear fused) and =0 (every linear by the two steps);
--prompt-pass-only measures that alone.  --json writes the tables to PATH (sections already in that file are kept)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from guidedquant_amd import ap_gemv  # noqa: E402

SHAPES = {"wqkv": (6144, 4096), "wo": (4096, 4096), "w1w3": (28672, 4096), "w2": (4096, 14336)}
ROTATE_BYTES = 600e6


def timed(fn, iters=20):
    """best-of-3 mean of `iters` back-to-back calls (the round-3 figures; tools/gemm_ablation.py)"""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e9
    for _ in range(3):
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / iters)
    return best


def timed_median(fn, iters=24, warm=3):
    """fn(i) -> median, p10, p90 us of `iters` calls, each between its own pair of events"""
    for i in range(warm):
        fn(i)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for i, (e0, e1) in enumerate(ev):
        e0.record()
        fn(warm + i)
        e1.record()
    torch.cuda.synchronize()
    t = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
    return t[len(t) // 2], t[len(t) // 10], t[(9 * len(t)) // 10]


def kernels(bits_list, rows, d):
    out = []
    for bits in bits_list:
        for name, (N, K) in SHAPES.items():
            copies = max(2, min(48, int(ROTATE_BYTES // (bits * N * K // 8)) + 1))
            qs = [torch.randint(-2**31, 2**31 - 1, (bits, N, K // 32), dtype=torch.int32, device=d) for _ in range(copies)]
            lut = (torch.randn(N, 1 << bits, device=d) * 0.02).half().sort(dim=1).values.contiguous()
            for S in rows:
                x = torch.randn(S, K, device=d).half()
                t_f, f_lo, f_hi = timed_median(lambda i: ap_gemv.anyprec_gemm(x, qs[i % copies], lut, bits))
                t_r, r_lo, r_hi = timed_median(lambda i: torch.matmul(x, ap_gemv.anyprec_dequant(qs[i % copies], lut, bits).T))
                fl = 2.0 * S * N * K
                rec = {"shape": name, "N": N, "K": K, "S": S, "bits": bits, "weight_copies": copies, "fused_us": round(t_f, 1),
                       "fused_us_p10_p90": [round(f_lo, 1), round(f_hi, 1)], "dequant_matmul_us": round(t_r, 1),
                       "dequant_matmul_us_p10_p90": [round(r_lo, 1), round(r_hi, 1)], "fused_TFLOPs": round(fl / t_f / 1e6, 1),
                       "frac_of_2500_TF": round(fl / t_f / 1e6 / 2500, 4), "speedup_vs_reference_steps": round(t_r / t_f, 2)}
                print(json.dumps(rec), flush=True)
                out.append(rec)
            del qs
            torch.cuda.empty_cache()
    return out


def prompt_pass(bits_list, rows, d):
    from guidedquant_amd.generate import load_model
    out = []
    for bits in bits_list:
        torch.manual_seed(0)
        m = load_model("meta-llama/Meta-Llama-3.1-8B", d, "ap", bits, random_init=True)
        m.setup_caches(1, max(rows) + 8)
        for S in rows:
            x = torch.randint(0, 128000, (1, S), dtype=torch.int32, device=d)
            pos = torch.arange(S, dtype=torch.int32, device=d)
            res = {}
            for mode in ("auto", "1", "0"):
                os.environ["GQ_PREFILL_FUSED"] = mode
                with torch.no_grad():
                    res[mode] = timed_median(lambda i: m.prefill_native(x, pos, start=0, last_only=True), iters=7, warm=2)
            os.environ.pop("GQ_PREFILL_FUSED", None)
            rec = {"model": "Llama-3.1-8B", "bits": bits, "prompt_tokens": S, "prefill_ms_auto": round(res["auto"][0] / 1e3, 3),
                   "prefill_ms_auto_p10_p90": [round(res["auto"][1] / 1e3, 3), round(res["auto"][2] / 1e3, 3)],
                   "prefill_ms_all_fused": round(res["1"][0] / 1e3, 3), "prefill_ms_two_steps": round(res["0"][0] / 1e3, 3),
                   "prefill_ms_two_steps_p10_p90": [round(res["0"][1] / 1e3, 3), round(res["0"][2] / 1e3, 3)],
                   "speedup_vs_two_steps": round(res["0"][0] / res["auto"][0], 3)}
            print(json.dumps(rec), flush=True)
            out.append(rec)
        del m
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    d = torch.device("cuda:0")
    args = sys.argv[1:]

    def opt(name, dflt=None):
        if name in args:
            i = args.index(name)
            v = args[i + 1]
            del args[i:i + 2]
            return v
        return dflt

    path = opt("--json")
    rows = [int(s) for s in opt("--rows", "128,512,2048").split(",")]
    only_pass = "--prompt-pass-only" in args
    with_pass = only_pass or "--prompt-pass" in args
    args = [a for a in args if not a.startswith("--prompt-pass")]
    bits_list = [int(b) for b in args[0].split(",")] if args else [2, 4]
    doc = json.load(open(path)) if path and os.path.exists(path) else {}
    doc.update({"tool": "tools/bench_prefill.py", "device": torch.cuda.get_device_name(0), "timing": "HIP events per call, median (p10, p90)"})
    if not only_pass:
        doc["kernels"] = kernels(bits_list, rows, d)
    if with_pass:
        doc["prompt_pass"] = prompt_pass(bits_list, [s for s in rows if s <= 512] or rows, d)
    if path:
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
