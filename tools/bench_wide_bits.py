"""Measure the Any-Precision GEMV at 5 to 8 bits (ap_wide.hip) against the generic kernel it replaces, and the 8B decode at those widths.

Prints one JSON object:
  * "gemv": per (bits, Llama 8B / 70B matrix, launch form) the launch time in us of the default dispatch (the wide kernel) and of
    GQ_AP_FORCE_GENERIC=1 (the generic kernel; the plain form only -- it has no fused forms), HIP events inside a captured graph over
    > 512 MB of distinct weights (bench.py::bench_ap_shape), and the fraction of the 8 TB/s HBM peak each reaches;
  * "decode": tokens/s of the random-init Llama-3.1-8B at each width on the fused route (the captured DecodeGraph, bench.py's
    decode_tok_s) and on the module tree (the Transformer's eager forward, one launch per module).

    python tools/bench_wide_bits.py [--bits 5 6 7 8] [--iters 50] [--steps 100] [--no-decode] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

SHAPES = {"8B": {"wqkv": (6144, 4096), "wo": (4096, 4096), "w1w3": (28672, 4096), "w2": (4096, 14336)},
          "70B": {"wqkv": (10240, 8192), "wo": (8192, 8192), "w1w3": (57344, 8192), "w2": (8192, 28672)}}
# the decode step's launch of each matrix (bench_ap_shape's `fused` names)
DECODE_FORM = {"wqkv": "norm", "wo": "resid", "w1w3": "norm_pairs", "w2": "resid"}


def _generic(on):
    from guidedquant_amd import _lib
    if on:
        os.environ["GQ_AP_FORCE_GENERIC"] = "1"
    else:
        os.environ.pop("GQ_AP_FORCE_GENERIC", None)
    _lib.lib().gq_reset_env_cache()


def gemv_rows(bits_list, iters):
    from guidedquant_amd import _lib
    rows = []
    for bits in bits_list:
        for model, shapes in SHAPES.items():
            for name, (N, K) in shapes.items():
                for fused in (None, DECODE_FORM[name]):
                    form = fused or "plain"
                    route = _lib.ap_plan_route(N, K, bits, 1, fused in ("norm", "norm_pairs"), {"resid": 1, "norm_pairs": 4}.get(fused, 0))
                    rec = bench.bench_ap_shape(f"{model}_{name}", N, K, bits, iters=iters, fused=fused)
                    row = {"bits": bits, "model": model, "matrix": name, "N": N, "K": K, "launch": form, "route": route[0],
                           "wide_us": rec["us"], "wide_frac": rec["frac"]}
                    if fused is None:
                        _generic(True)
                        try:
                            assert _lib.ap_plan_route(N, K, bits)[0] == "generic"
                            g = bench.bench_ap_shape(f"{model}_{name}", N, K, bits, iters=iters)
                        finally:
                            _generic(False)
                        row.update(generic_us=g["us"], generic_frac=g["frac"], speedup=round(g["us"] / rec["us"], 2))
                    print(json.dumps(row), file=sys.stderr, flush=True)
                    rows.append(row)
    return rows


def module_tree_tok_s(model, dev, steps):
    """the Transformer's eager forward, one token per call (every linear its own APLinear launch), greedy"""
    import torch
    tok = torch.ones((1, 1), dtype=torch.int32, device=dev)
    with torch.no_grad():
        for p in range(3):
            model(tok, torch.tensor([p], dtype=torch.int32, device=dev))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for p in range(steps):
            lg = model(tok, torch.tensor([p % bench.SEQ_NEW_TOKENS], dtype=torch.int32, device=dev))
            tok = lg[:, -1:].argmax(dim=-1).to(torch.int32)
        torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def decode_rows(bits_list, steps):
    import torch
    from guidedquant_amd.generate import load_model
    dev = torch.device("cuda:0")
    rows = []
    for bits in bits_list:
        model = load_model(bench.MODEL, dev, "ap", bits, random_init=True)
        model.setup_caches(1, bench.SEQ_NEW_TOKENS + 1)
        assert model.native_ready(), f"no fused decode form at {bits} bits"
        graph, run = bench.decode_tok_s(model, dev, steps, 10)
        run(10)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        fused = steps / (time.perf_counter() - t0)
        graph.close()
        tree = module_tree_tok_s(model, dev, max(20, steps // 5))
        row = {"bits": bits, "fused_tok_s": round(fused, 1), "module_tree_tok_s": round(tree, 1)}
        print(json.dumps(row), file=sys.stderr, flush=True)
        rows.append(row)
        del model, graph
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--bits", type=int, nargs="+", default=[5, 6, 7, 8])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--no-gemv", action="store_true")
    ap.add_argument("--no-decode", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert all(5 <= b <= 8 for b in a.bits)
    import torch
    res = {"gpu": torch.cuda.get_device_name(0), "hbm_peak_GBps": bench.HBM_PEAK_GBPS}
    if not a.no_gemv:
        res["gemv"] = gemv_rows(a.bits, a.iters)
    if not a.no_decode:
        res["decode"] = decode_rows(a.bits, a.steps)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
