"""Score a file of token ids on the fused prompt path and print ONE JSON line: perplexity by the reference's definition
(any_precision/evaluate/eval.py:205-226: non-overlapping chunks of --chunk_size tokens, the mean of the chunks' mean negative
log-likelihoods, exp of it; a shorter tail is dropped), the per-chunk values, the share of greedy hits.  No tokenizer and no dataset:
the ids come from an .npy file or an .npz entry (--key, default the first array), the model from the arguments of
guidedquant_amd/generate.py (`Transformer.score_native`: the HIP prompt pass with the scoring head; GQ_SCORE_HEAD picks the head).
    python tools/score_tokens.py tokens.npy --model_name meta-llama/Meta-Llama-3.1-8B --backend ap --bitwidth 2 --checkpoint_path DIR
    python tools/score_tokens.py tokens.npz --key wikitext2 --model_name ... --backend ap --bitwidth 2 --random_init --chunk_size 512
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_ids(path, key=None):
    import numpy as np
    a = np.load(path)
    if hasattr(a, "files"):
        a = a[key if key is not None else a.files[0]]
    a = np.asarray(a).reshape(-1)
    if a.dtype.kind not in "iu":
        raise ValueError(f"{path}: token ids must be integers, not {a.dtype}")
    return a.astype(np.int64)


def main():
    ap = argparse.ArgumentParser(description="perplexity / log-likelihood of token ids on the fused prompt path")
    ap.add_argument("tokens", help=".npy, or .npz with --key")
    ap.add_argument("--key", type=str, default=None)
    ap.add_argument("--chunk_size", type=int, default=2048)
    ap.add_argument("--device", type=str, default="cuda")
    ap.add_argument("--model_name", type=str, required=True)
    ap.add_argument("--bitwidth", type=int, default=None, choices=[2, 3, 4, 5, 6, 7, 8])
    ap.add_argument("--checkpoint_path", type=str, default=None)
    ap.add_argument("--dtype", type=str, default="float16", choices=["float16"])
    ap.add_argument("--backend", type=str, default="ap", choices=["ap", "qtip"])
    ap.add_argument("--random_init", action="store_true")
    ap.add_argument("--kv_cache_dtype", type=str, default=None, choices=["fp16", "fp8"])
    a = ap.parse_args()
    import torch
    from guidedquant_amd.generate import load_model
    ids = load_ids(a.tokens, a.key)
    n = len(ids) // a.chunk_size if a.chunk_size >= 2 else 0
    if n < 1:
        raise SystemExit(f"{a.tokens}: {len(ids)} tokens hold no whole chunk of {a.chunk_size} (>= 2)")
    model = load_model(a.model_name, a.device, a.backend, a.bitwidth, random_init=a.random_init, checkpoint_path=a.checkpoint_path)
    if int(ids.min()) < 0 or int(ids.max()) >= model.config.vocab_size:
        raise SystemExit(f"{a.tokens}: token ids must lie in [0, {model.config.vocab_size})")
    if a.chunk_size > model.config.block_size:
        raise SystemExit(f"--chunk_size {a.chunk_size} exceeds the model's context ({model.config.block_size})")
    model.setup_caches(1, a.chunk_size, kv_cache_dtype=a.kv_cache_dtype)
    dev_ids = torch.from_numpy(ids[:n * a.chunk_size]).to(device=a.device, dtype=torch.int32)
    if not model.prefill_ready(dev_ids[:a.chunk_size]):
        raise SystemExit("the fused prompt pass does not serve this model on this device (no fallback)")
    nlls, hits = [], 0
    with torch.no_grad():
        for i in range(n):
            lp, greedy = model.score_native(dev_ids[i * a.chunk_size:(i + 1) * a.chunk_size])
            nlls.append(float(-lp.double().mean()))
            hits += int(greedy.sum())
    print(json.dumps(dict(ppl=math.exp(sum(nlls) / n), nll_per_chunk=nlls, chunks=n, chunk_size=a.chunk_size, tokens_dropped=len(ids) - n * a.chunk_size,
                          greedy_share=hits / (n * (a.chunk_size - 1)), head=model.last_prefill_plan["head"], kv_cache_dtype=model.kv_cache_dtype)))


if __name__ == "__main__":
    main()
