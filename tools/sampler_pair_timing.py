"""Time of the fused sampler's two launches (sample_stage1 + sample_stage2, csrc/sampler.hip) inside a captured graph, per vocabulary.

One hipGraph holds PAIRS calls of one entry point on fixed random fp16 logits (T = 0.8, top_k = 50 by default: the 64-candidate
instances; --top-k 32 times the 32-candidate ones the benchmark's greedy step runs); the graph is replayed REPLAYS times between two
device events after a warm-up, and the time of one pair is window / (PAIRS * REPLAYS).  Inside a graph the pairs run back to back with
the logits in cache, as the step's last two launches do behind the lm_head GEMV that has just written them.

--entry p (default): gq_sample_topk_p.  --entry rep: gq_sample_topk_rep with repetition_penalty 1.05, a `seen` set of 512 tokens (every
draw adds its own) and a `suppress` set of 8.  --entry lp: gq_sample_topk_lp with both outputs, once without a penalty or a set (the
fp16-key instances; records V.._k..) and once with the penalty and the sets of `rep` (the fp32-key ones; records V.._k.._rp1.05).

Merges one record per label into profiles/sampler_wide_vocab.json under "pair_time" (other keys of that file are kept).  To time
another build of the library, point GQ_LIB_PATH at it:
    python tools/sampler_pair_timing.py --label this_tree --vocab 128256 151936 262144
    GQ_LIB_PATH=/path/to/parent/libgq_hip.so python tools/sampler_pair_timing.py --label parent --vocab 128256
    python tools/sampler_pair_timing.py --entry rep --label rep_this_tree --vocab 128256 151936
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "sampler_wide_vocab.json")
PAIRS, REPLAYS, WINDOWS = 50, 40, 5


def pair_us(V, top_k, temperature, dev, entry="p", penalty=False):
    import torch
    from guidedquant_amd import _lib
    L = _lib.lib()
    g = torch.Generator(device=dev)
    g.manual_seed(V)
    logits = (torch.randn(V, device=dev, generator=g) * 2).half()
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
    wv, wi = z(128 * 64, torch.float32), z(128 * 64, torch.int32)
    ctr, tok, pos, nt = (z(1, torch.int32) for _ in range(4))
    rp, seen, sup = 1.0, None, None
    if penalty:
        rp, seen, sup = 1.05, z((V + 31) // 32, torch.int32), z((V + 31) // 32, torch.int32)
        ids = torch.randperm(V, device=dev, generator=g)[:520].int()
        _lib.check(L.gq_token_set_build(ids.data_ptr(), 512, V, seen.data_ptr(), 1, _lib.current_stream_ptr()), "gq_token_set_build")
        _lib.check(L.gq_token_set_build(ids[512:].data_ptr(), 8, V, sup.data_ptr(), 1, _lib.current_stream_ptr()), "gq_token_set_build")
    lp_cap = 8 + PAIRS * (6 + REPLAYS * WINDOWS)  # (the position advances with every draw of the run: a slot for each)
    lws, lraw, ldrawn = z(_lib.SAMPLER_LP_WS, torch.float32), z(lp_cap, torch.float32), z(lp_cap, torch.float32)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731

    def pair():
        a = (logits.data_ptr(), V, top_k, 1.0, temperature, 7, ctr.data_ptr(), wv.data_ptr(), wi.data_ptr(), tok.data_ptr(), pos.data_ptr(),
             nt.data_ptr(), None, None, 0, None, None, 0, None)
        s = _lib.current_stream_ptr()
        if entry == "p":
            _lib.check(L.gq_sample_topk_p(*a, s), "gq_sample_topk_p")
        elif entry == "rep":
            _lib.check(L.gq_sample_topk_rep(*a, rp, ptr(seen), ptr(sup), s), "gq_sample_topk_rep")
        else:
            _lib.check(L.gq_sample_topk_lp(*a, rp, ptr(seen), ptr(sup), lws.data_ptr(), lraw.data_ptr(), ldrawn.data_ptr(), lp_cap, s), "gq_sample_topk_lp")

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pair()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(PAIRS):
            pair()
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    vals = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPLAYS):
            graph.replay()
        b.record()
        torch.cuda.synchronize()
        vals.append(a.elapsed_time(b) * 1e3 / (PAIRS * REPLAYS))
    del graph
    return [round(v, 3) for v in vals]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", required=True)
    ap.add_argument("--vocab", type=int, nargs="+", default=[128256, 151936, 262144])
    ap.add_argument("--top-k", type=int, nargs="+", default=[32, 50])
    ap.add_argument("--entry", choices=("p", "rep", "lp"), default="p")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    import torch
    from guidedquant_amd import _lib
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    rec = dict(library=os.path.relpath(_lib.LIB_PATH, ROOT), entry=args.entry, protocol="%d pairs per graph, %d replays per window, %d windows, T = 0.8; us per pair" % (PAIRS, REPLAYS, WINDOWS))
    for V in args.vocab:
        for k in args.top_k:
            for penalty in {"p": (False,), "rep": (True,), "lp": (False, True)}[args.entry]:
                v = pair_us(V, k, 0.8, dev, args.entry, penalty)
                rec["V%d_k%d%s" % (V, k, "_rp1.05" if penalty and args.entry == "lp" else "")] = dict(us_per_pair=v, median=sorted(v)[len(v) // 2])
    whole = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            whole = json.load(f)
    whole.setdefault("pair_time", {})[args.label] = rec
    with open(args.out, "w") as f:
        json.dump(whole, f, indent=1)
        f.write("\n")
    print(json.dumps({args.label: rec}))


if __name__ == "__main__":
    main()
