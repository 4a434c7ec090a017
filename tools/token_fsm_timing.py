"""What a token-level state machine (constrained decoding, token_fsm) costs inside the fused sampler, per draw and per token of the captured
decode step.  The protocol of tools/sampler_adjust_timing.py.

  draws     gq_sample_topk_fsm against gq_sample_topk_rep (top_k 50, T 0.8) and gq_sample_full_fsm against gq_sample_full (no top-k, top_p
            0.9) over 128256 and 151936 gaussian logits, with machines of 1, 64 and 4096 states.  Every state allows everything but 300
            tokens of its own (300 edges: the transition's binary search has nine rounds) and leads to the next state, so every draw reads
            another mask row; the other leg suppresses a static set of the same population (300 tokens).  ONE process, alternating legs: a
            window is `draws` consecutive calls on one stream between two events; per leg the windows' us per draw, the best and the
            median, and the difference of the medians.
  decode    tokens/s of the captured random-init Meta-Llama-3-8B 2-bit step (bench.py's protocol: ten token steps per replay, the embedding
            folded, greedy top_k 32, sequences of 100 new tokens from a BOS prompt) with a one-state machine that allows every token
            (gq_sample_topk_fsm, `reset_fsm` before every sequence) and without (gq_sample_topk_p): TWO graphs over ONE model, alternating
            windows.

Writes profiles/token_fsm.json and prints the record.
    python tools/token_fsm_timing.py [--draws 200] [--steps 200] [--warmup 20] [--repeats 5] [--no-decode]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "token_fsm.json")
LLAMA = "meta-llama/Meta-Llama-3-8B"
SEQ_NEW_TOKENS, SPR = 100, 10
VOCABS, STATES, FORBIDDEN = (128256, 151936), (1, 64, 4096), 300


def _summary(v):
    return dict(us_per_draw=[round(x, 2) for x in v], best=round(min(v), 2), median=round(statistics.median(v), 2))


def ring_tables(S, V):
    """CSR tables of S states: state s forbids FORBIDDEN tokens of its own (a stride through the vocabulary from an offset of its own: no
    token twice) and everything else leads to state s + 1"""
    import numpy as np
    assert FORBIDDEN * 401 < V
    off = (np.arange(S, dtype=np.int64) * 7919) % V
    tok = np.sort((off[:, None] + np.arange(FORBIDDEN, dtype=np.int64)[None, :] * 401) % V, axis=1)
    row_ptr = np.arange(S + 1, dtype=np.int32) * FORBIDDEN
    return row_ptr, tok.reshape(-1).astype(np.int32), np.full(S * FORBIDDEN, -1, dtype=np.int32), ((np.arange(S) + 1) % S).astype(np.int32), tok[0]


def make_draw(V, S, full, fsm, dev):
    """one leg: a closure that makes one draw on the current stream (its state lives in the closure)"""
    import torch
    from guidedquant_amd import _lib
    L = _lib.lib()
    g = torch.Generator(device="cpu")
    g.manual_seed(V + S)
    logits = (torch.randn(V, generator=g) * 2).to(torch.float16).to(dev)

    def z(n, dtype=torch.int32):
        return torch.zeros(int(n), dtype=dtype, device=dev)
    words = (V + 31) // 32
    counter, tok, pos, nxt = z(1), z(1), z(1), z(1)
    s = _lib.current_stream_ptr()
    tables = ring_tables(S, V)
    keep = [logits, counter, tok, pos, nxt]
    suppress = machine = None
    if fsm:
        dt = [torch.from_numpy(a).to(dev) for a in tables[:4]]
        masks, state = z(S * words), z(1)
        _lib.check(L.gq_token_fsm_build(*(t.data_ptr() for t in dt), S, V, None, masks.data_ptr(), s), "gq_token_fsm_build")
        machine = _lib.GqTokenFsm(masks.data_ptr(), words, S, *(t.data_ptr() for t in dt), state.data_ptr())
        keep += dt + [masks, state, machine]
    else:  # a static set of the same population: state 0's
        ids = torch.from_numpy(tables[4].astype("int32")).to(dev)
        suppress = z(words)
        _lib.check(L.gq_token_set_build(ids.data_ptr(), ids.numel(), V, suppress.data_ptr(), 1, s), "gq_token_set_build")
        keep += [ids, suppress]
    sup = suppress.data_ptr() if suppress is not None else None
    if full:
        ws = z(L.gq_sample_full_ws_bytes(V) // 8, torch.int64)
        keep.append(ws)
        args = (logits.data_ptr(), V, 0, 0.9, 0.0, 0.8, 7, counter.data_ptr(), ws.data_ptr(), ws.numel() * 8, tok.data_ptr(), pos.data_ptr(), nxt.data_ptr(),
                None, None, 0, None, None, 0, None, 1.0, None, sup, None, None, 0)
        name = "gq_sample_full_fsm" if fsm else "gq_sample_full"
    else:
        wv, wi = z(128 * 64, torch.float32), z(128 * 64)
        keep += [wv, wi]
        args = (logits.data_ptr(), V, 50, 1.0, 0.8, 7, counter.data_ptr(), wv.data_ptr(), wi.data_ptr(), tok.data_ptr(), pos.data_ptr(), nxt.data_ptr(),
                None, None, 0, None, None, 0, None, 1.0, None, sup)
        name = "gq_sample_topk_fsm" if fsm else "gq_sample_topk_rep"
        if fsm:
            args += (None, None, None, 0)
    if fsm:
        args += (0, None, None, None, None, ctypes.byref(machine))
    fn = getattr(L, name)

    def draw():
        _lib.check(fn(*args, _lib.current_stream_ptr()), name)
    draw.keep = keep
    return draw


def draws(dev, n, repeats):
    import torch
    rec = {}
    for full in (False, True):
        for V in VOCABS:
            for S in STATES:
                legs = {fsm: make_draw(V, S, full, fsm, dev) for fsm in (False, True)}
                vals = {a: [] for a in legs}
                for d in legs.values():
                    for _ in range(20):
                        d()
                torch.cuda.synchronize()
                for _ in range(repeats):
                    for a, d in legs.items():  # alternating: a drift of the box falls on both legs
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(n):
                            d()
                        e1.record()
                        e1.synchronize()
                        vals[a].append(1e3 * e0.elapsed_time(e1) / n)
                base, new = ("gq_sample_full", "gq_sample_full_fsm") if full else ("gq_sample_topk_rep", "gq_sample_topk_fsm")
                r = {base: _summary(vals[False]), new: _summary(vals[True])}
                r["fsm_us_per_draw"] = round(r[new]["median"] - r[base]["median"], 2)
                rec["%s_v%d_states%d" % ("full" if full else "topk", V, S)] = r
                del legs
    return rec


def make_runner(model, dev, fsm):
    import torch
    from guidedquant_amd.generate import DecodeGraph
    from guidedquant_amd.token_fsm import TokenFSM
    graph = DecodeGraph(model, dev, native_sampling=True, temperature=0.0, top_k=32, fold_embed=True, steps_per_replay=SPR,
                        token_fsm=TokenFSM(1, [], default_next=[0]) if fsm else None)
    assert graph.native_sampling and (graph.sampler.token_fsm is not None) == fsm
    bos = torch.tensor([[128000]], dtype=torch.int32, device=dev)
    zero = torch.zeros((1, ), dtype=torch.int32, device=dev)

    def run_steps(n):
        done = 0
        while done < n:
            graph.set_token(bos, zero)
            graph.reset_fsm()  # (one small fill per 100 tokens on the machine's leg; nothing on the other)
            k = min(SEQ_NEW_TOKENS, n - done)
            for _ in range(k // SPR):
                graph.step()
            for _ in range(k % SPR):
                graph.step_one()
            done += k

    run_steps(2 * SEQ_NEW_TOKENS)  # (both captured graphs replayed, clocks up: set-up, outside every timed window)
    graph.step_one()
    torch.cuda.synchronize()
    return graph, run_steps


def decode(dev, steps, warmup, repeats):
    import torch
    from guidedquant_amd.APLinear import APLinear
    from guidedquant_amd.generate import random_init_
    from guidedquant_amd.model import ModelArgs, Transformer, transformer_configs
    torch.manual_seed(1234)
    model = Transformer(torch.float16, ModelArgs(**transformer_configs[LLAMA]), linear_class=APLinear, linear_kwargs=dict(bitwidth=2, device=dev))
    model = random_init_(model.to(device=dev, dtype=torch.float16)).eval()
    model.setup_caches(1, SEQ_NEW_TOKENS + 1)
    assert model.native_ready(), "the fused HIP decode step does not serve this model"
    legs = {fsm: make_runner(model, dev, fsm) for fsm in (False, True)}
    vals = {fsm: [] for fsm in legs}
    for _ in range(repeats):
        for fsm, (graph, run_steps) in legs.items():
            run_steps(warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_steps(steps)
            torch.cuda.synchronize()
            vals[fsm].append(steps / (time.perf_counter() - t0))
    for g, _ in legs.values():
        g.close()
    rec = dict(model=model.config.model_name, n_layer=model.config.n_layer, vocab_size=model.config.vocab_size)
    for fsm, v in vals.items():
        rec["token_fsm" if fsm else "plain"] = dict(tok_s=[round(x, 2) for x in v], best=round(max(v), 2), median=round(statistics.median(v), 2),
                                                    us_per_token_median=round(1e6 / statistics.median(v), 2))
    a, b = rec["plain"]["us_per_token_median"], rec["token_fsm"]["us_per_token_median"]
    rec["fsm_us_per_token"] = round(b - a, 2)
    rec["fsm_per_cent"] = round(100.0 * (b - a) / a, 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=200)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-decode", action="store_true")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU (the HIP path has no fallback)"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rec = dict(protocol="draws: %d alternating windows of %d calls per leg between two events, 20 calls before; top_k 50 / T 0.8 (two-stage), no top-k / "
               "top_p 0.9 (whole vocabulary); the machine's states forbid %d tokens each (a row of %d edges) and lead to the next state, the other leg "
               "suppresses a static set of %d tokens.  decode: random init, 2-bit, DecodeGraph with %d steps per replay, embedding folded, greedy top_k 32, "
               "sequences of %d new tokens, a one-state machine that allows every token; %d alternating windows of %d token steps per leg behind %d "
               "warm-up steps, host clock ending in a synchronise"
               % (args.repeats, args.draws, FORBIDDEN, FORBIDDEN, FORBIDDEN, SPR, SEQ_NEW_TOKENS, args.repeats, args.steps, args.warmup),
               draws=draws(dev, args.draws, args.repeats))
    if not args.no_decode:
        rec["decode"] = decode(dev, args.steps, args.warmup, args.repeats)
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
