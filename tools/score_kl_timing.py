"""What the KL head costs: KL(P || Q) of two sets of final-norm rows over one lm_head, on the Llama-3.1-8B head geometry (dim 4096,
vocabulary 128256), random init, at S = 2048 and 4096 rows.  Three legs, alternating in one process (tools/score_head_q8_timing.py's
protocol: `--rounds` windows per leg and size, a window is `--launches` calls between two events behind 5 warm-up calls):
  kl        (a) gq_head_kl -- native_prompt.kl_head(kernel=True): output.weight streamed once for both models;
  two-nll   (b) two gq_head_nll calls, one per model -- the floor of any scheme that streams output.weight twice; it yields NO KL (the
            logits of the two models never meet), only the two scoring heads' results;
  torch     (c) the torch form -- native_prompt.kl_head(kernel=False): two logit blocks of 512 rows -> fp32 log_softmax -> the sum.
Per leg and size: ms per call (one figure per window, their median and spread) and the peak of torch's allocator above what the model and
the inputs hold (workspaces and, for the torch form, the logit blocks and their fp32 copies).  The record also holds mean KL of the kernel
and the torch form on the same rows and their largest difference.  No threshold is asserted: the record says what came out, including
where the kernel loses.
    python tools/score_kl_timing.py [--rounds 5] [--launches 10] [--layers 1] [--out profiles/score_kl.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (2048, 4096)
LEGS = ("kl", "two-nll", "torch")


def run_leg(model, leg, xq, xp_rows, targets):
    from guidedquant_amd import native_prompt
    if leg == "kl":
        return native_prompt.kl_head(model, xq, xp_rows, True)
    if leg == "torch":
        return native_prompt.kl_head(model, xq, xp_rows, False)
    return model._score_head(xq, targets, True), model._score_head(xp_rows, targets, True)


def window(model, leg, args3, launches):
    """(ms per call, peak bytes above the resident tensors) of one window"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        for _ in range(5):
            run_leg(model, leg, *args3)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        e0.record()
        for _ in range(launches):
            run_leg(model, leg, *args3)
        e1.record()
        torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / launches, 3), int(torch.cuda.max_memory_allocated() - base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--layers", type=int, default=1, help="the legs read the final norm and output.weight only")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "score_kl.json"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU (the HIP path has no fallback)"
    from guidedquant_amd import native_prompt
    from guidedquant_amd.APLinear import APLinear
    from guidedquant_amd.generate import random_init_
    from guidedquant_amd.model import ModelArgs, Transformer, transformer_configs
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(1234)
    cfg = ModelArgs(**dict(transformer_configs["meta-llama/Meta-Llama-3.1-8B"], block_size=max(SIZES), n_layer=args.layers))
    model = Transformer(torch.float16, cfg, linear_class=APLinear, linear_kwargs=dict(bitwidth=2, device=dev))
    model = random_init_(model.to(device=dev, dtype=torch.float16)).eval()
    rec = dict(protocol="random init, Llama-3.1-8B head geometry (dim %d, vocabulary %d); legs alternating in one process, %d windows per leg and size, "
               "%d calls between two events behind 5 warm-up calls; peak_bytes: torch's allocator above the model and the inputs during a window"
               % (cfg.dim, cfg.vocab_size, args.rounds, args.launches), sizes=list(SIZES),
               legs={leg: {"S_%d" % S: dict(ms=[], peak_bytes=0) for S in SIZES} for leg in LEGS}, agreement={})
    g = torch.Generator(device=dev).manual_seed(5)
    rows = {}
    for S in SIZES:  # residual rows of the model under test, final-norm rows of a reference a little away from them, targets for leg (b)
        x = torch.randn(S, cfg.dim, device=dev, generator=g).half()
        xp_rows = model.norm((x.float() + 0.1 * torch.randn(S, cfg.dim, device=dev, generator=g)).half())
        rows[S] = (x, xp_rows, torch.randint(0, cfg.vocab_size, (S, ), dtype=torch.int32, device=dev, generator=g))
        with torch.no_grad():
            a, b = native_prompt.kl_head(model, x, xp_rows, True), native_prompt.kl_head(model, x, xp_rows, False)
        rec["agreement"]["S_%d" % S] = dict(kl_mean_kernel=float(a[0].double().mean()), kl_mean_torch=float(b[0].double().mean()),
                                            max_abs_diff=float((a[0].double() - b[0].double()).abs().max()),
                                            top1_p_equal=float((a[1] == b[1]).double().mean()), top1_q_equal=float((a[2] == b[2]).double().mean()))
        print(json.dumps({"S": S, **rec["agreement"]["S_%d" % S]}), flush=True)
    for r in range(args.rounds):
        for leg in LEGS:
            for S in SIZES:
                cell = rec["legs"][leg]["S_%d" % S]
                ms, peak = window(model, leg, rows[S], args.launches)
                cell["ms"].append(ms)
                cell.update(median_ms=statistics.median(cell["ms"]), spread_ms=[min(cell["ms"]), max(cell["ms"])], peak_bytes=max(cell["peak_bytes"], peak))
            print(json.dumps({"round": r, "leg": leg, **{k: v["ms"][-1] for k, v in rec["legs"][leg].items()}}), flush=True)
        with open(args.out, "w") as f:  # (written round by round: a run cut short leaves what it measured)
            json.dump(rec, f, indent=1)
            f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
