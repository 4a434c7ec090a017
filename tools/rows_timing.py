"""The row-write entries of the prompt pass alone, two builds of the library against each other (needs the GPU):
    python tools/rows_timing.py OLD/libgq_hip.so NEW/libgq_hip.so [--rounds 4] > profiles/rows_unified.json
    python tools/rows_timing.py OLD/libgq_hip.so NEW/libgq_hip.so --entries kv8 > profiles/kv8_rows_nan.json
gq_rope_cache_rows and gq_qknorm_rope_cache_rows on the 8B geometry (32 / 8 heads, head_dim 128) at S = 128 and S = 4096 rows, random fp16
rows, positions 0 .. S - 1 of a 4096-row cache.  --entries kv8: gq_rope_cache_rows_kv8 instead, its plain, qknorm and bias forms at S = 1 (the
decode step), 128 and 4096 into fp8 caches, reciprocal scales 1 / 0.37 and 1 / 2.9.  One child process per leg (GQ_LIB_PATH picks its
library); a round is the legs OLD, OLD, NEW in turn, so OLD is measured against itself (A/A) in the scheme that compares NEW with it.  A child times each case as `--reps` batches
of `--launches` launches between two events behind a warm-up and reports the median batch in us per launch.  The record: every child's
figures and per case `old_range_us` (all 2 x rounds medians of OLD), `aa_spread_us` (the largest |OLD - OLD| inside a round),
`new_median_us` (the median of NEW's medians), `within` = it lies inside the range widened by the spread on both sides, `slower` = it lies
above.  The verdicts go to stderr too, and the exit status is 1 when a case is `slower`."""
import argparse
import json
import os
import statistics
import subprocess
import sys

H, HKV, HD, MAX_SEQ = 32, 8, 128, 4096
FP16_CASES = [(entry, S) for entry in ("gq_rope_cache_rows", "gq_qknorm_rope_cache_rows") for S in (128, 4096)]
KV8_CASES = [(f"gq_rope_cache_rows_kv8 {form}", S) for form in ("plain", "qknorm", "bias") for S in (1, 128, 4096)]


def leg(a):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from guidedquant_amd import _lib
    L = _lib.lib()
    d = torch.device("cuda:0")
    g = torch.Generator(device=d).manual_seed(0)
    f16 = dict(dtype=torch.float16, device=d)
    cos, sin = torch.rand((MAX_SEQ, HD), generator=g, **f16), torch.rand((MAX_SEQ, HD), generator=g, **f16)
    kc, vc = torch.zeros((HKV, MAX_SEQ, HD), **f16), torch.zeros((HKV, MAX_SEQ, HD), **f16)  # (the fp8 entry fills the first half of them)
    k_inv, v_inv = torch.full((HKV, ), 1 / 0.37, device=d), torch.full((HKV, ), 1 / 2.9, device=d)
    qn, kn = 1 + 0.1 * torch.randn(HD, generator=g, **f16), 1 + 0.1 * torch.randn(HD, generator=g, **f16)
    st = _lib.current_stream_ptr()
    out = {}
    for entry, S in case_list(a.entries):
        qkv = torch.randn((S, (H + 2 * HKV) * HD), generator=g, **f16)
        pos = torch.arange(S, dtype=torch.int32, device=d)
        q = torch.empty((H, S, HD), **f16)
        head = (qkv.data_ptr(), pos.data_ptr(), cos.data_ptr(), sin.data_ptr(), q.data_ptr(), kc.data_ptr(), vc.data_ptr())
        if entry.startswith("gq_rope_cache_rows_kv8"):
            form = entry.split()[1]
            bias = torch.randn((H + 2 * HKV) * HD, generator=g, **f16)
            norm = (qn.data_ptr(), kn.data_ptr()) if form == "qknorm" else (None, None)
            args = (*head, k_inv.data_ptr(), v_inv.data_ptr(), S, H, HKV, HD, MAX_SEQ, *norm, 1e-6, bias.data_ptr() if form == "bias" else None, st)
        else:
            norm = (qn.data_ptr(), kn.data_ptr(), 1e-6) if entry == "gq_qknorm_rope_cache_rows" else ()
            args = (*head, S, H, HKV, HD, MAX_SEQ, *norm, st)
        fn = getattr(L, entry.split()[0])
        n = a.launches if S > 1024 else 4 * a.launches
        for _ in range(50):
            _lib.check(fn(*args), entry)
        torch.cuda.synchronize()
        us = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn(*args)
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / n)
        out[f"{entry} S={S}"] = dict(median_us=round(statistics.median(us), 3), min_us=round(min(us), 3), max_us=round(max(us), 3), launches=n)
    print(json.dumps(out))


def case_list(entries):
    return KV8_CASES if entries == "kv8" else FP16_CASES


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--entries", choices=("fp16", "kv8"), default="fp16")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--leg", action="store_true", help="(internal) one child: time the library of GQ_LIB_PATH")
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    assert len(a.libs) == 2, __doc__
    runs = {"old": [], "old_again": [], "new": []}
    for _ in range(a.rounds):
        for side, lib in (("old", a.libs[0]), ("old_again", a.libs[0]), ("new", a.libs[1])):
            env = dict(os.environ, GQ_LIB_PATH=os.path.abspath(lib))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "--reps", str(a.reps), "--launches", str(a.launches), "--entries", a.entries],
                               env=env, capture_output=True, text=True, timeout=240)
            if r.returncode != 0:  # (nothing more is started on the GPU behind a child that failed)
                sys.exit(f"{side} child failed ({r.returncode}): {r.stderr[-2000:]}")
            runs[side].append(json.loads(r.stdout.strip().split("\n")[-1]))
    cases = {}
    for entry, S in case_list(a.entries):
        key = f"{entry} S={S}"
        old, again, new = ([r[key]["median_us"] for r in runs[side]] for side in ("old", "old_again", "new"))
        lo, hi = min(old + again), max(old + again)
        spread = round(max(abs(x - y) for x, y in zip(old, again)), 3)
        med = statistics.median(new)
        cases[key] = dict(old_medians_us=old, old_again_medians_us=again, new_medians_us=new, old_range_us=[lo, hi], aa_spread_us=spread, new_median_us=med,
                          within=bool(lo - spread <= med <= hi + spread), slower=bool(med > hi + spread))
        print(f"{key}: OLD {lo} .. {hi} us, A/A spread {spread}, NEW {med} -> {'SLOWER' if cases[key]['slower'] else 'within' if cases[key]['within'] else 'faster'}",
              file=sys.stderr)
    print(json.dumps(dict(what=f"{a.entries} row-write entries alone; rounds of OLD, OLD, NEW in child processes; us per launch, median of "
                               f"{a.reps} batches per child behind 50 warm-up launches", geometry=dict(n_head=H, n_kv_head=HKV, head_dim=HD, max_seq=MAX_SEQ),
                          rounds=a.rounds, cases=cases, runs=runs), indent=1))
    return 1 if any(c["slower"] for c in cases.values()) else 0


if __name__ == "__main__":
    sys.exit(main())
