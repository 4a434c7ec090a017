"""Host model of the two log-probabilities gq_sample_topk_lp leaves next to gq_sample_topk_rep's draw (include/gq_hip.h), in numpy and
float64.  Like tests/sampler_model.py and tests/sampler_rep_model.py, whose pieces it is built from, it restates the CONTRACT, not the
kernels: no slices, partials or workspaces appear here.

One draw at position p with token `tok` (the draw itself is sampler_rep_model's: this model is TEACHER-FORCED with the tokens a device run
drew, and says what the two numbers of each of them must be)
  slot      i = p + 1, the index seq_out uses; two floats are written when i < lp_cap, nothing else is touched
  lp_raw    v_tok - log sum_t exp(v_t) over ALL vocab tokens, v_t the fp16 logit: banned, suppressed and penalised tokens count with
            their raw value, a -inf logit contributes 0
  lp_drawn  a_tok - log sum_{c in C} exp(a_c), C the kept candidates of the draw (suppress / ban, penalty, top-k, nucleus -- as
            sampler_rep_model.run forms them), a_c = fl32(s_c / max(T, 1e-5)): the fp32 quotient the race forms; the sum in float64.
            A one-member C gives exactly 0
  empty C   both are NaN (the token is EMPTY_TOKEN)
Logits with +inf, or all -inf: unspecified (`specified`).  A NaN logit is no candidate (sampler_model.py): lp_drawn is taken over the kept
candidates as ever, and lp_raw, whose sum runs over ALL tokens, is NaN for every draw (`lse64` returns NaN); all logits NaN: empty C.

Which draws' lp_drawn a device run may decide differently: the kept set is key-exact behind top-k; behind a nucleus it depends on an fp32
cumulative sum against 1 - top_p.  A draw whose nearest cumulative sum lies within NUCLEUS_GRANT = 1e-5 of the threshold -- the distance
the sampler tests ask of every case but the one built on the threshold -- has `decided` False and is not compared.

ref_err(x): the yardstick of the GPU test's bound, the largest finite-entry error of torch's CPU fp32 log_softmax against float64 on x.

`fault=` injects one deviation (FAULTS), for tests/test_sampler_lp_model_cpu.py only.
"""
from collections import namedtuple

import numpy as np

import sampler_model as sm
import sampler_rep_model as rm
from sampler_rep_model import EMPTY_TOKEN  # noqa: F401

FAULTS = ("raw_without_banned", "raw_penalised", "slot_p", "drawn_no_temperature", "drawn_no_nucleus", "drawn_over_vocab")
NUCLEUS_GRANT = 1e-5


def lse64(x):
    """log sum exp of the finite-or--inf entries of x in float64 (-inf for none)"""
    x = np.asarray(x, dtype=np.float64)
    m = x.max() if x.size else -np.inf
    if not np.isfinite(m):
        return float(m)
    return float(m + np.log(np.exp(x - m).sum()))


def ulp32(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def ref_err(x):
    """largest |torch CPU fp32 log_softmax - float64 log_softmax| over the finite entries, on the fp32 values of x"""
    import torch
    x32 = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    got = torch.log_softmax(torch.from_numpy(x32.copy()), dim=0).numpy().astype(np.float64)
    want = x32.astype(np.float64) - lse64(x32)
    ok = np.isfinite(want)
    return float(np.abs(got[ok] - want[ok]).max()) if ok.any() else 0.0


def specified(logits):
    x = np.asarray(logits, dtype=np.float32)
    return not (np.isnan(x).any() or (x == np.inf).any() or not np.isfinite(x).any())


Draw = namedtuple("Draw", "slot raw drawn ids a decided member lse_raw lse_drawn")
Run = namedtuple("Run", "draws raw drawn")


def run(logits, tokens, top_k, T, top_p=1.0, pos=0, ban=None, rp=1.0, seen0=(), suppress=(), lp_cap=0, fault=None):
    """tokens: what a device run drew, in order.  Returns Run(draws, raw, drawn): per draw a Draw (slot = the index written or None; raw,
    drawn = the two numbers; ids, a = the kept candidates and their fp32 a_c; decided; member = the token is one of them; the two
    log-sums), and the two arrays as dicts slot -> value."""
    logits = np.ascontiguousarray(logits, dtype=np.float16)
    V = logits.size
    k = min(max(top_k, 1), 32 if top_k <= 32 else 64)
    Tq = max(np.float32(T), np.float32(1e-5))
    v32 = logits.astype(np.float32)
    dead = np.zeros(V, dtype=bool)
    dead[np.asarray([t for t in suppress if 0 <= t < V], dtype=np.int64)] = True
    dead[np.isnan(v32)] = True  # (no candidate; in lp_raw's sum over ALL tokens it counts as what it is: the sum is NaN)
    static = np.lexsort((np.arange(V), -rm.image32(v32)))
    static = static[~dead[static]]
    nb, until, bids = (ban[0], ban[1], [b for b in ban[2][:ban[0]] if 0 <= b < V]) if ban is not None and ban[0] > 0 else (0, 0, [])
    seen, seen_ids = np.zeros(V, dtype=bool), []
    track = np.float32(rp) != np.float32(1.0)  # (without a penalty the history changes nothing)
    for t in seen0 if track else ():
        if 0 <= t < V and not seen[t]:
            seen[t] = True
            seen_ids.append(int(t))
    full = lse64(v32)
    draws, raw, drawn = [], {}, {}
    memo = {}
    for i, tok in enumerate(int(t) for t in tokens):
        banned = bids if (nb and pos + i < until) else []
        key = (bool(banned), len(seen_ids))
        if key not in memo:  # (the seen set only grows: its size names it within one run)
            head = static[:k + len(seen_ids) + len(banned)]
            head = head[~seen[head]]
            sid = np.asarray(seen_ids, dtype=np.int64)
            sid = sid[~dead[sid]] if sid.size else sid
            ids = np.concatenate([head, sid])
            s = np.concatenate([v32[head], rm.penalised(v32[sid], rp)]).astype(np.float32)
            if banned:
                live = ~np.isin(ids, banned)
                ids, s = ids[live], s[live]
            sel = np.lexsort((ids, -rm.image32(s)))[:k]
            ids, s = ids[sel], s[sel]
            dist = np.inf
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                a = (s / Tq).astype(np.float32) if fault != "drawn_no_temperature" else s.copy()
            if ids.size and fault != "drawn_no_nucleus":
                keep, dist = sm.nucleus((s.astype(np.float64) / float(Tq)), ids, top_p)
                ids, s, a = ids[keep], s[keep], a[keep]
            memo = {key: (ids, s, a, dist)}
        ids, s, a, dist = memo[key]
        slot = pos + i + (0 if fault == "slot_p" else 1)
        if tok == EMPTY_TOKEN or not ids.size:
            r = d = lr = ld = float("nan")
            member = tok == EMPTY_TOKEN and not ids.size
        else:
            hit = np.nonzero(ids == tok)[0]  # (no member: only where the device may keep another set -- an undecided nucleus)
            member = hit.size == 1
            lr = full
            if fault == "raw_without_banned":
                out = dead.copy()
                out[banned] = True
                lr = lse64(v32[~out])
            vt = float(s[hit[0]]) if fault == "raw_penalised" and member else float(v32[tok])
            r = vt - lr
            ld = lse64(a) if fault != "drawn_over_vocab" else lse64((v32 / Tq).astype(np.float32))
            if not member:
                d = float("nan")
            else:
                d = float(a[hit[0]]) - ld if ids.size > 1 or fault == "drawn_over_vocab" else 0.0
        written = slot if 0 <= slot < lp_cap else None
        draws.append(Draw(written, r, d, ids, a, bool(dist >= NUCLEUS_GRANT), bool(member), lr, ld))
        if written is not None:
            raw[written], drawn[written] = r, d
        if track and 0 <= tok < V and not seen[tok]:
            seen[tok] = True
            seen_ids.append(tok)
    return Run(draws, raw, drawn)


def case_args(c):
    """run()'s keyword arguments of a case of sampler_model.CASES (entry ex / p) or of sampler_rep_model.CASES, and its logits"""
    if hasattr(c, "rp"):
        x, seen0, suppress, ban = rm.case_inputs(c)
        return x, dict(top_k=c.top_k, T=c.T, top_p=c.top_p, pos=c.pos0, ban=ban, rp=c.rp, seen0=seen0, suppress=suppress)
    x, ban = sm.case_inputs(c)
    return x, dict(top_k=c.top_k, T=c.T, top_p=c.top_p, pos=c.pos0, ban=ban)


ALL_CASES = [c for c in sm.CASES if c.entry in ("ex", "p")] + list(rm.CASES)
CASE_BY_NAME = {c.name: c for c in ALL_CASES}
assert len(CASE_BY_NAME) == len(ALL_CASES)
