"""Host model of the prompt attention (csrc/prefill_attn.hip, gq_attn_prefill): the mask rule, a float64 reference on the fp16 inputs
as given, and the probe builders of tests/test_prefill_attn_gpu.py.  Plain torch: no GPU, no library.

Layouts of the launch:  q [H][S][hd],  K / V [Hkv][max_seq][hd],  out [S][H * hd].  Query row i has position p = start + i and attends
the cache rows t <= p, with a window W also t > p - W (guidedquant_amd.model.window_mask).

What each probe pins
  count    K = 0 (every attended weight exactly 1 / n), V one-hot by a class of the row: out[i][d] = #attended rows of class d / n --
           every attended row exactly once for every query row, across tile, diagonal and window edges.  Rows of [0, T) outside the
           window hold 65504 in K and V (finite: they must contribute exactly 0); rows >= T hold attn_probes.POISON_BITS.
  profile  scores laid along the keys (attn_probes.PROFILES: ramps, +-300, stairs per key tile, a spike at the own position) or random
           normal q / k / v, against the float64 reference.
"""
import torch

import attn_probes

POISON_BITS = attn_probes.POISON_BITS


def attend_mask(S, start, T, window):
    """bool [S, T]: query row i (position start + i) attends key t"""
    p = start + torch.arange(S)[:, None]
    t = torch.arange(T)[None, :]
    m = t <= p
    return m if not window else m & (t > p - int(window))


def reference(q, K, V, start, scale, window):
    """float64 softmax(scale q k^T + mask) v of the fp16 inputs: q [H, S, hd], K / V [Hkv, >= T, hd] -> [S, H * hd]; rows >= T unread"""
    H, S, hd = q.shape
    G = H // K.shape[0]
    T = start + S
    sc = float(torch.tensor(scale, dtype=torch.float32))
    Kd = K[:, :T].double().repeat_interleave(G, dim=0)
    Vd = V[:, :T].double().repeat_interleave(G, dim=0)
    s = torch.einsum("hsd,htd->hst", q.double(), Kd) * sc
    m = attend_mask(S, start, T, window).to(q.device)
    s = torch.where(m[None], s, torch.full((), -float("inf"), dtype=torch.float64, device=q.device))
    w = torch.softmax(s, dim=-1)
    w = torch.where(m[None], w, torch.zeros((), dtype=torch.float64, device=q.device))  # (exact zeros: 0 x 65504 stays 0)
    return torch.einsum("hst,htd->shd", w, Vd).reshape(S, H * hd)


def poison_rows(K, V, T):
    """rows >= T of both caches: whole rows of NaN, +Inf, -Inf, 65504 in a cycle (stale rows of an earlier sequence)"""
    n = K.shape[1] - T
    if n > 0:
        bits = torch.tensor(POISON_BITS, dtype=torch.int32)[torch.arange(n) % 4].to(torch.int16)
        row = bits.view(torch.float16)[None, :, None]
        K[:, T:] = row
        V[:, T:] = row
    return K, V


def count_probe(H, Hkv, hd, S, start, window, max_seq, coarse):
    """q random (it meets K = 0), K = 0, V one-hot by t % hd (coarse: (t // hd) % hd).  Rows of [0, T) that no query of the launch
    attends (below every row's window) hold 65504 in K and V; a row outside ONE query's window that another query attends keeps its
    one-hot V, and is pinned by the count of the query that must not see it.  Returns q, K, V and the expectation fp16 [S, H * hd]."""
    T = start + S
    g = torch.Generator().manual_seed(1000 * S + 10 * start + (window or 0))
    q = torch.randn(H, S, hd, generator=g).half()
    K = torch.zeros(Hkv, max_seq, hd, dtype=torch.float16)
    t = torch.arange(max_seq)
    cls = ((t // hd) % hd) if coarse else (t % hd)
    V = (cls[:, None] == torch.arange(hd)[None, :]).half()[None].repeat(Hkv, 1, 1)
    m = attend_mask(S, start, T, window)  # [S, T]
    unused = ~m.any(dim=0)  # rows of [0, T) below every query's window
    K[:, :T][:, unused] = 65504.0
    V[:, :T][:, unused] = 65504.0
    onehot = (cls[:T, None] == torch.arange(hd)[None, :]).double()
    cnt = (m.double() @ onehot) / m.double().sum(dim=1, keepdim=True)  # [S, hd]
    expect = cnt.half()[:, None, :].expand(S, H, hd).reshape(S, H * hd).contiguous()
    poison_rows(K, V, T)
    return q, K, V, expect


def profile_scores(name, T, BK, own):
    """the wanted scaled score of every key 0 .. T - 1 for a query whose own position is `own` (float64); differences <= 120"""
    t = torch.arange(T, dtype=torch.float64)
    g = torch.Generator().manual_seed(5)
    jit = (2.0 * torch.rand(4096, generator=g) - 1.0)[:T].double()
    last = max(T - 1, 1)
    if name == "ramp_up":
        return 100.0 * t / last
    if name == "ramp_down":
        return 100.0 * (1.0 - t / last)
    if name == "hi300":
        return 300.0 + jit
    if name == "lo300":
        return -300.0 + jit
    if name in ("stairs_first", "stairs_last"):
        tile = (torch.arange(T) // BK)
        k = tile if name == "stairs_first" else int(tile.max()) - tile
        return -60.0 * (k % 3).double()
    if name in ("cur_above", "cur_below"):
        s = jit.clone()
        s[own] = 100.0 if name == "cur_above" else -100.0
        return s
    raise KeyError(name)


def profile_probe(name, H, Hkv, hd, S, start, max_seq, scale, BK):
    """K rows = multiples of one direction u per KV group, every q row = u (the heads of a group alternate in sign: every second one sees
    -s(t)), so query i of head h sees the scores +-s(t) along the keys; the spike of cur_above / cur_below sits at the LAST query's own
    position.  "random": normal q / k / v.  V uniform in [-2, 2)."""
    T = start + S
    G = H // Hkv
    g = torch.Generator().manual_seed(31 + S + start)
    V = (4.0 * torch.rand(Hkv, max_seq, hd, generator=g) - 2.0).half()
    if name == "random":
        q = torch.randn(H, S, hd, generator=g).half()
        K = torch.randn(Hkv, max_seq, hd, generator=g).half()
    else:
        u = attn_probes.hadamard_q(Hkv, Hkv, hd)  # [Hkv, hd], +-1
        sign = torch.tensor([1.0 if (h % G) % 2 == 0 else -1.0 for h in range(H)])
        q = (u.repeat_interleave(G, dim=0).float() * sign[:, None]).half()[:, None, :].expand(H, S, hd).contiguous()
        s = profile_scores(name, T, BK, T - 1)
        sc = float(torch.tensor(scale, dtype=torch.float32))
        K = torch.zeros(Hkv, max_seq, hd, dtype=torch.float16)
        for kv in range(Hkv):
            ud = u[kv].double()
            K[kv, :T] = ((s / (float(ud @ ud) * sc))[:, None] * ud[None, :]).half()
    poison_rows(K, V, T)
    return q, K, V


def covering_cases(BQ, BK):
    """(S, start, window, max_seq - T, head_dim): every S x window pair, every value of every axis, at most 80 launches.  start, the slack
    behind T and head_dim rotate along the 35 pairs with co-prime periods, so every S meets several starts and both head_dims."""
    Ss = (1, BQ - 1, BQ, BQ + 1, 2 * BQ + 3)
    starts = (0, 1, BK - 1, BK, BK + 5)
    wins = (0, 1, 2, BK - 1, BK, BK + 1, "T+7")
    cases, n = [], 0
    for S in Ss:
        for w in wins:
            start = starts[(n + n // 7) % 5]
            T = start + S
            cases.append((S, start, T + 7 if w == "T+7" else w, (0, 3)[n % 2], (64, 128)[(n // 2 + n // 7) % 2]))
            n += 1
    assert len(cases) <= 80
    for axis, vals in ((0, Ss), (1, starts), (3, (0, 3)), (4, (64, 128))):
        assert {c[axis] for c in cases} == set(vals), (axis, {c[axis] for c in cases})
    return cases
