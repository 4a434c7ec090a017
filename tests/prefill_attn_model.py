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
  sink     sink_first / sink_last (SINK_PROFILES): ONE key at scaled score 0 and every other attended key at ln(0.9) - 25 ln 2, a
           softmax weight of 0.9 * 2^-25 relative to the large key -- under half of the smallest fp16 subnormal, so a weight rounded
           to fp16 at scale 1 is exactly 0 while the fp32 normaliser keeps it.  V is -2 on the large key's row and +2 on every other:
           one sign, so nothing averages out, and T - 1 such keys carry (T - 1) * 0.9 * 2^-25 of the softmax (0.35 % at 2^17 keys).
           sink_first has the large key at position 0 (the running maximum is fixed by the first tile: the pattern of an attention
           sink), sink_last at the last query's own position (every earlier tile is rounded relative to its own maximum and rescaled
           in fp32: nothing is lost at any scale).
  long     long_count_cases / LONG_PROFILE_CASES: the same probes at starts of 2^17 and lengths of 2^17 + 69 and 2^18 + 69 keys --
           thousands of key tiles through the register prefetch, a first tile kt0 near 2000, windows over many tiles.

emulate_row is a float32 emulation of the kernel's online softmax for one query row (tile by tile: running maximum, exp2, the four
lane groups' normaliser shares, P rounded to fp16 into an fp32 numerator), with the scale 2^k at which P is rounded as a switch:
k = 0 is the kernel as first written, k = P_SCALE_LOG2 the kernel as it stands.  error_bound is the bound every float64 comparison
of the prompt attention is held to (the measured worst of every profile: the docstring of tests/test_prefill_attn_gpu.py).
"""
import math

import torch

import attn_probes

POISON_BITS = attn_probes.POISON_BITS
SINK_PROFILES = ("sink_first", "sink_last")
SINK_TAIL = math.log(0.9) - 25.0 * math.log(2.0)  # the tail keys' scaled score: a weight of r = 0.9 of 2^-25, the fp16 flush point
P_SCALE_LOG2 = 15  # csrc/prefill_attn.hip rounds P * 2^15 to fp16 (P <= 1: at most 32768)


def error_bound(T, vmax):
    """|out - float64| of the prompt attention over at most T keys, elementwise: (4 * 2^-11 + (T / 32 + T / 64) * 2^-24) * max|V|.
    P rounded to fp16 costs 2^-11 relative in the numerator and at most as much in the normaliser, the output's own fp16 rounding
    2^-11 -- together under 4 * 2^-11; the fp32 accumulator of the second product is rounded once per MFMA (32 keys) and a lane's
    share of the normaliser once per key tile (64 keys), each by at most 2^-24 relative, all taken with one sign."""
    return (4.0 * 2.0**-11 + (T / 32.0 + T / 64.0) * 2.0**-24) * vmax


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
    lo = max(0, start + 1 - int(window)) if window else 0  # (rows below every query's window: weight exactly 0 -- left out)
    Kd = K[:, lo:T].double().repeat_interleave(G, dim=0)
    Vd = V[:, lo:T].double().repeat_interleave(G, dim=0)
    s = torch.einsum("hsd,htd->hst", q.double(), Kd) * sc
    m = attend_mask(S, start, T, window)[:, lo:].to(q.device)
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
    if name in SINK_PROFILES:
        s = torch.full((T,), SINK_TAIL, dtype=torch.float64)
        s[0 if name == "sink_first" else own] = 0.0
        return s
    g = torch.Generator().manual_seed(5)
    jit = 2.0 * torch.rand(4096, generator=g) - 1.0
    if T > 4096:  # (the first 4096 values are those of every earlier case: the same generator goes on)
        jit = torch.cat([jit, 2.0 * torch.rand(T - 4096, generator=g) - 1.0])
    jit = jit[:T].double()
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
    -s(t)), so query i of head h sees the scores +-s(t) along the keys; the spike of cur_above / cur_below / sink_last sits at the LAST
    query's own position.  "random": normal q / k / v.  V uniform in [-2, 2); sink_first / sink_last: exactly -2 on the large key's row
    and +2 on every other row of [0, T)."""
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
        if name in SINK_PROFILES:
            V[:, :T] = 2.0
            V[:, 0 if name == "sink_first" else T - 1] = -2.0
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


def long_count_cases(BQ, BK):
    """(S, start, window, max_seq - T, head_dim) of the count probe at a far start: S = BQ + 1 (two query tiles, one of a single row),
    every start x window pair; the slack behind T and head_dim rotate along the 8 pairs so that every start and every window meets both
    values of each.  window 0 walks 2049 key tiles per block, the others begin at a first tile kt0 of about 2000."""
    S = BQ + 1
    cases, n = [], 0
    for start in (2**17 - BK + 5, 2**17):
        for w in (0, BK + 1, 4099, "T+7"):
            T = start + S
            cases.append((S, start, T + 7 if w == "T+7" else w, (0, 3)[(n + n // 4) % 2], (64, 128)[(n // 2 + n // 4) % 2]))
            n += 1
    for axis, vals in ((3, (0, 3)), (4, (64, 128))):
        assert {c[axis] for c in cases} == set(vals)
    return cases


# (n_head, n_kv_head, head_dim, T, windows) of the profiles at long T: S = BQ + 3, start = T - S
LONG_PROFILE_CASES = [(2, 1, 128, 2**17 + 69, (0,)), (2, 1, 64, 2**18 + 69, (0, 4099))]


def emulate_row(x, V, BK, k=0, first=0):
    """float32 emulation of the kernel's online softmax for ONE query row.  x: fp32 [T], the scores of the attended keys first ..
    first + T - 1 in the exp2 domain (what the kernel holds after its multiply by scale * log2 e); V: [T, n] (fp16 values).
    Key tiles of BK rows on the cache's tile grid, as the kernel walks them: the running maximum, alpha = exp2(m_run - m_new) and
    P = exp2(x - (m_new - k)) in fp32; a lane group's share of the normaliser (the keys 8 g .. 8 g + 7 of every 32) summed in fp32 in
    the kernel's order; P rounded to fp16 and multiplied into V 32 keys at a time (one MFMA: exact inside, one fp32 rounding onto the
    accumulator).  k: log2 of the scale at which P is rounded (0: unscaled).  Returns float64 [n], (o / l) before the fp16 store."""
    f32 = torch.float32
    T = x.numel()
    x = x.to(f32)
    Vd = V.double()
    m_run = torch.tensor(-1.0e30, dtype=f32)
    l_run = torch.zeros(4, dtype=f32)
    o = torch.zeros(Vd.shape[1], dtype=f32)
    kk = torch.tensor(float(k), dtype=f32)
    a = -(first % BK)  # (the first tile begins on the grid, in front of the first attended key)
    while a < T:
        lo, hi = max(a, 0), min(a + BK, T)
        xs = x[lo:hi]
        m_new = torch.maximum(m_run, xs.max())
        alpha = torch.exp2(m_run - m_new)
        m_run = m_new
        pe = torch.zeros(BK, dtype=f32)
        pe[lo - a:hi - a] = torch.exp2(xs - (m_new - kk))
        lane = pe.view(BK // 32, 4, 8).permute(1, 0, 2).reshape(4, BK // 4)  # lane group g: keys 32 c + 8 g .. + 7, c ascending
        psum = torch.zeros(4, dtype=f32)
        for j in range(BK // 4):
            psum = psum + lane[:, j]
        l_run = l_run * alpha + psum
        ph = pe.half().double()
        o = o * alpha
        for c in range(BK // 32):
            c0, c1 = max(a + 32 * c, 0), min(a + 32 * c + 32, T)
            if c0 < c1:
                o = (o.double() + ph[c0 - a:c1 - a] @ Vd[c0:c1]).to(f32)
        a += BK
    l = (l_run[0] + l_run[1]) + (l_run[2] + l_run[3])  # (the two exchanges at the end: lanes l ^ 16, then l ^ 32)
    return (o * (torch.ones((), dtype=f32) / l)).double()
