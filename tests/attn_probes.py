"""Probes for the decode attention launches (csrc/decode.hip: attn_decode_kernel, attn_roped_kernel, attn_combine_kernel): inputs
whose exact result says WHICH cached rows a launch used, a float64 reference, and a float32 host emulator of the kernels' data flow
that takes injected faults.  Plain torch: no GPU, no library.

What each probe pins
  count    K = 0 (every weight exactly 1), V one-hot by row class: out[d] = #rows of class d / (pos + 1) -- every cached row exactly
           once, anywhere in the context.  (Blind to a loss of k * hd consecutive rows -- a whole split: the needles and the
           staircase profiles see that.)
  needle   one row per head takes the whole softmax (>= 1 - 2^-14): out[h] = V[j_h] -- row j_h is read, and with ITS V row.
  twin     two rows with the same K bits, V = +v and -v/2: out = v/4 -- neither of a pair astride a boundary is dropped or doubled.
  profile  scores laid out along q (ramps, +-300, staircases per split, a spike at the current position): the online softmax's
           rescale paths, against float64.
Rows behind the position hold NaN / +-Inf / 65504 (stale rows of an earlier sequence): they must never reach a result.

Geometry of the launches, restated from csrc/attn_core.h (AttnGeom, attn_solo, attn_per; NW = 8 waves, U = 4 rows in flight per lane group):
  LPP = hd / 8 lanes per row, PPW = 64 / LPP rows per wave instruction, PASS = NW * PPW * U rows per pass of a block
  solo: n_split > 1 and pos + 1 <= 2 PASS -> one block does it all (n_split := 1), no combine
  per = ceil(ceil((pos + 1) / n_split) / PASS) * PASS; split s takes [s per, min(pos + 1, (s + 1) per))
  row t of split [p0, p1): r = t - p0, pass r / PASS, wave (r % PASS) / (PPW U), u = (r % (PPW U)) / PPW, sub = r % PPW;
  stream (wave, sub) keeps a running (max, sum, acc), rescaled once per batch of U rows; streams merged in ascending order; the
  split partials (o, M, l) combined in ascending order (32 from registers, then 8 at a time).
"""
import math
from collections import namedtuple

import torch

NW, U, SPEC, NEG = 8, 4, 32, -3.0e38
NMAX = 64 * 256 + 40  # rows of the noise pools: the longest cache any test uses (64 passes at head_dim 64, + 40)
POISON_BITS = (0x7e00, 0x7c00, 0xfc00, 0x7bff)  # NaN, +Inf, -Inf, 65504
PROFILES = ("ramp_up", "ramp_down", "hi300", "lo300", "stairs_first", "stairs_last", "cur_above", "cur_below")

Geometry = namedtuple("Geometry", "hd pos n_split LPP PPW PASS solo eff_split per splits boundary")


def geometry(hd, pos, n_split):
    LPP = hd // 8
    PPW = 64 // LPP
    PASS = NW * PPW * U
    n = pos + 1
    solo = n_split > 1 and n <= 2 * PASS
    eff = 1 if solo else n_split
    per = -(-(-(-n // eff)) // PASS) * PASS if eff > 1 else n
    splits = [(s * per, min(n, (s + 1) * per)) for s in range(eff)]  # (p0 >= p1: an empty split)
    full = [(a, b) for a, b in splits if a < b]
    B = {0, 1, PPW * U - 1, PPW * U, SPEC - 1, SPEC, SPEC + 1, PASS - 1, PASS, 2 * PASS - 1, 2 * PASS, pos - 1, pos}
    ends = full[:3] + full[-3:]
    for a, b in ends:
        B |= {a - 1, a, b - 1}
    return Geometry(hd, pos, n_split, LPP, PPW, PASS, solo, eff, per, splits, sorted(t for t in B if 0 <= t <= pos))


def twin_pairs(geo):
    """pairs (j, j + 1) astride a boundary: the start of every one of the first / last three splits, and the current position"""
    full = [(a, b) for a, b in geo.splits if a < b]
    P = {a - 1 for a, b in full[:3] + full[-3:] if a >= 1}
    if geo.pos >= 1:
        P.add(geo.pos - 1)
    return sorted(P)


def plan_rows(items, width, H, Hkv, pos):
    """spread `items` (first rows of `width` consecutive planted rows) over launches of H heads: the heads of a KV group get disjoint
    rows.  Free heads repeat items (round robin) where that fits; returns a list of launches, each a list of H rows (None: no row)."""
    items, launches, G = list(items), [], H // Hkv
    i = 0
    while i < len(items) or not launches:
        rows, used = [None] * H, [set() for _ in range(Hkv)]

        def fits(h, j):
            return all(r not in used[h // G] for r in range(j, j + width))
        for h in range(H):
            if i < len(items) and fits(h, items[i]):
                rows[h] = items[i]
                i += 1
            else:  # (a conflict, or nothing left: any item that fits keeps the head busy)
                for k in range(len(items)):
                    j = items[(i + k + h) % len(items)] if items else None
                    if j is not None and fits(h, j):
                        rows[h] = j
                        break
            if rows[h] is not None:
                used[h // G] |= set(range(rows[h], rows[h] + width))
        if all(r is None for r in rows):
            break
        launches.append(rows)
        if not items:
            break
    return launches


# ------------------------------------------------------------------------------------------------------------------ reference
def reference(q, K, V, pos, scale):
    """float64 softmax(q k^T scale) v over rows 0..pos of the fp16 inputs as given (q [H, hd], K / V [Hkv, n, hd], grouped heads);
    scale is the fp32 value the launch gets.  Returns out [H, hd], the weights w [H, pos + 1] and A = sum_t w_t |v_t| [H, hd]."""
    H, Hkv = q.shape[0], K.shape[0]
    G = H // Hkv
    sc = float(torch.tensor(scale, dtype=torch.float32))
    Kd = K[:, :pos + 1].double().repeat_interleave(G, dim=0)
    Vd = V[:, :pos + 1].double().repeat_interleave(G, dim=0)
    s = torch.einsum("hd,htd->ht", q.double(), Kd) * sc
    w = torch.softmax(s, dim=-1)
    return torch.einsum("ht,htd->hd", w, Vd), w, torch.einsum("ht,htd->hd", w, Vd.abs())


# ------------------------------------------------------------------------------------------------------------------ builders
Probe = namedtuple("Probe", "kind q K V expect heads q_in k_in v_in pos max_seq")
# q [H, hd] as the softmax sees it, K / V [Hkv, max_seq, hd] with row pos and the poisoned rows behind it, expect [H, hd] (fp16 for
# the exact probes, None for the profiles: the reference is the expectation), heads: bool [H], the heads whose result is pinned;
# q_in / k_in / v_in: what a launch that rotates (and normalises) the current token itself is handed, K[:, pos] = rot_k(k_in).

_pool = {}


def _noise(name, shape, device, lo, hi, seed):
    """uniform fp16 noise in [lo, hi), generated once per (name, shape, device)"""
    key = (name, tuple(shape), str(device), lo, hi, seed)
    if key not in _pool:
        g = torch.Generator()
        g.manual_seed(seed)
        _pool[key] = (lo + (hi - lo) * torch.rand(shape, generator=g)).half().to(device)
    return _pool[key]


def hadamard_q(H, Hkv, hd, device="cpu"):
    """q heads = rows of the hd-point Sylvester matrix (+-1): the heads of a KV group are mutually orthogonal, every dot product of
    a head with a multiple of a head is exact in fp32"""
    i = torch.arange(hd)
    bits = (i[:, None] & i[None, :])
    par = torch.zeros(hd, hd, dtype=torch.int64)
    for b in range(8):
        par ^= (bits >> b) & 1
    Hm = (1 - 2 * par).half()
    G = H // Hkv
    rows = [1 + 5 * (h % G) + 3 * (h // G) for h in range(H)]  # (distinct inside a group; not row 0, which is constant)
    return Hm[rows].to(device)


def poison(K, V, pos):
    """rows pos + 1 .. of both caches: whole rows of NaN, +Inf, -Inf, 65504 in a cycle"""
    n = K.shape[1] - (pos + 1)
    if n > 0:
        bits = torch.tensor(POISON_BITS, dtype=torch.int32, device=K.device)[torch.arange(n, device=K.device) % 4].to(torch.int16)
        row = bits.view(torch.float16)[None, :, None]
        K[:, pos + 1:] = row
        V[:, pos + 1:] = row
    return K, V


def _ident(x):
    return x


def _finish(kind, q, K, V, expect, heads, q_in, k_in, v_in, pos, max_seq):
    poison(K, V, pos)
    return Probe(kind, q, K, V, expect, heads, q_in, k_in, v_in, pos, max_seq)


def count_probe(H, Hkv, hd, pos, max_seq, q_in=None, rot_q=_ident, rot_k=_ident, device="cpu"):
    assert max_seq > pos + 1
    q_in = hadamard_q(H, Hkv, hd, device) if q_in is None else q_in
    q = rot_q(q_in)
    K = torch.zeros(Hkv, max_seq, hd, dtype=torch.float16, device=device)
    t, d, g = torch.arange(max_seq, device=device), torch.arange(hd, device=device), torch.arange(Hkv, device=device)
    V = (t[None, :, None] % hd == (d[None, None, :] + g[:, None, None]) % hd).half()
    k_in = torch.zeros(Hkv, hd, dtype=torch.float16, device=device)
    K[:, pos] = rot_k(k_in)  # (zero through a rotation or a norm)
    cnt = V[:, :pos + 1].double().sum(1) / (pos + 1)
    expect = cnt.repeat_interleave(H // Hkv, dim=0).half()
    return _finish("count", q, K, V, expect, torch.ones(H, dtype=torch.bool), q_in, k_in, V[:, pos].clone(), pos, max_seq)


def _planted(kind, rows, width, vsign, H, Hkv, hd, pos, max_seq, scale, a, q_in, rot_q, rot_k, zero_cur, device, seed):
    """the needle (width 1) and the twin needle (width 2, V = +v, -v/2): head h owns rows rows[h] .. rows[h] + width - 1"""
    assert max_seq > pos + 1
    G = H // Hkv
    q_in = hadamard_q(H, Hkv, hd, device) if q_in is None else q_in
    q = rot_q(q_in)
    K = _noise("k", (Hkv, NMAX, hd), device, -0.05, 0.05, seed)[:, :max_seq].clone()
    V = _noise("v", (Hkv, NMAX, hd), device, -2.0, 2.0, seed + 1)[:, :max_seq].clone()
    vn = _noise("vn", (H, hd), device, 1.0, 2.0, seed + 2) * (1 - 2 * (_noise("vs", (H, hd), device, 0.0, 1.0, seed + 3 + pos) < 0.5).half())
    k_in = torch.zeros(Hkv, hd, dtype=torch.float16, device=device) if zero_cur else K[:, pos].clone()
    heads = torch.tensor([r is not None for r in rows])
    for h, j in enumerate(rows):
        if j is None:
            continue
        g = h // G
        for i in range(width):
            assert 0 <= j + i <= pos
            K[g, j + i] = (q[h].float() * a).half()
            V[g, j + i] = (vn[h].float() * vsign[i]).half()
            if j + i == pos:
                k_in[g] = (q_in[h].float() * a).half()
    K[:, pos] = rot_k(k_in)
    for h, j in enumerate(rows):  # (a pair's rows carry the same bits, whichever way the current row came about)
        if j is not None and width == 2 and j + 1 == pos:
            K[h // G, j] = K[h // G, pos]
    expect = (vn.float() * 0.25).half() if width == 2 else vn.clone()  # (+v - v/2) / 2
    # the condition of the probe: the planted rows carry all but 2^-14 of the softmax (float64, before anything is launched)
    _, w, _ = reference(q, K, V, pos, scale)
    for h, j in enumerate(rows):
        if j is not None:
            assert float(w[h, j:j + width].sum()) >= 1 - 2.0**-14, (kind, h, j, float(w[h, j:j + width].sum()))
            if width == 2:
                assert float((w[h, j] - w[h, j + 1]).abs()) <= 2.0**-20
    return _finish(kind, q, K, V, expect, heads, q_in, k_in, V[:, pos].clone(), pos, max_seq)


def needle_probe(rows, H, Hkv, hd, pos, max_seq, scale, a=8.0, q_in=None, rot_q=_ident, rot_k=_ident, zero_cur=False, device="cpu", seed=11):
    return _planted("needle", rows, 1, (1.0,), H, Hkv, hd, pos, max_seq, scale, a, q_in, rot_q, rot_k, zero_cur, device, seed)


def twin_probe(rows, H, Hkv, hd, pos, max_seq, scale, a=8.0, q_in=None, rot_q=_ident, rot_k=_ident, zero_cur=False, device="cpu", seed=23):
    return _planted("twin", rows, 2, (1.0, -0.5), H, Hkv, hd, pos, max_seq, scale, a, q_in, rot_q, rot_k, zero_cur, device, seed)


def profile_scores(name, geo, device="cpu"):
    """the wanted scaled score s(t) of every row 0..pos (float64); all differences <= 120"""
    pos, n = geo.pos, geo.pos + 1
    t = torch.arange(n, dtype=torch.float64, device=device)
    jit = _noise("jit", (NMAX,), device, -1.0, 1.0, 5)[:n].double()
    if name == "ramp_up":
        return 100.0 * t / max(pos, 1)
    if name == "ramp_down":
        return 100.0 * (1.0 - t / max(pos, 1))
    if name == "hi300":
        return 300.0 + jit
    if name == "lo300":
        return -300.0 + jit
    if name in ("stairs_first", "stairs_last"):
        full = [(a, b) for a, b in geo.splits if a < b]
        s = torch.zeros(n, dtype=torch.float64, device=device)
        for i, (a, b) in enumerate(full):
            k = i if name == "stairs_first" else len(full) - 1 - i
            s[a:b] = -60.0 * (k % 3)
        return s
    if name in ("cur_above", "cur_below"):
        s = jit.clone()
        s[pos] = 100.0 if name == "cur_above" else -100.0
        return s
    raise KeyError(name)


def profile_probe(name, H, Hkv, hd, pos, n_split, max_seq, scale, q_in=None, rot_q=_ident, rot_k=_ident, device="cpu", seed=31):
    """K rows = multiples of q: head 0 of a group sees s(t), the heads of a group alternate in sign (every second one sees -s(t): the
    rising ramp falls, +300 is -300).  V random.  No expectation of its own: reference() on the rounded inputs is."""
    assert max_seq > pos + 1
    G = H // Hkv
    if q_in is None:
        base = hadamard_q(Hkv, Hkv, hd, device)
        sign = torch.tensor([1.0 if (h % G) % 2 == 0 else -1.0 for h in range(H)], device=device)
        q_in = (base.repeat_interleave(G, dim=0).float() * sign[:, None]).half()
    q = rot_q(q_in)
    geo = geometry(hd, pos, n_split)
    s = profile_scores(name, geo, device)
    sc = float(torch.tensor(scale, dtype=torch.float32))
    K = torch.zeros(Hkv, max_seq, hd, dtype=torch.float16, device=device)
    V = _noise("v", (Hkv, NMAX, hd), device, -2.0, 2.0, seed)[:, :max_seq].clone()
    k_in = torch.zeros(Hkv, hd, dtype=torch.float16, device=device)
    for g in range(Hkv):
        qg, qi = q[g * G].double(), q_in[g * G].double()
        K[g, :pos + 1] = ((s / (float(qg @ qg) * sc))[:, None] * qg[None, :]).half()
        k_in[g] = (float(s[pos]) / (float(qi @ qi) * sc) * qi).half()
    K[:, pos] = rot_k(k_in)
    return _finish(name, q, K, V, None, torch.ones(H, dtype=torch.bool), q_in, k_in, V[:, pos].clone(), pos, max_seq)


# ------------------------------------------------------------------------------------------------------------------ assertions
def ulp_distance(a, b):
    """distance in fp16 steps (sign-magnitude bit patterns mapped to a line); NaN / Inf count as far away"""
    def key(x):
        i = x.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
        return torch.where(i >= 0x8000, 0x8000 - i, i)
    d = (key(a) - key(b)).abs()
    bad = ~torch.isfinite(a.float()) | ~torch.isfinite(b.float())
    return torch.where(bad, torch.full_like(d, 1 << 20), d)


def check_exact(out, probe):
    """count / needle / twin: every element of the pinned heads finite and within 1 fp16 step of the expectation.  Returns the
    worst distance; raises AssertionError naming head and element."""
    out = out.view(probe.expect.shape)
    assert torch.isfinite(out.float()).all(), (probe.kind, probe.pos, "not finite")
    d = ulp_distance(out, probe.expect.to(out.device))[probe.heads.to(out.device)]
    worst = int(d.max()) if d.numel() else 0
    if worst > 1:
        idx = (ulp_distance(out, probe.expect.to(out.device)) * probe.heads.to(out.device)[:, None]).argmax()
        h, e = divmod(int(idx), out.shape[1])
        raise AssertionError("%s probe at pos %d: head %d element %d is %r, expected %r (%d fp16 steps)" %
                             (probe.kind, probe.pos, h, e, float(out[h, e]), float(probe.expect[h, e]), worst))
    return worst


PROFILE_C = 2.0**-14


def profile_ratio(out, probe, scale):
    """worst (|out - ref| - 2^-10 |ref|) / A over the elements (float; inf when something is not finite)"""
    ref, _, A = reference(probe.q, probe.K, probe.V, probe.pos, scale)
    o = out.view(ref.shape).double()
    if not torch.isfinite(o).all():
        return float("inf")
    return float((((o - ref).abs() - 2.0**-10 * ref.abs()) / A).max())


def check_profile(out, probe, scale, c=PROFILE_C):
    r = profile_ratio(out, probe, scale)
    assert r <= c, "%s profile at pos %d: (err - 2^-10 |ref|) / A = %.3e > %.3e" % (probe.kind, probe.pos, r, c)
    return r


# ------------------------------------------------------------------------------------------------------------------ host emulator
FAULTS = ("skip", "double", "vshift", "nomax", "norescale", "droplast", "first32")


def emulate(q, K, V, pos, n_split, scale, fault=None, row=None):
    """float32 emulation of the data flow of one launch + combine.  fault: one of FAULTS; `row` is the row j of skip / double /
    vshift.  Returns fp16 out [H, hd]."""
    assert fault is None or fault in FAULTS
    H, hd = q.shape
    Hkv = K.shape[0]
    G = H // Hkv
    geo = geometry(hd, pos, n_split)
    PPW, PASS = geo.PPW, geo.PASS
    NS = NW * PPW
    f32 = torch.float32
    sc = torch.tensor(scale, dtype=f32)
    n = pos + 1
    Kf = K[:, :n].float().repeat_interleave(G, dim=0)
    vidx = torch.arange(n)
    if fault == "vshift":
        vidx[row] = row + 1  # (K row j with V row j + 1: behind the position that is a stale row)
    Vf = V.float().repeat_interleave(G, dim=0)[:, vidx]
    s = torch.einsum("hd,htd->ht", q.float(), Kf) * sc  # [H, n]
    mult = torch.ones(n, dtype=f32)
    if fault == "skip":
        mult[row] = 0.0
    if fault == "double":
        mult[row] = 2.0
    # index of (wave, u, sub) inside a pass
    wv, uu, sb = torch.meshgrid(torch.arange(NW), torch.arange(U), torch.arange(PPW), indexing="ij")
    off = wv * PPW * U + uu * PPW + sb  # [NW, U, PPW]
    parts = []
    for p0, p1 in geo.splits:
        m_run = torch.full((H, NW, PPW), NEG, dtype=f32)
        s_run = torch.zeros(H, NW, PPW, dtype=f32)
        acc = torch.zeros(H, NW, PPW, hd, dtype=f32)
        for base in range(p0, max(p0, p1), PASS):
            t = base + off
            ok = (t < p1)
            tc = t.clamp(max=n - 1)
            ok = ok & (mult[tc] > 0)
            pu = torch.where(ok[None], s[:, tc], torch.full((), NEG, dtype=f32))  # [H, NW, U, PPW]
            vf = Vf[:, tc]  # [H, NW, U, PPW, hd]
            active = (t[:, 0, 0] < p1)[None, :, None]  # (a wave whose batch starts behind p1 does not run the iteration)
            m_new = torch.maximum(m_run, pu.amax(dim=2))
            if fault == "nomax":
                m_new = torch.zeros_like(m_new)
            resc = torch.exp(m_run - m_new)
            wgt = torch.where(pu > -2.0e38, torch.exp(pu - m_new[:, :, None]), torch.zeros((), dtype=f32)) * mult[tc][None]
            s_new = s_run * resc
            a_new = acc if fault == "norescale" else acc * resc[..., None]
            for u in range(U):
                s_new = s_new + wgt[:, :, u]
                a_new = a_new + wgt[:, :, u, :, None] * torch.where(ok[None, :, u, :, None], vf[:, :, u], torch.zeros((), dtype=f32))
            m_run = torch.where(active, m_new, m_run)
            s_run = torch.where(active, s_new, s_run)
            acc = torch.where(active[..., None], a_new, acc)
        # merge of the streams, ascending
        m_s, l_s, a_s = m_run.reshape(H, NS), s_run.reshape(H, NS), acc.reshape(H, NS, hd)
        M = m_s.amax(dim=1)
        f = torch.exp(m_s - M[:, None])
        o, l = torch.zeros(H, hd, dtype=f32), torch.zeros(H, dtype=f32)
        for i in range(NS):
            l = l + l_s[:, i] * f[:, i]
            o = o + a_s[:, i] * f[:, i, None]
        parts.append((o, M, l))
    if geo.eff_split == 1:
        o, M, l = parts[0]
        return (o / l[:, None]).half()
    if fault == "droplast":
        parts = parts[:max(i for i, (a, b) in enumerate(geo.splits) if a < b)]
    if fault == "first32":
        parts = parts[:32]
    M = torch.stack([p[1] for p in parts]).amax(dim=0)
    o, l = torch.zeros(H, hd, dtype=f32), torch.zeros(H, dtype=f32)
    for po, pM, pl in parts:
        f = torch.exp(pM - M)
        l = l + pl * f
        o = o + po * f[:, None]
    return (o / l[:, None]).half()


def contexts(hd):
    """the (pos, n_split) of the GPU tests, in four groups"""
    P = geometry(hd, 0, 1).PASS
    short = [(p, ns) for p in (0, 1, 15, 16, 17, 31, 32, 33) for ns in (1, 4)]
    solo = [(p, ns) for p in (2 * P - 2, 2 * P - 1, 2 * P) for ns in (1, 2, 4)]
    jump = [(ns * P + d, ns) for ns in (4, 5, 8) for d in (-1, 0, 1)]
    wide = [(p, ns) for ns in (33, 64) for p in (3 * P, 64 * P - 1, 64 * P)]
    return dict(short=short, solo=solo, jump=jump, wide=wide)


def profile_names(hd, pos, n_split):
    """which score profiles a context runs"""
    P = geometry(hd, 0, 1).PASS
    if (n_split == 8 and pos in (8 * P - 1, 8 * P, 8 * P + 1)) or (n_split == 64 and pos == 64 * P - 1):
        return PROFILES
    if pos == 33:
        return ("hi300", "lo300", "cur_above", "cur_below")
    return ()


def default_scale(hd):
    return 1.0 / math.sqrt(hd)
