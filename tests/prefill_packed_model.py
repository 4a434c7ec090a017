"""Host model of the packed prompt attention (csrc/prefill_attn.hip, gq_attn_prefill_packed): the mask rule, a float64 reference on the
fp16 inputs as given, the window of the one-sequence launch a packed row equals bit for bit, and the segment layouts of
tests/test_prefill_packed_attn_gpu.py.  Plain torch: no GPU, no library.

N sequences lie end to end as one run of S rows; seg_begin[i] is the packed row at which row i's own sequence starts (non-decreasing,
seg_begin[i] <= i).  Query row i attends the cache rows max(seg_begin[i], i + 1 - window) <= t <= i (window 0: no window) -- the causal
(and window) masks of the sequences, block-diagonal.
"""
import torch

import prefill_attn_model as pam


def seg_begin_of(lengths):
    """int32 [sum(lengths)]: the packed row at which each row's sequence starts"""
    out, b = [], 0
    for n in lengths:
        out += [b] * n
        b += n
    return torch.tensor(out, dtype=torch.int32)


def lengths_of_cuts(S, cuts):
    """the segment lengths of S rows cut in front of the rows `cuts` (those inside (0, S))"""
    edges = [0] + sorted({c for c in cuts if 0 < c < S}) + [S]
    return [b - a for a, b in zip(edges[:-1], edges[1:])]


def attend_mask_packed(seg_begin, window):
    """bool [S, S]: packed query row i attends cache row t"""
    S = seg_begin.numel()
    i = torch.arange(S)[:, None]
    t = torch.arange(S)[None, :]
    m = (t <= i) & (t >= seg_begin.long()[:, None])
    return m if not window else m & (t > i - int(window))


def row_window(seg_begin, window):
    """w_i of every row: packed row i is row i of gq_attn_prefill(S = i + 1, start = 0, window = w_i) -- the keys back to its segment's
    begin, or the window where that is shorter"""
    w = torch.arange(seg_begin.numel()) - seg_begin.long() + 1
    return [min(int(x), int(window)) if window else int(x) for x in w]


def reference(q, K, V, seg_begin, scale, window):
    """float64 softmax(scale q k^T + mask) v of the fp16 inputs (prefill_attn_model.reference's formula under the packed mask):
    q [H, S, hd], K / V [Hkv, >= S, hd] -> [S, H * hd]; rows >= S unread"""
    H, S, hd = q.shape
    G = H // K.shape[0]
    sc = float(torch.tensor(scale, dtype=torch.float32))
    Kd = K[:, :S].double().repeat_interleave(G, dim=0)
    Vd = V[:, :S].double().repeat_interleave(G, dim=0)
    s = torch.einsum("hsd,htd->hst", q.double(), Kd) * sc
    m = attend_mask_packed(seg_begin.cpu(), window).to(q.device)
    s = torch.where(m[None], s, torch.full((), -float("inf"), dtype=torch.float64, device=q.device))
    w = torch.softmax(s, dim=-1)
    w = torch.where(m[None], w, torch.zeros((), dtype=torch.float64, device=q.device))  # (exact zeros: 0 x 65504 stays 0)
    return torch.einsum("hst,htd->shd", w, Vd).reshape(S, H * hd)


def layouts(S, BQ=64, BK=64):
    """the segment layouts of S rows, name -> lengths: one segment; every segment one row; boundaries at the rows 1, BK - 1, BK, BK + 1;
    a segment astride an edge of the query-tile grid and of the key-tile grid (the two grids coincide at multiples of 64)"""
    assert BQ == BK
    out = {"one": [S]}
    if S > 1:
        out["ones"] = [1] * S
        out["cuts"] = lengths_of_cuts(S, (1, BK - 1, BK, BK + 1))
    if S > BK:
        # (cut in front of the rows 40 and 100: the second segment holds the rows 40 .. 99, astride row 64; at S = 131 the third, astride 128)
        out["astride"] = lengths_of_cuts(S, (40, 100))
    return out
