"""The HIP prompt pass: the host side of `Transformer.prefill_native` and `Transformer.score_native` -- a prompt of S > 1 tokens, batch 1,
through the C ABI (include/gq_hip.h) and the quantized linears' own forwards.

  * `prompt_pass`: the chunk loop (`prefill_chunks`: chunks outer, layers inner, over the same caches) and what it decides once per pass --
    `attention_plan`, a pure function of the GQ_PREFILL_ATTN mode, the number of pieces, the cache format and the library's answer.
  * `_Piece`: one piece through every layer.  Per layer, the step list of `_Piece.layers`:
        RMSNorm rows (+ the residual add in front) -> wqkv -> RoPE + KV-cache rows + attention (`rows_and_attention`: THE place that picks
        the row-write entry and the attention) -> wo -> RMSNorm rows (+ residual) -> w1w3 -> silu * up -> w2
    with the element-wise steps as one launch each (csrc/prefill.hip) and the attention as gq_attn_prefill / _kv8 (csrc/prefill_attn.hip) or
    torch SDPA over the cache rows [0, start + S).
  * the heads: logits (`Transformer.output`), or the scoring head (`score_head`: gq_head_nll, or log_softmax in row blocks), chosen by
    `score_head_choice`, a pure function of the GQ_SCORE_HEAD mode.

  * packed scoring: `pack_plan` (first fit in input order) and `score_packed` -- several short sequences as ONE piece, `_PackedPiece`'s
    `rows_and_attention` through gq_rope_cache_rows_packed and gq_attn_prefill_packed (or SDPA under the block-diagonal `packed_mask`).

`Transformer` keeps `prefill_ready`, `prefill_native`, `score_native` and `_score_head` as delegations to this module, and the attributes the
pass reads and writes on the model (`last_prefill_plan`, `SCORE_HEAD_ROWS`, `SCORE_HEAD_AUTO`).  What a pass launches, in which order, with
which arguments, is pinned by tests/golden/prefill_calls.json.
"""
import math
import os
from typing import Optional

import torch
from torch import Tensor
from torch.nn import functional as F

from . import _lib, native_step


def mask_rows(input_pos: Tensor, n: int, window: Optional[int] = None) -> Tensor:
    """bool [len(input_pos), n]: the rows `window_mask(m, window)[input_pos, :n]` of any table of m >= n rows, built from the positions on
    the spot -- key t is attended by the query at position p when t <= p, and with a window also t > p - window"""
    p = input_pos.long()[:, None]
    t = torch.arange(n, device=input_pos.device)[None, :]
    m = t <= p
    return m if window is None else m & (t > p - int(window))


def prefill_chunks(S: int, chunk: int, start: int = 0):
    """the (start, S) pieces a prompt of S tokens at position `start` is passed in: whole chunks in order, then the tail (one token included)"""
    assert S >= 1 and chunk >= 1
    return [(start + a, min(chunk, S - a)) for a in range(0, S, chunk)]


_SDPA_GQA = [True]  # F.scaled_dot_product_attention(enable_gqa=True): grouped K / V heads without the repeat_interleave copies


def _sdpa_gqa(q, k, v, mask, rep):
    """q [1, H, S, hd], k / v [1, Hkv, T, hd] (views of the cache), causal when mask is None.  Bit-identical to the form with the
    K / V heads repeated (measured on this stack: 21.6 vs 34.3 us at S = 128); older torch versions take the copies."""
    if _SDPA_GQA[0] and rep > 1:
        try:
            return F.scaled_dot_product_attention(q, k, v, attn_mask=mask, dropout_p=0.0, is_causal=mask is None, enable_gqa=True)
        except (TypeError, RuntimeError):
            _SDPA_GQA[0] = False
    if rep > 1:
        Hkv, T, hd = k.shape[1], k.shape[2], k.shape[3]
        k = k[0].unsqueeze(1).expand(Hkv, rep, T, hd).reshape(1, Hkv * rep, T, hd)
        v = v[0].unsqueeze(1).expand(Hkv, rep, T, hd).reshape(1, Hkv * rep, T, hd)
    return F.scaled_dot_product_attention(q, k, v, attn_mask=mask, dropout_p=0.0, is_causal=mask is None)


# ------------------------------------------------------------------------------------------------ what a pass decides on the host
def attention_plan(mode: str, n_pieces: int, kv8: bool, supported: bool) -> str:
    """the attention of every layer of a pass: "hip" (gq_attn_prefill) | "sdpa", on an fp8 cache "hip-kv8" (gq_attn_prefill_kv8) |
    "sdpa-kv8" (SDPA on the dequantised rows).  mode = GQ_PREFILL_ATTN: "0" never the kernel, "1" the kernel wherever the library supports
    the geometry, "auto" the kernel inside a chunked pass (a prompt of one piece launches what it always did) -- and for any number of
    pieces on an fp8 cache"""
    if mode not in ("auto", "0", "1"):
        raise ValueError(f"GQ_PREFILL_ATTN={mode!r}: auto, 0 or 1")
    hip = mode != "0" and (mode == "1" or n_pieces > 1 or kv8) and supported
    return ("hip" if hip else "sdpa") + ("-kv8" if kv8 else "")


def score_head_choice(mode: str, served: bool, auto: str) -> bool:
    """True: the kernel gq_head_nll, False: the torch head.  mode = GQ_SCORE_HEAD: "1" / "0" as they say (an unserved shape then fails in
    the kernel's own check), "auto" the model's SCORE_HEAD_AUTO where the kernel serves the shape"""
    if mode not in ("auto", "0", "1"):
        raise ValueError(f"GQ_SCORE_HEAD={mode!r}: auto, 0 or 1")
    return mode == "1" or (mode == "auto" and served and auto == "1")


def ready(model, idx) -> bool:
    """`Transformer.prefill_ready`"""
    cfg = model.config
    return (model._native_kind() in ("ap", "qtip") and idx.is_cuda and idx.numel() > 1 and (idx.dim() == 1 or idx.shape[0] == 1)
            and cfg.head_dim % 16 == 0 and cfg.dim % 8 == 0 and cfg.dim <= 16384 and cfg.intermediate_size % 8 == 0)


# ------------------------------------------------------------------------------------------------ the pass
def prompt_pass(model, idx, input_pos, start: int, last_only: bool, chunk: Optional[int], score: Optional[dict] = None):
    """the chunk loop of `prefill_native` (score None: its logits) and of `score_native` (score = dict(targets int32 [S], kernel bool):
    every piece runs the scoring head on its rows; the list of the pieces' (logprob, top1))"""
    L = _lib.lib()
    cfg = model.config
    S, H, Hkv, hd = idx.numel(), cfg.n_head, cfg.n_local_heads, cfg.head_dim
    assert model.prefill_ready(idx) and input_pos.numel() == S and input_pos.dtype == torch.int32 and start + S <= model.max_seq_length
    if chunk is None:
        chunk = int(os.environ.get("GQ_PREFILL_CHUNK", "4096"))
    assert chunk >= 1, chunk
    pieces = prefill_chunks(S, chunk, start)
    mode = os.environ.get("GQ_PREFILL_ATTN", "auto")
    kv8 = model.kv_cache_dtype == "fp8"
    plan = attention_plan(mode, len(pieces), kv8, True)  # (the plan where the library serves the geometry; a bad mode raises here)
    if kv8:
        assert model._native_kind() == "ap" and model.kv8_unserved() is None, model.kv8_unserved()
    needs_library = plan.startswith("hip")  # (mode and pieces want the kernel: only then does the library's answer decide, and is it asked)
    if needs_library and not L.gq_attn_prefill_supported(H, Hkv, hd):
        plan = attention_plan(mode, len(pieces), kv8, False)
    model.last_prefill_plan = dict(chunks=pieces, attn=[plan] * len(model.layers))
    dev = idx.device
    Sc = min(chunk, S)
    f16 = dict(dtype=torch.float16, device=dev)
    bufs = dict(xn=torch.empty((Sc, cfg.dim), **f16), q=torch.empty((H * Sc * hd, ), **f16), hbuf=torch.empty((Sc, cfg.intermediate_size), **f16),
                y=torch.empty((Sc, H * hd), **f16) if plan.startswith("hip") else None)
    flat, out = idx.reshape(-1), []
    for a, n in pieces:
        o = a - start
        head = (not last_only) or a + n == start + S
        piece_score = None if score is None else dict(score, targets=score["targets"][o:o + n])
        r = _run_piece(model, flat[o:o + n], input_pos[o:o + n], a, bufs, plan, head, last_only, piece_score)
        if head:
            out.append(r)
    if score is not None:
        return out
    return out[0] if len(out) == 1 else torch.cat(out, dim=1)


def _run_piece(model, idx, input_pos, start: int, bufs: dict, plan: str, head: bool, last_only: bool, score: Optional[dict]):
    """one piece of the prompt pass: S tokens at positions start .. start + S - 1 through every layer, attending the cache rows
    [0, start + S); the logits ([1, 1 | S, V]) when `head`, else None.  With `score` (the third head mode) the head is the scoring
    head on the piece's rows and targets: (logprob fp32 [S], top1 int [S])"""
    cfg = model.config
    S = idx.numel()
    x = model.tok_embeddings(idx.view(1, S)).view(S, cfg.dim).contiguous()
    pending = _Piece(model, input_pos, start, bufs, plan).layers(x)
    if not head:
        return None
    x = x + pending
    if score is not None:
        return score_head(model, x, score["targets"], score["kernel"])
    x = x[-1:] if last_only else x
    return model.output(model.norm(x)).view(1, -1, cfg.vocab_size)


class _Piece:
    """the buffers and positions of one piece, and its launches"""

    def __init__(self, model, input_pos, start: int, bufs: dict, plan: str):
        cfg = model.config
        self.m, self.pos, self.start, self.S, self.plan = model, input_pos, start, input_pos.numel(), plan
        S, H, hd = self.S, cfg.n_head, cfg.head_dim
        self.xn, self.hbuf = bufs["xn"][:S], bufs["hbuf"][:S]
        self.q = bufs["q"][:H * S * hd].view(H, S, hd)
        self.y = bufs["y"][:S] if plan.startswith("hip") else None  # (the kernel's output, already in the row layout wo reads)
        self.masks = {}

    def sdpa_mask(self, win):
        """the [S, T] rows SDPA needs, from the positions: none at start == 0 without a window (is_causal); a sliding-window layer whose
        window the T keys outgrow takes the explicit mask at start == 0 too (is_causal would attend them all)"""
        T = self.start + self.S
        if win is not None and T <= win:
            win = None
        if win is None and self.start == 0:
            return None
        if win not in self.masks:
            self.masks[win] = mask_rows(self.pos, T, win)[None, None]
        return self.masks[win]

    def rows_and_attention(self, att, qkv, win, st):
        """RoPE + KV-cache row write and the attention of one layer on its q | k | v rows `qkv` [S][(H + 2 Hkv) hd]: y [1, S, H hd].
        ONE row-write launch per cache layout and block layout -- gq_rope_cache_rows, gq_qknorm_rope_cache_rows (Qwen3: the per-head RMSNorm
        of q and k in front of the rotation) or, on an fp8 cache, gq_rope_cache_rows_kv8 (the norm weights ride along; a bias is already in
        the rows: the quantized linear added it) -- then the plan's attention over batch slot 0 of the caches"""
        m, cfg, L, kvc = self.m, self.m.config, _lib.lib(), att.kv_cache
        S, H, Hkv, hd = self.S, cfg.n_head, cfg.n_local_heads, cfg.head_dim
        kc, vc = kvc.k_cache, kvc.v_cache
        kv8 = self.plan.endswith("-kv8")
        rows = (qkv.data_ptr(), self.pos.data_ptr(), m.rope_cos.data_ptr(), m.rope_sin.data_ptr(), self.q.data_ptr(), kc.data_ptr(), vc.data_ptr())
        shape = (S, H, Hkv, hd, kc.shape[2])
        if kv8:
            entry, args = "gq_rope_cache_rows_kv8", (*rows, kvc.k_inv.data_ptr(), kvc.v_inv.data_ptr(), *shape, *native_step.qk_norm_args(att, cfg), None)
        elif cfg.qk_norm:
            entry, args = "gq_qknorm_rope_cache_rows", (*rows, *shape, *native_step.qk_norm_args(att, cfg))
        else:
            entry, args = "gq_rope_cache_rows", (*rows, *shape)
        _lib.check(getattr(L, entry)(*args, st), entry)
        if self.plan.startswith("hip"):
            entry, scales = ("gq_attn_prefill_kv8", (kvc.k_scale.data_ptr(), kvc.v_scale.data_ptr())) if kv8 else ("gq_attn_prefill", ())
            _lib.check(getattr(L, entry)(self.q.data_ptr(), kc.data_ptr(), vc.data_ptr(), *scales, self.y.data_ptr(), S, self.start, H, Hkv, hd, kc.shape[2],
                                         1.0 / math.sqrt(hd), 0 if win is None else int(win), st), entry)
            return self.y.view(1, S, H * hd)
        T = self.start + S
        k, v = kc[:1, :, :T], vc[:1, :, :T]
        if kv8:
            k, v = kvc.dequant(k, kvc.k_scale), kvc.dequant(v, kvc.v_scale)
        return _sdpa_gqa(self.q.unsqueeze(0), k, v, self.sdpa_mask(win), H // Hkv).transpose(1, 2).reshape(1, S, H * hd)

    def layers(self, x):
        """every layer on the residual rows x fp16 [S, D], per layer
            norm -> qkv -> rows + attention -> wo -> norm -> gate / up -> silu * up -> down.
        x is updated in place by the residual adds that ride in the RMSNorm launches; the last block's MLP output has none behind it and is
        returned.  The linears go through `APLinear.forward` (fused prefill GEMM / split K / the reference's two steps by size; one row: the
        GEMV) or, for QTIP models, `QuantizedLinear.forward` of the unfused q | k | v and gate | up, side by side."""
        m, cfg, L = self.m, self.m.config, _lib.lib()
        S, D, inter = self.S, cfg.dim, cfg.intermediate_size
        qt = m._native_kind() == "qtip"
        xn = self.xn.view(1, S, D)
        pending = None  # the previous block's MLP output: its residual add rides in the next RMSNorm launch
        with torch.cuda.device(x.device):
            st = _lib.current_stream_ptr()  # (the model's device's current stream: inside the guard)

            def norm(n, delta):
                _lib.check(L.gq_rmsnorm_rows(x.data_ptr(), native_step._ptr(delta), n.weight.data_ptr(), self.xn.data_ptr(), S, D, n.eps, st), "gq_rmsnorm_rows")
            for b, win in zip(m.layers, cfg.layer_windows or (None,) * len(m.layers)):
                att, ff = b.attention, b.feed_forward
                norm(b.input_layernorm, pending)
                qkv = torch.cat([att.wq(xn), att.wk(xn), att.wv(xn)], dim=-1) if qt else att.wqkv(xn)
                y = self.rows_and_attention(att, qkv.view(S, -1), win, st)
                norm(b.post_attention_layernorm, att.wo(y).view(S, D))
                gu = torch.cat([ff.w1(xn), ff.w3(xn)], dim=-1) if qt else ff.w1w3(xn)
                paired = 1 if not qt and getattr(ff.w1w3, "gq_row_pairs", False) else 0  # (QTIP: gate | up side by side)
                _lib.check(L.gq_silu_mul_rows(gu.view(S, 2 * inter).data_ptr(), self.hbuf.data_ptr(), S, inter, paired, st), "gq_silu_mul_rows")
                pending = ff.w2(self.hbuf.view(1, S, inter)).view(S, D)
        return pending


# ------------------------------------------------------------------------------------------------ scoring
def score_head(model, x, targets, kernel: bool):
    """`Transformer._score_head`: the kernel gq_head_nll, or the torch head in blocks of the model's SCORE_HEAD_ROWS rows"""
    n, V = x.shape[0], model.config.vocab_size
    if kernel:
        L = _lib.lib()
        xn = model.norm(x).contiguous()
        W = model.output.weight
        assert xn.dtype == torch.float16 and W.dtype == torch.float16 and W.is_contiguous() and targets.dtype == torch.int32 and targets.numel() == n
        lp = torch.empty(n, dtype=torch.float32, device=x.device)
        top1 = torch.empty(n, dtype=torch.int32, device=x.device)
        with torch.cuda.device(x.device):  # (the automatic split follows the compute units of the model's device: one guard for both calls)
            nws = int(L.gq_head_nll_ws_bytes(n, V, xn.shape[1], 0))
            ws = torch.empty(max(nws, 4), dtype=torch.uint8, device=x.device)
            _lib.check(L.gq_head_nll(xn.data_ptr(), W.data_ptr(), targets.data_ptr(), n, V, xn.shape[1], lp.data_ptr(), None, top1.data_ptr(), 0,
                                     ws.data_ptr(), nws, _lib.current_stream_ptr()), "gq_head_nll")
        return lp, top1
    lps, tops = [], []
    for a in range(0, n, model.SCORE_HEAD_ROWS):
        t = targets[a:a + model.SCORE_HEAD_ROWS].long()
        ls = F.log_softmax(model.output(model.norm(x[a:a + model.SCORE_HEAD_ROWS])).float(), dim=-1)
        lp = ls.gather(1, t.clamp(min=0)[:, None])[:, 0]
        lps.append(torch.where(t >= 0, lp, torch.zeros_like(lp)))
        tops.append(ls.argmax(dim=-1).to(torch.int32))
    return torch.cat(lps), torch.cat(tops)


def score(model, idx, chunk: Optional[int] = None):
    """`Transformer.score_native`: the pass from position 0 with the scoring head on every piece"""
    flat = idx.reshape(-1)
    S = flat.numel()
    assert model.prefill_ready(idx) and 2 <= S <= model.max_seq_length
    served = model.config.dim % 64 == 0 and model.output.weight.dtype == torch.float16  # (else the kernel answers GQ_ENOTSUP)
    kernel = score_head_choice(os.environ.get("GQ_SCORE_HEAD", "auto"), served, model.SCORE_HEAD_AUTO)
    flat = flat.to(torch.int32)
    targets = torch.cat([flat[1:], torch.full((1, ), -1, dtype=torch.int32, device=flat.device)])
    pos = torch.arange(0, S, device=flat.device, dtype=torch.int32)
    out = prompt_pass(model, flat, pos, 0, False, chunk, score=dict(targets=targets, kernel=kernel))
    model.last_prefill_plan["head"] = "hip-nll" if kernel else "torch"
    lp = torch.cat([o[0] for o in out])[:S - 1]
    top1 = torch.cat([o[1] for o in out])[:S - 1]
    return lp, top1 == flat[1:]


# ------------------------------------------------------------------------------------------------ packed scoring
def pack_capacity(model) -> int:
    """the rows of a pack where the caller names none: a chunk of the prompt pass, within the model's context"""
    return min(int(os.environ.get("GQ_PREFILL_CHUNK", "4096")), int(model.config.block_size))


def pack_plan(lengths, capacity: int):
    """Groups the sequences 0 .. n - 1 of the given lengths into packs of at most `capacity` rows: first fit in input order -- a sequence
    goes into the first pack it still fits into, else it opens a new pack -- so the same lengths always give the same packs, the indices
    ascend inside a pack and the packs are ordered by their first index.  A sequence longer than `capacity` is a pack of its own (the
    caller scores it through the one-sequence pass).  Pure host logic."""
    capacity = int(capacity)
    if capacity < 1:
        raise ValueError(f"pack_plan: capacity {capacity}")
    packs, room = [], []
    for i, n in enumerate(lengths):
        n = int(n)
        if n < 1:
            raise ValueError(f"pack_plan: sequence {i} has length {n}")
        for j, r in enumerate(room):
            if n <= r:
                packs[j].append(i)
                room[j] -= n
                break
        else:
            packs.append([i])
            room.append(capacity - n if n <= capacity else 0)
    return packs


def packed_mask(seg_begin: Tensor, window: Optional[int] = None) -> Tensor:
    """bool [S, S]: packed row i attends row t when max(seg_begin[i], i + 1 - window) <= t <= i -- the causal (and window) masks of the
    sequences, block-diagonal"""
    S = seg_begin.numel()
    i = torch.arange(S, device=seg_begin.device)[:, None]
    t = torch.arange(S, device=seg_begin.device)[None, :]
    m = (t <= i) & (t >= seg_begin.long()[:, None])
    return m if window is None else m & (t > i - int(window))


class _PackedPiece(_Piece):
    """a pack as one piece: the position of a row inside its sequence apart from its cache row, and a segment begin per row"""

    def __init__(self, model, pos, row, seg_begin, bufs: dict, plan: str):
        super().__init__(model, pos, 0, bufs, plan)
        self.row, self.seg_begin = row, seg_begin

    def rows_and_attention(self, att, qkv, win, st):
        """gq_rope_cache_rows_packed (the rotation by the position inside the sequence, k / v to the packed row), then
        gq_attn_prefill_packed or SDPA under the block-diagonal mask over the cache rows [0, S)"""
        m, cfg, L, kvc = self.m, self.m.config, _lib.lib(), att.kv_cache
        S, H, Hkv, hd = self.S, cfg.n_head, cfg.n_local_heads, cfg.head_dim
        kc, vc = kvc.k_cache, kvc.v_cache
        norm = native_step.qk_norm_args(att, cfg)  # (null weights: the plain form)
        _lib.check(L.gq_rope_cache_rows_packed(qkv.data_ptr(), self.pos.data_ptr(), self.row.data_ptr(), m.rope_cos.data_ptr(), m.rope_sin.data_ptr(),
                                               self.q.data_ptr(), kc.data_ptr(), vc.data_ptr(), S, H, Hkv, hd, kc.shape[2], *norm, st), "gq_rope_cache_rows_packed")
        if self.plan.startswith("hip"):
            _lib.check(L.gq_attn_prefill_packed(self.q.data_ptr(), kc.data_ptr(), vc.data_ptr(), self.seg_begin.data_ptr(), self.y.data_ptr(), S, H, Hkv, hd,
                                                kc.shape[2], 1.0 / math.sqrt(hd), 0 if win is None else int(win), st), "gq_attn_prefill_packed")
            return self.y.view(1, S, H * hd)
        if win is not None and win >= S:
            win = None
        if win not in self.masks:
            self.masks[win] = packed_mask(self.seg_begin, win)[None, None]
        return _sdpa_gqa(self.q.unsqueeze(0), kc[:1, :, :S], vc[:1, :, :S], self.masks[win], H // Hkv).transpose(1, 2).reshape(1, S, H * hd)


def score_packed(model, seqs, rows: Optional[Tensor] = None):
    """`Transformer.score_packed_native`: the sequences `seqs` (1-D int tensors on the model's device, two tokens or more each) as ONE
    piece of S = sum of their lengths rows -- never chunked -- with the scoring head on the rows `rows` (bool [S]; None: every row).
    Returns (logprob fp32 [k], hit bool [k]) over the head's rows in packed order: logprob of the next token of the row's own sequence
    and whether it is the most probable one; a sequence's last row has no next token (logprob 0, hit False)."""
    if model.kv_cache_dtype == "fp8":
        raise NotImplementedError("packed scoring: fp8 KV cache")
    cfg = model.config
    lens = [int(s.numel()) for s in seqs]
    if not lens or min(lens) < 2:
        raise ValueError("packed scoring: at least one sequence, two tokens or more each")
    flat = torch.cat([s.reshape(-1) for s in seqs]).to(torch.int32)
    S, dev = int(flat.numel()), flat.device
    if model.max_seq_length < S:
        model.setup_caches(max(1, model.max_batch_size), S, kv_cache_dtype=model.kv_cache_dtype)
    assert model.prefill_ready(flat) and max(lens) <= model.max_seq_length
    H, Hkv, hd = cfg.n_head, cfg.n_local_heads, cfg.head_dim
    mode = os.environ.get("GQ_PREFILL_ATTN", "auto")
    attention_plan(mode, 1, False, True)  # (a bad mode raises here)
    plan = "hip-packed" if mode != "0" and _lib.lib().gq_attn_prefill_supported(H, Hkv, hd) else "sdpa-packed"
    served = cfg.dim % 64 == 0 and model.output.weight.dtype == torch.float16
    kernel = score_head_choice(os.environ.get("GQ_SCORE_HEAD", "auto"), served, model.SCORE_HEAD_AUTO)
    begins = [0]
    for n in lens[:-1]:
        begins.append(begins[-1] + n)
    lens_t = torch.tensor(lens, device=dev)
    seg_begin = torch.repeat_interleave(torch.tensor(begins, dtype=torch.int32, device=dev), lens_t)
    row = torch.arange(S, dtype=torch.int32, device=dev)
    pos = row - seg_begin
    targets = torch.cat([flat[1:], torch.full((1, ), -1, dtype=torch.int32, device=dev)])
    targets[torch.tensor([b + n - 1 for b, n in zip(begins, lens)], device=dev)] = -1
    f16 = dict(dtype=torch.float16, device=dev)
    bufs = dict(xn=torch.empty((S, cfg.dim), **f16), q=torch.empty((H * S * hd, ), **f16), hbuf=torch.empty((S, cfg.intermediate_size), **f16),
                y=torch.empty((S, H * hd), **f16) if plan.startswith("hip") else None)
    x = model.tok_embeddings(flat.view(1, S)).view(S, cfg.dim).contiguous()
    pending = _PackedPiece(model, pos, row, seg_begin, bufs, plan).layers(x)
    if rows is None:
        x = x + pending
    else:
        assert rows.dtype == torch.bool and rows.numel() == S
        sel = torch.nonzero(rows.to(dev)).reshape(-1)
        x, targets = x[sel] + pending[sel], targets[sel].contiguous()
    k = int(x.shape[0])
    model.last_prefill_plan = dict(chunks=[(0, S)], attn=[plan] * len(model.layers), head="hip-nll" if kernel else "torch",
                                   packed=dict(sequences=len(lens), rows=S, head_rows=k))
    if k == 0:
        return torch.empty(0, dtype=torch.float32, device=dev), torch.empty(0, dtype=torch.bool, device=dev)
    lp, top1 = score_head(model, x, targets, kernel)
    return lp, top1 == targets
