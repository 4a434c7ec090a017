"""The fused HIP decode step: the host side of `Transformer.decode_native` -- one bs=1 token through the C ABI (include/gq_hip.h).

  * `StepState`: what both families share -- the per-model buffers, the split of the attention over the cache, the embedding and lm_head
    launches and THE attention launch (`attend`: one argument list for its four entry points).
  * `ApStep`: fused-linear Any-Precision models, 5 launches per layer (RMSNorm -> wqkv | RoPE + KV update + attention | wo + residual |
    RMSNorm -> w1w3 | SiLU*up -> w2 + residual).
  * `QtipStep`: unfused QTIP models -- launch plans built once (`_QtipPlanner`), launches as named records (one namedtuple per entry
    point, fields = the C prototype's parameters), and the loop that runs them.

`Transformer` keeps `_native_state()`, `native_embed / _layers / _head` and `_handover_plan` as delegations to this module; the states
answer `state["x"]` as well as `state.x` for the callers that subscript (bench.py, generate.py, the tests).  What a step launches, in
which order, with which arguments, is pinned by tests/golden/decode_calls.json.
"""
import ctypes
import math
import os
from collections import namedtuple
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib


# ------------------------------------------------------------------------------------------------ knobs
# Every environment knob of the step, with its measured verdict.  Read when a state is built or a step is issued, never at import: the
# tests flip them between models in one process.
def _knob(name, default):
    return lambda: os.environ.get(name, default) != "0"


native_qtip = _knob("GQ_NATIVE_QTIP", "1")      # 0: unfused QTIP models take the module-by-module forward
attn_gqa = _knob("GQ_ATTN_GQA", "1")            # the query heads of a KV group share an attention block where the wqkv launch rotates
native_pairs = _knob("GQ_NATIVE_PAIRS", "1")    # gate / up rows paired in place: w1w3 writes silu(gate) * up itself
# OFF by default: measured on the 8B decode it LOSES 1.4 % (855 vs 867 tokens/s, profiles/r05_handover.txt), see handover_plan
ssq_handover = _knob("GQ_SSQ_HANDOVER", "0")
qtip_ksplit = _knob("GQ_QTIP_KSPLIT", "1")      # K ranges per band (wo, down: 128 bands on 256 units -> 2)
qtip_ksplit_group = _knob("GQ_QTIP_KSPLIT_GROUP", "1")  # the same for linears that share a launch (q / k / v)
# Folding (default OFF): the transform-out of wo (+ residual) is rebuilt by the gate / up launch, that of down (+ residual) by the NEXT
# layer's q / k / v launch (gq_qtip_linear_in with n_prev = 1; bit-identical, the vector is stored once for the residual stream): two
# launches per layer less, but every one of the 256 blocks repeats the 4096-point transform and takes the slower prologue path --
# measured 365 vs 385 tokens/s on the Llama-2-7b shape (400 vs 422 with a power-of-two MLP), so it stays off.  Needs power-of-two
# widths on both sides of the fold.
qtip_fold = _knob("GQ_QTIP_FOLD", "0")
# (default OFF): transform-out inside the matvec launch (gq_qtip_linear, see _QtipPlanner.group).  Bit-identical, three launches per
# layer less -- and measured 302 vs 384 tokens/s on the Llama-2-7b shape: the device-scope release / acquire fences around the
# per-linear counter (L2 write-back + invalidate on 8 XCDs) cost ~7 us per launch, more than the launch they save.
qtip_one_launch = _knob("GQ_QTIP_ONE_LAUNCH", "0")
qtip_out_seg = _knob("GQ_QTIP_OUT_SEG", "1")    # M / 128 blocks per linear instead of one (equal up to fp32 rounding): 2.9 vs 4.6 us
# (default ON): a factor MLP width n = Kf * 64 (Llama-2-7b: 172 * 64) -- the two gq_qtip_transform launches between the matvecs of
# gate / up and down (output side, then input side with silu * up) become ONE launch that works column by column (gq_qtip_mlp_mid),
# the 64-point row transforms of the input side move into the prologue of down's matvec launch (gq_qtip_linear_in_rows).  gate / up
# bit-identical, the input of down equal up to fp32 rounding.
qtip_mlp_mid = _knob("GQ_QTIP_MLP_MID", "1")
# (default ON): the transform-out of q / k / v runs inside the attention launch -- every head block needs head_dim of the outputs: the
# segments combined with the signs of its row, then one head_dim-point transform (equal to gq_qtip_linear_out up to fp32 rounding) --:
# one launch (4.8 us) per layer less.  Needs power-of-two q / k / v widths.  (gq_attn_decode_qtip serves n_head * head_dim <= 8192, a
# power of two; wider models keep gq_qtip_linear_out + attention)
qtip_attn_fold = _knob("GQ_QTIP_ATTN_FOLD", "1")
# Round 5 (default OFF -- measured 421 vs 427 tokens/s on Llama-2-7b, profiles/r05_qtip_pre.txt: the one-block launch grows by more
# than the 256-block launch shrinks, whose prologue ran under its first tile requests anyway): the transform-out launch of wo / down
# ALSO runs the transform-in of the linears that read its output through an RMSNorm -- gate / up, the next layer's q / k / v -- one
# block per consumer (gq_qtip_linear_out_in), and their matvec launch takes the pre-transformed vectors as they are: its 256 blocks no
# longer repeat RMSNorm . SU . Hadamard.  Needs power-of-two widths on that edge and the plain launch forms (no folding, no one-launch
# form).
qtip_pre = _knob("GQ_QTIP_PRE", "0")


def attn_split_knob(planned):
    return int(os.environ.get("GQ_ATTN_SPLIT", planned))  # the planned number of cache splits, overridden


def _ptr(t):
    return t.data_ptr() if t is not None else None


def qk_norm_args(at, c):
    """(q_norm weight, k_norm weight, eps) of an attention module for the launches that take a QK-norm form by argument (null weights:
    the plain form): gq_rope_cache_rows_kv8 of the decode step and the prompt pass, gq_qknorm_rope_cache_rows"""
    return (at.q_norm.weight.data_ptr(), at.k_norm.weight.data_ptr(), at.q_norm.eps) if c.qk_norm else (None, None, 0.0)


def kv_slot_bytes(n_kv_head, max_seq, head_dim, elem_size):
    """bytes of one batch slot of a K (or V) cache [batch][n_kv_head][max_seq][head_dim]: elem_size 2 (fp16) or 1 (fp8)"""
    return n_kv_head * max_seq * head_dim * elem_size


class _Keyed:
    """state["x"] for state.x"""

    def __getitem__(self, key):
        try:
            return getattr(self, key)
        except AttributeError:
            raise KeyError(key) from None


# ------------------------------------------------------------------------------------------------ what both families share
class StepState(_Keyed):
    pairs = False  # gate / up rows paired (ApStep)
    ap_ws = None   # workspace of the down projection (ApStep)

    def __init__(self, model):
        self.m = model
        dev = model.output.weight.device
        c = model.config
        f16 = dict(dtype=torch.float16, device=dev)
        self.x, self.h, self.y = torch.zeros(c.dim, **f16), torch.zeros(c.dim, **f16), torch.zeros(c.n_head * c.head_dim, **f16)
        self.qkv = torch.zeros((c.n_head + 2 * c.n_local_heads) * c.head_dim, **f16)
        self.ssq = torch.zeros(_lib.SSQ_SLOTS, dtype=torch.float32, device=dev)  # statistics hand-over slots (gq_hip.h GQ_SSQ_SLOTS)
        # one flag line per query head for the attention heads that run inside the wqkv launch (gq_anyprec_gemv_qkv_rope_attn:
        # zero between launches; one buffer for all layers)
        self.attn_flags = torch.zeros(c.n_head * _lib.ATTN_FLAG_STRIDE, dtype=torch.int32, device=dev)
        self.gu, self.logits = torch.zeros(2 * c.intermediate_size, **f16), torch.zeros(1, 1, c.vocab_size, **f16)
        # long caches: split-KV attention (gq_attn_decode_split), n_split blocks per head + a combine launch; a context of
        # up to 256 positions is still finished by one block per head at run time
        S = model.max_seq_length
        l0 = model.layers[0].attention

        def plan(S):
            ns = 1 if S <= 1024 else (4 if S <= 2048 else 8)
            # grouped-query models whose wqkv launch rotates q / k (gq_attn_decode_roped): the four query heads of a KV group share a
            # block, so the splits can be as short as one 128-position pass -- n_kv_head x n_split blocks ~ one per CU
            # (not for QK-norm or attn_bias models: their wqkv launch never rotates, see ApStep.layers)
            if (S > 1024 and c.n_head % (4 * c.n_local_heads) == 0 and model._native_kind() != "qtip" and attn_gqa()
                    and not c.qk_norm and not c.attn_bias and _lib.lib().gq_anyprec_qkv_rope_supported(l0.wqkv.out_features, c.dim, l0.wqkv.bitwidth, c.head_dim)):
                ns = max(4, min(32, (S + 127) // 128, 256 // max(1, c.n_head // 4)))
            return attn_split_knob(ns)

        self.attn_split = plan(S)
        # sliding-window layers (ModelArgs.layer_windows): a layer whose window is shorter than the cache attends the rows
        # (pos - W, pos] through the _window entry of its form; it never reads more than W rows, so its splits are planned from
        # min(S, W) by the same rule.  Layers without a window (or with one the cache never outgrows) launch what they always did.
        lw = getattr(c, "layer_windows", None) or (None,) * len(model.layers)
        assert len(lw) == len(model.layers), "ModelArgs.layer_windows: one entry per layer"
        self.layer_window = [int(w) if w is not None and int(w) < S else None for w in lw]
        assert all(w is None or w >= 1 for w in self.layer_window), "ModelArgs.layer_windows: a window is at least 1"
        self.layer_split = [self.attn_split if w is None else plan(w) for w in self.layer_window]
        ns_max = max([self.attn_split] + self.layer_split)  # (one workspace, sized for the largest)
        self.attn_ws = torch.zeros(c.n_head * ns_max * (c.head_dim + 2), dtype=torch.float32, device=dev) if ns_max > 1 else None
        # an fp8 KV cache (Transformer.setup_caches(.., kv_cache_dtype="fp8")): the rotated q of attend_kv8
        self.kv8 = getattr(model, "kv_cache_dtype", "fp16") == "fp8"
        self.q8 = torch.zeros(c.n_head * c.head_dim, **f16) if self.kv8 else None

    def kv(self, at, slot):
        """the K / V cache of batch slot `slot` of one attention module"""
        c = self.m.config
        off = slot * kv_slot_bytes(c.n_local_heads, self.m.max_seq_length, c.head_dim, at.kv_cache.k_cache.element_size())
        return at.kv_cache.k_cache.data_ptr() + off, at.kv_cache.v_cache.data_ptr() + off

    def attend(self, entry, src, pos, kv, sp, extra=(), layer=None):
        """the attention launch, entry = gq_attn_decode_split / _split_qknorm / _split_bias / _roped / _qtip.  src: the packed q | k | v vector (or
        the q / k / v descriptors of gq_attn_decode_qtip); _roped takes no tables (the wqkv launch rotated); extra: what an entry
        point takes behind the workspace.  layer: its index -- a sliding-window layer takes the `_window` entry of the form, with its own
        split count and the window behind `extra`"""
        m, c = self.m, self.m.config
        rope = () if entry == "gq_attn_decode_roped" else (m.rope_cos.data_ptr(), m.rope_sin.data_ptr())
        win, ns = (None, self.attn_split) if layer is None else (self.layer_window[layer], self.layer_split[layer])
        if win is not None:
            assert entry != "gq_attn_decode_qtip", "QTIP models have no sliding-window form"
            entry, extra = entry + "_window", (*extra, win)
        _lib.check(getattr(_lib.lib(), entry)(src, pos.data_ptr(), *rope, *kv, self.y.data_ptr(), c.n_head, c.n_local_heads, c.head_dim,
                                              m.max_seq_length, 1.0 / math.sqrt(c.head_dim), ns, _ptr(self.attn_ws), *extra, sp), entry)

    def attend_kv8(self, at, pos, kv, sp, layer):
        """the fp8 cache's route of one layer, behind the plain wqkv GEMV: gq_rope_cache_rows_kv8 (S = 1, the graph's position word; the
        layer's norm weights or bias) rotates q into its own buffer and writes the cache row, gq_attn_decode_roped_kv8 attends it with the
        layer's window and split plan.  One route for Llama, Mistral, Qwen2 and Qwen3; one launch per layer more than the fp16 routes."""
        m, c, L, kvc = self.m, self.m.config, _lib.lib(), at.kv_cache
        _lib.check(L.gq_rope_cache_rows_kv8(self.qkv.data_ptr(), pos.data_ptr(), m.rope_cos.data_ptr(), m.rope_sin.data_ptr(), self.q8.data_ptr(), *kv,
                                            kvc.k_inv.data_ptr(), kvc.v_inv.data_ptr(), 1, c.n_head, c.n_local_heads, c.head_dim, m.max_seq_length, *qk_norm_args(at, c),
                                            _ptr(at.wqkv.bias), sp), "gq_rope_cache_rows_kv8")
        _lib.check(L.gq_attn_decode_roped_kv8(self.q8.data_ptr(), pos.data_ptr(), *kv, kvc.k_scale.data_ptr(), kvc.v_scale.data_ptr(), self.y.data_ptr(),
                                              c.n_head, c.n_local_heads, c.head_dim, m.max_seq_length, 1.0 / math.sqrt(c.head_dim),
                                              self.layer_split[layer], _ptr(self.attn_ws), self.layer_window[layer] or 0, sp), "gq_attn_decode_roped_kv8")

    def head(self, x):
        """the one call site of the dense GEMV (both families): final RMSNorm + lm_head -> the fp16 logits.  An int8-head model
        (Transformer.set_lm_head_dtype) launches gq_dense_gemv_i8 over its int8 copy, every other model what it always launched."""
        m, c = self.m, self.m.config
        if getattr(m, "lm_head_dtype", "fp16") == "int8":
            q, scale = m.head_q8()
            _lib.check(_lib.lib().gq_dense_gemv_i8(x.data_ptr(), q.data_ptr(), scale.data_ptr(), self.logits.data_ptr(), c.vocab_size,
                                                   c.dim, m.norm.weight.data_ptr(), c.norm_eps, _lib.current_stream_ptr()), "lm_head (int8)")
            return self.logits
        _lib.check(_lib.lib().gq_dense_gemv_f16(x.data_ptr(), m.output.weight.data_ptr(), self.logits.data_ptr(), c.vocab_size,
                                                c.dim, m.norm.weight.data_ptr(), c.norm_eps, _lib.current_stream_ptr()), "lm_head")
        return self.logits


def embed(model, tok, x, ssq=None):
    """x = tok_embeddings[tok]; with `ssq` (the hand-over slots of the state) also the statistics of x for layer 0's RMSNorm"""
    _lib.check(_lib.lib().gq_embed_lookup_ho(tok.data_ptr(), model.tok_embeddings.weight.data_ptr(), x.data_ptr(), model.config.dim,
                                             model.config.vocab_size, _ptr(ssq), _lib.current_stream_ptr()), "gq_embed_lookup")


# ------------------------------------------------------------------------------------------------ Any-Precision
def handover_plan(model, blk):
    """Statistics hand-over (include/gq_hip.h, round 5) on the two RMSNorm edges of a layer -- (w2 or the embedding) -> wqkv and
    wo -> w1w3: the producer's residual epilogue leaves the partial sums of squares of the hidden state it writes, the consumer's
    RMSNorm prologue adds them instead of exchanging per-wave sums.  An edge is used only when BOTH ends have the form (the plan is
    the library's own dispatch run dry): 8B-class 2-bit models.  OFF by default (GQ_SSQ_HANDOVER=1 turns it on): measured on the
    8B decode it LOSES 1.4 % (855 vs 867 tokens/s, profiles/r05_handover.txt) -- the partial sums come out of memory no earlier
    than the activations themselves, the wave that adds them holds the launch barrier ~700 cycles, and the producers pay 0.1 us."""
    # (not cached: the answer follows gq_set_ap_mode / the environment like the dispatch itself; 4 host calls per layer, paid by
    # eager steps and graph captures only)
    if not ssq_handover():
        return dict(qkv_in=False, w13=False, w2_out=False)
    plan = _lib.lib().gq_anyprec_handover_plan
    c, at, ff = model.config, blk.attention, blk.feed_forward
    qkv_in = bool(plan(at.wqkv.out_features, c.dim, at.wqkv.bitwidth, 1, 0) & 1)
    w13_in = bool(plan(2 * c.intermediate_size, c.dim, ff.w1w3.bitwidth, 1, 4) & 1)
    wo_out = bool(plan(c.dim, c.n_head * c.head_dim, at.wo.bitwidth, 0, 1) & 2)
    w2_out = bool(plan(c.dim, c.intermediate_size, ff.w2.bitwidth, 0, 1) & 2)
    return dict(qkv_in=qkv_in, w13=w13_in and wo_out, w2_out=w2_out)


def _lin(m):
    """the weight arguments of an AP-GEMV entry point: qweight, lut, N, K, bits"""
    return m.qweight.data_ptr(), m.lut.data_ptr(), m.out_features, m.in_features, m.bitwidth


class ApStep(StepState):

    def __init__(self, model):
        from .model import pair_gate_up_rows_
        super().__init__(model)
        c = model.config
        if self.kv8 and model.kv8_unserved():
            raise ValueError("fp8 KV cache: " + model.kv8_unserved())
        # workspace of the down projection where the library splits its rows along K over blocks (K > 16384: 70B)
        wb = max(int(_lib.lib().gq_anyprec_gemv_fused_ws_bytes(c.dim, c.intermediate_size, b.feed_forward.w2.bitwidth, 1)) for b in model.layers)
        if wb:
            self.ap_ws = torch.zeros(wb // 4, dtype=torch.float32, device=self.x.device)
        # Gate/up pairing (GQ_EPI_SILU_PAIRS): every fused w1w3 tensor is re-ordered in place to (gate_0, up_0, gate_1,
        # up_1, ..) rows so that the w1w3 GEMV writes silu(gate) * up directly (model.py:266 of the reference) and w2
        # reads a plain vector; state_dict() still exports the reference layout (pair_gate_up_rows_).
        if native_pairs():
            for b in model.layers:
                pair_gate_up_rows_(b.feed_forward.w1w3)
            self.pairs = True
        else:
            assert not any(getattr(b.feed_forward.w1w3, "gq_row_pairs", False) for b in model.layers), \
                "GQ_NATIVE_PAIRS=0 on a model whose gate/up rows were already paired"

    def layers(self, x, pos, l0, l1, slot=0, ssq_ready=False):
        from .model import pair_gate_up_rows_
        m, c, L = self.m, self.m.config, _lib.lib()
        sp = _lib.current_stream_ptr()
        if self.pairs:  # a load_state_dict into a sub-module bypasses _reset_native: the rows must still be paired at launch
            for blk in m.layers[l0:l1]:
                if not getattr(blk.feed_forward.w1w3, "gq_row_pairs", False):
                    pair_gate_up_rows_(blk.feed_forward.w1w3)
                    m._alloc_gen = getattr(m, "_alloc_gen", 0) + 1  # (the re-pair assigned new tensors)

        def launch(entry, *args):
            _lib.check(getattr(L, entry)(*args, sp), entry)

        h, y, qkv, gu = self.h.data_ptr(), self.y.data_ptr(), self.qkv.data_ptr(), self.gu.data_ptr()
        xp, ssq = x.data_ptr(), self.ssq.data_ptr()
        ws = (self.ap_ws.data_ptr(), self.ap_ws.numel() * 4) if self.ap_ws is not None else (None, 0)
        x_has_ssq = ssq_ready  # the slots hold the statistics of the current x
        for li, blk in enumerate(m.layers[l0:l1]):
            at, ff = blk.attention, blk.feed_forward
            kv = self.kv(at, slot)
            ho = handover_plan(m, blk)
            nxt = m.layers[l0 + li + 1] if l0 + li + 1 < len(m.layers) else None
            # (w2 writes the statistics only when the NEXT layer's wqkv reads them: the last layer feeds the lm_head's own norm)
            w2_ssq = ssq if (self.pairs and ho["w2_out"] and nxt is not None and l0 + li + 1 < l1 and handover_plan(m, nxt)["qkv_in"]) else None
            ssq_in = ssq if (x_has_ssq and ho["qkv_in"]) else None
            # what every wqkv form starts with, and what the forms that rotate and write the cache row add
            wqkv = (xp, qkv, *_lin(at.wqkv), blk.input_layernorm.weight.data_ptr(), c.norm_eps)
            rope = (pos.data_ptr(), m.rope_cos.data_ptr(), m.rope_sin.data_ptr(), *kv, c.n_head, c.n_local_heads, c.head_dim, m.max_seq_length)
            # RoPE + KV-cache write in the epilogue of the wqkv GEMV, attention without them, where the library serves the layer's
            # wqkv that way (fast mode, 2-bit, K <= 4096: csrc/ap_stream.hip); else the two launches of rounds 1-3
            if self.kv8:
                launch("gq_anyprec_gemv_fused_ho", *wqkv, None, 0, None, 0, ssq_in, None)
                self.attend_kv8(at, pos, kv, sp, l0 + li)
            elif c.qk_norm:
                # Qwen3: q and k are normalised per head BEFORE the rotation, so the wqkv launch must not rotate (its RoPE epilogue holds a
                # head's rows in eight 16-row groups: no per-head statistic there) -- plain wqkv GEMV, then ONE attention launch that
                # normalises, rotates, writes the cache row and attends
                launch("gq_anyprec_gemv_fused_ho", *wqkv, None, 0, None, 0, ssq_in, None)
                self.attend("gq_attn_decode_split_qknorm", qkv, pos, kv, sp, qk_norm_args(at, c), layer=l0 + li)
            elif at.wqkv.bias is not None:
                # Qwen2 / Qwen2.5: the bias of q / k / v belongs in front of the rotation, and the RoPE epilogues of the wqkv launch
                # (gq_anyprec_gemv_qkv_rope*) rotate what the GEMV summed -- the unbiased q / k.  Plain wqkv GEMV, then ONE attention launch
                # that adds the bias, rotates, writes the cache row and attends (_native_kind admits a bias here only on attn_bias models)
                launch("gq_anyprec_gemv_fused_ho", *wqkv, None, 0, None, 0, ssq_in, None)
                self.attend("gq_attn_decode_split_bias", qkv, pos, kv, sp, (at.wqkv.bias.data_ptr(),), layer=l0 + li)
            elif (self.attn_split == 1 and ssq_in is None and self.layer_window[l0 + li] is None  # (no window form inside the wqkv launch)
                    and L.gq_anyprec_qkv_rope_attn_supported(at.wqkv.out_features, c.dim, at.wqkv.bitwidth, c.head_dim, c.n_head, c.n_local_heads)):
                # round 6: the attention heads as extra blocks of the wqkv launch (they wait on device flags for q / the new cache row):
                # one launch and one kernel boundary less per layer, outputs bit-identical to the two launches below
                launch("gq_anyprec_gemv_qkv_rope_attn", *wqkv, *rope, y, 1.0 / math.sqrt(c.head_dim), self.attn_flags.data_ptr())
            elif L.gq_anyprec_qkv_rope_supported(at.wqkv.out_features, c.dim, at.wqkv.bitwidth, c.head_dim):
                launch("gq_anyprec_gemv_qkv_rope_ho", *wqkv, *rope, ssq_in)
                self.attend("gq_attn_decode_roped", qkv, pos, kv, sp, layer=l0 + li)
            else:
                launch("gq_anyprec_gemv_fused", *wqkv, None, 0)
                self.attend("gq_attn_decode_split", qkv, pos, kv, sp, layer=l0 + li)
            # x, out, weights, norm weight, eps, residual (wo's input width is n_head * head_dim: not dim for a model with a head_dim of its own)
            wo = (y, h, *_lin(at.wo), None, 0.0, xp)
            w13 = (h, gu, *_lin(ff.w1w3), blk.post_attention_layernorm.weight.data_ptr(), c.norm_eps, None)
            w2 = (gu, xp, *_lin(ff.w2), None, 0.0, h)
            if self.pairs:  # flags, workspace, its bytes, statistics in, statistics out
                w13_ssq = ssq if ho["w13"] else None
                launch("gq_anyprec_gemv_fused_ho", *wo, 1, None, 0, None, w13_ssq)
                launch("gq_anyprec_gemv_fused_ho", *w13, 4, None, 0, w13_ssq, None)
                launch("gq_anyprec_gemv_fused_ho", *w2, 1, *ws, None, w2_ssq)
            else:
                launch("gq_anyprec_gemv_fused", *wo, 1)
                launch("gq_anyprec_gemv_fused", *w13, 0)
                launch("gq_anyprec_gemv_fused", *w2, 1 | 2)
            x_has_ssq = w2_ssq is not None


# ------------------------------------------------------------------------------------------------ QTIP: launches as records
def _record(entry, fields):
    """the argument record of one C entry point (fields: the prototype's parameter names, include/gq_hip.h, without the stream)"""
    rec = namedtuple(entry, fields)
    rec.entry = entry
    return rec


LinearIn = _record("gq_qtip_linear_in", "x x2 norm_weight eps prologue K R n lin n_prev prev ksplit")
Linear = _record("gq_qtip_linear", "x x2 norm_weight eps prologue K R n lin finish ksplit counters")
LinearOut = _record("gq_qtip_linear_out", "n lin")  # (and gq_qtip_linear_out_seg)
LinearOutIn = _record("gq_qtip_linear_out_in", "prev norm_weight eps n_next SU_next xt_next")
Transform = _record("gq_qtip_transform", "input_side x x2 norm_weight eps prologue n_lin lin n Kf transpose")
MlpMid = _record("gq_qtip_mlp_mid", "m parts n Kf")
LinearInRows = _record("gq_qtip_linear_in_rows", "z32 K P R n lin ksplit")


def _launch(rec, entry=None):
    """a plan entry: (entry point name, its arguments)"""
    return (entry or rec.entry, rec)


OUT_ENTRIES = ("gq_qtip_linear_out", "gq_qtip_linear_out_seg")


@dataclass
class QtipLayer(_Keyed):
    """the launch plans of one layer: lists of (entry point name, record)"""
    qkv: list
    qkv_f: Optional[list]    # q / k / v with the previous layer's down folded in (GQ_QTIP_FOLD)
    attn_qt: object          # the q / k / v transform-out descriptors the attention launch rebuilds, or None
    o: list
    gu: list
    d: list
    d_out: Optional[list]    # the transform-out of down, when it is left to the next layer's q / k / v launch
    d_pre: Optional[list] = None    # down / the next layer's q / k / v in the GQ_QTIP_PRE form
    qkv_pre: Optional[list] = None


class _Copies:
    """fp32 / fp16 device copies the plans point into, and every descriptor array (kept alive with the state)"""

    def __init__(self, dev):
        self.dev, self.keep = dev, []
        self.tables = {}  # one device copy per distinct Hadamard factor table (every layer's module holds its own buffer)

    def hold(self, obj):
        self.keep.append(obj)
        return obj

    def f32(self, t, mul=1.0):
        return self.hold((t.detach().to(self.dev).float() * mul).contiguous()).data_ptr()

    def table(self, t):
        key = (tuple(t.shape), hash(t.detach().float().cpu().numpy().tobytes()))
        if key not in self.tables:
            self.tables[key] = self.f32(t)
        return self.tables[key]

    def table16(self, t):  # (gq_qtip_mlp_mid reads its factor tables as fp16: +-1 entries, checked by _pm1)
        t16 = t.detach().to(self.dev).half().contiguous()
        key = ("h", tuple(t16.shape), hash(t16.cpu().numpy().tobytes()))
        if key not in self.tables:
            self.tables[key] = self.hold(t16).data_ptr()
        return self.tables[key]


def _pm1(t):
    return bool((t.detach().float().abs() == 1.0).all())


def _p2(n):
    return n > 0 and (n & (n - 1)) == 0


class _QtipPlanner:
    """launch plans of the QTIP linears, per layer four groups of linears that share an input -- (q, k, v), (o), (gate, up), (down) --
    each a list of (entry point name, record) built once: SU as fp32, SV * 32 as fp32 (the values BitshiftLinear.forward multiplies
    with, bitshift.py:441,470), q/k/v landing in the packed buffer the attention kernel reads.  Per side of a linear: power-of-two
    width -> the fused kernels (gq_qtip_linear_in / _out); width with a Hadamard factor -> gq_qtip_transform around the bare matvec
    (GQ_QPRO_PRETRANSFORMED)."""

    def __init__(self, st):
        self.st, self.c, self.cp = st, st.m.config, st.copies
        self.fold, self.one_launch, self.out_seg, self.mlp_mid = qtip_fold(), qtip_one_launch(), qtip_out_seg(), qtip_mlp_mid()
        qw = self.c.n_head * self.c.head_dim
        self.attn_fold = qtip_attn_fold() and not self.one_launch and self.c.head_dim in (64, 128) and qw <= 8192 and _p2(qw)
        self.pre = qtip_pre() and not self.fold and not self.one_launch and 256 <= self.c.dim <= 8192 and _p2(self.c.dim)

    def ksplit(self, mods):
        """K ranges per band: the split with the fewest band-equivalents per block (wo, down: 128 bands on 256 units -> 2); for linears
        that share a launch (q / k / v: 384 bands on 256 units) 2 K ranges, 3 rounds of half a band"""
        if not qtip_ksplit() or (len(mods) > 1 and not qtip_ksplit_group()):
            return 1
        widths = (ctypes.c_uint32 * len(mods))(*[m.out_features for m in mods])
        return int(_lib.lib().gq_qtip_plan_ksplit(len(mods), widths, mods[0].in_features, 2 if len(mods) == 1 else 4))

    def outs(self, mods, idx, ysl, resid, outs, ks):
        """GqQtipOut descriptors of the linears `idx` of a group"""
        return self.cp.hold((_lib.GqQtipOut * len(idx))(*[
            _lib.GqQtipOut(ysl[i].data_ptr(), self.cp.f32(mods[i].SV, 32.0), resid, outs[i], mods[i].out_features, ks) for i in idx]))

    def group(self, mods, xp, x2p, normw, pro, outs, resid, prev=None, defer=None, out_to=None, parts_ok=False):
        """launches of one group: mods share the input vector xp (x2p for silu*mul); outs[i] fp16 destinations.
        prev: GqQtipOut of the linear that PRODUCES xp, its transform-out folded into this group's first launch (which then
        stores xp itself); defer = row of y32: this group's own transform-out is left to the consumer (-> returned descriptor)"""
        c, cp, y32, xs16 = self.c, self.cp, self.st.y32, self.st.xs16
        R, K, n = mods[0].K, mods[0].in_features, len(mods)
        plan = []
        # split-K partial sums are added by the consumer of the sums: the fused transform-out (single linears with a power-of-two
        # output width), the attention launch with the q / k / v transform-out folded in (out_to), gq_qtip_mlp_mid (parts_ok)
        if n == 1:
            ks = self.ksplit(mods) if mods[0].K_right == 1 else 1
        elif mods[0].K_left == 1 and ((out_to is not None and all(m.K_right == 1 for m in mods)) or parts_ok):
            ks = self.ksplit(mods)
        else:
            ks = 1
        ysl = [y32[defer]] if defer is not None else [y32[i] for i in range(n)]
        if mods[0].K_left == 1:  # fused transform-in + matvec, all linears in one launch
            arr = cp.hold((_lib.GqQtipIn * n)(*[_lib.GqQtipIn(m.trellis.data_ptr(), cp.f32(m.SU), m.tlut.data_ptr(), ysl[i].data_ptr(), m.out_features)
                                                for i, m in enumerate(mods)]))
            if prev is not None:
                plan.append(_launch(LinearIn(None, None, normw, c.norm_eps, pro, K, R, n, arr, 1, cp.hold((_lib.GqQtipOut * 1)(prev)), ks)))
            else:
                plan.append(_launch(LinearIn(xp, x2p, normw, c.norm_eps, pro, K, R, n, arr, 0, None, ks)))
        else:  # factor transform of the shared input (one launch), then the bare matvec per linear
            xf = cp.hold((_lib.GqQtipXf * n)(*[_lib.GqQtipXf(None, cp.f32(m.SU), cp.table(m.had_left), None, xs16[i].data_ptr())
                                               for i, m in enumerate(mods)]))
            plan.append(_launch(Transform(1, xp, x2p, normw, c.norm_eps, pro, n, xf, K, mods[0].K_left, 1)))
            assert prev is None
            for i, m in enumerate(mods):
                arr = cp.hold((_lib.GqQtipIn * 1)(_lib.GqQtipIn(m.trellis.data_ptr(), None, m.tlut.data_ptr(), ysl[i].data_ptr(), m.out_features)))
                plan.append(_launch(LinearIn(xs16[i].data_ptr(), None, None, 0.0, 3, K, R, 1, arr, 0, None, ks)))
        p2 = [i for i, m in enumerate(mods) if m.K_right == 1]
        fac = [i for i, m in enumerate(mods) if m.K_right != 1]
        # One launch for transform-in + matvec + transform-out (gq_qtip_linear: the block that finishes a linear last
        # transforms it): every linear of the group has a power-of-two output width, nothing is folded or deferred
        if (self.one_launch and defer is None and prev is None and not fac and plan and plan[-1][0] == LinearIn.entry
                and all(m.out_features <= 16384 for m in mods)):
            a = plan.pop()[1]
            ctr = cp.hold(torch.zeros(4, dtype=torch.int32, device=cp.dev))
            fin = self.outs(mods, range(n), ysl, resid, outs, ks)
            plan.append(_launch(Linear(a.x, a.x2, a.norm_weight, a.eps, a.prologue, a.K, a.R, a.n, a.lin, fin, ks, ctr.data_ptr())))
            return plan
        if out_to is not None and not fac:
            # the consumer rebuilds the outputs itself (q / k / v: gq_attn_decode_qtip, the transform-out inside the attention
            # launch): descriptors instead of the gq_qtip_linear_out launch
            out_to.append(self.outs(mods, range(n), ysl, None, outs, ks))
            return plan
        if defer is not None:  # (a single linear with a power-of-two output width)
            arr = self.outs(mods, [0], ysl, resid, outs, ks)
            return plan, arr[0], [_launch(LinearOut(1, arr))]
        if p2:
            # M / 128 blocks per linear instead of one (GQ_QTIP_OUT_SEG, default ON; equal up to fp32 rounding): 2.9 vs 4.6 us
            seg = self.out_seg and all(128 <= mods[i].out_features <= 8192 for i in p2)
            plan.append(_launch(LinearOut(len(p2), self.outs(mods, p2, ysl, resid, outs, ks)), OUT_ENTRIES[1 if seg else 0]))
        for Kf, M in sorted({(mods[i].K_right, mods[i].out_features) for i in fac}):
            idx = [i for i in fac if (mods[i].K_right, mods[i].out_features) == (Kf, M)]
            xf = cp.hold((_lib.GqQtipXf * len(idx))(*[_lib.GqQtipXf(ysl[i].data_ptr(), cp.f32(mods[i].SV, 32.0), cp.table(mods[i].had_right), resid, outs[i])
                                                      for i in idx]))
            plan.append(_launch(Transform(0, None, None, None, 0.0, 0, len(idx), xf, M, Kf, 0)))
        return plan

    def layer(self, b, prev_down):
        """(QtipLayer of block b, GqQtipOut of its down projection when the next layer's q / k / v launch is to rebuild it)"""
        st, c, fold = self.st, self.c, self.fold
        at, ff = b.attention, b.feed_forward
        x, h, y, g, u = (t.data_ptr() for t in (st.x, st.h, st.y, st.g, st.u))
        qw, e = c.n_head * c.head_dim, st.qkv.element_size()
        qkv_outs = [st.qkv.data_ptr(), st.qkv.data_ptr() + qw * e, st.qkv.data_ptr() + (qw + c.n_local_heads * c.head_dim) * e]
        norm_in, norm_post = b.input_layernorm.weight.data_ptr(), b.post_attention_layernorm.weight.data_ptr()
        can_o = fold and at.wo.K_right == 1 and ff.w1.K_left == 1
        can_d = fold and ff.w2.K_right == 1 and at.wq.K_left == 1
        w1, w3, w2 = ff.w1, ff.w3, ff.w2
        n_mlp, Kf = w2.in_features, w2.K_left
        mid_ok = (self.mlp_mid and not can_o and not self.one_launch and Kf != 1 and w1.K_right == Kf and w3.K_right == Kf and n_mlp == Kf * 64
                  and Kf <= 176 and Kf % 4 == 0 and w1.K_left == 1 and w3.K_left == 1 and w2.K_right == 1
                  and w1.out_features == n_mlp and w3.out_features == n_mlp
                  and torch.equal(w1.had_right, w3.had_right) and _pm1(w1.had_right) and _pm1(w2.had_left))
        qkv_mods = [at.wq, at.wk, at.wv]
        fold_here = self.attn_fold and all(m.K_right == 1 for m in qkv_mods)
        desc = [] if fold_here else None
        qkv = self.group(qkv_mods, x, None, norm_in, 1, qkv_outs, None, out_to=desc)
        # (q / k / v of this layer with the previous layer's down folded in; the first layer of a range takes the plain form)
        qkv_f = self.group(qkv_mods, None, None, norm_in, 1, qkv_outs, None, prev=prev_down, out_to=[] if fold_here else None) \
            if prev_down is not None else None
        if can_o:
            o, desc_o, _ = self.group([at.wo], y, None, None, 0, [h], x, defer=3)
            gu = self.group([w1, w3], None, None, norm_post, 1, [g, u], None, prev=desc_o)
        else:
            o = self.group([at.wo], y, None, None, 0, [h], x)
            gu = self.group([w1, w3], h, None, norm_post, 1, [g, u], None, parts_ok=mid_ok)
        if can_d:
            d, prev_down, d_out = self.group([w2], g, u, None, 2, [x], h, defer=4)
        else:
            d, prev_down, d_out = self.group([w2], g, u, None, 2, [x], h), None, None
        if mid_ok:
            gu, d = self.with_mlp_mid(gu, d, w1, w3, w2)
        return QtipLayer(qkv=qkv, qkv_f=qkv_f, attn_qt=desc[0] if fold_here else None, o=o, gu=gu, d=d, d_out=d_out), prev_down

    def with_mlp_mid(self, gu, d, w1, w3, w2):
        """GQ_QTIP_MLP_MID: gate / up's output-side transform and down's input-side transform as gq_qtip_mlp_mid + gq_qtip_linear_in_rows"""
        st, cp = self.st, self.cp
        n_mlp, Kf = w2.in_features, w2.K_left
        assert (gu[-1][0] == Transform.entry and d[0][0] == Transform.entry and d[1][0] == LinearIn.entry
                and d[1][1].prologue == 3), "unexpected launch plan of a factor-width MLP"
        if st.z32 is None:
            st.z32 = torch.zeros(max(self.c.dim, self.c.intermediate_size), dtype=torch.float32, device=cp.dev)
        mid = cp.hold(_lib.GqQtipMid(st.y32[0].data_ptr(), st.y32[1].data_ptr(), cp.f32(w1.SV, 32.0), cp.f32(w3.SV, 32.0),
                                     cp.table16(w1.had_right.t()), cp.f32(w2.SU), cp.table16(w2.had_left), st.z32.data_ptr(), None, None))
        a_in = d[1][1]  # down's bare matvec on the transformed input
        return gu[:-1], [_launch(MlpMid(ctypes.pointer(mid), gu[0][1].ksplit, n_mlp, Kf)),  # (the split-K parts of the gate / up sums)
                         _launch(LinearInRows(st.z32.data_ptr(), n_mlp, 64, a_in.R, 1, a_in.lin, a_in.ksplit))] + d[2:]

    def with_pre(self, plan_out, plan_in, normw, mods):
        """GQ_QTIP_PRE: (plan of the producer with its last launch -- the transform-out -- replaced, plan of the consumers' matvec
        launch on the pre-transformed vectors), or None when the launches are not of the plain form"""
        if not (self.pre and plan_out and plan_in and plan_out[-1][0] in OUT_ENTRIES and plan_out[-1][1].n == 1 and plan_in[0][0] == LinearIn.entry):
            return None
        a_in, xt, cp, n = plan_in[0][1], self.st.xt, self.cp, len(mods)
        if not (a_in.prologue == 1 and a_in.n_prev == 0 and all(m.K_left == 1 and m.in_features == self.c.dim for m in mods)):
            return None
        su = cp.hold((ctypes.c_void_p * n)(*[cp.f32(m.SU) for m in mods]))
        xts = cp.hold((ctypes.c_void_p * n)(*[xt[i].data_ptr() for i in range(n)]))
        arr = cp.hold((_lib.GqQtipIn * n)(*[_lib.GqQtipIn(lin.trellis, xt[i].data_ptr(), lin.tlut, lin.y32, lin.M) for i, lin in zip(range(n), a_in.lin)]))
        return (plan_out[:-1] + [_launch(LinearOutIn(plan_out[-1][1].lin, normw, self.c.norm_eps, n, su, xts))],
                [_launch(a_in._replace(x=None, x2=None, norm_weight=None, eps=0.0, prologue=3, n=n, lin=arr))] + plan_in[1:])

    def pre_pass(self, layers):
        """GQ_QTIP_PRE over the finished plans: wo -> gate / up inside a layer, down -> the next layer's q / k / v"""
        blocks = self.st.m.layers
        for d, b in zip(layers, blocks):
            r = self.with_pre(d.o, d.gu, b.post_attention_layernorm.weight.data_ptr(), [b.feed_forward.w1, b.feed_forward.w3])
            if r is not None:
                d.o, d.gu = r
        for d, nd, nb in zip(layers, layers[1:], blocks[1:]):
            r = self.with_pre(d.d, nd.qkv, nb.input_layernorm.weight.data_ptr(), [nb.attention.wq, nb.attention.wk, nb.attention.wv])
            if r is not None and d.d_out is None:
                d.d_pre, nd.qkv_pre = r


class QtipStep(StepState):

    def __init__(self, model):
        super().__init__(model)
        if self.kv8:
            raise NotImplementedError("fp8 KV cache: QTIP models keep the fp16 cache (gq_attn_decode_qtip has no fp8 form)")
        c, dev = model.config, self.x.device
        self.g = torch.zeros(c.intermediate_size, dtype=torch.float16, device=dev)
        self.u = torch.zeros(c.intermediate_size, dtype=torch.float16, device=dev)
        mmax = max(c.dim, c.intermediate_size)
        # [linear][split-K part][M]; rows 3 / 4: the sums of wo / down while their transform-out is folded into the next launch
        self.y32 = torch.zeros(5, 4 * mmax, dtype=torch.float32, device=dev)
        self.xs16 = torch.zeros(3, mmax, dtype=torch.float16, device=dev)  # transformed inputs (factor widths)
        self.xt = torch.zeros(3, c.dim, dtype=torch.float16, device=dev)   # pre-transformed inputs (GQ_QTIP_PRE)
        self.z32 = None                                                    # column sums of gq_qtip_mlp_mid, when a layer takes it
        self.copies = _Copies(dev)
        planner = _QtipPlanner(self)
        self.qtip_layers, prev_down = [], None
        for b in model.layers:
            layer, prev_down = planner.layer(b, prev_down)
            self.qtip_layers.append(layer)
        planner.pre_pass(self.qtip_layers)

    def layers(self, x, pos, l0, l1, slot=0, ssq_ready=False):
        """one decode step of layers [l0, l1) of an unfused QTIP model (A = transform-in + trellis matvec, B = transform-out):
        A(q,k,v | RMSNorm) B(q,k,v) attention A(o) B(o + residual) A(gate,up | RMSNorm) B(gate,up) A(down | silu*mul)
        B(down + residual) -- 9 launches per layer with power-of-two widths; a width with a Hadamard factor replaces the A / B
        on its side by gq_qtip_transform (+ the bare matvec): 11 launches for Llama-2-7b / 70b (MLP width only)."""
        L = _lib.lib()
        sp = _lib.current_stream_ptr()
        assert x.data_ptr() == self.x.data_ptr(), "the QTIP launch plans are bound to the model's own hidden-state buffer"

        def run(plan):
            for name, args in plan:
                _lib.check(getattr(L, name)(*args, sp), name)

        pending = None  # transform-out of the previous layer's down projection, not yet run
        pre_in = False  # the previous layer's down launch left this layer's q / k / v inputs pre-transformed
        for li in range(l0, l1):
            d, at = self.qtip_layers[li], self.m.layers[li].attention
            if pre_in:
                run(d.qkv_pre)
            elif pending is not None and d.qkv_f is not None:
                run(d.qkv_f)  # (rebuilds and stores the hidden state itself)
            else:
                if pending is not None:
                    run(pending)
                run(d.qkv)
            if d.attn_qt is not None:
                self.attend("gq_attn_decode_qtip", d.attn_qt, pos, self.kv(at, slot), sp)
            else:
                self.attend("gq_attn_decode_split", self.qkv.data_ptr(), pos, self.kv(at, slot), sp)
            run(d.o)
            run(d.gu)
            pre_in = li + 1 < l1 and d.d_pre is not None
            run(d.d_pre if pre_in else d.d)
            pending = d.d_out
        if pending is not None:
            run(pending)
