"""The host side of the fused sampler (csrc/sampler.hip): its device state, its validation and its one C call.

Every decode route that draws on the device -- `generate.DecodeGraph`, route 2's `_CapturedStep`, `tp.TensorParallelDecoder`,
`pipeline.PipelinedDecoder` -- owns one `FusedSampler` and ends its token step with `launch`.  Which entry point a configuration
needs is decided here and nowhere else:
  * log-probabilities                  -> gq_sample_topk_lp;
  * top_logprobs = n > 0               -> the entry with the suffix _topn (gq_sample_topk_lp_topn / gq_sample_full_topn, csrc/topn.hip): the
                                          same draw, and two launches behind it for the n alternatives.  n = 0 calls what it called;
  * a penalty or a suppress list       -> gq_sample_topk_rep (the instances over fp32 candidate values and the token sets);
  * everything else                    -> gq_sample_topk_p -- never _rep or _lp with neutral arguments: those launch the fp32-key
                                          instances, about 10.8 us per token more;
  * a workspace of 32 candidates/block -> gq_sample_topk, the narrow call of the layer pipeline (draw only: no ban, no sequence store);
  * no top_k (None / 0), top_k > 64, or min_p > 0 -> gq_sample_full (csrc/sampler_full.hip: the whole vocabulary; it serves the penalty,
                                          the sets and the log-probabilities itself, from its own workspace);
  * frequency_penalty / presence_penalty != 0 or a logit_bias -> the entry with the suffix _adj (gq_sample_topk_adj / gq_sample_full_adj, by
                                          the rule above), which takes everything the others take.  Without the three the sampler makes
                                          exactly the calls listed above;
  * token_fsm = a TokenFSM             -> the entry with the suffix _fsm (gq_sample_topk_fsm / gq_sample_full_fsm, by the same rule): the _adj
                                          entry's parameters and the machine's tables; constrained decoding inside the same launches.
                                          Without a machine the sampler makes exactly the calls listed above.
"""
import ctypes
import math

import torch

from . import _lib
from .token_fsm import TokenFSM

BLOCKS = 128  # (stage 1's grid: the workspace holds `candidates` entries of each block)


def check_top_logprobs(n, logprobs):
    """top_logprobs as an int: 0 / None = off, else 1 .. _lib.TOPN_MAX and only next to the log-probabilities (ValueError otherwise)"""
    if n is None or n is False:
        return 0
    if isinstance(n, bool) or int(n) != n or not 0 <= int(n) <= _lib.TOPN_MAX:
        raise ValueError(f"top_logprobs must be an integer in 1..{_lib.TOPN_MAX} (0 / None: off), not {n!r}")
    if int(n) and not logprobs:
        raise ValueError("top_logprobs needs the log-probabilities (logprobs=True / output_logprobs=True): the list is normalised by lp_raw's log-sum-exp")
    return int(n)


def check_logit_bias(logit_bias, vocab_size):
    """logit_bias as {int id: float}: None / empty = off; a dict (ids as ints or, as serving APIs send them, as strings) of finite values
    with ids in [0, vocab_size) (ValueError otherwise)"""
    if logit_bias is None:
        return {}
    if not isinstance(logit_bias, dict):
        raise ValueError(f"logit_bias must be a dict {{token id: bias}}, not {type(logit_bias).__name__}")
    out = {}
    for k, v in logit_bias.items():
        try:
            if isinstance(k, (bool, float)):
                raise ValueError
            t = int(k)
            b = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"logit_bias: {k!r}: {v!r} is no (token id, number) pair") from None
        if not 0 <= t < vocab_size:
            raise ValueError(f"logit_bias: token id {t} is outside [0, {vocab_size})")
        if not math.isfinite(b) or not math.isfinite(torch.tensor(b, dtype=torch.float32).item()):
            raise ValueError(f"logit_bias: the bias of token {t} must be a finite fp32 number, not {v!r}")
        if t in out:
            raise ValueError(f"logit_bias: token id {t} is listed twice")
        out[t] = b
    return out


def check_additive_penalty(name, x):
    """frequency_penalty / presence_penalty as a float: None = 0; finite (ValueError otherwise).  Negative values are served: they reward."""
    try:
        f = 0.0 if x is None else float(x)
    except (TypeError, ValueError):
        f = math.nan
    if isinstance(x, (bool, str)) or not math.isfinite(f) or not math.isfinite(torch.tensor(f, dtype=torch.float32).item()):
        raise ValueError(f"{name} must be a finite number (0 = off), not {x!r}")
    return f


class FusedSampler:
    """State: `counter` (the RNG counter word), `work_val` / `work_idx` (stage 1's candidates; a whole-vocabulary configuration -- `full`: top_k
    None / 0 / above 64, or min_p > 0 -- has `ws`, gq_sample_full's workspace, instead), `ban` (int32 {n, until_pos, id0..id3}:
    tokens that cannot be drawn while pos < until_pos) -- and, only when asked for, `seq` (seq_capacity > 0: every drawn token at
    seq[pos + 1]), `seen` / `suppress` (a penalty != 1 or a suppress list: uint32 bitmaps over the vocabulary; every drawn token joins
    `seen` on the device), `lp_ws` / `lp_raw` / `lp_drawn` (logprobs: the log-probability of every drawn token at [pos + 1], under the
    model's unprocessed distribution and under the one the draw was made from), `top_ids` / `top_lps` / `topn_ws` (top_logprobs = n in
    1..20, with logprobs: int32 / fp32 [seq_capacity, n], row [pos + 1] = the n most probable tokens of the unprocessed distribution and
    their log-probabilities, against the log-sum-exp lp_raw is taken against), `bias_set` / `bias` (a logit_bias: the bitmap of the
    listed ids and fp32 [vocab], built once in the constructor), `out_set` / `out_count` (a frequency_penalty or presence_penalty != 0: the
    bitmap and the uint32 counts of the tokens generated in THIS request -- every drawn token is counted on the device;
    `reset_generated()` at the start of every request), `fsm_tables` / `fsm_masks` / `fsm_state` (a token_fsm: the machine's CSR tables, its
    mask rows -- uint32 [n_states, ceil(vocab / 32)], a state's FORBIDDEN set joined with the suppress list, built once in the constructor
    by gq_token_fsm_build -- and the device word every draw reads its row by and moves; `reset_fsm()` at the start of every request).  A
    request without them allocates nothing extra."""

    def __init__(self, vocab_size, device, top_k, top_p=1.0, temperature=1.0, seed=1234, seq_capacity=0, repetition_penalty=1.0,
                 suppress_tokens=(), logprobs=False, candidates=64, min_p=0.0, top_logprobs=0, frequency_penalty=0.0, presence_penalty=0.0,
                 logit_bias=None, token_fsm=None):
        self.min_p = float(min_p or 0.0)
        if not 0.0 <= self.min_p <= 1.0:
            raise ValueError(f"min_p must be in [0, 1], not {min_p!r}")
        if top_k is not None and int(top_k) < 0:
            raise ValueError(f"top_k must be None or >= 0, not {top_k!r}")
        # the whole-vocabulary entry: no top-k filter (None / 0), more candidates than the 64 of the two-stage kernels, or min_p
        self.full = top_k is None or int(top_k) == 0 or int(top_k) > 64 or self.min_p > 0.0
        top_k = int(top_k or 0) if self.full else top_k
        self.vocab_size, self.top_k, self.top_p, self.temperature, self.seed = int(vocab_size), top_k, float(top_p or 1.0), float(temperature), int(seed)
        self.repetition_penalty = float(repetition_penalty if repetition_penalty is not None else 1.0)
        suppress_tokens = [int(t) for t in (suppress_tokens if suppress_tokens is not None else ())]
        self.logprobs, self.narrow = bool(logprobs), candidates == 32
        self.top_logprobs = check_top_logprobs(top_logprobs, self.logprobs)
        if not (self.repetition_penalty > 0.0 and self.repetition_penalty != float("inf")):
            raise ValueError(f"repetition_penalty must be finite and > 0, not {repetition_penalty!r}")
        if self.logprobs and not seq_capacity:
            raise ValueError("logprobs=True needs seq_capacity > 0: the log-probabilities are stored where the tokens are")
        if self.narrow and (seq_capacity or self.repetition_penalty != 1.0 or suppress_tokens or self.top_p != 1.0):
            raise ValueError("a workspace of 32 candidates per block serves the draw alone (gq_sample_topk)")
        if self.narrow and self.full:
            raise ValueError("a workspace of 32 candidates per block serves top_k in 1..32 without min_p (gq_sample_topk)")
        self.frequency_penalty = check_additive_penalty("frequency_penalty", frequency_penalty)
        self.presence_penalty = check_additive_penalty("presence_penalty", presence_penalty)
        self.logit_bias = check_logit_bias(logit_bias, int(vocab_size))
        counted = self.frequency_penalty != 0.0 or self.presence_penalty != 0.0
        self.adjusted = counted or bool(self.logit_bias)  # (the entries with the suffix _adj)
        if self.narrow and self.adjusted:
            raise ValueError("a workspace of 32 candidates per block serves the draw alone (gq_sample_topk)")
        if token_fsm is not None and not isinstance(token_fsm, TokenFSM):
            raise ValueError(f"token_fsm must be a guidedquant_amd.token_fsm.TokenFSM, not {type(token_fsm).__name__}")
        if self.narrow and token_fsm is not None:
            raise ValueError("token_fsm: a workspace of 32 candidates per block serves the draw alone (gq_sample_topk)")
        self.token_fsm = token_fsm
        if token_fsm is not None:
            token_fsm.check(self.vocab_size)  # (ids inside the vocabulary, no dead end, the size of the masks)
            for s in token_fsm._reachable if suppress_tokens else ():  # (the suppress list joins every state's forbidden set)
                if token_fsm.default_next[s] < 0 and not set(token_fsm.allowed(s).tolist()) - set(suppress_tokens):
                    raise ValueError(f"token_fsm: state {s} allows no token that suppress_tokens leaves (a dead end)")

        def z(n, dtype=torch.int32):
            return torch.zeros((int(n), ), dtype=dtype, device=device)
        self.counter, self.ban = z(1), z(6)
        self.work_val = self.work_idx = self.ws = None
        if self.full:
            self.ws = z(_lib.lib().gq_sample_full_ws_bytes(self.vocab_size) // 8, torch.int64)  # (the 128 x 64 work buffers are not needed)
            if not self.ws.numel():
                raise ValueError(f"the fused sampler serves vocabularies up to {_lib.SAMPLER_MAX_VOCAB}, not {self.vocab_size}")
        else:
            self.work_val, self.work_idx = z(BLOCKS * candidates, torch.float32), z(BLOCKS * candidates)
        self.seq = z(seq_capacity) if seq_capacity else None
        self.seen = self.suppress = self.lp_ws = self.lp_raw = self.lp_drawn = None
        if self.repetition_penalty != 1.0 or suppress_tokens:
            words = (self.vocab_size + 31) // 32
            self.seen = z(words)
            if suppress_tokens:
                self.suppress = z(words)
                self.build_set(self.suppress, torch.tensor(suppress_tokens, dtype=torch.int32, device=device))
        if self.logprobs:
            self.lp_raw, self.lp_drawn = z(seq_capacity, torch.float32), z(seq_capacity, torch.float32)
            self.lp_ws = z(_lib.SAMPLER_LP_WS, torch.float32) if not self.full else None
        self.top_ids = self.top_lps = self.topn_ws = None
        if self.top_logprobs:
            n = self.top_logprobs
            self.top_ids, self.top_lps = z(seq_capacity * n).view(seq_capacity, n), z(seq_capacity * n, torch.float32).view(seq_capacity, n)
            self.topn_ws = z(_lib.TOPN_WS_BYTES // 8, torch.int64)
        self.bias_set = self.bias = self.out_set = self.out_count = self._adj = None
        if self.adjusted:
            words = (self.vocab_size + 31) // 32
            if self.logit_bias:
                self.bias_set, self.bias = z(words), z(self.vocab_size, torch.float32)
                ids = torch.tensor(list(self.logit_bias), dtype=torch.int32, device=device)
                values = torch.tensor(list(self.logit_bias.values()), dtype=torch.float32, device=device)
                _lib.check(_lib.lib().gq_token_bias_build(ids.data_ptr(), values.data_ptr(), ids.numel(), self.vocab_size, self.bias_set.data_ptr(),
                                                         self.bias.data_ptr(), _lib.current_stream_ptr()), "gq_token_bias_build")
            if counted:
                self.out_set, self.out_count = z(words), z(self.vocab_size)
            # (the struct is read by the C call on the host, at launch and at capture time: it lives as long as the sampler)
            self._adj = _lib.GqSampleAdjust(self.frequency_penalty, self.presence_penalty, *(t.data_ptr() if t is not None else None for t in
                                                                                          (self.bias_set, self.bias, self.out_set, self.out_count)))

        self.fsm_tables = self.fsm_masks = self.fsm_state = self._fsm = None
        if token_fsm is not None:
            f, words = token_fsm, (self.vocab_size + 31) // 32
            # (a machine without edges still gets one word per edge table: the C call takes no NULL for edge_next)
            self.fsm_tables = tuple(torch.tensor(a.tolist() or [0], dtype=torch.int32, device=device)
                                    for a in (f.row_ptr, f.edge_tok, f.edge_next, f.default_next))
            self.fsm_masks, self.fsm_state = z(f.n_states * words).view(f.n_states, words), z(1)
            _lib.check(_lib.lib().gq_token_fsm_build(*(t.data_ptr() for t in self.fsm_tables), f.n_states, self.vocab_size,
                                                    self.suppress.data_ptr() if self.suppress is not None else None, self.fsm_masks.data_ptr(),
                                                    _lib.current_stream_ptr()), "gq_token_fsm_build")
            self._fsm = _lib.GqTokenFsm(self.fsm_masks.data_ptr(), words, f.n_states, *(t.data_ptr() for t in self.fsm_tables), self.fsm_state.data_ptr())
            self.reset_fsm()

    def build_set(self, words, ids, clear=True):
        """words = (clear: the set of `ids`; else: joined by `ids`), one launch outside any graph"""
        ids = ids.to(device=words.device, dtype=torch.int32).contiguous().view(-1)
        _lib.check(_lib.lib().gq_token_set_build(ids.data_ptr() if ids.numel() else None, ids.numel(), self.vocab_size, words.data_ptr(),
                                                1 if clear else 0, _lib.current_stream_ptr()), "gq_token_set_build")

    def set_history(self, ids):
        """the sequence so far (a tensor or list of token ids: the prompt, with whatever was generated before): `seen` is cleared and
        rebuilt from it.  Before the first step of every request; without a penalty or a suppress list there is no set and nothing happens."""
        if self.seen is not None:
            self.build_set(self.seen, ids if torch.is_tensor(ids) else torch.tensor(list(ids), dtype=torch.int32))

    def set_ban(self, eos_ids, until_pos):
        """the (at most 4) tokens that cannot be drawn while pos < until_pos: HF's min_new_tokens on EOS"""
        eos_ids = [int(e) for e in eos_ids]
        self.ban.copy_(torch.tensor([len(eos_ids), int(until_pos)] + eos_ids + [0] * (4 - len(eos_ids)), dtype=torch.int32))

    def reseed(self, word):
        """the start of the counter stream (a device word or an int): the captured launches read it from device memory"""
        if torch.is_tensor(word):
            self.counter.copy_(word)
        else:
            self.counter.fill_(int(word))

    def reset_generated(self):
        """the start of a request: nothing has been generated yet -- `out_set` and `out_count` are cleared (the prompt does not count;
        `set_history` does not touch them).  Without a frequency or presence penalty there is no count and nothing happens."""
        if self.out_set is not None:
            self.out_set.zero_()
            self.out_count.zero_()

    def count_generated(self, ids):
        """tokens this request generated OUTSIDE the sampler (a first token drawn from the prompt pass's logits) join the counts: one
        index_add and one set build, outside any graph.  Without a frequency or presence penalty nothing happens."""
        if self.out_set is not None:
            ids = (ids if torch.is_tensor(ids) else torch.tensor(list(ids))).to(device=self.out_count.device, dtype=torch.int64).view(-1)
            self.out_count.index_add_(0, ids, torch.ones_like(ids, dtype=torch.int32))
            self.build_set(self.out_set, ids, clear=False)

    def reset_fsm(self, state=None):
        """the start of a request: the machine is in `state` (None: its start state).  Next to set_history / reset_generated; without a
        token_fsm nothing happens."""
        if self.token_fsm is not None:
            self._fsm_host = self.token_fsm._state(state)
            self.fsm_state.fill_(self._fsm_host)

    def advance_fsm(self, ids):
        """tokens this request produced OUTSIDE the sampler (a first token drawn from the prompt pass's logits) move the machine: walked on
        the host from the state reset_fsm / the last advance_fsm left, and the state word written.  ValueError at a token the machine
        forbids.  Without a token_fsm nothing happens."""
        if self.token_fsm is not None:
            ids = ids.view(-1).tolist() if torch.is_tensor(ids) else list(ids)
            self.reset_fsm(self.token_fsm.walk(ids, self._fsm_host))

    def clear_warmup(self):
        """the warm-up and capture-time draws joined `seen`, were counted and moved the machine: their bits and counts go, the state is
        the start state again"""
        if self.seen is not None:
            self.seen.zero_()
        self.reset_generated()
        self.reset_fsm()

    def launch(self, logits, tok_io, pos_io, next_tok, embed_table=None, x_out=None, dim=0, ssq_out=None):
        """one draw from `logits` on the current stream: the token to `next_tok` and, fed back, to `tok_io`, with `pos_io` advanced;
        embed_table / x_out / dim / ssq_out: the last block also writes the NEXT step's hidden state and its hand-over statistics"""
        def p(t):
            return t.data_ptr() if t is not None else None
        if self.full:
            args = (p(logits), self.vocab_size, int(self.top_k), self.top_p, self.min_p, self.temperature, self.seed, p(self.counter), p(self.ws),
                    self.ws.numel() * 8, p(tok_io), p(pos_io), p(next_tok), p(self.ban), p(self.seq), self.seq.numel() if self.seq is not None else 0,
                    p(embed_table), p(x_out), dim, p(ssq_out), self.repetition_penalty, p(self.seen), p(self.suppress), p(self.lp_raw), p(self.lp_drawn),
                    self.lp_raw.numel() if self.lp_raw is not None else 0)
            name = "gq_sample_full"
            if self.token_fsm is not None:
                name, args = "gq_sample_full_fsm", args + (self.top_logprobs, p(self.top_ids), p(self.top_lps), p(self.topn_ws),
                                                           ctypes.byref(self._adj) if self.adjusted else None, ctypes.byref(self._fsm))
            elif self.adjusted:
                name, args = "gq_sample_full_adj", args + (self.top_logprobs, p(self.top_ids), p(self.top_lps), p(self.topn_ws), ctypes.byref(self._adj))
            elif self.top_logprobs:
                name, args = "gq_sample_full_topn", args + (self.top_logprobs, p(self.top_ids), p(self.top_lps), p(self.topn_ws))
            return _lib.check(getattr(_lib.lib(), name)(*args, _lib.current_stream_ptr()), name)
        draw = (self.temperature, self.seed, p(self.counter), p(self.work_val), p(self.work_idx), p(tok_io), p(pos_io), p(next_tok))
        if self.narrow:
            name, args = "gq_sample_topk", (p(logits), self.vocab_size, int(self.top_k)) + draw
        else:
            name, args = "gq_sample_topk_p", (p(logits), self.vocab_size, int(self.top_k), self.top_p) + draw + (
                p(self.ban), p(self.seq), self.seq.numel() if self.seq is not None else 0, p(embed_table), p(x_out), dim, p(ssq_out))
            if self.adjusted or self.token_fsm is not None:  # (everything the others take: the sets and the log-probability arrays that do not exist go as NULL)
                name, args = "gq_sample_topk_adj", args + (
                    self.repetition_penalty, p(self.seen), p(self.suppress), p(self.lp_ws), p(self.lp_raw), p(self.lp_drawn),
                    self.lp_raw.numel() if self.lp_raw is not None else 0, self.top_logprobs, p(self.top_ids), p(self.top_lps), p(self.topn_ws),
                    ctypes.byref(self._adj) if self.adjusted else None)
                if self.token_fsm is not None:
                    name, args = "gq_sample_topk_fsm", args + (ctypes.byref(self._fsm), )
            elif self.logprobs or self.seen is not None:
                name, args = "gq_sample_topk_rep", args + (self.repetition_penalty, p(self.seen), p(self.suppress))
            if self.logprobs and not self.adjusted and self.token_fsm is None:
                name, args = "gq_sample_topk_lp", args + (p(self.lp_ws), p(self.lp_raw), p(self.lp_drawn), self.lp_raw.numel())
            if self.top_logprobs and not self.adjusted and self.token_fsm is None:
                name, args = "gq_sample_topk_lp_topn", args + (self.top_logprobs, p(self.top_ids), p(self.top_lps), p(self.topn_ws))
        _lib.check(getattr(_lib.lib(), name)(*args, _lib.current_stream_ptr()), name)
