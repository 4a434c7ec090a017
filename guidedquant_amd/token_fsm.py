"""The host description of a token-level finite state machine for constrained decoding (include/gq_hip.h: gq_sample_topk_fsm,
gq_sample_full_fsm, gq_token_fsm_build).

A machine is what an Outlines-style index is after a regex or a JSON schema has been compiled against a tokenizer's vocabulary: state ->
allowed tokens -> next state.  The compiler is out of scope here (it needs the vocabulary's strings); this class takes what it emits,
validates it and keeps the canonical CSR form the device tables are copied from:

    row_ptr[S + 1]     int32   the edges of state s are [row_ptr[s], row_ptr[s + 1])
    edge_tok[E]        int32   strictly ascending inside a row
    edge_next[E]       int32   the state behind the token; -1: the token is FORBIDDEN in this state (an exception in a state with a default)
    default_next[S]    int32   a token without an edge: -1 = forbidden, >= 0 = allowed and leads there ("free text" without 128k edges)

`FusedSampler(token_fsm=...)` builds the device tables, the mask rows (S * ceil(V / 32) * 4 bytes: 16 KB per state at 128256 tokens) and
the state word from it.  The vocabulary is known there, not here: `check(vocab_size)` is the part of the validation that needs it.
"""
import hashlib

import numpy as np

MAX_MASK_BYTES = 256 << 20


def _int(x, what):
    if isinstance(x, (bool, float, str)) or x is None:
        raise ValueError(f"token_fsm: {what} must be an integer, not {x!r}")
    try:
        i = int(x)
    except (TypeError, ValueError):
        raise ValueError(f"token_fsm: {what} must be an integer, not {x!r}") from None
    if i != x:
        raise ValueError(f"token_fsm: {what} must be an integer, not {x!r}")
    return i


class TokenFSM:
    """TokenFSM(n_states, edges, default_next=None, start=0): `edges` an iterable of (state, token, next_state), next_state -1 = the token
    is forbidden in that state; default_next a sequence of n_states entries (None: all -1).  ValueError, one message per mistake: a state
    outside [0, n_states), a token id < 0 (or, with `vocab_size`, outside [0, vocab_size)), a duplicate (state, token), a state reachable
    from `start` with no allowed token, masks above `max_mask_bytes`."""

    def __init__(self, n_states, edges, default_next=None, start=0, vocab_size=None, max_mask_bytes=MAX_MASK_BYTES):
        S = _int(n_states, "n_states")
        if S < 1:
            raise ValueError(f"token_fsm: n_states must be >= 1, not {S}")
        if S > 2**31 - 1:
            raise ValueError(f"token_fsm: n_states must fit an int32, not {S}")
        self.n_states = S
        self.start = _int(start, "start")
        if not 0 <= self.start < S:
            raise ValueError(f"token_fsm: start state {self.start} is outside [0, {S})")
        if default_next is None:
            dn = np.full(S, -1, dtype=np.int64)
        else:
            dn = np.array([_int(d, "default_next") for d in default_next], dtype=np.int64).reshape(-1)
            if dn.size != S:
                raise ValueError(f"token_fsm: default_next has {dn.size} entries for {S} states")
            bad = np.nonzero((dn < -1) | (dn >= S))[0]
            if bad.size:
                raise ValueError(f"token_fsm: default_next[{int(bad[0])}] = {int(dn[bad[0]])} is neither -1 nor a state in [0, {S})")
        rows = [(_int(s, "an edge's state"), _int(t, "an edge's token"), _int(n, "an edge's next state")) for s, t, n in edges]
        e = np.array(rows, dtype=np.int64).reshape(-1, 3)
        for col, what in ((0, "state"), (2, "next state")):
            lo = -1 if col == 2 else 0
            bad = np.nonzero((e[:, col] < lo) | (e[:, col] >= S))[0]
            if bad.size:
                s, t, n = (int(v) for v in e[bad[0]])
                raise ValueError(f"token_fsm: edge ({s}, {t}, {n}): {what} {int(e[bad[0], col])} is outside [{lo}, {S})")
        bad = np.nonzero((e[:, 1] < 0) | (e[:, 1] > 2**31 - 1))[0]
        if bad.size:
            s, t, n = (int(v) for v in e[bad[0]])
            raise ValueError(f"token_fsm: edge ({s}, {t}, {n}): token id {t} is outside [0, 2^31)")
        order = np.lexsort((e[:, 1], e[:, 0]))  # by state, then by token: the canonical form does not depend on the order of `edges`
        e = e[order]
        dup = np.nonzero((e[1:, 0] == e[:-1, 0]) & (e[1:, 1] == e[:-1, 1]))[0]
        if dup.size:
            raise ValueError(f"token_fsm: (state {int(e[dup[0], 0])}, token {int(e[dup[0], 1])}) is listed twice")
        self.row_ptr = np.zeros(S + 1, dtype=np.int32)
        np.cumsum(np.bincount(e[:, 0], minlength=S), out=self.row_ptr[1:])
        self.edge_tok, self.edge_next, self.default_next = e[:, 1].astype(np.int32), e[:, 2].astype(np.int32), dn.astype(np.int32)
        for a in (self.row_ptr, self.edge_tok, self.edge_next, self.default_next):
            a.setflags(write=False)
        self.vocab_size = None
        self._reachable = self._reach()
        # a dead end that shows without the vocabulary: everything forbidden by default and no edge that allows
        for s in self._reachable:
            if self.default_next[s] < 0 and not (self._row(s)[1] >= 0).any():
                raise ValueError(f"token_fsm: state {s} is reachable from state {self.start} and allows no token (a dead end)")
        if vocab_size is not None:
            self.check(vocab_size, max_mask_bytes)

    # ---- constructors ----
    @classmethod
    def from_index(cls, index, start=0, **kw):
        """{state: {token: next_state}}: the shape an Outlines index has.  The states are 0 .. the largest id that occurs; a token
        without an entry is forbidden."""
        if not isinstance(index, dict) or not index:
            raise ValueError("token_fsm: from_index takes a non-empty dict {state: {token: next_state}}")
        edges, top = [], _int(start, "start")
        for s, row in index.items():
            if not isinstance(row, dict):
                raise ValueError(f"token_fsm: from_index: the entry of state {s!r} must be a dict {{token: next_state}}")
            top = max(top, _int(s, "a state"))
            for t, n in row.items():
                edges.append((s, t, n))
                top = max(top, _int(n, "an edge's next state"))
        return cls(top + 1, edges, start=start, **kw)

    @classmethod
    def from_choices(cls, choices, eos_ids, **kw):
        """"answer with one of these token sequences": a trie over `choices` from state 0.  After a complete choice only the EOS ids are
        allowed (next to the continuation, where one choice is a prefix of another), and they lead to an absorbing state that allows only
        EOS: a multi-step replay that runs past EOS never meets a dead end."""
        eos = sorted({_int(t, "an EOS id") for t in (eos_ids if eos_ids is not None else ())})
        if not eos:
            raise ValueError("token_fsm: from_choices needs at least one EOS id")
        choices = [[_int(t, "a choice's token") for t in c] for c in choices]
        if not choices or any(not c for c in choices):
            raise ValueError("token_fsm: from_choices needs at least one choice, and every choice at least one token")
        nodes, final = [{}], set()
        for c in choices:
            s = 0
            for t in c:
                if t in eos:
                    raise ValueError(f"token_fsm: from_choices: a choice holds the EOS id {t}")
                if t not in nodes[s]:
                    nodes.append({})
                    nodes[s][t] = len(nodes) - 1
                s = nodes[s][t]
            final.add(s)
        end = len(nodes)  # the absorbing state
        edges = [(s, t, n) for s, row in enumerate(nodes) for t, n in row.items()]
        edges += [(s, t, end) for s in sorted(final) + [end] for t in eos]
        return cls(end + 1, edges, start=0, **kw)

    # ---- the part of the validation that needs the vocabulary ----
    def check(self, vocab_size, max_mask_bytes=MAX_MASK_BYTES):
        """ValueError when an edge's token is outside [0, vocab_size), when a reachable state forbids every token of the vocabulary, or when
        the mask rows take more than max_mask_bytes; returns the bytes of the masks.  Binds the machine to the vocabulary."""
        V = _int(vocab_size, "vocab_size")
        if V < 1:
            raise ValueError(f"token_fsm: vocab_size must be >= 1, not {V}")
        bad = np.nonzero(self.edge_tok >= V)[0]
        if bad.size:
            s = int(np.searchsorted(self.row_ptr, bad[0], side="right")) - 1
            raise ValueError(f"token_fsm: state {s}: token id {int(self.edge_tok[bad[0]])} is outside [0, {V})")
        for s in self._reachable:
            if self.default_next[s] >= 0 and int((self._row(s)[1] < 0).sum()) >= V:
                raise ValueError(f"token_fsm: state {s} is reachable from state {self.start} and allows no token (a dead end)")
        need = self.n_states * ((V + 31) // 32) * 4
        if need > max_mask_bytes:
            raise ValueError(f"token_fsm: the masks of {self.n_states} states over {V} tokens take {need} bytes, more than max_mask_bytes = {max_mask_bytes}")
        self.vocab_size = V
        return need

    # ---- the machine on the host ----
    def _row(self, s):
        a, b = int(self.row_ptr[s]), int(self.row_ptr[s + 1])
        return self.edge_tok[a:b], self.edge_next[a:b]

    def _reach(self):
        seen, todo = {self.start}, [self.start]
        while todo:
            s = todo.pop()
            nxt = set(int(n) for n in self._row(s)[1] if n >= 0)
            if self.default_next[s] >= 0:
                nxt.add(int(self.default_next[s]))
            for n in nxt - seen:
                seen.add(n)
                todo.append(n)
        return sorted(seen)

    def _state(self, state):
        s = self.start if state is None else _int(state, "state")
        if not 0 <= s < self.n_states:
            raise ValueError(f"token_fsm: state {s} is outside [0, {self.n_states})")
        return s

    def allowed(self, state, vocab_size=None):
        """the token ids state `state` allows, ascending (int64).  A state with a default needs the vocabulary: vocab_size, or check()'s."""
        s = self._state(state)
        tok, nxt = self._row(s)
        if self.default_next[s] < 0:
            return tok[nxt >= 0].astype(np.int64)
        V = vocab_size if vocab_size is not None else self.vocab_size
        if V is None:
            raise ValueError(f"token_fsm: state {s} allows every token without an edge: allowed() needs vocab_size")
        keep = np.ones(int(V), dtype=bool)
        keep[tok[(nxt < 0) & (tok < V)]] = False
        return np.nonzero(keep)[0].astype(np.int64)

    def step(self, state, token):
        """the state behind `token` in `state`; -1: the token is forbidden there"""
        s = self._state(state)
        tok, nxt = self._row(s)
        i = int(np.searchsorted(tok, token))
        if i < tok.size and tok[i] == token:
            return int(nxt[i])
        return int(self.default_next[s])

    def walk(self, ids, state=None):
        """the state behind the tokens `ids` from `state` (None: start); ValueError at the first token the machine forbids"""
        s = self._state(state)
        for i, t in enumerate(ids):
            n = self.step(s, int(t))
            if n < 0:
                raise ValueError(f"token_fsm: token {int(t)} (number {i} of the walk) is forbidden in state {s}")
            s = n
        return s

    def key(self):
        """a digest of the machine's content: two machines with equal tables and start are one machine (the decoder keys its sampler on it)"""
        h = hashlib.sha256()
        h.update(np.array([self.n_states, self.start], dtype=np.int64).tobytes())
        for a in (self.row_ptr, self.edge_tok, self.edge_next, self.default_next):
            h.update(a.tobytes())
        return h.hexdigest()

    def __repr__(self):
        return f"TokenFSM(n_states={self.n_states}, edges={self.edge_tok.size}, start={self.start})"
