"""The lockstep differential run behind tests/test_sampler_adj_gpu.py and tests/test_sampler_full_adj_gpu.py (a plain helper module).

Run A draws through the new entry (gq_sample_topk_adj / gq_sample_full_adj) on the RAW logits; run B, draw for draw from the same state,
through the existing entry (gq_sample_topk_lp / gq_sample_full) on `sampler_adj_model.adjusted_logits(raw, bias, counts so far)`.  After
every draw everything the draw writes is compared byte for byte, the two count arrays of A against the host's tally, and the guards of
A's buffers are checked.  All buffers are tests/guarded.py's; outputs, workspaces and the four new arrays start poisoned: bias_set / bias
are then built by gq_token_bias_build, out_set is laid out by the host and out_count holds the pre-counted tokens' counts and poison
everywhere else (a count means something for the tokens of out_set only).
"""
import ctypes

import numpy as np
import torch

import guarded
import sampler_adj_model as am
import sampler_model as sm
from sampler_rep_model import EMPTY_TOKEN, token_set

BLOCKS = sm.BLOCKS
POISON32 = np.uint32(0x7E7E7E7E)
EXTRA = 8  # slots of the log-probability arrays behind lp_cap


def _i32(v):
    return np.array(v, dtype=np.int32).reshape(-1)


def lp_cap(c):
    return c.pos0 + c.n + 2 - (c.lp_cut + 1 if c.lp_cut else 0)


class Run:
    """the buffers of one run of case `c` from its initial state; adjust=True: the run of the new entry (A), with the four new arrays"""

    def __init__(self, c, full, adjust, top_n=0):
        from guidedquant_amd import _lib
        self.L, self.c, self.full, self.adjust, self.top_n = _lib.lib(), c, full, adjust, top_n
        self.stream = _lib.current_stream_ptr()
        x, bias, pre, seen0, suppress, ban = am.case_inputs(c)
        self.raw, self.bias, self.pre = x, bias, pre
        L, s = self.L, self.stream
        gi, go = self.gi, self.go = guarded.Guards(), guarded.Guards()
        self.logits = gi.inp("logits", x.view(np.int16))
        self.ban = gi.inp("ban", _i32([ban[0], ban[1], *ban[2]]) if ban is not None else None)
        self.table = gi.inp("table", sm.embed_table(c).view(np.int16) if c.dim else None)
        if full:
            self.ws_bytes = L.gq_sample_full_ws_bytes(c.V)
            self.ws = go.out("ws", self.ws_bytes)
        else:
            self.wv, self.wi, self.lws = go.out("work_val", 4 * BLOCKS * 64), go.out("work_idx", 4 * BLOCKS * 64), go.out("lp_ws", 4 * 2 * BLOCKS)
        self.ctr, self.pos, self.tok = go.inp("counter", _i32([0])), go.inp("pos", _i32([c.pos0])), go.inp("tok", _i32([-5]))
        self.seq_cap = c.pos0 + c.n + 2
        self.nt, self.seq = go.out("next_tok", 4 * (c.n + 1)), go.out("seq", 4 * self.seq_cap)
        self.xo = go.out("x_out", 2 * c.n * c.dim) if c.dim else None
        self.ssq = go.out("ssq_out", 4 * c.n * 1024) if c.dim else None
        nw = (c.V + 31) // 32
        self.seen = self.sup = None
        if c.rp != 1.0 or seen0:
            self.seen = go.out("seen", 4 * nw)
            ids = torch.tensor(list(seen0), dtype=torch.int32, device="cuda:0") if seen0 else None
            _lib.check(L.gq_token_set_build(ids.data_ptr() if ids is not None else None, len(seen0), c.V, self.seen.ptr(), 1, s), "gq_token_set_build")
        if suppress:
            self.sup = gi.out("suppress", 4 * nw)
            ids = torch.tensor(list(suppress), dtype=torch.int32, device="cuda:0")
            _lib.check(L.gq_token_set_build(ids.data_ptr(), len(suppress), c.V, self.sup.ptr(), 1, s), "gq_token_set_build")
        self.lp_len = c.pos0 + c.n + 2 + EXTRA
        self.lraw, self.ldrawn = go.out("lp_raw", 4 * self.lp_len), go.out("lp_drawn", 4 * self.lp_len)
        self.top_ids = self.top_lps = self.topn_ws = None
        if top_n:
            self.top_ids, self.top_lps = go.out("top_ids", 4 * self.lp_len * top_n), go.out("top_lps", 4 * self.lp_len * top_n)
            self.topn_ws = go.out("topn_ws", _lib.TOPN_WS_BYTES)
        self.bias_set = self.biasv = self.out_set = self.out_count = self.adj = None
        if adjust:
            fp = pp = 0.0
            if bias:
                self.bias_set, self.biasv = gi.out("bias_set", 4 * nw), gi.out("bias", 4 * c.V)
                ids = torch.tensor(list(bias), dtype=torch.int32, device="cuda:0")
                vals = torch.tensor(list(bias.values()), dtype=torch.float32, device="cuda:0")
                _lib.check(L.gq_token_bias_build(ids.data_ptr(), vals.data_ptr(), len(bias), c.V, self.bias_set.ptr(), self.biasv.ptr(), s), "gq_token_bias_build")
            if c.fp != 0.0 or c.pp != 0.0 or pre.any():
                fp, pp = c.fp, c.pp
                self.out_set = go.inp("out_set", token_set(np.nonzero(pre)[0], c.V))
                self.out_count = go.inp("out_count", np.where(pre > 0, pre, int(POISON32)).astype(np.uint32))
            self.adj = _lib.GqSampleAdjust(fp, pp, guarded.ptr(self.bias_set), guarded.ptr(self.biasv), guarded.ptr(self.out_set), guarded.ptr(self.out_count))
        torch.cuda.synchronize()

    def set_logits(self, x16):
        self.logits.view(torch.int16).copy_(torch.from_numpy(np.ascontiguousarray(x16).view(np.int16)))

    def draw(self, i, expect=0, **over):
        """draw number i through the run's entry; over: arguments in place of the case's (adj, top_n, V, ...)"""
        c, p = self.c, guarded.ptr
        cap = over.get("cap", lp_cap(c))
        head = (self.logits.ptr(), over.get("V", c.V), over.get("top_k", c.top_k), c.top_p)
        tail = (self.tok.ptr(), self.pos.ptr(), self.nt.ptr() + 4 * i, p(self.ban), self.seq.ptr(), self.seq_cap, p(self.table),
                self.xo.ptr() + 2 * c.dim * i if c.dim else None, c.dim, self.ssq.ptr() + 4096 * i if c.dim else None, c.rp, p(self.seen), p(self.sup))
        lps = (over.get("lraw", self.lraw.ptr()), self.ldrawn.ptr(), cap)
        topn = (over.get("top_n", self.top_n), p(self.top_ids), p(self.top_lps), p(self.topn_ws))
        adj = over.get("adj", self.adj)
        adj = ctypes.byref(adj) if adj is not None else None
        if self.full:
            a = head + (c.min_p, c.T, c.seed, self.ctr.ptr(), self.ws.ptr(), self.ws_bytes) + tail + lps
            name = over.get("entry", "gq_sample_full_adj" if self.adjust else "gq_sample_full")
        else:
            a = head + (c.T, c.seed, self.ctr.ptr(), self.wv.ptr(), self.wi.ptr()) + tail + (over.get("lws", self.lws.ptr()), ) + lps
            name = over.get("entry", "gq_sample_topk_adj" if self.adjust else "gq_sample_topk_lp")
        if name.endswith("_adj"):
            a += topn + (adj, )
        elif name.endswith("_topn"):
            a += topn
        rc = getattr(self.L, name)(*a, self.stream)
        assert rc == expect, (c.name, name, i, rc, self.L.gq_last_error())

    def state(self):
        """everything a draw writes, as numpy arrays"""
        out = dict(nt=self.nt.numpy(np.int32), seq=self.seq.numpy(np.int32), ctr=self.ctr.numpy(np.int32), pos=self.pos.numpy(np.int32), tok=self.tok.numpy(np.int32),
                   raw=self.lraw.numpy(np.uint32), drawn=self.ldrawn.numpy(np.uint32))
        for k, b in (("seen", self.seen), ("x", self.xo), ("ssq", self.ssq), ("top_ids", self.top_ids), ("top_lps", self.top_lps), ("out_set", self.out_set),
                     ("out_count", self.out_count), ("bias_set", self.bias_set), ("bias", self.biasv)):
            if b is not None:
                out[k] = b.numpy(np.uint32 if k != "x" else np.uint16)
        return out


DRAW_STATE = ("seq", "seen", "xo", "ssq", "ldrawn")  # compared on the device after every draw (next_tok, tok_io, pos_io, counter: on the host)


def lockstep(c, full):
    """A and B in lockstep with every per-draw check; returns (A's final state, the tokens, the reference call's (M, L) and top-n row)"""
    A, B = Run(c, full, True, c.top_n), Run(c, full, False)
    counts = A.pre.copy()
    tokens = []
    for i in range(c.n):
        A.draw(i)
        A.go.check()  # (synchronises)
        B.set_logits(am.adjusted_logits(A.raw, A.bias, counts, c.fp, c.pp))
        B.draw(i)
        torch.cuda.synchronize()
        ta, tb = int(A.nt.view(torch.int32)[i]), int(B.nt.view(torch.int32)[i])
        assert ta == tb, (c.name, "draw", i, ta, tb)
        for k in ("tok", "pos", "ctr"):
            va, vb = int(getattr(A, k).view(torch.int32)[0]), int(getattr(B, k).view(torch.int32)[0])
            assert va == vb, (c.name, "draw", i, k, va, vb)
        assert int(A.tok.view(torch.int32)[0]) == ta and int(A.pos.view(torch.int32)[0]) == c.pos0 + i + 1 and int(A.ctr.view(torch.int32)[0]) == i + 1
        for k in DRAW_STATE:
            a, b = getattr(A, k), getattr(B, k)
            if a is not None:
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (c.name, "draw", i, k)
        if full:  # the workspace report {n, n_k, Z_k, Z_kept}
            ra, rb = A.ws.view(torch.uint8)[:24], B.ws.view(torch.uint8)[:24]
            assert torch.equal(ra, rb), (c.name, "draw", i, "report", ra.cpu().numpy().view(np.uint32), rb.cpu().numpy().view(np.uint32))
        tokens.append(ta)
        if 0 <= ta < c.V:
            counts[ta] += 1
        else:
            assert ta == EMPTY_TOKEN
        if A.out_set is not None:  # the host's tally, and nothing else changed: a non-member's count keeps the poison
            want_set = torch.from_numpy(token_set(np.nonzero(counts)[0], c.V).view(np.int32)).cuda()
            want_count = torch.from_numpy(np.where(counts > 0, counts, int(POISON32)).astype(np.uint32).view(np.int32)).cuda()
            assert torch.equal(A.out_set.view(torch.int32), want_set), (c.name, "draw", i, "out_set")
            assert torch.equal(A.out_count.view(torch.int32), want_count), (c.name, "draw", i, "out_count")
    A.go.check()
    A.gi.check()
    B.go.check()
    B.gi.check()
    # the raw log-sum-exp and the raw order: ONE call of the existing top-n entry on the raw logits
    R = Run(c, full, False, max(c.top_n, 1))
    R.draw(0, entry="gq_sample_full_topn" if full else "gq_sample_topk_lp_topn")
    R.go.check()
    M, Lz = R.topn_ws.numpy(np.float32)[:2]
    n = max(c.top_n, 1)
    row = (R.top_ids.numpy(np.int32).reshape(-1, n)[c.pos0 + 1], R.top_lps.numpy(np.uint32).reshape(-1, n)[c.pos0 + 1])
    return A.state(), tokens, (np.float32(M), np.float32(Lz)), row


def check_case(c, full):
    """the whole differential of one case; returns the tokens"""
    state, tokens, (M, Lz), (row_ids, row_lps) = lockstep(c, full)
    cap = lp_cap(c)
    written = np.zeros(state["raw"].size, dtype=bool)
    written[c.pos0 + 1:min(c.pos0 + c.n + 1, cap)] = True
    # lp_raw: fl32(fl32(v_raw[tok] - M) - L) on the RAW logits, bit for bit; NaN for an empty candidate set; poison outside the run
    v = A_raw = am.case_inputs(c)[0].astype(np.float32)
    for arr in ("raw", "drawn"):
        assert (state[arr][~written] == POISON32).all(), (c.name, arr, "a slot outside the run or past lp_cap was written")
        assert (state[arr][written] != POISON32).all(), (c.name, arr, "a slot of the run was not written")
    for i, t in enumerate(tokens):
        slot = c.pos0 + 1 + i
        if slot >= cap:
            continue
        got = state["raw"][slot:slot + 1].view(np.float32)[0]
        if t == EMPTY_TOKEN:
            assert np.isnan(got) and np.isnan(state["drawn"][slot:slot + 1].view(np.float32)[0]), (c.name, i)
            continue
        with np.errstate(all="ignore"):
            want = np.float32(np.float32(v[t] - M) - Lz)
        assert got.view(np.uint32) == want.view(np.uint32), (c.name, "lp_raw", i, t, float(got), float(want), float(A_raw[t]), float(M), float(Lz))
    # the top-n rows: the raw order's, the same at every step
    if c.top_n:
        ids, lps = state["top_ids"].view(np.int32).reshape(-1, c.top_n), state["top_lps"].reshape(-1, c.top_n)
        assert (ids[written] == row_ids[None, :]).all() and (lps[written] == row_lps[None, :]).all(), (c.name, "top-n rows")
        assert (ids[~written].view(np.uint32) == POISON32).all() and (lps[~written] == POISON32).all(), (c.name, "a top-n row outside the run was written")
    # determinism: a second run of A, no host in between
    A2 = Run(c, full, True, c.top_n)
    for i in range(c.n):
        A2.draw(i)
    A2.go.check()
    again = A2.state()
    assert sorted(again) == sorted(state)
    for k in state:
        assert np.array_equal(state[k], again[k]), (c.name, k, "two runs from the same state differ")
    return tokens
